"""Serial reference of the level quantiles, the thresholds from them and the adaptive events (include/x3hip.h, "LEVEL
QUANTILES AND ADAPTIVE THRESHOLDS"; not a test module).  Plain Python integers throughout.

  counts  a row counts for its entry when it lies in one and its n != 0; K = the entry's counting rows
  key     PEAK: max(max, -min) clamped to 0 .. 32768;  MEAN_SQ: min(sum_sq // n, 2^30)
  value   sorted(keys)[(K - 1) * q_ppm // 1_000_000], 0 when K == 0
  thr     min(max(value * mul // div + add, 1), limit) for a criterion with div != 0 and K != 0, else 0
  hot     events_ref.is_hot with the entry's two thresholds; one above its limit is off

Which rows an entry has is the events calls' rule.  rows_by_table() states it for ANY entry table, also one overwritten with
wild sample counts: the row prefix is the sum of the entries' rows modulo 2^64, a row's owner is the last entry of a
bisection on that prefix, and the row is the owner's when it lies inside the owner's rows."""
from collections import namedtuple

import numpy as np

import events_ref as E
from levels_ref import n_bins_for

PEAK, MEAN_SQ = 0, 1
PEAK_MAX, MEAN_SQ_MAX = 32768, 1 << 30
M64 = (1 << 64) - 1

# a criterion: (q_ppm, mul, div, add) or None when it is off
TRule = namedtuple("TRule", "peak mean_sq", defaults=(None, None))


def key_of(rec, key):
    """the key of a record whose n != 0"""
    if key == PEAK:
        return min(max(int(rec["max"]), -int(rec["min"]), 0), PEAK_MAX)
    return min(int(rec["sum_sq"]) // int(rec["n"]), MEAN_SQ_MAX)


def quantiles_of(keys, q_ppm):
    """keys: the counting keys of one entry, any order -> [value per q]"""
    srt = sorted(keys)
    return [srt[(len(srt) - 1) * q // 1_000_000] if srt else 0 for q in q_ppm]


def rows_by_table(n_samples, bin_len, n_rows):
    """-> per entry the list of its rows, for any table of sample counts (see the module text)"""
    n = len(n_samples)
    rows = [n_bins_for(int(ns), bin_len) for ns in n_samples]
    first = [0] * (n + 1)
    for e in range(n):
        first[e + 1] = (first[e] + rows[e]) & M64
    out = [[] for _ in range(n)]
    for r in range(n_rows):
        lo, hi = 0, n
        while hi - lo > 1:
            mid = lo + ((hi - lo) >> 1)
            if first[mid] <= r:
                lo = mid
            else:
                hi = mid
        if first[lo] <= r and r - first[lo] < rows[lo]:
            out[lo].append(r)
    return out


def _entries(levels, n_samples, bin_len):
    return [[levels[r] for r in rows] for rows in rows_by_table(n_samples, bin_len, len(levels))]


def _stream_rows(levels, total, bin_len):
    return levels[:min(len(levels), -(-int(total) // bin_len))]


def entry_quantiles(recs, key, q_ppm):
    keys = [key_of(r, key) for r in recs if int(r["n"]) != 0]
    return quantiles_of(keys, q_ppm), len(keys)


def _pack_q(per_entry, n_q):
    values = np.array([v for v, _ in per_entry], dtype=np.uint32).reshape(len(per_entry), n_q)
    return values, np.array([k for _, k in per_entry], dtype=np.uint32)


def stream_quantiles(levels, total, bin_len, key, q_ppm):
    """x3_level_quantiles_dev -> (values uint32 [1, n_q], counted uint32 [1])"""
    return _pack_q([entry_quantiles(_stream_rows(levels, total, bin_len), key, q_ppm)], len(q_ppm))


def corpus_quantiles(levels, n_samples, bin_len, key, q_ppm):
    """x3_corpus_level_quantiles_dev -> (values uint32 [n_entries, n_q], counted uint32 [n_entries])"""
    return _pack_q([entry_quantiles(recs, key, q_ppm) for recs in _entries(levels, n_samples, bin_len)], len(q_ppm))


def map_threshold(value, crit, limit):
    q, mul, div, add = crit
    return min(max(value * mul // div + add, 1), limit)


def entry_threshold(recs, trule):
    """-> (mean_sq_min, peak_min, counted) of one entry"""
    k = sum(1 for r in recs if int(r["n"]) != 0)
    peak = mean_sq = 0
    if k and trule.peak and trule.peak[2]:
        peak = map_threshold(entry_quantiles(recs, PEAK, [trule.peak[0]])[0][0], trule.peak, PEAK_MAX)
    if k and trule.mean_sq and trule.mean_sq[2]:
        mean_sq = map_threshold(entry_quantiles(recs, MEAN_SQ, [trule.mean_sq[0]])[0][0], trule.mean_sq, MEAN_SQ_MAX)
    return mean_sq, peak, k


def stream_thresholds(levels, total, bin_len, trule):
    return [entry_threshold(_stream_rows(levels, total, bin_len), trule)]


def corpus_thresholds(levels, n_samples, bin_len, trule):
    return [entry_threshold(recs, trule) for recs in _entries(levels, n_samples, bin_len)]


def adaptive_rule(rule, thr):
    """the events rule of an entry whose threshold record is thr = (mean_sq_min, peak_min[, counted]): a value above its
    limit is off"""
    m, p = int(thr[0]), int(thr[1])
    return rule._replace(mean_sq_min=m if m <= MEAN_SQ_MAX else 0, peak_min=p if p <= PEAK_MAX else 0)


def stream_adaptive_events(levels, total, bin_len, thr, rule):
    """x3_events_adaptive_dev -> ([(start, len)], LEVEL_DTYPE[events]); thr: one record"""
    return E.stream_events(levels, total, bin_len, adaptive_rule(rule, thr))


def corpus_adaptive_events(levels, n_samples, bin_len, thrs, rule):
    """x3_corpus_events_adaptive_dev -> ([(entry, start, len)], LEVEL_DTYPE[events]); thrs: a record per entry"""
    ev, at = [], 0
    for e, ns in enumerate(n_samples):
        rows = min(n_bins_for(int(ns), bin_len), len(levels) - at)
        ev += [(e,) + x for x in E.entry_events(levels[at:at + rows], int(ns), bin_len, adaptive_rule(rule, thrs[e]))]
        at += rows
    return E._pack(ev)
