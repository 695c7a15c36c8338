"""Serial reference of x3_events_dev / x3_corpus_events_dev (include/x3hip.h, "EVENTS"; not a test module).

Level records in, the FULL ordered list of events (entry, start, len) and their merged records out; a caller applies its
own cap.  One loop over the rows of each entry, plain Python integers:

  hot     n != 0 and (mean_sq_min != 0 and sum_sq >= mean_sq_min * n  or  peak_min != 0 and max(max, -min) >= peak_min)
  run     hot rows of one entry with at most join_bins cold rows between neighbours; spans first hot .. last hot
  kept    last - first + 1 >= min_bins
  padded  [max(first - pad_bins, 0), min(last + 1 + pad_bins, rows of the entry))
  pieces  of max_bins rows (0: 0xFFFFFFFF // bin_len), the last one shorter
  event   start = p0 * bin_len, len = min(p1 * bin_len, n_samples) - start
  record  from the identities: sum_sq (mod 2^64), sum (mod 2^64, signed), n (mod 2^32) added, min and max taken"""
from collections import namedtuple

import numpy as np

from levels_ref import LEVEL_DTYPE, empty, n_bins_for

Rule = namedtuple("Rule", "mean_sq_min peak_min join_bins min_bins pad_bins max_bins", defaults=(0, 0, 0, 0, 0, 0))


def is_hot(rec, rule):
    n = int(rec["n"])
    if n == 0:
        return False
    if rule.mean_sq_min and int(rec["sum_sq"]) >= rule.mean_sq_min * n:
        return True
    return bool(rule.peak_min) and max(int(rec["max"]), -int(rec["min"])) >= rule.peak_min


def merge(recs):
    out = empty(1)[0]
    sq, sm, n, mn, mx = 0, 0, 0, 32767, -32768
    for r in recs:
        sq, sm, n = sq + int(r["sum_sq"]), sm + int(r["sum"]), n + int(r["n"])
        mn, mx = min(mn, int(r["min"])), max(mx, int(r["max"]))
    sm &= (1 << 64) - 1
    out["sum_sq"], out["sum"], out["n"] = sq & ((1 << 64) - 1), sm - (1 << 64) if sm >> 63 else sm, n & 0xFFFFFFFF
    out["min"], out["max"] = mn, mx
    return out


def entry_events(recs, n_samples, bin_len, rule):
    """the events of ONE entry whose rows are `recs` -> [(start, len, merged record)]"""
    rows = len(recs)
    runs, cur = [], None
    for b in range(rows):
        if not is_hot(recs[b], rule):
            continue
        if cur is not None and b - cur[1] - 1 <= rule.join_bins:
            cur[1] = b
        else:
            cur = [b, b]
            runs.append(cur)
    mb = rule.max_bins or 0xFFFFFFFF // bin_len
    out = []
    for first, last in runs:
        if last - first + 1 < rule.min_bins:
            continue
        b0, b1 = max(first - rule.pad_bins, 0), min(last + 1 + rule.pad_bins, rows)
        for p0 in range(b0, b1, mb):
            p1 = min(p0 + mb, b1)
            start = p0 * bin_len
            out.append((start, min(p1 * bin_len, n_samples) - start, merge(recs[p0:p1])))
    return out


def _pack(ev):
    lv = empty(len(ev))
    for i, e in enumerate(ev):
        lv[i] = e[-1]
    return [e[:-1] for e in ev], lv


def stream_events(levels, total, bin_len, rule):
    """x3_events_dev: rows min(len(levels), ceil(total / bin_len)) count -> ([(start, len)], LEVEL_DTYPE[events])"""
    rows = min(len(levels), -(-int(total) // bin_len))
    return _pack(entry_events(levels[:rows], int(total), bin_len, rule))


def corpus_events(levels, n_samples, bin_len, rule):
    """x3_corpus_events_dev: entry e has max(1, ceil(n_samples[e] / bin_len)) rows, one entry behind the other, clipped to
    len(levels) -> ([(entry, start, len)], LEVEL_DTYPE[events])"""
    ev, at = [], 0
    for e, ns in enumerate(n_samples):
        rows = min(n_bins_for(int(ns), bin_len), len(levels) - at)
        ev += [(e,) + x for x in entry_events(levels[at:at + rows], int(ns), bin_len, rule)]
        at += rows
    return _pack(ev)


def slots(events, levels, cap, with_entries):
    """what the device arrays of `cap` slots hold: the first events, then the filler -> (entries or None, starts, lens, levels)"""
    n = min(len(events), cap)
    ent, st, ln = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    lv = empty(cap)
    for i in range(n):
        if with_entries:
            ent[i] = events[i][0]
        st[i], ln[i] = events[i][-2], events[i][-1]
    lv[:n] = levels[:n]
    return (ent if with_entries else None), st, ln, lv
