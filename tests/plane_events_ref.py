"""Serial reference of x3_plane_events_dev / x3_corpus_plane_events_dev (include/x3hip.h, "PLANE EVENTS"; not a test module).

One rule: plane events are the events of events_ref on ONE synthetic row verdict.

  loud    plane t at row b: events_ref.is_hot(record (t, b), the plane's own two values)
  hot     row b: at least min_planes planes are loud at b
  events  events_ref.entry_events on a synthetic record array that is hot under peak_min = 1 exactly at the hot rows
          (join_bins, min_bins, pad_bins, max_bins as given); every synthetic record counts one sample, so a piece's
          merged synthetic record tells its rows
  mask    bit t: plane t is loud in at least one row of the piece, padding rows included
  levels  events_ref.merge of plane t's records over the piece's rows, per plane

K planes of level records in, the FULL ordered list of events ([entry,] start, len, mask) and their merged records
[K, events] out; a caller applies its own cap (slots)."""
from collections import namedtuple

import numpy as np

import events_ref as E
import quantiles_ref as Q
import tone_bank_levels_ref as B
from levels_ref import empty, n_bins_for

PLANES_MAX = 8

# mean_sq_min, peak_min: a value per plane
PlaneRule = namedtuple("PlaneRule", "mean_sq_min peak_min min_planes join_bins min_bins pad_bins max_bins",
                       defaults=(1, 0, 0, 0, 0))


def plane_rules(rule, n_planes, thr=None):
    """the events rule of every plane: the rule's own values, or those of thr[t] = (mean_sq_min, peak_min[, counted]) of
    the entry at hand, one above its limit being off"""
    if thr is None:
        return [E.Rule(mean_sq_min=int(rule.mean_sq_min[t]), peak_min=int(rule.peak_min[t])) for t in range(n_planes)]
    return [Q.adaptive_rule(E.Rule(), thr[t]) for t in range(n_planes)]


def entry_plane_events(planes, n_samples, bin_len, rule, thr=None):
    """the events of ONE entry; planes: K sequences of the entry's rows -> [(start, len, mask, [merged record per plane])]"""
    k, rows = len(planes), len(planes[0])
    assert 1 <= rule.min_planes <= k <= PLANES_MAX
    per = plane_rules(rule, k, thr)
    loud = [[E.is_hot(planes[t][b], per[t]) for b in range(rows)] for t in range(k)]
    syn = empty(rows)
    syn["n"], syn["min"] = 1, 0
    syn["max"] = [1 if sum(loud[t][b] for t in range(k)) >= rule.min_planes else 0 for b in range(rows)]
    ev = E.entry_events(syn, n_samples, bin_len,
                        E.Rule(0, 1, rule.join_bins, rule.min_bins, rule.pad_bins, rule.max_bins))
    out = []
    for start, ln, m in ev:
        p0 = start // bin_len
        p1 = p0 + int(m["n"])
        mask = sum(1 << t for t in range(k) if any(loud[t][p0:p1]))
        out.append((start, ln, mask, [E.merge(planes[t][p0:p1]) for t in range(k)]))
    return out


def _pack(ev, k):
    lv = np.stack([empty(len(ev)) for _ in range(k)])
    for i, e in enumerate(ev):
        for t in range(k):
            lv[t, i] = e[-1][t]
    return [e[:-1] for e in ev], lv


def stream_plane_events(planes, total, bin_len, rule, thr=None):
    """x3_plane_events_dev; planes: LEVEL_DTYPE [K, n_bins], thr: None or K records (plane-major, one entry) ->
    ([(start, len, mask)], LEVEL_DTYPE [K, events])"""
    rows = min(planes.shape[1], -(-int(total) // bin_len))
    return _pack(entry_plane_events([p[:rows] for p in planes], int(total), bin_len, rule, thr), len(planes))


def corpus_plane_events(planes, n_samples, bin_len, rule, thr=None):
    """x3_corpus_plane_events_dev; planes: LEVEL_DTYPE [K, n_rows], thr: None or records [K][n_entries] ->
    ([(entry, start, len, mask)], LEVEL_DTYPE [K, events])"""
    ev, at = [], 0
    for e, ns in enumerate(n_samples):
        rows = min(n_bins_for(int(ns), bin_len), planes.shape[1] - at)
        te = None if thr is None else [thr[t][e] for t in range(len(planes))]
        ev += [(e,) + x for x in entry_plane_events([p[at:at + rows] for p in planes], int(ns), bin_len, rule, te)]
        at += rows
    return _pack(ev, len(planes))


def slots(events, levels, cap, with_entries):
    """what the device arrays of `cap` slots hold: the first events, then the filler ->
    (entries or None, starts, lens, masks uint32 [cap], levels [K, cap])"""
    n = min(len(events), cap)
    ent, st, ln = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
    mk = np.zeros(cap, dtype=np.uint32)
    lv = np.stack([empty(cap) for _ in range(levels.shape[0])])
    for i in range(n):
        if with_entries:
            ent[i] = events[i][0]
        st[i], ln[i], mk[i] = events[i][-3], events[i][-2], events[i][-1]
    lv[:, :n] = levels[:, :n]
    return (ent if with_entries else None), st, ln, mk, lv


# DESIGN.md section 28's signal: section 26's, and five more bursts of amplitude 1 000 and 200 samples -- a step from band 0
# to band 1 at 8 000, three bands at once at 16 000
EXAMPLE_BURSTS = ((8_000, 200, 0.0817, 0.7), (8_200, 200, 0.2310, 0.2), (16_000, 200, 0.0817, 0.5),
                  (16_000, 200, 0.2310, 1.9), (16_000, 200, 0.15, 2.6))


def example():
    w = B.example().astype(np.int64)
    for a, n, f, ph in EXAMPLE_BURSTS:
        t = np.arange(a, a + n)
        w[a:a + n] += np.rint(1_000 * np.sin(2 * np.pi * f * t + ph)).astype(np.int64)
    return np.clip(w, -32768, 32767).astype(np.int16)
