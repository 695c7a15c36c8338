"""numpy reference of x3_fir_levels_dev / x3_corpus_fir_levels_dev (include/x3hip.h, "FIR LEVELS"; not a test module).

Positions and bins are levels_ref's.  With taps c[0 .. T-1] and a shift, position i of a stream or entry holds
    y[i] = clamp((sum over t < T of c[t] * x[i - t]) >> shift, -32768, 32767)      (>>: arithmetic, floor)
and counts if and only if all T positions i - T + 1 .. i exist (i >= T - 1) and every one lies in a frame with status 0
(THE HISTORY RULE).  Every other position adds nothing.  Entries of a corpus are separate calls here, so no history crosses
from one into the next."""
import numpy as np

import levels_ref as R

LEVEL_DTYPE = R.LEVEL_DTYPE


def check(taps, shift):
    """what the calls refuse: not 1 .. 8 taps of 16 bits, shift above 15, sum |c| above 32768"""
    taps = [int(c) for c in taps]
    return (1 <= len(taps) <= 8 and 0 <= shift <= 15 and all(-32768 <= c <= 32767 for c in taps)
            and sum(abs(c) for c in taps) <= 32768)


def signal(frames, statuses, sample_offsets, taps, shift):
    """-> (y int64 [total], counts bool [total]) over the positions 0 .. total - 1 the good frames reach"""
    assert check(taps, shift)
    T = len(taps)
    good = [(int(so), np.asarray(w, dtype=np.int64)) for w, st, so in zip(frames, statuses, sample_offsets) if st == 0 and len(w)]
    total = max([so + len(w) for so, w in good], default=0)
    x, have = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=bool)
    for so, w in good:
        x[so:so + len(w)] = w
        have[so:so + len(w)] = True
    acc, counts = np.zeros(total, dtype=np.int64), np.ones(total, dtype=bool)
    for t, c in enumerate(taps):
        xt, ht = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=bool)
        if t < total:                                            # x[i - t]; positions in front of the first do not exist
            xt[t:], ht[t:] = x[:total - t], have[:total - t]
        acc += int(c) * xt
        counts &= ht
    assert total == 0 or int(np.abs(acc).max()) <= 1 << 30
    return np.clip(acc >> shift, -32768, 32767), counts


def fir_levels(frames, statuses, sample_offsets, bin_len, n_bins, taps, shift=0):
    """levels_ref.levels' arguments, the taps and the shift -> LEVEL_DTYPE[n_bins]"""
    out = R.empty(n_bins)
    y, counts = signal(frames, statuses, sample_offsets, taps, shift)
    pos = np.nonzero(counts)[0].astype(np.int64)
    val = y[pos]
    bins = pos // bin_len if bin_len else np.zeros_like(pos)
    keep = bins < n_bins
    bins, val = bins[keep], val[keep]
    np.add.at(out["n"], bins, 1)
    np.add.at(out["sum"], bins, val)
    np.add.at(out["sum_sq"], bins, (val * val).astype(np.uint64))
    np.minimum.at(out["min"], bins, val.astype(np.int32))
    np.maximum.at(out["max"], bins, val.astype(np.int32))
    return out


def corpus_fir_levels(entries, bin_len, taps, shift=0):
    """levels_ref.corpus_levels' entries (frames, statuses, sample offsets relative to the entry, n_samples), the taps and
    the shift -> (LEVEL_DTYPE[rows], row_first)"""
    rf = R.corpus_row_first([e[3] for e in entries], bin_len)
    out = R.empty(int(rf[-1]))
    for e, (frames, statuses, so, _) in enumerate(entries):
        a, b = int(rf[e]), int(rf[e + 1])
        out[a:b] = fir_levels(frames, statuses, so, bin_len, b - a, taps, shift)
    return out, rf
