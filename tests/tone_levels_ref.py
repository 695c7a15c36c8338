"""numpy reference of x3_tone_levels_dev / x3_corpus_tone_levels_dev and x3_tone_power_levels_dev (include/x3hip.h, "TONE
LEVELS"; not a test module).  This file is the definition: integers only.

Positions and bins are levels_ref's.  With a step and a table of 1 024 (cos, sin) int16 pairs, position i of a stream or
entry has the phase ph(i) = (i * step) mod 2^32 and the pair k(i) = ph(i) >> 22; a bin's record holds
    re = sum of x[i] * cos[k(i)],  im = sum of x[i] * sin[k(i)]
over its positions in frames with status 0, and the min, max and n of those samples.  Entries of a corpus are separate
calls here, so the phase restarts at every entry."""
import numpy as np

import levels_ref as R

TONE_DTYPE = np.dtype([("re", np.int64), ("im", np.int64), ("min", np.int32), ("max", np.int32), ("n", np.uint32),
                       ("reserved", np.uint32)])
LEVEL_DTYPE = R.LEVEL_DTYPE
PAIRS = 1024


def table():
    """the usual table, int16 [1024, 2]: round(32767 cos(2 pi k / 1024)), round(32767 sin(2 pi k / 1024))"""
    a = 2.0 * np.pi * np.arange(PAIRS) / PAIRS
    return np.stack([np.rint(32767.0 * np.cos(a)), np.rint(32767.0 * np.sin(a))], axis=1).astype(np.int16)


def empty(n_bins):
    out = np.zeros(n_bins, dtype=TONE_DTYPE)
    out["min"], out["max"] = 32767, -32768
    return out


def pair_index(pos, step):
    """k(i) of positions pos (int64 array, below 2^63) for a step of 32 bits"""
    assert 0 <= step <= 0xFFFFFFFF
    return ((pos.astype(np.uint64) * np.uint64(step)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)   # (the product wraps mod 2^64)


def tone_levels(frames, statuses, sample_offsets, bin_len, n_bins, step, tab=None):
    """levels_ref.levels' arguments, the step and the table (None: the usual one) -> TONE_DTYPE[n_bins]"""
    tab = table() if tab is None else np.asarray(tab, dtype=np.int16).reshape(PAIRS, 2)
    out = empty(n_bins)
    pos, val = [], []
    for w, st, so in zip(frames, statuses, sample_offsets):
        if st == 0 and len(w):
            pos.append(int(so) + np.arange(len(w), dtype=np.int64))
            val.append(np.asarray(w, dtype=np.int64))
    if not pos:
        return out
    pos, val = np.concatenate(pos), np.concatenate(val)
    k = pair_index(pos, step).astype(np.int64)
    bins = pos // bin_len if bin_len else np.zeros_like(pos)
    keep = bins < n_bins
    bins, val, k = bins[keep], val[keep], k[keep]
    np.add.at(out["n"], bins, 1)
    np.add.at(out["re"], bins, val * tab[k, 0].astype(np.int64))
    np.add.at(out["im"], bins, val * tab[k, 1].astype(np.int64))
    np.minimum.at(out["min"], bins, val.astype(np.int32))
    np.maximum.at(out["max"], bins, val.astype(np.int32))
    return out


def corpus_tone_levels(entries, bin_len, step, tab=None):
    """levels_ref.corpus_levels' entries (frames, statuses, sample offsets relative to the entry, n_samples) -> (TONE_DTYPE
    [rows], row_first)"""
    rf = R.corpus_row_first([e[3] for e in entries], bin_len)
    out = empty(int(rf[-1]))
    for e, (frames, statuses, so, _) in enumerate(entries):
        a, b = int(rf[e]), int(rf[e + 1])
        out[a:b] = tone_levels(frames, statuses, so, bin_len, b - a, step, tab)
    return out, rf


def isqrt(x):
    """floor square root of a Python int >= 0"""
    x = int(x)
    r = int(np.sqrt(float(x)))
    while r * r > x:
        r -= 1
    while (r + 1) * (r + 1) <= x:
        r += 1
    return r


def power_record(re, im, n):
    """one record of x3_tone_power_levels_dev in Python integers -> (sum_sq, sum, min, max, n), and P for the caller's checks"""
    re, im, n = int(re), int(im), int(n)
    if n == 0:
        return (0, 0, 32767, -32768, 0), 0
    e = max(0, n.bit_length() - 15)
    a, b = re >> (15 + e), im >> (15 + e)   # (Python's >> on negative integers is the arithmetic shift)
    P = a * a + b * b
    m = n >> e
    ms = min(1 << 30, (2 * P // m) // m)
    peak = min(32767, isqrt(2 * ms))
    return (ms * n, 0, -peak, peak, n), P


def tone_power_levels(tone):
    """TONE_DTYPE[n] -> LEVEL_DTYPE[n], record by record"""
    out = np.zeros(len(tone), dtype=LEVEL_DTYPE)
    for i, r in enumerate(tone):
        (out["sum_sq"][i], out["sum"][i], out["min"][i], out["max"][i], out["n"][i]), _ = power_record(r["re"], r["im"], r["n"])
    return out
