"""The definition of x3_tone_range_levels_dev / x3_corpus_tone_range_levels_dev (include/x3hip.h, "TONE RANGE LEVELS") in
numpy, from what the CPU oracle says about every frame (not a test module).  Integers only.

ONE RULE: the call cuts the stream's (or entry's) tone signal; it does not restart the oscillator at the range.  Position i
of the stream or entry that holds the range has the pair k(i) = tone_levels_ref.pair_index(i, step) -- i counted from the
stream's or entry's first position, whatever the range's start -- and bin b of range (start, len) holds
    re = sum of x[i] * cos[k(i)],  im = sum of x[i] * sin[k(i)]
over its positions i in [start + b * bin_len, start + (b + 1) * bin_len) cut to the range that lie in frames of status 0,
with the min, max and n of those samples: field for field range_levels_ref's.  Rows, layouts, row offsets, refusals and the
STATUSES are range_levels_ref.range_levels' own: the status of a range never depends on the tone.  (An entry of a corpus is
a stream of its own here, so the phase is 0 at every entry's first position.)"""
import numpy as np

import range_levels_ref as R
import tone_levels_ref as TL

TONE_DTYPE = TL.TONE_DTYPE
ERR_BAD_ARG = R.ERR_BAD_ARG
rows_of = R.rows_of


def one(frames, so, start, length, bin_len, step, tab):
    """the single range (start, length) -> (TONE_DTYPE [R], status); tab: int16 [1024, 2]"""
    plain, status = R.one(frames, so, start, length, bin_len)
    out = TL.empty(len(plain))
    if status == ERR_BAD_ARG and (start > int(so[-1]) or length > int(so[-1]) - start):
        return out, status
    for f in range(len(frames)):
        st, w = frames[f]
        a, b = int(so[f]), int(so[f + 1])
        lo, hi = max(a, start), min(b, start + length)
        if st or lo >= hi:
            continue
        pos = np.arange(lo, hi, dtype=np.int64)          # positions of the stream or entry: the phase is theirs
        val = np.asarray(w[lo - a:hi - a], dtype=np.int64)
        k = TL.pair_index(pos, step).astype(np.int64)
        bins = (pos - start) // bin_len if bin_len else np.zeros(hi - lo, dtype=np.int64)
        np.add.at(out["n"], bins, 1)
        np.add.at(out["re"], bins, val * tab[k, 0].astype(np.int64))
        np.add.at(out["im"], bins, val * tab[k, 1].astype(np.int64))
        np.minimum.at(out["min"], bins, val.astype(np.int32))
        np.maximum.at(out["max"], bins, val.astype(np.int32))
    for name in ("min", "max", "n"):
        assert np.array_equal(out[name], plain[name])
    return out, status


def range_levels(frames, so, starts, lens, bin_len, stride, cap, step, tab=None, fill=0x5A):
    """range_levels_ref.range_levels' arguments, the step and the table (None: the usual one) -> (records uint8 [cap, 32],
    row offsets, status); ValueError where the call is refused"""
    tab = TL.table() if tab is None else np.asarray(tab, dtype=np.int16).reshape(TL.PAIRS, 2)
    out, off, status = R.range_levels(frames, so, starts, lens, bin_len, stride, cap, fill)
    rec = out.view(TONE_DTYPE).reshape(cap)
    for w in range(len(starts)):
        base, r = int(off[w]), rows_of(lens[w], bin_len)
        if (r > stride) if stride else (base + r > cap):
            continue                          # (no room: the layout's verdict and records stand)
        rec[base:base + r], st = one(frames, so, int(starts[w]), int(lens[w]), bin_len, step, tab)
        assert st == status[w]
    return out, off, status


def view(records):
    """uint8 [rows, 32] (or any buffer of whole records) -> TONE_DTYPE [rows]"""
    return np.ascontiguousarray(records).view(TONE_DTYPE).reshape(-1)
