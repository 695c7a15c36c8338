"""The definition of x3_fir_range_levels_dev / x3_corpus_fir_range_levels_dev (include/x3hip.h, "FIR RANGE LEVELS") in numpy,
from what the CPU oracle says about every frame (not a test module).

ONE RULE: the call cuts the stream's (or entry's) FIR signal; it does not filter the cut.  signal_of() builds that signal y
and the mask of the positions that count with fir_levels_ref.signal -- THE HISTORY RULE: position i counts iff all T
positions i - T + 1 .. i exist and lie in frames of status 0 -- padded with positions that do not count up to so[-1] (the
frames at the end may have failed).  Range w then has the records of range_levels_ref with y[start + r] in place of
x[start + r]: signal_range_levels_ref.one(..., sig=...) reduces y[start:start + len] by bins counted from `start`.  Rows,
layouts, row offsets, refusals and the STATUSES are range_levels_ref.range_levels' own: the status of a range never depends on
the taps, and a frame in front of a range's first covering frame never gives it one.  (An entry of a corpus is a stream of
its own here, so no history crosses from one entry into the next.)"""
import numpy as np

import fir_levels_ref as FL
import range_levels_ref as R
import signal_range_levels_ref as S
from levels_ref import LEVEL_DTYPE

ERR_BAD_ARG = R.ERR_BAD_ARG
rows_of, view = R.rows_of, R.view


def signal_of(frames, so, taps, shift=0):
    """-> (y int64 [total], counted bool [total]) of the stream whose frames are (status, samples or None)"""
    total = int(so[-1])
    y, counted = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=bool)
    ys, cs = FL.signal([w if st == 0 else [] for st, w in frames], [st for st, _ in frames], [int(v) for v in so[:-1]], taps, shift)
    assert ys.size <= total
    y[:ys.size], counted[:ys.size] = ys, cs
    return y, counted


def one(frames, so, start, length, bin_len, taps, shift=0, sig=None):
    """the single range (start, length) -> (LEVEL_DTYPE [R], status)"""
    return S.one(frames, so, start, length, bin_len, S.DIFF, sig if sig is not None else signal_of(frames, so, taps, shift))


def range_levels(frames, so, starts, lens, bin_len, stride, cap, taps, shift=0, fill=0x5A):
    """range_levels_ref.range_levels' arguments, the taps and the shift -> (records uint8 [cap, 32], row offsets, status);
    ValueError where the call is refused"""
    out, off, status = R.range_levels(frames, so, starts, lens, bin_len, stride, cap, fill)
    rec = out.view(LEVEL_DTYPE).reshape(cap)
    sig = signal_of(frames, so, taps, shift)
    for w in range(len(starts)):
        base, r = int(off[w]), rows_of(lens[w], bin_len)
        if (r > stride) if stride else (base + r > cap):
            continue                          # (no room: the layout's verdict and records stand)
        rec[base:base + r], st = one(frames, so, int(starts[w]), int(lens[w]), bin_len, taps, shift, sig)
        assert st == status[w]
    return out, off, status
