"""The definition of x3_signal_range_levels_dev / x3_corpus_signal_range_levels_dev (include/x3hip.h, "SIGNAL RANGE LEVELS") in
numpy, from what the CPU oracle says about every frame (not a test module).

ONE RULE: the call cuts the stream's (or entry's) difference signal; it does not difference the cut.  signal_of() builds that
signal y and the mask of the positions that count from the frames (ranges_ref.frames_of) and the sample offsets, exactly as
x3_signal_levels_dev defines them:
    sample i >= 1 of frame f: y = clamp(x_f[i] - x_f[i-1]), counted iff frame f has status 0;
    sample 0 of frame f:      y = clamp(x_f[0] - x_{f-1}[last]), counted iff f >= 1 and frames f - 1 and f both have status 0;
    the first position of the stream: never counted.
(An entry of a corpus is a stream of its own here, so no seam crosses from one entry into the next.)  Range w then has the
records of range_levels_ref with y[start + r] in place of x[start + r]: one() reduces y[start:start + len] by bins counted
from `start`.  Rows, layouts, row offsets, refusals and the STATUSES are range_levels_ref.range_levels' own -- the status of a
range never depends on the signal, and the frame in front of a range's first covering frame never gives it one."""
import numpy as np

import range_levels_ref as R
from levels_ref import LEVEL_DTYPE, empty

SAMPLES, DIFF = 0, 1
ERR_BAD_ARG = R.ERR_BAD_ARG
rows_of, view = R.rows_of, R.view


def signal_of(frames, so):
    """-> (y int64 [total], counted bool [total]) of the stream whose frames are (status, samples or None)"""
    total = int(so[-1])
    y, counted = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=bool)
    for f, (st, w) in enumerate(frames):
        if st:
            continue
        a = int(so[f])
        x = np.asarray(w, dtype=np.int64)
        y[a + 1:a + x.size] = x[1:] - x[:-1]
        counted[a + 1:a + x.size] = True
        if f >= 1 and frames[f - 1][0] == 0:
            y[a] = int(x[0]) - int(frames[f - 1][1][-1])
            counted[a] = True
    return np.clip(y, -32768, 32767), counted


def one(frames, so, start, length, bin_len, signal=DIFF, sig=None):
    """the single range (start, length) -> (LEVEL_DTYPE [R], status); sig: signal_of(frames, so), when the caller has it"""
    out, status = R.one(frames, so, start, length, bin_len)
    total = int(so[-1])
    if signal == SAMPLES or start > total or length > total - start or length == 0:   # (off the end: identities)
        return out, status
    y, counted = sig if sig is not None else signal_of(frames, so)
    out = empty(rows_of(length, bin_len))
    pos = np.flatnonzero(counted[start:start + length])
    val = y[start:start + length][pos]
    bins = pos // bin_len if bin_len else np.zeros_like(pos)
    np.add.at(out["n"], bins, 1)
    np.add.at(out["sum"], bins, val)
    np.add.at(out["sum_sq"], bins, (val * val).astype(np.uint64))
    np.minimum.at(out["min"], bins, val.astype(np.int32))
    np.maximum.at(out["max"], bins, val.astype(np.int32))
    return out, status


def range_levels(frames, so, starts, lens, bin_len, stride, cap, signal=DIFF, fill=0x5A):
    """range_levels_ref.range_levels' arguments and `signal` -> (records uint8 [cap, 32], row offsets, status); ValueError
    where the call is refused"""
    out, off, status = R.range_levels(frames, so, starts, lens, bin_len, stride, cap, fill)
    if signal == SAMPLES:
        return out, off, status
    assert signal == DIFF
    rec = out.view(LEVEL_DTYPE).reshape(cap)
    sig = signal_of(frames, so)
    for w in range(len(starts)):
        base, r = int(off[w]), rows_of(lens[w], bin_len)
        if (r > stride) if stride else (base + r > cap):
            continue                          # (no room: the layout's verdict and records stand)
        rec[base:base + r], st = one(frames, so, int(starts[w]), int(lens[w]), bin_len, DIFF, sig)
        assert st == status[w]
    return out, off, status
