"""numpy reference of x3_signal_levels_dev / x3_corpus_signal_levels_dev (include/x3hip.h, "SIGNAL LEVELS"; not a test module).

Positions and bins are levels_ref's.  With "diff" the position of sample i >= 1 of frame f holds clamp(x_f[i] - x_f[i-1]),
counted iff frame f has status 0; the position of sample 0 of frame f holds clamp(x_f[0] - x_{f-1}[last]), counted iff
f >= 1 and frames f - 1 and f both have status 0 (entries of a corpus are separate calls here, so no seam crosses from one
into the next).  Every other position adds nothing.  clamp is to [-32768, 32767]."""
import numpy as np

import levels_ref as R

LEVEL_DTYPE = R.LEVEL_DTYPE
SAMPLES, DIFF = 0, 1


def _bin(out, pos, val, bin_len):
    """levels_ref.levels' binning of values at positions"""
    n_bins = out.size
    bins = pos // bin_len if bin_len else np.zeros_like(pos)
    keep = bins < n_bins
    bins, val = bins[keep], val[keep]
    np.add.at(out["n"], bins, 1)
    np.add.at(out["sum"], bins, val)
    np.add.at(out["sum_sq"], bins, (val * val).astype(np.uint64))
    np.minimum.at(out["min"], bins, val.astype(np.int32))
    np.maximum.at(out["max"], bins, val.astype(np.int32))


def signal_levels(frames, statuses, sample_offsets, bin_len, n_bins, signal):
    """levels_ref.levels' arguments and `signal` (SAMPLES | DIFF) -> LEVEL_DTYPE[n_bins]"""
    if signal == SAMPLES:
        return R.levels(frames, statuses, sample_offsets, bin_len, n_bins)
    assert signal == DIFF
    out = R.empty(n_bins)
    pos, val = [], []
    for f, (w, st, so) in enumerate(zip(frames, statuses, sample_offsets)):
        if st != 0 or not len(w):
            continue
        x = np.asarray(w, dtype=np.int64)
        pos.append(int(so) + np.arange(1, len(x), dtype=np.int64))
        val.append(x[1:] - x[:-1])
        if f >= 1 and statuses[f - 1] == 0 and len(frames[f - 1]):
            pos.append(np.array([int(so)], dtype=np.int64))
            val.append(np.array([int(x[0]) - int(frames[f - 1][-1])], dtype=np.int64))
    if pos:
        _bin(out, np.concatenate(pos), np.clip(np.concatenate(val), -32768, 32767), bin_len)
    return out


def corpus_signal_levels(entries, bin_len, signal):
    """levels_ref.corpus_levels' entries and `signal` -> (LEVEL_DTYPE[rows], row_first)"""
    rf = R.corpus_row_first([e[3] for e in entries], bin_len)
    out = R.empty(int(rf[-1]))
    for e, (frames, statuses, so, _) in enumerate(entries):
        a, b = int(rf[e]), int(rf[e + 1])
        out[a:b] = signal_levels(frames, statuses, so, bin_len, b - a, signal)
    return out, rf
