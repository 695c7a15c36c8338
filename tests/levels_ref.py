"""numpy reference of x3_levels_dev / x3_corpus_levels_dev (include/x3hip.h; not a test module).

Positions: sample i of frame f is at sample_offsets[f] + i.  Bin b covers [b * bin_len, (b + 1) * bin_len), bin_len 0 = one
bin.  A frame with status 0 adds every sample to its bin, any other frame adds nothing; positions at or beyond n_bins *
bin_len are not counted; an empty bin holds the identities (min 32767, max -32768, n 0)."""
import numpy as np

LEVEL_DTYPE = np.dtype([("sum_sq", np.uint64), ("sum", np.int64), ("min", np.int32), ("max", np.int32), ("n", np.uint32),
                        ("reserved", np.uint32)])


def empty(n_bins):
    out = np.zeros(n_bins, dtype=LEVEL_DTYPE)
    out["min"], out["max"] = 32767, -32768
    return out


def n_bins_for(total, bin_len):
    """bins that exactly cover `total` positions (at least one)"""
    return max(1, -(-total // bin_len)) if bin_len else 1


def levels(frames, statuses, sample_offsets, bin_len, n_bins):
    """frames: per frame its samples (int16 array; ignored where the status is not 0), statuses: per frame, sample_offsets:
    per frame the position of its sample 0 -> LEVEL_DTYPE[n_bins]"""
    out = empty(n_bins)
    pos, val = [], []
    for w, st, so in zip(frames, statuses, sample_offsets):
        if st == 0 and len(w):
            pos.append(int(so) + np.arange(len(w), dtype=np.int64))
            val.append(np.asarray(w, dtype=np.int64))
    if not pos:
        return out
    pos, val = np.concatenate(pos), np.concatenate(val)
    bins = pos // bin_len if bin_len else np.zeros_like(pos)
    keep = bins < n_bins
    bins, val = bins[keep], val[keep]
    np.add.at(out["n"], bins, 1)
    np.add.at(out["sum"], bins, val)
    np.add.at(out["sum_sq"], bins, (val * val).astype(np.uint64))
    np.minimum.at(out["min"], bins, val.astype(np.int32))
    np.maximum.at(out["max"], bins, val.astype(np.int32))
    return out


def corpus_row_first(n_samples, bin_len):
    """entry e has max(1, ceil(n_samples[e] / bin_len)) rows, one with bin_len 0 -> the exclusive prefix, n + 1 words"""
    rows = [n_bins_for(int(n), bin_len) for n in n_samples]
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)


def corpus_levels(entries, bin_len):
    """entries: per entry (frames, statuses, sample_offsets relative to the entry, n_samples) -> (LEVEL_DTYPE[rows], row_first)"""
    rf = corpus_row_first([e[3] for e in entries], bin_len)
    out = empty(int(rf[-1]))
    for e, (frames, statuses, so, _) in enumerate(entries):
        a, b = int(rf[e]), int(rf[e + 1])
        out[a:b] = levels(frames, statuses, so, bin_len, b - a)
    return out, rf
