"""The definition of x3_range_levels_dev / x3_corpus_range_levels_dev (include/x3hip.h, "RANGE LEVELS") in numpy, from what
the CPU oracle says about every frame (not a test module).

Inputs: per frame (status, samples) as ranges_ref.frames_of() gives them, the sample offsets, starts and lengths, the bin
length, the row stride (0: packed) and the capacity in records.  Outputs: the whole record array as bytes [cap, 32]
(records no call may write keep `fill`), the row offsets and the statuses.

Range w is positions [starts[w], starts[w] + lens[w]); its bin b covers [start + b * bin_len, start + (b + 1) * bin_len) cut
to the range (bin_len 0, or 2^32 and above: one bin); it has R(w) = max(1, ceil(len / bin_len)) rows, for bad ranges too.  A
sample counts when the frame that holds it has status 0, any other frame adds nothing; the range's status is that of the
first covering frame, in frame order, that is not 0.  Off the end (start > total or len > total - start): ERR_BAD_ARG and
identities.  Packed rows lie at the exclusive sum of ALL R(w), a range without room is ERR_BAD_ARG and not written; padded
rows lie at w * stride with identities behind R(w), R(w) above the stride is ERR_BAD_ARG and a row of identities."""
import numpy as np

from levels_ref import LEVEL_DTYPE, empty
from ranges_ref import ERR_BAD_ARG, frames_of, sample_offsets   # noqa: F401  (what the callers build the inputs with)


def rows_of(length, bin_len):
    """R(w): max(1, ceil(len / bin_len)), one with bin_len 0"""
    return max(1, -(-int(length) // int(bin_len))) if bin_len else 1


def one(frames, so, start, length, bin_len):
    """the single range (start, length) -> (LEVEL_DTYPE [R], status)"""
    out = empty(rows_of(length, bin_len))
    total = int(so[-1])
    if start > total or length > total - start:
        return out, ERR_BAD_ARG
    if length == 0:
        return out, 0
    status = 0
    f = int(np.searchsorted(np.asarray(so, dtype=np.uint64), np.uint64(start), side="right")) - 1
    while f < len(frames) and int(so[f]) < start + length:
        st, w = frames[f]
        a, b = int(so[f]), int(so[f + 1])
        if st:
            status = status or st              # (the first in frame order; the frames behind it still count)
        else:
            lo, hi = max(a, start), min(b, start + length)
            val = np.asarray(w[lo - a:hi - a], dtype=np.int64)
            bins = (np.arange(lo, hi, dtype=np.int64) - start) // bin_len if bin_len else np.zeros(hi - lo, dtype=np.int64)
            np.add.at(out["n"], bins, 1)
            np.add.at(out["sum"], bins, val)
            np.add.at(out["sum_sq"], bins, (val * val).astype(np.uint64))
            np.minimum.at(out["min"], bins, val.astype(np.int32))
            np.maximum.at(out["max"], bins, val.astype(np.int32))
        f += 1
    return out, status


def range_levels(frames, so, starts, lens, bin_len, stride, cap, fill=0x5A):
    """-> (records uint8 [cap, 32], row offsets uint64 [n + 1], status int32 [n]); ValueError where the call is refused"""
    n = len(starts)
    if n == 0 or cap == 0 or (stride and n * stride > cap):
        raise ValueError("the call is refused")
    out = np.full((cap, LEVEL_DTYPE.itemsize), fill, dtype=np.uint8)
    rec = out.view(LEVEL_DTYPE).reshape(cap)
    lens = [int(v) for v in lens]
    rows = [rows_of(ln, bin_len) for ln in lens]
    off = np.concatenate([[0], np.cumsum(rows, dtype=np.uint64)]).astype(np.uint64) if not stride else \
        np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
    status = np.zeros(n, dtype=np.int32)
    for w in range(n):
        base, r = int(off[w]), rows[w]
        if stride:
            rec[base:base + stride] = empty(stride)
            if r > stride:
                status[w] = ERR_BAD_ARG
                continue
        elif base + r > cap:
            status[w] = ERR_BAD_ARG          # (no room: none of its records is written)
            continue
        rec[base:base + r], status[w] = one(frames, so, int(starts[w]), lens[w], bin_len)
    return out, off, status


def view(records):
    """uint8 [rows, 32] (or any buffer of whole records) -> LEVEL_DTYPE [rows]"""
    return np.ascontiguousarray(records).view(LEVEL_DTYPE).reshape(-1)
