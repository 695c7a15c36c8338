"""The definition of x3_decode_ranges_dev / x3_corpus_ranges_dev (include/x3hip.h, "RANGES") in numpy, from what the CPU
oracle says about every frame (not a test module).

Inputs: per frame (status, samples) as the oracle's reader gives them -- frames_of() below makes them from a stream --, the
sample offsets, starts and lengths, the row stride (0: packed) and the capacity in samples.  Outputs: the whole output
buffer (positions no call may write keep `fill`), the offsets and the statuses.

Range w is what the single window (starts[w], window_len = lens[w]) is: the samples in front of the first covering frame
that fails, zeros behind them, that frame's status; off the end: ERR_BAD_ARG and zeros; a length of 0 writes nothing and is
0 when start <= total.  Packed rows lie at the exclusive sum of ALL lengths, a row without room is ERR_BAD_ARG and not
written; padded rows lie at w * stride with zeros behind the length, a length above the stride is ERR_BAD_ARG and a row of
zeros."""
import numpy as np

import oracle_lib as O

ERR_BAD_ARG = 24
ERR_HEADER_CRC, ERR_PAYLOAD_CRC = 13, 14


def frame_offsets(stream):
    offs = [0]
    while offs[-1] < stream.size:
        offs.append(offs[-1] + 20 + ((int(stream[offs[-1] + 6]) << 8) | int(stream[offs[-1] + 7])))
    return offs


def frames_of(stream, offs, op=None, so=None):
    """per frame (status, samples or None): header CRC, payload CRC, decode_frame; with `so` (the caller's sample offsets)
    also the header's sample count against so[f + 1] - so[f] (ERR_BAD_ARG: the offsets are not this stream's)"""
    out = []
    for f in range(len(offs) - 1):
        h = stream[offs[f]:offs[f] + 20]
        samples = (int(h[4]) << 8) | int(h[5])
        plen = (int(h[6]) << 8) | int(h[7])
        payload = stream[offs[f] + 20:offs[f] + 20 + plen]
        if O.crc16(h[:16].tobytes()) != ((int(h[16]) << 8) | int(h[17])):
            out.append((ERR_HEADER_CRC, None))
        elif O.crc16(payload.tobytes()) != ((int(h[18]) << 8) | int(h[19])):
            out.append((ERR_PAYLOAD_CRC, None))
        elif so is not None and int(so[f + 1]) - int(so[f]) != samples:
            out.append((ERR_BAD_ARG, None))
        else:
            rc, w = O.decode_frame(payload, samples, op)
            out.append((rc, w if rc == 0 else None))
    return out


def sample_offsets(frames_samples):
    return np.concatenate([[0], np.cumsum(frames_samples)]).astype(np.uint64)


def one(frames, so, start, length):
    """the single window (start, length) -> (row int16 [length], status)"""
    row = np.zeros(length, dtype=np.int16)
    total = int(so[-1])
    if start > total or length > total - start:
        return row, ERR_BAD_ARG
    if length == 0:
        return row, 0
    f = int(np.searchsorted(np.asarray(so, dtype=np.uint64), np.uint64(start), side="right")) - 1
    while f < len(frames) and int(so[f]) < start + length:
        st, w = frames[f]
        a, b = int(so[f]), int(so[f + 1])
        if st:
            return row, st          # (the samples in front of frame f are in place, the rest is zero)
        lo, hi = max(a, start), min(b, start + length)
        row[lo - start:hi - start] = w[lo - a:hi - a]
        f += 1
    return row, 0


def ranges(frames, so, starts, lens, stride, cap, fill=0x5A5A):
    """-> (out int16 [cap], offsets uint64 [n + 1], status int32 [n]); ValueError where the call itself is refused"""
    n = len(starts)
    if n == 0 or (stride and n * stride > cap):
        raise ValueError("the call is refused")
    out = np.full(cap, fill, dtype=np.uint16).view(np.int16)
    lens = [int(v) for v in lens]
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64) if not stride else \
        np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
    status = np.zeros(n, dtype=np.int32)
    for w in range(n):
        base, ln = int(off[w]), lens[w]
        if stride:
            if ln > stride:
                status[w] = ERR_BAD_ARG
                out[base:base + stride] = 0
                continue
            out[base + ln:base + stride] = 0
        elif base + ln > cap:
            status[w] = ERR_BAD_ARG          # (no room: nothing of the row is written)
            continue
        row, status[w] = one(frames, so, int(starts[w]), ln)
        out[base:base + ln] = row
    return out, off, status


def f32_bits(a):
    return (np.asarray(a, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).view(np.uint32)
