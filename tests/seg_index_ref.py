"""The segment index of a stream, from the CPU oracle alone (include/x3hip.h, "The SEGMENT INDEX").

Per frame: x3o_br_new on the payload behind its first sample, x3o_decode_block block by block; in front of every
seg_blocks-th block the reader's position (8 * idx - rem_bit of x3o_bitreader, counted from the payload's first byte) and
last_wav.  The oracle's decoder is hard-wired to codes (0, 1, 3), so this reference serves those codes only.  Test
infrastructure: no GPU."""
import ctypes as C

import numpy as np

import oracle_lib as O

SEG_MAGIC = 0x58335347
SEG_VALID = 0x10000


def frames(stream):
    """byte offsets of the frames of a clean stream (header to header), n + 1 entries"""
    offs = [0]
    while offs[-1] + 20 <= stream.size:
        nxt = offs[-1] + 20 + ((int(stream[offs[-1] + 6]) << 8) | int(stream[offs[-1] + 7]))
        if nxt > stream.size:
            break
        offs.append(nxt)
    return offs


def header(stream, off):
    """(samples, payload_len) of the frame header at byte `off`"""
    return (int(stream[off + 4]) << 8) | int(stream[off + 5]), (int(stream[off + 6]) << 8) | int(stream[off + 7])


def n_seg(params, seg_blocks):
    return (params.blocks_per_frame + seg_blocks - 1) // seg_blocks


def n_words(n_frames, params, seg_blocks):
    ns = n_seg(params, seg_blocks)
    return 1 + n_frames * (ns - 1) if ns >= 2 else 0


def reader_at(payload, bit):
    """the oracle's reader over `payload` (np.uint8, kept alive by the caller), standing at bit `bit` of it"""
    br = O.BitReader()
    byte = bit >> 3
    O.lib().x3o_br_new(C.byref(br), payload.ctypes.data + byte, payload.size - byte)
    if bit & 7:
        O.lib().x3o_br_read_nbits(C.byref(br), bit & 7)
    return br, byte


def position(br, byte0):
    return 8 * (byte0 + br.idx) - br.rem_bit


def decode_from(payload, samples, params, block, bit, prev):
    """samples of blocks block, block + 1, ... of the frame, the reader started at `bit` with `prev` in front.
    -> (rc, np.int16 array of what decoded, [(block, bit, prev) in front of every block walked])"""
    L = O.lib()
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    br, byte0 = reader_at(payload, bit)
    bl = params.block_len
    out = np.zeros(max(samples, 1), dtype=np.int16)
    last = C.c_int16(np.int16(np.uint16(prev & 0xFFFF)))
    at = 1 + block * bl
    n_out = 0
    marks = []
    b = block
    while at < samples:
        marks.append((b, position(br, byte0), int(last.value) & 0xFFFF))
        n = min(bl, samples - at)
        rc = L.x3o_decode_block(C.byref(br), out.ctypes.data + 2 * n_out, n, C.byref(last), C.byref(params))
        if rc:
            return rc, out[:n_out].copy(), marks
        at += n
        n_out += n
        b += 1
    return 0, out[:n_out].copy(), marks


def build(stream, frame_offsets, params, seg_blocks):
    """the index of the frames at `frame_offsets` (byte offsets; intact frames) -> np.uint64 words, and per frame the
    number of entries that must be valid (those in front of a block the frame has)"""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    ns = n_seg(params, seg_blocks)
    F = len(frame_offsets)
    words = np.zeros(n_words(F, params, seg_blocks), dtype=np.uint64)
    expect = []
    if ns < 2:
        return words, [0] * F
    words[0] = np.uint64(SEG_MAGIC | (seg_blocks << 32))
    for f, off in enumerate(frame_offsets):
        off = int(off)
        samples, plen = header(stream, off)
        payload = stream[off + 20:off + 20 + plen]
        first = (int(payload[0]) << 8) | int(payload[1])
        rc, _, marks = decode_from(payload, samples, params, 0, 16, first)
        assert rc == 0, "seg_index_ref.build: frame %d does not decode (%d)" % (f, rc)
        k = 0
        for b, bit, prev in marks:
            if b and b % seg_blocks == 0 and b // seg_blocks <= ns - 1:
                words[1 + f * (ns - 1) + b // seg_blocks - 1] = np.uint64(bit | ((prev | SEG_VALID) << 32))
                k += 1
        expect.append(k)
    return words, expect
