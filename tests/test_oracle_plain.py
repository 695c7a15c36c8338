"""The oracle's plain-frame predicate (x3o_frame_plain) against the oracle's decode_frame, on the CPU.

The GPU's fast decoders hand every frame they are unsure of to the reference's reader (x3_decode_replay.h), and the GPU
tests count those replays against this predicate.  That rests on two claims the replay header makes in prose:
  * what an encoder writes is plain -- read as a plain bit string, every block decodes, no zero run reaches 32 bits, no
    read lies behind the payload (so conforming streams never reach the reference's reader);
  * on a plain frame the reference's reader, with its one-word peeks and phantom counts, gives the same samples and status
    (so a fast decoder that decodes a plain frame itself is exact).
Pinned here on oracle-encoded streams of every parameter set the GPU code-set tests use, and on the crafted, edge and
damaged frames they decode."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_code_sets import PIDS, PSETS, content, edge_frames
from x3_cases import crafted_frames, damage, frame_offsets, patchwork

GEOMS = [(10, 200), (20, 100), (40, 50), (13, 100)]


class _Synth:
    """crafted_frames' use of x3hip: synth kind 2 (white noise) stands in as a seeded draw"""
    @staticmethod
    def synth(kind, seed, start, n):
        return np.random.default_rng(seed + start).integers(-32768, 32768, size=n).astype(np.int16)


def _frames(stream):
    """(payload, samples) of every frame of an intact stream"""
    out = []
    for o in frame_offsets(stream):
        n = int(stream[o + 4]) << 8 | int(stream[o + 5])
        plen = int(stream[o + 6]) << 8 | int(stream[o + 7])
        out.append((stream[o + 20:o + 20 + plen], n))
    return out


def _same_as_decode_frame(pay, n, po, what):
    """-> plain?  A plain frame decodes to decode_frame's samples with status 0"""
    pl, w = O.frame_plain(pay, n, po)
    assert pl in ((-1,) if n == 0 else (0, 1)), what
    if pl:
        rc_o, w_o = O.decode_frame(pay, n, po)
        assert rc_o == 0, (what, rc_o)
        assert np.array_equal(w, w_o), what
    return pl


def conforming(codes, thr):
    """the reference's decoder reads what its encoder writes: it hard-wires the Rice codes (0, 1, 3) -- a type-1 codeword
    without sub-bits, 2 and 4 bits behind the zeros of types 2 and 3 (decoder.rs:147-196) -- and refuses BFP widths of 5
    bits or less, which thresholds[2] < 16 lets the encoder write"""
    return tuple(codes) == (0, 1, 3) and thr[2] >= 16


@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_encoded_frames_are_plain(codes, thr):
    """every frame the oracle's encoder writes is plain wherever its decoder reads what it writes (elsewhere: a plain
    frame still decodes exactly as decode_frame does), for patchwork, white noise and silence at block lengths 10, 20, 40, 13"""
    for bl, bpf in GEOMS:
        po = O.Params.make(bl, bpf, codes, thr)
        spf = bl * bpf
        n = 7 * spf + spf // 3 + 1
        rng = np.random.default_rng(bl)
        clips = [content(codes, thr, bl, bpf, 5 * bl + 1, n), np.zeros(n, dtype=np.int16)]
        white = rng.integers(-32768, 32768, size=n).astype(np.int16)
        if O.encode(white, po)[0] == 0:   # (past the single-pass encoders' edge a literal may be outside the tables)
            clips.append(white)
        for k, w in enumerate(clips):
            rc, s, _ = O.encode(w, po)
            assert rc == 0
            for f, (pay, m) in enumerate(_frames(s)):
                pl = _same_as_decode_frame(pay, m, po, (bl, k, f))
                if conforming(codes, thr):
                    assert pl == 1, (bl, k, f)


@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_plain_frames_decode_as_decode_frame(codes, thr):
    """crafted frames (cut, overlong, zero runs, garbage), the edge codewords of every index bound and the 32-bit run limit,
    and every frame of damaged streams: each one that is plain decodes exactly as decode_frame does; and the predicate's
    verdicts are not all one way (both kinds are there)"""
    rng = np.random.default_rng(sum(codes) * 1000 + thr[0] * 100 + thr[1] * 10 + thr[2])
    for bl, bpf in GEOMS:
        po = O.Params.make(bl, bpf, codes, thr)
        p = type("P", (), {"block_len": bl, "codes": codes, "thresholds": thr})
        frames = crafted_frames(_Synth, rng, p, 600) + edge_frames(bl)
        spf = bl * bpf
        rc, stream, _ = O.encode(content(codes, thr, bl, bpf, 11 * bl + 3, 41 * spf + 7), po)
        assert rc == 0
        offs = frame_offsets(stream)
        for _ in range(10):
            frames += _frames(damage(rng, stream, offs))
        kinds = set()
        for i, (pay, n) in enumerate(frames):
            if pay.size < 2 or n == 0:
                continue
            kinds.add(_same_as_decode_frame(pay, n, po, (bl, i, pay.size, n)))
        assert kinds == {0, 1}, bl


def test_edge_codewords():
    """one-block frames at each type's index bound: index bound - 1 is plain, the bound is not; runs of 31 zeros can be plain,
    32 never (a type-1 block under codes 2 and 3 takes runs up to 43 and 59 as indices, and decode_frame decodes them; the
    predicate does not: the reference's reader counts such runs by its own rules)"""
    for codes in ((0, 1, 3), (1, 1, 3), (2, 1, 3), (3, 1, 3)):
        po = O.Params.make(20, 100, codes, (3, 8, 20))
        bound = (16, 26, 44, 60)[codes[0]]   # the inverse tables' lengths (x3.rs:187-194)
        for z in range(62):
            bits = "01" + ("0" * z + "1") + "1" * 19
            bits += "0" * (-len(bits) % 8)
            body = np.array([int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)], dtype=np.uint8)
            pay = np.concatenate([np.array([0, 0], dtype=np.uint8), body])
            pl, _ = O.frame_plain(pay, 21, po)
            assert pl == (1 if z < min(bound, 32) else 0), (codes, z)
            rc_o, _ = O.decode_frame(pay, 21, po)
            if z < bound:
                assert rc_o == 0, (codes, z)


def test_multichannel_frames_are_plain():
    """multi-channel frames from the oracle's encoder are plain, and decode as decode_stream_mc does"""
    po = O.Params.make(20, 100, (0, 1, 3), (3, 8, 20))
    for n_ch in (2, 3):
        wavs = [patchwork(17 + c, 9 * 2000 + 77) for c in range(n_ch)]
        rc, s, _ = O.encode_mc(wavs, po)
        assert rc == 0
        at = 0
        for pay, m in _frames(s):
            pl, w = O.frame_plain(pay, m, po, n_ch=n_ch)
            assert pl == 1
            for c in range(n_ch):
                assert np.array_equal(w[c], wavs[c][at:at + m]), (n_ch, c, at)
            at += m
        assert at == wavs[0].size
