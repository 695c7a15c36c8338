"""GPU parity on SHORT and CORRUPT payloads: the reference's BitReader is not "a bit string that is zero behind its
end" there (src/bitreader.rs:128-139: a zero run is extended by at most one peeked word; :148-163 + :76-92: behind
the last byte zero runs come back as phantom counts), so a frame whose header asks for more samples than its payload
encodes decodes "successfully" in the reference, to values that depend on that state machine.  The GPU decoders defer
such frames to an exact replay (x3_decode_replay.h); these tests feed thousands of them -- payloads cut inside
Rice0 / Rice1 / Rice3 / BFP / literal blocks, sample counts beyond the payload, zero runs of 32 bits and more (also
with codes[0] in {2, 3}, where such runs are valid indices), plain garbage -- and compare status and samples of every
frame with the oracle's decode_frame, through each of the three decoder kernels.  `pytest -m gpu`."""
import numpy as np
import pytest

import oracle_lib as O
from x3_cases import compare, crafted_frames, oparams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.mark.parametrize("mode", ["batch", "offsets", "offsets_x4"])
def test_short_and_corrupt_payloads_default_params(x3, mode):
    rng = np.random.default_rng(20261004)
    p = x3.Params.default()
    frames = crafted_frames(x3, rng, p, 3000)
    ctx = x3.Context(0)
    try:
        seen = compare(x3, ctx, p, frames, mode)
    finally:
        ctx.close()
    # all three outcomes occur: phantom decodes that succeed, OutOfBoundsInverse, InvalidBPF
    assert seen.get(0, 0) > 300 and seen.get(5, 0) > 100 and seen.get(20, 0) > 100, seen


def test_single_wave_kernel_forced(x3):
    rng = np.random.default_rng(77)
    p = x3.Params.default()
    frames = crafted_frames(x3, rng, p, 1500)
    ctx = x3.Context(0)
    try:
        ctx.set_option("decode_single", 1)
        compare(x3, ctx, p, frames, "batch")
    finally:
        ctx.close()


@pytest.mark.parametrize("codes,thr,bl", [((2, 1, 3), (3, 8, 20), 20), ((3, 1, 3), (3, 8, 20), 20),
                                          ((3, 3, 3), (2, 9, 27), 20), ((0, 1, 3), (3, 8, 20), 7),
                                          ((2, 2, 2), (3, 8, 18), 33), ((0, 0, 0), (1, 2, 5), 20)])
def test_zero_runs_general_codes(x3, codes, thr, bl):
    """codes[0] in {2,3}: the r1 path bounds the run by inv_len 44 / 60, so runs of 32 and more are valid indices
    and the reference's one-word peek decides what they decode to; other block lengths take the single-wave kernels"""
    rng = np.random.default_rng(sum(codes) * 100 + bl)
    p = x3.Params.make(bl, 500, codes, thr)
    frames = crafted_frames(x3, rng, p, 1200)
    ctx = x3.Context(0)
    try:
        for mode in ("batch", "offsets"):
            compare(x3, ctx, p, frames, mode)
    finally:
        ctx.close()


def test_stream_walk_continues_over_phantom_frames(x3):
    """a frame that only decodes through phantom reads is a GOOD frame to the reference's walk: the frames behind it
    are decoded too, and the sample count includes it (x3_decode_stream, both walks, and x3_decode_frame)"""
    rng = np.random.default_rng(5)
    p = x3.Params.default()
    op = oparams(p)
    good = O.encode(x3.synth(2, 9, 0, 20000))[1]
    frames = crafted_frames(x3, rng, p, 400)
    ctx = x3.Context(0)
    try:
        tried = 0
        for pay, n in frames:
            rc_o, w_o = O.decode_frame(pay, n, op)
            stream = np.concatenate([good, x3.write_frame_header(n, 1, pay.size, O.crc16(pay)), pay, good])
            r_o = O.decode_stream(stream, op, wav_cap=200000)
            for host_walk in (1, 0):
                ctx.set_option("host_walk", host_walk)
                r_g = ctx.decode_stream(stream, p, wav_cap=200000)
                ctx.set_option("host_walk", -1)
                assert (r_g[0], r_g[2], r_g[3]) == (r_o[0], r_o[2], r_o[3]), (host_walk, pay.size, n, r_g[0], r_g[2:], r_o[0], r_o[2:])
                assert np.array_equal(r_g[1], r_o[1])
            rc_g, w_g = ctx.decode_frame(pay, n)
            assert rc_g == rc_o and (rc_o != 0 or np.array_equal(w_g, w_o))
            tried += 1
            if tried >= 60:
                break
        assert tried >= 40
    finally:
        ctx.close()
