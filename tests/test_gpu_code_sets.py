"""Every encoder generation and every decoder kernel against the oracle on Rice code sets and thresholds other than the
defaults (codes (0, 1, 3), thresholds (3, 8, 20)), at block lengths 10, 20, 40 and 13.

x3_params_validate accepts any code per block type and thresholds up to the code's table offset, and the kernels take
such parameters.  The decoder's kernel choice depends on the codes (x3_decode.hip, decode_route): the branch-free kernels need codes[0]
in {0, 1}; the three-wave and block-per-lane kernels also need codes[1] == 1 and codes[2] == 3 -- so (1, 1, 3) goes
through both flagship decoders.  The reference's decoder hard-wires the sub-code widths of block types 2 and 3
(decoder.rs:180): a stream written with another code set decodes to errors or to other samples.  That is the point here:
valid headers and CRCs around bit patterns the default encoder never writes, with an exact answer from the oracle.
Encoders: bytes, statistics, status and the generation in use.  Decoders: status, frame counts, first failing frame,
samples and the 0x5A guard behind each row, and the kernel in use (a coverage table that must be filled).
No output can show a fast kernel whose index bound is too LOW: every index it refuses sends the frame to the reference's
reader (x3_decode_replay.h), which decides exactly.  So every decode here also counts those replays (option
last_decode_replays) against the oracle's plain-frame predicate (oracle_lib.frame_plain): a kernel must hand over exactly
the frames that are not plain -- the edge codewords test each index bound from the fast side too.  A bound too high, or a
parse that hard-wires part of the default code set, gives other statuses or samples."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from x3_cases import AMPS, compare, crafted_frames, damage, frame_offsets, not_plain, oparams, patchwork, walked_frames

pytestmark = pytest.mark.gpu

RICE_OFFSET, RICE_LEN = (6, 11, 20, 28), (14, 22, 40, 56)

# (codes, thresholds)
PSETS = [
    ((0, 1, 3), (3, 8, 20)),     # the defaults: control
    ((1, 1, 3), (3, 8, 20)),     # the fast kernels' other code set
    ((1, 1, 3), (5, 9, 24)),
    ((1, 1, 3), (9, 4, 20)),     # thr0 >= thr1: no block of type 2
    ((1, 1, 3), (3, 8, 12)),     # thr2 < 16: BFP blocks the reference's decoder refuses
    ((1, 1, 3), (6, 10, 27)),    # the edge of what the single-pass encoders take (x3_encode.hip, stream_safe_thresholds)
    ((1, 1, 3), (6, 10, 28)),    # one past it: the general encoder
    ((0, 1, 3), (6, 10, 27)),    # the edge on the default codes
    ((0, 1, 3), (6, 4, 14)),     # thr0 >= thr1 and thr2 < 16 on the default codes
    ((0, 0, 0), (2, 4, 6)),
    ((0, 1, 2), (3, 8, 18)),
    ((1, 2, 3), (5, 10, 25)),
    ((0, 2, 3), (3, 8, 20)),
    ((3, 3, 3), (2, 9, 27)),
    ((2, 1, 3), (3, 8, 20)),
    ((3, 1, 3), (3, 8, 20)),
]
PIDS = ["c%d%d%d-t%d_%d_%d" % (c + t) for c, t in PSETS]

# (block_len, blocks_per_frame): 2 000 samples a frame (100 runs of 20: the single-pass encoders), and an odd length
GEOMS = [(10, 200), (20, 100), (40, 50), (13, 100)]

# decoder settings: (name, options)
DECODERS = [("default", {}), ("blocks", {"decode_blocks": 1}), ("no_blocks", {"decode_blocks": 0}),
            ("single", {"decode_single": 1}), ("blocks_off", {"decode_blocks_off": 1})]
OPTS = ("decode_blocks", "decode_single", "decode_blocks_off")

COVER = {}   # (codes, thr, bl, decoder) -> kernels seen on intact layouts


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def stream_safe(codes, thr):
    """x3_encode.hip's stream_safe_thresholds (encode_route): no block can need a difference outside its code's table"""
    mmax, used = [0, 0, 0], [False] * 3
    for m in range(min(thr[2], 70000) + 1):
        ft = (m > thr[0]) + (m > thr[1])
        used[ft], mmax[ft] = True, m
    return all(not used[ft] or mmax[ft] <= min(RICE_OFFSET[codes[ft]], RICE_LEN[codes[ft]] - RICE_OFFSET[codes[ft]] - 1)
               for ft in range(3))


def expected_gen(codes, thr, bl, bpf, n, gen, two_pass):
    """the generation x3_encode* runs: the one asked for, or the general kernel (1) when the block length is not 10/20/40,
    frames are not a multiple of four samples, a frame holds more than 512 runs of 20, or the thresholds are not
    stream-safe; two passes (0) when asked for"""
    if two_pass:
        return 0
    spf = bl * bpf
    if bl not in (10, 20, 40) or spf % 4 or (min(spf, n) + 18) // 20 > 512 or not stream_safe(codes, thr):
        return 1
    return gen


def expected_kernel(codes, bl, blocks, single, blocks_off):
    """decode_kernel_in_use on a layout whose rows sit on 8-byte boundaries: 3 block per lane, 2 three waves, 1 single wave
    (branch-free), 0 single wave (general)"""
    if codes[0] not in (0, 1):
        return 0                       # (a Rice-1 codeword of codes 2 and 3 can pass 32 bits)
    if codes[1:] != (1, 3) or single:
        return 1
    if bl == 20:
        return 3 if blocks else 2
    if bl in (10, 40):
        return 1 if blocks_off else 3
    return 1


def content(codes, thr, bl, bpf, seed, n):
    """patchwork; for thresholds past the single-pass encoders' edge, the first seed whose content the reference can
    encode (a difference outside the code's table is a panic there, X3_ERR_BAD_ARG here)"""
    if stream_safe(codes, thr):
        return patchwork(seed, n)
    op = O.Params.make(bl, bpf, codes, thr)
    quiet = tuple(a for a in AMPS if a <= 21 or 100 <= a <= 1000)
    for k in range(64):
        w = patchwork(seed + 1000 * k, n, amps=quiet)
        if O.encode(w, op)[0] == 0:
            return w
    raise AssertionError("no encodable content for %s %s" % (codes, thr))


class _opts:
    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        self.old = {k: self.ctx.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)


_POISON = {}


def poison(ctx, x3, want):
    """run a decode on a kernel other than `want`, so that decode_kernel_in_use cannot report a kernel of an earlier call"""
    other = 0 if want else 1
    if other not in _POISON:
        codes = (2, 1, 3) if other == 0 else (0, 0, 0)
        p = x3.Params.make(20, 100, codes, (3, 8, 20) if other == 0 else (2, 4, 6))
        _POISON[other] = (p, O.encode(patchwork(7, 900), oparams(p))[1])
    p, s = _POISON[other]
    with _opts(ctx, {"decode_single": 1}):
        ctx.decode_stream(s, p, wav_cap=1000)
    assert ctx.get_option("decode_kernel_in_use") == other


def same(a, o, what):
    assert (a[0], a[2], a[3]) == (o[0], o[2], o[3]), (what, a[0], a[2:], o[0], o[2:])
    assert np.array_equal(a[1], o[1]), what


def edge_frames(bl):
    """one-block frames of a Rice block whose codeword at position 0, bl // 2 or bl - 1 has z = 0 .. 33 zeros (sub-bits all
    ones or all zeros), every other codeword the smallest index: each type's index bound, and the 32-bit run limit, from both
    sides -- the oracle says which are OutOfBoundsInverse (decoder.rs:147-196); the payload holds every bit the block reads"""
    small = {1: "1", 2: "10", 3: "1000"}
    frames = []
    for ft in (1, 2, 3):
        for z in range(34):
            for sub in ("0", "1"):
                for at in sorted({0, bl // 2, bl - 1}):
                    edge = "0" * z + "1" + sub * (0, 0, 1, 3)[ft]
                    bits = format(ft, "02b") + "".join(edge if j == at else small[ft] for j in range(bl))
                    bits += "0" * (-len(bits) % 8)
                    body = np.array([int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)], dtype=np.uint8)
                    pay = np.concatenate([np.array([0x12, 0x34], dtype=np.uint8), body, np.zeros(8, dtype=np.uint8)])
                    frames.append((pay, 1 + bl))
    return frames


# ------------------------------------------------------------------ encoders

@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_encoders(ctx, x3, codes, thr):
    """every generation (wave encoder, second generation, the general kernel, two passes) on whole frames and ragged
    tails, start_pos 0 and odd; x3_encode_batch with ragged clips; x3_encode_frames_dev (frames from a table)"""
    for bl, bpf in GEOMS:
        p, po = x3.Params.make(bl, bpf, codes, thr), O.Params.make(bl, bpf, codes, thr)
        assert x3.lib().x3_params_validate(C.byref(p)) == 0
        spf = bl * bpf
        for k, n in enumerate((40 * spf, 61 * spf + spf // 3 + 1, spf // 2 + 3, 333 * spf + 2 * bl + 1)):
            wav = content(codes, thr, bl, bpf, 31 * bl + k, n)
            for sp in (0, 7):
                rc_o, so, st_o = O.encode(wav, po, start_pos=sp)
                assert rc_o == 0
                for gen, two_pass in ((3, 0), (2, 0), (3, 1)):
                    ctx.set_option("enc_gen", gen)   # (also forgets what earlier calls said about dense content)
                    with _opts(ctx, {"two_pass": two_pass}):
                        rc, s, st = ctx.encode(wav, p, start_pos=sp)
                        used = ctx.get_option("enc_gen_in_use")
                    what = (bl, bpf, n, sp, gen, two_pass)
                    assert rc == rc_o, (what, rc, ctx.last_error())
                    assert used == expected_gen(codes, thr, bl, bpf, n, gen, two_pass), (what, used)
                    assert s.size == so.size and np.array_equal(s[sp:], so[sp:]), \
                        (what, int(np.argmax(s[sp:so.size] != so[sp:s.size])) + sp)
                    assert st.tolist() == st_o.tolist(), what
        ctx.set_option("enc_gen", 3)
        # clips of different lengths in one call
        lens = [2 * spf + 1, 5, spf, 1, 3 * spf + 2 * bl + 3, 2 * spf + 1, spf - 1]
        clips = [content(codes, thr, bl, bpf, 7 * i + bl, ln) for i, ln in enumerate(lens)]
        for gen in (3, 2):
            ctx.set_option("enc_gen", gen)
            rc, out, offs, st = ctx.encode_batch(clips, p)
            assert rc == 0, ctx.last_error()
            tot = np.zeros(6, dtype=np.uint64)
            for i, cl in enumerate(clips):
                rc_o, so, st_o = O.encode(cl, po)
                assert rc_o == 0 and np.array_equal(out[offs[i]:offs[i + 1]], so), (bl, gen, i, len(cl))
                tot += st_o
            assert st.tolist() == tot.tolist(), (bl, gen)
        # frames from a table (the TAB instantiations)
        rng = np.random.default_rng(bl + sum(codes) + 10 * thr[2])
        wav = content(codes, thr, bl, bpf, 5 + bl, 20 * spf)
        F = 60
        src_n = rng.integers(1, spf + 1, size=F).astype(np.uint32)
        src_n[::5] = spf
        src_off = (rng.integers(0, wav.size - spf, size=F) & ~1).astype(np.uint64)
        for f in range(F):   # (past the edge: frames whose content the reference can encode)
            while O.encode(wav[int(src_off[f]):int(src_off[f]) + int(src_n[f])], po)[0]:
                src_off[f] = int(rng.integers(0, wav.size - spf)) & ~1
        cap = int(sum(20 + 2 * int(m) + (int(m) // bl + 1) + 4 for m in src_n)) + 64
        d_wav, d_out, d_off = ctx.alloc(2 * wav.size), ctx.alloc(cap), ctx.alloc(8 * (F + 1))
        try:
            ctx.upload(d_wav, wav)
            for gen in (3, 2):
                ctx.set_option("enc_gen", gen)
                assert ctx.encode_frames_dev(d_wav, src_off, src_n, p, d_out, cap, d_frame_offsets=d_off) == 0
                rc, pos, _ = ctx.encode_result()
                assert rc == 0, ctx.last_error()
                assert ctx.get_option("enc_gen_in_use") == expected_gen(codes, thr, bl, bpf, spf, gen, 0), (bl, gen)
                got = ctx.download(d_out, pos, np.uint8)
                offs = ctx.download(d_off, 8 * (F + 1), np.uint64)
                for f in range(F):
                    rc_o, so, _ = O.encode(wav[int(src_off[f]):int(src_off[f]) + int(src_n[f])], po)
                    assert rc_o == 0
                    assert np.array_equal(got[int(offs[f]):int(offs[f]) + so.size], so), (bl, gen, f, int(src_n[f]))
        finally:
            ctx.set_option("enc_gen", 3)
            for d in (d_wav, d_out, d_off):
                ctx.free(d)


# ------------------------------------------------------------------ decoders

def _walks(ctx, stream, p, cap, o, replays=None):
    """x3_decode_stream with the walk on the host, on the GPU, and in chunks of three frames; `replays`: the frames all of
    them hand to the reference's reader (the chunked walk stops after the chunk of the first failing frame: there only when
    that is none)"""
    for host_walk, chunk in ((1, -1), (0, -1), (-1, 3)):
        with _opts(ctx, {"host_walk": host_walk, "host_chunk_frames": chunk}):
            same(ctx.decode_stream(stream, p, wav_cap=cap), o, ("walk", host_walk, chunk))
            if replays is not None and (chunk < 0 or replays == 0):
                assert ctx.get_option("last_decode_replays") == replays, ("walk", host_walk, chunk)


def _per_frame(ctx, x3, stream, p, x4):
    """x3_decode_dev over every frame of an intact stream (caller's frame and sample offsets, per-frame statuses) against
    the oracle's decode_frame of each: statuses, samples of the good frames, the 0x5A guard behind every row"""
    offs = frame_offsets(stream)
    F = len(offs)
    ns = [int(stream[o + 4]) << 8 | int(stream[o + 5]) for o in offs]
    gap = 8                                               # (samples of guard behind every row; multiples of four apart)
    wo = np.cumsum([0] + [m + gap + (-(m + gap)) % 4 for m in ns])
    total = int(wo[-1]) + 64
    d_x3, d_off, d_wo = ctx.alloc(stream.size + 64), ctx.alloc(8 * (F + 1)), ctx.alloc(8 * F)
    d_wav, d_st = ctx.alloc(2 * total), ctx.alloc(4 * F)
    try:
        ctx.upload(d_x3, np.concatenate([stream, np.zeros(64, dtype=np.uint8)]))
        ctx.upload(d_off, np.array(offs + [stream.size], dtype=np.uint64))
        ctx.upload(d_wo, wo[:F].astype(np.uint64))
        ctx.upload(d_wav, np.full(total, 0x5A5A, dtype=np.int16))
        with _opts(ctx, {"wav_offsets_x4": x4}):
            assert ctx.decode_dev(d_x3, stream.size, d_off, F, p, d_wav, total, d_wav_offsets=d_wo, d_status=d_st) == 0
        rc, first_bad, st0, before = ctx.decode_result()
        assert rc == 0
        replays = ctx.get_option("last_decode_replays")
        status = ctx.download(d_st, 4 * F, np.int32)
        wav = ctx.download(d_wav, 2 * total, np.int16)
    finally:
        for d in (d_x3, d_off, d_wo, d_wav, d_st):
            ctx.free(d)
    op = oparams(p)
    assert replays == not_plain(walked_frames(stream, total), op), (x4, replays)
    exp_first = F
    for f, o in enumerate(offs):
        plen = int(stream[o + 6]) << 8 | int(stream[o + 7])
        rc_o, w_o = O.decode_frame(stream[o + 20:o + 20 + plen], ns[f], op)
        assert status[f] == rc_o, (f, int(status[f]), rc_o)
        if rc_o == 0:
            a = int(wo[f])
            assert np.array_equal(wav[a:a + ns[f]], w_o), f
            assert (wav[a + ns[f]:a + ns[f] + gap] == 0x5A5A).all(), f
        elif exp_first == F:
            exp_first = f
    assert first_bad == exp_first
    return status


@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_decoders(ctx, x3, codes, thr):
    """the oracle's stream, damaged copies with refreshed CRCs and crafted frames through every decoder kernel that takes
    them; x3_decode_stream (three walks), x3_decode_dev frame by frame, x3_decode_stream_dev"""
    rng = np.random.default_rng(sum(codes) * 1000 + thr[0] * 100 + thr[1] * 10 + thr[2])
    for bl, bpf in GEOMS:
        p, po = x3.Params.make(bl, bpf, codes, thr), O.Params.make(bl, bpf, codes, thr)
        spf = bl * bpf
        n = 201 * spf + spf // 3 + 1
        wav = content(codes, thr, bl, bpf, 11 * bl + 3, n)
        rc, stream, _ = O.encode(wav, po)
        assert rc == 0
        offs = frame_offsets(stream)
        cases = [stream] + [damage(rng, stream, offs) for _ in range(10)]
        cap = n + 70000
        want = {o: O.decode_stream(s, po, wav_cap=cap) for o, s in enumerate(cases)}
        if codes == (0, 1, 3) and thr[2] >= 16:
            assert want[0][0] == 0 and np.array_equal(want[0][1], wav)
        frames = crafted_frames(x3, rng, p, 1000) + edge_frames(bl)
        # the frames each case's decode launch hands to the reference's reader (none on a stream of the default codes)
        replays = [not_plain(walked_frames(s, cap), po) for s in cases]
        if codes == (0, 1, 3) and thr[2] >= 16:
            assert replays[0] == 0
        for name, kv in DECODERS:
            with _opts(ctx, kv):
                eff = [ctx.get_option(k) for k in OPTS]
                exp = expected_kernel(codes, bl, *eff)
                cell = COVER.setdefault((codes, thr, bl, name), set())
                for i, s in enumerate(cases):
                    if i == 0:
                        poison(ctx, x3, exp)
                    same(ctx.decode_stream(s, p, wav_cap=cap), want[i], (bl, name, i))
                    assert ctx.get_option("last_decode_replays") == replays[i], (bl, name, i, replays[i])
                    if i == 0:
                        used = ctx.get_option("decode_kernel_in_use")
                        assert used == exp, (bl, name, used, exp)
                        cell.add(used)
                for mode in ("batch", "offsets", "offsets_x4"):
                    poison(ctx, x3, exp if mode != "offsets" else expected_kernel(codes, bl, 0, 1, 1))
                    compare(x3, ctx, p, frames, mode)
                    used = ctx.get_option("decode_kernel_in_use")
                    assert used == (exp if mode != "offsets" else expected_kernel(codes, bl, 0, 1, 1)), (bl, name, mode, used)
                    cell.add(used)
                for x4 in (1, 0):
                    _per_frame(ctx, x3, stream, p, x4)
        _walks(ctx, stream, p, cap, want[0], replays[0])
        _walks(ctx, cases[1], p, cap, want[1])
        # a device-resident stream in one trip (block length 20) or two
        d_wav = ctx.alloc(2 * cap)
        try:
            for i, s in enumerate(cases):
                d = ctx.alloc(s.size + 64)
                ctx.upload(d, np.concatenate([s, np.zeros(64, dtype=np.uint8)]))
                b = ctx.decode_stream_dev(d, s.size, p, d_wav, cap)
                ctx.free(d)
                assert ctx.get_option("last_decode_replays") == replays[i], (bl, i, replays[i])
                o = want[i]
                assert b == (o[0], o[1].size, o[2], o[3]), (bl, i, b, o[0], o[1].size, o[2:])
                assert np.array_equal(ctx.download(d_wav, 2 * b[1], np.int16), o[1]), (bl, i)
        finally:
            ctx.free(d_wav)
    # this parameter set's row of the coverage table
    for bl, _ in GEOMS:
        for name, _ in DECODERS:
            assert COVER[(codes, thr, bl, name)], (bl, name)


def test_coverage_table_is_filled():
    """every (parameter set, block length, decoder setting) cell ran, and every kernel the routing table names was hit:
    3 and 2 for codes (0|1, 1, 3), 1 for other codes with codes[0] in {0, 1}, 0 for codes[0] in {2, 3}"""
    if len({k[:2] for k in COVER}) < len(PSETS):
        pytest.skip("the decoder matrix did not run in full (-k?)")
    seen = {}
    for (codes, thr, bl, name), kernels in COVER.items():
        assert kernels, (codes, thr, bl, name)
        cls = "fast" if codes[0] in (0, 1) and codes[1:] == (1, 3) else ("k0<2" if codes[0] in (0, 1) else "k0>=2")
        seen.setdefault((cls, bl), set()).update(kernels)
    for bl, _ in GEOMS:
        assert seen[("k0>=2", bl)] == {0}, bl
        assert seen[("k0<2", bl)] == {1}, bl
        assert seen[("fast", bl)] == {20: {1, 2, 3}, 10: {1, 3}, 40: {1, 3}}.get(bl, {1}), (bl, seen[("fast", bl)])


# ------------------------------------------------------------------ the other decode entry points

def _ragged(x3, codes, thr, bl, bpf, seed):
    lens = [3 * bl * bpf + 7, 5, bl * bpf, 1, 2 * bl * bpf + bl + 3, 777]
    clips = [content(codes, thr, bl, bpf, seed + i, m) for i, m in enumerate(lens)]
    po = O.Params.make(bl, bpf, codes, thr)
    return [O.encode(c, po)[1] for c in clips]


@pytest.mark.parametrize("codes,thr", [s for s in PSETS if s[0] in ((0, 1, 3), (1, 1, 3))][:4] +
                         [s for s in PSETS if s[0] in ((2, 1, 3), (0, 0, 0), (1, 2, 3))])
def test_decode_dev_batch_of_ragged_clips(ctx, x3, codes, thr):
    """x3_decode_dev on the frames of clips of different lengths, one after the other (sample offsets from the caller,
    with and without the promise that they are multiples of four)"""
    for bl, bpf in GEOMS:
        p = x3.Params.make(bl, bpf, codes, thr)
        stream = np.concatenate(_ragged(x3, codes, thr, bl, bpf, 100 + bl))
        for x4 in (1, 0):
            _per_frame(ctx, x3, stream, p, x4)


@pytest.mark.parametrize("codes,thr", [((1, 1, 3), (3, 8, 20)), ((1, 1, 3), (9, 4, 20)), ((0, 1, 3), (3, 8, 20))])
def test_decode_by_the_encoders_segment_index(ctx, x3, codes, thr):
    """x3_decode_dev_seg driven by the index the wave encoder wrote: where the encoder's blocks begin is not where the
    decoder's parse of a (1, 1, 3) stream puts them, so the index is a hint that is wrong on real data"""
    bl, bpf, sb = 20, 100, 8
    p = x3.Params.make(bl, bpf, codes, thr)
    po = oparams(p)
    L = x3.lib()
    n = 97 * bl * bpf + 1234
    wav = content(codes, thr, bl, bpf, 4321, n)
    F = L.x3_num_frames(n, C.byref(p))
    cap = L.x3_encode_bound(n, C.byref(p))
    ne = L.x3_seg_index_entries(F, C.byref(p), sb)
    assert ne > F
    d_wav, d_x3, d_off = ctx.alloc(2 * n + 64), ctx.alloc(cap + 64), ctx.alloc(8 * (F + 1))
    d_seg, d_back, d_st = ctx.alloc(8 * ne), ctx.alloc(2 * n + 64), ctx.alloc(4 * F)
    try:
        ctx.upload(d_wav, wav)
        ctx.set_option("enc_gen", 3)
        assert ctx.encode_dev_seg(d_wav, n, p, d_x3, cap, d_seg, sb, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0 and ctx.get_option("enc_gen_in_use") == 3
        stream = ctx.download(d_x3, pos, np.uint8)
        assert np.array_equal(stream, O.encode(wav, po)[1])
        assert int(ctx.download(d_seg, 8, np.uint64)[0]) == (sb << 32) | 0x58335347   # (the encoder wrote an index)
        offs = frame_offsets(stream)
        exp_first = F
        verdicts = []
        for f, o in enumerate(offs):
            ns = int(stream[o + 4]) << 8 | int(stream[o + 5])
            plen = int(stream[o + 6]) << 8 | int(stream[o + 7])
            verdicts.append(O.decode_frame(stream[o + 20:o + 20 + plen], ns, po))
            if verdicts[-1][0] and exp_first == F:
                exp_first = f
        for stretches in (0, 2, 5):
            ctx.set_option("seg_stretches", stretches)
            ctx.upload(d_back, np.full(n + 32, 0x5A5A, dtype=np.int16))
            assert ctx.decode_dev_seg(d_x3, pos, d_off, F, p, d_back, n, d_seg, sb, record=False, n_per_clip=n,
                                      d_status=d_st) == 0
            rc, first_bad, st0, before = ctx.decode_result()
            assert rc == 0 and first_bad == exp_first, (stretches, first_bad, exp_first)
            assert ctx.get_option("decode_kernel_in_use") == 2 and ctx.get_option("last_seg_stretches") >= 2
            status = ctx.download(d_st, 4 * F, np.int32)
            back = ctx.download(d_back, 2 * (n + 32), np.int16)
            for f, (rc_o, w_o) in enumerate(verdicts):
                assert status[f] == rc_o, (stretches, f, int(status[f]), rc_o)
                if rc_o == 0:
                    assert np.array_equal(back[f * bl * bpf:f * bl * bpf + w_o.size], w_o), (stretches, f)
            assert (back[n:n + 32] == 0x5A5A).all()
    finally:
        ctx.set_option("seg_stretches", 0)
        for d in (d_wav, d_x3, d_off, d_seg, d_back, d_st):
            ctx.free(d)


def _expected_window(frames, so, s, L):
    row = np.zeros(L, dtype=np.int16)
    f = int(np.searchsorted(so, s, side="right")) - 1
    while f < len(frames) and int(so[f]) < s + L:
        st, w = frames[f]
        if st:
            return row, st
        a, b = int(so[f]), int(so[f + 1])
        lo, hi = max(a, s), min(b, s + L)
        row[lo - s:hi - s] = w[lo - a:hi - a]
        f += 1
    return row, 0


@pytest.mark.parametrize("codes", [(1, 1, 3), (2, 1, 3), (3, 1, 3)])
@pytest.mark.parametrize("sb", [32, 0])
def test_windows(ctx, x3, codes, sb):
    """WindowSource with a recorded index (32 blocks a stretch) and without; (2, 1, 3) and (3, 1, 3) give type-1 zero
    runs of 32 bits and more, which the window decoder leaves to the reference's reader"""
    bl, bpf = 20, 200
    p = x3.Params.make(bl, bpf, codes, (3, 8, 20))
    po = oparams(p)
    wav = patchwork(sb + sum(codes), 45 * bl * bpf + 321)
    stream = O.encode(wav, po)[1]
    # sparse garbage frames spliced in: long zero runs inside type-1 blocks, valid headers and CRCs
    rng = np.random.default_rng(len(stream))
    extra = []
    for pay, m in crafted_frames(x3, rng, p, 40):
        if pay.size & 1:
            pay = np.concatenate([pay, np.zeros(1, dtype=np.uint8)])
        extra.append(np.concatenate([x3.write_frame_header(m, 1, pay.size, O.crc16(pay)), pay]))
    offs = frame_offsets(stream)
    stream = np.concatenate([stream[:offs[20]]] + extra + [stream[offs[20]:]])
    offs = frame_offsets(stream)
    frames, so = [], [0]
    for o in offs:
        m = int(stream[o + 4]) << 8 | int(stream[o + 5])
        plen = int(stream[o + 6]) << 8 | int(stream[o + 7])
        rc, w = O.decode_frame(stream[o + 20:o + 20 + plen], m, po)
        frames.append((rc, w if rc == 0 else None))
        so.append(so[-1] + m)
    so = np.array(so, dtype=np.uint64)
    total = int(so[-1])
    src = x3.WindowSource(ctx, stream, p, seg_blocks=sb)
    try:
        assert src.n_frames == len(offs) and src.total == total
        for L in (1, 37, 2000, 9000):
            starts = sorted({0, total - L, int(so[20]), int(so[21]) - 3, int(so[40]) + 5} |
                            {int(v) for v in rng.integers(0, total - L + 1, 6)})
            for fmt in (0, 1):
                rows, st = src.decode(starts, L, fmt)
                for r, s0, got in zip(rows, starts, st):
                    want, wst = _expected_window(frames, so, s0, L)
                    assert got == wst, (L, s0, int(got), wst)
                    if fmt:
                        assert np.array_equal(r.view(np.uint32),
                                              (want.astype(np.float32) / np.float32(32768.0)).view(np.uint32)), (L, s0)
                    else:
                        assert np.array_equal(r, want), (L, s0)
    finally:
        src.close()


@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_decode_frame_and_reader(ctx, x3, codes, thr):
    """x3_decode_frame frame by frame (with and without x3_decode_prefetch) on a bare stream, and x3_reader_* on the same
    frames behind an archive header that carries the parameters"""
    bl, bpf = 20, 100
    p = x3.Params.make(bl, bpf, codes, thr)
    po = oparams(p)
    wav = content(codes, thr, bl, bpf, 99, 23 * bl * bpf + 17)
    stream = O.encode(wav, po)[1]
    rng = np.random.default_rng(sum(thr))
    s = np.ascontiguousarray(damage(rng, stream, frame_offsets(stream)))
    for data in (stream, s):
        for pre in (False, True):
            if pre:
                assert ctx.decode_prefetch(data, p) == 0
            try:
                for o in frame_offsets(data):
                    m = int(data[o + 4]) << 8 | int(data[o + 5])
                    plen = int(data[o + 6]) << 8 | int(data[o + 7])
                    if m == 0 or o + 20 + plen > data.size:
                        continue
                    pay = data[o + 20:o + 20 + plen]
                    r_o = O.decode_frame(pay, m, po)
                    r_g = ctx.decode_frame(pay, m, p)
                    assert r_g[0] == r_o[0], (pre, o, r_g[0], r_o[0])
                    assert r_o[0] != 0 or np.array_equal(r_g[1], r_o[1]), (pre, o)
            finally:
                if pre:
                    ctx.decode_prefetch(None)
        rc, hdr = O.archive_header_write(16000, po)
        assert rc == 0
        arch = np.concatenate([hdr, data])
        r_o = O.x3a_decode(arch, wav_cap=wav.size + 70000)
        r = x3.Reader(ctx, arch)
        try:
            assert r.rc == 0 and tuple(r.spec()[1].codes) == codes and tuple(r.spec()[1].thresholds) == thr
            out = []
            while True:
                rc, smp = r.next_frame()
                if rc or smp is None:
                    break
                out.append(smp)
            got = np.concatenate(out) if out else np.zeros(0, dtype=np.int16)
            assert (rc, r.frame_errors()) == (r_o[0], r_o[4]), (rc, r.frame_errors(), r_o[0], r_o[4])
            assert np.array_equal(got, r_o[1])
        finally:
            r.close()
