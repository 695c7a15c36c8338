"""The 9 728-byte edge on the GPU: payloads of exactly 9 726, 9 728 and 9 730 bytes, every bit count of them, every row
boundary of the wave encoder's image (38 rows of 256 bytes), a full image in half-empty lanes, and blocks of 10 and 40 --
frames built bit for bit by payload_cases.py (test_payload_cases.py holds them against the oracle without a GPU).

The edge is shared by the wave encoder (x3_encode_wave_kernel.h: `ovf = L > X3W_IMG_BYTES` decides between emitting into
the image and the dense pass behind it), the second generation (x3_encode_stream2_kernel.h: the count behind the hint that
moves a context between the generations) and the three-wave and block-per-lane decoders (`dense_grp`: how far ahead a
group of 64 frames requests its ring).  Everything is compared with == against the oracle: stream bytes, frame offsets,
statistics, decoded samples, statuses, and the number of dense frames against the oracle's headers."""
import ctypes as C

import numpy as np
import pytest

import levels_ref as R
import oracle_lib as O
import payload_cases as PC

pytestmark = pytest.mark.gpu

STREAM_SPECS = PC.stream_specs()
GROUP_SPECS = PC.group_specs()
SEG_BLOCKS = 64
# (name, options, enc_gen_in_use)
ENCODERS = (("wave", {"enc_gen": 3, "two_pass": 0}, 3), ("second generation", {"enc_gen": 2, "two_pass": 0}, 2),
            ("two-pass", {"enc_gen": 3, "two_pass": 1}, 0))


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _params(x3, spec):
    return x3.Params.make(spec.block_len, spec.blocks_per_frame)


def _dense(plens):
    return sum(L > PC.IMAGE_BYTES for L in plens)


def _positions(x3_bytes, start):
    """byte offsets of the frames of an oracle stream whose first header is at `start`, and the stream's end"""
    offs, pos = [], start
    while pos < x3_bytes.size:
        offs.append(pos)
        pos += 20 + (int(x3_bytes[pos + 6]) << 8 | int(x3_bytes[pos + 7]))
    assert pos == x3_bytes.size
    return offs + [pos]


class _Bufs:
    """device buffers of one test, freed together"""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def alloc(self, n):
        p = self.ctx.alloc(n)
        self.all.append(p)
        return p

    def up(self, arr, extra=64):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes + extra)
        self.ctx.upload(p, arr)
        return p

    def close(self):
        for p in self.all:
            self.ctx.free(p)
        self.all = []


# ------------------------------------------------------------------ encoders

def _expectations(b):
    """the oracle's answers for every encoder call of one spec:
    {call: (start_pos, stream bytes incl. the prefix, frame offsets, statistics, payload lengths)}"""
    spec, po = b.spec, b.spec.oparams
    spf, F = spec.spf, len(b.frames)
    out = {"stream@0": (0, b.x3, list(b.offsets), list(b.stats), list(b.plens))}
    rc, s, st = O.encode(b.wav, po, start_pos=321)
    assert rc == 0 and np.array_equal(s[322:], b.x3)
    out["stream@321"] = (321, s, _positions(s, 322), st.tolist(), list(b.plens))
    nfull = sum(f.size == spf for f in b.frames)
    rc, s, st = O.encode(b.wav[:nfull * spf], po)
    assert rc == 0
    out["clips"] = (0, s, _positions(s, 0), st.tolist(), list(b.plens[:nfull]))
    if nfull < F:   # a short last frame: three clips of it
        rc, s, st = O.encode(b.frames[-1], po)
        assert rc == 0 and s.size == 20 + b.plens[-1]
        out["short clips"] = (0, np.concatenate([s] * 3), [0, s.size, 2 * s.size, 3 * s.size], (3 * st).tolist(), [b.plens[-1]] * 3)
    rev = [b.x3[b.offsets[f]:b.offsets[f + 1]] for f in reversed(range(F))]
    s = np.concatenate(rev)
    out["table"] = (0, s, _positions(s, 0), list(b.stats), list(reversed(b.plens)))
    return out


@pytest.mark.parametrize("spec", STREAM_SPECS, ids=[s.name for s in STREAM_SPECS])
def test_encoders_at_the_image_edge(ctx, x3, spec):
    """the stream from start positions 0 and 321, as a batch of equal clips at two strides, as a table of frames in
    reversed order and with the segment index, through the wave encoder (and its dense pass), the second generation
    and the two-pass kernels: bytes, frame offsets and statistics are the oracle's, the count of dense frames is the
    number of oracle headers with payload_len > 9 728, and no call is encoded twice"""
    b = PC.built(spec)
    p, L = _params(x3, spec), x3.lib()
    want = _expectations(b)
    spf, F, n = spec.spf, len(b.frames), b.wav.size
    nfull = sum(f.size == spf for f in b.frames)
    starts = np.arange(F, dtype=np.uint64) * np.uint64(spf)
    bufs = _Bufs(ctx)
    try:
        d_wav = bufs.up(b.wav)
        cap = int(L.x3_encode_bound(n, C.byref(p))) + 3 * int(L.x3_encode_bound(spf, C.byref(p))) + 321 + 64
        d_out, d_off = bufs.alloc(cap + 16), bufs.alloc(8 * (F + 4))
        # the clips: whole frames side by side, and three copies of a short last frame (strides: multiples of four samples)
        clips = {}
        for extra in (0, 4):
            lay = np.full((nfull, spf + extra), 0x5A5A, dtype=np.int16)
            lay[:, :spf] = b.wav[:nfull * spf].reshape(nfull, spf)
            clips["clips", extra] = (bufs.up(lay), spf, nfull, spf + extra)
            if nfull < F:
                ns = b.frames[-1].size
                stride = ((ns + 3) & ~3) + extra
                lay = np.full((3, stride), 0x5A5A, dtype=np.int16)
                lay[:, :ns] = b.frames[-1]
                clips["short clips", extra] = (bufs.up(lay), ns, 3, stride)
        # the segment index a recording decode of the oracle's stream leaves (blocks of 20: the three-wave decoder's)
        ne = int(L.x3_seg_index_entries(F, C.byref(p), SEG_BLOCKS))
        assert ne == 1 + F * ((spec.blocks_per_frame + SEG_BLOCKS - 1) // SEG_BLOCKS - 1)
        d_seg = bufs.alloc(8 * ne)
        recorded = None
        if spec.block_len == 20:
            d_x3, d_xoff, d_back, d_rec = bufs.up(b.x3), bufs.up(np.array(b.offsets, dtype=np.uint64)), bufs.alloc(2 * n + 64), bufs.alloc(8 * ne)
            assert ctx.decode_dev_seg(d_x3, b.x3.size, d_xoff, F, p, d_back, n, d_rec, SEG_BLOCKS, record=True, n_per_clip=n) == 0
            assert ctx.decode_result() == (0, F, 0, n)
            recorded = ctx.download(d_rec, 8 * ne, np.uint64)
            assert int(recorded[0]) == (SEG_BLOCKS << 32) | 0x58335347

        def run(what, key, call, n_frames):
            start, s_o, offs_o, st_o, plens = want[key]
            ctx.upload(d_out, np.full(cap, 0xA5, dtype=np.uint8))
            assert call(start) == 0, (what, ctx.last_error())
            rc, pos, st = ctx.encode_result()
            used, dense = ctx.get_option("enc_gen_in_use"), ctx.get_option("last_dense_frames")
            print(spec.name, what, "rc", rc, "pos", pos, "want", s_o.size, "enc_gen_in_use", used, "last_dense_frames", dense,
                  "want", _dense(plens))
            assert rc == 0 and pos == s_o.size, (what, rc, pos, s_o.size)
            got = ctx.download(d_out, pos)
            assert (got[:start] == 0xA5).all(), (what, "bytes in front of start_pos were written")
            bad = np.flatnonzero(got[start:] != s_o[start:])
            assert bad.size == 0, (what, "first differing byte", start + int(bad[0]))
            assert ctx.download(d_off, 8 * (n_frames + 1), np.uint64).tolist() == offs_o, what
            assert st.tolist() == st_o, what
            assert used == gen, (what, used)
            if gen in (3, 2):   # (either single-pass generation counts them: `L > 9728` in both kernels)
                assert dense == _dense(plens), (what, dense, _dense(plens), plens)

        for name, opts, gen in ENCODERS:
            for k, v in opts.items():
                ctx.set_option(k, v)      # (setting enc_gen also forgets what earlier calls said about dense content)
            forget = lambda: ctx.set_option("enc_gen", opts["enc_gen"])
            for key in ("stream@0", "stream@321"):
                forget()
                run((name, key), key, lambda sp: ctx.encode_dev(d_wav, n, p, d_out, cap, sp, d_off), F)
            for (key, extra), (d_clips, npc, ncl, stride) in clips.items():
                forget()
                run((name, key, stride), key,
                    lambda sp: ctx.encode_dev(d_clips, npc, p, d_out, cap, sp, d_off, n_clips=ncl, clip_stride=stride), ncl)
            forget()
            run((name, "table"), "table",
                lambda sp: ctx.encode_frames_dev(d_wav, starts[::-1], [f.size for f in reversed(b.frames)], p, d_out, cap, sp, d_off), F)
            forget()
            ctx.upload(d_seg, np.full(ne, 0xDEADBEEFDEADBEEF, dtype=np.uint64))
            run((name, "segment index"), "stream@0",
                lambda sp: ctx.encode_dev_seg(d_wav, n, p, d_out, cap, d_seg, SEG_BLOCKS, sp, d_off), F)
            seg = ctx.download(d_seg, 8 * ne, np.uint64)
            if gen == 3 and recorded is not None:
                assert np.array_equal(seg, recorded), (name, np.flatnonzero(seg != recorded)[:8])
            else:               # (only the wave encoder on blocks of 20 fills it: any other says "no index")
                assert int(seg[0]) == 0, (name, hex(int(seg[0])))
        assert ctx.get_option("encode_dense_reruns") == 0 and ctx.get_option("encode_fallbacks") == 0
    finally:
        ctx.set_option("two_pass", 0)
        ctx.set_option("enc_gen", 3)
        bufs.close()


def test_the_dense_hint_turns_at_9730_bytes(ctx, x3):
    """A call whose frames are all 9 728 bytes (the image full to its last bit) leaves the context on the wave encoder; a
    call whose frames are all 9 730 bytes moves the NEXT call to the second generation, which counts none in 9 728-byte
    frames and hands the context back (the pattern of test_wave_encoder_dense_hint_is_only_a_hint)."""
    po, p = O.Params.default(), x3.Params.default()
    full = PC.stream([PC.FrameSpec(77809 + i, 10000, PC.ARRANGEMENTS[i % 5], 900 + i) for i in range(16)], po)[0]
    over = PC.stream([PC.FrameSpec(77825 + i, 10000, PC.ARRANGEMENTS[i % 5], 950 + i) for i in range(16)], po)[0]
    bufs = _Bufs(ctx)
    try:
        cap = int(x3.lib().x3_encode_bound(full.size, C.byref(p)))
        d_out, d_wav = bufs.alloc(cap + 16), bufs.alloc(2 * full.size + 64)
        for i, (wav, gen, dense) in enumerate(((full, 3, 0), (full, 3, 0), (over, 3, 16), (full, 2, 0), (full, 3, 0), (over, 3, 16),
                                               (over, 2, 16), (full, 2, 0), (full, 3, 0))):
            rc_o, s_o, st_o = O.encode(wav, po)
            assert rc_o == 0 and {int(s_o[k + 6]) << 8 | int(s_o[k + 7]) for k in _positions(s_o, 0)[:-1]} == {9730 if dense else 9728}
            ctx.upload(d_wav, wav)
            assert ctx.encode_dev(d_wav, wav.size, p, d_out, cap, 0) == 0
            rc, pos, st = ctx.encode_result()
            used, counted = ctx.get_option("enc_gen_in_use"), ctx.get_option("last_dense_frames")
            print("call", i, "enc_gen_in_use", used, "want", gen, "last_dense_frames", counted, "want", dense)
            assert rc == 0 and pos == s_o.size and np.array_equal(ctx.download(d_out, pos), s_o) and st.tolist() == st_o.tolist()
            assert used == gen, (i, used, gen)
            assert counted == dense, (i, counted, dense)
        assert ctx.get_option("encode_dense_reruns") == 0 and ctx.get_option("encode_fallbacks") == 0
    finally:
        bufs.close()


# ------------------------------------------------------------------ decoders

@pytest.mark.parametrize("spec", STREAM_SPECS + GROUP_SPECS, ids=[s.name for s in STREAM_SPECS + GROUP_SPECS])
def test_decoders_at_the_image_edge(ctx, x3, spec):
    """the oracle's stream through the three-wave kernel (caller's sample offsets, multiples of four), the block-per-lane
    kernel, the single-wave kernels and x3_decode_stream_dev: the samples, status 0 for every frame, and no frame handed
    to the reference's reader.  The two group specs are 64 + 64 frames of 9 728 bytes -- no group dense, the late
    requests carry the most they ever do -- and the same with one frame of 9 730 bytes in each group, which makes both
    groups dense."""
    b = PC.built(spec)
    p = _params(x3, spec)
    F, n, bl = len(b.frames), b.wav.size, spec.block_len
    sample_at = np.arange(F, dtype=np.uint64) * np.uint64(spec.spf)
    bufs = _Bufs(ctx)
    names = ("wav_offsets_x4", "decode_blocks", "decode_single", "decode_blocks_off")
    try:
        d_x3 = bufs.up(np.concatenate([b.x3, np.zeros(64, dtype=np.uint8)]), 0)
        d_off, d_wo = bufs.up(np.array(b.offsets, dtype=np.uint64)), bufs.up(sample_at)
        d_back, d_st = bufs.alloc(2 * n + 64), bufs.alloc(4 * F)
        # (what, options, caller's sample offsets, decode_kernel_in_use: 2 three waves, 3 block per lane, 1 single wave)
        runs = [("three-wave", {"wav_offsets_x4": 1}, True, 2 if bl == 20 else 3),
                ("block-per-lane", {"decode_blocks": 1}, False, 3),
                ("single-wave", {"decode_single": 1}, False, 1),
                ("blocks off", {"decode_blocks_off": 1}, False, 2 if bl == 20 else 1)]
        for what, opts, by_offsets, kernel in runs:
            for k in names:
                ctx.set_option(k, opts.get(k, 0))
            ctx.upload(d_back, np.full(n + 32, 0x5A5A, dtype=np.int16))
            ctx.upload(d_st, np.full(F, -1, dtype=np.int32))
            if by_offsets:
                rc = ctx.decode_dev(d_x3, b.x3.size, d_off, F, p, d_back, n, d_wav_offsets=d_wo, d_status=d_st)
            else:
                rc = ctx.decode_dev(d_x3, b.x3.size, d_off, F, p, d_back, n, n_per_clip=n, d_status=d_st)
            assert rc == 0, (what, ctx.last_error())
            res = ctx.decode_result()
            used, replays = ctx.get_option("decode_kernel_in_use"), ctx.get_option("last_decode_replays")
            print(spec.name, what, "decode_kernel_in_use", used, "result", res, "replays", replays)
            assert res == (0, F, 0, n), (what, res)
            assert used == kernel, (what, used, kernel)
            back = ctx.download(d_back, 2 * n + 64, np.int16)
            bad = np.flatnonzero(back[:n] != b.wav)
            assert bad.size == 0, (what, "first differing sample", int(bad[0]), "frame", int(bad[0]) // spec.spf)
            assert (back[n:] == 0x5A5A).all(), (what, "samples written behind the stream's")
            assert not ctx.download(d_st, 4 * F, np.int32).any(), what
            assert replays == 0, (what, replays)
        for k in names:
            ctx.set_option(k, 0)
        ctx.upload(d_back, np.full(n + 32, 0x5A5A, dtype=np.int16))
        r = ctx.decode_stream_dev(d_x3, b.x3.size, p, d_back, n)
        used, replays = ctx.get_option("decode_kernel_in_use"), ctx.get_option("last_decode_replays")
        print(spec.name, "x3_decode_stream_dev", "decode_kernel_in_use", used, "result", r, "replays", replays)
        assert r == (0, n, F, 0), r
        assert used == (2 if bl == 20 else 3), used
        back = ctx.download(d_back, 2 * n + 64, np.int16)
        assert np.array_equal(back[:n], b.wav) and (back[n:] == 0x5A5A).all()
        assert replays == 0
    finally:
        for k in names:
            ctx.set_option(k, 0)
        bufs.close()


# ------------------------------------------------------------------ windows and levels: the same payloads through their rings

@pytest.mark.parametrize("seg_blocks", [32, 0])
def test_windows_and_levels_over_the_edge_frames(ctx, x3, seg_blocks):
    """x3_decode_windows_dev with windows of exactly one frame each and x3_levels_dev with bins of one frame over spec A,
    by a walk-built segment index and frame by frame"""
    b = PC.built(PC.spec_a())
    F, n = len(b.frames), b.wav.size
    ws = x3.WindowSource(ctx, b.x3, seg_blocks=seg_blocks, index="walk")
    try:
        assert (ws.n_frames, ws.total, ws.seg_blocks) == (F, n, seg_blocks)
        rows, st = ws.decode(np.arange(F, dtype=np.uint64) * np.uint64(10000), 10000)
        assert not st.any(), st
        bad = np.flatnonzero((rows != b.wav.reshape(F, 10000)).any(axis=1))
        assert bad.size == 0, ("windows differ", bad[:8])
        lv, fst = ws.levels(10000)
        assert lv.size == F and not fst.any()
        want = R.levels(b.frames, [0] * F, [10000 * f for f in range(F)], 10000, F)
        for k in R.LEVEL_DTYPE.names:
            assert np.array_equal(lv[k], want[k]), (k, np.flatnonzero(lv[k] != want[k])[:8])
    finally:
        ws.close()
