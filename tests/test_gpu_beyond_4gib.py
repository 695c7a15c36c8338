"""Device calls on a stream whose bytes AND sample positions pass 2^32 (include/x3hip.h promises 64-bit offsets, lengths and
positions everywhere; the kernels narrow to 32 bits relative to a frame, a group or an entry, which is right only where the
64-bit base was added in the right place).

The stream is tests/big_cases.py's: 6 921 places of 64 frames tiled on the device from four tiles that the CPU oracle
encodes, 5.1 GB and 4.43 G samples, with another tile at the place that holds byte 2^32, at the one that holds sample 2^32
and at the last one.  The reference is closed-form in the tiles (tests/test_big_cases.py proves it on the CPU); what is large
is compared on the device with torch.equal, what is small is downloaded.  One module-scoped fixture builds the stream; tests
that damage it flip the bits back.  Peak device memory stays below 40 GB: the large buffers of a test are freed before the
next one allocates.

Sections E2, E3 and F (the FIR, tone and tone bank forms of the levels, range levels and corpus calls) and S (the spectra
rows from a sample buffer of more than 2^32 elements and into an output of more than 2^32 words, the band levels into
planes past byte 2^33 and over the whole stream, plane events on those) came later.  Tone records are not periodic in the
places, so their reference for the whole stream is built by torch on the device from the virtual signal and itself held to
the numpy definition at the marked places."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import big_cases as B
import diff_levels_ref as DR
import events_ref as ER
import fir_levels_ref as FL
import fir_range_levels_ref as FRL
import frame_walk_ref as FW
import levels_ref as LR
import oracle_lib as O
import plane_events_ref as PE
import quantiles_ref as QR
import ranges_ref as RR
import seg_index_ref as SR
import spectra_levels_ref as SL
import spectra_ref as S
import tone_levels_ref as TL
import tone_range_levels_ref as TRL

pytestmark = pytest.mark.gpu

EDGE, SPF, FPT, TS, SB = B.EDGE, B.SPF, B.FPT, B.TS, 32
BAD = B.BAD_ARG
NEED = 44 << 30          # free HBM the module asks for (it peaks below 40 GB)
FILL16 = 0x5A5A


class Big:
    """the stream in HBM with its tables, the virtual signal beside it on demand, and the context"""

    def __init__(self, x3, torch):
        t0 = time.perf_counter()
        self.x3, self.torch, self.dev = x3, torch, torch.device("cuda:0")
        self.ctx = x3.Context(0)
        self.p = x3.Params.default()
        self.case = c = B.Case()
        self.tile_wav = torch.from_numpy(np.stack([t.wav for t in c.tiles])).to(self.dev)
        self.stream = self.lay(c)
        self.fo, self.so = self.u64(c.frame_offsets()), self.u64(c.sample_offsets())
        self._virtual = self._seg = None
        self.refs = {}         # references a later case reuses (device tensors among them): released with the fixture
        self.low_free = torch.cuda.mem_get_info(self.dev)[0]
        torch.cuda.synchronize(self.dev)
        self.build_s = time.perf_counter() - t0

    def lay(self, case):
        """case's stream on the device, place by place from the uploaded tiles (64 bytes of slack behind it)"""
        torch = self.torch
        out = torch.empty(case.total_bytes + 64, dtype=torch.uint8, device=self.dev)
        out[case.total_bytes:] = 0
        tl = [torch.from_numpy(t.stream.copy()).to(self.dev) for t in case.tiles]
        po = case.place_off
        for m in range(case.M):
            out[int(po[m]):int(po[m + 1])] = tl[case.kind[m]]
        return out

    def signal_of(self, case):
        """case's samples on the device, by the same tiling"""
        kind = self.torch.from_numpy(case.kind.astype(np.int64)).to(self.dev)
        return self.tile_wav[kind].reshape(-1)

    def virtual(self):
        if self._virtual is None:
            self._virtual = self.signal_of(self.case)
        return self._virtual

    def drop_virtual(self):
        self._virtual = None
        self.torch.cuda.empty_cache()

    def u64(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(self.dev)

    def u32(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.dev)

    def full(self, shape, value, dtype):
        return self.torch.full(shape, value, dtype=dtype, device=self.dev)

    def ready(self):
        """torch's work is done: the context's stream is not torch's"""
        self.torch.cuda.synchronize(self.dev)
        self.low_free = min(self.low_free, self.torch.cuda.mem_get_info(self.dev)[0])

    def args(self):
        """(d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, params) of the window, range and level calls"""
        return (self.stream.data_ptr(), self.case.total_bytes, self.fo.data_ptr(), self.so.data_ptr(), self.case.F, self.p)

    def seg(self):
        """the segment index of the whole stream by x3_seg_index_build_dev (built once)"""
        if self._seg is None:
            n = self.x3.lib().x3_seg_index_entries(self.case.F, C.byref(self.p), SB)
            idx = self.full((n,), 0x5A5A5A5A5A5A5A5A, self.torch.int64)
            self.ready()
            assert self.ctx.seg_index_build_dev(self.stream.data_ptr(), self.case.total_bytes, self.fo.data_ptr(), self.case.F, self.p,
                                                idx.data_ptr(), SB) == 0, self.ctx.last_error()
            assert self.ctx.get_option("last_seg_index_irregular") == 0
            self._seg = idx
        return self._seg

    def seg_args(self, use):
        return (self.seg().data_ptr(), SB) if use else (None, 0)

    @contextlib.contextmanager
    def damaged(self, frames, where="payload"):
        """the stream with one bit flipped in each (place, frame in tile); -> the case that knows of it"""
        c = B.Case()
        c.damage(frames, where)
        self.flip(c.flips)
        try:
            yield c
        finally:
            self.flip(c.flips)

    def flip(self, flips):
        for pos, mask in flips:
            self.stream[pos] ^= mask
        self.ready()

    def close(self):
        self.ready()
        self.refs.clear()
        self.ctx.close()


@pytest.fixture(scope="module")
def big():
    torch = pytest.importorskip("torch")
    import x3hip
    dev = torch.device("cuda:0")
    if torch.cuda.mem_get_info(dev)[0] < NEED:
        pytest.skip("needs 44 GB of free HBM")
    free0, total = torch.cuda.mem_get_info(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    b = Big(x3hip, torch)
    b.peak = torch.cuda.max_memory_allocated(dev)
    yield b
    b.close()
    print("\nbeyond_4gib: fixture build %.2f s; peak device memory: torch's tensors %.2f GB, everything on the device "
          "(the library's workspaces included) %.2f GB of %.0f GB" % (b.build_s, b.peak / 1e9, (free0 - b.low_free) / 1e9, total / 1e9))


@pytest.fixture(autouse=True)
def _release(big, request):
    """a test's large buffers are gone before the next one allocates; its own peak is printed (-s shows it)"""
    big.torch.cuda.reset_peak_memory_stats(big.dev)
    yield
    peak = big.torch.cuda.max_memory_allocated(big.dev)
    big.low_free = min(big.low_free, big.torch.cuda.mem_get_info(big.dev)[0])
    big.peak = max(big.peak, peak)
    print(" [peak %.2f GB: %s]" % (peak / 1e9, request.node.name), end="")
    big.torch.cuda.empty_cache()


def three_bad(c):
    """(place, frame in tile) of a frame below byte 2^32, the one that holds it and one above"""
    f = c.frame_of_byte(EDGE)
    return [divmod(f - 3 * FPT - 7, FPT), divmod(f, FPT), divmod(f + 5 * FPT + 3, FPT)]


def first_diff(a, b):
    return np.flatnonzero(a != b)[:4].tolist()


# ------------------------------------------------------------------------------------------------ A. decoders

def _decode(big, case, stream, fo, p, opts, seg=None, record=False, status=None):
    """one x3_decode_dev[_seg] of the whole stream into a fresh buffer -> (samples, x3_decode_result)"""
    ctx, torch = big.ctx, big.torch
    back = big.full((case.total,), 0x1111, torch.int16)
    old = {k: ctx.get_option(k) for k in opts}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        big.ready()
        a = (stream.data_ptr(), case.total_bytes, fo.data_ptr(), case.F, p, back.data_ptr(), case.total)
        st = status.data_ptr() if status is not None else None
        if seg is None:
            rc = ctx.decode_dev(*a, n_per_clip=case.total, d_status=st)
        else:
            rc = ctx.decode_dev_seg(*a, seg.data_ptr(), SB, record=record, n_per_clip=case.total, d_status=st)
        assert rc == 0, ctx.last_error()
        return back, ctx.decode_result()
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


@pytest.mark.parametrize("mode", ["default", "blocks", "single", "seg"])
def test_decode_whole_stream(big, mode):
    """x3_decode_dev over 442 944 frames: every sample against the virtual signal, clean and with three damaged frames"""
    c, ctx, torch = big.case, big.ctx, big.torch
    opts = {"default": {}, "blocks": {"decode_blocks": 1}, "single": {"decode_single": 1}, "seg": {}}[mode]
    kernel = {"default": 2, "blocks": 3, "single": 1, "seg": 2}[mode]
    virt = big.virtual()
    seg = None
    if mode == "seg":
        seg = torch.zeros(big.x3.lib().x3_seg_index_entries(c.F, C.byref(big.p), SB), dtype=torch.int64, device=big.dev)
        back, res = _decode(big, c, big.stream, big.fo, big.p, opts, seg, record=True)
        assert res == (0, c.F, 0, c.total), ("record", res)
        assert torch.equal(back, virt), "decode that records the index"
        del back
        assert torch.equal(seg, big.u64(expected_index(c))), "the recorded index is not the oracle's"
    back, res = _decode(big, c, big.stream, big.fo, big.p, opts, seg)
    assert res == (0, c.F, 0, c.total), (mode, res)
    assert ctx.get_option("last_decode_replays") == 0 and ctx.get_option("decode_kernel_in_use") == kernel, mode
    assert torch.equal(back, virt), "%s: samples differ from the virtual signal" % mode
    del back
    with big.damaged(three_bad(c)) as d:
        status = big.full((c.F,), -1, torch.int32)
        back, res = _decode(big, d, big.stream, big.fo, big.p, opts, seg, status=status)
        bad = sorted(d.bad)
        assert res == (0, bad[0], d.bad[bad[0]], bad[0] * SPF), (mode, res)
        nz = torch.nonzero(status).reshape(-1).cpu().tolist()
        assert nz == bad and [int(status[f]) for f in bad] == [d.bad[f] for f in bad], (mode, nz, bad)
        for f in bad:     # (what a failed frame leaves in its own samples is not specified: every other sample is)
            back[f * SPF:(f + 1) * SPF] = virt[f * SPF:(f + 1) * SPF]
        assert torch.equal(back, virt), "%s: a damaged frame disturbed its neighbours" % mode


def test_decode_block_length_40_past_byte_2_32(big):
    """the same tiles encoded at block length 40 (250 blocks a frame): the block-per-lane kernel by default"""
    big.drop_virtual()
    torch = big.torch
    c = B.Case(block_len=40)
    assert c.total_bytes > EDGE + B.MARGIN
    p = big.x3.Params.make(block_len=40, blocks_per_frame=250)
    stream, fo = big.lay(c), big.u64(c.frame_offsets())
    back, res = _decode(big, c, stream, fo, p, {})
    assert res == (0, c.F, 0, c.total), res
    assert big.ctx.get_option("decode_kernel_in_use") == 3 and big.ctx.get_option("last_decode_replays") == 0
    del stream
    assert torch.equal(back, big.signal_of(c)), "block length 40: samples differ from the virtual signal"


# ------------------------------------------------------------------------------------------------ B. frame walk

@pytest.mark.parametrize("no_fast", [0, 1])
def test_frame_walk(big, no_fast):
    """x3_index_dev and x3_decode_stream_dev find the builder's 442 944 offsets; a header damaged above byte 2^32 ends the walk
    where the reference's walk of that neighbourhood ends"""
    c, ctx, torch = big.case, big.ctx, big.torch
    ctx.set_option("index_no_fast", no_fast)
    try:
        fo = big.full((c.F + 8,), -1, torch.int64)
        wo = big.full((c.F + 8,), -1, torch.int64)
        big.ready()
        walks = ctx.get_option("index_general_walks"), ctx.get_option("index_fast_walks")
        res = ctx.index_dev(big.stream.data_ptr(), c.total_bytes, c.F + 8, fo.data_ptr(), wo.data_ptr())
        assert res == (0, c.F, c.total, 0), (no_fast, res)
        walks = ctx.get_option("index_general_walks") - walks[0], ctx.get_option("index_fast_walks") - walks[1]
        assert walks == ((1, 0) if no_fast else (0, 1)), "the walk took another path: (general, fast) = %s" % (walks,)
        assert torch.equal(fo[:c.F], big.fo[:c.F]) and torch.equal(wo[:c.F], big.so[:c.F]), "offsets of the walk"
        assert int((fo[c.F:] != -1).sum()) == 0 and int((wo[c.F:] != -1).sum()) == 0
        back = big.full((c.total,), 0x1111, torch.int16)
        big.ready()
        res = ctx.decode_stream_dev(big.stream.data_ptr(), c.total_bytes, big.p, back.data_ptr(), c.total)
        assert res == (0, c.total, c.F, 0), (no_fast, res)
        assert torch.equal(back, big.virtual()), "x3_decode_stream_dev: samples"
        del back
        m, i = divmod(c.frame_of_byte(EDGE) + 9 * FPT + 21, FPT)
        with big.damaged([(m, i)], where="header") as d:
            w = FW.walk(d.stream_bytes(int(d.place_off[m]), int(d.place_off[m + 1])))
            assert (w.n_frames, w.terminal) == (i, FW.INVALID_HEADER_CRC)
            nf = m * FPT + w.n_frames
            res = ctx.index_dev(big.stream.data_ptr(), c.total_bytes, c.F + 8, fo.data_ptr(), wo.data_ptr())
            assert res == (0, nf, nf * SPF, w.terminal), (no_fast, res)
            assert torch.equal(fo[:nf], big.fo[:nf]) and torch.equal(wo[:nf], big.so[:nf])
    finally:
        ctx.set_option("index_no_fast", 0)


# ------------------------------------------------------------------------------------------------ C. segment index by a walk

_INDEX = {}


def tile_index(c):
    """seg_index_ref's words of each tile: [tiles, 64 * 15] and word 0"""
    if "t" not in _INDEX:
        w = [SR.build(t.stream, t.fo[:-1], O.Params.default(), SB)[0] for t in c.tiles]
        _INDEX["t"] = (np.stack([x[1:] for x in w]), w[0][0])
    return _INDEX["t"]


def expected_index(c):
    words, w0 = tile_index(c)
    return np.concatenate([[w0], words[c.kind].reshape(-1)])


def test_seg_index_build(big):
    c = big.case
    idx = big.seg()
    words, w0 = tile_index(c)
    per = words.shape[1] // FPT
    fb, fs = c.frame_of_byte(EDGE), EDGE // SPF
    for name, f0, n in (("first 64", 0, 64), ("last 64", c.F - 64, 64), ("around byte 2^32", fb - 64, 128),
                        ("around sample 2^32", fs - 64, 128)):
        got = idx[1 + f0 * per:1 + (f0 + n) * per].cpu().numpy().view(np.uint64)
        want = np.concatenate([words[c.kind[f // FPT]][(f % FPT) * per:(f % FPT + 1) * per] for f in range(f0, f0 + n)])
        assert np.array_equal(got, want), (name, first_diff(got, want))
    assert big.torch.equal(idx, big.u64(expected_index(c))), "a word of the whole index differs"


# ------------------------------------------------------------------------------------------------ D. windows and ranges

def _windows(big, starts, L, fmt, use_seg):
    torch, ctx = big.torch, big.ctx
    n = len(starts)
    d_starts = big.u64(starts)
    out = big.full((n, L), 0x5A5A5A5A if fmt else FILL16, torch.int32 if fmt else torch.int16)
    st = big.full((n,), -1, torch.int32)
    seg = big.seg_args(use_seg)
    big.ready()
    rc = ctx.decode_windows_dev(*big.args(), d_starts.data_ptr(), n, L, out.data_ptr(), fmt, st.data_ptr(), *seg)
    assert rc == 0, ctx.last_error()
    return out, st, ctx.decode_windows_result()


def _window_starts(c, L, rng):
    fb = c.frame_of_byte(EDGE)
    s = [0, EDGE - L, EDGE - 1, EDGE, c.total - L, c.total - L + 1, (fb - 1) * SPF + 5, fb * SPF - 100, fb * SPF, (fb + 1) * SPF + 7,
         EDGE - L // 2, c.total - 1, c.total]
    s += [int(v) for v in rng.integers(0, c.total - L, size=24)]
    return s + [f * SPF - 3000 for f in sorted(c.bad)] + [f * SPF + 10 for f in sorted(c.bad)] + [(f + 1) * SPF - L // 3 for f in sorted(c.bad)]


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_windows(big, damage, use_seg):
    """fixed-length windows at the edges: rows, statuses and zeros behind a damaged covering frame, I16 and F32"""
    L = 12000
    with big.damaged(three_bad(big.case) if damage else []) as c:
        starts = _window_starts(c, L, np.random.default_rng(3))
        want = [c.window(s, L) for s in starts]
        rows, sts = np.stack([w[0] for w in want]), np.array([w[1] for w in want], dtype=np.int32)
        assert sts[5] == BAD and sts[0] == sts[1] == sts[2] == sts[3] == sts[4] == 0 and (not damage or (sts[-9:] != 0).all())
        bad = np.flatnonzero(sts)
        for fmt in (big.x3.WINDOW_I16, big.x3.WINDOW_F32):
            out, st, res = _windows(big, starts, L, fmt, use_seg)
            st = st.cpu().numpy()
            assert np.array_equal(st, sts), (fmt, [(starts[i], int(st[i]), int(sts[i])) for i in first_diff(st, sts)])
            assert res == (0, bad.size, int(bad[0]), int(sts[bad[0]])), res
            got = out.cpu().numpy()
            exp = RR.f32_bits(rows).view(np.int32) if fmt else rows
            for i in range(len(starts)):
                assert np.array_equal(got[i], exp[i]), ("window at %d, format %d" % (starts[i], fmt), first_diff(got[i], exp[i]))


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
def test_windows_more_than_2_32_elements(big, use_seg):
    """70 000 windows of 65 536 samples in one call: 4.59 G output elements, the rows compared on the device"""
    c, torch = big.case, big.torch
    n, L, step, s0 = 70000, 65536, 63000, 123457
    j = (np.arange(n, dtype=np.int64) * 23) % n                     # window w is chunk j[w] of the signal
    starts = s0 + j * step
    assert n * L > EDGE and int(starts.max()) + L <= c.total and int(starts.max()) > EDGE
    out, st, res = _windows(big, starts, L, big.x3.WINDOW_I16, use_seg)
    assert res == (0, 0, n, 0), res
    assert int(torch.count_nonzero(st)) == 0
    rows = big.virtual().as_strided((n, L), (step, 1), s0)          # (overlapping rows of the signal, no copy)
    jt = torch.from_numpy(j).to(big.dev)
    for a in range(0, n, 5000):
        assert torch.equal(out[a:a + 5000], rows[jt[a:a + 5000]]), "a row of windows %d .. %d" % (a, a + 5000)


def _ranges(big, starts, lens, stride, cap, use_seg, out=None):
    torch, ctx = big.torch, big.ctx
    n = len(starts)
    d_starts, d_lens = big.u64(starts), big.u32(lens)
    if out is None:
        out = big.full((cap,), FILL16, torch.int16)
    off = big.full((n + 1,), -1, torch.int64)
    st = big.full((n,), -1, torch.int32)
    seg = big.seg_args(use_seg)
    big.ready()
    rc = ctx.decode_ranges_dev(*big.args(), d_starts.data_ptr(), d_lens.data_ptr(), n, stride, out.data_ptr(), cap,
                               big.x3.WINDOW_I16, off.data_ptr(), st.data_ptr(), *seg)
    assert rc == 0, ctx.last_error()
    res = ctx.decode_ranges_result()      # (waits: only then are the tensors the call's)
    return out, off.cpu().numpy(), st.cpu().numpy(), res


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
def test_packed_ranges_past_element_2_32(big, use_seg):
    """lengths [2^31 + 5, 3, 2^31 + 7, 0, 1000]: off[] is the exact 64-bit prefix; the third row begins past byte 2^32 of the
    output and ends past element 2^32, where the last two rows begin"""
    c, torch = big.case, big.torch
    virt = big.virtual()
    lens = [(1 << 31) + 5, 3, (1 << 31) + 7, 0, 1000]
    starts = [(1 << 31) + 12345, EDGE + 1, 100_000_007, c.total, c.total - 1000]
    pre = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(pre[-1])
    assert starts[0] < EDGE < starts[0] + lens[0] and 2 * pre[2] > EDGE and pre[2] < EDGE < pre[3] == pre[4]
    out, off, st, res = _ranges(big, starts, lens, 0, total + 4096, use_seg)
    assert np.array_equal(off, pre), (off, pre)
    assert st.tolist() == [0] * 5 and res == (0, 0, 5, 0, total), (st, res)
    for w in range(5):
        a = int(pre[w])
        assert torch.equal(out[a:a + lens[w]], virt[starts[w]:starts[w] + lens[w]]), "row %d of the packed ranges" % w
    assert int((out[total:] != FILL16).sum()) == 0, "written behind the rows"
    # an out_cap that cuts the third range: BAD_ARG for it alone, and nothing of it is written
    cap = int(pre[3]) - 1
    out[int(pre[2]):] = FILL16
    out, off, st, res = _ranges(big, starts[:3], lens[:3], 0, cap, use_seg, out=out)
    assert np.array_equal(off, pre[:4]) and st.tolist() == [0, 0, BAD] and res == (0, 1, 2, BAD, int(pre[3])), (st, res)
    assert not bool((out[int(pre[2]):] != FILL16).any()), "a range without room was written"
    assert torch.equal(out[:lens[0]], virt[starts[0]:starts[0] + lens[0]])


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
def test_padded_ranges_with_a_stride_past_2_31(big, use_seg):
    """row_stride 2^31 + 16, three rows: the samples, and zero in every element of [len, stride)"""
    c, torch = big.case, big.torch
    big.drop_virtual()
    stride = (1 << 31) + 16
    with big.damaged(three_bad(c)[1:2]) as d:
        fbad = sorted(d.bad)[0]
        lens, starts = [5000, 12001, 30000], [EDGE - 2500, c.total - 12001, fbad * SPF - 10007]
        out, off, st, res = _ranges(big, starts, lens, stride, 3 * stride, use_seg)
        assert off.tolist() == [w * stride for w in range(4)]
        want = [d.window(s, n) for s, n in zip(starts, lens)]
        assert st.tolist() == [0, 0, d.bad[fbad]] and res == (0, 1, 2, d.bad[fbad], sum(lens)), (st, res)
        for w in range(3):
            got = out[w * stride:w * stride + lens[w]].cpu().numpy()
            assert np.array_equal(got, want[w][0]), ("padded row %d" % w, first_diff(got, want[w][0]))
            assert int(torch.count_nonzero(out[w * stride + lens[w]:(w + 1) * stride])) == 0, "row %d is not zero behind its length" % w


# ------------------------------------------------------------------------------------------------ E. levels family

def _levels(big, bin_len, n_bins, signal, use_seg, plain=False):
    """-> (records, frame statuses, x3_levels_result); plain: x3_levels_dev itself"""
    torch, ctx = big.torch, big.ctx
    lv = big.full((n_bins, 32), 0x5A, torch.uint8)
    st = big.full((big.case.F,), -1, torch.int32)
    seg = big.seg_args(use_seg)
    big.ready()
    if plain:
        rc = ctx.levels_dev(*big.args(), bin_len, lv.data_ptr(), n_bins, st.data_ptr(), *seg)
    else:
        rc = ctx.signal_levels_dev(*big.args(), bin_len, lv.data_ptr(), n_bins, st.data_ptr(), *seg, signal=signal)
    assert rc == 0, ctx.last_error()
    res = ctx.levels_result()
    return lv.cpu().numpy().reshape(-1).view(LR.LEVEL_DTYPE), st, res


def _same_records(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    d = first_diff(got, want)
    assert not d, (what, d, got[d[:1]], want[d[:1]])


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_levels(big, damage, use_seg):
    """x3_levels_dev and x3_signal_levels_dev (DIFF) at bin lengths 10 000 and 640 000: every record of the stream"""
    bad = three_bad(big.case) if damage else []
    if damage:     # (and a place's last frame with the next place's first: the seams between tiles)
        m = EDGE // TS
        bad = bad + [(m, FPT - 1), (m + 3, 0)]
    with big.damaged(bad) as c:
        for bin_len in (10000, 640000):
            n_bins = c.total // bin_len
            for signal in (B.SAMPLES, B.DIFF):
                got, st, res = _levels(big, bin_len, n_bins, signal, use_seg, plain=signal == B.SAMPLES)
                what = "levels: bin length %d, signal %d" % (bin_len, signal)
                _same_records(got, c.levels(bin_len, signal=signal), what)
                b = sorted(c.bad)
                assert res == ((0, len(b), b[0], c.bad[b[0]]) if b else (0, 0, c.F, 0)), (what, res)
                assert big.torch.nonzero(st).reshape(-1).cpu().tolist() == b, what
                if not damage:
                    assert int(got["n"].sum()) == c.total - (signal == B.DIFF)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
def test_levels_one_bin_and_a_bin_short_of_2_32(big, use_seg):
    """bin_len 0 is one bin whose n counts modulo 2^32; n_bins that end one bin short of position 2^32 count nothing behind"""
    c = big.case
    for signal in (B.SAMPLES, B.DIFF):
        got, _, res = _levels(big, 0, 1, signal, use_seg)
        assert res == (0, 0, c.F, 0)
        _same_records(got, c.levels(0, signal=signal), "one bin for everything, signal %d" % signal)
        assert int(got["n"][0]) == (c.total - (signal == B.DIFF)) & 0xFFFFFFFF     # (n counts modulo 2^32)
        n_bins = EDGE // 10000                                     # positions from 4 294 960 000 on are not counted
        got, _, _ = _levels(big, 10000, n_bins, signal, use_seg)
        _same_records(got, c.levels(10000, n_bins, signal), "bins that stop short of position 2^32, signal %d" % signal)
        assert int(got["n"].sum(dtype=np.uint64)) == n_bins * 10000 - (signal == B.DIFF)


def _range_levels(big, starts, lens, bin_len, signal, use_seg):
    torch, ctx = big.torch, big.ctx
    n = len(starts)
    rows = [max(1, -(-x // bin_len)) for x in lens]
    cap = sum(rows)
    lv = big.full((cap + 2, 32), 0x5A, torch.uint8)
    off = big.full((n + 1,), -1, torch.int64)
    st = big.full((n,), -1, torch.int32)
    d_starts, d_lens = big.u64(starts), big.u32(lens)
    seg = big.seg_args(use_seg)
    big.ready()
    rc = ctx.signal_range_levels_dev(*big.args(), d_starts.data_ptr(), d_lens.data_ptr(), n, bin_len, 0, lv.data_ptr(), cap,
                                     off.data_ptr(), st.data_ptr(), *seg, signal=signal)
    assert rc == 0, ctx.last_error()
    res = ctx.range_levels_result()
    raw = lv.cpu().numpy()
    assert (raw[cap:] == 0x5A).all(), "written behind rows_cap"
    assert off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist()
    return raw[:cap].reshape(-1).view(LR.LEVEL_DTYPE), rows, st.cpu().numpy(), res


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_range_levels(big, damage, use_seg):
    """x3_range_levels_dev / x3_signal_range_levels_dev: bins from each range's own start, on both sides of 2^32"""
    with big.damaged(three_bad(big.case) + [(EDGE // TS, EDGE // SPF % FPT)] if damage else []) as c:
        starts = [EDGE - 5000, EDGE + 5000, (1 << 31) + 12345, EDGE - 7, c.total - 20001]
        lens = [30000, 30000, (1 << 31) + 7, 14, 20001]
        for signal in (B.SAMPLES, B.DIFF):
            got, rows, st, res = _range_levels(big, starts, lens, 10000, signal, use_seg)
            want_st = [c.range_status(s, n) for s, n in zip(starts, lens)]
            assert st.tolist() == want_st and (res[0], res[1], res[4]) == (0, sum(1 for v in want_st if v), sum(rows)), (st, want_st, res)
            at = 0
            for w, (s, n) in enumerate(zip(starts, lens)):
                _same_records(got[at:at + rows[w]], c.range_levels(s, n, 10000, signal),
                              "range (%d, %d), signal %d" % (s, n, signal))
                at += rows[w]


def test_range_levels_of_everything_equal_levels(big):
    """a length has 32 bits, so (0, total) is three ranges back to back, each a multiple of the bin length: their records
    are the levels call's, record for record"""
    c = big.case
    lens = [2_000_000_000, 2_000_000_000, c.total - 4_000_000_000]
    starts = [0, lens[0], lens[0] + lens[1]]
    for signal in (B.SAMPLES, B.DIFF):
        got, rows, st, res = _range_levels(big, starts, lens, 10000, signal, True)
        assert st.tolist() == [0, 0, 0] and sum(rows) == c.total // 10000
        lv, _, _ = _levels(big, 10000, c.total // 10000, signal, True)
        _same_records(got, lv, "ranges against the levels call, signal %d" % signal)
        _same_records(got, c.levels(10000, signal=signal), "ranges against the reference, signal %d" % signal)


def test_chain_levels_events_ranges(big):
    """levels -> x3_events_dev -> x3_decode_ranges_dev with no host trip: the loud tile stands above sample 2^32 only"""
    c, ctx, torch = big.case, big.ctx, big.torch
    bin_len, cap = 10000, 16
    n_bins = c.total // bin_len
    rule = ER.Rule(mean_sq_min=B.LOUD_MEAN_SQ, join_bins=2, pad_bins=1)
    ev, elv = ER.stream_events(c.levels(bin_len), c.total, bin_len, rule)
    assert 1 <= len(ev) <= cap and all(s > EDGE for s, _ in ev)
    stride = max(n for _, n in ev)
    lv = big.full((n_bins, 32), 0x5A, torch.uint8)
    starts, lens = big.full((cap,), -1, torch.int64), big.full((cap,), -1, torch.int32)
    evl, count = big.full((cap, 32), 0x5A, torch.uint8), big.full((1,), -1, torch.int64)
    out = big.full((cap, stride), FILL16, torch.int16)
    st = big.full((cap,), -1, torch.int32)
    big.ready()
    seg = big.seg_args(True)
    assert ctx.levels_dev(*big.args(), bin_len, lv.data_ptr(), n_bins, None, *seg) == 0
    r = big.x3.EventRule.make(mean_sq_min=rule.mean_sq_min, join_bins=rule.join_bins, pad_bins=rule.pad_bins)
    assert ctx.events_dev(lv.data_ptr(), n_bins, bin_len, big.so.data_ptr() + 8 * c.F, r, starts.data_ptr(), lens.data_ptr(),
                          evl.data_ptr(), cap, count.data_ptr()) == 0, ctx.last_error()
    assert ctx.decode_ranges_dev(*big.args(), starts.data_ptr(), lens.data_ptr(), cap, stride, out.data_ptr(), cap * stride,
                                 big.x3.WINDOW_I16, None, st.data_ptr(), *seg) == 0, ctx.last_error()
    assert ctx.decode_ranges_result()[:4] == (0, 0, cap, 0)
    assert ctx.events_result() == (0, len(ev)) and ctx.levels_result() == (0, 0, c.F, 0)
    _, w_st, w_ln, w_lv = ER.slots(ev, elv, cap, False)
    assert int(count[0]) == len(ev)
    assert np.array_equal(starts.cpu().numpy().view(np.uint64), w_st) and np.array_equal(lens.cpu().numpy().view(np.uint32), w_ln)
    assert np.array_equal(evl.cpu().numpy().reshape(-1).view(LR.LEVEL_DTYPE), w_lv)
    rows = out.cpu().numpy()
    for i, (s, n) in enumerate(ev):
        assert np.array_equal(rows[i, :n], c.samples(s, s + n)) and not rows[i, n:].any(), "event %d at %d" % (i, s)
    assert not rows[len(ev):].any()


# ------------------------------------------------------------------------------------------------ E2. FIR, tone and bank levels

TONE_STEP = 276168143                     # Tone.at(12 345.678, 192 000)'s step made odd: no period in the places
BANK_STEPS = (TONE_STEP, 0, 1 << 30, 1 << 31, 0xFFFFFFFF, 1, 3 * 5 * 7 * 11 * 13 * 17 * 19 + 2, 0x9E3779B1)
M32 = 0xFFFFFFFF


def seam_bad(c):
    """test_levels' damage: three_bad, and a place's last frame with a later place's first one (the seams between tiles)"""
    m = EDGE // TS
    return three_bad(c) + [(m, FPT - 1), (m + 3, 0)]


def _signal_levels(big, call, arg, bin_len, n_bins, use_seg, planes=1):
    """one x3_fir_levels_dev / x3_tone_levels_dev / x3_tone_bank_levels_dev (call: the Context's method, arg: its Fir, Tone
    or Tones) -> (the records on the device uint8 [planes * n_bins, 32], frame statuses, x3_levels_result)"""
    torch, ctx = big.torch, big.ctx
    lv = big.full((planes * n_bins, 32), 0x5A, torch.uint8)
    st = big.full((big.case.F,), -1, torch.int32)
    seg = big.seg_args(use_seg)
    big.ready()
    rc = getattr(ctx, call)(*big.args(), bin_len, lv.data_ptr(), n_bins, st.data_ptr(), *seg, arg)
    assert rc == 0, ctx.last_error()
    return lv, st, ctx.levels_result()


def _level_records(lv):
    return lv.cpu().numpy().reshape(-1).view(LR.LEVEL_DTYPE)


def _tone_words(lv):
    """tone records on the device uint8 [..., n, 32] as int64 [..., n, 4]: re, im, (min, max), (n, reserved)"""
    import torch
    return lv.view(torch.int64)


def _check_result(c, st, res, torch, what):
    b = sorted(c.bad)
    assert res == ((0, len(b), b[0], c.bad[b[0]]) if b else (0, 0, c.F, 0)), (what, res)
    assert torch.nonzero(st).reshape(-1).cpu().tolist() == b, what


def _tone_bins(big, good, g0, n_bins, bin_len, steps):
    """the torch reference of tone records on the device, from the virtual signal: n_bins bins of bin_len positions from g0,
    for every step -> int64 [len(steps), n_bins, 4] as _tone_words gives them.  good: None, or a bool tensor per frame (a
    failed frame adds nothing).  All in int64 without a wrap: the pair of position i is (((i mod 2^32) * step) mod 2^32) >> 22
    with the step split into halves of 16 bits, so that no product exceeds 2^48"""
    torch = big.torch
    virt = big.virtual()
    tab = torch.from_numpy(TL.table().astype(np.int32)).to(big.dev)
    out = torch.empty((len(steps), n_bins, 4), dtype=torch.int64, device=big.dev)
    per = max(1, (1 << 25) // bin_len)
    for b in range(0, n_bins, per):
        nb = min(per, n_bins - b)
        a, n = g0 + b * bin_len, nb * bin_len
        x = virt[a:a + n].to(torch.int32)
        pos = torch.arange(a, a + n, dtype=torch.int64, device=big.dev)
        if good is None:
            mn, mx = x, x
            cnt = torch.full((nb,), bin_len, dtype=torch.int64, device=big.dev)
        else:
            ok = good[pos // SPF]
            mn, mx = torch.where(ok, x, 32767), torch.where(ok, x, -32768)
            x = torch.where(ok, x, 0)
            cnt = ok.view(nb, bin_len).sum(dim=1, dtype=torch.int64)
        mn, mx = mn.view(nb, bin_len).amin(dim=1).to(torch.int64), mx.view(nb, bin_len).amax(dim=1).to(torch.int64)
        p = pos & M32
        del pos
        for t, step in enumerate(steps):
            lo, hi = step & 0xFFFF, step >> 16
            k = (((p * lo) + (((p * hi) & 0xFFFF) << 16)) & M32) >> 22
            cs = tab[k]
            out[t, b:b + nb, 0] = (x * cs[:, 0]).view(nb, bin_len).sum(dim=1, dtype=torch.int64)   # (|product| <= 2^30: int32 holds it)
            out[t, b:b + nb, 1] = (x * cs[:, 1]).view(nb, bin_len).sum(dim=1, dtype=torch.int64)
            out[t, b:b + nb, 2] = (mn & M32) | (mx << 32)
            out[t, b:b + nb, 3] = cnt
            del k, cs
    return out


def _good_frames(big, c):
    good = big.torch.ones(c.F, dtype=big.torch.bool, device=big.dev)
    for f in c.bad:
        good[f] = False
    return good


def _tone_ref(big, c, g0, n_bins, bin_len, steps):
    """_tone_bins of the clean stream, computed once for (g0, n_bins, bin_len, steps); for a damaged case the bins that a
    failed frame touches are computed again with the mask -> a tensor the caller must not write to"""
    key = (g0, n_bins, bin_len, tuple(steps))
    key = ("tone",) + key
    if key not in big.refs:
        big.refs[key] = _tone_bins(big, None, g0, n_bins, bin_len, steps)
    ref = big.refs[key]
    if c.bad:
        ref = ref.clone()
        good = _good_frames(big, c)
        for f in sorted(c.bad):
            j0, j1 = (f * SPF - g0) // bin_len, ((f + 1) * SPF - 1 - g0) // bin_len
            j0, j1 = max(j0, 0), min(j1, n_bins - 1)
            if j0 <= j1:
                ref[:, j0:j1 + 1] = _tone_bins(big, good, g0 + j0 * bin_len, j1 - j0 + 1, bin_len, steps)
    return ref


def _fold(big, ref, k):
    """the records of bins k times as long, from reference records [T, n, 4] with n a multiple of k"""
    torch = big.torch
    T, n, _ = ref.shape
    r = ref.view(T, n // k, k, 4)
    mn = (r[..., 2] << 32 >> 32).amin(dim=2)
    mx = (r[..., 2] >> 32).amax(dim=2)
    return torch.stack([r[..., 0].sum(dim=2), r[..., 1].sum(dim=2), (mn & M32) | (mx << 32), r[..., 3].sum(dim=2)], dim=2)


def _same_words(torch, got, want, what):
    if not torch.equal(got, want):
        d = torch.nonzero((got != want).any(dim=-1)).reshape(-1)
        i = int(d[0])
        raise AssertionError((what, "records differ: %d, the first at %d" % (d.numel(), i), got[i].tolist(), want[i].tolist()))


def _edge_places(c):
    return sorted({c.place_of_byte(EDGE), EDGE // TS, c.M - 1})


def _words_to_records(w):
    return np.ascontiguousarray(w.cpu().numpy()).reshape(-1).view(TL.TONE_DTYPE)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_fir_levels(big, damage, use_seg):
    """x3_fir_levels_dev at bin lengths 10 000 and 640 000: every record of the stream, eight taps against the closed form,
    taps (1, -1) against DIFF's records, which tests/test_big_cases.py proves equal"""
    x3 = big.x3
    with big.damaged(seam_bad(big.case) if damage else []) as c:
        for bin_len in (10000, 640000):
            n_bins = c.total // bin_len
            for sig, ref in ((B.FIR8, B.FIR8), (B.FIR_DIFF, B.DIFF)):
                lv, st, res = _signal_levels(big, "fir_levels_dev", x3.Fir(sig[1], sig[2]), bin_len, n_bins, use_seg)
                what = "FIR levels: bin length %d, taps %s" % (bin_len, sig[1])
                got = _level_records(lv)
                _same_records(got, c.levels(bin_len, signal=ref), what)
                _check_result(c, st, res, big.torch, what)
                if not damage:
                    assert int(got["n"].sum()) == c.total - (len(sig[1]) - 1)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_tone_levels(big, damage, use_seg):
    """x3_tone_levels_dev at one odd step: every record of the stream against the torch reference on the device, the bins of
    the three marked places against Case.tone_records as well, and x3_tone_power_levels_dev in place on those"""
    x3, torch, ctx = big.x3, big.torch, big.ctx
    assert x3.Tone.at(12345.678, 192000).step | 1 == TONE_STEP
    with big.damaged(seam_bad(big.case) if damage else []) as c:
        ref = _tone_ref(big, c, 0, c.total // SPF, SPF, BANK_STEPS)[0:1]
        for bin_len in (10000, 640000):
            n_bins = c.total // bin_len
            lv, st, res = _signal_levels(big, "tone_levels_dev", x3.Tone(TONE_STEP), bin_len, n_bins, use_seg)
            what = "tone levels: bin length %d" % bin_len
            want = _fold(big, ref, bin_len // SPF)[0]
            got = _tone_words(lv)
            _same_words(torch, got, want, what)
            _check_result(c, st, res, torch, what)
            per = TS // bin_len
            for m in _edge_places(c):
                rec = _words_to_records(got[m * per:(m + 1) * per])
                cpu = c.tone_records(m * TS, (m + 1) * TS, bin_len, TONE_STEP)
                assert np.array_equal(rec, cpu), (what, "place %d" % m, first_diff(rec, cpu))
                part = lv[m * per:(m + 1) * per].clone()
                big.ready()
                assert ctx.tone_power_levels_dev(part.data_ptr(), per, part.data_ptr()) == 0, ctx.last_error()
                ctx.sync()
                _same_records(_level_records(part), TL.tone_power_levels(cpu), what + ": the band's level, place %d" % m)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_tone_bank_levels(big, damage, use_seg):
    """x3_tone_bank_levels_dev with eight steps (0, 2^30, 2^31, 2^32 - 1 and the tone's among them): plane t is the single
    call's records for step t, from the same reference"""
    x3, torch = big.x3, big.torch
    tones = [x3.Tone(s) for s in BANK_STEPS]
    with big.damaged(seam_bad(big.case) if damage else []) as c:
        ref = _tone_ref(big, c, 0, c.total // SPF, SPF, BANK_STEPS)
        for bin_len in (10000, 640000):
            n_bins = c.total // bin_len
            lv, st, res = _signal_levels(big, "tone_bank_levels_dev", tones, bin_len, n_bins, use_seg, planes=len(tones))
            what = "tone bank levels: bin length %d" % bin_len
            _same_words(torch, _tone_words(lv).view(len(tones), n_bins, 4), _fold(big, ref, bin_len // SPF), what)
            _check_result(c, st, res, torch, what)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
def test_signal_levels_one_bin_and_a_bin_short_of_2_32(big, use_seg):
    """as test_levels_one_bin_and_a_bin_short_of_2_32, for the FIR, the tone and the bank: bin_len 0 is one record whose n
    counts modulo 2^32; n_bins that end one bin short of position 2^32 count nothing from 4 294 960 000 on"""
    x3, torch, c = big.x3, big.torch, big.case
    tones = [x3.Tone(s) for s in BANK_STEPS]
    ref = _tone_ref(big, c, 0, c.total // SPF, SPF, BANK_STEPS)
    short = EDGE // 10000
    # FIR
    fir = x3.Fir(B.FIR8[1], B.FIR8[2])
    lv, _, res = _signal_levels(big, "fir_levels_dev", fir, 0, 1, use_seg)
    assert res == (0, 0, c.F, 0)
    got = _level_records(lv)
    _same_records(got, c.levels(0, signal=B.FIR8), "FIR: one bin for everything")
    assert int(got["n"][0]) == (c.total - 7) & M32
    lv, _, _ = _signal_levels(big, "fir_levels_dev", fir, 10000, short, use_seg)
    got = _level_records(lv)
    _same_records(got, c.levels(10000, short, B.FIR8), "FIR: bins that stop short of position 2^32")
    assert int(got["n"].sum(dtype=np.uint64)) == short * 10000 - 7
    # tone and bank: one record is the fold of all, n modulo 2^32
    one = _fold(big, ref, ref.shape[1])
    assert int(one[0, 0, 3]) == c.total
    one[:, :, 3] &= M32
    lv, _, _ = _signal_levels(big, "tone_levels_dev", tones[0], 0, 1, use_seg)
    _same_words(torch, _tone_words(lv), one[0], "tone: one bin for everything")
    lv, _, _ = _signal_levels(big, "tone_bank_levels_dev", tones, 0, 1, use_seg, planes=len(tones))
    _same_words(torch, _tone_words(lv).view(len(tones), 1, 4), one, "tone bank: one bin for everything")
    lv, _, _ = _signal_levels(big, "tone_levels_dev", tones[0], 10000, short, use_seg)
    _same_words(torch, _tone_words(lv), ref[0, :short], "tone: bins that stop short of position 2^32")
    lv, _, _ = _signal_levels(big, "tone_bank_levels_dev", tones, 10000, short, use_seg, planes=len(tones))
    _same_words(torch, _tone_words(lv).view(len(tones), short, 4), ref[:, :short].contiguous(), "tone bank: bins short of 2^32")


# ------------------------------------------------------------------------------------------------ E3. their range forms

def _signal_range_levels(big, call, arg, starts, lens, bin_len, use_seg, planes=1):
    """one x3_fir_range_levels_dev / x3_tone_range_levels_dev / x3_tone_bank_range_levels_dev, packed -> (records on the
    device uint8 [planes, cap, 32], rows of every range, statuses, x3_range_levels_result); two records of 0x5A behind every
    plane's last must survive"""
    torch, ctx = big.torch, big.ctx
    n = len(starts)
    rows = [max(1, -(-x // bin_len)) for x in lens]
    cap = sum(rows)
    lv = big.full((planes * cap + 2, 32), 0x5A, torch.uint8)
    off = big.full((n + 1,), -1, torch.int64)
    st = big.full((n,), -1, torch.int32)
    d_starts, d_lens = big.u64(starts), big.u32(lens)
    seg = big.seg_args(use_seg)
    big.ready()
    rc = getattr(ctx, call)(*big.args(), d_starts.data_ptr(), d_lens.data_ptr(), n, bin_len, 0, lv.data_ptr(), cap, off.data_ptr(),
                            st.data_ptr(), *seg, arg)
    assert rc == 0, ctx.last_error()
    res = ctx.range_levels_result()
    assert bool((lv[planes * cap:] == 0x5A).all()), "written behind the last plane's rows_cap"
    assert off.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist()
    return lv[:planes * cap].view(planes, cap, 32), rows, st.cpu().numpy(), res


def _range_cases(c):
    """test_range_levels' ranges: both sides of 2^32, 2^31 + 7 samples across it, 14 samples across it, the stream's end"""
    return ([EDGE - 5000, EDGE + 5000, (1 << 31) + 12345, EDGE - 7, c.total - 20001], [30000, 30000, (1 << 31) + 7, 14, 20001])


def _range_damage(c):
    return three_bad(c) + [(EDGE // TS, EDGE // SPF % FPT)]


def _check_range_status(c, starts, lens, rows, st, res):
    want_st = [c.range_status(s, n) for s, n in zip(starts, lens)]
    assert st.tolist() == want_st and (res[0], res[1], res[4]) == (0, sum(1 for v in want_st if v), sum(rows)), (st, want_st, res)


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_fir_range_levels(big, damage, use_seg):
    """x3_fir_range_levels_dev: the filtered stream cut to ranges on both sides of 2^32, bins from each range's own start"""
    x3 = big.x3
    with big.damaged(_range_damage(big.case) if damage else []) as c:
        starts, lens = _range_cases(c)
        for sig, ref in ((B.FIR8, B.FIR8), (B.FIR_DIFF, B.DIFF)):
            lv, rows, st, res = _signal_range_levels(big, "fir_range_levels_dev", x3.Fir(sig[1], sig[2]), starts, lens, 10000, use_seg)
            _check_range_status(c, starts, lens, rows, st, res)
            got, at = _level_records(lv[0]), 0
            for w, (s, n) in enumerate(zip(starts, lens)):
                _same_records(got[at:at + rows[w]], c.range_levels(s, n, 10000, ref), "FIR range (%d, %d), taps %s" % (s, n, sig[1]))
                at += rows[w]


def _tone_range_check(big, c, lv, rows, starts, lens, steps, what):
    """planes of tone range records [T, cap, 32] against Case.tone_records (the short ranges, and the last, short bin of the
    long one) and against the device reference at the range's own phase (the whole bins of the long one)"""
    torch = big.torch
    words = _tone_words(lv).view(len(steps), -1, 4)
    at = 0
    for w, (s, n) in enumerate(zip(starts, lens)):
        got = words[:, at:at + rows[w]]
        full = n // 10000 if n > 100000 else 0
        if full:
            assert tuple(steps) == BANK_STEPS[:len(steps)]
            ref = _tone_ref(big, c, s, full, 10000, BANK_STEPS)[:len(steps)]
            _same_words(torch, got[:, :full], ref, "%s: range (%d, %d)" % (what, s, n))
        for t, step in enumerate(steps):
            rec = _words_to_records(got[t, full:])
            cpu = c.tone_records(s + full * 10000, s + n, 10000, step)
            assert np.array_equal(rec, cpu), ("%s: range (%d, %d), step %d" % (what, s, n, step), first_diff(rec, cpu))
        at += rows[w]


@pytest.mark.parametrize("use_seg", [False, True], ids=["no_index", "index"])
@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_tone_range_levels(big, damage, use_seg):
    """x3_tone_range_levels_dev and x3_tone_bank_range_levels_dev: the oscillators do not restart at a range, so a start past
    2^32 decides the phase"""
    x3 = big.x3
    with big.damaged(_range_damage(big.case) if damage else []) as c:
        starts, lens = _range_cases(c)
        lv, rows, st, res = _signal_range_levels(big, "tone_range_levels_dev", x3.Tone(TONE_STEP), starts, lens, 10000, use_seg)
        _check_range_status(c, starts, lens, rows, st, res)
        _tone_range_check(big, c, lv, rows, starts, lens, BANK_STEPS[:1], "tone")
        tones = [x3.Tone(s) for s in BANK_STEPS]
        lv, rows, st, res = _signal_range_levels(big, "tone_bank_range_levels_dev", tones, starts, lens, 10000, use_seg, planes=8)
        _check_range_status(c, starts, lens, rows, st, res)
        _tone_range_check(big, c, lv, rows, starts, lens, BANK_STEPS, "tone bank")


def test_signal_range_levels_of_everything_equal_levels(big):
    """test_range_levels_of_everything_equal_levels for the FIR and the tone: three ranges back to back, each a multiple of the
    bin length, give the levels call's records, record for record"""
    x3, torch, c = big.x3, big.torch, big.case
    lens = [2_000_000_000, 2_000_000_000, c.total - 4_000_000_000]
    starts = [0, lens[0], lens[0] + lens[1]]
    n_bins = c.total // 10000
    for what, arg in (("fir", x3.Fir(B.FIR8[1], B.FIR8[2])), ("tone", x3.Tone(TONE_STEP))):
        got, rows, st, res = _signal_range_levels(big, what + "_range_levels_dev", arg, starts, lens, 10000, True)
        assert st.tolist() == [0, 0, 0] and sum(rows) == n_bins
        lv, _, _ = _signal_levels(big, what + "_levels_dev", arg, 10000, n_bins, True)
        assert torch.equal(got[0], lv), "ranges against the levels call: " + what


# ------------------------------------------------------------------------------------------------ F. entries of one buffer

def entry_table(c):
    """about 40 entries (first frame, frames): runs of whole frames below 2^31 bytes, across 2^31, across 2^32, above it and
    in the buffer's last bytes; two that overlap, one that repeats"""
    f31, f32 = c.frame_of_byte(1 << 31), c.frame_of_byte(EDGE)
    rng = np.random.default_rng(12)
    ents = [(0, 1), (5, 64), (1000, 3), (f31 - 70, 7), (f31 - 2, 5), (f31, 1), (f31 - 63, 64), (f32 - 2, 5), (f32, 1),
            (f32 - 40, 64), (f32 - 1, 2), (f32 + 1, 9), (f32 + 100, 33), (c.F - 300, 17), (c.F - 64, 64), (c.F - 1, 1),
            (c.F - 3, 3), (f32 + 200, 10), (f32 + 205, 10), (f32 - 2, 5), (EDGE // SPF - 3, 8)]
    for lo, hi in ((0, f31 - 64), (f31, f32 - 64), (f32 + 300, c.F - 400)):
        ents += [(int(rng.integers(lo, hi)), int(rng.integers(1, 65))) for _ in range(6)]
    assert len(ents) == 39
    return ents


ENTRY_BAD = 12      # the entry (f32 + 100, 33) holds the damaged frame


def _entry_bytes(c, ents):
    fo = c.frame_offsets().astype(np.int64)
    return [int(fo[g]) for g, _ in ents], [int(fo[g + k] - fo[g]) for g, k in ents]


@contextlib.contextmanager
def _entries_damaged(big):
    f32 = big.case.frame_of_byte(EDGE)
    with big.damaged([divmod(f32 + 104, FPT)]) as c:
        yield c, entry_table(c)


def test_decode_streams(big):
    """x3_decode_streams_dev on the entry table: rows and x3_stream_result against the oracle on each entry's own bytes,
    whose samples are a slice of the virtual signal"""
    ctx, torch, x3 = big.ctx, big.torch, big.x3
    row_len = FPT * SPF
    with _entries_damaged(big) as (c, ents):
        offs, lens = _entry_bytes(c, ents)
        assert offs[4] < (1 << 31) < offs[4] + lens[4] and offs[7] < EDGE < offs[7] + lens[7] and offs[14] + lens[14] == c.total_bytes
        want = np.zeros((len(ents), row_len), dtype=np.int16)
        wres = np.zeros(len(ents), dtype=x3.STREAM_RESULT_DTYPE)
        for e, (g, k) in enumerate(ents):
            rc, wav, fok, ferr = O.decode_stream(c.stream_bytes(offs[e], offs[e] + lens[e]), wav_cap=row_len)
            f, st = c.first_bad(g, g + k)
            assert (rc, wav.size) == ((0, k * SPF) if f is None else (st, (f - g) * SPF)) and np.array_equal(wav, c.samples(g * SPF, g * SPF + wav.size))
            want[e, :wav.size] = wav
            wres[e] = (wav.size, fok, rc, ferr)
        nbad = int((wres["status"] != 0).sum())
        assert nbad == 1 and wres["status"][ENTRY_BAD] != 0
        for fmt in (x3.WINDOW_I16, x3.WINDOW_F32):
            out = big.full((len(ents), row_len), 0x5A5A5A5A if fmt else FILL16, torch.int32 if fmt else torch.int16)
            res = big.full((len(ents), 24), 0x5A, torch.uint8)
            big.ready()
            assert ctx.decode_streams_dev(big.stream.data_ptr(), c.total_bytes, offs, lens, big.p, out.data_ptr(), row_len, fmt,
                                          res.data_ptr()) == 0, ctx.last_error()
            assert ctx.decode_streams_result() == (0, nbad, ENTRY_BAD, int(wres["status"][ENTRY_BAD]))
            got = res.cpu().numpy().reshape(-1).view(x3.STREAM_RESULT_DTYPE)
            assert np.array_equal(got, wres), [(e, got[e], wres[e]) for e in first_diff(got, wres)]
            exp = RR.f32_bits(want).view(np.int32) if fmt else want
            got = out.cpu().numpy()
            for e in range(len(ents)):
                assert np.array_equal(got[e], exp[e]), ("entry %d %s, format %d" % (e, ents[e], fmt), first_diff(got[e], exp[e]))


def _entry_window(c, ents, e, s, n):
    g, k = ents[e]
    if s > k * SPF or n > k * SPF - s:
        return np.zeros(n, dtype=np.int16), BAD
    return c.window(g * SPF + s, n)


def _corpus_levels(c, ents, signal):
    """x3_corpus_signal_levels_dev's records at bin length 10 000: an entry is whole frames, so its bins are the stream's,
    but for the first difference at the entry's first position, which an entry on its own does not have"""
    glob = c.levels(SPF, signal=signal)
    parts = []
    for g, k in ents:
        r = glob[g:g + k].copy()
        if signal == B.DIFF:
            r[0] = DR.signal_levels([c.samples(g * SPF, (g + 1) * SPF)], [c.bad.get(g, 0)], [0], SPF, 1, B.DIFF)[0]
        parts.append(r)
    return np.concatenate(parts)


def _corpus_signal_refs(big, c, ents):
    """fir_levels_ref.corpus_fir_levels and tone_levels_ref.corpus_tone_levels on the entries' own samples at bin length
    10 000 (computed once: both index forms see the same entries), and the bank's planes [8, rows]: plane 0 is the tone's, the
    others Case's tone_records_of from each entry's first position, which tests/test_big_cases.py holds to the same reference"""
    if "corpus" not in big.refs:
        entries = []
        for g, k in ents:
            st = [c.bad.get(g + i, 0) for i in range(k)]
            entries.append(([c.samples((g + i) * SPF, (g + i + 1) * SPF) for i in range(k)], st, [i * SPF for i in range(k)], k * SPF))
        fir = FL.corpus_fir_levels(entries, SPF, B.FIR8[1], B.FIR8[2])[0]
        tone = TL.corpus_tone_levels(entries, SPF, TONE_STEP)[0]
        bank = np.stack([tone] + [np.concatenate([B.tone_records_of(np.concatenate(fr), np.repeat(np.array(st) == 0, SPF), 0, SPF, step)
                                                  for fr, st, _, _ in entries]) for step in BANK_STEPS[1:]])
        big.refs["corpus"] = (fir, tone, bank)
    return big.refs["corpus"]


def _entry_frames(c, ents, e, s, n):
    """(frames, sample offsets) of the frames of entry e that cover the range (s, n), and the one in front of them (a FIR
    value reaches 7 samples back), as the range references take them: positions relative to the entry"""
    g, k = ents[e]
    a, b = max(s // SPF - 1, 0), min((s + max(n, 1) - 1) // SPF, k - 1)
    st = [c.bad.get(g + j, 0) for j in range(a, b + 1)]
    frames = [(v, None if v else c.samples((g + j) * SPF, (g + j + 1) * SPF)) for v, j in zip(st, range(a, b + 1))]
    return frames, np.arange(a, b + 2, dtype=np.uint64) * np.uint64(SPF)


@pytest.mark.parametrize("index", ["decode", "walk"])
def test_corpus(big, index):
    """x3_corpus_build over the entry table (seg_blocks 32, recorded by a decode or built by the walk) and every corpus call
    against the slices of the virtual signal"""
    ctx, torch, x3 = big.ctx, big.torch, big.x3
    with _entries_damaged(big) as (c, ents):
        offs, lens = _entry_bytes(c, ents)
        E = len(ents)
        big.ready()
        corpus = x3.Corpus(ctx, (big.stream.data_ptr(), c.total_bytes), offs, lens, params=big.p, seg_blocks=SB, index=index)
        try:
            ns = [k * SPF for _, k in ents]
            first = np.concatenate([[0], np.cumsum([k for _, k in ents])])
            assert corpus.entries["n_samples"].tolist() == ns and corpus.entries["n_frames"].tolist() == [k for _, k in ents]
            assert corpus.entries["first_frame"].tolist() == first[:-1].tolist() and not corpus.entries["walk_status"].any()
            assert corpus.seg_blocks == SB and corpus.n_frames == first[-1]
            rng = np.random.default_rng(5)
            # windows
            L = 3000
            we = np.repeat(np.arange(E), 5)
            ws = np.array([[0, n - L, n - L + 1, int(rng.integers(0, n - L)), int(rng.integers(0, n - L))] for n in ns]).reshape(-1)
            want = [_entry_window(c, ents, int(e), int(s), L) for e, s in zip(we, ws)]
            for fmt in (x3.WINDOW_I16, x3.WINDOW_F32):
                rows, st = corpus.decode(we, ws, L, fmt)
                assert st.tolist() == [w[1] for w in want], "corpus windows: statuses"
                for i, w in enumerate(want):
                    exp = RR.f32_bits(w[0]) if fmt else w[0]
                    assert np.array_equal(rows[i].view(exp.dtype), exp), "corpus window %d of entry %d at %d" % (i, we[i], ws[i])
            # ranges, packed
            rl = rng.integers(0, 25000, size=we.size)
            rl[::7] = 0
            rs = np.array([int(rng.integers(0, max(ns[e] - n, 0) + 1)) for e, n in zip(we, rl)])
            rs[3], rl[3] = ns[we[3]] - 10, 11                           # (runs past its entry)
            out, off, st = corpus.ranges(we, rs, rl)
            pre = np.concatenate([[0], np.cumsum(rl)])
            assert off.cpu().numpy().tolist() == pre.tolist()
            out, st = out.cpu().numpy(), st.cpu().numpy()
            for i in range(we.size):
                row, s = _entry_window(c, ents, int(we[i]), int(rs[i]), int(rl[i]))
                assert st[i] == s and np.array_equal(out[pre[i]:pre[i + 1]], row), "corpus range %d of entry %d" % (i, we[i])
            assert st[3] == BAD
            # levels of every entry, and the quantiles and adaptive events from them
            fst = [c.bad.get(g + i, 0) for g, k in ents for i in range(k)]
            for signal, name in ((B.SAMPLES, "samples"), (B.DIFF, "diff")):
                rec, rf, st = corpus.levels(SPF, signal=name)
                assert rf.tolist() == first.tolist() and st.tolist() == fst
                _same_records(rec, _corpus_levels(c, ents, signal), "corpus levels, " + name)
            lv = _corpus_levels(c, ents, B.SAMPLES)
            q = [100_000, 500_000, 1_000_000]
            val, cnt = corpus.level_quantiles(SPF, x3.LEVEL_KEY_MEAN_SQ, q)
            wv, wc = QR.corpus_quantiles(lv, ns, SPF, QR.MEAN_SQ, q)
            assert np.array_equal(val.cpu().numpy().view(np.uint32), wv) and np.array_equal(cnt.cpu().numpy().view(np.uint32), wc)
            trule, rule = QR.TRule(mean_sq=(500_000, 3, 1, 0)), ER.Rule(join_bins=2, pad_bins=1, max_bins=6)
            thrs = QR.corpus_thresholds(lv, ns, SPF, trule)
            ev, elv = QR.corpus_adaptive_events(lv, ns, SPF, thrs, rule)
            cap = len(ev) + 7
            r = corpus.adaptive_events(SPF, x3.ThresholdRule.make(trule.peak, trule.mean_sq),
                                       x3.EventRule.make(join_bins=2, pad_bins=1, max_bins=6), cap)
            assert len(ev) > 10 and int(r[3]) == len(ev)
            w_en, w_st, w_ln, w_lv = ER.slots(ev, elv, cap, True)
            assert [tuple(int(v) for v in t) for t in r[5].cpu().numpy().reshape(-1).view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == \
                [tuple(t) for t in thrs]
            assert np.array_equal(r[0].cpu().numpy().view(np.uint32), w_en) and np.array_equal(r[1].cpu().numpy().view(np.uint64), w_st)
            assert np.array_equal(r[2].cpu().numpy().view(np.uint32), w_ln)
            assert np.array_equal(x3.event_levels_view(r[4]), w_lv)
            # range levels: bins of 2 000 from starts inside the entries
            ke = np.array([e for e in range(E) if ns[e] >= 40000][::2] + [ENTRY_BAD])
            ks = np.array([int(rng.integers(1, (ns[e] - 25000) // 2000)) * 2000 + (777 if i % 2 else 0) for i, e in enumerate(ke)])
            kl = rng.integers(1, 23000, size=ke.size)
            ks[-1], kl[-1] = 3 * SPF - 7, 2 * SPF + 9                    # (covers the damaged frame)
            ks[0], kl[0] = ns[ke[0]] - 5, 6                              # (runs past its entry)
            for signal, name in ((B.SAMPLES, "samples"), (B.DIFF, "diff")):
                lvs, roff, st = corpus.range_levels(ke, ks, kl, 2000, signal=name)
                got, roff, st = x3.event_levels_view(lvs), roff.cpu().numpy(), st.cpu().numpy()
                for i, (e, s, n) in enumerate(zip(ke, ks, kl)):
                    g, k = ents[e]
                    over = s + n > ns[e]
                    want = LR.empty(max(1, -(-int(n) // 2000))) if over else c.range_levels(g * SPF + int(s), int(n), 2000, signal)
                    assert st[i] == (BAD if over else c.range_status(g * SPF + int(s), int(n))), (name, i)
                    _same_records(got[roff[i]:roff[i + 1]], want, "corpus range levels %d of entry %d, %s" % (i, e, name))
                assert st[0] == BAD and st[-1] == c.bad[ents[ENTRY_BAD][0] + 4]
            # the FIR, tone and bank forms: the filter's history and the oscillators' phase restart at every entry
            fir, tone = x3.Fir(B.FIR8[1], B.FIR8[2]), x3.Tone(TONE_STEP)
            tones = [x3.Tone(v) for v in BANK_STEPS]
            want_fir, want_tone, want_bank = _corpus_signal_refs(big, c, ents)
            rec, rf, st = corpus.levels(SPF, signal=fir)
            assert rf.tolist() == first.tolist() and st.tolist() == fst
            _same_records(rec, want_fir, "corpus FIR levels")
            rec, rf, st = corpus.tone_levels(SPF, tone)
            assert rf.tolist() == first.tolist() and st.tolist() == fst
            _same_records(rec, want_tone, "corpus tone levels")
            rec, rf, st = corpus.tone_bank_levels(SPF, tones)
            assert rf.tolist() == first.tolist() and st.tolist() == fst and rec.shape == want_bank.shape
            for t in range(len(tones)):
                _same_records(rec[t], want_bank[t], "corpus tone bank levels, plane %d" % t)
            sub = [_entry_frames(c, ents, int(e), int(s), int(n)) for e, s, n in zip(ke, ks, kl)]
            over = [s + n > ns[e] for e, s, n in zip(ke, ks, kl)]
            want_st = [BAD if o else c.range_status(ents[e][0] * SPF + int(s), int(n)) for o, e, s, n in zip(over, ke, ks, kl)]
            rows = [max(1, -(-int(n) // 2000)) for n in kl]
            lvs, roff, st = corpus.fir_range_levels(ke, ks, kl, 2000, fir)
            got, roff = x3.event_levels_view(lvs), roff.cpu().numpy()
            assert st.cpu().numpy().tolist() == want_st
            for i, (s, n) in enumerate(zip(ks, kl)):
                want = LR.empty(rows[i]) if over[i] else FRL.one(*sub[i], int(s), int(n), 2000, B.FIR8[1], B.FIR8[2])[0]
                _same_records(got[roff[i]:roff[i + 1]], want, "corpus FIR range levels %d of entry %d" % (i, ke[i]))
            tab = TL.table()
            lvs, roff, st = corpus.tone_range_levels(ke, ks, kl, 2000, tone)
            got, roff = lvs.cpu().numpy().reshape(-1).view(TL.TONE_DTYPE), roff.cpu().numpy()
            assert st.cpu().numpy().tolist() == want_st
            lvb, roffb, stb = corpus.tone_bank_range_levels(ke, ks, kl, 2000, tones)
            gotb = lvb.cpu().numpy().reshape(len(tones), -1).view(TL.TONE_DTYPE)
            assert stb.cpu().numpy().tolist() == want_st and roffb.cpu().numpy().tolist() == roff.tolist() and gotb.shape[1] == got.size
            for i, (s, n) in enumerate(zip(ks, kl)):
                for t, step in enumerate(BANK_STEPS):
                    want = TL.empty(rows[i]) if over[i] else TRL.one(*sub[i], int(s), int(n), 2000, step, tab)[0]
                    _same_records(gotb[t, roff[i]:roff[i + 1]], want, "corpus tone bank range levels %d of entry %d, plane %d" % (i, ke[i], t))
                    if t == 0:
                        _same_records(got[roff[i]:roff[i + 1]], want, "corpus tone range levels %d of entry %d" % (i, ke[i]))
        finally:
            corpus.close()


# ------------------------------------------------------------------------------------------------ S. spectra and band levels

FILL64 = 0x5A5A5A5A5A5A5A5A


def _spectra_ranges(c, n_fft):
    """(offset, len) into the virtual signal as a sample buffer of c.total elements: around element 2^31, below, across and
    above element 2^32, the buffer's end, two that run off it, lengths N - 1, N and 0"""
    N = n_fft
    return [(5, 2100), ((1 << 31) - 100, 2200), (EDGE - 1 - 2500, 2500), (EDGE - 700, 3000), (EDGE, 2500), (EDGE + 12345, 3001),
            (c.total - 2222, 2222), (c.total - 2000, 2001), (c.total + 1, 100), (EDGE - N + 6, N - 1), (EDGE - N // 2, N),
            (EDGE + (1 << 27) + 7, 4000), (EDGE + 1, 0)]


def _compact(c, ranges):
    """the ranges' samples back to back on the host -> (samples, remapped offsets, lens, in_status): a range that runs off the
    buffer keeps its length and carries BAD_ARG in, as the call gives it"""
    parts, offs, at, st = [], [], 0, []
    for o, n in ranges:
        off_end = o > c.total or n > c.total - o
        st.append(BAD if off_end else 0)
        offs.append(at)
        if not off_end:
            parts.append(c.samples(o, o + n))
            at += n
    return np.concatenate(parts + [np.zeros(4096, dtype=np.int16)]), offs, [n for _, n in ranges], st


def _spectra_call(big, ranges, n_fft, hop, fmt, stride, rows_cap, fold=None, out=None):
    """x3_spectra_rows_dev, or with fold = (per_bin, n_bands, plane_stride, bin_band) x3_spectra_levels_dev into out, on
    the virtual signal -> (out on the device, row offsets, statuses, x3_spectra_result)"""
    torch, ctx, x3 = big.torch, big.ctx, big.x3
    n = len(ranges)
    virt = big.virtual()
    d_off, d_len = big.u64([o for o, _ in ranges]), big.u32([l for _, l in ranges])
    ro, st = big.full((n + 1,), -1, torch.int64), big.full((n,), -1, torch.int32)
    rule = x3.SpectraRule(n_fft, hop, fmt, 0, ctx.tone_table_dev())
    if fold is None:
        words = (n_fft // 2 + 1) * (2 if fmt == S.SUMS else 1)
        if out is None:
            out = big.full((rows_cap + 1, words), FILL64 if fmt == S.SUMS else 0x5A5A5A5A, torch.int64 if fmt == S.SUMS else torch.int32)
        big.ready()
        rc = ctx.spectra_rows_dev(virt.data_ptr(), big.case.total, d_off.data_ptr(), d_len.data_ptr(), None, n, rule, stride,
                                  out.data_ptr(), rows_cap, ro.data_ptr(), st.data_ptr())
    else:
        d_map = big.u32(fold[3])
        f = x3.SpectraFold(fold[0], fold[1], fold[2], d_map.data_ptr(), 0)
        big.ready()
        rc = ctx.spectra_levels_dev(virt.data_ptr(), big.case.total, d_off.data_ptr(), d_len.data_ptr(), None, n, rule, f, stride,
                                    out.data_ptr(), rows_cap, ro.data_ptr(), st.data_ptr())
    assert rc == 0, ctx.last_error()
    res = ctx.spectra_result()
    return out, ro.cpu().numpy().view(np.uint64), st.cpu().numpy(), res


def _spectra_result_of(want_st, total):
    bad = np.flatnonzero(want_st)
    return (0, bad.size, int(bad[0]) if bad.size else len(want_st), int(want_st[bad[0]]) & 0xFF if bad.size else 0, total)


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("fmt", [S.SUMS, S.POWER], ids=["sums", "power"])
@pytest.mark.parametrize("n_fft,hop", [(64, 1), (1024, 1029)])
def test_spectra_rows_of_a_buffer_past_2_32_elements(big, n_fft, hop, fmt, padded):
    """x3_spectra_rows_dev on the virtual signal, samples_cap 4.43 G: offsets below, across, at and above element 2^32, the
    buffer's last samples and past them, against spectra_ref on a compacted host copy of the same slices"""
    c = big.case
    assert B.modulo_conditions(c)["samples"] and c.kind[EDGE // TS] == 2      # (a wrapped offset reads another tile)
    ranges = _spectra_ranges(c, n_fft)
    rows = [S.n_rows(l, n_fft, hop) for _, l in ranges]
    assert rows[9] == 0 and rows[10] == 1 and ranges[2][0] + ranges[2][1] == EDGE - 1 and ranges[6][0] + ranges[6][1] == c.total
    r = (EDGE - 1 - ranges[3][0]) // hop              # a frame of the fourth range begins below element 2^32 and ends above it
    assert ranges[7][0] + ranges[7][1] == c.total + 1 and r < rows[3] and ranges[3][0] + r * hop < EDGE < ranges[3][0] + r * hop + n_fft
    stride = max(rows) if padded else 0
    cap = (len(ranges) * stride if padded else sum(rows)) + 3
    host, offs, lens, in_st = _compact(c, ranges)
    want, w_off, w_st, w_total = S.spectra_rows(host, offs, lens, in_st, n_fft, hop, fmt, stride, cap)
    assert w_st.tolist() == [0] * 7 + [BAD, BAD] + [0] * 4
    out, ro, st, res = _spectra_call(big, ranges, n_fft, hop, fmt, stride, cap)
    assert st.tolist() == w_st.tolist() and np.array_equal(ro, w_off), (st, ro, w_off)
    assert res == _spectra_result_of(w_st, w_total), res
    got = out.cpu().numpy()
    got = got.view(np.int64).reshape(cap + 1, -1, 2) if fmt == S.SUMS else got.view(np.uint32)
    assert (got[cap:].view(np.uint8) == 0x5A).all(), "written behind rows_cap"
    if not np.array_equal(got[:cap], want):
        r = np.flatnonzero((got[:cap] != want).reshape(cap, -1).any(axis=1))
        w = int(np.searchsorted(w_off.astype(np.int64), r[0], side="right")) - 1
        raise AssertionError("N %d hop %d: %d rows differ, the first %d (range %d %s)" % (n_fft, hop, r.size, r[0], w, ranges[min(w, len(ranges) - 1)]))


def _band_map(n_fft):
    """three bands, band 1 empty: the bins go to band 0 and 2 in turn, every fifth to no band (a word above K, a wild one)"""
    m = np.where(np.arange(n_fft // 2 + 1) % 2, 2, 0).astype(np.uint32)
    m[::5] = 7
    m[3] = 0xFFFFFFFF
    return m


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("n_fft,hop", [(64, 1), (1024, 1029)])
def test_spectra_levels_planes_past_byte_2_33(big, n_fft, hop, padded):
    """x3_spectra_levels_dev on the ranges above with plane_stride 2^27 + 5 records: planes 1 and 2 begin past byte 2^32 and
    2^33 of a 12.9 GB buffer.  The records the call owns against spectra_levels_ref, every other byte still 0x5A"""
    c, torch = big.case, big.torch
    K, M, ps = 3, 3, (1 << 27) + 5
    assert 32 * ps > EDGE and 64 * ps > 2 * EDGE
    ranges = _spectra_ranges(c, n_fft)
    bins = [SL.n_bins_of(S.n_rows(l, n_fft, hop), M) for _, l in ranges]
    stride = max(bins) if padded else 0
    cap = (len(ranges) * stride if padded else sum(bins)) + 2
    host, offs, lens, in_st = _compact(c, ranges)
    want, w_off, w_st, w_total = SL.spectra_levels(host, offs, lens, in_st, n_fft, hop, M, _band_map(n_fft), K, stride, cap)
    buf = big.full((K * ps, 4), FILL64, torch.int64)
    out, ro, st, res = _spectra_call(big, ranges, n_fft, hop, S.POWER, stride, cap, fold=(M, K, ps, _band_map(n_fft)), out=buf)
    assert st.tolist() == w_st.tolist() and np.array_equal(ro, w_off), (st, ro, w_off)
    assert res == _spectra_result_of(w_st, w_total), res
    for b in range(K):
        got = buf[b * ps:b * ps + cap].cpu().numpy().reshape(-1).view(SL.LEVEL)
        d = first_diff(got, want[b])
        assert not d, ("plane %d" % b, d, got[d[:1]], want[b][d[:1]])
        assert int((buf[b * ps + cap:(b + 1) * ps] != FILL64).sum()) == 0, "written between rows_cap and plane_stride of plane %d" % b
    if not padded:
        assert (want[:, w_total:].view(np.uint8) == 0x5A).all() and w_total == cap - 2    # (so were the records behind the total)


def _sums_ref(big, a, n_rows, n_fft, hop):
    """the SUMS rows of the frames at a + r * hop, r < n_rows, of the virtual signal by a float64 matmul on the device ->
    int64 [n_rows, B, 2].  Exact: every term is an integer below 2^30 in magnitude and a frame has at most 2^10 of them, so
    every partial sum, in any order, stays below 2^40, far inside the 2^53 a float64 holds exactly"""
    torch = big.torch
    basis = torch.from_numpy(S.basis(n_fft).astype(np.float64).reshape(n_fft, -1)).to(big.dev)
    x = big.virtual()[a:a + (n_rows - 1) * hop + n_fft].to(torch.float64).unfold(0, n_fft, hop)
    return (x @ basis).to(torch.int64).view(n_rows, n_fft // 2 + 1, 2)


def _power_ref(big, sums, n_fft):
    """spectra_ref.power_of's integer formula on the device -> int64 [rows, B]"""
    a, b = sums[..., 0] >> 15, sums[..., 1] >> 15
    return (2 * (a * a + b * b) // n_fft // n_fft).clamp_(max=1 << 30)


@pytest.mark.parametrize("fmt", [S.POWER, S.SUMS], ids=["power_past_word_2_32", "sums_past_byte_2_32"])
def test_spectra_rows_output_past_2_32(big, fmt):
    """x3_spectra_rows_dev, n_fft 64 and hop 1, packed.  POWER: 130 150 500 rows of a range that straddles sample 2^32, then
    100 rows of the last place, which begin 24 rows below word 2^32 of the 17.2 GB output and end behind it: windows of 2^20
    rows at the first rows, around words 2^30 and 2^31 and at the first range's last rows, which end 796 words below word
    2^32 -- the crossing itself is held by the second range's 100 rows, the output's last.  SUMS: 8 200 000 rows, 4.33 GB, for
    the byte offset: the first 2^20 rows, the last, and 2^20 rows around byte 2^32 (only 65 593 rows lie behind that byte, so
    this window ends 32 768 rows behind it and overlaps the last).  SUMS past element 2^32 would need 34 GB: left out.  The
    windows against a float64 matmul on the device, 64 rows of each against spectra_ref on the CPU; a canary row behind
    rows_cap survives"""
    c, torch = big.case, big.torch
    N, nb, W = 64, 33, 1 << 20
    if fmt == S.POWER:
        R1 = 130_150_500
        ranges = [(EDGE - 65_000_000, R1 + N - 1), (c.total - 5000, 100 + N - 1)]
        assert R1 + N - 1 < EDGE and R1 * nb < EDGE < (R1 + 100) * nb
        windows = [(0, 0, W), (0, (1 << 30) // nb - W // 2, W), (0, (1 << 31) // nb - W // 2, W), (0, R1 - W, W), (1, 0, 100)]
    else:
        R1 = 8_200_000
        ranges = [(EDGE - 4_100_000, R1 + N - 1)]
        rb = EDGE // (nb * 16)                                 # the row that holds byte 2^32 of the output
        assert R1 - W < rb < R1 - 32768
        windows = [(0, 0, W), (0, rb + 32768 - W, W), (0, R1 - W, W)]
    rows = [S.n_rows(l, N, 1) for _, l in ranges]
    total = sum(rows)
    pre = np.concatenate([[0], np.cumsum(rows)])
    out, ro, st, res = _spectra_call(big, ranges, N, 1, fmt, 0, total)
    assert ro.tolist() == pre.tolist() and st.tolist() == [0] * len(ranges) and res == (0, 0, len(ranges), 0, total), (ro, st, res)
    assert int((out[total] != (FILL64 if fmt == S.SUMS else 0x5A5A5A5A)).sum()) == 0, "the canary row behind rows_cap"
    for w, r0, n in windows:
        a = ranges[w][0] + r0
        want = _sums_ref(big, a, n, N, 1)
        got = out[int(pre[w]) + r0:int(pre[w]) + r0 + n]
        if fmt == S.POWER:
            want = _power_ref(big, want, N).to(torch.int32)
        else:
            got = got.view(n, nb, 2)
        if not torch.equal(got, want):
            d = torch.nonzero((got != want).reshape(n, -1).any(dim=1)).reshape(-1)
            raise AssertionError("range %d, rows from %d: %d rows differ, the first at %d" % (w, r0, d.numel(), r0 + int(d[0])))
        k = min(n, 64)
        cpu = S.sums(c.samples(a + n - k, a + n + N - 1), N, 1)
        cpu = S.power_of(cpu, N).astype(np.int64) if fmt == S.POWER else cpu
        assert np.array_equal(want[n - k:].cpu().numpy().astype(np.int64), cpu), "the device reference, range %d rows from %d" % (w, r0 + n - k)


BL_N, BL_M, BL_EDGES = 256, 32, [1, 9, 40, 41, 129]      # n_fft = hop, frames a row, four bands (the third one bin wide)
BL_LEN = BL_N * BL_M                                       # 8 192 positions a row


def _band_levels_ref(big):
    """WindowSource.band_levels(256, 256, frames_per_bin=32, bands=BL_EDGES) of the clean stream by torch on the device,
    from the virtual signal in chunks of 2^13 rows -> int64 [4, rows, 4]: the words of the level records (sum_sq, sum = 0,
    (min, max), (n, reserved = 0)).  The float64 matmul is exact (sums below 2^38, see _sums_ref)"""
    if "band" in big.refs:
        return big.refs["band"]
    torch, c = big.torch, big.case
    K = len(BL_EDGES) - 1
    m = big.x3.spectra_bin_band(BL_N, BL_EDGES)[0].astype(np.int64)
    keep = torch.from_numpy(np.flatnonzero(m < K)).to(big.dev)
    band = torch.from_numpy(m[m < K]).to(big.dev)
    frames = c.total // BL_N
    rows = -(-c.total // BL_LEN)
    assert frames * BL_N == c.total and frames % BL_M
    out = torch.zeros((K, rows, 4), dtype=torch.int64, device=big.dev)
    for r0 in range(0, rows, 1 << 13):
        nr = min(1 << 13, rows - r0)
        nf = min(nr * BL_M, frames - r0 * BL_M)
        ms = _power_ref(big, _sums_ref(big, r0 * BL_LEN, nf, BL_N, BL_N), BL_N)
        bp = torch.zeros((nr * BL_M, K), dtype=torch.int64, device=big.dev)          # (frames of zeros change neither sum nor max)
        bp[:nf] = torch.zeros((nf, K), dtype=torch.int64, device=big.dev).index_add_(1, band, ms[:, keep]).clamp_(max=1 << 30)
        bp = bp.view(nr, BL_M, K)
        v = 2 * bp.amax(dim=1)
        s = torch.sqrt(v.to(torch.float64)).to(torch.int64)                         # floor square root, in integers from here
        s = s - (s * s > v).to(torch.int64)
        s = s + ((s + 1) * (s + 1) <= v).to(torch.int64)
        assert bool(((s * s <= v) & ((s + 1) * (s + 1) > v)).all())
        peak = s.clamp_(max=32767)
        out[:, r0:r0 + nr, 0] = bp.sum(dim=1).T
        out[:, r0:r0 + nr, 2] = (((-peak) & M32) | (peak << 32)).T
        out[:, r0:r0 + nr, 3] = (frames - torch.arange(r0, r0 + nr, device=big.dev) * BL_M).clamp_(max=BL_M)[None, :]
    big.refs["band"] = out
    return out


def _band_source(big):
    c = big.case
    return big.x3.WindowSource(big.ctx, (big.stream.data_ptr(), c.total_bytes), big.p, seg_blocks=SB, frame_offsets=big.fo.data_ptr(),
                               n_frames=c.F, seg_index=big.seg().data_ptr())


@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
def test_band_levels_of_the_whole_stream(big, damage):
    """WindowSource.band_levels over 4.43 G samples (its range starts are computed on the host): every record of the four
    planes against the torch reference; the rows of the three marked places against spectra_levels_ref on the CPU; with one
    damaged frame above 2^32 exactly the q rows of each range that touches it are the identity.  Then x3_plane_events_dev on
    the planes under a rule that only the loud tile passes: starts above 2^32, equal to plane_events_ref on the reference"""
    torch, c, x3 = big.torch, big.case, big.x3
    K, q = len(BL_EDGES) - 1, 4
    ref = _band_levels_ref(big)
    rows = ref.shape[1]
    f_bad = EDGE // SPF + 3 * FPT + 5
    with big.damaged([divmod(f_bad, FPT)] if damage else []):
        big.ready()
        src = _band_source(big)
        try:
            assert src.total == c.total
            planes = src.band_levels(BL_N, BL_N, frames_per_bin=BL_M, bands=BL_EDGES, q=q)
            assert tuple(planes.shape) == (K, rows, 32)
            got = planes.view(torch.int64)
            want = ref
            if damage:
                g0, g1 = f_bad * SPF // (q * BL_LEN), ((f_bad + 1) * SPF - 1) // (q * BL_LEN)
                assert f_bad * SPF > EDGE and g1 >= g0
                want = ref.clone()
                want[:, q * g0:q * (g1 + 1)] = torch.tensor([0, 0, (32767 & M32) | (-32768 << 32), 0], dtype=torch.int64, device=big.dev)
            _same_words(torch, got.reshape(K * rows, 4), want.reshape(K * rows, 4), "band levels of the whole stream")
            if damage:
                return
            m = x3.spectra_bin_band(BL_N, BL_EDGES)[0]
            for p in _edge_places(c):            # (past position 2^32 the rows hold tile 2's, then the ordinary tiles' content)
                i0, i1 = -(-p * TS // BL_LEN), min((p + 1) * TS // BL_LEN, rows)
                cpu = SL.levels_of(c.samples(i0 * BL_LEN, min(i1 * BL_LEN, c.total)), BL_N, BL_N, BL_M, m, K)
                rec = planes[:, i0:i1].cpu().numpy().reshape(K, -1).view(SL.LEVEL)
                assert np.array_equal(rec, cpu), ("place %d" % p, first_diff(rec.reshape(-1), cpu.reshape(-1)))
            # plane events: a mean square that, in any band, only rows of the last place reach
            i_last = (c.M - 1) * TS // BL_LEN
            ms = ref[:, :, 0] // ref[:, :, 3].clamp(min=1)
            thr = [int(v) + 1 for v in ms[:, :i_last].amax(dim=1).cpu()]
            assert bool((ms[:, i_last + 1:] >= torch.tensor(thr, device=big.dev)[:, None]).any())
            rule = PE.PlaneRule(mean_sq_min=thr, peak_min=[0] * K, min_planes=1, join_bins=2, pad_bins=1)
            r0 = i_last - 16      # (no row below i_last is loud and pad_bins is 1: the rows from r0 on decide every event)
            cpu_planes = np.ascontiguousarray(ref[:, r0:].cpu().numpy()).reshape(K, -1).view(LR.LEVEL_DTYPE)
            ev, elv = PE.stream_plane_events(cpu_planes, c.total - r0 * BL_LEN, BL_LEN, rule)
            ev = [(s + r0 * BL_LEN, n, mask) for s, n, mask in ev]
            cap = len(ev) + 5
            assert 1 <= len(ev) and all(s > EDGE for s, _, _ in ev)
            r = src.plane_events(planes, BL_LEN, x3.PlaneEventRule.make(mean_sq_min=thr, min_planes=1, join_bins=2, pad_bins=1), cap)
            _, w_st, w_ln, w_mk, w_lv = PE.slots(ev, elv, cap, False)
            assert int(r[2]) == len(ev)
            assert np.array_equal(r[0].cpu().numpy().view(np.uint64), w_st) and np.array_equal(r[1].cpu().numpy().view(np.uint32), w_ln)
            assert np.array_equal(r[3].cpu().numpy().view(np.uint32), w_mk)
            assert np.array_equal(r[4].cpu().numpy().reshape(K, -1).view(LR.LEVEL_DTYPE), w_lv)
        finally:
            src.close()


# ------------------------------------------------------------------------------------------------ G. encoders

def _clip(n):
    """mixed content: the head of tile 0 (dense, ordinary and quiet frames)"""
    return B.tiles()[0].wav[:n].copy()


ENCODERS = {
    # name: (block_len, blocks_per_frame, options, enc_gen_in_use, how)
    "wave": (20, 500, {}, 3, "dev"),
    "gen2": (20, 500, {"enc_gen": 2}, 2, "dev"),
    "two_pass": (20, 500, {"two_pass": 1}, 0, "dev"),
    "block_40": (40, 250, {}, None, "dev"),
    "general_33x64": (33, 64, {}, 1, "dev"),
    "frames": (20, 500, {}, None, "frames"),
    "seg": (20, 500, {}, 3, "seg"),
}


@pytest.mark.parametrize("name", list(ENCODERS))
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd"])
def test_encode_at_a_start_pos_across_2_32(big, name, odd):
    """30 frames, the last one ragged, written so that the stream straddles byte 2^32 of a 4.3 GB buffer: the bytes, the end
    position and the frame offsets are the oracle's at a small start_pos of the same parity, shifted; 4 KiB on both sides stay
    untouched"""
    ctx, torch, x3 = big.ctx, big.torch, big.x3
    big.drop_virtual()
    bl, bpf, opts, gen, how = ENCODERS[name]
    spf = bl * bpf
    n = 29 * spf + spf // 3
    wav = _clip(n)
    p, op = x3.Params.make(block_len=bl, blocks_per_frame=bpf), O.Params.make(bl, bpf)
    small = 6 + odd
    rc, ref, st_o = O.encode(wav, op, start_pos=small)
    assert rc == 0
    body = ref[small:]
    start = (EDGE - body.size // 2) // 2 * 2 + odd
    shift = start - small
    cap = start + body.size + 8192
    assert start < EDGE < start + body.size and cap > EDGE
    ref_off = np.array([small + odd] + [small + odd + o for o in RR.frame_offsets(ref[small + odd:])[1:]], dtype=np.int64)
    F = ref_off.size - 1
    assert F == 30
    out = big.full((cap + 64,), 0xA5, torch.uint8)
    d_wav = torch.from_numpy(wav).to(big.dev)
    off = big.full((F + 1 + 8,), -1, torch.int64)
    seg = big.full((x3.lib().x3_seg_index_entries(F, C.byref(p), SB) + 8,), -1, torch.int64)
    old = {k: ctx.get_option(k) for k in opts}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        big.ready()
        if how == "dev":
            rc = ctx.encode_dev(d_wav.data_ptr(), n, p, out.data_ptr(), cap, start, off.data_ptr())
        elif how == "seg":
            rc = ctx.encode_dev_seg(d_wav.data_ptr(), n, p, out.data_ptr(), cap, seg.data_ptr(), SB, start, off.data_ptr())
        else:
            src = np.arange(F, dtype=np.uint64) * np.uint64(spf)
            cnt = np.array([spf] * (F - 1) + [n - (F - 1) * spf], dtype=np.uint32)
            rc = ctx.encode_frames_dev(d_wav.data_ptr(), src, cnt, p, out.data_ptr(), cap, start, off.data_ptr())
        assert rc == 0, ctx.last_error()
        rc, pos, st = ctx.encode_result()
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)
        ctx.set_option("enc_gen", 3)
    assert rc == 0 and pos == start + body.size, (name, rc, pos, start + body.size, ctx.last_error())
    assert st.tolist() == st_o.tolist() and ctx.get_option("encode_fallbacks") == 0
    if gen is not None:
        assert ctx.get_option("enc_gen_in_use") == gen, (name, ctx.get_option("enc_gen_in_use"))
    got = out[start - 4096:pos + 4096].cpu().numpy()
    assert (got[:4096] == 0xA5).all(), "%s: bytes in front of start_pos were written" % name
    assert (got[4096 + body.size:] == 0xA5).all(), "%s: bytes behind the end were written" % name
    assert np.array_equal(got[4096:4096 + body.size], body), (name, first_diff(got[4096:4096 + body.size], body))
    assert not bool((out[:start - 4096] != 0xA5).any()), "%s: a write 4 GiB below" % name
    assert np.array_equal(off[:F + 1].cpu().numpy(), ref_off + shift), (name, off[:4], ref_off[:4] + shift)
    assert int((off[F + 1:] != -1).sum()) == 0
    if how == "seg":
        words, _ = SR.build(ref, ref_off[:-1], op, SB)
        assert np.array_equal(seg[:words.size].cpu().numpy().view(np.uint64), words), "the encoder's segment index"
        assert int((seg[words.size:] != -1).sum()) == 0


@pytest.mark.parametrize("stride", [(1 << 31) + 6, (1 << 31) + 8], ids=["stride_2_31_plus_6", "stride_2_31_plus_8"])
def test_batch_with_a_clip_stride_past_2_31(big, stride):
    """three clips of 50 001 samples, clip_stride samples apart: the third starts past sample 2^32 of d_wav.  Encode against
    the oracle per clip, the tuner on the same batch, and decode back through the batch layout with every gap untouched"""
    ctx, torch, x3 = big.ctx, big.torch, big.x3
    big.drop_virtual()
    n_per, n_clips = 50001, 3
    size = 2 * stride + n_per + 4096
    wav = big.full((size,), FILL16, torch.int16)
    clips = [B.tiles()[k].wav[170000:170000 + n_per].copy() for k in range(3)]
    for k, cl in enumerate(clips):
        wav[k * stride:k * stride + n_per] = torch.from_numpy(cl).to(big.dev)
    assert 2 * stride > EDGE
    refs = [O.encode(cl)[1] for cl in clips]
    ref = np.concatenate(refs)
    F = 6 * n_clips
    out = big.full((ref.size + 4096,), 0xA5, torch.uint8)
    off = big.full((F + 1,), -1, torch.int64)
    big.ready()
    assert ctx.encode_dev(wav.data_ptr(), n_per, big.p, out.data_ptr(), ref.size + 4096, 0, off.data_ptr(), n_clips=n_clips,
                          clip_stride=stride) == 0, ctx.last_error()
    rc, pos, st = ctx.encode_result()
    assert rc == 0 and pos == ref.size, (rc, pos, ref.size)
    got = out.cpu().numpy()
    at = 0
    for k, r in enumerate(refs):
        assert np.array_equal(got[at:at + r.size], r), ("clip %d" % k, first_diff(got[at:at + r.size], r))
        at += r.size
    assert (got[pos:] == 0xA5).all()
    assert off.cpu().numpy().tolist() == RR.frame_offsets(ref)
    # the tuner on the same batch: the sizes of a sample of candidates are the sum of the oracle's over the clips
    tuner = x3.Tuner(ctx)
    try:
        assert tuner.add_dev(wav.data_ptr(), n_per, stride, n_clips) == 0, ctx.last_error()
        rc, best, best_bytes, sizes = tuner.result()
        assert rc == 0
        cand = sorted(set(np.random.default_rng(7).choice(x3.TUNE_CANDIDATES, size=64, replace=False).tolist() + [x3.TUNE_DEFAULT_INDEX]))
        for i in cand:
            rc, tp = x3.tune_candidate(i)
            assert rc == 0
            op = O.Params.make(tp.block_len, tp.blocks_per_frame, (0, 1, 3), tuple(tp.thresholds))
            assert int(sizes[i]) == sum(O.encode(cl, op)[1].size for cl in clips), "tuner candidate %d" % i
        assert int(sizes[x3.TUNE_DEFAULT_INDEX]) == ref.size and best_bytes == int(sizes.min())
    finally:
        tuner.close()
    # back through the batch layout: the clips, and not one sample of the gaps
    back = big.full((size,), FILL16, torch.int16)
    big.ready()
    assert ctx.decode_dev(out.data_ptr(), pos, off.data_ptr(), F, big.p, back.data_ptr(), 2 * stride + n_per, n_per_clip=n_per,
                          n_clips=n_clips, clip_stride=stride) == 0, ctx.last_error()
    assert ctx.decode_result() == (0, F, 0, n_per * n_clips)
    for k in range(n_clips):
        a = k * stride
        assert torch.equal(back[a:a + n_per], wav[a:a + n_per]), "clip %d" % k
        assert int((back[max(a - 2048, 0):a] != FILL16).sum()) == 0 and int((back[a + n_per:a + n_per + 2048] != FILL16).sum()) == 0
    assert torch.equal(back, wav), "a sample of a gap was written"


def test_decode_to_wav_offsets_on_both_sides_of_2_32(big):
    """d_wav_offsets: 30 frames sent to sample offsets that straddle element 2^32 of a large output, in a scattered order"""
    ctx, torch = big.ctx, big.torch
    big.drop_virtual()
    n = 29 * SPF + 3333
    wav = _clip(n)
    ref = O.encode(wav)[1]
    fo = RR.frame_offsets(ref)
    F = len(fo) - 1
    gap = SPF + 24
    order = (np.arange(F) * 7) % F
    wo = EDGE - 15 * gap + order.astype(np.int64) * gap
    assert wo.min() < EDGE < wo.max() and not np.any(wo % 4)
    size = int(wo.max()) + SPF + 4096
    back = big.full((size,), FILL16, torch.int16)
    want_lo = int(wo.min()) - 4096
    stream = torch.from_numpy(np.concatenate([ref, np.zeros(64, dtype=np.uint8)])).to(big.dev)
    d_fo, d_wo = big.u64(fo), big.u64(wo)
    for x4 in (0, 1):
        back[want_lo:] = FILL16
        ctx.set_option("wav_offsets_x4", x4)
        try:
            big.ready()
            assert ctx.decode_dev(stream.data_ptr(), ref.size, d_fo.data_ptr(), F, big.p, back.data_ptr(), size,
                                  d_wav_offsets=d_wo.data_ptr()) == 0, ctx.last_error()
            res = ctx.decode_result()
        finally:
            ctx.set_option("wav_offsets_x4", 0)
        assert res[:3] == (0, F, 0), res
        got = back[want_lo:].cpu().numpy()
        exp = np.full(got.size, FILL16, dtype=np.int16)
        for f in range(F):
            a = int(wo[f]) - want_lo
            fr = wav[f * SPF:(f + 1) * SPF]
            exp[a:a + fr.size] = fr
        assert np.array_equal(got, exp), ("wav_offsets_x4 = %d" % x4, first_diff(got, exp))
        assert not bool((back[:want_lo] != FILL16).any()), "a write 8 GiB below"
