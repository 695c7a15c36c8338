"""Random access (include/x3hip.h, "RANDOM ACCESS"): x3_sample_offsets_dev, x3_decode_windows_dev, WindowSource, the C++
mirror.  Every window is held against the samples the stream was encoded from, or against the oracle's decode_stream /
decode_frame of the same bytes: a window is the slice [start, start + L) of what a clean decode returns, and a window that
a failing frame covers is exact in front of that frame and zero behind it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 24
LENGTHS = [1, 19, 20, 640, 10_000, 192_000]


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _f32(a):
    return (np.asarray(a, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).view(np.uint32)


def _frame_offsets(stream):
    offs = [0]
    while offs[-1] < stream.size:
        offs.append(offs[-1] + 20 + ((int(stream[offs[-1] + 6]) << 8) | int(stream[offs[-1] + 7])))
    return offs


class Dev:
    """a stream in HBM with its frame offsets, sample offsets and (optionally) the encoder's segment index"""

    def __init__(self, ctx, x3, stream=None, wav=None, p=None, sb=32, encode_seg=True):
        self.ctx, self.x3, self.p = ctx, x3, p or x3.Params.default()
        self.bufs = []
        L = x3.lib()
        if stream is None:
            n = wav.size
            self.F = L.x3_num_frames(n, C.byref(self.p))
            cap = L.x3_encode_bound(n, C.byref(self.p))
            d_wav = self.alloc(2 * n + 64)
            self.d_x3 = self.alloc(cap + 64)
            self.d_off = self.alloc(8 * (self.F + 1))
            ctx.upload(d_wav, wav)
            ne = L.x3_seg_index_entries(self.F, C.byref(self.p), sb) if sb else 0
            self.d_seg = self.alloc(8 * ne) if ne else None
            if self.d_seg and encode_seg:
                assert ctx.encode_dev_seg(d_wav, n, self.p, self.d_x3, cap, self.d_seg, sb, 0, self.d_off) == 0
            else:
                assert ctx.encode_dev(d_wav, n, self.p, self.d_x3, cap, 0, self.d_off) == 0
            rc, self.len, _ = ctx.encode_result()
            assert rc == 0
        else:
            offs = _frame_offsets(stream)
            self.F = len(offs) - 1
            self.len = stream.size
            self.d_x3 = self.alloc(stream.size + 64)
            self.d_off = self.alloc(8 * (self.F + 1))
            ctx.upload(self.d_x3, stream)
            ctx.upload(self.d_off, np.array(offs, dtype=np.uint64))
            self.d_seg = None
        self.sb = sb if self.d_seg else 0
        self.d_so = self.alloc(8 * (self.F + 1))
        assert ctx.sample_offsets_dev(self.d_x3, self.len, self.d_off, self.F, self.d_so) == 0
        self.so = ctx.download(self.d_so, 8 * (self.F + 1), np.uint64)
        self.total = int(self.so[-1])

    def alloc(self, n):
        p = self.ctx.alloc(max(n, 8))
        self.bufs.append(p)
        return p

    def windows(self, starts, L, fmt=0, seg=True, d_seg=None, d_off=None, d_so=None):
        starts = np.array([int(s) for s in starts], dtype=np.uint64)
        n = starts.size
        esz = 4 if fmt else 2
        d_st, d_out, d_status = self.ctx.alloc(8 * n), self.ctx.alloc(esz * n * L), self.ctx.alloc(4 * n)
        try:
            self.ctx.upload(d_st, starts)
            self.ctx.upload(d_out, np.full(esz * n * L, 0x5A, dtype=np.uint8))   # (every sample must be written)
            idx = d_seg if d_seg is not None else (self.d_seg if seg else None)
            rc = self.ctx.decode_windows_dev(self.d_x3, self.len, d_off or self.d_off, d_so or self.d_so, self.F, self.p,
                                             d_st, n, L, d_out, fmt, d_status, idx, self.sb if idx else 0)
            assert rc == 0, self.ctx.last_error()
            res = self.ctx.decode_windows_result()
            self.replays = self.ctx.get_option("last_window_replays")
            rows = self.ctx.download(d_out, esz * n * L, np.uint32 if fmt else np.int16).reshape(n, L)
            st = self.ctx.download(d_status, 4 * n, np.int32)
        finally:
            for q in (d_st, d_out, d_status):
                self.ctx.free(q)
        bad = np.nonzero(st)[0]
        assert res == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0)
        return rows, st

    def close(self):
        for q in self.bufs:
            self.ctx.free(q)


def _starts(total, L, rng, spf=10_000):
    last = total - L
    s = {0, last, min(last, 12_345), min(last, max(0, spf - L // 2)), min(last, max(0, 3 * spf - 7))}
    s.update(int(v) for v in rng.integers(0, last + 1, 4))
    return sorted(s)


def _check_exact(dev, wav, L, starts, seg=True, d_seg=None, replays=0):
    """windows of an intact stream are its samples; `replays`: (window, frame) pairs re-decoded by the reference's reader
    (none: every stretch's proof holds; None: not asserted)"""
    for fmt in (0, 1):
        rows, st = dev.windows(starts, L, fmt, seg=seg, d_seg=d_seg)
        assert not st.any(), (L, st)
        if replays is not None:
            assert dev.replays == replays, (L, fmt, dev.replays)
        for r, s in zip(rows, starts):
            want = wav[s:s + L]
            if fmt:
                assert np.array_equal(r, _f32(want)), (L, s)
            else:
                assert np.array_equal(r, want), (L, s)


@pytest.mark.parametrize("sb", [32, 64])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_windows_are_slices_of_the_input_encoders_index(ctx, x3, kind, sb):
    n = 250_003
    wav = x3.synth(kind, 77 + kind, 0, n)
    dev = Dev(ctx, x3, wav=wav, sb=sb)
    assert dev.total == n and int(dev.so[1]) == 10_000
    rng = np.random.default_rng(kind * 100 + sb)
    for L in LENGTHS + [n]:
        _check_exact(dev, wav, L, _starts(n, L, rng))
    dev.close()


def test_windows_without_an_index_and_with_a_none_index(ctx, x3):
    n = 123_457
    wav = x3.synth(2, 5, 0, n)
    dev = Dev(ctx, x3, wav=wav, sb=32)
    none = dev.alloc(8 * x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), 32))
    ctx.upload(none, np.zeros(x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), 32), dtype=np.uint64))
    rng = np.random.default_rng(3)
    for L in (1, 640, 10_000, 60_000, n):
        st = _starts(n, L, rng)
        _check_exact(dev, wav, L, st, seg=False)
        _check_exact(dev, wav, L, st, d_seg=none)
    dev.close()


def test_batches_of_ragged_clips(ctx, x3):
    """x3_encode_frames_dev: clips of different lengths, each cut as encoder::encode cuts it; windows across clip ends"""
    clips = [x3.synth(2, 11, 0, 12_345), x3.synth(3, 12, 0, 10_000), x3.synth(4, 13, 0, 7), x3.synth(1, 14, 0, 30_001),
             x3.synth(2, 15, 0, 4_999)]
    wav = np.concatenate(clips)
    so, sn, base = [], [], 0
    for c in clips:
        for a in range(0, c.size, 10_000):
            so.append(base + a)
            sn.append(min(10_000, c.size - a))
        base += c.size
    p = x3.Params.default()
    F = len(so)
    cap = sum(x3.lib().x3_encode_bound(c.size, C.byref(p)) for c in clips) + 64
    d_wav, d_out, d_off = ctx.alloc(2 * wav.size + 64), ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    ctx.upload(d_wav, wav)
    assert ctx.encode_frames_dev(d_wav, so, sn, p, d_out, cap, 0, d_off) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    stream = ctx.download(d_out, pos)
    rc, ref, fok, ferr = O.decode_stream(stream, wav_cap=wav.size + 10)
    assert rc == 0 and np.array_equal(ref, wav)
    src = x3.WindowSource(ctx, stream, p)
    assert src.n_frames == F and src.total == wav.size
    rng = np.random.default_rng(8)
    for L in (1, 20, 641, 10_000, 20_000, wav.size):
        starts = sorted({0, wav.size - L, min(wav.size - L, 12_340), min(wav.size - L, 22_344)} |
                        set(int(v) for v in rng.integers(0, wav.size - L + 1, 5)))
        for fmt in (0, 1):
            rows, st = src.decode(starts, L, fmt)
            assert not st.any()
            for r, s in zip(rows, starts):
                want = ref[s:s + L]
                assert np.array_equal(r.view(np.uint32) if fmt else r, _f32(want) if fmt else want), (L, s)
    src.close()
    for q in (d_wav, d_out, d_off):
        ctx.free(q)


def test_a_foreign_stream_index_dev_sample_offsets_recorded_index(ctx, x3):
    """a stream somebody else wrote (the oracle's encoder): x3_index_dev, x3_sample_offsets_dev, a recording decode"""
    n = 333_333
    wav = x3.synth(2, 31, 0, n)
    rc, stream, _ = O.encode(wav)
    assert rc == 0
    src = x3.WindowSource(ctx, stream)
    assert src.total == n and src.d_seg_index is not None
    seg = ctx.download(src.d_seg_index, 8, np.uint64)
    assert int(seg[0]) == (32 << 32) | 0x58335347   # (recorded: the index is in use)
    rng = np.random.default_rng(4)
    for L in LENGTHS + [n]:
        starts = _starts(n, L, rng)
        for fmt in (0, 1):
            rows, st = src.decode(starts, L, fmt)
            assert not st.any()
            for r, s in zip(rows, starts):
                assert np.array_equal(r.view(np.uint32) if fmt else r, _f32(wav[s:s + L]) if fmt else wav[s:s + L])
    src.close()


def test_a_broken_index_costs_time_not_correctness(ctx, x3):
    n = 400_000
    wav = x3.synth(2, 4242, 0, n)
    dev = Dev(ctx, x3, wav=wav, sb=64)
    ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), 64)
    good = ctx.download(dev.d_seg, 8 * ne, np.uint64)
    other = Dev(ctx, x3, wav=x3.synth(3, 1, 0, n), sb=64)
    foreign = ctx.download(other.d_seg, 8 * ne, np.uint64)
    other.close()
    rng = np.random.default_rng(5)
    cases = []
    a = good.copy(); a[1:] = 0; cases.append(("header but no entry", a))
    a = good.copy(); a[3] += 1; cases.append(("one bit late", a))
    a = good.copy(); a[10] -= 1; cases.append(("one bit early", a))
    a = good.copy(); a[17] = (a[17] & ~np.uint64(0xFFFFFFFF)) | np.uint64(8 * 30000); cases.append(("behind the payload", a))
    a = good.copy(); a[20] ^= np.uint64(1 << 32); cases.append(("wrong sample", a))
    a = good.copy(); a[8:15] = good[15:22]; cases.append(("shifted entries", a))
    a = foreign.copy(); cases.append(("another stream's index", a))
    a = good.copy(); a[::3] = rng.integers(0, 1 << 49, a[::3].size, dtype=np.uint64); a[0] = good[0]; cases.append(("random thirds", a))
    a = rng.integers(0, 1 << 63, good.size, dtype=np.uint64); a[0] = good[0]; cases.append(("all random", a))
    a = good.copy(); a[1::2] ^= np.uint64(1 << 5); cases.append(("flipped bits", a))
    d_bad = dev.alloc(8 * ne)
    for name, idx in cases:
        ctx.upload(d_bad, idx)
        for L in (640, 25_000):
            _check_exact(dev, wav, L, _starts(n, L, rng), d_seg=d_bad, replays=None)
    dev.close()


def _expected_frames(stream, offs, op=None):
    """per frame (oracle parameters op, default if None): (status, samples) as the oracle's reader gives them (header CRC, payload CRC,
    decode_frame)"""
    out = []
    for f in range(len(offs) - 1):
        h = stream[offs[f]:offs[f] + 20]
        samples = (int(h[4]) << 8) | int(h[5])
        plen = (int(h[6]) << 8) | int(h[7])
        payload = stream[offs[f] + 20:offs[f] + 20 + plen]
        if O.crc16(h[:16].tobytes()) != ((int(h[16]) << 8) | int(h[17])):
            out.append((13, None)); continue
        if O.crc16(payload.tobytes()) != ((int(h[18]) << 8) | int(h[19])):
            out.append((14, None)); continue
        rc, w = O.decode_frame(payload, samples, op)
        out.append((rc, w if rc == 0 else None))
    return out


def _expected_window(frames, so, s, L):
    row = np.zeros(L, dtype=np.int16)
    f = int(np.searchsorted(so, s, side="right")) - 1
    while f < len(frames) and int(so[f]) < s + L:
        st, w = frames[f]
        a, b = int(so[f]), int(so[f + 1])
        if st:
            return row, st
        lo, hi = max(a, s), min(b, s + L)
        row[lo - s:hi - s] = w[lo - a:hi - a]
        f += 1
    return row, 0


def test_damaged_streams_first_failing_frame(ctx, x3):
    n = 200_000
    wav = x3.synth(2, 99, 0, n)
    rc, clean, _ = O.encode(wav)
    offs = _frame_offsets(clean)
    p = x3.Params.default()
    so = np.arange(0, n + 1, 10_000, dtype=np.uint64)
    so[-1] = n
    damaged = []
    s = clean.copy(); s[offs[3] + 20 + 500] ^= 0x10; damaged.append(("payload byte (CRC)", s))
    s = clean.copy(); s[offs[5] + 1] ^= 0x01; damaged.append(("header byte", s))
    s = clean.copy()
    a, plen = offs[7] + 20, (int(clean[offs[7] + 6]) << 8) | int(clean[offs[7] + 7])
    s[a + 2000:a + 2040] = 0           # a zero run: an index of the inverse table out of range
    c = O.crc16(s[a:a + plen].tobytes())
    s[offs[7] + 18], s[offs[7] + 19] = c >> 8, c & 0xFF
    damaged.append(("valid-CRC corrupt payload", s))
    rng = np.random.default_rng(6)
    for name, stream in damaged:
        frames = _expected_frames(stream, offs)
        assert any(st for st, _ in frames), name
        # (the caller knows where the frames are: a walk of the damaged stream would stop at a damaged header)
        d_off = ctx.alloc(8 * len(offs))
        ctx.upload(d_off, np.array(offs, dtype=np.uint64))
        src = x3.WindowSource(ctx, stream, p, frame_offsets=d_off, n_frames=len(offs) - 1)
        assert src.total == n
        for L in (1, 640, 10_000, 35_000):
            starts = sorted({0, n - L} | set(int(v) for v in rng.integers(0, n - L + 1, 12)) |
                            {max(0, 10_000 * k - L // 2) for k in (3, 4, 5, 6, 7, 8)})
            for fmt in (0, 1):
                rows, st = src.decode(starts, L, fmt)
                for r, s0, got in zip(rows, starts, st):
                    want, wst = _expected_window(frames, so, s0, L)
                    assert got == wst, (name, L, s0, got, wst)
                    assert np.array_equal(r.view(np.uint32) if fmt else r, _f32(want) if fmt else want), (name, L, s0)
        src.close()
        ctx.free(d_off)
    # a header sample count that disagrees with the caller's offsets: X3_ERR_BAD_ARG from that frame on
    dev = Dev(ctx, x3, stream=clean)
    bad_so = dev.so.copy()
    bad_so[4] += 2   # frames 3 and 4 disagree with their headers
    d_so = dev.alloc(8 * bad_so.size)
    ctx.upload(d_so, bad_so)
    starts = [0, 25_000, 29_990, 35_000, 45_000, 50_000, 150_000]
    rows, st = dev.windows(starts, 10_000, d_so=d_so)
    for r, s0, got in zip(rows, starts, st):
        if s0 + 10_000 <= 30_000 or s0 >= int(bad_so[5]):
            assert got == 0 and np.array_equal(r, wav[s0:s0 + 10_000]), (s0, got)
        else:
            assert got == BAD, (s0, got)
            cut = max(0, 30_000 - s0)
            assert np.array_equal(r[:cut], wav[s0:s0 + cut]) and not r[cut:].any()
    dev.close()


def test_wild_starts_offsets_and_host_arguments(ctx, x3):
    n = 100_000
    wav = x3.synth(4, 3, 0, n)
    dev = Dev(ctx, x3, wav=wav, sb=32)
    L = 1000
    starts = [0, n - L + 1, 2 ** 63, 2 ** 64 - 1, 5000, n - L, 2 ** 64 - L]
    for fmt in (0, 1):
        rows, st = dev.windows(starts, L, fmt)
        for r, s0, got in zip(rows, starts, st):
            if s0 <= n - L:
                assert got == 0 and np.array_equal(r.view(np.uint32) if fmt else r, _f32(wav[s0:s0 + L]) if fmt else wav[s0:s0 + L])
            else:
                assert got == BAD and not r.any(), (s0, got)
    # wild frame offsets: that frame fails, nothing faults
    offs = ctx.download(dev.d_off, 8 * (dev.F + 1), np.uint64)
    for wild in (dev.len + 100, 2 ** 63, 2 ** 64 - 1, dev.len - 3):
        o = offs.copy(); o[4] = wild
        d_o = dev.alloc(8 * o.size)
        ctx.upload(d_o, o)
        starts = [0, 35_000, 39_000, 45_000, 80_000]
        rows, st = dev.windows(starts, 10_000, d_off=d_o)
        for r, s0, got in zip(rows, starts, st):
            if s0 + 10_000 <= 40_000 or s0 >= 50_000:
                assert got == 0 and np.array_equal(r, wav[s0:s0 + 10_000])
            else:
                assert got != 0
                cut = max(0, 40_000 - s0)
                assert np.array_equal(r[:cut], wav[s0:s0 + cut]) and not r[cut:].any()
    # non-monotone sample offsets: frame errors, no fault
    so = dev.so.copy(); so[3], so[6] = so[6], so[3]
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    rows, st = dev.windows([0, 25_000, 45_000, 65_000, 85_000], 10_000, d_so=d_so)
    assert st[0] == 0 and np.array_equal(rows[0], wav[:10_000])
    assert all(v in (0, BAD) for v in st)
    so = np.zeros_like(dev.so); so[-1] = n
    ctx.upload(d_so, so)
    rows, st = dev.windows([0, 50_000, n - 1000], 1000, d_so=d_so)
    assert (st == BAD).all() or st.any()
    # host argument errors: X3_ERR_BAD_ARG, nothing enqueued
    d_st, d_out, d_status = dev.alloc(8), dev.alloc(64), dev.alloc(4)
    ctx.upload(d_st, np.zeros(1, dtype=np.uint64))
    W = ctx.decode_windows_dev
    args = (dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_st)
    assert W(*args, 1, 0, d_out, 0, d_status) == BAD                       # window_len 0
    assert W(*args, 0, 4, d_out, 0, d_status) == BAD                       # no window
    assert W(*args, 1, 4, d_out, 7, d_status) == BAD                       # unknown format
    assert W(*args, 1, 4, d_out + 1, 0, d_status) == BAD                   # misaligned int16 rows
    assert W(*args, 1, 4, d_out + 2, 1, d_status) == BAD                   # misaligned float rows
    assert W(*args, 1, 4, d_out, 0, d_status, dev.d_seg, 3) == BAD         # seg_blocks not a multiple of 4
    assert W(*args, 1, 4, d_out, 0, d_status, dev.d_seg, 0) == BAD         # an index without seg_blocks
    assert ctx.decode_windows_result()[0] == BAD                            # (nothing pending)
    dev.close()


@pytest.mark.parametrize("bl,bpf,codes", [(10, 500, (0, 1, 3)), (40, 500, (0, 1, 3)), (20, 100, (0, 1, 3)),
                                          (20, 256, (0, 1, 3)), (20, 501, (0, 1, 3)), (20, 500, (1, 2, 3)),
                                          (20, 500, (0, 2, 3)), (13, 77, (0, 1, 3))])
def test_other_parameter_sets(ctx, x3, bl, bpf, codes):
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    n = 150_001
    wav = x3.synth(2, bl * 1000 + bpf, 0, n)
    op = O.Params.make(bl, bpf, codes, (3, 8, 20))
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    # (the reference's decoder hard-wires the sub-code widths of block types 2 and 3: with other code sets its frames are
    # decode errors or other samples -- the oracle's per-frame verdicts are the expectation, whatever they are)
    offs = _frame_offsets(stream)
    frames = _expected_frames(stream, offs, op)
    so = np.zeros(len(offs), dtype=np.uint64)
    for f in range(len(offs) - 1):
        so[f + 1] = so[f] + ((int(stream[offs[f] + 4]) << 8) | int(stream[offs[f] + 5]))
    if codes == (0, 1, 3):
        assert all(st == 0 for st, _ in frames) and np.array_equal(np.concatenate([w for _, w in frames]), wav)
    for sb in (32, 0):
        src = x3.WindowSource(ctx, stream, p, seg_blocks=sb)
        rng = np.random.default_rng(bl + bpf)
        for L in (1, 20, 997, 20_000):
            starts = _starts(n, L, rng, spf=bl * bpf)
            for fmt in (0, 1):
                rows, st = src.decode(starts, L, fmt)
                for r, s0, got in zip(rows, starts, st):
                    want, wst = _expected_window(frames, so, s0, L)
                    assert got == wst, (sb, L, s0, got, wst)
                    assert np.array_equal(r.view(np.uint32) if fmt else r, _f32(want) if fmt else want), (sb, L, s0)
        src.close()


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_window_counts_round_the_threads_of_the_scan(ctx, x3, n):
    """x3_window_scan_kernel's workgroup of 1 024 walks a run of windows per thread: one each up to 1 024, then two, three
    at 2 049.  Windows of 1 to 3 samples over six frames of 400 (the last of 137)."""
    total = 2137
    wav = x3.synth(2, 1616, 0, total)
    rc, stream, _ = O.encode(wav, O.Params.make(20, 20, (0, 1, 3), (3, 8, 20)))
    assert rc == 0
    dev = Dev(ctx, x3, stream=stream, p=x3.Params.make(block_len=20, blocks_per_frame=20, codes=(0, 1, 3)))
    assert dev.F == 6 and dev.total == total
    rng = np.random.default_rng(n)
    for L in (1, 2, 3):
        _check_exact(dev, wav, L, rng.integers(0, total - L + 1, n).tolist(), seg=False, replays=None)
    dev.close()


def test_full_size_1024_random_one_second_windows(ctx, x3):
    """config 3's size: 691.2 M samples (1 h at 192 kHz), 1 024 random one-second windows in both formats"""
    n, L, nw, kind, seed = 691_200_000, 192_000, 1024, x3.SYNTH_HYDROPHONE, 0x58330003
    p = x3.Params.default()
    F = x3.lib().x3_num_frames(n, C.byref(p))
    cap = x3.lib().x3_encode_bound(n, C.byref(p))
    ne = x3.lib().x3_seg_index_entries(F, C.byref(p), 32)
    d_wav, d_x3, d_off, d_seg = ctx.alloc(2 * n), ctx.alloc(cap), ctx.alloc(8 * (F + 1)), ctx.alloc(8 * ne)
    d_so, d_st, d_out, d_status = ctx.alloc(8 * (F + 1)), ctx.alloc(8 * nw), ctx.alloc(4 * nw * L), ctx.alloc(4 * nw)
    try:
        ctx.synth_dev(kind, seed, 0, n, d_wav)
        assert ctx.encode_dev_seg(d_wav, n, p, d_x3, cap, d_seg, 32, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        assert ctx.sample_offsets_dev(d_x3, pos, d_off, F, d_so) == 0
        starts = np.sort(np.random.default_rng(9).integers(0, n - L + 1, nw)).astype(np.uint64)
        ctx.upload(d_st, starts)
        for fmt in (0, 1):
            assert ctx.decode_windows_dev(d_x3, pos, d_off, d_so, F, p, d_st, nw, L, d_out, fmt, d_status, d_seg, 32) == 0
            assert ctx.decode_windows_result() == (0, 0, nw, 0)
            rows = ctx.download(d_out, (4 if fmt else 2) * nw * L, np.uint32 if fmt else np.int16).reshape(nw, L)
            for w in range(0, nw, 1 if fmt == 0 else 8):
                want = x3.synth(kind, seed, int(starts[w]), L)
                assert np.array_equal(rows[w], _f32(want) if fmt else want), (fmt, w)
    finally:
        for q in (d_wav, d_x3, d_off, d_seg, d_so, d_st, d_out, d_status):
            ctx.free(q)


def test_a_window_call_leaves_the_pending_decode_alone(ctx, x3):
    n = 100_000
    wav = x3.synth(2, 2, 0, n)
    rc, stream, _ = O.encode(wav)
    stream = stream.copy()
    offs = _frame_offsets(stream)
    stream[offs[6] + 20 + 100] ^= 0x40   # frame 6: payload CRC
    dev = Dev(ctx, x3, stream=stream)
    d_back = dev.alloc(2 * n)
    assert ctx.decode_dev(dev.d_x3, dev.len, dev.d_off, dev.F, dev.p, d_back, n, n_per_clip=n) == 0
    rows, st = dev.windows([0, 20_000], 5_000)
    assert not st.any() and np.array_equal(rows[1], wav[20_000:25_000])
    rc, first_bad, status, before = ctx.decode_result()
    assert (rc, first_bad, status, before) == (0, 6, 14, 60_000)
    dev.close()


def test_window_source_from_host_bytes(ctx, x3):
    n = 54_321
    wav = x3.synth(3, 8, 0, n)
    rc, stream, _ = O.encode(wav)
    src = x3.WindowSource(ctx, stream)
    rows, st = src.decode([0, 1, n - 300], 300, x3.WINDOW_F32)
    assert not st.any()
    assert np.array_equal(rows.view(np.uint32), np.stack([_f32(wav[s:s + 300]) for s in (0, 1, n - 300)]))
    rows, st = src.decode([n - 299], 300)
    assert st.tolist() == [BAD] and not rows.any()
    src.close()


def test_x3_hpp_decode_windows():
    """tests/host_cpp/test_windows_hpp.cpp: device::decode_windows of the C++ mirror"""
    import x3hip
    O.lib()
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_windows_hpp.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_windows_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
