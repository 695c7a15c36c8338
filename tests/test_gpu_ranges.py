"""Ranges (include/x3hip.h, "RANGES"): x3_decode_ranges_dev, x3_corpus_ranges_dev, x3_decode_ranges_result and the Python
surface.  Every sample, offset and status is compared with == against ranges_ref.py, the definition written from the CPU
oracle's decode; every output buffer is filled with 0x5A first and carries canary words behind its end.

The base stream: 2 137 samples in frames of 400 (block length 20, 20 blocks a frame), five whole frames and one of 137.
Its index (seg_blocks 4) is seg_index_ref's, the words x3_encode_dev_seg writes where the encoder fills an index at all
(the default geometry only: tests/async_cases.py holds the two against each other)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_lib as O
import ranges_ref as R
import seg_index_ref as SR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD = R.ERR_BAD_ARG
N, SPF, SB = 2137, 400, 4
LENS = [0, 1, 19, 20, 21, 399, 400, 401, 1000, N]
GUARD = 64          # canary bytes behind every output array


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


class Dev:
    """a stream in HBM with its frame offsets, sample offsets and an index (words, None: none)"""

    def __init__(self, ctx, x3, stream, p, op, index=None, sb=SB):
        self.ctx, self.x3, self.p, self.op, self.stream = ctx, x3, p, op, stream
        self.offs = R.frame_offsets(stream)
        self.F, self.len = len(self.offs) - 1, stream.size
        self.bufs = []
        self.d_x3, self.d_off, self.d_so = self.alloc(stream.size), self.alloc(8 * (self.F + 1)), self.alloc(8 * (self.F + 1))
        ctx.upload(self.d_x3, stream)
        ctx.upload(self.d_off, np.array(self.offs, dtype=np.uint64))
        assert ctx.sample_offsets_dev(self.d_x3, self.len, self.d_off, self.F, self.d_so) == 0
        self.so = ctx.download(self.d_so, 8 * (self.F + 1), np.uint64)
        self.total = int(self.so[-1])
        self.sb = sb
        self.d_seg = None
        if index is not None:
            self.d_seg = self.alloc(8 * index.size)
            ctx.upload(self.d_seg, index)

    def alloc(self, n):
        q = self.ctx.alloc(max(n, 8))
        self.bufs.append(q)
        return q

    def frames(self, so=None):
        return R.frames_of(self.stream, self.offs, self.op, so)

    def call(self, d_starts, d_lens, n, stride, d_out, cap, fmt, d_off, d_status, seg=True, d_so=None):
        idx = self.d_seg if seg else None
        return self.ctx.decode_ranges_dev(self.d_x3, self.len, self.d_off, d_so or self.d_so, self.F, self.p, d_starts,
                                          d_lens, n, stride, d_out, cap, fmt, d_off, d_status, idx, self.sb if idx else 0)

    def close(self):
        for q in self.bufs:
            self.ctx.free(q)


def run(ctx, enqueue, starts, lens, stride, cap, fmt, guard=GUARD, entries=None):
    """one call -> (out [cap] as int16 / uint32 bits, offsets, status, total); the result call and the canaries are checked"""
    starts = np.array([int(s) for s in starts], dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    n, esz = starts.size, 4 if fmt else 2
    sizes = (esz * cap, 8 * (n + 1), 4 * n)
    bufs = [ctx.alloc(max(s + guard, 8)) for s in sizes] + [ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)]
    d_out, d_off, d_status, d_starts, d_lens, d_ent = bufs
    try:
        for q, s in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(s + guard, 0x5A, dtype=np.uint8))
        ctx.upload(d_starts, starts)
        ctx.upload(d_lens, lens)
        args = (d_starts, d_lens, n, stride, d_out, cap, fmt, d_off, d_status)
        if entries is not None:
            ctx.upload(d_ent, np.array(entries, dtype=np.uint32))
            args = (d_ent,) + args
        rc = enqueue(*args)
        assert rc == 0, ctx.last_error()
        res = ctx.decode_ranges_result()
        raw = [ctx.download(q, s + guard) for q, s in zip(bufs[:3], sizes)]
    finally:
        for q in bufs:
            ctx.free(q)
    for name, a, s in zip(("d_out", "d_out_offsets", "d_status"), raw, sizes):
        assert (a[s:] == 0x5A).all(), "the canary behind %s is damaged" % name
    out = raw[0][:sizes[0]].view(np.uint32 if fmt else np.int16)
    off, st = raw[1][:sizes[1]].view(np.uint64), raw[2][:sizes[2]].view(np.int32)
    bad = np.nonzero(st)[0]
    assert res[:4] == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0), res
    return out, off, st, res[4]


def expect(frames, so, starts, lens, stride, cap, fmt):
    """ranges_ref's answer in the output's bits; positions nobody may write keep the 0x5A fill"""
    a, off, st = R.ranges(frames, so, starts, lens, stride, cap, 0x5A5A)
    if fmt:
        b = R.ranges(frames, so, starts, lens, stride, cap, 0x1111)[0]
        a = np.where(a == b, R.f32_bits(a), np.uint32(0x5A5A5A5A))
    return a, off, st


def check(ctx, dev, frames, so, starts, lens, stride, cap, fmt, **kw):
    got = run(ctx, lambda *a: dev.call(*a, **kw), starts, lens, stride, cap, fmt)
    want = expect(frames, so, starts, lens, stride, cap, fmt)
    assert np.array_equal(got[2], want[2]), (np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert got[3] == sum(int(v) for v in lens)
    return got


# ------------------------------------------------------------------------------------------------ the base stream

def base_wav(x3):
    return x3.synth(2, 1616, 0, N)


def base(ctx, x3, index="ref", bl=20, bpf=20, codes=(0, 1, 3)):
    op = O.Params.make(bl, bpf, codes, (3, 8, 20))
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    rc, s, _ = O.encode(base_wav(x3), op)
    assert rc == 0
    words = SR.build(s, R.frame_offsets(s)[:-1], op, SB)[0] if index == "ref" else None
    return Dev(ctx, x3, s, p, op, words)


def base_ranges(total=N, seed=1):
    """every length at every start of the issue's list, shuffled, with repeats and overlaps"""
    rng = np.random.default_rng(seed)
    out = []
    for ln in LENS:
        starts = {0, total - 1, 2 ** 63}
        for b in range(SPF, total, SPF):
            starts |= {b - 1, b, b + 1}
        starts |= {max(total - ln, 0), max(total - ln, 0) + 1}        # ending exactly at the total, and one past it
        out += [(s, ln) for s in starts]
    out += [out[i] for i in rng.integers(0, len(out), 20)]              # repeats
    out += [(total, 0), (total + 1, 0)]                                 # a length of 0 at the total and behind it
    rng.shuffle(out)
    return [s for s, _ in out], [ln for _, ln in out]


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("stride", [0, 1024])
@pytest.mark.parametrize("seg", [True, False])
def test_base_stream_every_length_at_every_boundary(ctx, x3, seg, stride, fmt):
    dev = base(ctx, x3)
    assert dev.total == N and dev.F == 6 and dev.so.tolist() == [0, 400, 800, 1200, 1600, 2000, 2137]
    starts, lens = base_ranges()
    cap = len(starts) * stride if stride else sum(lens)
    frames = dev.frames()
    assert all(st == 0 for st, _ in frames)
    out, off, st, _ = check(ctx, dev, frames, dev.so, starts, lens, stride, cap, fmt, seg=seg)
    assert (st != 0).any() and (st == 0).any()
    if stride:
        assert all(st[w] == BAD for w, ln in enumerate(lens) if ln > stride)     # (the whole stream: longer than the stride)
    assert ctx.get_option("last_window_replays") == 0
    dev.close()


def test_ranges_agree_with_the_window_call(ctx, x3):
    dev = base(ctx, x3)
    starts, lens = base_ranges()
    out, off, st, _ = run(ctx, dev.call, starts, lens, 0, sum(lens), 0)
    for L in (19, 400, 1000):
        ws = [w for w, ln in enumerate(lens) if ln == L]
        n = len(ws)
        d_st, d_rows, d_status = ctx.alloc(8 * n), ctx.alloc(2 * n * L), ctx.alloc(4 * n)
        ctx.upload(d_st, np.array([starts[w] for w in ws], dtype=np.uint64))
        assert ctx.decode_windows_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_st, n, L, d_rows, 0, d_status,
                                      dev.d_seg, SB) == 0
        assert ctx.decode_ranges_result()[0] == BAD            # (the pending call is a windows call)
        assert ctx.decode_windows_result()[0] == 0
        rows = ctx.download(d_rows, 2 * n * L, np.int16).reshape(n, L)
        wst = ctx.download(d_status, 4 * n, np.int32)
        for k, w in enumerate(ws):
            assert wst[k] == st[w] and np.array_equal(rows[k], out[int(off[w]):int(off[w]) + L]), (L, starts[w])
        for q in (d_st, d_rows, d_status):
            ctx.free(q)
    dev.close()


def capacity_case(ctx, x3, guard):
    """a packed capacity in the middle of a range (also run under the fence, with guard 0: buffers that end at their mapping)"""
    dev = base(ctx, x3)
    starts, lens = base_ranges(seed=2)
    off = np.concatenate([[0], np.cumsum(lens)])
    k = next(w for w in range(len(lens) // 2, len(lens)) if lens[w] > 1)
    cap = int(off[k]) + lens[k] // 2
    for fmt in (0, 1):
        got = run(ctx, dev.call, starts, lens, 0, cap, fmt, guard=guard)
        want = expect(dev.frames(), dev.so, starts, lens, 0, cap, fmt)
        for g, w in zip(got[:3], want):
            assert np.array_equal(g, w)
        assert got[3] == int(off[-1]) and int(got[1][-1]) == int(off[-1])       # complete, whatever fits
        assert got[2][k] == BAD and all(got[2][w] == BAD for w in range(k, len(lens)) if off[w] + lens[w] > cap)
    dev.close()
    return cap


def test_packed_capacity_in_the_middle_of_a_range(ctx, x3):
    assert capacity_case(ctx, x3, GUARD) > 0


def test_packed_capacity_under_the_fence():
    env = dict(os.environ, X3HIP_FENCE="16", X3HIP_FENCE_FILL="165")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x3-rust_amd"), HERE, env.get("PYTHONPATH", "")])
    code = """
        import x3hip, test_gpu_ranges as T
        ctx = x3hip.Context(0)
        print("cap", T.capacity_case(ctx, x3hip, 0))
        ctx.close()
        """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-15:])
    assert r.returncode == 0, "child under the fence ended with %d:\n%s" % (r.returncode, tail)
    assert int(r.stdout.split("cap")[1]) > 0


# ------------------------------------------------------------------------------------------------ damage

@pytest.mark.parametrize("stride", [0, 1024])
def test_a_flipped_payload_byte_in_frame_3(ctx, x3, stride):
    clean = base(ctx, x3)
    s = clean.stream.copy()
    s[clean.offs[3] + 20 + 30] ^= 0x08
    dev = Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, 0, R.ERR_PAYLOAD_CRC, 0, 0]
    starts, lens = base_ranges(seed=3)
    cap = len(starts) * stride if stride else sum(lens)
    for fmt in (0, 1):
        out, off, st, _ = check(ctx, dev, frames, dev.so, starts, lens, stride, cap, fmt)
        for w, (s0, ln) in enumerate(zip(starts, lens)):
            covers = ln and s0 < 1600 and s0 + ln > 1200 and s0 + ln <= N
            if ln <= (stride or ln):
                assert (st[w] == R.ERR_PAYLOAD_CRC) == bool(covers), (s0, ln, st[w])
    clean.close()
    dev.close()


def test_a_contradicted_and_a_zeroed_index(ctx, x3):
    dev = base(ctx, x3)
    nw = SR.n_words(6, dev.op, SB)
    good = ctx.download(dev.d_seg, 8 * nw, np.uint64)
    starts, lens = base_ranges(seed=4)
    frames = dev.frames()
    per = (nw - 1) // 6
    bad = good.copy()
    bad[1 + 2 * per + 1] += np.uint64(1)               # frame 2, entry 2: one bit late
    ctx.upload(dev.d_seg, bad)
    check(ctx, dev, frames, dev.so, starts, lens, 0, sum(lens), 0)
    assert ctx.get_option("last_window_replays") > 0
    ctx.upload(dev.d_seg, np.zeros(nw, dtype=np.uint64))
    check(ctx, dev, frames, dev.so, starts, lens, 1024, 1024 * len(starts), 1)
    assert ctx.get_option("last_window_replays") == 0
    dev.close()


def test_sample_offsets_of_another_stream(ctx, x3):
    dev = base(ctx, x3)
    so = np.array([0, 300, 600, 900, 1200, 1500, 1637], dtype=np.uint64)     # frames of 300; the last frame agrees
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    frames = dev.frames(so)
    assert [st for st, _ in frames] == [BAD] * 5 + [0]
    starts, lens = base_ranges(total=1637, seed=5)
    out, off, st, _ = check(ctx, dev, frames, so, starts, lens, 0, sum(lens), 0, d_so=d_so)
    assert all(st[w] == BAD for w, (s0, ln) in enumerate(zip(starts, lens)) if ln and s0 < 1500)
    dev.close()


# ------------------------------------------------------------------------------------------------ scan, parameters

def test_more_ranges_than_threads_of_the_scan(ctx, x3):
    dev = base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 6, 3000).tolist()
    starts = rng.integers(0, N - 4, 3000).tolist()
    out, off, st, total = check(ctx, dev, dev.frames(), dev.so, starts, lens, 0, sum(lens), 0)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)) and total == sum(lens)
    dev.close()


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_range_counts_round_the_threads_of_the_scan(ctx, x3, n):
    """x3_range_scan_kernel's workgroup of 1 024 walks a run of ranges per thread: one each up to 1 024, then two, three at
    2 049.  Packed with room for all, packed with the last ranges left without room, padded."""
    dev = base(ctx, x3)
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 4, n).tolist()
    starts = rng.integers(0, N - 3, n).tolist()
    frames = dev.frames()
    check(ctx, dev, frames, dev.so, starts, lens, 0, sum(lens), 0)
    check(ctx, dev, frames, dev.so, starts, lens, 0, sum(lens) - 4, 0)
    check(ctx, dev, frames, dev.so, starts, lens, 4, 4 * n, 1)
    dev.close()


def test_block_length_40_with_a_walk_built_index(ctx, x3):
    dev = base(ctx, x3, index=None, bl=40, bpf=10)
    ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), SB)
    assert ne > 0
    dev.d_seg = dev.alloc(8 * ne)
    assert ctx.seg_index_build_dev(dev.d_x3, dev.len, dev.d_off, dev.F, dev.p, dev.d_seg, SB) == 0
    starts, lens = base_ranges(seed=7)
    frames = dev.frames()
    assert all(st == 0 for st, _ in frames)
    check(ctx, dev, frames, dev.so, starts, lens, 0, sum(lens), 0)
    assert ctx.get_option("last_window_replays") == 0
    check(ctx, dev, frames, dev.so, starts, lens, 1024, 1024 * len(starts), 1)
    dev.close()


def test_codes_1_1_3(ctx, x3):
    dev = base(ctx, x3, index=None, codes=(1, 1, 3))
    starts, lens = base_ranges(seed=8)
    check(ctx, dev, dev.frames(), dev.so, starts, lens, 0, sum(lens), 0, seg=False)     # (the oracle's verdicts, whatever they are)
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

ENTRY_SAMPLES = (137, 400, 801, 2000, 5003)


def test_corpus_ranges_equal_the_stream_form_on_each_entry(ctx, x3):
    op = O.Params.make(20, 20)
    p = x3.Params.make(block_len=20, blocks_per_frame=20)
    ents, parts, offsets, pos = [], [], [], 0
    for e, n in enumerate(ENTRY_SAMPLES):
        rc, s, _ = O.encode(x3.synth(2, 900 + e, 0, n), op)
        assert rc == 0
        pad = np.zeros(1 if pos % 2 == 0 else 2, dtype=np.uint8)           # (odd byte offsets)
        parts += [pad, s]
        offsets.append(pos + pad.size)
        pos += pad.size + s.size
        ents.append(s)
    assert all(o % 2 == 1 for o in offsets)
    buf = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf, offsets, [s.size for s in ents], params=p, seg_blocks=SB, index="walk")
    assert corpus.entries["n_samples"].tolist() == list(ENTRY_SAMPLES)
    rng = np.random.default_rng(9)
    tab = [(e, 0, n) for e, n in enumerate(ENTRY_SAMPLES)]                       # the whole of every entry in one call
    tab += [(e, 1, n) for e, n in enumerate(ENTRY_SAMPLES)]                      # one past the entry's end
    tab += [(5, 0, 10), (2 ** 32 - 1, 0, 0), (0, 137, 0), (0, 138, 0), (4, 4999, 4), (4, 2 ** 63, 1)]
    for _ in range(40):
        e = int(rng.integers(0, 5))
        ln = int(rng.integers(0, min(ENTRY_SAMPLES[e], 900) + 1))
        tab.append((e, int(rng.integers(0, ENTRY_SAMPLES[e] - ln + 1)), ln))
    rng.shuffle(tab)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    devs = [Dev(ctx, x3, s, p, op, None) for s in ents]
    for stride, fmt in ((0, 0), (0, 1), (5003, 0), (1024, 1)):
        cap = len(tab) * stride if stride else sum(lens)
        out, off, st, total = run(ctx, corpus.ranges_into, starts, lens, stride, cap, fmt, entries=ent)
        assert total == sum(lens)
        assert off.tolist() == ([w * stride for w in range(len(tab) + 1)] if stride else
                                np.concatenate([[0], np.cumsum(lens)]).tolist())
        for w, (e, s0, ln) in enumerate(tab):
            row = out[int(off[w]):int(off[w]) + (stride or ln)]
            if e >= 5:
                assert st[w] == BAD and not row.any(), (e, s0, ln)             # an entry that is not in the corpus
                continue
            one = run(ctx, lambda *a: devs[e].call(*a, seg=False), [s0], [ln], stride, stride or ln, fmt)
            want = expect(devs[e].frames(), devs[e].so, [s0], [ln], stride, stride or ln, fmt)
            assert one[2][0] == want[2][0] and np.array_equal(one[0], want[0])
            assert st[w] == one[2][0] and np.array_equal(row, one[0]), (e, s0, ln, st[w])
    for d in devs:
        d.close()
    corpus.close()


# ------------------------------------------------------------------------------------------------ surface

def test_argument_refusals_enqueue_nothing(ctx, x3):
    dev = base(ctx, x3)
    n = 4
    sizes = {"out": 2 * 64, "off": 8 * (n + 1), "st": 4 * n}
    d = {k: dev.alloc(v) for k, v in sizes.items()}
    d_starts, d_lens = dev.alloc(8 * n), dev.alloc(4 * n)
    ctx.upload(d_starts, np.zeros(n, dtype=np.uint64))
    ctx.upload(d_lens, np.full(n, 16, dtype=np.uint32))
    for k, v in sizes.items():
        ctx.upload(d[k], np.full(v, 0x5A, dtype=np.uint8))
    Rg = ctx.decode_ranges_dev
    a = (dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p)
    ok = dict(d_starts=d_starts, d_lens=d_lens, n_ranges=n, row_stride=0, d_out=d["out"], out_cap=64, out_format=0,
              d_out_offsets=d["off"], d_status=d["st"], d_seg_index=dev.d_seg, seg_blocks=SB)
    refusals = [dict(n_ranges=0), dict(n_ranges=2 ** 31), dict(d_starts=None), dict(d_lens=None), dict(d_out=None),
                dict(d_status=None), dict(d_out_offsets=None), dict(d_starts=d_starts + 4), dict(d_lens=d_lens + 2),
                dict(d_out=d["out"] + 1), dict(d_out=d["out"] + 2, out_format=1), dict(d_out_offsets=d["off"] + 4),
                dict(d_status=d["st"] + 2), dict(out_format=2), dict(seg_blocks=3), dict(seg_blocks=0),
                dict(row_stride=17, out_cap=64)]                       # 4 rows of 17 do not fit 64
    for r in refusals:
        assert Rg(*a, **dict(ok, **r)) == BAD, r
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert Rg(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, bad_p, **ok) != 0           # parameters the window calls refuse
    assert Rg(dev.d_x3, dev.len, dev.d_off + 4, dev.d_so, dev.F, dev.p, **ok) == BAD
    # the corpus form: its own pointer, and the shared refusals through its entry
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, row_stride=0, d_out=d["out"], out_cap=64, fmt=0,
               d_out_offsets=d["off"], d_status=d["st"])
    crefusals = [dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(n=2 ** 31), dict(d_starts=None),
                 dict(d_lens=None), dict(d_out=None), dict(d_status=None), dict(d_out_offsets=None),
                 dict(d_starts=d_starts + 4), dict(d_lens=d_lens + 2), dict(d_out=d["out"] + 1),
                 dict(d_out=d["out"] + 2, fmt=1), dict(d_out_offsets=d["off"] + 4), dict(d_status=d["st"] + 2), dict(fmt=2),
                 dict(row_stride=17, out_cap=64)]
    for r in crefusals:
        assert corpus.ranges_into(**dict(cok, **r)) == BAD, r
    ctx.graph_begin()
    try:
        assert Rg(*a, **ok) == BAD                                       # a context that records a graph
        assert corpus.ranges_into(**cok) == BAD
    finally:
        try:
            ctx.graph_destroy(ctx.graph_end())
        except x3.X3Error:
            pass                                                         # (a recording of nothing)
    assert ctx.decode_ranges_result()[0] == BAD                          # nothing is pending
    ctx.sync()
    for k, v in sizes.items():
        assert (ctx.download(d[k], v) == 0x5A).all(), k
    assert Rg(*a, **dict(ok, row_stride=16, d_out_offsets=None)) == 0    # padded: the offsets may be NULL
    assert ctx.decode_windows_result()[0] == BAD                         # (the pending call is a ranges call)
    assert ctx.decode_ranges_result() == (0, 0, n, 0, 64)
    assert (ctx.download(d["off"], sizes["off"]) == 0x5A).all()
    assert np.array_equal(ctx.download(d["out"], 128, np.int16), np.tile(base_wav(x3)[:16], 4))
    assert corpus.ranges_into(**cok) == 0                                # (what the corpus refusals were cut from is a good call)
    assert ctx.decode_windows_result()[0] == BAD                         # (the corpus form's pending call is a ranges call too)
    assert ctx.decode_ranges_result() == (0, 0, n, 0, 64)
    corpus.close()
    dev.close()


def test_torch_surface_of_window_source_and_corpus(ctx, x3):
    import torch
    wav = base_wav(x3)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    p = x3.Params.make(block_len=20, blocks_per_frame=20)
    src = x3.WindowSource(ctx, s, p, seg_blocks=SB, index="walk")
    starts = torch.tensor([0, 399, 2000, 2137, 5], dtype=torch.int64, device="cuda")
    lens = torch.tensor([400, 3, 137, 0, 3000], dtype=torch.int32, device="cuda")
    out, off, st = src.ranges(starts, lens)
    assert out.is_cuda and off.is_cuda and st.is_cuda and out.dtype == torch.int16
    assert off.tolist() == [0, 400, 403, 540, 540, 3540] and st.tolist() == [0, 0, 0, 0, BAD]
    assert np.array_equal(out[:540].cpu().numpy(), np.concatenate([wav[:400], wav[399:402], wav[2000:]]))
    assert not out[540:].any()
    out, off, st = src.ranges([0, 399], [400, 3], padded_to=512, dtype=torch.float32)
    assert out.shape == (2, 512) and off.tolist() == [0, 512, 1024] and st.tolist() == [0, 0]
    assert np.array_equal(out[1].cpu().numpy().view(np.uint32), R.f32_bits(np.concatenate([wav[399:402], np.zeros(509, np.int16)])))
    out, off, st = src.ranges(starts, lens, capacity=402)
    assert st.tolist() == [0, BAD, BAD, BAD, BAD] and off[-1].item() == 3540 and out.numel() == 402
    src.close()
    corpus = x3.Corpus(ctx, s, [0], [s.size], params=p, seg_blocks=SB, index="walk")
    out, off, st = corpus.ranges([0, 0, 1], [2000, 0, 0], [137, 2137, 1])
    assert st.tolist() == [0, 0, BAD] and off.tolist() == [0, 137, 2274, 2275]
    assert np.array_equal(out[:2274].cpu().numpy(), np.concatenate([wav[2000:], wav]))
    corpus.close()


# ------------------------------------------------------------------------------------------------ async

def _ranges_case():
    import async_cases as A

    class RangesPair(A.Case):
        """x3_sample_offsets_dev, then x3_decode_ranges_dev packed (int16) and padded (float): the stream, its frame offsets,
        the starts and the lengths are device data and arrive behind the stall"""
        name = "ranges_pair"
        W, STRIDE = 64, 4096

        def __init__(self):
            a, b = A.padded([A.encoded("A")[0], A.encoded("B")[0]])
            self.x3 = {"A": a, "B": b}
            self.len = a.size

        def table(self, which):
            rng = np.random.default_rng({"A": 30, "B": 40}[which])
            lens = rng.integers(0, self.STRIDE + 1, size=self.W).astype(np.uint32)       # (their sum fits CAP)
            starts = np.array([rng.integers(0, A.N0 - int(n) + 1) for n in lens], dtype=np.uint64)
            return starts, lens

        CAP = 64 * 4096

        def inputs(self, which):
            s, n = self.table(which)
            return {"x3": self.x3[which], "off": A.encoded(which)[1], "starts": s, "lens": n}

        def outputs(self):
            return {"so": 8 * (A.F0 + 1), "rows1": 2 * self.CAP, "off1": 8 * (self.W + 1), "st1": 4 * self.W,
                    "rows2": 4 * self.W * self.STRIDE, "st2": 4 * self.W}

        def enqueue(self, x3, ctx, d, which, probe):
            p = x3.Params.default()
            assert ctx.sample_offsets_dev(d["x3"], self.len, d["off"], A.F0, d["so"]) == 0
            assert ctx.decode_ranges_dev(d["x3"], self.len, d["off"], d["so"], A.F0, p, d["starts"], d["lens"], self.W, 0,
                                         d["rows1"], self.CAP, x3.WINDOW_I16, d["off1"], d["st1"]) == 0, ctx.last_error()
            assert ctx.decode_ranges_dev(d["x3"], self.len, d["off"], d["so"], A.F0, p, d["starts"], d["lens"], self.W,
                                         self.STRIDE, d["rows2"], self.W * self.STRIDE, x3.WINDOW_F32, None, d["st2"]) == 0

        def results(self, x3, ctx, d, which):
            return {"ranges": tuple(ctx.decode_ranges_result())}

        def expect(self, which):
            w = A.wav(which)
            starts, lens = self.table(which)
            off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
            r1 = [(2 * int(o), w[int(s):int(s) + int(n)], False) for o, s, n in zip(off, starts, lens) if n]
            r2 = np.zeros((self.W, self.STRIDE), dtype=np.int16)
            for k, (s, n) in enumerate(zip(starts, lens)):
                r2[k, :int(n)] = w[int(s):int(s) + int(n)]
            z = np.zeros(self.W, dtype=np.int32)
            so = np.arange(A.F0 + 1, dtype=np.uint64) * np.uint64(A.SPF)
            out = {"so": [(0, so, False)], "rows1": r1, "off1": [(0, off, False)], "st1": [(0, z, False)],
                   "rows2": [(0, A.f32_bits(r2), False)], "st2": [(0, z, False)]}
            return {"out": out, "result": {"ranges": (0, 0, self.W, 0, int(off[-1]))}}

        same_ok = {"so": "both contents are cut into the same full frames", "st1": "intact streams", "st2": "intact streams"}

        def valid(self, which):
            starts, lens = self.table(which)
            assert all(int(s) + int(n) <= A.N0 for s, n in zip(starts, lens)) and int(lens.sum()) <= self.CAP
            assert int(lens.max()) <= self.STRIDE and int(A.encoded(which)[1][-1]) <= self.len

    return A, RangesPair()


def test_a_ranges_call_behind_a_stalled_stream_returns_before_the_stall_ends(x3):
    import torch
    A, case = _ranges_case()
    A.check_pair_differs(case)
    A.run_stalled(x3, torch, case, A.calibrate_sleep(torch))
