"""Range levels (include/x3hip.h, "RANGE LEVELS"): x3_range_levels_dev, x3_corpus_range_levels_dev, x3_range_levels_result
and the Python surface.  Every record, offset and status is compared with == against range_levels_ref.py, the definition
written from the CPU oracle's decode (all five fields are integers: no tolerance anywhere); every output array is filled
with 0x5A first and carries canary bytes behind its end.

The base stream is tests/test_gpu_ranges.py's: 2 137 samples in frames of 400 (block length 20, 20 blocks a frame), five
whole frames and one of 137; its index (seg_blocks 4) is seg_index_ref's."""
import ctypes as C

import numpy as np
import pytest

import events_ref as ER
import levels_ref as LR
import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR
import seg_index_ref as SR
from x3_cases import refresh_crcs

pytestmark = pytest.mark.gpu

BAD = R.ERR_BAD_ARG
CRC = RR.ERR_PAYLOAD_CRC
N, SPF, SB = 2137, 400, 4
LENS = [0, 1, 19, 20, 21, 399, 400, 401, 1000, N]
BINS = [0, 1, 7, 20, 399, 400, 401, 1000, 2 ** 32, 2 ** 40]
GUARD = 64          # canary bytes behind every output array
REC = LR.LEVEL_DTYPE.itemsize


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
        self.offs = RR.frame_offsets(stream)
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
        self._frames = {}

    def alloc(self, n):
        q = self.ctx.alloc(max(n, 8))
        self.bufs.append(q)
        return q

    def frames(self, so=None):
        key = None if so is None else tuple(int(v) for v in so)
        if key not in self._frames:
            self._frames[key] = RR.frames_of(self.stream, self.offs, self.op, so)
        return self._frames[key]

    def call(self, d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status, seg=True, d_so=None):
        idx = self.d_seg if seg else None
        return self.ctx.range_levels_dev(self.d_x3, self.len, self.d_off, d_so or self.d_so, self.F, self.p, d_starts, d_lens,
                                         n, bin_len, stride, d_levels, cap, d_off, d_status, idx, self.sb if idx else 0)

    def levels(self, bin_len, n_bins, seg=True):
        """x3_levels_dev on the stream -> (LEVEL_DTYPE [n_bins], frame status)"""
        d_lv, d_st = self.alloc(REC * n_bins), self.alloc(4 * self.F)
        idx = self.d_seg if seg else None
        assert self.ctx.levels_dev(self.d_x3, self.len, self.d_off, self.d_so, self.F, self.p, bin_len, d_lv, n_bins, d_st, idx,
                                   self.sb if idx else 0) == 0
        assert self.ctx.levels_result()[0] == 0
        return self.ctx.download(d_lv, REC * n_bins, LR.LEVEL_DTYPE), self.ctx.download(d_st, 4 * self.F, np.int32)

    def close(self):
        for q in self.bufs:
            self.ctx.free(q)


def run(ctx, enqueue, starts, lens, bin_len, stride, cap, guard=GUARD, entries=None):
    """one call -> (records uint8 [cap, 32], offsets, status, total rows); the result call and the canaries are checked"""
    starts = np.array([int(s) for s in starts], dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    n = starts.size
    sizes = (REC * cap, 8 * (n + 1), 4 * n)
    bufs = [ctx.alloc(max(s + guard, 8)) for s in sizes] + [ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)]
    d_lv, d_off, d_status, d_starts, d_lens, d_ent = bufs
    try:
        for q, s in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(s + guard, 0x5A, dtype=np.uint8))
        ctx.upload(d_starts, starts)
        ctx.upload(d_lens, lens)
        args = (d_starts, d_lens, n, bin_len, stride, d_lv, cap, d_off, d_status)
        if entries is not None:
            ctx.upload(d_ent, np.array(entries, dtype=np.uint32))
            args = (d_ent,) + args
        rc = enqueue(*args)
        assert rc == 0, ctx.last_error()
        res = ctx.range_levels_result()
        raw = [ctx.download(q, s + guard) for q, s in zip(bufs[:3], sizes)]
    finally:
        for q in bufs:
            ctx.free(q)
    for name, a, s in zip(("d_levels", "d_row_offsets", "d_status"), raw, sizes):
        assert (a[s:] == 0x5A).all(), "the canary behind %s is damaged" % name
    out = raw[0][:sizes[0]].reshape(cap, REC)
    off, st = raw[1][:sizes[1]].view(np.uint64), raw[2][:sizes[2]].view(np.int32)
    bad = np.nonzero(st)[0]
    assert res[:4] == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0), res
    return out, off, st, res[4]


def same(got, want, what=""):
    """records (uint8 [rows, 32]) equal, byte for byte; the first rows that differ are named"""
    if not np.array_equal(got, want):
        rows = np.flatnonzero((got != want).any(axis=1))[:4]
        raise AssertionError("%s records %s: got %s, want %s" % (what, rows.tolist(), [R.view(got[r:r + 1])[0] for r in rows],
                                                                  [R.view(want[r:r + 1])[0] for r in rows]))


def check(ctx, dev, frames, so, starts, lens, bin_len, stride, cap, **kw):
    got = run(ctx, lambda *a: dev.call(*a, **kw), starts, lens, bin_len, stride, cap)
    want = R.range_levels(frames, so, starts, lens, bin_len, stride, cap)
    assert np.array_equal(got[2], want[2]), (np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
    assert np.array_equal(got[1], want[1])
    same(got[0], want[0], (bin_len, stride))
    assert got[3] == sum(R.rows_of(v, bin_len) for v in lens)
    return got


def rows_total(lens, bin_len):
    return sum(R.rows_of(v, bin_len) for v in lens)


# ------------------------------------------------------------------------------------------------ the base stream

def base_wav(x3):
    return x3.synth(2, 1616, 0, N)


def base(ctx, x3, index="ref", bl=20, bpf=20, codes=(0, 1, 3)):
    op = O.Params.make(bl, bpf, codes, (3, 8, 20))
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    rc, s, _ = O.encode(base_wav(x3), op)
    assert rc == 0
    words = SR.build(s, RR.frame_offsets(s)[:-1], op, SB)[0] if index == "ref" else None
    dev = Dev(ctx, x3, s, p, op, words)
    if index == "walk":
        ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(p), SB)
        assert ne > 0
        dev.d_seg = dev.alloc(8 * ne)
        assert ctx.seg_index_build_dev(dev.d_x3, dev.len, dev.d_off, dev.F, p, dev.d_seg, SB) == 0
    return dev


def base_ranges(total=N, seed=1):
    """every length at 0, at every frame edge and one either side of it, at the total and at total - len (and one behind it),
    shuffled, with repeats and overlaps"""
    rng = np.random.default_rng(seed)
    out = []
    for ln in LENS:
        starts = {0, total - 1, total, 2 ** 63}
        for b in range(SPF, total, SPF):
            starts |= {b - 1, b, b + 1}
        starts |= {max(total - ln, 0), max(total - ln, 0) + 1}
        out += [(s, ln) for s in starts]
    out += [out[i] for i in rng.integers(0, len(out), 12)]              # repeats
    out += [(total, 0), (total + 1, 0)]                                 # a length of 0 at the total and behind it
    rng.shuffle(out)
    return [s for s, _ in out], [ln for _, ln in out]


@pytest.mark.parametrize("bin_len", BINS)
@pytest.mark.parametrize("index", ["ref", None, "walk"])
def test_every_length_at_every_boundary_at_every_bin_length(ctx, x3, index, bin_len):
    dev = base(ctx, x3, index)
    assert dev.total == N and dev.F == 6 and dev.so.tolist() == [0, 400, 800, 1200, 1600, 2000, 2137]
    starts, lens = base_ranges()
    frames = dev.frames()
    assert all(st == 0 for st, _ in frames)
    out, off, st, _ = check(ctx, dev, frames, dev.so, starts, lens, bin_len, 0, rows_total(lens, bin_len), seg=index is not None)
    assert (st == BAD).any() and (st == 0).any()
    assert ctx.get_option("last_range_levels_replays") == 0 and ctx.get_option("last_range_levels_overflow") == 0
    dev.close()


# ------------------------------------------------------------------------------------------------ layouts

def test_packed_capacity_in_the_middle_of_a_range(ctx, x3):
    dev = base(ctx, x3)
    starts, lens = base_ranges(seed=2)
    for bin_len in (20, 0):
        rows = [R.rows_of(v, bin_len) for v in lens]
        off = np.concatenate([[0], np.cumsum(rows)])
        k = next(w for w in range(len(lens) // 2, len(lens)) if rows[w] > 1) if bin_len else len(lens) // 2
        cap = int(off[k]) + rows[k] // 2
        out, goff, st, total = check(ctx, dev, dev.frames(), dev.so, starts, lens, bin_len, 0, cap)
        assert total == int(off[-1]) and int(goff[-1]) == int(off[-1])                 # complete, whatever fits
        assert all(st[w] == BAD for w in range(len(lens)) if off[w] + rows[w] > cap)
        if bin_len:
            assert st[k] == BAD and (out[int(off[k]):] == 0x5A).all()                  # the cut range and all behind it
        assert any(st[w] == 0 for w in range(k))
    dev.close()


def test_padded_strides_equal_to_above_and_below_the_most_rows(ctx, x3):
    dev = base(ctx, x3)
    starts, lens = base_ranges(seed=3)
    bin_len = 100
    most = max(R.rows_of(v, bin_len) for v in lens)
    assert most == 22
    for stride in (most, most + 9, 5, 1):
        out, off, st, _ = check(ctx, dev, dev.frames(), dev.so, starts, lens, bin_len, stride, len(starts) * stride)
        assert off.tolist() == [w * stride for w in range(len(starts) + 1)]
        for w, ln in enumerate(lens):
            if R.rows_of(ln, bin_len) > stride:
                assert st[w] == BAD and np.array_equal(R.view(out[w * stride:(w + 1) * stride]), LR.empty(stride))
    check(ctx, dev, dev.frames(), dev.so, starts, lens, 0, 1, len(starts) + 3)         # one bin a range, room to spare
    dev.close()


def test_off_the_end(ctx, x3):
    dev = base(ctx, x3)
    starts = [N + 1, 2 ** 64 - 1, 0, 1, N, N, N - 1, 2 ** 63, 0]
    lens = [0, 1, N + 1, N, 0, 1, 2, 2 ** 32 - 1, 2 ** 32 - 1]
    for bin_len, stride in ((2 ** 20, 0), (0, 0), (2 ** 31, 2), (1000, 3)):
        rows = rows_total(lens, bin_len)
        out, off, st, _ = check(ctx, dev, dev.frames(), dev.so, starts, lens, bin_len, stride, len(lens) * stride or rows)
        assert st.tolist() == [BAD, BAD, BAD, BAD, 0, BAD, BAD, BAD, BAD]
    dev.close()


# ------------------------------------------------------------------------------------------------ damage

DAMAGE_RANGES = ([0, 100, 799, 800, 900, 1199, 700, 0, 799, 1200, 1201, 1600, 1199],
                 [800, 50, 1, 400, 100, 1, 600, N, 402, 400, 936, 537, 2])     # before, in, across, behind frame 2


def _damage_check(ctx, dev, frames, so=None, d_so=None, total=N):
    so = dev.so if so is None else so
    starts, lens = base_ranges(total=total, seed=4)
    starts, lens = list(DAMAGE_RANGES[0]) + starts, list(DAMAGE_RANGES[1]) + lens
    got = None
    for bin_len, stride in ((7, 0), (400, 0), (0, 0), (100, 25)):
        cap = len(starts) * stride or rows_total(lens, bin_len)
        got = check(ctx, dev, frames, so, starts, lens, bin_len, stride, cap, d_so=d_so)
    return starts, lens, got


def test_a_payload_crc_failure_in_frame_2(ctx, x3):
    clean = base(ctx, x3)
    s = clean.stream.copy()
    s[clean.offs[2] + 20 + 30] ^= 0x08
    dev = Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, CRC, 0, 0, 0]
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == CRC) == bool(covers), (s0, ln, st[w])
    # the frames behind the bad one still count: (700, 600) at bins of 100 is 100 samples, four empty bins, 100 samples
    w = 6
    assert (starts[w], lens[w]) == (700, 600) and R.view(out[w * 25:w * 25 + 6])["n"].tolist() == [100, 0, 0, 0, 0, 100]
    assert ctx.get_option("last_range_levels_replays") == 0
    clean.close()
    dev.close()


def test_a_decode_error_under_a_valid_crc_in_frame_2(ctx, x3):
    clean = base(ctx, x3)
    s = clean.stream.copy()
    o = clean.offs[2]
    plen = int(s[o + 6]) << 8 | int(s[o + 7])
    payload = s[o + 20:o + 20 + plen].copy()
    rc2 = 0
    for at in range(40, plen - 16, 37):                       # (tests/async_cases.py: a zero run until the frame fails)
        s[o + 20:o + 20 + plen] = payload
        s[o + 20 + at:o + 20 + at + 12] = 0
        rc2 = O.decode_frame(s[o + 20:o + 20 + plen], 400, clean.op)[0]
        if rc2:
            break
    assert rc2, "no zero run made frame 2 fail to decode"
    refresh_crcs(s, o)
    dev = Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, rc2, 0, 0, 0] and rc2 not in (CRC, BAD)
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    assert ctx.get_option("last_range_levels_replays") > 0     # its stretches cannot tell: the reader does
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == rc2) == bool(covers), (s0, ln, st[w])
    clean.close()
    dev.close()


def test_a_contradicted_index_entry_is_replayed_and_complete(ctx, x3):
    dev = base(ctx, x3)
    nw = SR.n_words(6, dev.op, SB)
    good = ctx.download(dev.d_seg, 8 * nw, np.uint64)
    per = (nw - 1) // 6
    bad = good.copy()
    bad[1 + 2 * per + 1] += np.uint64(1)               # frame 2, entry 2: one bit late
    ctx.upload(dev.d_seg, bad)
    frames = dev.frames()
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    assert ctx.get_option("last_range_levels_replays") > 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        assert st[w] == (0 if s0 <= N and ln <= N - s0 else BAD)
    ctx.upload(dev.d_seg, np.zeros(nw, dtype=np.uint64))     # "no index": one stretch a frame
    check(ctx, dev, frames, dev.so, starts, lens, 7, 0, rows_total(lens, 7))
    assert ctx.get_option("last_range_levels_replays") == 0
    dev.close()


def test_sample_offsets_of_another_stream(ctx, x3):
    dev = base(ctx, x3)
    so = np.array([0, 300, 600, 900, 1200, 1500, 1637], dtype=np.uint64)     # frames of 300; the last frame agrees
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    frames = dev.frames(so)
    assert [st for st, _ in frames] == [BAD] * 5 + [0]
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames, so=so, d_so=d_so, total=1637)
    assert all(st[w] == BAD for w, (s0, ln) in enumerate(zip(starts, lens)) if ln and s0 < 1500)
    assert any(st[w] == 0 for w, (s0, ln) in enumerate(zip(starts, lens)) if ln and s0 >= 1500)
    dev.close()


# ------------------------------------------------------------------------------------------------ shared frames

@pytest.mark.parametrize("n, overflow", [(2, False), (40, True)])
def test_ranges_that_all_cover_all_six_frames(ctx, x3, n, overflow):
    """40 ranges over 6 frames are 240 pairs against P = min(40 * 6, 4 * (6 + 40)) = 184: the pairs beyond go through the
    reader, and the records are the same"""
    dev = base(ctx, x3)
    starts = [w % 3 for w in range(n)]
    lens = [N - 2 - (w % 5) for w in range(n)]
    for bin_len in (0, 7, 400):
        check(ctx, dev, dev.frames(), dev.so, starts, lens, bin_len, 0, rows_total(lens, bin_len))
        assert (ctx.get_option("last_range_levels_overflow") > 0) == overflow
        if overflow:
            assert ctx.get_option("last_range_levels_overflow") == 240 - 184
            assert ctx.get_option("last_range_levels_replays") == 240 - 184
    dev.close()


def test_sliding_ranges_of_800_with_hop_200_do_not_overflow(ctx, x3):
    dev = base(ctx, x3)
    starts = list(range(0, N - 800 + 1, 200))
    lens = [800] * len(starts)
    for bin_len in (0, 100, 399):
        check(ctx, dev, dev.frames(), dev.so, starts, lens, bin_len, 0, rows_total(lens, bin_len))
        assert ctx.get_option("last_range_levels_overflow") == 0 and ctx.get_option("last_range_levels_replays") == 0
    dev.close()


def test_more_ranges_than_threads_of_the_scans(ctx, x3):
    dev = base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 60, 3000).tolist()
    starts = rng.integers(0, N - 60, 3000).tolist()
    check(ctx, dev, dev.frames(), dev.so, starts, lens, 7, 0, rows_total(lens, 7))
    check(ctx, dev, dev.frames(), dev.so, starts, lens, 0, 2, 6000)
    dev.close()


# ------------------------------------------------------------------------------------------------ against existing GPU paths

def _damaged_base(ctx, x3):
    clean = base(ctx, x3)
    s = clean.stream.copy()
    s[clean.offs[2] + 20 + 30] ^= 0x08
    dev = Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    clean.close()
    return dev


@pytest.mark.parametrize("hurt", [False, True])
def test_the_whole_stream_equals_x3_levels_dev(ctx, x3, hurt):
    dev = _damaged_base(ctx, x3) if hurt else base(ctx, x3)
    for bin_len in (400, 0):
        n_bins = R.rows_of(N, bin_len)
        lv, fst = dev.levels(bin_len, n_bins)
        assert fst.tolist() == [0, 0, CRC if hurt else 0, 0, 0, 0]
        out, off, st, total = run(ctx, dev.call, [0], [N], bin_len, 0, n_bins)
        assert total == n_bins and st.tolist() == [CRC if hurt else 0]
        assert np.array_equal(R.view(out), lv)
        assert int(lv["n"].sum()) == (N - 400 if hurt else N)
    dev.close()


def test_the_slots_of_x3_events_dev_at_bin_len_0_equal_its_event_levels(ctx, x3):
    dev = base(ctx, x3)
    bin_len, cap = 50, 48
    n_bins = R.rows_of(N, bin_len)
    lv, _ = dev.levels(bin_len, n_bins)
    peak = int(np.sort(np.maximum(lv["max"], -lv["min"]))[n_bins // 2])            # half of the bins are hot
    rule = x3.EventRule.make(peak_min=peak, join_bins=2, pad_bins=1, max_bins=4)
    d_lv, d_st, d_ln, d_el, d_cnt = (dev.alloc(REC * n_bins), dev.alloc(8 * cap), dev.alloc(4 * cap), dev.alloc(REC * cap),
                                     dev.alloc(8))
    ctx.upload(d_lv, lv)
    assert ctx.events_dev(d_lv, n_bins, bin_len, dev.d_so + 8 * dev.F, rule, d_st, d_ln, d_el, cap, d_cnt) == 0
    rc, count = ctx.events_result()
    assert rc == 0 and 0 < count < cap                                             # events, and fillers behind them
    want = ER.stream_events(lv, N, bin_len, ER.Rule(peak_min=peak, join_bins=2, pad_bins=1, max_bins=4))
    assert len(want[0]) == count
    d_out, d_off, d_status = dev.alloc(REC * cap), dev.alloc(8 * (cap + 1)), dev.alloc(4 * cap)
    assert dev.call(d_st, d_ln, cap, 0, 0, d_out, cap, d_off, d_status) == 0       # the arrays as they are
    assert ctx.range_levels_result() == (0, 0, cap, 0, cap)
    got = ctx.download(d_out, REC * cap, LR.LEVEL_DTYPE)
    assert np.array_equal(got, ctx.download(d_el, REC * cap, LR.LEVEL_DTYPE))
    assert np.array_equal(got[:count], want[1]) and np.array_equal(got[count:], LR.empty(cap - count))
    assert ctx.download(d_off, 8 * (cap + 1), np.uint64).tolist() == list(range(cap + 1))
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

ENTRY_SAMPLES = (1, 399, 400, N, 1000)


def _corpus(ctx, x3, bl=20, bpf=20, index="decode"):
    """five entries at odd byte offsets; the last has a payload-CRC failure in its frame 1"""
    op = O.Params.make(bl, bpf)
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf)
    ents, parts, offsets, pos = [], [], [], 0
    for e, n in enumerate(ENTRY_SAMPLES):
        rc, s, _ = O.encode(x3.synth(2, 900 + e, 0, n), op)
        assert rc == 0
        if e == 4:
            s = s.copy()
            s[RR.frame_offsets(s)[1] + 20 + 11] ^= 0x40
        pad = np.zeros(1 if pos % 2 == 0 else 2, dtype=np.uint8)
        parts += [pad, s]
        offsets.append(pos + pad.size)
        pos += pad.size + s.size
        ents.append(s)
    buf = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf, offsets, [s.size for s in ents], params=p, seg_blocks=SB, index=index)
    assert corpus.entries["n_samples"].tolist() == list(ENTRY_SAMPLES)
    return corpus, [Dev(ctx, x3, s, p, op, None) for s in ents]


def _corpus_table(seed):
    rng = np.random.default_rng(seed)
    tab = [(e, 0, n) for e, n in enumerate(ENTRY_SAMPLES)]                       # the whole of every entry
    tab += [(e, 1, n) for e, n in enumerate(ENTRY_SAMPLES)]                      # one past the entry's end
    tab += [(5, 0, 10), (2 ** 32 - 1, 0, 0), (0, 1, 0), (0, 2, 0), (4, 996, 4), (4, 2 ** 63, 1), (4, 0, 400), (4, 399, 2),
            (4, 800, 200), (3, 399, 402)]
    for _ in range(30):
        e = int(rng.integers(0, 5))
        ln = int(rng.integers(0, min(ENTRY_SAMPLES[e], 900) + 1))
        tab.append((e, int(rng.integers(0, ENTRY_SAMPLES[e] - ln + 1)), ln))
    rng.shuffle(tab)
    return tab


@pytest.mark.parametrize("bl, bpf, index", [(20, 20, "decode"), (40, 10, "walk")])
def test_corpus_ranges_equal_the_stream_form_on_each_entry(ctx, x3, bl, bpf, index):
    corpus, devs = _corpus(ctx, x3, bl, bpf, index)
    tab = _corpus_table(9)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    seen = set()
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 22)):
        cap = len(tab) * stride or rows_total(lens, bin_len)
        out, off, st, total = run(ctx, corpus.range_levels_into, starts, lens, bin_len, stride, cap, entries=ent)
        assert total == rows_total(lens, bin_len)
        for w, (e, s0, ln) in enumerate(tab):
            rows = stride or R.rows_of(ln, bin_len)
            mine = out[int(off[w]):int(off[w]) + rows]
            if e >= 5:
                assert st[w] == BAD and np.array_equal(R.view(mine), LR.empty(rows)), (e, s0, ln)   # not in the corpus
                continue
            d = devs[e]
            want = R.range_levels(d.frames(), d.so, [s0], [ln], bin_len, stride, rows)
            one = run(ctx, lambda *a: d.call(*a, seg=False), [s0], [ln], bin_len, stride, rows)   # the stream form, on that entry alone
            assert st[w] == one[2][0], (e, s0, ln, st[w])
            same(mine, one[0], (e, s0, ln))
            assert one[2][0] == want[2][0]                     # ... and both are the reference's
            same(one[0], want[0], (e, s0, ln))
            seen.add(int(st[w]))
    assert seen == {0, BAD, CRC}
    for d in devs:
        d.close()
    corpus.close()


def test_an_entry_table_overwritten_after_the_build(ctx, x3):
    """nothing is trusted: whatever the device's entry table says, only the caller's arrays are written (run() brackets every
    output with canaries), ranges without room keep their fill, and what the table still describes is right"""
    corpus, devs = _corpus(ctx, x3)
    d_ent = corpus.d_entries
    assert ctx.download(d_ent, 32 * corpus.n_entries, x3.CORPUS_ENTRY_DTYPE).tobytes() == corpus.entries.tobytes()
    tab = _corpus_table(10)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    rng = np.random.default_rng(3)
    for wild in ([0] * 5, [2 ** 64 - 1] * 5, [10 ** 6] * 5, [1, 2 ** 63, 7, 2 ** 64 - 5, 3]):
        t = corpus.entries.copy()
        t["n_samples"] = np.array(wild, dtype=np.uint64)
        if wild[0] != 10 ** 6:
            t["first_frame"] = rng.integers(0, 2 ** 62, 5)
            t["n_frames"] = rng.integers(0, 2 ** 62, 5)
        ctx.upload(d_ent, t)
        for bin_len, stride in ((7, 0), (0, 3), (100, 0)):
            rows = [R.rows_of(v, bin_len) for v in lens]
            full = len(tab) * stride or sum(rows)
            for cap in (full, max(full // 2, len(tab) * stride)):
                out, off, st, total = run(ctx, corpus.range_levels_into, starts, lens, bin_len, stride, cap, entries=ent)
                assert total == sum(rows)
                if not stride:
                    roff = np.concatenate([[0], np.cumsum(rows)])
                    assert off.tolist() == roff.tolist()
                    k = next((w for w in range(len(tab)) if roff[w] + rows[w] > cap), len(tab))
                    assert (out[int(roff[k]):] == 0x5A).all() and all(st[w] == BAD for w in range(k, len(tab)))
                assert all(st[w] == BAD for w, (e, _, _) in enumerate(tab) if e >= 5)
    ctx.upload(d_ent, corpus.entries)                          # the table as the build left it: the reference again
    out, off, st, _ = run(ctx, corpus.range_levels_into, starts, lens, 7, 0, rows_total(lens, 7), entries=ent)
    for w, (e, s0, ln) in enumerate(tab):
        if e < 5:
            want = R.range_levels(devs[e].frames(), devs[e].so, [s0], [ln], 7, 0, R.rows_of(ln, 7))
            assert st[w] == want[2][0]
            same(out[int(off[w]):int(off[w + 1])], want[0], (e, s0, ln))
    for d in devs:
        d.close()
    corpus.close()


# ------------------------------------------------------------------------------------------------ pending state

def test_levels_events_range_levels_and_ranges_back_to_back(ctx, x3):
    dev = _damaged_base(ctx, x3)
    bin_len, cap = 50, 16
    n_bins = R.rows_of(N, bin_len)
    rule = x3.EventRule.make(peak_min=1, join_bins=0, pad_bins=0, max_bins=4)          # every counted bin is hot
    d_lv, d_st, d_ln, d_el, d_cnt = (dev.alloc(REC * n_bins), dev.alloc(8 * cap), dev.alloc(4 * cap), dev.alloc(REC * cap),
                                     dev.alloc(8))
    d_rl, d_roff, d_rst = dev.alloc(REC * cap), dev.alloc(8 * (cap + 1)), dev.alloc(4 * cap)
    d_out, d_ooff, d_ost = dev.alloc(2 * cap * 200), dev.alloc(8 * (cap + 1)), dev.alloc(4 * cap)
    assert ctx.levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, None, dev.d_seg, SB) == 0
    assert ctx.events_dev(d_lv, n_bins, bin_len, dev.d_so + 8 * dev.F, rule, d_st, d_ln, d_el, cap, d_cnt) == 0
    assert dev.call(d_st, d_ln, cap, 0, 0, d_rl, cap, d_roff, d_rst) == 0
    assert ctx.decode_ranges_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_st, d_ln, cap, 200, d_out, cap * 200, 0,
                                 d_ooff, d_ost, dev.d_seg, SB) == 0
    # the four result calls, in another order than the calls: each answers its own
    assert ctx.decode_ranges_result() == (0, 0, cap, 0, 800 + 937)   # (what frames 0, 1 and 3 .. 5 hold)
    assert ctx.range_levels_result() == (0, 0, cap, 0, cap)
    assert ctx.events_result() == (0, 9)                       # 16 and 19 counted bins in pieces of 4: 4 + 5
    assert ctx.levels_result() == (0, 1, 2, CRC)
    assert np.array_equal(ctx.download(d_rl, REC * cap, LR.LEVEL_DTYPE), ctx.download(d_el, REC * cap, LR.LEVEL_DTYPE))
    for r in (ctx.decode_ranges_result, ctx.range_levels_result, ctx.events_result, ctx.levels_result):
        assert r()[0] == BAD                                   # nothing is pending any more
    # a second call replaces the first's summary; the other slots are not touched
    d_s2, d_l2 = dev.alloc(16), dev.alloc(8)
    ctx.upload(d_s2, np.array([0, 2000], dtype=np.uint64))
    ctx.upload(d_l2, np.array([N, 138], dtype=np.uint32))
    assert dev.call(d_s2, d_l2, 2, 400, 0, d_rl, cap, d_roff, d_rst) == 0
    assert dev.call(d_s2, d_l2, 1, 400, 0, d_rl, cap, d_roff, d_rst) == 0
    assert ctx.range_levels_result() == (0, 1, 0, CRC, 6)
    assert ctx.range_levels_result()[0] == BAD
    assert ctx.levels_result()[0] == BAD and ctx.decode_ranges_result()[0] == BAD and ctx.events_result()[0] == BAD
    dev.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_argument_refusals_enqueue_nothing(ctx, x3):
    dev = base(ctx, x3)
    n = 4
    sizes = {"lv": REC * 64, "off": 8 * (n + 1), "st": 4 * n}
    d = {k: dev.alloc(v) for k, v in sizes.items()}
    d_starts, d_lens = dev.alloc(8 * n), dev.alloc(4 * n)
    ctx.upload(d_starts, np.zeros(n, dtype=np.uint64))
    ctx.upload(d_lens, np.full(n, 16, dtype=np.uint32))
    for k, v in sizes.items():
        ctx.upload(d[k], np.full(v, 0x5A, dtype=np.uint8))
    Rg = ctx.range_levels_dev
    a = (dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p)
    ok = dict(d_starts=d_starts, d_lens=d_lens, n_ranges=n, bin_len=4, row_stride=0, d_levels=d["lv"], rows_cap=64,
              d_row_offsets=d["off"], d_status=d["st"], d_seg_index=dev.d_seg, seg_blocks=SB)
    refusals = [dict(n_ranges=0), dict(n_ranges=2 ** 31), dict(rows_cap=0), dict(rows_cap=2 ** 31), dict(d_starts=None),
                dict(d_lens=None), dict(d_levels=None), dict(d_status=None), dict(d_row_offsets=None),
                dict(d_starts=d_starts + 4), dict(d_lens=d_lens + 2), dict(d_levels=d["lv"] + 4),
                dict(d_row_offsets=d["off"] + 4), dict(d_status=d["st"] + 2), dict(seg_blocks=3), dict(seg_blocks=0),
                dict(row_stride=17, rows_cap=64),                      # 4 rows of 17 do not fit 64
                dict(row_stride=2 ** 63, rows_cap=64)]                 # ... and the product is never formed
    for r in refusals:
        assert Rg(*a, **dict(ok, **r)) == BAD, r
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert Rg(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, bad_p, **ok) != 0           # parameters the window calls refuse
    assert Rg(dev.d_x3, dev.len, dev.d_off + 4, dev.d_so, dev.F, dev.p, **ok) == BAD
    assert Rg(None, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, **ok) == BAD
    assert Rg(dev.d_x3, dev.len, dev.d_off, dev.d_so + 4, dev.F, dev.p, **ok) == BAD
    # the corpus form: its own pointer, and the shared refusals through its entry
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, bin_len=4, row_stride=0, d_levels=d["lv"], rows_cap=64,
               d_row_offsets=d["off"], d_status=d["st"])
    crefusals = [dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(n=2 ** 31), dict(rows_cap=0),
                 dict(rows_cap=2 ** 31), dict(d_starts=None), dict(d_lens=None), dict(d_levels=None), dict(d_status=None),
                 dict(d_row_offsets=None), dict(d_starts=d_starts + 4), dict(d_lens=d_lens + 2), dict(d_levels=d["lv"] + 4),
                 dict(d_row_offsets=d["off"] + 4), dict(d_status=d["st"] + 2), dict(row_stride=17, rows_cap=64)]
    for r in crefusals:
        assert corpus.range_levels_into(**dict(cok, **r)) == BAD, r
    ctx.graph_begin()
    try:
        assert Rg(*a, **ok) == BAD                                       # a context that records a graph
        assert corpus.range_levels_into(**cok) == BAD
    finally:
        try:
            ctx.graph_destroy(ctx.graph_end())
        except x3.X3Error:
            pass                                                         # (a recording of nothing)
    assert ctx.range_levels_result()[0] == BAD                           # nothing is pending
    ctx.sync()
    for k, v in sizes.items():
        assert (ctx.download(d[k], v) == 0x5A).all(), k
    assert Rg(*a, **dict(ok, row_stride=16, d_row_offsets=None)) == 0    # padded: the offsets may be NULL
    assert ctx.range_levels_result() == (0, 0, n, 0, 16)
    assert (ctx.download(d["off"], sizes["off"]) == 0x5A).all()
    want = R.range_levels(dev.frames(), dev.so, [0] * n, [16] * n, 4, 16, 64)[0]
    same(ctx.download(d["lv"], REC * 64).reshape(64, REC), want)
    assert corpus.range_levels_into(**cok) == 0                          # (what the corpus refusals were cut from is a good call)
    assert ctx.range_levels_result() == (0, 0, n, 0, 16)
    import torch
    if torch.cuda.device_count() > 1:                                    # a context on another device than the corpus
        other = x3.Context(1)
        try:
            q = [other.alloc(64) for _ in range(6)]
            assert other.corpus_range_levels_dev(corpus, q[0], q[1], q[2], 1, 0, 0, q[3], 1, q[4], q[5]) == BAD
            assert "another device" in other.last_error() and other.range_levels_result()[0] == BAD
            for ptr in q:
                other.free(ptr)
        finally:
            other.close()
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ the Python surface

def test_torch_surface_of_window_source_and_corpus(ctx, x3):
    import torch
    wav = base_wav(x3)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    p = x3.Params.make(block_len=20, blocks_per_frame=20)
    offs = RR.frame_offsets(s)
    frames = RR.frames_of(s, offs, op)
    so = R.sample_offsets([400] * 5 + [137])
    src = x3.WindowSource(ctx, s, p, seg_blocks=SB, index="walk")
    starts = torch.tensor([0, 399, 2000, 2137, 5], dtype=torch.int64, device="cuda")
    lens = torch.tensor([400, 3, 137, 0, 3000], dtype=torch.int32, device="cuda")
    lv, off, st = src.range_levels(starts, lens, 100)
    assert lv.is_cuda and off.is_cuda and st.is_cuda and lv.dtype == torch.uint8 and lv.shape == (4 + 1 + 2 + 1 + 30, 32)
    assert off.tolist() == [0, 4, 5, 7, 8, 38] and st.tolist() == [0, 0, 0, 0, BAD]
    want = R.range_levels(frames, so, starts.tolist(), lens.tolist(), 100, 0, 38)
    same(lv.cpu().numpy(), want[0])
    assert np.array_equal(x3.event_levels_view(lv), R.view(want[0]))
    lv, off, st = src.range_levels([0, 399], [400, 3], 0)
    assert lv.shape == (2, 32) and off.tolist() == [0, 1, 2] and st.tolist() == [0, 0]
    same(lv.cpu().numpy(), R.range_levels(frames, so, [0, 399], [400, 3], 0, 0, 2)[0])
    lv, off, st = src.range_levels([0, 399], [400, 3], 2 ** 63)                 # one bin as well: no sum on the host
    assert lv.shape == (2, 32) and off.tolist() == [0, 1, 2]
    same(lv.cpu().numpy(), R.range_levels(frames, so, [0, 399], [400, 3], 0, 0, 2)[0])
    lv, off, st = src.range_levels([0, 399], [400, 3], 100, padded_to=6)
    assert lv.shape == (12, 32) and off.tolist() == [0, 6, 12]
    same(lv.cpu().numpy(), R.range_levels(frames, so, [0, 399], [400, 3], 100, 6, 12)[0])
    lv, off, st = src.range_levels(starts, lens, 100, capacity=6)
    assert st.tolist() == [0, 0, BAD, BAD, BAD] and off[-1].item() == 38 and lv.shape == (6, 32)
    # events() output fed in unchanged: the records at bin_len 0 are the events' merged records, fillers included
    rule = x3.EventRule.make(peak_min=1, join_bins=0, pad_bins=0, max_bins=8)
    e_starts, e_lens, count, e_lv = src.events(50, rule, 12)
    assert 0 < int(count) < 12
    lv, off, st = src.range_levels(e_starts, e_lens, 0)
    assert off.tolist() == list(range(13)) and not st.any() and torch.equal(lv, e_lv)
    src.close()
    corpus = x3.Corpus(ctx, s, [0], [s.size], params=p, seg_blocks=SB, index="walk")
    lv, off, st = corpus.range_levels([0, 0, 1], [2000, 0, 0], [137, 2137, 1], 400)
    assert st.tolist() == [0, 0, BAD] and off.tolist() == [0, 1, 7, 8]
    want = R.range_levels(frames, so, [2000, 0, N + 1], [137, 2137, 1], 400, 0, 8)
    same(lv.cpu().numpy(), want[0])
    ent, e_starts, e_lens, count, e_lv = corpus.events(50, rule, 12)
    lv, off, st = corpus.range_levels(ent, e_starts, e_lens, 0, padded_to=1)
    assert not st.any() and torch.equal(lv, e_lv)
    corpus.close()
