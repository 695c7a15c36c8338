"""Levels (include/x3hip.h, "LEVELS"): x3_levels_dev, x3_levels_result, x3_corpus_levels_rows, x3_corpus_levels_dev and
their mirrors.  Every field of every record is held with == against levels_ref.py fed with the CPU oracle's samples; frame
statuses against the oracle's decode_frame and against x3_decode_windows_dev's status of a window that is exactly the frame.
Streams are six full frames and a short last one of 3 457 samples unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import levels_ref as R
import oracle_lib as O
import test_gpu_windows as TW
import x3_cases as XC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 24
CRC = 14
BPF = 20
TAIL = 3_457
BIN_LENS = [0, 1, 7, 20, 640, 641, 10_000, 10_007, 1 << 20]
KINDS = ["silence", "rice0", "rice1", "rice3", "bfp", "literal", "patchwork"]
CANARY = 0xC3


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _content(kind, n, seed=5):
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    if kind == "silence":
        return np.zeros(n, dtype=np.int16)
    if kind == "literal":        # white noise with both ends of the scale in it
        w = rng.integers(-32768, 32768, size=n).astype(np.int16)
        w[::97], w[50::101] = -32768, 32767
        return w
    if kind == "patchwork":      # every block type side by side
        return XC.patchwork(seed, n)
    amp = {"rice0": 1, "rice1": 5, "rice3": 15, "bfp": 700}[kind]
    return np.clip(np.cumsum(rng.integers(-amp, amp + 1, size=n)), -32768, 32767).astype(np.int16)


def _block_types(stream, offs, op):
    """the block types (0 BFP / literal, 1..3 Rice) the stream's frames hold, by the oracle's reader -- only used to make
    sure the content kinds reach what they are named for"""
    seen = set()
    for a in offs:
        samples, plen = int(stream[a + 4]) << 8 | int(stream[a + 5]), int(stream[a + 6]) << 8 | int(stream[a + 7])
        seen.add(int(stream[a + 22]) >> 6)   # the first block's type: the two bits behind the first sample
    return seen


def _oracle_frames(stream, offs, op):
    """-> (per frame its samples or None, per frame the oracle's decode_frame status)"""
    frames, st = [], []
    for a in offs:
        samples, plen = int(stream[a + 4]) << 8 | int(stream[a + 5]), int(stream[a + 6]) << 8 | int(stream[a + 7])
        rc, w = O.decode_frame(stream[a + 20:a + 20 + plen], samples, op)
        frames.append(w if rc == 0 else np.zeros(0, dtype=np.int16))
        st.append(rc)
    return frames, st


def _levels(dev, bin_len, n_bins, d_seg="own", sb=None, d_off=None, d_so=None, want_rc=0):
    """x3_levels_dev into a poisoned buffer with a canary behind it -> (records, frame statuses, x3_levels_result, replays)"""
    ctx = dev.ctx
    nb = 32 * n_bins
    d_lv, d_st = ctx.alloc(nb + 64), ctx.alloc(4 * dev.F + 64)
    try:
        ctx.upload(d_lv, np.full(nb + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * dev.F + 64, CANARY, dtype=np.uint8))
        idx = dev.d_seg if isinstance(d_seg, str) else d_seg
        rc = ctx.levels_dev(dev.d_x3, dev.len, d_off or dev.d_off, d_so or dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st,
                            idx, (sb if sb is not None else dev.sb) if idx else 0)
        assert rc == want_rc, (rc, ctx.last_error())
        if rc:
            return None
        res = ctx.levels_result()
        replays = ctx.get_option("last_levels_replays")
        raw, raw_st = ctx.download(d_lv, nb + 64, np.uint8), ctx.download(d_st, 4 * dev.F + 64, np.uint8)
        assert (raw[nb:] == CANARY).all() and (raw_st[4 * dev.F:] == CANARY).all(), "written behind the buffers"
        st = raw_st[:4 * dev.F].view(np.int32).copy()
        bad = np.nonzero(st)[0]
        assert res == (0, bad.size, int(bad[0]) if bad.size else dev.F, int(st[bad[0]]) if bad.size else 0), (res, st)
        return raw[:nb].view(R.LEVEL_DTYPE).copy(), st, res, replays
    finally:
        ctx.free(d_lv)
        ctx.free(d_st)


def _same(got, want, what):
    for k in R.LEVEL_DTYPE.names:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def _encoded(ctx, x3, wav, p=None, sb=32):
    """the stream by the GPU encoder with its segment index, which must be the oracle's stream byte for byte"""
    dev = TW.Dev(ctx, x3, wav=wav, p=p, sb=sb)
    rc, stream, _ = O.encode(wav, XC.oparams(dev.p))
    assert rc == 0 and dev.len == stream.size
    assert np.array_equal(ctx.download(dev.d_x3, dev.len), stream)
    return dev, stream


def _frame_windows(dev, d_off=None, d_so=None, so=None):
    """per frame the status x3_decode_windows_dev gives the window that is exactly that frame (one call per frame length)"""
    so = dev.so if so is None else so
    st = np.zeros(dev.F, dtype=np.int32)
    lens = (so[1:].astype(np.int64) - so[:-1].astype(np.int64))
    for L in sorted(set(int(v) for v in lens)):
        fs = [f for f in range(dev.F) if int(lens[f]) == L]
        assert L > 0
        _, s = dev.windows([int(so[f]) for f in fs], L, 0, seg=False, d_off=d_off, d_so=d_so)
        st[fs] = s
    return st


# ---- 1. exactness over bin geometry
@pytest.mark.parametrize("kind", KINDS)
def test_exact_over_bin_geometry(ctx, x3, kind):
    """default parameters, the encoder's index, stretches of 640 samples; n_bins exact, one short, three too many"""
    n = 60_000 + TAIL
    wav = _content(kind, n)
    dev, stream = _encoded(ctx, x3, wav)
    try:
        assert dev.F == 7 and dev.sb == 32 and dev.total == n
        first = {"silence": 1, "rice0": 1, "rice1": 2, "rice3": 3, "bfp": 0, "literal": 0}.get(kind)
        types = _block_types(stream, XC.frame_offsets(stream), None)
        assert first is None or first in types, (kind, types)
        frames = [wav[int(a):int(b)] for a, b in zip(dev.so[:-1], dev.so[1:])]
        for bin_len in BIN_LENS:
            exact = R.n_bins_for(n, bin_len)
            for n_bins in sorted({exact, max(1, exact - 1), exact + 3}):
                got, st, res, replays = _levels(dev, bin_len, n_bins)
                assert not st.any() and replays == 0, (bin_len, n_bins, st, replays)
                _same(got, R.levels(frames, st, dev.so[:-1], bin_len, n_bins), (kind, bin_len, n_bins))
            if kind == "literal":
                one, _, _, _ = _levels(dev, bin_len, exact)
                assert int(one["min"].min()) == -32768 and int(one["max"].max()) == 32767
    finally:
        dev.close()


# ---- 2. other parameter sets, walk-built index
PARAM_SETS = [(10, 1000, (0, 1, 3)), (40, 250, (0, 1, 3)), (13, 300, (0, 1, 3)), (60, 50, (0, 1, 3)), (20, 500, (1, 1, 3))]


@pytest.mark.parametrize("bl,bpf,codes", PARAM_SETS)
def test_parameter_sets_by_a_walk_built_index(ctx, x3, bl, bpf, codes):
    """x3_seg_index_build_dev's index, no index, and an index whose header says "none": the same records.  Codes (1, 1, 3)
    at the default thresholds: the encoder writes blocks of type 1 with code 1, every decoder reads them with code 0 as
    the reference does, so frames of this content fail to decode -- they add nothing, with the window path's status"""
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf, codes), O.Params.make(bl, bpf, codes)
    n = 6 * spf + min(TAIL, spf - 1)
    wav = XC.patchwork(bl + bpf, n)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    sb = 4 if spf // bl <= 64 else 32
    ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(p), sb)
    assert ne > 0
    d_idx, d_none = dev.alloc(8 * ne), dev.alloc(8 * ne)
    try:
        assert ctx.seg_index_build_dev(dev.d_x3, dev.len, dev.d_off, dev.F, p, d_idx, sb) == 0
        idx = ctx.download(d_idx, 8 * ne, np.uint64)
        none = idx.copy()
        none[0] = 0
        ctx.upload(d_none, none)
        frames, ost = _oracle_frames(stream, XC.frame_offsets(stream), op)
        wst = _frame_windows(dev)
        assert np.array_equal(wst, np.array(ost, dtype=np.int32))
        if tuple(codes) == (1, 1, 3):
            assert any(ost), ost
        else:
            assert not any(ost)
        for bin_len in (0, 7, 641, 10_007):
            n_bins = R.n_bins_for(n, bin_len)
            want = R.levels(frames, ost, dev.so[:-1], bin_len, n_bins)
            for what, seg in (("walk", d_idx), ("no index", None), ("none", d_none)):
                got, st, res, replays = _levels(dev, bin_len, n_bins, d_seg=seg, sb=sb)
                assert np.array_equal(st, wst), (what, st, wst)
                _same(got, want, (what, bin_len))
                if not any(ost):
                    assert replays == 0, (what, bin_len, replays)
    finally:
        dev.close()


# ---- 3. rollback
def _index_words(ctx, x3, dev):
    ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), dev.sb)
    return ctx.download(dev.d_seg, 8 * ne, np.uint64), ne


@pytest.mark.parametrize("how", ["bit offset", "sample"])
@pytest.mark.parametrize("bin_len", [641, 10_007])
def test_a_contradicted_late_entry_changes_nothing(ctx, x3, bin_len, how):
    """a late entry of frame 2 is wrong: the stretches in front of it have added to the frame's rows already; the frame is
    decoded again by the reader, records and statuses are those of the intact index"""
    n = 60_000 + TAIL
    wav = _content("patchwork", n, seed=11)
    dev, stream = _encoded(ctx, x3, wav)
    try:
        idx, ne = _index_words(ctx, x3, dev)
        pitch = (ne - 1) // dev.F
        assert pitch == 15
        at = 1 + 2 * pitch + 11                   # frame 2, entry 12 of 15
        assert (int(idx[at]) >> 48) & 1
        idx[at] = np.uint64(int(idx[at]) + 1) if how == "bit offset" else np.uint64(int(idx[at]) ^ (1 << 32))
        d_bad = dev.alloc(8 * ne)
        ctx.upload(d_bad, idx)
        n_bins = R.n_bins_for(n, bin_len)
        good, st0, _, rep0 = _levels(dev, bin_len, n_bins)
        got, st, _, replays = _levels(dev, bin_len, n_bins, d_seg=d_bad)
        assert rep0 == 0 and replays >= 1
        assert not st.any() and not st0.any()
        _same(got, good, how)
        frames = [wav[int(a):int(b)] for a, b in zip(dev.so[:-1], dev.so[1:])]
        _same(got, R.levels(frames, st, dev.so[:-1], bin_len, n_bins), how)
    finally:
        dev.close()


@pytest.mark.parametrize("bin_len", [641, 10_007, 0])
def test_a_late_decode_error_takes_the_whole_frame_back(ctx, x3, bin_len):
    """a late block of frame 3 becomes a BFP block with E = 1 (CRCs made good again): the frame's status is the decode
    error and it adds nothing -- not the stretches that decoded in front of the block, not to the bins it shares with
    frames 2 and 4, whose samples stay"""
    n = 60_000 + TAIL
    wav = _content("patchwork", n, seed=12)
    dev, stream = _encoded(ctx, x3, wav)
    try:
        idx, ne = _index_words(ctx, x3, dev)
        pitch = (ne - 1) // dev.F
        entry = int(idx[1 + 3 * pitch + 12])       # frame 3, entry 13: the block 416 of 500 starts at this bit
        assert (entry >> 48) & 1
        offs = XC.frame_offsets(stream)
        bit = (offs[3] + 20) * 8 + (entry & 0xFFFFFFFF)
        s = stream.copy()
        for k in range(bit, bit + 6):              # block type 0, E - 1 = 0
            s[k >> 3] &= ~(0x80 >> (k & 7)) & 0xFF
        XC.refresh_crcs(s, offs[3])
        ctx.upload(dev.d_x3, s)
        op = XC.oparams(dev.p)
        frames, ost = _oracle_frames(s, offs, op)
        assert ost == [0, 0, 0, BPF, 0, 0, 0]
        n_bins = R.n_bins_for(n, bin_len)
        got, st, res, replays = _levels(dev, bin_len, n_bins)
        assert st.tolist() == ost and res == (0, 1, 3, BPF) and replays == 1
        want = R.levels(frames, ost, dev.so[:-1], bin_len, n_bins)
        _same(got, want, bin_len)
        if bin_len == 10_007:                      # bins 2 and 3 hold frame 2's and frame 4's samples alone
            assert int(got["n"][2]) == 30_000 - 2 * 10_007 and int(got["n"][3]) == 4 * 10_007 - 40_000
        assert np.array_equal(_frame_windows(dev), st)
    finally:
        dev.close()


# ---- 4. damage
def test_damaged_frames_add_nothing(ctx, x3):
    """a flipped payload byte, a broken header key, a header sample count that disagrees with the offsets, a frame offset
    past x3_len: the statuses are the window path's, frame for frame, the records levels_ref's with those statuses"""
    n = 60_000 + TAIL
    wav = _content("patchwork", n, seed=13)
    dev, stream = _encoded(ctx, x3, wav)
    try:
        offs = XC.frame_offsets(stream)
        s = stream.copy()
        s[offs[1] + 20 + 777] ^= 0x10                                  # frame 1: payload CRC
        s[offs[2]] ^= 0xFF                                             # frame 2: the key
        s[offs[4] + 4], s[offs[4] + 5] = 9_999 >> 8, 9_999 & 0xFF      # frame 4: 9 999 samples by a header with a good CRC
        hc = O.crc16(s[offs[4]:offs[4] + 16])
        s[offs[4] + 16], s[offs[4] + 17] = hc >> 8, hc & 0xFF
        ctx.upload(dev.d_x3, s)
        table = np.array(offs + [stream.size], dtype=np.uint64)
        table[5] = stream.size + 100                                   # frame 5: an offset past x3_len
        d_off = dev.alloc(8 * table.size)
        ctx.upload(d_off, table)
        wst = _frame_windows(dev, d_off=d_off)
        assert wst[1] == CRC and wst[2] != 0 and wst[4] == BAD and wst[5] == BAD and not wst[[0, 3, 6]].any(), wst
        frames = [wav[int(a):int(b)] for a, b in zip(dev.so[:-1], dev.so[1:])]
        for bin_len in (0, 641, 10_007):
            n_bins = R.n_bins_for(n, bin_len)
            for seg in ("own", None):
                got, st, res, replays = _levels(dev, bin_len, n_bins, d_seg=seg, d_off=d_off)
                assert np.array_equal(st, wst), (st, wst)
                assert res == (0, 4, 1, CRC) and replays == 0
                _same(got, R.levels(frames, wst, dev.so[:-1], bin_len, n_bins), bin_len)
    finally:
        dev.close()


# ---- 5. corpus
@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("bin_len", [0, 1_000])
def test_corpus_rows_are_each_entrys_own_levels(ctx, x3, bin_len, walk):
    """entries of 1, 2 and 3 frames (the middle frame of the last damaged), one of 0 bytes, one repeated, one of junk"""
    p = x3.Params.default()
    clips = [_content("patchwork", k * 10_000 - 1_234 * (k - 1), seed=20 + k) for k in (1, 2, 3)]
    entries = []
    for w in clips:
        rc, s, _ = O.encode(w, O.Params.make(20, 500, (0, 1, 3)))
        assert rc == 0
        entries.append(s)
    damaged = entries[2].copy()
    offs3 = XC.frame_offsets(damaged)
    damaged[offs3[1] + 20 + 99] ^= 0x01
    junk = np.random.default_rng(4).integers(0, 256, 37, dtype=np.uint8)
    ents = [entries[0], entries[1], damaged, np.zeros(0, dtype=np.uint8), entries[1], junk]
    buf, offs, lens = _place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=32, index="walk" if walk else "decode")
    try:
        assert corpus.seg_blocks == 32
        assert corpus.entries["n_frames"].tolist() == [1, 2, 3, 0, 2, 0]
        rf = corpus.levels_rows(bin_len)
        assert np.array_equal(rf, R.corpus_row_first(corpus.entries["n_samples"], bin_len))
        rows, rf2, st = corpus.levels(bin_len)
        assert np.array_equal(rf, rf2) and rows.size == int(rf[-1]) and st.size == corpus.n_frames == 8
        assert st.tolist() == [0, 0, 0, 0, CRC, 0, 0, 0]
        assert ctx.levels_result()[0] == BAD                       # (the result has been read)
        assert ctx.get_option("last_levels_replays") == 0
        op = XC.oparams(p)
        ref_entries = []
        for e, s in enumerate(ents):
            a, b = int(rf[e]), int(rf[e + 1])
            nf = int(corpus.entries["n_frames"][e])
            if nf == 0:
                assert b - a == 1 and np.array_equal(rows[a:b], R.empty(1)), e
                ref_entries.append(([], [], [], 0))
                continue
            ws = x3.WindowSource(ctx, s, p, seg_blocks=32, index="walk")      # the entry alone, its own frame table
            try:
                assert ws.n_frames == nf and ws.total == int(corpus.entries["n_samples"][e])
                alone, st_alone = ws.levels(bin_len, b - a)
            finally:
                ws.close()
            _same(rows[a:b], alone, ("alone", e))
            first = int(corpus.entries["first_frame"][e])
            assert np.array_equal(st_alone, st[first:first + nf])
            fo = XC.frame_offsets(s)
            frames, ost = _oracle_frames(s, fo, op)
            fst = [CRC if (e == 2 and f == 1) else ost[f] for f in range(nf)]
            assert fst == st_alone.tolist()
            lens_f = [int(s[o + 4]) << 8 | int(s[o + 5]) for o in fo]
            ref_entries.append((frames, fst, np.concatenate([[0], np.cumsum(lens_f)])[:-1], sum(lens_f)))
        want, rf3 = R.corpus_levels(ref_entries, bin_len)
        assert np.array_equal(rf3, rf)
        _same(rows, want, "levels_ref")
        # a wrong row count is refused, with nothing enqueued
        d_lv = ctx.alloc(32 * (int(rf[-1]) + 1))
        try:
            for n_rows in (int(rf[-1]) - 1, int(rf[-1]) + 1):
                if n_rows:
                    assert ctx.corpus_levels_dev(corpus, bin_len, d_lv, n_rows) == BAD
            assert ctx.levels_result()[0] == BAD
        finally:
            ctx.free(d_lv)
    finally:
        corpus.close()


# ---- 5b. more items than the one-workgroup scans have threads
def test_more_frames_than_threads_of_the_scans(ctx, x3):
    """2 049 frames of 40 samples (the last of 17): x3_window_sample_offsets_kernel and x3_levels_scan_kernel, one workgroup
    of 1 024 each, walk a run of three frames per thread"""
    bl, bpf, spf = 20, 2, 40
    p, op = x3.Params.make(bl, bpf, (0, 1, 3)), O.Params.make(bl, bpf, (0, 1, 3))
    n = 2048 * spf + 17
    wav = _content("rice3", n, seed=9)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    try:
        fo = XC.frame_offsets(stream)
        frames, ost = _oracle_frames(stream, fo, op)
        assert dev.F == len(frames) == 2049
        assert np.array_equal(dev.so, np.concatenate([[0], np.cumsum([len(w) for w in frames])]).astype(np.uint64))
        for bin_len in (0, 7, spf, 1_000):
            n_bins = R.n_bins_for(n, bin_len)
            got, st, res, replays = _levels(dev, bin_len, n_bins, d_seg=None)
            assert np.array_equal(st, np.array(ost, dtype=np.int32))
            _same(got, R.levels(frames, ost, dev.so[:-1], bin_len, n_bins), bin_len)
    finally:
        dev.close()


def test_more_entries_than_threads_of_the_row_scan(ctx, x3):
    """a corpus of 1 025 one-frame entries of 30 to 90 samples: x3_corpus_levels_rows_kernel's workgroup of 1 024 walks a run
    of two entries per thread; the rows of every entry lie where the host's prefix and levels_ref put them"""
    p = x3.Params.default()
    op = XC.oparams(p)
    rng = np.random.default_rng(1025)
    ents, ref_entries = [], []
    for e in range(1025):
        w = _content("rice3", int(rng.integers(30, 91)), seed=100 + e)
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        frames, ost = _oracle_frames(s, XC.frame_offsets(s), op)
        assert len(frames) == 1
        ents.append(s)
        ref_entries.append((frames, ost, [0], w.size))
    buf, offs, lens = _place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=32, index="walk")
    try:
        for bin_len in (16, 0):
            want, rf = R.corpus_levels(ref_entries, bin_len)
            assert np.array_equal(corpus.levels_rows(bin_len), rf)
            rows, rf2, st = corpus.levels(bin_len)
            assert np.array_equal(rf2, rf) and st.tolist() == [o for _, ost, _, _ in ref_entries for o in ost]
            _same(rows, want, bin_len)
    finally:
        corpus.close()


def _place_even(entries):
    blob, offs = bytearray(), []
    for e in entries:
        blob += b"\x5a" * (6 + (len(blob) & 1))
        offs.append(len(blob))
        blob += bytes(e)
    return np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8)[:-16], offs, [len(e) for e in entries]


# ---- 6. arguments and state
def test_arguments_and_pending_states(ctx, x3):
    L = x3.lib()
    n = 20_000 + TAIL
    wav = _content("patchwork", n, seed=14)
    dev, stream = _encoded(ctx, x3, wav)
    d_lv, d_st, d_back = dev.alloc(32 * 8), dev.alloc(4 * dev.F), dev.alloc(2 * n)
    try:
        def call(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=32, bl=4_000, lv=d_lv,
                 nb=8, st=d_st):
            return L.x3_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, bl, lv, nb, st)
        poison = np.full(32 * 8, CANARY, dtype=np.uint8)
        ctx.upload(d_lv, poison)
        for bad in (dict(nb=0), dict(nb=1 << 31), dict(nf=0), dict(nf=1 << 31), dict(c=None), dict(x=None), dict(fo=None),
                    dict(so=None), dict(lv=None), dict(x=dev.d_x3 + 2), dict(fo=dev.d_off + 4), dict(so=dev.d_so + 4),
                    dict(lv=d_lv + 4), dict(st=d_st + 2), dict(idx=dev.d_seg + 4), dict(sb=0), dict(sb=30), dict(sb=3204),
                    dict(params=x3.Params.make(codes=(0, 1, 4))), dict(params=x3.Params.make(0, 10))):
            assert call(**bad) == BAD, bad
        assert ctx.levels_result()[0] == BAD                                   # nothing is pending
        ctx.sync()
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)    # ... and nothing was enqueued
        # a context that records a graph
        ctx.graph_begin()
        try:
            assert call() == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass                                                           # (a recording of nothing)
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)
        # no status array: fine
        assert call(st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        frames = [wav[int(a):int(b)] for a, b in zip(dev.so[:-1], dev.so[1:])]
        want = R.levels(frames, [0] * dev.F, dev.so[:-1], 4_000, 8)
        _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), want, "no status array")
        # a pending x3_decode_dev reports through x3_decode_result afterwards
        assert ctx.decode_dev(dev.d_x3, dev.len, dev.d_off, dev.F, dev.p, d_back, n, n_per_clip=n) == 0
        assert call() == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        rc, first_bad, _, before = ctx.decode_result()
        assert (rc, first_bad, before) == (0, dev.F, n) and np.array_equal(ctx.download(d_back, 2 * n, np.int16), wav)
        # a levels call between x3_decode_windows_dev and its result leaves that result intact
        starts = np.array([0, 5, n - 100, n], dtype=np.uint64)                  # (the last one is off the end)
        d_s, d_out, d_ws = dev.alloc(32), dev.alloc(2 * 4 * 100), dev.alloc(16)
        ctx.upload(d_s, starts)
        assert ctx.decode_windows_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_s, 4, 100, d_out, 0, d_ws,
                                      dev.d_seg, 32) == 0
        assert call() == 0
        assert ctx.levels_result() == (0, 0, dev.F, 0)
        assert ctx.decode_windows_result() == (0, 1, 3, BAD)
        rows = ctx.download(d_out, 800, np.int16).reshape(4, 100)
        for i in range(3):
            assert np.array_equal(rows[i], wav[int(starts[i]):int(starts[i]) + 100])
        _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), want, "between windows")
        # the corpus call: a wrong device is covered by the C ABI's check; NULL handles
        assert L.x3_corpus_levels_dev(ctx._h, None, 0, d_lv, 1, None) == BAD
        assert L.x3_corpus_levels_rows(None, 0, None) == BAD
        # ... a recording context is refused, and a call with no bad frame reports the frame count and status 0
        corpus = x3.Corpus(ctx, (dev.d_x3, dev.len), [0], [dev.len], params=dev.p, seg_blocks=32, index="walk")
        try:
            n_rows = int(corpus.levels_rows(4_000)[-1])
            assert n_rows == 6 and corpus.n_frames == dev.F
            ctx.upload(d_lv, poison)
            ctx.graph_begin()
            try:
                assert ctx.corpus_levels_dev(corpus, 4_000, d_lv, n_rows) == BAD
            finally:
                try:
                    ctx.graph_destroy(ctx.graph_end())
                except x3.X3Error:
                    pass
            assert ctx.levels_result()[0] == BAD
            assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)
            assert ctx.corpus_levels_dev(corpus, 4_000, d_lv, n_rows) == 0
            assert ctx.levels_result() == (0, 0, dev.F, 0)
            _same(ctx.download(d_lv, 32 * n_rows, R.LEVEL_DTYPE), want[:n_rows], "corpus, one entry")
        finally:
            corpus.close()
    finally:
        dev.close()


# ---- 7. mirrors
def test_python_mirror_round_trip(ctx, x3):
    n = 30_000 + TAIL
    wav = _content("patchwork", n, seed=15)
    rc, stream, _ = O.encode(wav)
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, seg_blocks=32, index="walk")
    try:
        lv, st = ws.levels(1_000)
        assert lv.dtype == x3.LEVEL_DTYPE == R.LEVEL_DTYPE and lv.size == 34 and st.tolist() == [0, 0, 0, 0]
        frames = [wav[i:i + 10_000] for i in range(0, n, 10_000)]
        _same(lv, R.levels(frames, st, [0, 10_000, 20_000, 30_000], 1_000, 34), "WindowSource.levels")
        one, _ = ws.levels(0)
        assert one.size == 1 and int(one["n"][0]) == n and int(one["sum"][0]) == int(wav.astype(np.int64).sum())
        assert int(one["min"][0]) == int(wav.min()) and int(one["max"][0]) == int(wav.max())
        two, _ = ws.levels(1_000, n_bins=2)
        _same(two, lv[:2], "n_bins")
    finally:
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], index="walk")
    try:
        rows, rf, st = corpus.levels(1_000)
        assert rf.tolist() == [0, 34, 68] and not st.any()
        _same(rows[:34], lv, "Corpus.levels")
        _same(rows[34:], lv, "Corpus.levels")
    finally:
        corpus.close()


def test_x3_hpp_levels(tmp_path):
    """tests/host_cpp/test_levels_hpp.cpp: device::levels and device::Corpus::levels of the C++ mirror"""
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_levels_hpp.cpp")
    exe = str(tmp_path / "test_levels_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
