"""Tone bank levels (include/x3hip.h, "TONE BANK LEVELS"): x3_tone_bank_levels_dev, x3_corpus_tone_bank_levels_dev and their
Python mirror.  ONE RULE is held: plane t of a bank call is, byte for byte, the single tone call at steps[t] -- every field
of every record of every plane with == against tone_bank_levels_ref.py (tone_levels_ref.py per step) fed with the CPU
oracle's samples, and against x3_tone_levels_dev itself.  Helpers, geometries and streams are test_gpu_tone_levels.py's and
test_gpu_fir_levels.py's.  Buffers are poisoned, with canaries behind n_tones * n_bins records and behind the statuses; the
struct's spare steps hold garbage and the struct is overwritten behind every call."""
import ctypes as C

import numpy as np
import pytest

import async_analysis_cases as AA
import async_cases as AC
import events_ref as E
import levels_ref as R
import oracle_lib as O
import test_gpu_fir_levels as TF
import test_gpu_levels as TL
import test_gpu_signal_levels as TS
import test_gpu_tone_levels as TT
import test_gpu_windows as TW
import tone_bank_levels_ref as B
import tone_levels_ref as TR
import x3_cases as XC

pytestmark = pytest.mark.gpu

BAD, CRC, BPF, TAIL, CANARY = TL.BAD, TL.CRC, TL.BPF, TL.TAIL, TL.CANARY
ODD = TT.ODD
# [0, 2^30, 2^31, 2^32 - 1, ODD] and duplicates; the first k are a bank of k
POOL = [ODD, 0, 1 << 30, ODD, 1 << 31, (1 << 32) - 1, 0, 1 << 30]
SIZES = [1, 2, 3, 4, 5, 8]          # both instance edges (2 | 3, 4 | 5), the spare slots of 3 and 5, and the single call
GARBAGE = 0xDEADBEEF                # in the struct's steps behind n_tones: never read


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _bank_struct(x3, steps, d_tab, reserved=0, n_tones=None):
    k = len(steps)
    return x3.LevelToneBank(k if n_tones is None else n_tones, reserved, d_tab,
                            (C.c_uint32 * 8)(*(list(steps) + [GARBAGE] * (8 - k))))


def _bank(dev, bin_len, n_bins, steps, d_tab=None, d_seg="own", sb=None):
    """x3_tone_bank_levels_dev into a poisoned buffer with a canary behind its len(steps) * n_bins records -> (records
    [K, n_bins], frame statuses, result, replays)"""
    ctx, k = dev.ctx, len(steps)
    nb = 32 * k * n_bins
    d_lv, d_st = ctx.alloc(nb + 64), ctx.alloc(4 * dev.F + 64)
    try:
        ctx.upload(d_lv, np.full(nb + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * dev.F + 64, CANARY, dtype=np.uint8))
        idx = dev.d_seg if isinstance(d_seg, str) else d_seg
        bank = _bank_struct(dev.x3, steps, d_tab or ctx.tone_table_dev())
        rc = ctx.tone_bank_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, idx,
                                      (sb if sb is not None else dev.sb) if idx else 0, bank)
        bank.n_tones, bank.d_table = 77, 8                   # (the struct was copied at the call)
        for t in range(8):
            bank.steps[t] = 0xDEAD
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.levels_result()
        replays = ctx.get_option("last_levels_replays")
        raw, raw_st = ctx.download(d_lv, nb + 64, np.uint8), ctx.download(d_st, 4 * dev.F + 64, np.uint8)
        assert (raw[nb:] == CANARY).all() and (raw_st[4 * dev.F:] == CANARY).all(), "written behind the buffers"
        st = raw_st[:4 * dev.F].view(np.int32).copy()
        bad = np.nonzero(st)[0]
        assert res == (0, bad.size, int(bad[0]) if bad.size else dev.F, int(st[bad[0]]) if bad.size else 0), (res, st)
        return raw[:nb].view(TR.TONE_DTYPE).reshape(k, n_bins).copy(), st, res, replays
    finally:
        ctx.free(d_lv)
        ctx.free(d_st)


def _same_planes(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for t in range(got.shape[0]):
        TT._same(got[t], want[t], (what, "plane", t))


# ---- 1. identity: every plane is the single GPU call and the reference
@pytest.mark.parametrize("k", SIZES)
def test_every_plane_is_the_single_call(ctx, x3, k):
    """the encoder's index (32 blocks: stretches begin mid-frame), a walk-built one at 4 blocks and none; the usual table and
    a random one; bin lengths round the frame's 10 000 samples"""
    n = 30_000 + TAIL
    wav = TL._content("patchwork", n, seed=21 + k)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        assert dev.F == 4 and dev.sb == 32
        frames, ok = TS._frames_of(dev, wav), [0] * dev.F
        d_idx4, _ = TS._walk_index(ctx, x3, dev, 4)
        tab = TT._random_table(k)
        d_tab = TT._table(dev, tab)
        steps = POOL[:k]
        for bin_len in (0, 1, 7, 641, 9_999, 10_000, 10_001):
            n_bins = R.n_bins_for(n, bin_len)
            for t_host, t_dev in ((None, None), (tab, d_tab)):
                want = B.tone_bank_levels(frames, ok, dev.so[:-1], bin_len, n_bins, steps, t_host)
                for what, seg, sb in (("encoder 32", "own", None), ("walk 4", d_idx4, 4), ("no index", None, None)):
                    got, st, _, replays = _bank(dev, bin_len, n_bins, steps, t_dev, d_seg=seg, sb=sb)
                    assert not st.any() and replays == 0
                    _same_planes(got, want, (k, bin_len, what, t_host is None))
                    assert int(got["n"].sum()) == k * n
                singles = {}
                for t, step in enumerate(steps):             # ... and the single call itself, once per distinct step
                    if step not in singles:
                        singles[step] = TT._tone(dev, bin_len, n_bins, step, t_dev)[0]
                    assert got[t].tobytes() == singles[step].tobytes(), (k, bin_len, t)
    finally:
        dev.close()


# ---- 2. plane strides
@pytest.mark.parametrize("bl,bpf,codes", TF.GEOMETRIES)
@pytest.mark.parametrize("k", [8, 3])
def test_plane_strides_over_geometry(ctx, x3, k, bl, bpf, codes):
    """nine frames and a short one per content kind, a walk-built index at 4 blocks and none.  Bins of spf - 1, spf, spf + 1:
    neighbouring frames share a boundary bin.  n_bins one fewer and one more than the bins that cover the stream: bins at or
    behind n_bins are dropped in every plane and nothing spills into plane t + 1.  With codes (1, 1, 3) frames fail to
    decode and add nothing, to no plane."""
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf, codes), O.Params.make(bl, bpf, codes)
    n = 9 * spf + min(57, spf - 1)
    steps = POOL[8 - k:]
    for kind in TL.KINDS:
        wav = TL._content(kind, n, seed=bl + bpf + k)
        rc, stream, _ = O.encode(wav, op)
        assert rc == 0
        dev = TW.Dev(ctx, x3, stream=stream, p=p)
        try:
            assert dev.F == 10
            frames, ost = TL._oracle_frames(stream, XC.frame_offsets(stream), op)
            assert tuple(codes) == (1, 1, 3) or not any(ost)
            indexes = TF._indexes(ctx, x3, dev)
            assert len(indexes) == 2
            for bin_len in (7, 100, spf - 1, spf, spf + 1, 0):
                cover = R.n_bins_for(n, bin_len)
                for n_bins in sorted({max(1, cover - 1), cover, cover + 1}):
                    want = B.tone_bank_levels(frames, ost, dev.so[:-1], bin_len, n_bins, steps)
                    for what, seg in indexes:
                        got, st, _, replays = _bank(dev, bin_len, n_bins, steps, d_seg=seg, sb=4)
                        assert st.tolist() == ost, (kind, what, st, ost)
                        _same_planes(got, want, (kind, what, bin_len, n_bins))
                        if n_bins > cover:
                            assert all(got[t][-1].tobytes() == TR.empty(1).tobytes() for t in range(k))
                        if not any(ost):
                            assert replays == 0
                            counted = n if n_bins >= cover else (cover - 1) * bin_len
                            assert got["n"].sum(axis=1).tolist() == [counted] * k, (kind, what, bin_len, n_bins)
        finally:
            dev.close()


# ---- 3. short streams
@pytest.mark.parametrize("n", [1, 2, 19, 20, 21, 1_281])
def test_short_streams_and_a_one_sample_last_frame(ctx, x3, n):
    p, op = x3.Params.make(20, 64), O.Params.make(20, 64, (0, 1, 3))
    wav = TL._content("bfp", n, seed=n)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    try:
        assert dev.F == (2 if n == 1_281 else 1) and int(dev.so[-1] - dev.so[-2]) == (1 if n == 1_281 else n)
        frames = TS._frames_of(dev, wav)
        d_idx32, _ = TS._walk_index(ctx, x3, dev, 32)
        d_idx4, _ = TS._walk_index(ctx, x3, dev, 4)
        for k in (2, 5, 8):
            steps = POOL[:k]
            for bin_len in (0, 1, 5, 20):
                n_bins = R.n_bins_for(n, bin_len) + 1
                want = B.tone_bank_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, steps)
                for seg, sb in ((d_idx32, 32), (d_idx4, 4), (None, 0)):
                    got, st, _, replays = _bank(dev, bin_len, n_bins, steps, d_seg=seg, sb=sb)
                    assert not st.any() and replays == 0
                    _same_planes(got, want, (n, k, sb, bin_len))
                    assert got["n"].sum(axis=1).tolist() == [n] * k
    finally:
        dev.close()


# ---- 4. the arithmetic edge
def test_one_bin_of_full_scale_in_all_eight_planes(ctx, x3):
    """70 001 samples of -32768 in one bin against a table of all (32767, -32768): im is n * 2^30 exactly, the largest sum a
    bin can hold per sample, in each of the 8 planes at once"""
    wav = np.full(70_001, -32768, dtype=np.int16)
    n = wav.size
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        d_full = TT._table(dev, TT.FULL)
        frames = TS._frames_of(dev, wav)
        steps = POOL
        want = B.tone_bank_levels(frames, [0] * dev.F, dev.so[:-1], 0, 1, steps, TT.FULL)
        for seg in ("own", None):
            got, st, _, replays = _bank(dev, 0, 1, steps, d_full, d_seg=seg)
            assert not st.any() and replays == 0
            _same_planes(got, want, seg)
            for t in range(8):
                assert (int(got["re"][t, 0]), int(got["im"][t, 0]), int(got["n"][t, 0])) == (-32768 * 32767 * n, n << 30, n)
    finally:
        dev.close()


# ---- 5. rollback and fix-up, in every plane
@pytest.mark.parametrize("where", [0, 4, 9])
def test_a_crc_damaged_frame_adds_nothing_to_any_plane(ctx, x3, where):
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    spf, n = 320, 9 * 320 + 57
    wav = TL._content("patchwork", n, seed=13)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    s = stream.copy()
    s[XC.frame_offsets(stream)[where] + 20 + 33] ^= 0x10
    dev = TW.Dev(ctx, x3, stream=s, p=p)
    try:
        ok = [CRC if f == where else 0 for f in range(10)]
        frames = TS._frames_of(dev, wav)
        for k in (3, 8):
            steps = POOL[:k]
            for bin_len in (1, 0, 7, 100, spf, spf + 1):
                n_bins = R.n_bins_for(n, bin_len)
                want = B.tone_bank_levels(frames, ok, dev.so[:-1], bin_len, n_bins, steps)
                for what, seg in TF._indexes(ctx, x3, dev):
                    got, st, res, replays = _bank(dev, bin_len, n_bins, steps, d_seg=seg, sb=4)
                    assert st.tolist() == ok and res == (0, 1, where, CRC) and replays == 0
                    _same_planes(got, want, (where, k, what, bin_len))
                    if bin_len == 1:                                  # its own records are identities, in every plane
                        a, b = where * spf, min((where + 1) * spf, n)
                        for t in range(k):
                            assert got[t, a:b].tobytes() == TR.empty(b - a).tobytes() and int(got[t]["n"].sum()) == n - (b - a)
    finally:
        dev.close()


def test_a_late_decode_error_takes_the_whole_frame_back_in_every_plane(ctx, x3):
    dev, s, offs, n = TF._late_error_stream(ctx, x3)
    try:
        frames, ost = TL._oracle_frames(s, offs, XC.oparams(dev.p))
        assert ost == [0, 0, 0, BPF, 0, 0, 0]
        for k in (2, 5, 8):
            steps = POOL[:k]
            for bin_len in (641, 10_000, 0):
                n_bins = R.n_bins_for(n, bin_len)
                got, st, res, replays = _bank(dev, bin_len, n_bins, steps)
                assert st.tolist() == ost and res == (0, 1, 3, BPF) and replays == 1
                _same_planes(got, B.tone_bank_levels(frames, ost, dev.so[:-1], bin_len, n_bins, steps), (k, bin_len))
                assert got["n"].sum(axis=1).tolist() == [n - 10_000] * k
    finally:
        dev.close()


@pytest.mark.parametrize("how", ["sample", "bit offset"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """entry 12 of frame 2 has a wrong sample or a wrong bit offset: the frame goes through the reader -- the fix-up instance,
    which writes slot t at plane stride n_bins into the caller's records -- and last_levels_replays says so"""
    n = 60_000 + TAIL
    wav = TL._content("patchwork", n, seed=11)
    dev, stream = TL._encoded(ctx, x3, wav)
    try:
        idx, ne = TL._index_words(ctx, x3, dev)
        pitch = (ne - 1) // dev.F
        at = 1 + 2 * pitch + 11
        assert (int(idx[at]) >> 48) & 1
        idx[at] = np.uint64(int(idx[at]) ^ (0x1234 << 32)) if how == "sample" else np.uint64(int(idx[at]) + 1)
        d_bad = dev.alloc(8 * ne)
        ctx.upload(d_bad, idx)
        frames = TS._frames_of(dev, wav)
        for k in (2, 3, 8):
            steps = POOL[:k]
            for bin_len in (1, 641, 10_001, 0):
                n_bins = R.n_bins_for(n, bin_len) + 1
                good, st0, _, rep0 = _bank(dev, bin_len, n_bins, steps)
                got, st, _, replays = _bank(dev, bin_len, n_bins, steps, d_seg=d_bad)
                assert rep0 == 0 and replays == 1 and not st.any() and not st0.any()
                assert got.tobytes() == good.tobytes()
                _same_planes(got, B.tone_bank_levels(frames, [0] * 7, dev.so[:-1], bin_len, n_bins, steps), (how, k, bin_len))
    finally:
        dev.close()


# ---- 6. corpus
@pytest.mark.parametrize("index,sb", [("walk", 4), ("decode", 32)])
def test_corpus_entries_are_each_the_stream_call_alone_in_every_plane(ctx, x3, index, sb):
    """test_gpu_tone_levels.py's entries (one frame, one sample, seven samples, none, several frames with one damaged, one
    repeated): the plane stride is the corpus's rows, not an entry's; every entry starts at phase 0 in every plane"""
    p = x3.Params.make(20, 16) if index == "walk" else x3.Params.default()
    op = XC.oparams(p)
    spf = int(p.block_len) * int(p.blocks_per_frame)
    clips = [TL._content("patchwork", spf, seed=51), TL._content("bfp", 1, seed=52), TL._content("literal", 7, seed=53),
             np.zeros(0, dtype=np.int16), TL._content("rice3", 3 * spf + 19, seed=54), TL._content("bfp", 8, seed=55)]
    ents = TF._corpus_entries(x3, op, clips, damage=(4, 1))
    ents.append(ents[0])
    buf, offs, lens = TL._place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=sb, index=index)
    try:
        assert corpus.entries["n_frames"].tolist() == [1, 1, 1, 0, 4, 1, 1]
        ref_entries = []
        for e, s in enumerate(ents):
            if s.size == 0:
                ref_entries.append(([], [], [], 0))
                continue
            fo = XC.frame_offsets(s)
            frames, ost = TL._oracle_frames(s, fo, op)
            fst = [CRC if (e == 4 and f == 1) else ost[f] for f in range(len(fo))]
            lens_f = [int(s[o + 4]) << 8 | int(s[o + 5]) for o in fo]
            ref_entries.append((frames, fst, np.concatenate([[0], np.cumsum(lens_f)])[:-1], sum(lens_f)))
        for k in (1, 2, 3, 8):                                         # the single call and each of the three bank instances
            tones = tuple(x3.Tone(s) for s in POOL[:k])
            for bin_len in (0, 1, 100):
                rows, rf, st = corpus.tone_bank_levels(bin_len, tones)
                assert rows.dtype == x3.TONE_DTYPE and rows.shape == (k, int(rf[-1]))
                assert np.array_equal(rf, R.corpus_row_first(corpus.entries["n_samples"], bin_len))
                assert st.tolist() == [0, 0, 0, 0, CRC, 0, 0, 0, 0] and ctx.get_option("last_levels_replays") == 0
                want, rf3 = B.corpus_tone_bank_levels(ref_entries, bin_len, POOL[:k])
                assert np.array_equal(rf3, rf)
                _same_planes(rows, want, (k, bin_len))
                for t, tone in enumerate(tones):                       # the single corpus call, plane by plane
                    one, rf1, _ = corpus.tone_levels(bin_len, tone)
                    assert np.array_equal(rf1, rf) and rows[t].tobytes() == one.tobytes(), (k, bin_len, t)
                    assert rows[t, int(rf[0]):int(rf[1])].tobytes() == rows[t, int(rf[6]):int(rf[7])].tobytes()    # the repeated entry
            for e in (0, 4):                                           # ... and the stream call on an entry alone
                ws = x3.WindowSource(ctx, ents[e], p, seg_blocks=4, index="walk")
                try:
                    a, b = int(rf[e]), int(rf[e + 1])
                    alone, _ = ws.tone_bank_levels(100, tones, b - a)
                finally:
                    ws.close()
                assert alone.tobytes() == np.ascontiguousarray(rows[:, a:b]).tobytes(), (k, e)
    finally:
        corpus.close()


# ---- 7. refusals and state
def test_refusals_and_pending_states(ctx, x3):
    L = x3.lib()
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 5 * 320 + 57
    wav = TL._content("patchwork", n, seed=14)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    d_idx, _ = TS._walk_index(ctx, x3, dev, 4)
    K, NB = 3, 8
    d_lv, d_old, d_st = dev.alloc(32 * K * NB), dev.alloc(32 * NB), dev.alloc(4 * dev.F)
    d_tab = ctx.tone_table_dev()
    frames = TS._frames_of(dev, wav)
    steps = POOL[:K]
    corpus = None
    try:
        def bank_of(steps=steps, reserved=0, table=d_tab, n_tones=None):
            return _bank_struct(x3, steps, table, reserved, n_tones)

        def call(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=d_idx, sb=4, bl=250, lv=d_lv, nb=NB,
                 st=d_st, bank=bank_of()):
            return L.x3_tone_bank_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, bl, lv, nb, st,
                                             C.byref(bank) if bank is not None else None)
        corpus = x3.Corpus(ctx, (dev.d_x3, dev.len), [0], [dev.len], params=dev.p, seg_blocks=4, index="walk")
        n_rows = int(corpus.levels_rows(250)[-1])
        assert n_rows == 7

        def ccall(c=ctx._h, k=corpus._h, bl=250, lv=d_lv, nr=n_rows, st=d_st, bank=bank_of()):
            return L.x3_corpus_tone_bank_levels_dev(c, k, bl, lv, nr, st, C.byref(bank) if bank is not None else None)
        poison = np.full(32 * K * NB, CANARY, dtype=np.uint8)
        ctx.upload(d_lv, poison)
        # a levels call is pending: every refusal leaves its result intact
        assert ctx.levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, 250, d_old, NB, None, d_idx, 4) == 0
        bank_refused = [dict(bank=None), dict(bank=bank_of(n_tones=0)), dict(bank=bank_of(n_tones=9)),
                        dict(bank=bank_of(n_tones=1 << 31)), dict(bank=bank_of(reserved=1)), dict(bank=bank_of(reserved=1 << 31)),
                        dict(bank=bank_of(table=None)), dict(bank=bank_of(table=d_tab + 2)), dict(bank=bank_of(table=d_tab + 1))]
        # n_tones * n_bins > 2^31 - 1 with n_bins itself legal: 3 * 715 827 883 = 2^31 + 1; 8 * 2^28 = 2^31
        too_many = [dict(nb=715_827_883), dict(nb=1 << 28, bank=bank_of(steps=POOL))]
        refused = bank_refused + too_many + [dict(nb=0), dict(nb=1 << 31), dict(nf=0), dict(c=None), dict(x=None), dict(fo=None),
                                             dict(so=None), dict(lv=None), dict(lv=d_lv + 4), dict(st=d_st + 2), dict(idx=d_idx + 4),
                                             dict(sb=30), dict(params=x3.Params.make(codes=(0, 1, 4)))]
        for bad in refused:
            assert call(**bad) == BAD, bad
        for bad in bank_refused + [dict(k=None), dict(c=None), dict(nr=0), dict(nr=n_rows - 1), dict(nr=n_rows + 1), dict(lv=None),
                                   dict(lv=d_lv + 4), dict(st=d_st + 2)]:
            assert ccall(**bad) == BAD, bad
        for one in (bank_of(steps=steps[:1], n_tones=0), bank_of(steps=steps[:1], reserved=1), bank_of(steps=steps[:1], table=None)):
            assert call(bank=one) == BAD and ccall(bank=one) == BAD            # (one tone is refused by the same rules)
        ctx.graph_begin()                                                       # a context that records a graph
        try:
            assert call() == BAD and ccall() == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass                                                           # (a recording of nothing)
        assert ctx.levels_result() == (0, 0, dev.F, 0)                          # the pending call's, intact
        TL._same(ctx.download(d_old, 32 * NB, R.LEVEL_DTYPE), R.levels(frames, [0] * dev.F, dev.so[:-1], 250, NB), "pending")
        assert ctx.levels_result()[0] == BAD                                   # nothing else is pending
        ctx.sync()
        assert np.array_equal(ctx.download(d_lv, 32 * K * NB, np.uint8), poison)    # ... and nothing was enqueued
        # a table at an address that is 4-byte aligned and no more; no status array; the largest legal n_tones * n_bins needs no
        # such buffer here, so the bound is held by the refusals above
        d_odd = dev.alloc(4096 + 4)
        ctx.upload(d_odd + 4, TR.table())
        want = B.tone_bank_levels(frames, [0] * dev.F, dev.so[:-1], 250, NB, steps)
        assert call(bank=bank_of(table=d_odd + 4), st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        _same_planes(ctx.download(d_lv, 32 * K * NB, TR.TONE_DTYPE).reshape(K, NB), want, "a table at 4 mod 8")
        assert ccall(st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        _same_planes(ctx.download(d_lv, 32 * K * n_rows, TR.TONE_DTYPE).reshape(K, n_rows), want[:, :n_rows], "corpus, one entry")
        # two bank calls without a result call between them: the second's result is the one that is pending
        assert call() == 0 and call(bank=bank_of(steps=steps[:2])) == 0
        assert ctx.levels_result() == (0, 0, dev.F, 0) and ctx.levels_result()[0] == BAD
        _same_planes(ctx.download(d_lv, 32 * 2 * NB, TR.TONE_DTYPE).reshape(2, NB), want[:2], "the second call's planes")
        # a bank call, a tone call and a SAMPLES call on one context, twice over: each is right (the workspace grows and shrinks)
        for _ in range(2):
            got, _, _, _ = _bank(dev, 250, NB, POOL, d_seg=d_idx, sb=4)
            _same_planes(got, B.tone_bank_levels(frames, [0] * dev.F, dev.so[:-1], 250, NB, POOL), "bank")
            one, _, _, _ = TT._tone(dev, 250, NB, ODD, d_seg=d_idx, sb=4)
            TT._same(one, want[0], "tone")
            old, _, _, _ = TL._levels(dev, 250, NB, d_seg=d_idx, sb=4)
            TL._same(old, R.levels(frames, [0] * dev.F, dev.so[:-1], 250, NB), "samples")
    finally:
        if corpus is not None:
            corpus.close()
        dev.close()


# ---- 8. the chain: the adapter over all planes in one launch, and the example end to end
def test_the_adapter_takes_all_planes_in_one_launch(ctx, x3):
    n = 30_000 + TAIL
    wav = TL._content("patchwork", n, seed=23)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        frames = TS._frames_of(dev, wav)
        for k in (3, 8):
            steps = POOL[:k]
            for bin_len in (0, 100, 10_001):
                n_bins = R.n_bins_for(n, bin_len) + 1
                got, _, _, _ = _bank(dev, bin_len, n_bins, steps)
                want = B.tone_bank_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, steps)
                for in_place in (True, False):
                    lv = TT._adapter(ctx, x3, got.reshape(-1), in_place).reshape(k, n_bins)
                    for t in range(k):
                        assert lv[t].tobytes() == TR.tone_power_levels(want[t]).tobytes(), (k, bin_len, in_place, t)
    finally:
        dev.close()


def test_two_bursts_and_a_bank_of_four(ctx, x3):
    """DESIGN.md section 26's example end to end: tone_bank_levels(..., band=True), then events per plane.  By
    tone_bank_levels_ref.py on the CPU (test_tone_bank_levels_ref.py asserts the figures): the band mean square is 655 216 in
    bin 22 of plane 0 (150 707 elsewhere), 518 188 in bin 60 of plane 1 (138 273 elsewhere), 322 926 at most in plane 2 and
    150 040 in plane 3, so mean_sq_min = 400 000 finds (4 400, 200) in plane 0, (12 000, 200) in plane 1 and nothing else"""
    import torch
    w = B.example()
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [w[a:a + 2_000] for a in range(0, 20_000, 2_000)], range(0, 20_000, 2_000)
    tones = x3.Tone.bank(B.EXAMPLE_FREQS, 1.0)
    assert tuple(t.step for t in tones) == B.EXAMPLE_STEPS
    planes = B.tone_bank_levels(frames, [0] * 10, so, 200, 100, B.EXAMPLE_STEPS)
    bands = [TR.tone_power_levels(pl) for pl in planes]
    rule, rrule = x3.EventRule.make(mean_sq_min=400_000), E.Rule(mean_sq_min=400_000)
    found = [E.stream_events(b, 20_000, 200, rrule) for b in bands]
    assert [ev for ev, _ in found] == [[(4_400, 200)], [(12_000, 200)], [], []]
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_lv = ctx.alloc(32 * 4 * 100)
    try:
        got, st = ws.tone_bank_levels(200, tones)
        assert not st.any() and got.dtype == x3.TONE_DTYPE
        _same_planes(got, planes, "tone_bank_levels")
        lv, st = ws.tone_bank_levels(200, tones, band=True)
        assert lv.dtype == x3.LEVEL_DTYPE and lv.shape == (4, 100) and not st.any()
        for t in range(4):
            assert lv[t].tobytes() == bands[t].tobytes(), t
        ms = (lv["sum_sq"] // lv["n"]).astype(np.int64)
        assert [(int(m.argmax()), int(m.max())) for m in ms] == [(22, 655_216), (60, 518_188), (19, 322_926), (34, 150_040)]
        # on the device: the bank with the adapter in place, then x3_events_dev on every plane as it lies
        assert ws.tone_bank_levels_into(200, tones, d_lv, 100, band=True) == 0 and ctx.levels_result() == (0, 0, 10, 0)
        for t, (ev, elv) in enumerate(found):
            h_st, h_ln = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
            h_el, h_cnt = torch.empty((4, 32), dtype=torch.uint8, device=dev), torch.empty((), dtype=torch.int64, device=dev)
            torch.cuda.current_stream().synchronize()
            assert ws.events_into(d_lv + 32 * 100 * t, 100, 200, rule, h_st.data_ptr(), h_ln.data_ptr(), h_el.data_ptr(), 4,
                                  h_cnt.data_ptr()) == 0
            assert ctx.events_result()[0] == 0
            _, wst, wln, wlv = E.slots(ev, elv, 4, False)
            assert int(h_cnt) == len(ev), t
            assert np.array_equal(h_st.cpu().numpy().view(np.uint64), wst) and np.array_equal(h_ln.cpu().numpy().view(np.uint32), wln)
            assert np.array_equal(x3.event_levels_view(h_el), wlv)
        out, offsets, status = ws.ranges(torch.tensor([4_400, 12_000], dtype=torch.int64, device=dev),
                                         torch.tensor([200, 200], dtype=torch.int32, device=dev), padded_to=200)
        assert not status.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), np.stack([w[4_400:4_600], w[12_000:12_200]]))
    finally:
        ctx.free(d_lv)
        ws.close()


# ---- 9. the asynchronous contract: a bank call behind a stalled caller stream whose inputs still hold a decoy
class BankBehindAStall(AA.LevelsCase):
    """x3_tone_bank_levels_dev of three tones with the frame statuses, on damaged content: every record of every plane,
    d_frame_status and x3_levels_result"""
    STEPS = (ODD, 1 << 31, 350_898_828)

    def __init__(self):
        self.name, self.signal, self.content = "tone_bank_levels_damaged", "bank", "Bd"

    def own_outputs(self):
        return {"lv": 32 * len(self.STEPS) * AA.NB, "fst": 4 * AA.F0}

    def enqueue(self, x3, ctx, d, which, probe):
        src = self.prelude(x3, ctx, d)
        rc = ctx.tone_bank_levels_dev(*(src + (AA.BIN, d["lv"], AA.NB, d["fst"], d["seg"], AA.SB)),
                                      tones=[x3.Tone(s) for s in self.STEPS])
        assert rc == 0, ctx.last_error()

    def own_expect(self, which):
        k = self.kind(which)
        st = AA.stream(k)[1]
        planes = B.tone_bank_levels(AA.wav_frames(k), st, AA.SO[:-1], AA.BIN, AA.NB, self.STEPS)
        return {"lv": [(0, planes.reshape(-1), False)], "fst": [(0, st, False)]}, {"levels": AA.summary(st)}


def test_behind_a_stalled_stream():
    import torch
    import x3hip
    AC.run_stalled(x3hip, torch, BankBehindAStall(), AC.calibrate_sleep(torch))


# ---- 10. the Python mirror
def test_python_mirror(ctx, x3):
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 3 * 320 + 57
    wav = TL._content("patchwork", n, seed=15)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    frames, so = [wav[i:i + 320] for i in range(0, n, 320)], list(range(0, n, 320))
    tones = [x3.Tone(s) for s in POOL[:5]]
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=4, index="walk")
    try:
        tl, st = ws.tone_bank_levels(100, tones)
        assert tl.dtype == x3.TONE_DTYPE and tl.shape == (5, 11) and st.dtype == np.int32 and st.tolist() == [0, 0, 0, 0]
        want = B.tone_bank_levels(frames, st, so, 100, 11, POOL[:5])
        _same_planes(tl, want, "WindowSource.tone_bank_levels")
        two, _ = ws.tone_bank_levels(100, tuple(tones), n_bins=2)
        assert two.shape == (5, 2) and two.tobytes() == np.ascontiguousarray(tl[:, :2]).tobytes()
        one, _ = ws.tone_bank_levels(0, tones[:1])
        assert one.shape == (1, 1) and one[0].tobytes() == ws.tone_levels(0, tones[0])[0].tobytes()
        lv, _ = ws.tone_bank_levels(100, tones, band=True)
        assert lv.dtype == x3.LEVEL_DTYPE and lv.shape == (5, 11)
        for t in range(5):
            assert lv[t].tobytes() == TR.tone_power_levels(want[t]).tobytes()
            assert lv[t].tobytes() == ws.levels(100, signal=tones[t])[0].tobytes()       # the keyword's records, plane by plane
        for bad in ((), tones + tones, tones[0], [1, 2], None):
            with pytest.raises(ValueError, match="1 .. 8 Tone"):
                ws.tone_bank_levels(100, bad)
        with pytest.raises(x3.X3Error):
            ws.tone_bank_levels(100, tones, n_bins=0)
        with pytest.raises(ValueError):
            ws.levels(100, signal=tuple(tones))                                          # the keyword takes no bank
    finally:
        ws.close()
    buf, offs, lens_b = TL._place_even([stream, stream])
    corpus = x3.Corpus(ctx, buf, offs, lens_b, params=p, seg_blocks=4, index="walk")
    try:
        rows, rf, st = corpus.tone_bank_levels(100, tones)
        assert rows.shape == (5, 22) and rf.tolist() == [0, 11, 22] and not st.any()
        assert rows[:, :11].tobytes() == tl.tobytes() and rows[:, 11:].tobytes() == tl.tobytes()
        band, rf, _ = corpus.tone_bank_levels(100, tones, band=True)
        assert band.dtype == x3.LEVEL_DTYPE and band[:, :11].tobytes() == lv.tobytes() and band[:, 11:].tobytes() == lv.tobytes()
        with pytest.raises(ValueError, match="1 .. 8 Tone"):
            corpus.tone_bank_levels(100, [])
    finally:
        corpus.close()
