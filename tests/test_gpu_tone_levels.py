"""Tone levels (include/x3hip.h, "TONE LEVELS"): x3_tone_levels_dev, x3_corpus_tone_levels_dev, x3_tone_power_levels_dev and
their Python mirror.  Every field of every record is held with == against tone_levels_ref.py fed with the CPU oracle's
samples, as test_gpu_fir_levels.py (whose geometries and helpers these tests use) holds the FIR calls.  Shapes are small:
frames of 20 x 8 .. 20 x 64 samples unless a test needs the encoder's index, a late block of a long frame or 70 000 samples
in one bin."""
import ctypes as C

import numpy as np
import pytest

import diff_levels_ref as D
import events_ref as E
import fir_levels_ref as FR
import levels_ref as R
import oracle_lib as O
import quantiles_ref as Q
import test_gpu_fir_levels as TF
import test_gpu_levels as TL
import test_gpu_signal_levels as TS
import test_gpu_windows as TW
import test_tone_levels_ref as TRT
import tone_levels_ref as TR
import x3_cases as XC

pytestmark = pytest.mark.gpu

BAD, CRC, BPF, TAIL, CANARY = TL.BAD, TL.CRC, TL.BPF, TL.TAIL, TL.CANARY
ODD = 2_718_281_829                                     # an odd step drawn once
STEPS = [0, 1 << 30, 1 << 31, (1 << 32) - 1, ODD]
EXAMPLE_STEP = 350_898_828                               # round(0.0817 * 2^32)
ONES = np.tile(np.array([[1, 0]], dtype=np.int16), (1024, 1))
FULL = np.tile(np.array([[32767, -32768]], dtype=np.int16), (1024, 1))


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    for k in TR.TONE_DTYPE.names:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def _random_table(seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (1024, 2)).astype(np.int16)


def _table(dev, tab):
    """the device pointer of a table: None is the context's usual one, an array is uploaded (and freed with dev)"""
    if tab is None:
        return dev.ctx.tone_table_dev()
    d = dev.alloc(4096)
    dev.ctx.upload(d, np.ascontiguousarray(tab, dtype=np.int16))
    return d


def _tone(dev, bin_len, n_bins, step, d_tab=None, d_seg="own", sb=None):
    """x3_tone_levels_dev into a poisoned buffer with a canary behind it -> (records, frame statuses, result, replays)"""
    ctx = dev.ctx
    nb = 32 * n_bins
    d_lv, d_st = ctx.alloc(nb + 64), ctx.alloc(4 * dev.F + 64)
    try:
        ctx.upload(d_lv, np.full(nb + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * dev.F + 64, CANARY, dtype=np.uint8))
        idx = dev.d_seg if isinstance(d_seg, str) else d_seg
        tone = dev.x3.LevelTone(step, 0, d_tab or ctx.tone_table_dev())
        rc = ctx.tone_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, idx,
                                 (sb if sb is not None else dev.sb) if idx else 0, tone)
        tone.step, tone.d_table = 0xDEAD, 8                  # (the struct was copied at the call)
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.levels_result()
        replays = ctx.get_option("last_levels_replays")
        raw, raw_st = ctx.download(d_lv, nb + 64, np.uint8), ctx.download(d_st, 4 * dev.F + 64, np.uint8)
        assert (raw[nb:] == CANARY).all() and (raw_st[4 * dev.F:] == CANARY).all(), "written behind the buffers"
        st = raw_st[:4 * dev.F].view(np.int32).copy()
        bad = np.nonzero(st)[0]
        assert res == (0, bad.size, int(bad[0]) if bad.size else dev.F, int(st[bad[0]]) if bad.size else 0), (res, st)
        return raw[:nb].view(TR.TONE_DTYPE).copy(), st, res, replays
    finally:
        ctx.free(d_lv)
        ctx.free(d_st)


def _samples_fields(got, lv, what):
    for k in ("min", "max", "n"):
        assert np.array_equal(got[k], lv[k]), (what, k)
    assert not got["reserved"].any()


# ---- 1. the two identities, on the encoder's index (a recording's), a walk-built one and none
@pytest.mark.parametrize("kind", ["patchwork", "literal"])
def test_identities_on_a_stream(ctx, x3, kind):
    n = 30_000 + TAIL
    wav = TL._content(kind, n)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        assert dev.F == 4 and dev.sb == 32
        d_idx4, _ = TS._walk_index(ctx, x3, dev, 4)
        d_ones = _table(dev, ONES)
        for bin_len in (0, 1, 641, 10_000, 10_001):
            n_bins = R.n_bins_for(n, bin_len) + 1
            old, st_o, _, _ = TL._levels(dev, bin_len, n_bins)
            for what, seg, sb in (("encoder 32", "own", None), ("walk 4", d_idx4, 4), ("no index", None, None)):
                one, st, _, replays = _tone(dev, bin_len, n_bins, ODD, d_ones, d_seg=seg, sb=sb)
                assert np.array_equal(st, st_o) and replays == 0
                assert np.array_equal(one["re"], old["sum"]) and not one["im"].any(), (what, bin_len)
                _samples_fields(one, old, (what, bin_len))
                dc, st, _, replays = _tone(dev, bin_len, n_bins, 0, d_seg=seg, sb=sb)
                assert np.array_equal(dc["re"], 32767 * old["sum"]) and not dc["im"].any() and replays == 0, (what, bin_len)
                _samples_fields(dc, old, (what, bin_len))
    finally:
        dev.close()


# ---- 2. a recording's index (the encoder's at 32 blocks of 20: stretches begin mid-frame at 1 + 640 j), every step
@pytest.mark.parametrize("step", STEPS)
def test_steps_on_the_encoders_index(ctx, x3, step):
    n = 30_000 + TAIL
    wav = TL._content("patchwork", n, seed=21)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        frames, ok = TS._frames_of(dev, wav), [0] * dev.F
        tab = _random_table(step % 1000)
        d_tab = _table(dev, tab)
        for bin_len in (0, 1, 7, 100, 641, 9_999, 10_000, 10_001):
            n_bins = R.n_bins_for(n, bin_len)
            for t, d_t in ((None, None), (tab, d_tab)):
                want = TR.tone_levels(frames, ok, dev.so[:-1], bin_len, n_bins, step, t)
                for seg in ("own", None):
                    got, st, _, replays = _tone(dev, bin_len, n_bins, step, d_t, d_seg=seg)
                    assert not st.any() and replays == 0
                    _same(got, want, (step, bin_len, seg, t is None))
    finally:
        dev.close()


# ---- 3. steps over the geometries and code sets of the FIR tests
@pytest.mark.parametrize("bl,bpf,codes", TF.GEOMETRIES)
@pytest.mark.parametrize("step", STEPS)
def test_steps_over_geometry(ctx, x3, step, bl, bpf, codes):
    """nine frames and a short one per content kind; a walk-built index at 4 blocks (at block length 40 a stretch is 160
    samples and begins mid-frame) and none; with codes (1, 1, 3) frames fail to decode and add nothing"""
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf, codes), O.Params.make(bl, bpf, codes)
    n = 9 * spf + min(57, spf - 1)
    for kind in TL.KINDS:
        wav = TL._content(kind, n, seed=bl + bpf)
        rc, stream, _ = O.encode(wav, op)
        assert rc == 0
        dev = TW.Dev(ctx, x3, stream=stream, p=p)
        try:
            assert dev.F == 10
            frames, ost = TL._oracle_frames(stream, XC.frame_offsets(stream), op)
            assert tuple(codes) == (1, 1, 3) or not any(ost)
            indexes = TF._indexes(ctx, x3, dev)
            assert len(indexes) == 2
            for bin_len in (1, 7, 100, spf, spf - 1, spf + 1, 0):
                n_bins = R.n_bins_for(n, bin_len)
                want = TR.tone_levels(frames, ost, dev.so[:-1], bin_len, n_bins, step)
                _samples_fields(want, R.levels(frames, ost, dev.so[:-1], bin_len, n_bins), "reference")
                for what, seg in indexes:
                    got, st, _, replays = _tone(dev, bin_len, n_bins, step, d_seg=seg, sb=4)
                    assert st.tolist() == ost, (kind, what, st, ost)
                    _same(got, want, (kind, what, bin_len))
                    if not any(ost):
                        assert replays == 0 and int(got["n"].sum()) == n, (kind, what, bin_len)
        finally:
            dev.close()


# ---- 4. short streams
@pytest.mark.parametrize("n", [1, 2, 19, 20, 21, 1_281])
def test_short_streams_and_a_one_sample_last_frame(ctx, x3, n):
    """1 .. 21 samples round the block length of 20, and 1 281 in frames of 1 280: a last frame of one sample"""
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
        for step in STEPS:
            for bin_len in (0, 1, 5, 20):
                n_bins = R.n_bins_for(n, bin_len) + 1
                want = TR.tone_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, step)
                for seg, sb in ((d_idx32, 32), (d_idx4, 4), (None, 0)):
                    got, st, _, replays = _tone(dev, bin_len, n_bins, step, d_seg=seg, sb=sb)
                    assert not st.any() and replays == 0
                    _same(got, want, (n, step, sb, bin_len))
                    assert int(got["n"].sum()) == n and got[-1].tobytes() == TR.empty(1).tobytes()
    finally:
        dev.close()


# ---- 5. arithmetic edges
def _adapter(ctx, x3, rec, in_place):
    """x3_tone_power_levels_dev over the records `rec`, in place or into rows of their own, canaries behind both"""
    n = rec.size
    d_a, d_b = ctx.alloc(32 * n + 64), ctx.alloc(32 * n + 64)
    try:
        for d in (d_a, d_b):
            ctx.upload(d, np.full(32 * n + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_a, rec)
        assert ctx.tone_power_levels_dev(d_a, n, d_a if in_place else d_b) == 0, ctx.last_error()
        ctx.sync()
        a, b = ctx.download(d_a, 32 * n + 64, np.uint8), ctx.download(d_b, 32 * n + 64, np.uint8)
        assert (a[32 * n:] == CANARY).all() and (b[32 * n:] == CANARY).all()
        if in_place:
            assert (b == CANARY).all()
            return a[:32 * n].view(R.LEVEL_DTYPE).copy()
        assert a[:32 * n].tobytes() == rec.tobytes()                 # the tone records are read only
        return b[:32 * n].view(R.LEVEL_DTYPE).copy()
    finally:
        ctx.free(d_a)
        ctx.free(d_b)


def test_arithmetic_edges(ctx, x3):
    """a table of all (32767, -32768): a square wave between the ends of the scale, 72 000 samples, and 70 001 samples of
    -32768, whose im is n * 2^30 exactly -- the largest sum a bin can hold per sample; through the adapter both clamp"""
    square = np.concatenate([np.full(36_000, -32768), np.full(36_000, 32767)]).astype(np.int16)
    floor = np.full(70_001, -32768, dtype=np.int16)
    for wav in (square, floor):
        n = wav.size
        dev, _ = TL._encoded(ctx, x3, wav)
        try:
            d_full = _table(dev, FULL)
            frames = TS._frames_of(dev, wav)
            for bin_len in (0, 36_000):
                n_bins = R.n_bins_for(n, bin_len)
                want = TR.tone_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, ODD, FULL)
                for seg in ("own", None):
                    got, st, _, replays = _tone(dev, bin_len, n_bins, ODD, d_full, d_seg=seg)
                    assert not st.any() and replays == 0
                    _same(got, want, (n, bin_len, seg))
                s = int(wav.astype(np.int64).sum()) if bin_len == 0 else int(wav[:36_000].astype(np.int64).sum())
                assert (int(got["re"][0]), int(got["im"][0])) == (32767 * s, -32768 * s)
                if wav is floor or bin_len:
                    assert int(got["im"][0]) == int(got["n"][0]) << 30                  # n * 2^30: the bound
                for in_place in (True, False):
                    lv = _adapter(ctx, x3, got, in_place)
                    assert lv.tobytes() == TR.tone_power_levels(got).tobytes()
                    if wav is floor or bin_len:                                        # clamped both ways
                        k = int(got["n"][0])
                        assert (int(lv["sum_sq"][0]), int(lv["sum"][0]), int(lv["min"][0]), int(lv["max"][0]), int(lv["n"][0])) == \
                            ((1 << 30) * k, 0, -32767, 32767, k)
        finally:
            dev.close()


def test_the_adapter_on_crafted_records(ctx, x3):
    """test_tone_levels_ref.py's crafted records and random ones through the kernel, in place and out of place"""
    recs = []
    for n in (0, 1, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 32) - 1):
        for sre in (1, -1):
            for sim in (1, -1, 0):
                recs.append((sre * n * (1 << 30), sim * n * (1 << 30), -5, 9, n, 0))
    edges = [e for r in TRT.SQUARE_ROOTS for e in TRT.square_edge_records(r)]    # 2 * ms at r * r - 1, r * r, r * r + 1
    assert len(edges) == sum(1 for r in TRT.SQUARE_ROOTS for t in (r * r - 1, r * r, r * r + 1) if t % 2 == 0)   # every even one
    first_edge = len(recs)
    for target, re, im, n in edges:
        recs.append((re, im, 0, 0, n, 0))
    rng = np.random.default_rng(77)
    for _ in range(300):
        n = int(rng.integers(1, 1 << 32)) >> int(rng.integers(0, 32))
        n = max(n, 1)
        recs.append((int(rng.integers(-n, n + 1)) << int(rng.integers(0, 31)), int(rng.integers(-n, n + 1)) << int(rng.integers(0, 31)),
                     -1, 1, n, 0))
    rec = np.array(recs, dtype=TR.TONE_DTYPE)
    want = TR.tone_power_levels(rec)
    for r in rec:
        assert TR.power_record(r["re"], r["im"], r["n"])[1] < 1 << 62
    assert (want["sum_sq"] // np.maximum(want["n"], 1).astype(np.uint64) <= 1 << 30).all() and (want["max"] <= 32767).all()
    for in_place in (True, False):
        got = _adapter(ctx, x3, rec, in_place)
        assert got.tobytes() == want.tobytes()
        for k, (target, _, _, n) in enumerate(edges, first_edge):          # ... and the device's own figures at the edges
            assert 2 * (int(got["sum_sq"][k]) // n) == target and int(got["max"][k]) == min(32767, TR.isqrt(target)) == -int(got["min"][k])
        assert [int(v) for v in got["max"][first_edge + len(edges) - 2:first_edge + len(edges)]] == [32766, 32767]   # r = 32767
    # refusals: NULL, misaligned, no rows, too many, an overlap that is not "in place"
    d = ctx.alloc(32 * 8)
    try:
        for a, n, b in ((None, 4, d), (d, 4, None), (d + 4, 4, d), (d, 4, d + 4), (d, 0, d), (d, 1 << 31, d), (d, 4, d + 32),
                        (d + 96, 4, d), (d, 4, d + 96)):
            assert ctx.tone_power_levels_dev(a, n, b) == BAD, (a, n, b)
        assert x3.lib().x3_tone_power_levels_dev(None, d, 4, d) == BAD
        assert ctx.tone_power_levels_dev(d, 4, d + 128) == 0 and ctx.tone_power_levels_dev(d + 128, 4, d) == 0   # side by side
        ctx.sync()
    finally:
        ctx.free(d)


# ---- 6. damage
@pytest.mark.parametrize("where", [0, 4, 9])
def test_a_crc_damaged_frame_adds_nothing(ctx, x3, where):
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
        for step in (ODD, 1 << 31):
            for bin_len in (1, 0, 7, 100, spf, spf + 1):
                n_bins = R.n_bins_for(n, bin_len)
                want = TR.tone_levels(frames, ok, dev.so[:-1], bin_len, n_bins, step)
                for what, seg in TF._indexes(ctx, x3, dev):
                    got, st, res, replays = _tone(dev, bin_len, n_bins, step, d_seg=seg, sb=4)
                    assert st.tolist() == ok and res == (0, 1, where, CRC) and replays == 0
                    _same(got, want, (where, step, what, bin_len))
                    if bin_len == 1:                                  # its own records are identities, its neighbours' are not
                        a, b = where * spf, min((where + 1) * spf, n)
                        assert got[a:b].tobytes() == TR.empty(b - a).tobytes() and int(got["n"].sum()) == n - (b - a)
    finally:
        dev.close()


def test_a_late_decode_error_takes_the_whole_frame_back(ctx, x3):
    dev, s, offs, n = TF._late_error_stream(ctx, x3)
    try:
        frames, ost = TL._oracle_frames(s, offs, XC.oparams(dev.p))
        assert ost == [0, 0, 0, BPF, 0, 0, 0]
        for step in (ODD, (1 << 32) - 1):
            for bin_len in (641, 10_000, 0):
                n_bins = R.n_bins_for(n, bin_len)
                got, st, res, replays = _tone(dev, bin_len, n_bins, step)
                assert st.tolist() == ost and res == (0, 1, 3, BPF) and replays == 1
                _same(got, TR.tone_levels(frames, ost, dev.so[:-1], bin_len, n_bins, step), (step, bin_len))
                assert int(got["n"].sum()) == n - 10_000
    finally:
        dev.close()


@pytest.mark.parametrize("how", ["sample", "bit offset"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """entry 12 of frame 2 has a wrong sample or a wrong bit offset: the frame goes through the reader, whose lane seeds the
    phase with the frame's first position, and last_levels_replays says so"""
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
        for step in (ODD, 1 << 30):
            for bin_len in (1, 641, 10_001):
                n_bins = R.n_bins_for(n, bin_len)
                good, st0, _, rep0 = _tone(dev, bin_len, n_bins, step)
                got, st, _, replays = _tone(dev, bin_len, n_bins, step, d_seg=d_bad)
                assert rep0 == 0 and replays == 1 and not st.any() and not st0.any()
                assert got.tobytes() == good.tobytes()
                _same(got, TR.tone_levels(frames, [0] * 7, dev.so[:-1], bin_len, n_bins, step), (how, step, bin_len))
    finally:
        dev.close()


# ---- 7. corpus
@pytest.mark.parametrize("index,sb", [("walk", 4), ("decode", 32)])
def test_corpus_entries_are_each_the_stream_call_alone(ctx, x3, index, sb):
    """entries of one frame, one sample, seven samples, none, several frames with one damaged, and one repeated: every
    entry's rows are the stream call's on that entry alone, so the phase restarts at 0 with every entry"""
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
        for step in (ODD, 1 << 31, 0):
            tone = x3.Tone(step)
            for bin_len in (0, 1, 100):
                rows, rf, st = corpus.tone_levels(bin_len, tone)
                assert rows.dtype == x3.TONE_DTYPE
                assert np.array_equal(rf, R.corpus_row_first(corpus.entries["n_samples"], bin_len)) and rows.size == int(rf[-1])
                assert st.tolist() == [0, 0, 0, 0, CRC, 0, 0, 0, 0] and ctx.get_option("last_levels_replays") == 0
                ref_entries = []
                for e, s in enumerate(ents):
                    a, b = int(rf[e]), int(rf[e + 1])
                    if s.size == 0:
                        assert rows[a:b].tobytes() == TR.empty(1).tobytes()
                        ref_entries.append(([], [], [], 0))
                        continue
                    ws = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
                    try:
                        alone, _ = ws.tone_levels(bin_len, tone, b - a)
                    finally:
                        ws.close()
                    _same(rows[a:b], alone, ("alone", e, step, bin_len))
                    fo = XC.frame_offsets(s)
                    frames, ost = TL._oracle_frames(s, fo, op)
                    fst = [CRC if (e == 4 and f == 1) else ost[f] for f in range(len(fo))]
                    lens_f = [int(s[o + 4]) << 8 | int(s[o + 5]) for o in fo]
                    ref_entries.append((frames, fst, np.concatenate([[0], np.cumsum(lens_f)])[:-1], sum(lens_f)))
                want, rf3 = TR.corpus_tone_levels(ref_entries, bin_len, step)
                assert np.array_equal(rf3, rf)
                _same(rows, want, (step, bin_len))
                assert rows[int(rf[0]):int(rf[1])].tobytes() == rows[int(rf[6]):int(rf[7])].tobytes()    # the repeated entry
    finally:
        corpus.close()


# ---- 8. refusals and state
def test_refusals_and_pending_states(ctx, x3):
    L = x3.lib()
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 5 * 320 + 57
    wav = TL._content("patchwork", n, seed=14)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    d_idx, _ = TS._walk_index(ctx, x3, dev, 4)
    d_lv, d_old, d_st = dev.alloc(32 * 8), dev.alloc(32 * 8), dev.alloc(4 * dev.F)
    d_tab = ctx.tone_table_dev()
    frames = TS._frames_of(dev, wav)
    corpus = None
    try:
        def tone_of(step=ODD, reserved=0, table=d_tab):
            return x3.LevelTone(step, reserved, table)

        def call(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=d_idx, sb=4, bl=250, lv=d_lv, nb=8,
                 st=d_st, tone=tone_of()):
            return L.x3_tone_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, bl, lv, nb, st,
                                        C.byref(tone) if tone is not None else None)
        corpus = x3.Corpus(ctx, (dev.d_x3, dev.len), [0], [dev.len], params=dev.p, seg_blocks=4, index="walk")
        n_rows = int(corpus.levels_rows(250)[-1])
        assert n_rows == 7

        def ccall(c=ctx._h, k=corpus._h, bl=250, lv=d_lv, nr=n_rows, st=d_st, tone=tone_of()):
            return L.x3_corpus_tone_levels_dev(c, k, bl, lv, nr, st, C.byref(tone) if tone is not None else None)
        poison = np.full(32 * 8, CANARY, dtype=np.uint8)
        ctx.upload(d_lv, poison)
        # a levels call is pending: every refusal leaves its result intact
        assert ctx.levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, 250, d_old, 8, None, d_idx, 4) == 0
        tone_refused = [dict(tone=None), dict(tone=tone_of(table=None)), dict(tone=tone_of(table=d_tab + 2)),
                        dict(tone=tone_of(table=d_tab + 1)), dict(tone=tone_of(reserved=1)), dict(tone=tone_of(reserved=1 << 31))]
        refused = tone_refused + [dict(nb=0), dict(nb=1 << 31), dict(nf=0), dict(c=None), dict(x=None), dict(fo=None),
                                  dict(so=None), dict(lv=None), dict(lv=d_lv + 4), dict(st=d_st + 2), dict(idx=d_idx + 4),
                                  dict(sb=30), dict(params=x3.Params.make(codes=(0, 1, 4)))]
        for bad in refused:
            assert call(**bad) == BAD, bad
        for bad in tone_refused + [dict(k=None), dict(c=None), dict(nr=0), dict(nr=n_rows - 1), dict(nr=n_rows + 1), dict(lv=None),
                                   dict(lv=d_lv + 4), dict(st=d_st + 2)]:
            assert ccall(**bad) == BAD, bad
        ctx.graph_begin()                                                       # a context that records a graph
        try:
            assert call() == BAD and ccall() == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass                                                           # (a recording of nothing)
        assert ctx.levels_result() == (0, 0, dev.F, 0)                          # the pending call's, intact
        TL._same(ctx.download(d_old, 32 * 8, R.LEVEL_DTYPE), R.levels(frames, [0] * dev.F, dev.so[:-1], 250, 8), "pending")
        assert ctx.levels_result()[0] == BAD                                   # nothing else is pending
        ctx.sync()
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)    # ... and nothing was enqueued
        # a table at an address that is 4-byte aligned and no more; no status array
        d_odd = dev.alloc(4096 + 4)
        ctx.upload(d_odd + 4, TR.table())
        want = TR.tone_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, ODD)
        assert call(tone=tone_of(table=d_odd + 4), st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        _same(ctx.download(d_lv, 32 * 8, TR.TONE_DTYPE), want, "a table at 4 mod 8")
        assert ccall(st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        _same(ctx.download(d_lv, 32 * n_rows, TR.TONE_DTYPE), want[:n_rows], "corpus, one entry")
        # a tone call, a FIR call, a DIFF call and a SAMPLES call on one context: each is right
        for _ in range(2):
            got, _, _, _ = _tone(dev, 250, 8, ODD, d_seg=d_idx, sb=4)
            _same(got, want, "tone")
            fir, _, _, _ = TF._fir(dev, 250, 8, *TF.MIXED8, d_seg=d_idx, sb=4)
            TL._same(fir, FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, *TF.MIXED8), "fir")
            dif, _, _, _ = TS._levels(dev, 250, 8, TS.DIFF, d_seg=d_idx, sb=4)
            TL._same(dif, D.signal_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, D.DIFF), "diff")
            old, _, _, _ = TL._levels(dev, 250, 8, d_seg=d_idx, sb=4)
            TL._same(old, R.levels(frames, [0] * dev.F, dev.so[:-1], 250, 8), "samples")
    finally:
        if corpus is not None:
            corpus.close()
        dev.close()


# ---- 9. the adapter on the call's own records
def test_the_adapter_on_the_calls_own_records(ctx, x3):
    n = 30_000 + TAIL
    wav = TL._content("patchwork", n, seed=23)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        for step in (EXAMPLE_STEP, 0, 1 << 31):
            for bin_len in (0, 1, 100, 10_001):
                n_bins = R.n_bins_for(n, bin_len) + 1
                got, _, _, _ = _tone(dev, bin_len, n_bins, step)
                want = TR.tone_power_levels(got)
                for in_place in (True, False):
                    assert _adapter(ctx, x3, got, in_place).tobytes() == want.tobytes(), (step, bin_len, in_place)
                assert want[-1].tobytes() == R.empty(1).tobytes()
    finally:
        dev.close()


# ---- 10. the example: a tone burst under louder noise
def _example():
    w = np.random.RandomState(7).randint(-3000, 3001, 20_000).astype(np.int64)
    t = np.arange(4_400, 4_600)
    w[4_400:4_600] += np.rint(1_000 * np.sin(2 * np.pi * 0.0817 * t + 0.3)).astype(np.int64)
    return np.clip(w, -32768, 32767).astype(np.int16)


def test_a_tone_burst_under_louder_noise(ctx, x3):
    """uniform noise of +-3 000 with a 200-sample tone of amplitude 1 000 at 0.0817 fs on [4 400, 4 600), bins of 200.  By
    tone_levels_ref.py on the CPU: the band mean square (the adapter's sum_sq / n) is 655 216 in bin 22 and 150 707 at most
    elsewhere (bin 2), a ratio of 4.35, and the band peak of bin 22 is 1 144; the samples' mean square is 3 562 158 against
    3 460 551 (1.03), the first difference's ratio is 0.83 and {1, 0, -1}'s 0.85: no threshold on those isolates the burst."""
    import torch
    w = _example()
    assert round(0.0817 * 2 ** 32) == EXAMPLE_STEP
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [w[a:a + 2_000] for a in range(0, 20_000, 2_000)], range(0, 20_000, 2_000)
    tone = x3.Tone(EXAMPLE_STEP)
    assert tone == x3.Tone.at(0.0817, 1.0)
    tl = TR.tone_levels(frames, [0] * 10, so, 200, 100, EXAMPLE_STEP)
    band = TR.tone_power_levels(tl)
    ms = (band["sum_sq"] // band["n"]).astype(np.int64)
    assert int(ms[22]) == 655_216 and int(np.delete(ms, 22).max()) == 150_707 and int(ms[2]) == 150_707
    assert (int(tl["re"][22]), int(tl["im"][22]), int(band["max"][22])) == (1_635_481_371, 3_375_804_068, 1_144)
    assert (ms[22] >= 4 * np.delete(ms, 22)).all()
    others = {"samples": R.levels(frames, [0] * 10, so, 200, 100), "diff": D.signal_levels(frames, [0] * 10, so, 200, 100, D.DIFF),
              x3.Fir([1, 0, -1]): FR.fir_levels(frames, [0] * 10, so, 200, 100, [1, 0, -1])}
    assert int(others["samples"]["sum_sq"][22]) // 200 == 3_562_158
    rule, rrule = x3.EventRule.make(mean_sq_min=400_000), E.Rule(mean_sq_min=400_000)       # between 150 707 and 655 216
    ev, elv = E.stream_events(band, 20_000, 200, rrule)
    assert ev == [(4_400, 200)]
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        for signal, lv in others.items():
            got, st = ws.levels(200, signal=signal)
            assert not st.any()
            TL._same(got, lv, signal)
            m = (got["sum_sq"] // np.maximum(got["n"], 1)).astype(np.int64)
            assert 10 * int(m[22]) < 11 * int(np.delete(m, 22).max()), signal           # bin 22 below 1.1 x the loudest other bin
        got, st = ws.tone_levels(200, tone)
        assert not st.any() and got.dtype == x3.TONE_DTYPE
        _same(got, tl, "tone_levels")
        got, st = ws.levels(200, signal=tone)
        assert got.dtype == x3.LEVEL_DTYPE and got.tobytes() == band.tobytes()
        gm = (got["sum_sq"] // got["n"]).astype(np.int64)
        assert (gm[22] >= 4 * np.delete(gm, 22)).all()
        starts, lens, cnt, el = ws.events(200, rule, 4, signal=tone)
        _, wst, wln, wlv = E.slots(ev, elv, 4, False)
        assert int(cnt) == 1 and (int(starts[0]), int(lens[0])) == (4_400, 200)
        assert np.array_equal(starts.cpu().numpy().view(np.uint64), wst) and np.array_equal(lens.cpu().numpy().view(np.uint32), wln)
        assert np.array_equal(x3.event_levels_view(el), wlv)
        out, offsets, status = ws.ranges(starts, lens, padded_to=200)         # ... and the event, fed to ranges, is the burst
        assert isinstance(out, torch.Tensor) and not status.cpu().numpy().any()
        assert np.array_equal(out[0].cpu().numpy(), w[4_400:4_600])
        with pytest.raises(ValueError, match="not built yet"):
            ws.range_levels(starts, lens, 200, signal=tone)
    finally:
        ws.close()


# ---- 11. the Python mirror
def test_python_mirror(ctx, x3):
    import torch
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 3 * 320 + 57
    wav = TL._content("patchwork", n, seed=15)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    frames, so = [wav[i:i + 320] for i in range(0, n, 320)], list(range(0, n, 320))
    tone = x3.Tone(ODD)
    d_tab = ctx.tone_table_dev()
    assert d_tab == ctx.tone_table_dev() and np.array_equal(ctx.download(d_tab, 4096, np.int16).reshape(1024, 2), x3.tone_table())
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=4, index="walk")
    try:
        tl, st = ws.tone_levels(100, tone)
        assert tl.dtype == x3.TONE_DTYPE and tl.size == 11 and st.tolist() == [0, 0, 0, 0]
        want = TR.tone_levels(frames, st, so, 100, 11, ODD)
        _same(tl, want, "WindowSource.tone_levels")
        two, _ = ws.tone_levels(100, tone, n_bins=2)
        _same(two, tl[:2], "n_bins")
        one, _ = ws.tone_levels(0, tone)
        _same(one, TR.tone_levels(frames, st, so, 0, 1, ODD), "one bin")
        lv, _ = ws.levels(100, signal=tone)
        assert lv.tobytes() == TR.tone_power_levels(want).tobytes()
        # by hand: tone_levels_into, tone_power_levels_dev in place, events_into -- and events(signal=tone) gives the same
        rule = x3.EventRule.make(mean_sq_min=int(np.median(lv["sum_sq"] // np.maximum(lv["n"], 1))))
        starts, lens, cnt, el = ws.events(100, rule, 8, signal=tone)
        d_lv = ctx.alloc(32 * 11)
        dev = torch.device("cuda", torch.cuda.current_device())
        h_st, h_ln = torch.empty(8, dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.int32, device=dev)
        h_el, h_cnt = torch.empty((8, 32), dtype=torch.uint8, device=dev), torch.empty((), dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        try:
            assert ws.tone_levels_into(100, tone, d_lv, 11) == 0
            assert ctx.tone_power_levels_dev(d_lv, 11, d_lv) == 0
            assert ws.events_into(d_lv, 11, 100, rule, h_st.data_ptr(), h_ln.data_ptr(), h_el.data_ptr(), 8, h_cnt.data_ptr()) == 0
            assert ctx.events_result()[0] == 0 and ctx.levels_result() == (0, 0, 4, 0)
            assert ctx.download(d_lv, 32 * 11, x3.LEVEL_DTYPE).tobytes() == lv.tobytes()
            assert ws.levels_into(100, d_lv, 11, None, tone) == 0 and ctx.levels_result() == (0, 0, 4, 0)
            assert ctx.download(d_lv, 32 * 11, x3.LEVEL_DTYPE).tobytes() == lv.tobytes()
        finally:
            ctx.free(d_lv)
        assert int(cnt) == int(h_cnt) >= 1
        assert torch.equal(starts, h_st) and torch.equal(lens, h_ln) and torch.equal(el, h_el)
        ev, elv = E.stream_events(TR.tone_power_levels(want), n, 100, E.Rule(mean_sq_min=int(rule.mean_sq_min)))
        assert len(ev) == int(cnt) and [(int(a), int(b)) for a, b in zip(starts[:len(ev)], lens[:len(ev)])] == ev
        assert np.array_equal(x3.event_levels_view(el)[:len(ev)], elv)
        # quantiles and adaptive events take the keyword too
        v, k = ws.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [500_000, 1_000_000], signal=tone)
        ms = np.sort((lv["sum_sq"] // np.maximum(lv["n"], 1)).astype(np.int64))
        wv, wk = Q.stream_quantiles(lv, n, 100, Q.MEAN_SQ, [500_000, 1_000_000])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv) and np.array_equal(k.cpu().numpy().view(np.uint32), wk)
        assert int(wv[0][1]) == int(ms[-1])
        out = ws.adaptive_events(100, x3.ThresholdRule.make(mean_sq=(500_000, 2, 1, 0)), x3.EventRule.make(), 8, signal=tone)
        assert len(out) == 5 and int(out[2]) >= 0
        with pytest.raises(ValueError):
            ws.tone_levels(100, "tone")
        with pytest.raises(ValueError, match="not built yet"):
            ws.range_levels(starts, lens, 100, signal=tone)
    finally:
        ws.close()
    # the corpus keyword
    buf, offs, lens_b = TL._place_even([stream, stream])
    corpus = x3.Corpus(ctx, buf, offs, lens_b, params=p, seg_blocks=4, index="walk")
    try:
        rows, rf, st = corpus.levels(100, signal=tone)
        assert rf.tolist() == [0, 11, 22] and not st.any()
        assert rows[:11].tobytes() == lv.tobytes() and rows[11:].tobytes() == lv.tobytes()
        ent, starts2, lens2, cnt2, el2 = corpus.events(100, rule, 16, signal=tone)
        assert int(cnt2) == 2 * int(cnt) and ent[:int(cnt2)].tolist() == [0] * int(cnt) + [1] * int(cnt)
        assert starts2[:int(cnt)].tolist() == starts[:int(cnt)].tolist()
        v, k = corpus.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [1_000_000], signal=tone)
        assert v.cpu().numpy().reshape(-1).tolist() == [int(ms[-1])] * 2
        with pytest.raises(ValueError, match="not built yet"):
            corpus.range_levels(ent, starts2, lens2, 100, signal=tone)
    finally:
        corpus.close()
