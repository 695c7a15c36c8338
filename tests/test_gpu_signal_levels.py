"""Signal levels (include/x3hip.h, "SIGNAL LEVELS"): x3_signal_levels_dev, x3_corpus_signal_levels_dev and their mirrors.
Every field of every record is held with == against diff_levels_ref.py fed with the CPU oracle's samples, as
test_gpu_levels.py (whose helpers these tests use) holds x3_levels_dev against levels_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diff_levels_ref as D
import events_ref as E
import levels_ref as R
import oracle_lib as O
import quantiles_ref as Q
import test_gpu_levels as TL
import test_gpu_windows as TW
import x3_cases as XC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, CRC, BPF, TAIL, CANARY = TL.BAD, TL.CRC, TL.BPF, TL.TAIL, TL.CANARY
BIN_LENS = [0, 1, 7, 20, 640, 641, 10_000, 10_001, 1 << 20]
SAMPLES, DIFF = D.SAMPLES, D.DIFF
_same = TL._same


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _levels(dev, bin_len, n_bins, signal=DIFF, d_seg="own", sb=None, d_off=None):
    """x3_signal_levels_dev into a poisoned buffer with a canary behind it -> (records, frame statuses, result, replays)"""
    ctx = dev.ctx
    nb = 32 * n_bins
    d_lv, d_st = ctx.alloc(nb + 64), ctx.alloc(4 * dev.F + 64)
    try:
        ctx.upload(d_lv, np.full(nb + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * dev.F + 64, CANARY, dtype=np.uint8))
        idx = dev.d_seg if isinstance(d_seg, str) else d_seg
        rc = ctx.signal_levels_dev(dev.d_x3, dev.len, d_off or dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st,
                                   idx, (sb if sb is not None else dev.sb) if idx else 0, signal)
        assert rc == 0, (rc, ctx.last_error())
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


def _walk_index(ctx, x3, dev, sb):
    """x3_seg_index_build_dev's index of dev's stream at sb blocks per entry -> (device pointer, words)"""
    ne = x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), sb)
    assert ne > 0
    d_idx = dev.alloc(8 * ne)
    assert ctx.seg_index_build_dev(dev.d_x3, dev.len, dev.d_off, dev.F, dev.p, d_idx, sb) == 0
    return d_idx, ne


def _frames_of(dev, wav):
    return [wav[int(a):int(b)] for a, b in zip(dev.so[:-1], dev.so[1:])]


# ---- 1. exactness over bin geometry
@pytest.mark.parametrize("kind", TL.KINDS)
def test_exact_over_bin_geometry(ctx, x3, kind):
    """seven frames (the last of 3 457 samples); the encoder's index at 32 blocks (stretches of 640 samples) and a walk-built
    one at 4 (125 stretches a frame); DIFF against the definition, SAMPLES byte for byte x3_levels_dev's records"""
    n = 60_000 + TAIL
    wav = TL._content(kind, n)
    dev, stream = TL._encoded(ctx, x3, wav)
    try:
        assert dev.F == 7 and dev.sb == 32 and dev.total == n
        d_idx4, _ = _walk_index(ctx, x3, dev, 4)
        frames, ok = _frames_of(dev, wav), [0] * dev.F
        for bin_len in BIN_LENS:
            exact = R.n_bins_for(n, bin_len)
            for n_bins in sorted({exact, max(1, exact - 1), exact + 3}):
                want = D.signal_levels(frames, ok, dev.so[:-1], bin_len, n_bins, DIFF)
                for what, seg, sb in (("encoder 32", "own", None), ("walk 4", d_idx4, 4)):
                    got, st, res, replays = _levels(dev, bin_len, n_bins, DIFF, d_seg=seg, sb=sb)
                    assert not st.any() and replays == 0, (what, bin_len, n_bins, st, replays)
                    _same(got, want, (kind, what, bin_len, n_bins))
            got, _, _, _ = _levels(dev, bin_len, exact, DIFF)
            assert int(got["n"].sum()) == n - 1
            if bin_len == 1:                       # position-exact: every difference in a record of its own, none at 0
                assert int(got["n"][0]) == 0 and (got["n"][1:] == 1).all()
                d = np.clip(np.diff(wav.astype(np.int64)), -32768, 32767)
                assert np.array_equal(got["sum"][1:], d) and np.array_equal(got["min"][1:], d)
            same, st_s, _, _ = _levels(dev, bin_len, exact, SAMPLES)
            old, st_o, _, _ = TL._levels(dev, bin_len, exact)
            assert same.tobytes() == old.tobytes() and np.array_equal(st_s, st_o), bin_len
    finally:
        dev.close()


# ---- 2. seams
def _one_sample_frames(values, op):
    """a stream whose frames hold one sample each: every value encoded on its own, the frames back to back"""
    parts = []
    for v in values:
        rc, s, _ = O.encode(np.array([v], dtype=np.int16), op)
        assert rc == 0
        parts.append(s)
    return np.concatenate(parts)


def test_one_frame_and_one_sample_streams(ctx, x3):
    p, op = x3.Params.default(), XC.oparams(x3.Params.default())
    for n in (777, 2, 1):
        wav = TL._content("rice3", n, seed=n)
        dev, _ = TL._encoded(ctx, x3, wav)
        try:
            assert dev.F == 1
            for bin_len in (0, 1, 100):
                n_bins = R.n_bins_for(n, bin_len) + 1
                got, st, _, replays = _levels(dev, bin_len, n_bins, DIFF)
                assert not st.any() and replays == 0
                _same(got, D.signal_levels([wav], [0], [0], bin_len, n_bins, DIFF), (n, bin_len))
                assert int(got["n"].sum()) == n - 1
        finally:
            dev.close()


def test_frames_of_one_sample(ctx, x3):
    """nine frames of one sample, a frame of 50 in the middle: every difference but the frame's own 49 is a seam; a damaged
    one-sample frame takes the seam in front of it and the one behind it"""
    p = x3.Params.default()
    op = XC.oparams(p)
    vals = [-32768, 32767, 5, -7, 1000]
    mid = TL._content("bfp", 50, seed=3)
    rc, smid, _ = O.encode(mid, op)
    assert rc == 0
    tail_vals = [300, -300, 32767, -32768]
    stream = np.concatenate([_one_sample_frames(vals, op), smid, _one_sample_frames(tail_vals, op)])
    frames = [np.array([v], dtype=np.int16) for v in vals] + [mid] + [np.array([v], dtype=np.int16) for v in tail_vals]
    for damaged in (None, 2, 0, 9):
        s = stream.copy()
        ok = [0] * 10
        if damaged is not None:
            s[XC.frame_offsets(stream)[damaged] + 20] ^= 0x40
            ok[damaged] = CRC
        dev = TW.Dev(ctx, x3, stream=s, p=p)
        try:
            assert dev.F == 10 and dev.total == 59
            for bin_len in (0, 1, 4):
                n_bins = R.n_bins_for(59, bin_len)
                got, st, _, replays = _levels(dev, bin_len, n_bins, DIFF, d_seg=None)
                assert st.tolist() == ok and replays == 0
                _same(got, D.signal_levels(frames, ok, dev.so[:-1], bin_len, n_bins, DIFF), (damaged, bin_len))
            if damaged is None:
                one, _, _, _ = _levels(dev, 1, 59, DIFF, d_seg=None)
                assert one["sum"][:5].tolist() == [0, 32767, -32762, -12, 1007]      # (the first: clamped from 65 535)
        finally:
            dev.close()


def test_more_seams_than_a_wave_into_one_record(ctx, x3):
    """301 frames of 40 samples (the last of 17): with bin_len 0 every seam is the same record's, joined wave by wave"""
    bl, bpf, spf = 20, 2, 40
    p, op = x3.Params.make(bl, bpf, (0, 1, 3)), O.Params.make(bl, bpf, (0, 1, 3))
    n = 300 * spf + 17
    wav = TL._content("bfp", n, seed=9)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    try:
        assert dev.F == 301
        frames = _frames_of(dev, wav)
        for damaged in ((), (64, 65, 200)):
            s = stream.copy()
            ok = [0] * dev.F
            for f in damaged:
                s[XC.frame_offsets(stream)[f] + 21] ^= 0x01
                ok[f] = CRC
            ctx.upload(dev.d_x3, s)
            for bin_len in (0, 7, spf, 1_000):
                n_bins = R.n_bins_for(n, bin_len)
                got, st, _, _ = _levels(dev, bin_len, n_bins, DIFF, d_seg=None)
                assert st.tolist() == ok
                _same(got, D.signal_levels(frames, ok, dev.so[:-1], bin_len, n_bins, DIFF), (damaged, bin_len))
                if not damaged:
                    assert int(got["n"].sum()) == n - 1
    finally:
        dev.close()


# ---- 3. clamp
def test_full_scale_alternation_clamps_both_ways(ctx, x3):
    n = 20_000 + 57
    wav = np.tile(np.array([-32768, 32767], dtype=np.int16), n // 2 + 1)[:n]
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        frames, ok = _frames_of(dev, wav), [0] * dev.F
        one, _, _, _ = _levels(dev, 0, 1, DIFF)
        up, down = n // 2, (n - 1) - n // 2                       # differences of +65 535 and of -65 535
        assert (int(one["min"][0]), int(one["max"][0]), int(one["n"][0])) == (-32768, 32767, n - 1)
        assert int(one["sum_sq"][0]) == up * 32767 * 32767 + down * (1 << 30)
        assert int(one["sum"][0]) == up * 32767 - down * 32768
        for bin_len in (0, 1, 641, 10_000):
            n_bins = R.n_bins_for(n, bin_len)
            got, st, _, _ = _levels(dev, bin_len, n_bins, DIFF)
            assert not st.any()
            _same(got, D.signal_levels(frames, ok, dev.so[:-1], bin_len, n_bins, DIFF), bin_len)
    finally:
        dev.close()


# ---- 4. other parameter sets
@pytest.mark.parametrize("bl,bpf,codes", [(10, 1000, (0, 1, 3)), (40, 250, (0, 1, 3)), (20, 500, (1, 1, 3))])
def test_parameter_sets_by_a_walk_built_index(ctx, x3, bl, bpf, codes):
    """as test_gpu_levels.py's: a walk-built index, no index, an index that says "none"; with codes (1, 1, 3) frames fail to
    decode, and take their seams with them"""
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf, codes), O.Params.make(bl, bpf, codes)
    n = 6 * spf + min(TAIL, spf - 1)
    wav = XC.patchwork(bl + bpf, n)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    sb = 4 if spf // bl <= 64 else 32
    try:
        d_idx, ne = _walk_index(ctx, x3, dev, sb)
        none = ctx.download(d_idx, 8 * ne, np.uint64)
        none[0] = 0
        d_none = dev.alloc(8 * ne)
        ctx.upload(d_none, none)
        frames, ost = TL._oracle_frames(stream, XC.frame_offsets(stream), op)
        assert any(ost) == (tuple(codes) == (1, 1, 3))
        for bin_len in (0, 7, 641, 10_001):
            n_bins = R.n_bins_for(n, bin_len)
            want = D.signal_levels(frames, ost, dev.so[:-1], bin_len, n_bins, DIFF)
            for what, seg in (("walk", d_idx), ("no index", None), ("none", d_none)):
                got, st, _, replays = _levels(dev, bin_len, n_bins, DIFF, d_seg=seg, sb=sb)
                assert st.tolist() == ost, (what, st, ost)
                _same(got, want, (what, bin_len))
                if not any(ost):
                    assert replays == 0, (what, bin_len, replays)
    finally:
        dev.close()


# ---- 5. rollback and damage
@pytest.mark.parametrize("where", [3, 0, 6])
def test_a_crc_damaged_frame_loses_its_samples_and_both_seams(ctx, x3, where):
    n = 60_000 + TAIL
    wav = TL._content("patchwork", n, seed=13)
    dev, stream = TL._encoded(ctx, x3, wav)
    try:
        s = stream.copy()
        s[XC.frame_offsets(stream)[where] + 20 + 777] ^= 0x10
        ctx.upload(dev.d_x3, s)
        ok = [CRC if f == where else 0 for f in range(7)]
        frames = _frames_of(dev, wav)
        for bin_len in (0, 1, 641, 10_000, 10_001):
            n_bins = R.n_bins_for(n, bin_len)
            for seg in ("own", None):
                got, st, res, replays = _levels(dev, bin_len, n_bins, DIFF, d_seg=seg)
                assert st.tolist() == ok and res == (0, 1, where, CRC) and replays == 0
                _same(got, D.signal_levels(frames, ok, dev.so[:-1], bin_len, n_bins, DIFF), (where, bin_len))
                lost = int(dev.so[where + 1] - dev.so[where]) + (1 if where < 6 else 0)   # its positions and the seam behind
                assert int(got["n"].sum()) == n - (1 if where else 0) - lost
                if bin_len == 1 and where == 3:
                    assert got["n"][29_999:30_001].tolist() == [1, 0] and got["n"][39_999:40_002].tolist() == [0, 0, 1]
    finally:
        dev.close()


@pytest.mark.parametrize("bin_len", [641, 10_000, 0])
def test_a_late_decode_error_takes_the_whole_frame_and_both_seams_back(ctx, x3, bin_len):
    """test_gpu_levels.py's late BFP block with E = 1 in frame 3: stretches in front of it have added differences to the
    frame's rows already"""
    n = 60_000 + TAIL
    wav = TL._content("patchwork", n, seed=12)
    dev, stream = TL._encoded(ctx, x3, wav)
    try:
        idx, ne = TL._index_words(ctx, x3, dev)
        pitch = (ne - 1) // dev.F
        entry = int(idx[1 + 3 * pitch + 12])
        assert (entry >> 48) & 1
        offs = XC.frame_offsets(stream)
        bit = (offs[3] + 20) * 8 + (entry & 0xFFFFFFFF)
        s = stream.copy()
        for k in range(bit, bit + 6):
            s[k >> 3] &= ~(0x80 >> (k & 7)) & 0xFF
        XC.refresh_crcs(s, offs[3])
        ctx.upload(dev.d_x3, s)
        frames, ost = TL._oracle_frames(s, offs, XC.oparams(dev.p))
        assert ost == [0, 0, 0, BPF, 0, 0, 0]
        n_bins = R.n_bins_for(n, bin_len)
        got, st, res, replays = _levels(dev, bin_len, n_bins, DIFF)
        assert st.tolist() == ost and res == (0, 1, 3, BPF) and replays == 1
        _same(got, D.signal_levels(frames, ost, dev.so[:-1], bin_len, n_bins, DIFF), bin_len)
        assert int(got["n"].sum()) == n - 1 - 10_001
    finally:
        dev.close()


# ---- 6. unproven seeds
@pytest.mark.parametrize("how", ["sample", "bit offset"])
@pytest.mark.parametrize("bin_len", [1, 641, 10_001])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, bin_len, how):
    """entry 12 of frame 2 has a wrong sample (the seed of the stretch that starts there) or a wrong bit offset: the stretch
    that ends there contradicts it, the frame goes through the reader, and the records are those of the intact index"""
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
        n_bins = R.n_bins_for(n, bin_len)
        good, st0, _, rep0 = _levels(dev, bin_len, n_bins, DIFF)
        got, st, _, replays = _levels(dev, bin_len, n_bins, DIFF, d_seg=d_bad)
        assert rep0 == 0 and replays == 1 and not st.any() and not st0.any()
        assert got.tobytes() == good.tobytes()
        _same(got, D.signal_levels(_frames_of(dev, wav), [0] * 7, dev.so[:-1], bin_len, n_bins, DIFF), how)
    finally:
        dev.close()


# ---- 7. corpus
@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("bin_len", [0, 1, 1_000])
def test_corpus_rows_are_each_entrys_own_levels(ctx, x3, bin_len, walk):
    """entries of 1, 2 and 3 frames (the middle frame of the last damaged), one of 0 bytes, one of one sample, one repeated:
    every entry's rows are the stream call's on that entry alone, and no difference crosses from one entry into the next"""
    p = x3.Params.default()
    op = XC.oparams(p)
    clips = [TL._content("patchwork", k * 10_000 - 1_234 * (k - 1), seed=20 + k) for k in (1, 2, 3)]
    clips.append(np.array([-4321], dtype=np.int16))
    entries = []
    for w in clips:
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        entries.append(s)
    damaged = entries[2].copy()
    damaged[XC.frame_offsets(damaged)[1] + 20 + 99] ^= 0x01
    ents = [entries[0], entries[1], damaged, np.zeros(0, dtype=np.uint8), entries[3], entries[1], entries[0]]
    buf, offs, lens = TL._place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=32, index="walk" if walk else "decode")
    try:
        assert corpus.entries["n_frames"].tolist() == [1, 2, 3, 0, 1, 2, 1]
        rows, rf, st = corpus.levels(bin_len, signal="diff")
        assert np.array_equal(rf, R.corpus_row_first(corpus.entries["n_samples"], bin_len)) and rows.size == int(rf[-1])
        assert st.tolist() == [0, 0, 0, 0, CRC, 0, 0, 0, 0, 0]
        assert ctx.get_option("last_levels_replays") == 0
        ref_entries = []
        for e, s in enumerate(ents):
            a, b = int(rf[e]), int(rf[e + 1])
            nf = int(corpus.entries["n_frames"][e])
            if nf == 0:
                assert np.array_equal(rows[a:b], R.empty(1)), e
                ref_entries.append(([], [], [], 0))
                continue
            ws = x3.WindowSource(ctx, s, p, seg_blocks=32, index="walk")
            try:
                alone, st_alone = ws.levels(bin_len, b - a, signal="diff")
            finally:
                ws.close()
            _same(rows[a:b], alone, ("alone", e))
            first = int(corpus.entries["first_frame"][e])
            assert np.array_equal(st_alone, st[first:first + nf])
            fo = XC.frame_offsets(s)
            frames, ost = TL._oracle_frames(s, fo, op)
            fst = [CRC if (e == 2 and f == 1) else ost[f] for f in range(nf)]
            lens_f = [int(s[o + 4]) << 8 | int(s[o + 5]) for o in fo]
            ref_entries.append((frames, fst, np.concatenate([[0], np.cumsum(lens_f)])[:-1], sum(lens_f)))
        want, rf3 = D.corpus_signal_levels(ref_entries, bin_len, DIFF)
        assert np.array_equal(rf3, rf)
        _same(rows, want, "diff_levels_ref")
        for e in (0, 1, 5, 6):                                          # clean entries: N - 1 differences each
            assert int(rows["n"][int(rf[e]):int(rf[e + 1])].sum()) == int(corpus.entries["n_samples"][e]) - 1, e
        assert np.array_equal(rows[int(rf[4]):int(rf[5])], R.empty(1))   # one sample: no difference
        if bin_len == 1:
            assert all(int(rows["n"][int(rf[e])]) == 0 for e in range(7))
        # SAMPLES: byte for byte x3_corpus_levels_dev's records, canaries intact; a wrong row count is refused
        n_rows = int(rf[-1])
        d_a, d_b = ctx.alloc(32 * n_rows + 64), ctx.alloc(32 * n_rows + 64)
        try:
            for d in (d_a, d_b):
                ctx.upload(d, np.full(32 * n_rows + 64, CANARY, dtype=np.uint8))
            assert ctx.corpus_signal_levels_dev(corpus, bin_len, d_a, n_rows, None, SAMPLES) == 0
            assert ctx.levels_result() == (0, 1, 4, CRC)
            assert ctx.corpus_levels_dev(corpus, bin_len, d_b, n_rows) == 0
            assert ctx.levels_result() == (0, 1, 4, CRC)
            a, b = ctx.download(d_a, 32 * n_rows + 64, np.uint8), ctx.download(d_b, 32 * n_rows + 64, np.uint8)
            assert a.tobytes() == b.tobytes() and (a[32 * n_rows:] == CANARY).all()
            for bad_rows in (n_rows - 1, n_rows + 1):
                if bad_rows:
                    assert ctx.corpus_signal_levels_dev(corpus, bin_len, d_a, bad_rows, None, DIFF) == BAD
            assert ctx.corpus_signal_levels_dev(corpus, bin_len, d_a, n_rows, None, 2) == BAD
            assert ctx.levels_result()[0] == BAD
        finally:
            ctx.free(d_a)
            ctx.free(d_b)
    finally:
        corpus.close()


# ---- 8. arguments and state
def test_arguments_and_pending_states(ctx, x3):
    L = x3.lib()
    n = 20_000 + TAIL
    wav = TL._content("patchwork", n, seed=14)
    dev, stream = TL._encoded(ctx, x3, wav)
    d_lv, d_st, d_back = dev.alloc(32 * 8), dev.alloc(4 * dev.F), dev.alloc(2 * n)
    try:
        def call(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=32, bl=4_000, lv=d_lv,
                 nb=8, st=d_st, sig=DIFF):
            return L.x3_signal_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, bl, lv, nb, st, sig)
        poison = np.full(32 * 8, CANARY, dtype=np.uint8)
        ctx.upload(d_lv, poison)
        for bad in (dict(sig=2), dict(sig=-1), dict(sig=1 << 16), dict(nb=0), dict(nb=1 << 31), dict(nf=0), dict(c=None),
                    dict(x=None), dict(fo=None), dict(so=None), dict(lv=None), dict(x=dev.d_x3 + 2), dict(fo=dev.d_off + 4),
                    dict(so=dev.d_so + 4), dict(lv=d_lv + 4), dict(st=d_st + 2), dict(idx=dev.d_seg + 4), dict(sb=0), dict(sb=30),
                    dict(params=x3.Params.make(codes=(0, 1, 4)))):
            for sig in (SAMPLES, DIFF):
                assert call(**dict(dict(sig=sig), **bad)) == BAD, bad
        assert ctx.levels_result()[0] == BAD                                   # nothing is pending
        ctx.sync()
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)    # ... and nothing was enqueued
        ctx.graph_begin()                                                       # a context that records a graph
        try:
            assert call() == BAD and call(sig=SAMPLES) == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass                                                           # (a recording of nothing)
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)
        # no status array: fine; x3_levels_result serves the call
        assert call(st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        want = D.signal_levels(_frames_of(dev, wav), [0] * dev.F, dev.so[:-1], 4_000, 8, DIFF)
        _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), want, "no status array")
        # a pending x3_decode_dev reports through x3_decode_result afterwards
        assert ctx.decode_dev(dev.d_x3, dev.len, dev.d_off, dev.F, dev.p, d_back, n, n_per_clip=n) == 0
        assert call() == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        rc, first_bad, _, before = ctx.decode_result()
        assert (rc, first_bad, before) == (0, dev.F, n) and np.array_equal(ctx.download(d_back, 2 * n, np.int16), wav)
        # a call between x3_decode_windows_dev and its result leaves that result intact
        starts = np.array([0, 5, n - 100, n], dtype=np.uint64)
        d_s, d_out, d_ws = dev.alloc(32), dev.alloc(2 * 4 * 100), dev.alloc(16)
        ctx.upload(d_s, starts)
        assert ctx.decode_windows_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_s, 4, 100, d_out, 0, d_ws,
                                      dev.d_seg, 32) == 0
        assert call() == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        assert ctx.decode_windows_result() == (0, 1, 3, BAD)
        _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), want, "between windows")
        # the corpus call: NULL handles, a recording context
        assert L.x3_corpus_signal_levels_dev(ctx._h, None, 0, d_lv, 1, None, DIFF) == BAD
        assert L.x3_corpus_signal_levels_dev(None, None, 0, d_lv, 1, None, DIFF) == BAD
        corpus = x3.Corpus(ctx, (dev.d_x3, dev.len), [0], [dev.len], params=dev.p, seg_blocks=32, index="walk")
        try:
            n_rows = int(corpus.levels_rows(4_000)[-1])
            assert n_rows == 6
            ctx.upload(d_lv, poison)
            ctx.graph_begin()
            try:
                assert ctx.corpus_signal_levels_dev(corpus, 4_000, d_lv, n_rows, None, DIFF) == BAD
            finally:
                try:
                    ctx.graph_destroy(ctx.graph_end())
                except x3.X3Error:
                    pass
            assert ctx.levels_result()[0] == BAD
            assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)
            assert ctx.corpus_signal_levels_dev(corpus, 4_000, d_lv, n_rows, None, DIFF) == 0
            assert ctx.levels_result() == (0, 0, dev.F, 0)
            _same(ctx.download(d_lv, 32 * n_rows, R.LEVEL_DTYPE), want[:n_rows], "corpus, one entry")
        finally:
            corpus.close()
    finally:
        dev.close()


# ---- 9. what it is for
def _burst():
    i = np.arange(8_000)
    w = np.round(12_000 * np.sin(2 * np.pi * i / 2_000)).astype(np.int64)
    w[4_300:4_400] += 600 * (-1) ** i[4_300:4_400]
    return w.astype(np.int16)


def test_a_quiet_high_band_burst_under_a_loud_low_tone(ctx, x3):
    """a tone of amplitude 12 000 and period 2 000 with +-600 alternating on [4 300, 4 400), bins of 100, mean_sq_min 100 000:
    on the samples every bin is hot -- one event over everything; on the difference exactly bin 43 is"""
    import torch
    w = _burst()
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [w[a:a + 2_000] for a in range(0, 8_000, 2_000)], range(0, 8_000, 2_000)
    lv_s = D.signal_levels(frames, [0] * 4, so, 100, 80, SAMPLES)
    lv_d = D.signal_levels(frames, [0] * 4, so, 100, 80, DIFF)
    ms = (lv_d["sum_sq"] // np.maximum(lv_d["n"], 1)).astype(np.int64)
    assert ms[42:45].tolist() == [715, 1_429_311, 3_791] and int(np.delete(ms, 43).max()) == 3_791
    rule, rrule = x3.EventRule.make(mean_sq_min=100_000), E.Rule(mean_sq_min=100_000)
    assert E.stream_events(lv_s, 8_000, 100, rrule)[0] == [(0, 8_000)]
    assert E.stream_events(lv_d, 8_000, 100, rrule)[0] == [(4_300, 100)]
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        for signal, lv in (("samples", lv_s), ("diff", lv_d)):
            got, st = ws.levels(100, signal=signal)
            assert not st.any()
            _same(got, lv, signal)
            ev, elv = E.stream_events(lv, 8_000, 100, rrule)
            _, wst, wln, wlv = E.slots(ev, elv, 4, False)
            starts, lens, cnt, el = ws.events(100, rule, 4, signal=signal)
            assert int(cnt) == 1
            assert np.array_equal(starts.cpu().numpy().view(np.uint64), wst) and np.array_equal(lens.cpu().numpy().view(np.uint32), wln)
            assert np.array_equal(x3.event_levels_view(el), wlv)
        # a median-based rule: hot = mean square at least 50 times the median bin's
        trule = Q.TRule(mean_sq=(500_000, 50, 1, 0))
        thr_d = Q.stream_thresholds(lv_d, 8_000, 100, trule)
        starts, lens, cnt, el, thr = ws.adaptive_events(100, x3.ThresholdRule.make(mean_sq=trule.mean_sq), x3.EventRule.make(), 4,
                                                        signal="diff")
        assert [tuple(int(x) for x in t) for t in thr.cpu().numpy().reshape(-1).view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == thr_d
        ev, elv = Q.stream_adaptive_events(lv_d, 8_000, 100, thr_d[0], E.Rule())
        assert ev == [(4_300, 100)] and int(cnt) == 1
        assert int(starts[0]) == 4_300 and int(lens[0]) == 100 and np.array_equal(x3.event_levels_view(el)[:1], elv)
        ev_s = Q.stream_adaptive_events(lv_s, 8_000, 100, Q.stream_thresholds(lv_s, 8_000, 100, trule)[0], E.Rule())[0]
        _, _, cnt_s, _, _ = ws.adaptive_events(100, x3.ThresholdRule.make(mean_sq=trule.mean_sq), x3.EventRule.make(), 4)
        assert int(cnt_s) == len(ev_s) == 0                            # (no bin of the tone is 50 times its median)
        v, k = ws.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [500_000, 1_000_000], signal="diff")
        wv, wk = Q.stream_quantiles(lv_d, 8_000, 100, Q.MEAN_SQ, [500_000, 1_000_000])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv) and np.array_equal(k.cpu().numpy().view(np.uint32), wk)
        assert int(wv[0][1]) == 1_429_311
        # ... and the event, fed to ranges, is the burst
        out, offsets, status = ws.ranges(starts, lens, padded_to=100)
        assert not status.cpu().numpy().any() and np.array_equal(out[0].cpu().numpy(), w[4_300:4_400])
        assert isinstance(out, torch.Tensor)
    finally:
        ws.close()
    # the corpus form: the clip twice and a silent one between; one event per loud entry, none crosses an entry's end
    rc, quiet, _ = O.encode(np.zeros(700, dtype=np.int16), op)
    assert rc == 0
    buf, offs, lens = TL._place_even([stream, quiet, stream])
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=8, index="walk")
    try:
        rows, rf, st = corpus.levels(100, signal="diff")
        assert rf.tolist() == [0, 80, 87, 167] and not st.any()
        _same(rows[:80], lv_d, "entry 0")
        _same(rows[87:], lv_d, "entry 2")
        assert not rows["sum_sq"][80:87].any() and int(rows["n"][80:87].sum()) == 699
        ent, starts, lens, cnt, el = corpus.events(100, rule, 4, signal="diff")
        assert int(cnt) == 2 and ent[:2].tolist() == [0, 2] and starts[:2].tolist() == [4_300, 4_300] and lens[:2].tolist() == [100, 100]
        ent, starts, lens, cnt, el, thr = corpus.adaptive_events(100, x3.ThresholdRule.make(mean_sq=trule.mean_sq),
                                                                 x3.EventRule.make(), 4, signal="diff")
        assert int(cnt) == 2 and ent[:2].tolist() == [0, 2] and starts[:2].tolist() == [4_300, 4_300]
        v, k = corpus.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [1_000_000], signal="diff")
        assert v.cpu().numpy().reshape(-1).tolist() == [1_429_311, 0, 1_429_311]
        out, offsets, status = corpus.ranges(ent, starts, lens, padded_to=100)
        assert np.array_equal(out[1].cpu().numpy(), w[4_300:4_400])
    finally:
        corpus.close()


# ---- 10. mirrors
def test_python_mirror_round_trip(ctx, x3):
    n = 30_000 + TAIL
    wav = TL._content("patchwork", n, seed=15)
    rc, stream, _ = O.encode(wav)
    assert rc == 0
    frames, so = [wav[i:i + 10_000] for i in range(0, n, 10_000)], [0, 10_000, 20_000, 30_000]
    ws = x3.WindowSource(ctx, stream, seg_blocks=32, index="walk")
    try:
        lv, st = ws.levels(1_000, signal="diff")
        assert lv.dtype == x3.LEVEL_DTYPE and lv.size == 34 and st.tolist() == [0, 0, 0, 0]
        _same(lv, D.signal_levels(frames, st, so, 1_000, 34, DIFF), "WindowSource.levels")
        one, _ = ws.levels(0, signal=x3.LEVEL_SIGNAL_DIFF)
        d = np.clip(np.diff(wav.astype(np.int64)), -32768, 32767)
        assert one.size == 1 and int(one["n"][0]) == n - 1 and int(one["sum"][0]) == int(d.sum())
        assert int(one["min"][0]) == int(d.min()) and int(one["max"][0]) == int(d.max()) and int(one["sum_sq"][0]) == int((d * d).sum())
        two, _ = ws.levels(1_000, n_bins=2, signal="diff")
        _same(two, lv[:2], "n_bins")
        same, _ = ws.levels(1_000, signal="samples")
        old, _ = ws.levels(1_000)
        assert same.tobytes() == old.tobytes()
        _same(old, R.levels(frames, st, so, 1_000, 34), "the default")
        with pytest.raises(ValueError):
            ws.levels(1_000, signal="second")
    finally:
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], index="walk")
    try:
        rows, rf, st = corpus.levels(1_000, signal="diff")
        assert rf.tolist() == [0, 34, 68] and not st.any()
        _same(rows[:34], lv, "Corpus.levels")
        _same(rows[34:], lv, "Corpus.levels")
        assert corpus.levels(1_000)[0].tobytes() == old.tobytes() * 2
    finally:
        corpus.close()


def test_x3_hpp_signal_levels(tmp_path):
    """tests/host_cpp/test_signal_levels_hpp.cpp: device::levels and device::Corpus::levels of the C++ mirror with a signal"""
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_signal_levels_hpp.cpp")
    exe = str(tmp_path / "test_signal_levels_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
