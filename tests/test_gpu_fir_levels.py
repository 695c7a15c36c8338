"""FIR levels (include/x3hip.h, "FIR LEVELS"): x3_fir_levels_dev, x3_corpus_fir_levels_dev and their Python mirror.  Every
field of every record is held with == against fir_levels_ref.py fed with the CPU oracle's samples, as test_gpu_levels.py
and test_gpu_signal_levels.py (whose helpers these tests use) hold the levels and signal-levels calls.  Shapes are small:
frames of 20 x 8 .. 20 x 64 samples unless a test needs the encoder's index or a late block of a long frame."""
import ctypes as C

import numpy as np
import pytest

import diff_levels_ref as D
import events_ref as E
import fir_levels_ref as FR
import levels_ref as R
import oracle_lib as O
import quantiles_ref as Q
import test_gpu_levels as TL
import test_gpu_signal_levels as TS
import test_gpu_windows as TW
import x3_cases as XC

pytestmark = pytest.mark.gpu

BAD, CRC, BPF, TAIL, CANARY = TL.BAD, TL.CRC, TL.BPF, TL.TAIL, TL.CANARY
_same = TL._same
MIXED8 = ([-3000, 9000, -200, 7, 5000, -8000, 1, 6560], 7)      # sum |c| = 31 768
DELAY8 = ([0, 0, 0, 0, 0, 0, 0, 1], 0)                           # x[i - 7]: the history rule alone
TAP_SETS = [([1, -2, 1], 0), ([1, 0, -1], 0), ([1, 1, 1, 1], 2), MIXED8, DELAY8]


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _fir(dev, bin_len, n_bins, taps, shift=0, d_seg="own", sb=None):
    """x3_fir_levels_dev into a poisoned buffer with a canary behind it -> (records, frame statuses, result, replays)"""
    ctx = dev.ctx
    nb = 32 * n_bins
    d_lv, d_st = ctx.alloc(nb + 64), ctx.alloc(4 * dev.F + 64)
    try:
        ctx.upload(d_lv, np.full(nb + 64, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * dev.F + 64, CANARY, dtype=np.uint8))
        idx = dev.d_seg if isinstance(d_seg, str) else d_seg
        rc = ctx.fir_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, idx,
                                (sb if sb is not None else dev.sb) if idx else 0, dev.x3.Fir(taps, shift))
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


def _frames_stream(ctx, x3, wav, lens, p):
    """the stream x3_encode_frames_dev makes of wav cut into frames of `lens` samples, back to back"""
    assert sum(lens) == wav.size
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    cap = sum(x3.lib().x3_encode_bound(int(n), C.byref(p)) for n in lens) + 64
    d_wav, d_out = ctx.alloc(2 * wav.size + 64), ctx.alloc(cap + 16)
    try:
        ctx.upload(d_wav, wav)
        assert ctx.encode_frames_dev(d_wav, [int(s) for s in starts], [int(n) for n in lens], p, d_out, cap) == 0
        rc, end, _ = ctx.encode_result()
        assert rc == 0
        stream = ctx.download(d_out, end)
    finally:
        ctx.free(d_wav)
        ctx.free(d_out)
    assert [int(stream[o + 4]) << 8 | int(stream[o + 5]) for o in XC.frame_offsets(stream)] == list(lens)
    return stream


def _indexes(ctx, x3, dev, sb=4):
    """the index choices of a stream without the encoder's: a walk-built one at sb blocks, and none"""
    if x3.lib().x3_seg_index_entries(dev.F, C.byref(dev.p), sb) == 0:
        return [("no index", None)]
    return [("walk %d" % sb, TS._walk_index(ctx, x3, dev, sb)[0]), ("no index", None)]


# ---- 1. the two identities
@pytest.mark.parametrize("kind", ["patchwork", "literal"])
def test_identities_on_a_stream(ctx, x3, kind):
    """{1} is x3_levels_dev and {1, -1} the DIFF call, byte for byte, canaries intact (the helpers look): the encoder's index
    at 32 blocks, a walk-built one at 4, none"""
    n = 30_000 + TAIL
    wav = TL._content(kind, n)
    dev, _ = TL._encoded(ctx, x3, wav)
    try:
        assert dev.F == 4 and dev.sb == 32
        d_idx4, _ = TS._walk_index(ctx, x3, dev, 4)
        for bin_len in (0, 1, 641, 10_000, 10_001):
            n_bins = R.n_bins_for(n, bin_len) + 1
            old, st_o, _, _ = TL._levels(dev, bin_len, n_bins)
            dif, st_d, _, _ = TS._levels(dev, bin_len, n_bins, TS.DIFF)
            for what, seg, sb in (("encoder 32", "own", None), ("walk 4", d_idx4, 4), ("no index", None, None)):
                one, st, _, replays = _fir(dev, bin_len, n_bins, [1], d_seg=seg, sb=sb)
                assert one.tobytes() == old.tobytes() and np.array_equal(st, st_o) and replays == 0, (what, bin_len)
                two, st, _, replays = _fir(dev, bin_len, n_bins, [1, -1], d_seg=seg, sb=sb)
                assert two.tobytes() == dif.tobytes() and np.array_equal(st, st_d) and replays == 0, (what, bin_len)
    finally:
        dev.close()


def _corpus_entries(x3, op, clips, damage=None):
    """entries (streams by the oracle) of the clips; damage: (entry, frame) gets a payload bit flipped"""
    ents = []
    for k, w in enumerate(clips):
        if w.size == 0:
            ents.append(np.zeros(0, dtype=np.uint8))
            continue
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        if damage and damage[0] == k:
            s = s.copy()
            s[XC.frame_offsets(s)[damage[1]] + 20 + 1] ^= 0x01
        ents.append(s)
    return ents


@pytest.mark.parametrize("index,sb", [("decode", 32), ("walk", 4), ("walk", 0)])
def test_identities_on_a_corpus(ctx, x3, index, sb):
    p, op = x3.Params.default(), XC.oparams(x3.Params.default())
    clips = [TL._content("patchwork", 12_345, seed=31), TL._content("bfp", 1, seed=32), np.zeros(0, dtype=np.int16),
             TL._content("rice3", 20_001, seed=33)]
    ents = _corpus_entries(x3, op, clips, damage=(3, 1))
    buf, offs, lens = TL._place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=sb, index=index)
    try:
        assert index != "walk" or bool(corpus.d_seg_index) == (sb != 0)
        for bin_len in (0, 1, 1_000):
            old = corpus.levels(bin_len)
            dif = corpus.levels(bin_len, signal="diff")
            one = corpus.levels(bin_len, signal=x3.Fir([1]))
            two = corpus.levels(bin_len, signal=x3.Fir([1, -1]))
            assert one[2].tolist() == [0, 0, 0, 0, CRC, 0] and np.array_equal(two[2], one[2])
            assert one[0].tobytes() == old[0].tobytes() and two[0].tobytes() == dif[0].tobytes(), bin_len
        n_rows = int(corpus.levels_rows(1_000)[-1])
        d_a, d_b = ctx.alloc(32 * n_rows + 64), ctx.alloc(32 * n_rows + 64)
        try:
            for d in (d_a, d_b):
                ctx.upload(d, np.full(32 * n_rows + 64, CANARY, dtype=np.uint8))
            assert ctx.corpus_fir_levels_dev(corpus, 1_000, d_a, n_rows, None, x3.Fir([1])) == 0
            assert ctx.levels_result() == (0, 1, 4, CRC)
            assert ctx.corpus_levels_dev(corpus, 1_000, d_b, n_rows) == 0
            assert ctx.levels_result() == (0, 1, 4, CRC)
            a, b = ctx.download(d_a, 32 * n_rows + 64, np.uint8), ctx.download(d_b, 32 * n_rows + 64, np.uint8)
            assert a.tobytes() == b.tobytes() and (a[32 * n_rows:] == CANARY).all()
        finally:
            ctx.free(d_a)
            ctx.free(d_b)
    finally:
        corpus.close()


# ---- 2. tap sets over geometry
GEOMETRIES = [(20, 8, (0, 1, 3)), (20, 64, (0, 1, 3)), (10, 32, (0, 1, 3)), (40, 16, (0, 1, 3)), (20, 32, (1, 1, 3))]


@pytest.mark.parametrize("bl,bpf,codes", GEOMETRIES)
@pytest.mark.parametrize("taps,shift", TAP_SETS)
def test_tap_sets_over_geometry(ctx, x3, taps, shift, bl, bpf, codes):
    """nine frames and a short one per content kind; a walk-built index at 4 blocks (at block length 10 a stretch is 40
    samples) and none; with codes (1, 1, 3) frames fail to decode and take the T - 1 positions behind them"""
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
            indexes = _indexes(ctx, x3, dev)
            assert len(indexes) == 2
            for bin_len in (1, 7, spf, spf - 1, spf + 1, 0):
                n_bins = R.n_bins_for(n, bin_len)
                want = FR.fir_levels(frames, ost, dev.so[:-1], bin_len, n_bins, taps, shift)
                for what, seg in indexes:
                    got, st, _, replays = _fir(dev, bin_len, n_bins, taps, shift, d_seg=seg, sb=4)
                    assert st.tolist() == ost, (kind, what, st, ost)
                    _same(got, want, (kind, what, bin_len))
                    if not any(ost):
                        assert replays == 0 and int(got["n"].sum()) == n - len(taps) + 1, (kind, what, bin_len)
        finally:
            dev.close()


# ---- 3. short pieces
SHORT_LENS = [160, 1, 2, 3, 1, 1, 7, 8, 9, 160, 1, 160, 2, 2, 2, 160, 5]


@pytest.mark.parametrize("damaged", [None, 4, 9, 0])
def test_the_walk_back_across_short_frames(ctx, x3, damaged):
    """frames of 1, 2, 3, 1, 1, 7, 8, 9 samples between frames of 160: with eight taps a position's history lies in up to eight
    frames; a damaged one among them ends the walk"""
    p, op = x3.Params.make(20, 8), O.Params.make(20, 8, (0, 1, 3))
    wav = TL._content("literal", sum(SHORT_LENS), seed=41)
    stream = _frames_stream(ctx, x3, wav, SHORT_LENS, p)
    offs = XC.frame_offsets(stream)
    ok = [0] * len(SHORT_LENS)
    if damaged is not None:
        stream = stream.copy()
        stream[offs[damaged] + 20] ^= 0x40
        ok[damaged] = CRC
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    try:
        assert dev.F == len(SHORT_LENS) and dev.total == wav.size
        frames = TS._frames_of(dev, wav)
        for taps, shift in [DELAY8, MIXED8, ([1, -2, 1], 0), ([1, 1, 1, 1], 2)]:
            for bin_len in (1, 0, 7, 160):
                n_bins = R.n_bins_for(wav.size, bin_len)
                want = FR.fir_levels(frames, ok, dev.so[:-1], bin_len, n_bins, taps, shift)
                for what, seg in _indexes(ctx, x3, dev):
                    got, st, _, replays = _fir(dev, bin_len, n_bins, taps, shift, d_seg=seg, sb=4)
                    assert st.tolist() == ok and replays == 0
                    _same(got, want, (damaged, taps, what, bin_len))
        if damaged is None:
            one, _, _, _ = _fir(dev, 1, wav.size, *DELAY8, d_seg=None)
            assert one["n"].tolist() == [0] * 7 + [1] * (wav.size - 7)
            assert np.array_equal(one["sum"][7:], wav[:-7].astype(np.int64))
    finally:
        dev.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 9, 100, 1_380])
def test_streams_round_the_tap_count(ctx, x3, n):
    """one sample; T - 1 samples: every record is the identity; exactly T: one value; 100 and 1 380 samples in frames of
    1 280: a short (last) frame whose later stretches are empty"""
    p, op = x3.Params.make(20, 64), O.Params.make(20, 64, (0, 1, 3))
    wav = TL._content("bfp", n, seed=n)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    dev = TW.Dev(ctx, x3, stream=stream, p=p)
    try:
        frames = TS._frames_of(dev, wav)
        d_idx32, _ = TS._walk_index(ctx, x3, dev, 32)
        d_idx4, _ = TS._walk_index(ctx, x3, dev, 4)
        for taps, shift in TAP_SETS + [([1], 0), ([1, -1], 0)]:
            T = len(taps)
            for bin_len in (0, 1, 5):
                n_bins = R.n_bins_for(n, bin_len) + 1
                want = FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, taps, shift)
                for seg, sb in ((d_idx32, 32), (d_idx4, 4), (None, 0)):
                    got, st, _, replays = _fir(dev, bin_len, n_bins, taps, shift, d_seg=seg, sb=sb)
                    assert not st.any() and replays == 0
                    _same(got, want, (n, taps, sb, bin_len))
                    assert int(got["n"].sum()) == max(0, n - T + 1)
                    if n < T:
                        assert got.tobytes() == R.empty(n_bins).tobytes()
    finally:
        dev.close()


# ---- 4. arithmetic edges
def test_arithmetic_edges(ctx, x3):
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 1_000 + 57

    def dev_of(wav):
        rc, stream, _ = O.encode(wav, op)
        assert rc == 0
        return TW.Dev(ctx, x3, stream=stream, p=p)

    # full-scale alternation with {16384, -16384}: +-(2^30 - 16384) clamps both ways
    wav = np.tile(np.array([-32768, 32767], dtype=np.int16), n // 2 + 1)[:n]
    dev = dev_of(wav)
    try:
        one, st, _, _ = _fir(dev, 0, 1, [16384, -16384], d_seg=None)
        up, down = n // 2, (n - 1) - n // 2
        assert not st.any() and (int(one["min"][0]), int(one["max"][0]), int(one["n"][0])) == (-32768, 32767, n - 1)
        assert int(one["sum_sq"][0]) == up * 32767 * 32767 + down * (1 << 30)
        assert int(one["sum"][0]) == up * 32767 - down * 32768
        frames = TS._frames_of(dev, wav)
        for bin_len in (1, 7, 320):
            n_bins = R.n_bins_for(n, bin_len)
            for what, seg in _indexes(ctx, x3, dev):
                got, _, _, _ = _fir(dev, bin_len, n_bins, [16384, -16384], d_seg=seg, sb=4)
                _same(got, FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], bin_len, n_bins, [16384, -16384]), (what, bin_len))
        # {-32768} >> 15 on -32768: acc = 2^30, y = 32768 clamps to 32767; on the other samples y = -x exactly
        got, _, _, _ = _fir(dev, 1, n, [-32768], 15, d_seg=None)
        assert got["sum"].tolist() == [32767 if v == -32768 else -32767 for v in wav.tolist()]
        assert (got["sum_sq"] == 32767 * 32767).all() and (got["n"] == 1).all()
    finally:
        dev.close()
    # shift 15 on a small negative sum: floor, not truncation
    wav = TL._content("rice3", n, seed=4)
    wav[:6] = [1, -1, 0, 3, -3, 32767]
    dev = dev_of(wav)
    try:
        frames = TS._frames_of(dev, wav)
        for taps in ([-1], [1], [1, -1, 1]):
            got, _, _, _ = _fir(dev, 1, n, taps, 15, d_seg=None)
            _same(got, FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], 1, n, taps, 15), taps)
        got, _, _, _ = _fir(dev, 1, n, [-1], 15, d_seg=None)
        assert got["sum"][:6].tolist() == [-1, 0, 0, -1, 0, -1] and got["sum_sq"][:6].tolist() == [1, 0, 0, 1, 0, 1]
    finally:
        dev.close()


# ---- 5. damage
@pytest.mark.parametrize("where", [0, 4, 9])
def test_a_crc_damaged_frame_takes_the_positions_behind_it(ctx, x3, where):
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
        for taps, shift in TAP_SETS:
            T = len(taps)
            for bin_len in (1, 0, 7, spf, spf + 1):
                n_bins = R.n_bins_for(n, bin_len)
                want = FR.fir_levels(frames, ok, dev.so[:-1], bin_len, n_bins, taps, shift)
                for what, seg in _indexes(ctx, x3, dev):
                    got, st, res, replays = _fir(dev, bin_len, n_bins, taps, shift, d_seg=seg, sb=4)
                    assert st.tolist() == ok and res == (0, 1, where, CRC) and replays == 0
                    _same(got, want, (where, taps, what, bin_len))
                    if bin_len == 1:                    # its own records and the T - 1 behind it: identities; the next is not
                        a, b = where * spf, min((where + 1) * spf, n)
                        assert got[a:min(b + T - 1, n)].tobytes() == R.empty(min(b + T - 1, n) - a).tobytes()
                        if b + T - 1 < n:
                            assert int(got["n"][b + T - 1]) == 1
    finally:
        dev.close()


def _late_error_stream(ctx, x3):
    """test_gpu_levels.py's stream whose frame 3 has a late BFP block with E = 1 (CRCs good): a decode error"""
    n = 60_000 + TAIL
    wav = TL._content("patchwork", n, seed=12)
    dev, stream = TL._encoded(ctx, x3, wav)
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
    return dev, s, offs, n


def test_a_late_decode_error_takes_the_frame_and_the_positions_behind_it(ctx, x3):
    dev, s, offs, n = _late_error_stream(ctx, x3)
    try:
        frames, ost = TL._oracle_frames(s, offs, XC.oparams(dev.p))
        assert ost == [0, 0, 0, BPF, 0, 0, 0]
        for taps, shift in (MIXED8, ([1, 0, -1], 0)):
            for bin_len in (641, 10_000, 0):
                n_bins = R.n_bins_for(n, bin_len)
                got, st, res, replays = _fir(dev, bin_len, n_bins, taps, shift)
                assert st.tolist() == ost and res == (0, 1, 3, BPF) and replays == 1
                _same(got, FR.fir_levels(frames, ost, dev.so[:-1], bin_len, n_bins, taps, shift), (taps, bin_len))
                assert int(got["n"].sum()) == n - 10_000 - 2 * (len(taps) - 1)
    finally:
        dev.close()


@pytest.mark.parametrize("how", ["sample", "bit offset"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """entry 12 of frame 2 has a wrong sample or a wrong bit offset: the frame goes through the reader and is ONE stretch to
    the seam kernel, between frames 1 and 3 that were decoded in stretches -- its edge record is read from both sides"""
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
        for taps, shift in (MIXED8, DELAY8, ([1, -2, 1], 0)):
            for bin_len in (1, 641, 10_001):
                n_bins = R.n_bins_for(n, bin_len)
                good, st0, _, rep0 = _fir(dev, bin_len, n_bins, taps, shift)
                got, st, _, replays = _fir(dev, bin_len, n_bins, taps, shift, d_seg=d_bad)
                assert rep0 == 0 and replays == 1 and not st.any() and not st0.any()
                assert got.tobytes() == good.tobytes()
                _same(got, FR.fir_levels(frames, [0] * 7, dev.so[:-1], bin_len, n_bins, taps, shift), (how, taps, bin_len))
    finally:
        dev.close()


# ---- 6. corpus
@pytest.mark.parametrize("index,sb", [("walk", 4), ("decode", 32)])
def test_corpus_entries_are_each_the_stream_call_alone(ctx, x3, index, sb):
    """entries of one frame, one sample, T - 1 samples, none, several frames with one damaged, and one repeated: every
    entry's rows are the stream call's on that entry alone; no history crosses an entry boundary"""
    p = x3.Params.make(20, 16) if index == "walk" else x3.Params.default()
    op = XC.oparams(p)
    spf = int(p.block_len) * int(p.blocks_per_frame)
    clips = [TL._content("patchwork", spf, seed=51), TL._content("bfp", 1, seed=52), TL._content("literal", 7, seed=53),
             np.zeros(0, dtype=np.int16), TL._content("rice3", 3 * spf + 19, seed=54), TL._content("bfp", 8, seed=55)]
    ents = _corpus_entries(x3, op, clips, damage=(4, 1))
    ents.append(ents[0])
    buf, offs, lens = TL._place_even(ents)
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=sb, index=index)
    try:
        assert corpus.entries["n_frames"].tolist() == [1, 1, 1, 0, 4, 1, 1]
        for taps, shift in (DELAY8, MIXED8, ([1, 0, -1], 0)):
            fir = x3.Fir(taps, shift)
            for bin_len in (0, 1, 100):
                rows, rf, st = corpus.levels(bin_len, signal=fir)
                assert np.array_equal(rf, R.corpus_row_first(corpus.entries["n_samples"], bin_len)) and rows.size == int(rf[-1])
                assert st.tolist() == [0, 0, 0, 0, CRC, 0, 0, 0, 0] and ctx.get_option("last_levels_replays") == 0
                ref_entries = []
                for e, s in enumerate(ents):
                    a, b = int(rf[e]), int(rf[e + 1])
                    if s.size == 0:
                        assert rows[a:b].tobytes() == R.empty(1).tobytes()
                        ref_entries.append(([], [], [], 0))
                        continue
                    ws = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
                    try:
                        alone, _ = ws.levels(bin_len, b - a, signal=fir)
                    finally:
                        ws.close()
                    _same(rows[a:b], alone, ("alone", e, taps, bin_len))
                    fo = XC.frame_offsets(s)
                    frames, ost = TL._oracle_frames(s, fo, op)
                    fst = [CRC if (e == 4 and f == 1) else ost[f] for f in range(len(fo))]
                    lens_f = [int(s[o + 4]) << 8 | int(s[o + 5]) for o in fo]
                    ref_entries.append((frames, fst, np.concatenate([[0], np.cumsum(lens_f)])[:-1], sum(lens_f)))
                want, rf3 = FR.corpus_fir_levels(ref_entries, bin_len, taps, shift)
                assert np.array_equal(rf3, rf)
                _same(rows, want, (taps, bin_len))
                T = len(taps)
                for e in (0, 1, 2, 5, 6):                                # clean entries: max(0, N - T + 1) values each
                    N = int(corpus.entries["n_samples"][e])
                    assert int(rows["n"][int(rf[e]):int(rf[e + 1])].sum()) == max(0, N - T + 1), e
                if bin_len == 1:                                         # the first T - 1 records of every entry: identities
                    for e in range(7):
                        k = min(T - 1, int(rf[e + 1] - rf[e]))
                        assert rows[int(rf[e]):int(rf[e]) + k].tobytes() == R.empty(k).tobytes(), e
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
    d_lv, d_old, d_st = dev.alloc(32 * 8), dev.alloc(32 * 8), dev.alloc(4 * dev.F)
    frames = TS._frames_of(dev, wav)
    corpus = None
    try:
        def fir_of(taps, shift=0, n_taps=None):
            return x3.LevelFir(len(taps) if n_taps is None else n_taps, shift, (C.c_int16 * 8)(*taps))

        def call(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=d_idx, sb=4, bl=250, lv=d_lv, nb=8,
                 st=d_st, fir=fir_of([1, -2, 1])):
            return L.x3_fir_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, bl, lv, nb, st,
                                       C.byref(fir) if fir is not None else None)
        corpus = x3.Corpus(ctx, (dev.d_x3, dev.len), [0], [dev.len], params=dev.p, seg_blocks=4, index="walk")
        n_rows = int(corpus.levels_rows(250)[-1])
        assert n_rows == 7

        def ccall(c=ctx._h, k=corpus._h, bl=250, lv=d_lv, nr=n_rows, st=d_st, fir=fir_of([1, -2, 1])):
            return L.x3_corpus_fir_levels_dev(c, k, bl, lv, nr, st, C.byref(fir) if fir is not None else None)
        poison = np.full(32 * 8, CANARY, dtype=np.uint8)
        ctx.upload(d_lv, poison)
        # a levels call is pending: every refusal leaves its result intact
        assert ctx.levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, 250, d_old, 8, None, d_idx, 4) == 0
        refused = [dict(fir=fir_of([], n_taps=0)), dict(fir=fir_of([1] * 8, n_taps=9)), dict(fir=fir_of([1], 16)),
                   dict(fir=fir_of([16384, -16384, 1])), dict(fir=fir_of([-32768, 1])), dict(fir=None),
                   dict(nb=0), dict(nb=1 << 31), dict(nf=0), dict(c=None), dict(x=None), dict(fo=None),
                   dict(so=None), dict(lv=None), dict(lv=d_lv + 4), dict(st=d_st + 2), dict(idx=d_idx + 4), dict(sb=30),
                   dict(params=x3.Params.make(codes=(0, 1, 4)))]
        for bad in refused:
            assert call(**bad) == BAD, bad
        # ... and so with the corpus call on a valid corpus
        for bad in refused[:6] + [dict(k=None), dict(c=None), dict(nr=0), dict(nr=n_rows - 1), dict(nr=n_rows + 1), dict(lv=None),
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
        _same(ctx.download(d_old, 32 * 8, R.LEVEL_DTYPE), R.levels(frames, [0] * dev.F, dev.so[:-1], 250, 8), "pending")
        assert ctx.levels_result()[0] == BAD                                   # nothing else is pending
        ctx.sync()
        assert np.array_equal(ctx.download(d_lv, 32 * 8, np.uint8), poison)    # ... and nothing was enqueued
        # taps behind n_taps are ignored; sum |c| = 32768 and eight taps at shift 15 are fine
        assert call(fir=fir_of([1, -2, 1, 30_000, 30_000], n_taps=3), st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        want = FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, [1, -2, 1])
        _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), want, "taps behind n_taps")
        for taps, shift in (([16384, -16384], 0), ([4096] * 8, 15), ([-32768], 0)):
            assert call(fir=fir_of(taps, shift)) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
            _same(ctx.download(d_lv, 32 * 8, R.LEVEL_DTYPE), FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, taps, shift), taps)
        assert ccall(st=None) == 0 and ctx.levels_result() == (0, 0, dev.F, 0)
        _same(ctx.download(d_lv, 32 * n_rows, R.LEVEL_DTYPE), want[:n_rows], "corpus, one entry")
        # a FIR call, a DIFF call and a SAMPLES call on one context: each is right
        for _ in range(2):
            got, _, _, _ = _fir(dev, 250, 8, *MIXED8, d_seg=d_idx, sb=4)
            _same(got, FR.fir_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, *MIXED8), "fir")
            dif, _, _, _ = TS._levels(dev, 250, 8, TS.DIFF, d_seg=d_idx, sb=4)
            _same(dif, D.signal_levels(frames, [0] * dev.F, dev.so[:-1], 250, 8, D.DIFF), "diff")
            old, _, _, _ = TL._levels(dev, 250, 8, d_seg=d_idx, sb=4)
            _same(old, R.levels(frames, [0] * dev.F, dev.so[:-1], 250, 8), "samples")
    finally:
        if corpus is not None:
            corpus.close()
        dev.close()


# ---- 8. through the chain
def _burst():
    i = np.arange(8_000)
    w = np.round(12_000 * np.sin(2 * np.pi * i / 2_000)).astype(np.int64)
    w[4_300:4_400] += np.round(600 * np.cos(np.pi * i[4_300:4_400] / 2)).astype(np.int64)
    return w.astype(np.int16)


def test_a_quarter_rate_burst_under_a_loud_low_tone(ctx, x3):
    """a tone of amplitude 12 000 and period 2 000 with a burst of amplitude 600 at fs/4 on [4 300, 4 400), bins of 100,
    mean_sq_min 100 000: on the samples every bin is hot -- one event over everything; behind {1, 0, -1} exactly bin 43 is
    (mean square 710 060 against 5 508 at most elsewhere).  The numbers are fir_levels_ref.py's, on the CPU."""
    import torch
    w = _burst()
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [w[a:a + 2_000] for a in range(0, 8_000, 2_000)], range(0, 8_000, 2_000)
    band = x3.Fir([1, 0, -1])
    lv_s = FR.fir_levels(frames, [0] * 4, so, 100, 80, [1])
    lv_f = FR.fir_levels(frames, [0] * 4, so, 100, 80, [1, 0, -1])
    ms = (lv_f["sum_sq"] // np.maximum(lv_f["n"], 1)).astype(np.int64)
    assert ms[42:45].tolist() == [2_869, 710_060, 4_079] and int(np.delete(ms, 43).max()) == 5_508
    rule, rrule = x3.EventRule.make(mean_sq_min=100_000), E.Rule(mean_sq_min=100_000)
    assert E.stream_events(lv_s, 8_000, 100, rrule)[0] == [(0, 8_000)]
    assert E.stream_events(lv_f, 8_000, 100, rrule)[0] == [(4_300, 100)]
    trule = Q.TRule(mean_sq=(500_000, 50, 1, 0))                       # hot: mean square at least 50 times the median bin's
    thr_f = Q.stream_thresholds(lv_f, 8_000, 100, trule)
    assert thr_f == [(143_450, 0, 80)]
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        for signal, lv in (("samples", lv_s), (band, lv_f)):
            got, st = ws.levels(100, signal=signal)
            assert not st.any()
            _same(got, lv, signal)
            ev, elv = E.stream_events(lv, 8_000, 100, rrule)
            _, wst, wln, wlv = E.slots(ev, elv, 4, False)
            starts, lens, cnt, el = ws.events(100, rule, 4, signal=signal)
            assert int(cnt) == 1
            assert np.array_equal(starts.cpu().numpy().view(np.uint64), wst) and np.array_equal(lens.cpu().numpy().view(np.uint32), wln)
            assert np.array_equal(x3.event_levels_view(el), wlv)
        starts, lens, cnt, el, thr = ws.adaptive_events(100, x3.ThresholdRule.make(mean_sq=trule.mean_sq), x3.EventRule.make(), 4,
                                                        signal=band)
        assert [tuple(int(x) for x in t) for t in thr.cpu().numpy().reshape(-1).view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == thr_f
        ev, elv = Q.stream_adaptive_events(lv_f, 8_000, 100, thr_f[0], E.Rule())
        assert ev == [(4_300, 100)] and int(cnt) == 1
        assert int(starts[0]) == 4_300 and int(lens[0]) == 100 and np.array_equal(x3.event_levels_view(el)[:1], elv)
        v, k = ws.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [500_000, 1_000_000], signal=band)
        wv, wk = Q.stream_quantiles(lv_f, 8_000, 100, Q.MEAN_SQ, [500_000, 1_000_000])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv) and np.array_equal(k.cpu().numpy().view(np.uint32), wk)
        assert wv.tolist() == [[2_869, 710_060]]
        out, offsets, status = ws.ranges(starts, lens, padded_to=100)      # ... and the event, fed to ranges, is the burst
        assert not status.cpu().numpy().any() and np.array_equal(out[0].cpu().numpy(), w[4_300:4_400])
        assert isinstance(out, torch.Tensor)
        with pytest.raises(ValueError, match="not built yet"):
            ws.range_levels(starts, lens, 100, signal=band)
    finally:
        ws.close()
    # the corpus form: the clip twice and a silent one between; one event per loud entry, none crosses an entry's end
    rc, quiet, _ = O.encode(np.zeros(700, dtype=np.int16), op)
    assert rc == 0
    buf, offs, lens = TL._place_even([stream, quiet, stream])
    corpus = x3.Corpus(ctx, buf, offs, lens, params=p, seg_blocks=8, index="walk")
    try:
        rows, rf, st = corpus.levels(100, signal=band)
        assert rf.tolist() == [0, 80, 87, 167] and not st.any()
        _same(rows[:80], lv_f, "entry 0")
        _same(rows[87:], lv_f, "entry 2")
        assert not rows["sum_sq"][80:87].any() and int(rows["n"][80:87].sum()) == 698
        ent, starts, lens, cnt, el = corpus.events(100, rule, 4, signal=band)
        assert int(cnt) == 2 and ent[:2].tolist() == [0, 2] and starts[:2].tolist() == [4_300, 4_300] and lens[:2].tolist() == [100, 100]
        ent, starts, lens, cnt, el, thr = corpus.adaptive_events(100, x3.ThresholdRule.make(mean_sq=trule.mean_sq),
                                                                 x3.EventRule.make(), 4, signal=band)
        assert int(cnt) == 2 and ent[:2].tolist() == [0, 2] and starts[:2].tolist() == [4_300, 4_300]
        v, k = corpus.level_quantiles(100, x3.LEVEL_KEY_MEAN_SQ, [1_000_000], signal=band)
        assert v.cpu().numpy().reshape(-1).tolist() == [710_060, 0, 710_060]
        out, offsets, status = corpus.ranges(ent, starts, lens, padded_to=100)
        assert np.array_equal(out[1].cpu().numpy(), w[4_300:4_400])
        with pytest.raises(ValueError, match="not built yet"):
            corpus.range_levels(ent, starts, lens, 100, signal=band)
    finally:
        corpus.close()


# ---- 9. the Python mirror
def test_python_mirror(ctx, x3):
    for bad in ([], [1] * 9, [32768], [16385, -16384], [1.5]):
        with pytest.raises(ValueError):
            x3.Fir(bad)
    for bad in (16, -1, 0.5):
        with pytest.raises(ValueError):
            x3.Fir([1], bad)
    f = x3.Fir([1, -2, 1])
    with pytest.raises(AttributeError):
        f.shift = 3
    assert f == x3.Fir((1, -2, 1), 0) and f != x3.Fir([1, -2, 1], 1) and hash(f) == hash(x3.Fir((1, -2, 1))) and f.taps == (1, -2, 1)
    s = f.c_struct()
    assert (s.n_taps, s.shift, list(s.taps)) == (3, 0, [1, -2, 1, 0, 0, 0, 0, 0]) and C.sizeof(s) == 24
    p, op = x3.Params.make(20, 16), O.Params.make(20, 16, (0, 1, 3))
    n = 3 * 320 + 57
    wav = TL._content("patchwork", n, seed=15)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    frames, so = [wav[i:i + 320] for i in range(0, n, 320)], list(range(0, n, 320))
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=4, index="walk")
    try:
        lv, st = ws.levels(100, signal=f)
        assert lv.dtype == x3.LEVEL_DTYPE and lv.size == 11 and st.tolist() == [0, 0, 0, 0]
        _same(lv, FR.fir_levels(frames, st, so, 100, 11, [1, -2, 1]), "WindowSource.levels")
        two, _ = ws.levels(100, n_bins=2, signal=f)
        _same(two, lv[:2], "n_bins")
        assert ws.levels(100, signal=x3.Fir([1]))[0].tobytes() == ws.levels(100)[0].tobytes()
        d_lv = ctx.alloc(32 * 11)
        try:
            assert ws.levels_into(100, d_lv, 11, None, f) == 0 and ctx.levels_result() == (0, 0, 4, 0)
            _same(ctx.download(d_lv, 32 * 11, x3.LEVEL_DTYPE), lv, "levels_into")
        finally:
            ctx.free(d_lv)
        with pytest.raises(ValueError):
            ws.levels(100, signal="fir")
    finally:
        ws.close()
