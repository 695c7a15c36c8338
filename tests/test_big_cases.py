"""tests/big_cases.py proved on the CPU: the tiled stream at four places against the oracle's decode of the whole of it, the
reference's frame walk, and levels_ref / diff_levels_ref / the range references on the whole small signal -- with and
without damaged frames.  The builder's conditions at the full place count are arithmetic and checked here too.  What
tests/test_gpu_beyond_4gib.py compares the device with is this reference at 6 921 places instead of four."""
import numpy as np
import pytest

import big_cases as B
import diff_levels_ref as DR
import fir_levels_ref as FL
import fir_range_levels_ref as FRL
import frame_walk_ref as FW
import levels_ref as LR
import oracle_lib as O
import ranges_ref as RR
import range_levels_ref as RL
import signal_range_levels_ref as SRL
import tone_levels_ref as TL

DAMAGE = {"clean": [], "damaged": [(0, 63), (2, 17), (2, 18), (3, 0)]}   # (place, frame in tile)


class Small:
    def __init__(self, name):
        self.case = c = B.Case(4)
        self.statuses = c.damage(DAMAGE[name]) if DAMAGE[name] else []
        self.stream = c.stream_bytes(0, c.total_bytes)
        self.offs = RR.frame_offsets(self.stream)
        self.frames = RR.frames_of(self.stream, self.offs)
        self.so = RR.sample_offsets([B.SPF] * c.F)
        self.wavs = [c.samples(f * B.SPF, (f + 1) * B.SPF) for f in range(c.F)]
        self.st = [s for s, _ in self.frames]


@pytest.fixture(scope="module", params=list(DAMAGE))
def small(request):
    return Small(request.param)


def test_full_size_conditions():
    """at the full place count: both totals pass 2^32 + 2^27, the stream stays under 6 GB, a wrap modulo 2^32 lands on other
    content, and the three marked places differ from their neighbours"""
    c = B.Case()
    assert c.total_bytes > B.EDGE + B.MARGIN and c.total > B.EDGE + B.MARGIN and c.total_bytes <= B.MAX_BYTES
    cond = B.modulo_conditions(c)
    assert len(cond) == 1 + len(c.tiles) and all(cond.values()), cond
    mb, ms = c.place_of_byte(B.EDGE), B.EDGE // B.TS
    assert c.place_off[mb] <= B.EDGE < c.place_off[mb + 1] and ms * B.TS <= B.EDGE < (ms + 1) * B.TS
    for m in (mb, ms, c.M - 1):
        assert c.kind[m] not in (c.kind[m - 1], c.kind[(m + 1) % c.M]), m
    assert (c.kind[mb], c.kind[ms], c.kind[-1]) == (2, 2, 3) and set(c.kind[:ms + 1]) == {0, 1, 2}
    fo = c.frame_offsets()
    assert fo.size == c.F + 1 and fo[-1] == c.total_bytes and np.all(np.diff(fo.astype(np.int64)) >= 22)
    f = c.frame_of_byte(B.EDGE)
    assert fo[f] < B.EDGE < fo[f + 1] and c.frame_span(f) == (int(fo[f]), int(fo[f + 1]))
    # a span across byte 2^32 and one across sample 2^32 are the tiles' own content there
    a, b = c.frame_span(f)
    t = c.tiles[2]
    i = f % B.FPT
    assert np.array_equal(c.stream_bytes(a, b), t.stream[t.fo[i]:t.fo[i + 1]])
    g = B.EDGE - 3
    assert np.array_equal(c.samples(g, g + 6), t.wav[g % B.TS:g % B.TS + 6])


def test_tiles_mix():
    """every tile has quiet, ordinary and dense frames; only tile 3 has bins above the loud mean square"""
    for k, t in enumerate(B.tiles()):
        plen = np.diff(t.fo) - 20
        assert (plen > B.IMAGE).sum() >= 24 and (plen < 5000).sum() >= 10 and plen.max() < B.READER
        ms = (t.wav.astype(np.int64).reshape(B.FPT, B.SPF) ** 2).sum(axis=1) // B.SPF
        assert (ms >= B.LOUD_MEAN_SQ).any() == (k == 3)


def test_decode_and_offsets(small):
    c = small.case
    rc, wav, fok, ferr = O.decode_stream(small.stream)
    f, st = c.first_bad(0, c.F)
    if f is None:
        assert (rc, fok, ferr) == (0, c.F, 0) and np.array_equal(wav, c.samples(0, c.total))
    else:
        assert (rc, fok) == (st, f) and np.array_equal(wav, c.samples(0, f * B.SPF))
    w = FW.walk(small.stream)
    assert (w.n_frames, w.n_samples, w.terminal) == (c.F, c.total, 0)
    assert np.array_equal(w.frame_off, c.frame_offsets()[:-1]) and np.array_equal(w.wav_off, c.sample_offsets()[:-1])
    assert small.offs == c.frame_offsets().tolist()
    # the statuses are the oracle's, frame for frame, and undamaged frames decode to the virtual signal
    assert small.st == [c.bad.get(i, 0) for i in range(c.F)] and small.statuses == [c.bad[k] for k in sorted(c.bad)]
    assert all(s or np.array_equal(x, small.wavs[i]) for i, (s, x) in enumerate(small.frames))


def test_header_damage_ends_the_walk():
    c = B.Case(4)
    assert c.damage([(2, 9)], where="header") == [FW.INVALID_HEADER_CRC]
    w = FW.walk(c.stream_bytes(0, c.total_bytes))
    assert (w.n_frames, w.terminal) == (2 * B.FPT + 9, FW.INVALID_HEADER_CRC)


@pytest.mark.parametrize("bin_len", [10000, 640000, 20000, 2000, 128, 0])
def test_levels_records(small, bin_len):
    c = small.case
    nb = LR.n_bins_for(c.total, bin_len)
    for sig in (B.SAMPLES, B.DIFF):
        want = DR.signal_levels(small.wavs, small.st, small.so[:-1], bin_len, nb, sig)
        got = c.levels(bin_len, signal=sig)
        assert got.dtype == LR.LEVEL_DTYPE and np.array_equal(got, want), (bin_len, sig, np.flatnonzero(got != want)[:8])
    if bin_len:
        assert np.array_equal(c.levels(bin_len, nb - 3, B.DIFF), want[:nb - 3]) and np.array_equal(c.levels(bin_len, nb + 2)[nb:], LR.empty(2))


def test_range_levels_and_windows(small):
    c = small.case
    T = B.TS
    ranges = [(0, 3 * T), (T - 5000, 3 * 10000 + 7), (T + 5000, 25000), (2 * T - 1, 2), (17 * 10000 - 1, 10001), (12345, 2 * T + 7),
              (c.total - 10000, 10000), (c.total - 9999, 10000), (c.total, 0), (5, 0)]
    sig = SRL.signal_of(small.frames, small.so)
    for start, length in ranges:
        for bin_len in (10000, 2000):
            want, st = RL.one(small.frames, small.so, start, length, bin_len)
            assert c.range_status(start, length) == st, (start, length)
            assert np.array_equal(c.range_levels(start, length, bin_len), want), (start, length, bin_len)
            want = SRL.one(small.frames, small.so, start, length, bin_len, sig=sig)[0]
            assert np.array_equal(c.range_levels(start, length, bin_len, B.DIFF), want), (start, length, bin_len, "diff")
        row, st = RR.one(small.frames, small.so, start, length)
        got = c.window(start, length)
        assert got[1] == st and np.array_equal(got[0], row), (start, length)
    # the phase mechanism against the samples themselves
    for phase in (1, 2296, 9999):
        rec = c.records(10000, B.DIFF, phase)
        for i in (0, 63, 64, 127, 128, 255):
            a = phase + i * 10000
            assert rec[i] == c.record_of(a, min(a + 10000, c.total), B.DIFF)[0], (phase, i)


# ------------------------------------------------------------------------------------------------ FIR and tone signals

FIR_DAMAGE = {"clean": [], "damaged": DAMAGE["damaged"], "seam": [(1, 63), (2, 0)]}   # seam: a place's last frame and the next one's first


@pytest.fixture(scope="module", params=list(FIR_DAMAGE))
def fir_small(request):
    s = Small("clean")
    if FIR_DAMAGE[request.param]:
        s.case.damage(FIR_DAMAGE[request.param])
        s.st = [s.case.bad.get(f, 0) for f in range(s.case.F)]
        s.frames = [(st, None if st else w) for st, w in zip(s.st, s.wavs)]
    return s


@pytest.mark.parametrize("phase", [0, 777])
@pytest.mark.parametrize("bin_len", [10000, 640000])
def test_fir_records(fir_small, bin_len, phase):
    """the closed form in the tiles against fir_levels_ref run over the whole small signal, the bins `phase` into the places"""
    c = fir_small.case
    sh = (-phase) % bin_len                           # (positions moved up so that position `phase` begins a bin)
    b0, nb = (phase + sh) // bin_len, c.total // bin_len
    so = [int(v) + sh for v in fir_small.so[:-1]]
    for sig in (B.FIR8, B.FIR_DIFF):
        want = FL.fir_levels(fir_small.wavs, fir_small.st, so, bin_len, b0 + nb, sig[1], sig[2])[b0:]
        got = c.records(bin_len, sig, phase)
        assert got.dtype == LR.LEVEL_DTYPE and np.array_equal(got, want), (sig, np.flatnonzero(got != want)[:8])
        assert int(want["n"].sum()) > 0.9 * c.total and int(want["max"].max()) > 1000
        if phase == 0:
            assert np.array_equal(c.levels(bin_len, signal=sig), want) and np.array_equal(c.levels(bin_len, nb - 2, sig), want[:nb - 2])
            one = FL.fir_levels(fir_small.wavs, fir_small.st, so, 0, 1, sig[1], sig[2])
            assert np.array_equal(c.levels(0, signal=sig), one)
    # taps (1, -1) count the positions DIFF counts and hold the same values there: the records are DIFF's
    assert np.array_equal(c.records(bin_len, B.FIR_DIFF, phase), c.records(bin_len, B.DIFF, phase))
    # and the contract at the edges: the stream's first T - 1 samples and the first T - 1 behind a failed frame add nothing
    T = len(B.FIR8[1])
    v, ok = c.signal_values(0, 20, B.FIR8)
    assert ok.tolist() == [False] * (T - 1) + [True] * (21 - T)
    for f in sorted(c.bad):
        _, ok = c.signal_values(f * B.SPF - 3, (f + 1) * B.SPF + 12, B.FIR8)
        after = c.bad.get(f + 1, 0) == 0
        assert not ok[3:3 + B.SPF + T - 1].any() and (not after or ok[3 + B.SPF + T - 1:].all())


def test_fir_range_levels(fir_small):
    """range_levels of a FIR signal against fir_range_levels_ref: the call cuts the filtered stream, so a range's first T - 1
    positions count; starts at a frame seam +- 1, at a tile seam, and T - 1 behind a damaged frame"""
    c = fir_small.case
    T, S, TS = len(B.FIR8[1]), B.SPF, B.TS
    ranges = [(5 * S - 1, 25000), (5 * S, 25000), (5 * S + 1, 25000), (TS - 1, 2), (TS, 3 * S), (TS + 1, 20001), (0, 30000), (3, 5),
              (c.total - 10000, 10000), (c.total - 9999, 10000), (c.total, 0), (12345, 2 * TS + 7), (TS - 5000, 3 * 10000 + 7)]
    for f in sorted(c.bad):
        e = (f + 1) * S                               # the first position behind the damaged frame
        ranges += [(e + T - 2, 15000), (e + T - 1, 15000), (e, 6), (e - S - 4, 8), (e - 3, 2 * S)]
    for sig in (B.FIR8, B.FIR_DIFF):
        y = FRL.signal_of(fir_small.frames, fir_small.so, sig[1], sig[2])
        for start, length in ranges:
            for bin_len in (10000, 2000):
                want, st = FRL.one(fir_small.frames, fir_small.so, start, length, bin_len, sig[1], sig[2], sig=y)
                assert c.range_status(start, length) == st, (start, length)
                got = c.range_levels(start, length, bin_len, sig)
                assert np.array_equal(got, want), (sig, start, length, bin_len, np.flatnonzero(got != want)[:4])
    if c.bad:      # T - 1 behind a damaged frame: the first position that counts again
        e = (min(f for f in c.bad if f + 1 not in c.bad) + 1) * S
        assert int(c.range_levels(e, T - 1, 10000, B.FIR8)["n"][0]) == 0 and int(c.range_levels(e, T, 10000, B.FIR8)["n"][0]) == 1
    for phase in (1, 2296, 9999):                     # the phase mechanism against the samples themselves
        rec = c.records(10000, B.FIR8, phase)
        for i in (0, 63, 64, 127, 128, 255):
            a = phase + i * 10000
            assert rec[i] == c.record_of(a, min(a + 10000, c.total), B.FIR8)[0], (phase, i)


TONE_STEPS = (276168143, 0xFFFFFFFF, 1 << 31, 1 << 30, 0)     # an odd general one first (near 12 345.678 Hz at 192 kHz)


def test_tone_records_past_2_32():
    """Case.tone_records at the full size against tone_levels_ref on the same frames at their own sample offsets, which lie
    below and above 2^32: the phase is by absolute position"""
    c = B.Case()
    S = B.SPF
    f0 = B.EDGE // S - 2
    c.damage([divmod(f0 + 4, B.FPT)])                 # (a frame above 2^32)
    assert (f0 + 2) * S < B.EDGE < (f0 + 3) * S
    nf = 6
    wavs = [c.samples(f * S, (f + 1) * S) for f in range(f0, f0 + nf)]
    st = [c.bad.get(f, 0) for f in range(f0, f0 + nf)]
    so = [f * S for f in range(f0, f0 + nf)]
    for step in TONE_STEPS:
        for bin_len in (10000, 2000):
            per = S // bin_len
            want = TL.tone_levels(wavs, st, so, bin_len, (f0 + nf) * per, step)[f0 * per:]
            got = c.tone_records(f0 * S, (f0 + nf) * S, bin_len, step)
            assert got.dtype == TL.TONE_DTYPE and np.array_equal(got, want), (step, bin_len, np.flatnonzero(got != want)[:4])
            assert int(got["n"].sum()) == (nf - 1) * S and not got["n"][4 * per:5 * per].any()
    # a slice that begins and ends inside bins of the stream: bins from its own start, the last one short
    g0, g1 = f0 * S + 4000, (f0 + 2) * S + 321
    cut = [w.copy() for w in wavs[:3]]
    cut[0], cut[2] = cut[0][4000:], cut[2][:321]
    want = TL.tone_levels(cut, [0, 0, 0], [0, S - 4000, 2 * S - 4000], 5000, 4, 1)      # (step 1: the pair is the position >> 22)
    got = c.tone_records(g0, g1, 5000, 1)
    assert got.size == 4 and np.array_equal(got[["min", "max", "n"]], want[["min", "max", "n"]]) and int(got["n"][3]) == 1321
    tab = TL.table().astype(np.int64)
    x = c.samples(g0, g0 + 5000).astype(np.int64)
    k = ((np.arange(g0, g0 + 5000) % B.EDGE) >> 22)
    assert int(got["re"][0]) == int((x * tab[k, 0]).sum()) and int(got["im"][0]) == int((x * tab[k, 1]).sum())
    # a wrapped position gives other records: the test would see a phase computed from the low 32 bits of a byte or frame base
    assert not np.array_equal(c.tone_records(f0 * S, (f0 + 1) * S, 10000, TONE_STEPS[0])[["re", "im"]],
                              B.tone_records_of(wavs[0], np.ones(S, dtype=bool), f0 * S + 1, 10000, TONE_STEPS[0])[["re", "im"]])


def test_tone_records_near_2_33():
    """tone_records_of at positions across 2^33 (no stream here is that long: the arithmetic alone) against tone_levels_ref"""
    rng = np.random.default_rng(33)
    bin_len, pos0 = 25000, ((1 << 33) // 25000 - 1) * 25000
    assert pos0 < (1 << 33) < pos0 + 2 * bin_len
    x = rng.integers(-32768, 32768, size=3 * bin_len).astype(np.int16)
    counted = np.ones(x.size, dtype=bool)
    counted[30000:40000] = False
    frames = [x[:30000], x[30000:40000], x[40000:]]
    b0 = pos0 // bin_len
    for step in TONE_STEPS:
        want = TL.tone_levels(frames, [0, 5, 0], [pos0, pos0 + 30000, pos0 + 40000], bin_len, b0 + 3, step)[b0:]
        got = B.tone_records_of(x, counted, pos0, bin_len, step)
        assert np.array_equal(got, want), (step, got, want)
