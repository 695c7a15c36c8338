"""tests/big_cases.py proved on the CPU: the tiled stream at four places against the oracle's decode of the whole of it, the
reference's frame walk, and levels_ref / diff_levels_ref / the range references on the whole small signal -- with and
without damaged frames.  The builder's conditions at the full place count are arithmetic and checked here too.  What
tests/test_gpu_beyond_4gib.py compares the device with is this reference at 6 921 places instead of four."""
import numpy as np
import pytest

import big_cases as B
import diff_levels_ref as DR
import frame_walk_ref as FW
import levels_ref as LR
import oracle_lib as O
import ranges_ref as RR
import range_levels_ref as RL
import signal_range_levels_ref as SRL

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
