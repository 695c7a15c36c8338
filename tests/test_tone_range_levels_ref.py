"""tone_range_levels_ref.py, the numpy statement of x3_tone_range_levels_dev's definition, against a per-position loop and
its siblings (tone_levels_ref, range_levels_ref) on the oracle's decode of the base stream of tests/test_gpu_range_levels.py:
2 137 samples in frames of 400 (block length 20, 20 blocks a frame)."""
import numpy as np
import pytest

import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR
import tone_levels_ref as TL
import tone_range_levels_ref as TR

BAD, CRC = TR.ERR_BAD_ARG, RR.ERR_PAYLOAD_CRC
N = 2137
STEPS = [0, 350898828, 2 ** 31, 2 ** 32 - 1, 2 ** 22]          # (2^22: a period of 1 024 positions)


@pytest.fixture(scope="module")
def base():
    """(frames, sample offsets, wav, stream, frame offsets, op) of the intact stream"""
    import x3hip
    wav = x3hip.synth(2, 1616, 0, N)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    assert rc == 0
    offs = RR.frame_offsets(s)
    frames = RR.frames_of(s, offs, op)
    so = R.sample_offsets([len(w) for _, w in frames])
    assert so.tolist() == [0, 400, 800, 1200, 1600, 2000, 2137]
    return frames, so, wav, s, offs, op


def _hurt(base, f):
    frames, so, wav, s, offs, op = base
    h = s.copy()
    h[offs[f] + 20 + 30] ^= 0x08
    damaged = RR.frames_of(h, offs, op)
    assert [st for st, _ in damaged] == [CRC if g == f else 0 for g in range(6)]
    return damaged


def _random_table(seed=7):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(1024, 2)).astype(np.int16)


def _brute(wav, so, bad, start, length, bin_len, step, tab):
    """a loop over the positions in Python integers; bad: the frames with a status other than 0"""
    out = TL.empty(TR.rows_of(length, bin_len))
    edges = [int(v) for v in so]
    for g in range(start, start + length):
        if max(f for f in range(len(edges) - 1) if edges[f] <= g) in bad:
            continue
        k = ((g * step) % 2 ** 32) >> 22
        v = int(wav[g])
        r = out[(g - start) // bin_len if bin_len else 0]
        r["re"] += v * int(tab[k, 0])
        r["im"] += v * int(tab[k, 1])
        r["min"], r["max"] = min(r["min"], v), max(r["max"], v)
        r["n"] += 1
    return out


RANGES = [(0, N), (0, 1), (1, 1), (6, 3), (399, 3), (400, 400), (400, 1), (401, 1000), (2000, 137), (799, 9), (2136, 1), (81, 40),
          (5, 0), (395, 30)]


@pytest.mark.parametrize("bad", [(), (0,), (2,), (5,), (1, 2)])
def test_the_reference_against_a_loop_over_the_positions(base, bad):
    frames, so, wav = base[:3]
    fr = [(BAD if f == 1 else 13 + f, None) if f in bad else fw for f, fw in enumerate(frames)]
    for step, tab in zip(STEPS, [TL.table(), _random_table(), TL.table(), _random_table(3), TL.table()]):
        for start, ln in RANGES:
            for b in (0, 1, 7, 400):
                got, st = TR.one(fr, so, start, ln, b, step, tab)
                assert np.array_equal(got, _brute(wav, so, bad, start, ln, b, step, tab)), (step, start, ln, b)
                assert st == R.one(fr, so, start, ln, b)[1]          # the status is the SAMPLES call's


@pytest.mark.parametrize("bin_len", [0, 1, 7, 20, 400, 401, 2 ** 32])
def test_the_whole_stream_equals_tone_levels_ref(base, bin_len):
    """identity 1: (0, total) at b is x3_tone_levels_dev at b, damaged frames included"""
    frames, so = base[:2]
    for fr in (frames, _hurt(base, 0), _hurt(base, 2), _hurt(base, 5)):
        for step in STEPS:
            got, _ = TR.one(fr, so, 0, N, bin_len, step, TL.table())
            want = TL.tone_levels([w if st == 0 else [] for st, w in fr], [st for st, _ in fr], so[:-1], bin_len,
                                  TR.rows_of(N, bin_len), step)
            assert np.array_equal(got, want)


@pytest.mark.parametrize("b", [1, 7, 20, 100, 400])
def test_an_aligned_range_is_the_slice_of_the_tone_levels(base, b):
    """identity 2: start and length multiples of b -> the slice; a length that is not -> the last record cut to the range"""
    frames, so = base[:2]
    for fr in (frames, _hurt(base, 2)):
        for step in STEPS[1:]:
            full = TL.tone_levels([w if st == 0 else [] for st, w in fr], [st for st, _ in fr], so[:-1], b, TR.rows_of(N, b), step)
            for first, rows in ((0, 1), (1, 3), (N // b - 2, 2), (400 // b, 800 // b)):
                got, _ = TR.one(fr, so, first * b, rows * b, b, step, TL.table())
                assert np.array_equal(got, full[first:first + rows]), (b, step, first, rows)
            if b > 1:   # the last record cut: the same records but the last, which is the range's own
                got, _ = TR.one(fr, so, b, 2 * b + 1, b, step, TL.table())
                assert np.array_equal(got[:2], full[1:3]) and int(got["n"][2]) in (0, 1)
                assert np.array_equal(got[2:], TR.one(fr, so, 3 * b, 1, b, step, TL.table())[0])


def test_a_table_of_ones_gives_the_samples_records_and_step_0_their_multiple(base):
    """identities 3 and 4, on whole calls: records, row offsets and statuses"""
    frames, so = base[:2]
    ones = np.tile(np.array([1, 0], dtype=np.int16), (1024, 1))
    starts, lens = [0, 399, 2000, N, 900, 1, N + 1, 5, 400, 800], [400, 3, 137, 0, 1000, N, 0, 61, 400, 1]
    for bin_len, stride, cap in ((0, 0, 10), (7, 0, 400), (7, 0, 100), (400, 3, 30), (100, 25, 250)):
        for fr in (frames, _hurt(base, 2), _hurt(base, 0)):
            want, off, status = R.range_levels(fr, so, starts, lens, bin_len, stride, cap)
            plain = R.view(want)
            for step in STEPS:
                got = TR.range_levels(fr, so, starts, lens, bin_len, stride, cap, step, ones)
                assert np.array_equal(got[1], off) and np.array_equal(got[2], status)
                rec = TR.view(got[0])
                written = rec["reserved"] == 0                      # (records no call may write keep the fill)
                assert np.array_equal(written, plain["reserved"] == 0)
                assert np.array_equal(rec["re"][written], plain["sum"][written]) and not rec["im"][written].any()
                for name in ("min", "max", "n"):
                    assert np.array_equal(rec[name], plain[name])
                assert np.array_equal(got[0][~written], want[~written])
            got = TR.range_levels(fr, so, starts, lens, bin_len, stride, cap, 0)          # step 0, the usual table: pair 0 = (32767, 0)
            rec = TR.view(got[0])
            written = rec["reserved"] == 0
            assert np.array_equal(rec["re"][written], 32767 * plain["sum"][written]) and not rec["im"][written].any()
    with pytest.raises(ValueError):
        TR.range_levels(frames, so, [], [], 7, 0, 4, 1)


def test_the_phase_is_the_streams_not_the_ranges(base):
    """a range at a start that is no multiple of the oscillator's period differs from the same samples placed at position 0;
    at a multiple of the period it does not"""
    frames, so, wav = base[:3]
    step, period = 2 ** 22, 1024
    start, ln = 401, 300
    assert start % period
    got, _ = TR.one(frames, so, start, ln, 100, step, TL.table())
    moved = TL.tone_levels([wav[start:start + ln]], [0], [0], 100, 3, step)          # the same samples, a stream of their own
    for name in ("min", "max", "n"):
        assert np.array_equal(got[name], moved[name])
    assert not np.array_equal(got["re"], moved["re"]) and not np.array_equal(got["im"], moved["im"])
    want = TL.tone_levels([wav[400:800]], [0], [400], 100, 8, step)                  # samples at their own positions: bins 4 .. 7
    shifted = TR.one(frames, so, 400, 400, 100, step, TL.table())[0]
    assert np.array_equal(shifted, want[4:8])
    got, _ = TR.one(frames, so, period, ln, 100, step, TL.table())                   # a whole period in: the phase is 0 again
    assert np.array_equal(got, TL.tone_levels([wav[period:period + ln]], [0], [0], 100, 3, step))
    # two ranges over identical samples (a constant) at different starts differ in re and im
    flat = [(0, np.full(400, 1000, dtype=np.int16)) for _ in range(3)]
    fso = R.sample_offsets([400] * 3)
    a, b = TR.one(flat, fso, 0, 200, 0, 350898828, TL.table())[0], TR.one(flat, fso, 333, 200, 0, 350898828, TL.table())[0]
    assert (a["min"], a["max"], a["n"]) == (b["min"], b["max"], b["n"]) and a["re"] != b["re"] and a["im"] != b["im"]
