"""fir_range_levels_ref.py, the numpy statement of x3_fir_range_levels_dev's definition, against a per-position loop and its
siblings (range_levels_ref, signal_range_levels_ref, fir_levels_ref) on the oracle's decode of the base stream of
tests/test_gpu_range_levels.py: 2 137 samples in frames of 400 (block length 20, 20 blocks a frame)."""
import numpy as np
import pytest

import fir_levels_ref as FL
import fir_range_levels_ref as FR
import levels_ref as LR
import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR
import signal_range_levels_ref as S

BAD, CRC = FR.ERR_BAD_ARG, RR.ERR_PAYLOAD_CRC
N = 2137
FIRS = [((1,), 0), ((1, -1), 0), ((1, -2, 1), 0), ((1, 0, -1), 0), ((3, -5, 7, -11, 13, -17, 19, -23), 7), ((-3, 2), 15)]


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


def _brute(wav, so, bad, start, length, bin_len, taps, shift):
    """a loop over the positions; bad: the frames with a status other than 0"""
    out = LR.empty(FR.rows_of(length, bin_len))
    edges = [int(v) for v in so]
    frame_of = lambda g: max(f for f in range(len(edges) - 1) if edges[f] <= g)   # noqa: E731
    T = len(taps)
    for g in range(start, start + length):
        if g < T - 1 or any(frame_of(g - t) in bad for t in range(T)):
            continue
        v = min(max(sum(int(c) * int(wav[g - t]) for t, c in enumerate(taps)) >> shift, -32768), 32767)
        r = out[(g - start) // bin_len if bin_len else 0]
        r["sum_sq"] += v * v
        r["sum"] += v
        r["min"], r["max"] = min(r["min"], v), max(r["max"], v)
        r["n"] += 1
    return out


RANGES = [(0, N), (0, 1), (1, 1), (6, 3), (399, 3), (400, 400), (400, 1), (401, 1000), (406, 2), (407, 1), (2000, 137), (799, 9),
          (2136, 1), (81, 40), (5, 0), (395, 30)]


@pytest.mark.parametrize("bad", [(), (0,), (2,), (5,), (1, 2)])
def test_the_reference_against_a_loop_over_the_positions(base, bad):
    frames, so, wav = base[:3]
    fr = [(BAD if f == 1 else 13 + f, None) if f in bad else fw for f, fw in enumerate(frames)]
    for taps, shift in FIRS:
        sig = FR.signal_of(fr, so, taps, shift)
        for start, ln in RANGES:
            for b in (0, 1, 7, 400):
                got, st = FR.one(fr, so, start, ln, b, taps, shift, sig)
                assert np.array_equal(got, _brute(wav, so, bad, start, ln, b, taps, shift)), (taps, start, ln, b)
                assert st == R.one(fr, so, start, ln, b)[1]          # the status is the SAMPLES call's


def test_what_n_counts(base):
    frames, so = base[:2]
    taps = (1, 0, -1)
    assert int(FR.one(frames, so, 0, N, 0, taps)[0]["n"][0]) == N - 2          # the entry's first T - 1 positions have no output
    for start, ln in ((2, 2135), (399, 3), (400, 400), (800, 1), (2136, 1)):
        assert int(FR.one(frames, so, start, ln, 0, taps)[0]["n"][0]) == ln     # ... T - 1 in, a clean range has one per position
    hurt = _hurt(base, 1)                                                      # a failed lead frame: T - 1 positions, status 0
    got, st = FR.one(hurt, so, 800, 400, 0, taps)
    assert st == 0 and int(got["n"][0]) == 398
    got, st = FR.one(hurt, so, 801, 10, 0, taps)
    assert st == 0 and int(got["n"][0]) == 9
    got, st = FR.one(hurt, so, 0, N, 400, taps)
    assert st == CRC and got["n"].tolist() == [398, 0, 398, 400, 400, 137]


def test_one_tap_is_range_levels_ref_and_two_are_the_difference(base):
    frames, so = base[:2]
    starts, lens = [0, 399, 2000, N, 900, 1, N + 1, 5, 400, 800], [400, 3, 137, 0, 1000, N, 0, 61, 400, 1]
    for bin_len, stride, cap in ((0, 0, 10), (7, 0, 400), (7, 0, 100), (400, 3, 30), (100, 25, 250)):
        for fr in (frames, _hurt(base, 2), _hurt(base, 0)):
            want = R.range_levels(fr, so, starts, lens, bin_len, stride, cap)
            got = FR.range_levels(fr, so, starts, lens, bin_len, stride, cap, (1,))
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            want = S.range_levels(fr, so, starts, lens, bin_len, stride, cap, S.DIFF)
            got = FR.range_levels(fr, so, starts, lens, bin_len, stride, cap, (1, -1))
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        FR.range_levels(frames, so, [], [], 7, 0, 4, (1,))


@pytest.mark.parametrize("bin_len", [0, 1, 7, 20, 400, 401, 2 ** 32])
def test_the_whole_stream_equals_fir_levels_ref(base, bin_len):
    frames, so = base[:2]
    for fr in (frames, _hurt(base, 0), _hurt(base, 2), _hurt(base, 5)):
        for taps, shift in FIRS[2:]:
            got, _ = FR.one(fr, so, 0, N, bin_len, taps, shift)
            want = FL.fir_levels([w if st == 0 else [] for st, w in fr], [st for st, _ in fr], so[:-1], bin_len,
                                 FR.rows_of(N, bin_len), taps, shift)
            assert np.array_equal(got, want)
