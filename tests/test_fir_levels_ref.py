"""fir_levels_ref.py, the numpy definition the GPU tests hold x3_fir_levels_dev against, held itself against the definition
of include/x3hip.h ("FIR LEVELS") written as a loop over positions, and against levels_ref.py / diff_levels_ref.py for the
two identities.  CPU only."""
import numpy as np
import pytest

import diff_levels_ref as D
import fir_levels_ref as FR
import levels_ref as R

TAP_SETS = [([1], 0), ([1, -1], 0), ([1, -2, 1], 0), ([1, 0, -1], 0), ([1, 1, 1, 1], 2), ([-3000, 9000, -200, 7, 5000, -8000, 1, 6560], 7),
            ([0, 0, 0, 0, 0, 0, 0, 1], 0), ([16384, -16384], 0), ([-32768], 15), ([-1], 15)]


def _by_positions(frames, statuses, sample_offsets, bin_len, n_bins, taps, shift):
    """the header's definition, position by position, in Python integers"""
    x = {}
    for w, st, so in zip(frames, statuses, sample_offsets):
        if st == 0:
            for i, v in enumerate(w):
                x[int(so) + i] = int(v)
    out = R.empty(n_bins)
    T = len(taps)
    for i in sorted(x):
        if any(i - t not in x for t in range(T)):      # (a position in front of the first is in no frame)
            continue
        acc = sum(int(taps[t]) * x[i - t] for t in range(T))
        assert -(1 << 30) <= acc <= 1 << 30
        y = min(max(acc >> shift, -32768), 32767)      # (Python's >> floors)
        b = i // bin_len if bin_len else 0
        if b >= n_bins:
            continue
        r = out[b]
        r["n"] += 1
        r["sum"] += y
        r["sum_sq"] += y * y
        r["min"], r["max"] = min(int(r["min"]), y), max(int(r["max"]), y)
    return out


def _stream(seed, lens, full_scale=False):
    rng = np.random.default_rng(seed)
    hi = 32768 if full_scale else 3000
    frames = [rng.integers(-hi, hi, size=n).astype(np.int16) for n in lens]
    so = np.concatenate([[0], np.cumsum(lens)])[:-1]
    return frames, so


@pytest.mark.parametrize("taps,shift", TAP_SETS)
def test_against_the_loop_over_positions(taps, shift):
    lens = [40, 1, 2, 3, 1, 1, 7, 8, 9, 40, 17]
    frames, so = _stream(len(taps) * 16 + shift, lens, full_scale=True)
    n = sum(lens)
    for statuses in ([0] * 11, [0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0], [5] + [0] * 9 + [7], [0] * 9 + [5, 0], [5] * 11):
        for bin_len in (0, 1, 7, 40, 41):
            for n_bins in {R.n_bins_for(n, bin_len), max(1, R.n_bins_for(n, bin_len) - 1), R.n_bins_for(n, bin_len) + 2}:
                got = FR.fir_levels(frames, statuses, so, bin_len, n_bins, taps, shift)
                want = _by_positions(frames, statuses, so, bin_len, n_bins, taps, shift)
                assert got.tobytes() == want.tobytes(), (statuses, bin_len, n_bins)
        if not any(statuses):
            assert int(FR.fir_levels(frames, statuses, so, 0, 1, taps, shift)["n"][0]) == max(0, n - len(taps) + 1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 9])
def test_streams_shorter_than_the_taps(n):
    frames, so = _stream(n, [n], full_scale=True)
    for taps, shift in TAP_SETS:
        for bin_len in (0, 1, 3):
            n_bins = R.n_bins_for(n, bin_len) + 1
            got = FR.fir_levels(frames, [0], so, bin_len, n_bins, taps, shift)
            assert got.tobytes() == _by_positions(frames, [0], so, bin_len, n_bins, taps, shift).tobytes(), (taps, bin_len)
            assert int(got["n"].sum()) == max(0, n - len(taps) + 1)


def test_the_two_identities():
    lens = [50, 50, 1, 1, 50, 23]
    frames, so = _stream(7, lens, full_scale=True)
    for statuses in ([0] * 6, [0, 3, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0], [3, 0, 0, 0, 0, 3]):
        for bin_len in (0, 1, 7, 50, 51):
            n_bins = R.n_bins_for(sum(lens), bin_len)
            assert FR.fir_levels(frames, statuses, so, bin_len, n_bins, [1]).tobytes() == \
                R.levels(frames, statuses, so, bin_len, n_bins).tobytes()
            assert FR.fir_levels(frames, statuses, so, bin_len, n_bins, [1, -1]).tobytes() == \
                D.signal_levels(frames, statuses, so, bin_len, n_bins, D.DIFF).tobytes()


def test_a_failed_frame_takes_the_positions_behind_it():
    frames, so = _stream(3, [10, 10, 10])
    for T in range(1, 9):
        lv = FR.fir_levels(frames, [0, 9, 0], so, 1, 30, [0] * (T - 1) + [1])
        assert lv["n"].tolist() == [0] * (T - 1) + [1] * (10 - T + 1) + [0] * 10 + [0] * (T - 1) + [1] * (10 - T + 1)
        assert lv["sum"][20 + T - 1:].tolist() == [int(v) for v in frames[2][:10 - T + 1]]      # a pure delay


def test_arithmetic_edges():
    x = np.array([-32768, 32767] * 4, dtype=np.int16)
    lv = FR.fir_levels([x], [0], [0], 1, 8, [16384, -16384])
    assert lv["n"].tolist() == [0] + [1] * 7 and lv["sum"][1:].tolist() == [32767, -32768] * 3 + [32767]
    one = FR.fir_levels([np.array([-32768], dtype=np.int16)], [0], [0], 0, 1, [-32768], 15)
    assert (int(one["sum"][0]), int(one["sum_sq"][0]), int(one["n"][0])) == (32767, 32767 * 32767, 1)      # acc = 2^30
    neg = FR.fir_levels([np.array([1, 3, 32767], dtype=np.int16)], [0], [0], 1, 3, [-1], 15)
    assert neg["sum"].tolist() == [-1, -1, -1]                                                                 # floor, not 0


def test_corpus_entries_are_separate():
    a, so_a = _stream(1, [20, 5])
    b, so_b = _stream(2, [3])
    rows, rf = FR.corpus_fir_levels([(a, [0, 0], so_a, 25), ([], [], [], 0), (b, [0], so_b, 3)], 10, [1, 0, 0, -1])
    assert rf.tolist() == [0, 3, 4, 5] and rows["n"].tolist() == [7, 10, 5, 0, 0]
    assert FR.check([1] * 8, 15) and not FR.check([], 0) and not FR.check([1] * 9, 0) and not FR.check([1], 16)
    assert FR.check([-32768], 0) and not FR.check([32768], 0) and not FR.check([16385, -16384], 0)
