"""diff_levels_ref.py, the numpy statement of x3_signal_levels_dev's definition, against a per-position loop and on its edges."""
import numpy as np
import pytest

import diff_levels_ref as D
import levels_ref as R


def _clamp(v):
    return max(-32768, min(32767, v))


def _brute(frames, statuses, so, bin_len, n_bins):
    """include/x3hip.h, "SIGNAL LEVELS", position by position"""
    out = [dict(sum_sq=0, sum=0, min=32767, max=-32768, n=0) for _ in range(n_bins)]
    for f, (w, st, o) in enumerate(zip(frames, statuses, so)):
        for i in range(len(w)):
            if st != 0:
                continue
            if i >= 1:
                y = _clamp(int(w[i]) - int(w[i - 1]))
            elif f >= 1 and statuses[f - 1] == 0:
                y = _clamp(int(w[0]) - int(frames[f - 1][-1]))
            else:
                continue
            b = (int(o) + i) // bin_len if bin_len else 0
            if b >= n_bins:
                continue
            r = out[b]
            r["sum_sq"] += y * y
            r["sum"] += y
            r["min"], r["max"] = min(r["min"], y), max(r["max"], y)
            r["n"] += 1
    return out


def _same(got, want):
    assert got.dtype == R.LEVEL_DTYPE and len(got) == len(want)
    for b, r in enumerate(want):
        for k, v in r.items():
            assert int(got[k][b]) == v, (b, k, int(got[k][b]), v)
    assert not got["reserved"].any()


def _stream(rng, lengths, bad=()):
    frames = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in lengths]
    so = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    statuses = [14 if f in bad else 0 for f in range(len(lengths))]
    return frames, statuses, so


CASES = {
    "clean": ([100, 100, 37, 100, 1], ()),
    "failed frame in the middle": ([100, 100, 37, 100, 1], (2,)),
    "failed first frame": ([100, 100, 37], (0,)),
    "failed last frame": ([100, 100, 37], (2,)),
    "two failed neighbours": ([50, 20, 20, 50], (1, 2)),
    "one-sample frames": ([1, 1, 1, 5, 1, 1], ()),
    "one-sample frames, one failed": ([1, 1, 1, 5, 1, 1], (1,)),
    "one frame": ([64], ()),
    "one sample": ([1], ()),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("bin_len", [0, 1, 7, 100, 101])
def test_against_the_per_position_loop(case, bin_len):
    lengths, bad = CASES[case]
    frames, statuses, so = _stream(np.random.default_rng([bin_len, len(lengths)]), lengths, bad)
    exact = R.n_bins_for(sum(lengths), bin_len)
    for n_bins in {exact, max(1, exact - 1), exact + 3}:
        _same(D.signal_levels(frames, statuses, so, bin_len, n_bins, D.DIFF), _brute(frames, statuses, so, bin_len, n_bins))


def test_a_failed_frame_takes_both_of_its_seams():
    """bin_len 1: the positions of a failed frame, and sample 0 of the frame behind it, are empty; so is position 0"""
    frames, statuses, so = _stream(np.random.default_rng(1), [4, 3, 4], bad=(1,))
    got = D.signal_levels(frames, statuses, so, 1, 11, D.DIFF)
    assert got["n"].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1]
    clean = D.signal_levels(frames, [0, 0, 0], so, 1, 11, D.DIFF)
    assert clean["n"].tolist() == [0] + [1] * 10
    assert int(clean["sum"][4]) == _clamp(int(frames[1][0]) - int(frames[0][-1]))


def test_n_sums_to_samples_minus_one():
    frames, statuses, so = _stream(np.random.default_rng(2), [100, 1, 37, 1, 1, 64])
    for bin_len in (0, 1, 10, 1000):
        got = D.signal_levels(frames, statuses, so, bin_len, R.n_bins_for(204, bin_len), D.DIFF)
        assert int(got["n"].sum()) == 203, bin_len


def test_full_scale_alternation_clamps_both_ways():
    w = np.tile(np.array([-32768, 32767], dtype=np.int16), 8)
    frames, so = [w[:5], w[5:6], w[6:]], [0, 5, 6]
    got = D.signal_levels(frames, [0, 0, 0], so, 1, 16, D.DIFF)
    assert got["n"].tolist() == [0] + [1] * 15
    assert got["max"][1:].tolist() == [32767, -32768] * 7 + [32767]       # +65535 -> 32767, -65535 -> -32768
    assert np.array_equal(got["min"][1:], got["max"][1:])
    one = D.signal_levels(frames, [0, 0, 0], so, 0, 1, D.DIFF)
    assert (int(one["min"][0]), int(one["max"][0]), int(one["n"][0])) == (-32768, 32767, 15)
    assert int(one["sum_sq"][0]) == 8 * 32767 * 32767 + 7 * (1 << 30) and int(one["sum"][0]) == 8 * 32767 - 7 * 32768
    _same(got, _brute(frames, [0, 0, 0], so, 1, 16))


def test_two_entries_back_to_back_have_no_seam_between_them():
    rng = np.random.default_rng(5)
    e0 = _stream(rng, [30, 12]) + (42,)
    e1 = _stream(rng, [1]) + (1,)
    e2 = ([], [], [], 0)
    e3 = _stream(rng, [30, 30, 5], bad=(1,)) + (65,)
    for bin_len in (0, 1, 20):
        rows, rf = D.corpus_signal_levels([e0, e1, e2, e3], bin_len, D.DIFF)
        assert np.array_equal(rf, R.corpus_row_first([42, 1, 0, 65], bin_len))
        for e, ent in enumerate((e0, e1, e2, e3)):
            a, b = int(rf[e]), int(rf[e + 1])
            assert np.array_equal(rows[a:b], D.signal_levels(*ent[:3], bin_len, b - a, D.DIFF)), (bin_len, e)
            if ent[3]:
                _same(rows[a:b], _brute(*ent[:3], bin_len, b - a))
        assert int(rows["n"][int(rf[0]):int(rf[1])].sum()) == 41        # the first entry: N - 1
        assert np.array_equal(rows[int(rf[1]):int(rf[3])], R.empty(2))  # a one-sample entry and an empty one: identities
        if bin_len == 1:
            assert int(rows["n"][int(rf[3])]) == 0                       # the first sample of an entry has no difference


@pytest.mark.parametrize("bin_len", [0, 1, 7, 100])
def test_samples_is_levels_ref(bin_len):
    frames, statuses, so = _stream(np.random.default_rng(7), [100, 100, 37, 100, 1], bad=(1,))
    n_bins = R.n_bins_for(338, bin_len)
    assert np.array_equal(D.signal_levels(frames, statuses, so, bin_len, n_bins, D.SAMPLES), R.levels(frames, statuses, so, bin_len, n_bins))
    ent = (frames, statuses, so, 338)
    got, rf = D.corpus_signal_levels([ent, ent], bin_len, D.SAMPLES)
    want, rf2 = R.corpus_levels([ent, ent], bin_len)
    assert np.array_equal(got, want) and np.array_equal(rf, rf2)
