"""levels_ref.py, the numpy statement of x3_levels_dev's definition, against a per-sample loop and on its edges."""
import numpy as np
import pytest

import levels_ref as R


def _brute(frames, statuses, so, bin_len, n_bins):
    out = [dict(sum_sq=0, sum=0, min=32767, max=-32768, n=0) for _ in range(n_bins)]
    for w, st, o in zip(frames, statuses, so):
        if st != 0:
            continue
        for i, s in enumerate(w):
            b = (int(o) + i) // bin_len if bin_len else 0
            if b >= n_bins:
                continue
            r, s = out[b], int(s)
            r["sum_sq"] += s * s
            r["sum"] += s
            r["min"], r["max"] = min(r["min"], s), max(r["max"], s)
            r["n"] += 1
    return out


def _same(got, want):
    assert got.dtype == R.LEVEL_DTYPE and got.dtype.itemsize == 32 and len(got) == len(want)
    for b, r in enumerate(want):
        for k, v in r.items():
            assert int(got[k][b]) == v, (b, k, int(got[k][b]), v)
    assert not got["reserved"].any()


def _stream(rng, lengths, bad=()):
    frames = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in lengths]
    so = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    statuses = [14 if f in bad else 0 for f in range(len(lengths))]
    return frames, statuses, so


@pytest.mark.parametrize("bin_len", [0, 1, 7, 100, 101, 1000])
def test_against_the_per_sample_loop(bin_len):
    rng = np.random.default_rng(bin_len)
    frames, statuses, so = _stream(rng, [100, 100, 37, 100, 1], bad=(1,))
    total = 338
    for n_bins in {R.n_bins_for(total, bin_len), max(1, R.n_bins_for(total, bin_len) - 1), R.n_bins_for(total, bin_len) + 3}:
        _same(R.levels(frames, statuses, so, bin_len, n_bins), _brute(frames, statuses, so, bin_len, n_bins))


def test_full_scale_samples():
    """-32768 and 32767: sum_sq is 2^30 and 2^30 - 2^16 + 1 a sample; the sums of a bin of full-scale samples stay exact"""
    w = np.array([-32768, 32767, -32768, -32768], dtype=np.int16)
    got = R.levels([w], [0], [0], 2, 2)
    assert int(got["sum_sq"][0]) == (1 << 30) + 32767 * 32767 and int(got["sum_sq"][1]) == 2 << 30
    assert (int(got["min"][0]), int(got["max"][0]), int(got["sum"][0])) == (-32768, 32767, -1)
    assert (int(got["min"][1]), int(got["max"][1]), int(got["sum"][1]), int(got["n"][1])) == (-32768, -32768, -65536, 2)
    many = np.full(65535, -32768, dtype=np.int16)
    one = R.levels([many] * 3, [0] * 3, [0, 65535, 131070], 0, 1)
    assert int(one["sum_sq"][0]) == 3 * 65535 << 30 and int(one["sum"][0]) == -3 * 65535 * 32768 and int(one["n"][0]) == 196605


def test_empty_bins_and_the_cut_off():
    """a gap in the positions leaves identities; positions at or beyond n_bins * bin_len are not counted; a failed frame
    adds nothing, also to a bin it shares"""
    a, b = np.array([5, -6, 7], dtype=np.int16), np.array([100, 200], dtype=np.int16)
    got = R.levels([a, b], [0, 0], [0, 31], 10, 5)
    _same(got, _brute([a, b], [0, 0], [0, 31], 10, 5))
    for k in (1, 2, 4):
        assert (int(got["n"][k]), int(got["min"][k]), int(got["max"][k]), int(got["sum"][k])) == (0, 32767, -32768, 0)
    assert int(got["n"][3]) == 2
    cut = R.levels([a, b], [0, 0], [0, 31], 10, 3)
    assert int(cut["n"].sum()) == 3 and np.array_equal(cut, got[:3])
    shared = R.levels([a, b], [0, 20], [8, 11], 10, 2)     # frame 0 straddles bins 0 and 1, frame 1 (failed) lies in bin 1
    assert (int(shared["n"][0]), int(shared["n"][1]), int(shared["max"][1])) == (2, 1, 7)
    assert np.array_equal(R.levels([a], [1], [0], 10, 2), R.empty(2))


def test_bin_len_0_and_1():
    rng = np.random.default_rng(3)
    frames, statuses, so = _stream(rng, [50, 9, 50])
    every = R.levels(frames, statuses, so, 1, 109)
    flat = np.concatenate(frames).astype(np.int64)
    assert np.array_equal(every["min"], flat) and np.array_equal(every["max"], flat) and (every["n"] == 1).all()
    assert np.array_equal(every["sum_sq"].astype(np.int64), flat * flat)
    one = R.levels(frames, statuses, so, 0, 4)
    assert int(one["n"][0]) == 109 and int(one["sum"][0]) == int(flat.sum()) and np.array_equal(one[1:], R.empty(3))


def test_corpus_row_layout():
    """max(1, ceil(n / bin_len)) rows per entry, one with bin_len 0, an entry of 0 samples keeps one row of identities;
    positions are the entry's own"""
    assert R.corpus_row_first([0, 1, 1000, 1001, 0], 1000).tolist() == [0, 1, 2, 3, 5, 6]
    assert R.corpus_row_first([0, 1, 1000, 1001], 0).tolist() == [0, 1, 2, 3, 4]
    assert R.corpus_row_first([5], 1).tolist() == [0, 5]
    rng = np.random.default_rng(9)
    e0 = _stream(rng, [30, 12]) + (42,)
    e1 = ([], [], [], 0)
    e2 = _stream(rng, [30, 30, 5], bad=(1,)) + (65,)
    rows, rf = R.corpus_levels([e0, e1, e2], 20)
    assert rf.tolist() == [0, 3, 4, 8] and len(rows) == 8
    assert np.array_equal(rows[0:3], R.levels(*e0[:3], 20, 3))
    assert np.array_equal(rows[3:4], R.empty(1))
    assert np.array_equal(rows[4:8], R.levels(*e2[:3], 20, 4))
    assert int(rows["n"][4]) == 20 and int(rows["n"][5]) == 10 and int(rows["n"][6]) == 0 and int(rows["n"][7]) == 5
