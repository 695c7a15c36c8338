"""spectra_levels_ref.py, the definition of x3_spectra_levels_dev, against a plain Python loop over spectra_ref.power rows, at
the edges of the time bins, at the per-frame clamp, and in the layouts and statuses of spectra_ref.spectra_rows.  CPU only."""
import math

import numpy as np
import pytest

import spectra_levels_ref as SL
import spectra_ref as S

WILD = 0xFFFFFFFF


def noise(n, seed=3):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


def plain(ms, per_bin, bin_band, n_bands):
    """the definition word for word: Python integers, a loop per (time bin, band, frame, bin)"""
    ms = [[int(v) for v in row] for row in ms]
    t = (len(ms) + per_bin - 1) // per_bin
    out = np.zeros((n_bands, t), dtype=SL.LEVEL)
    for j in range(t):
        frames = ms[j * per_bin:min((j + 1) * per_bin, len(ms))]
        for b in range(n_bands):
            bp = [min(1 << 30, sum(v for k, v in enumerate(row) if int(bin_band[k]) == b)) for row in frames]
            peak = min(32767, math.isqrt(2 * max(bp)))
            out[b, j] = (sum(bp), 0, -peak, peak, len(frames), 0)
    return out


def some_map(nb, k, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, k + 2, nb).astype(np.uint32)           # (k and k + 1: no band)
    m[rng.random(nb) < 0.1] = WILD
    return m


@pytest.mark.parametrize("n_fft, hop", [(64, 16), (128, 133), (256, 256)])
def test_the_reference_is_the_plain_loop(n_fft, hop):
    x = noise(n_fft + 22 * hop + 5, n_fft)
    ms = S.power(x, n_fft, hop)
    assert ms.shape[0] == 23
    for per_bin in (1, 3, 7, 23, 24, 0x7FFFFFFF):
        for k in (1, 8, S.n_bins(n_fft)):
            m = some_map(S.n_bins(n_fft), k, per_bin % 97 + k)
            assert np.array_equal(SL.fold_rows(ms, per_bin, m, k), plain(ms, per_bin, m, k)), (per_bin, k)
            assert np.array_equal(SL.levels_of(x, n_fft, hop, per_bin, m, k), SL.fold_rows(ms, per_bin, m, k))


def test_one_frame_per_bin_and_a_band_per_bin_give_the_power_words():
    x = noise(64 + 9 * 48, 5)
    ms = S.power(x, 64, 48)
    lv = SL.levels_of(x, 64, 48, 1, np.arange(33), 33)
    assert np.array_equal(lv["sum_sq"].T, ms) and (lv["n"] == 1).all() and not lv["sum"].any() and not lv["reserved"].any()
    assert np.array_equal(lv["max"], np.minimum(SL.isqrt(2 * ms.T.astype(np.int64)), 32767)) and np.array_equal(lv["min"], -lv["max"])


def test_time_bins_of_0_1_m_minus_1_m_and_m_plus_1_frames():
    n_fft, hop, per_bin = 64, 10, 5
    m = np.zeros(33, dtype=np.uint32)
    for frames, bins, last in ((0, 0, None), (1, 1, 1), (per_bin - 1, 1, 4), (per_bin, 1, 5), (per_bin + 1, 2, 1)):
        ln = n_fft - 1 if frames == 0 else n_fft + (frames - 1) * hop + 3
        assert S.n_rows(ln, n_fft, hop) == frames and SL.n_bins_of(frames, per_bin) == bins
        lv = SL.levels_of(noise(ln, frames), n_fft, hop, per_bin, m, 1)
        assert lv.shape == (1, bins)
        if bins:
            assert lv["n"][0, -1] == last and (lv["n"][0, :-1] == per_bin).all()


def test_the_per_frame_clamp_is_reached():
    """rows of 32767 against a table of all (32767, 0), one band over all bins: every bin alone is at 2^30, the unclamped band
    sum is far above it, and the record holds 2^30 * n"""
    n_fft, hop, per_bin = 64, 64, 3
    tab = np.zeros((S.PAIRS, 2), dtype=np.int16)
    tab[:, 0] = 32767
    x = np.full(n_fft * 7, 32767, dtype=np.int16)
    ms = S.power(x, n_fft, hop, tab)
    assert ms.shape == (7, 33) and int(ms[0].astype(np.int64).sum()) > 1 << 30
    lv = SL.levels_of(x, n_fft, hop, per_bin, np.zeros(33, dtype=np.uint32), 1, tab)
    assert lv["n"][0].tolist() == [3, 3, 1] and lv["sum_sq"][0].tolist() == [3 << 30, 3 << 30, 1 << 30]
    assert (lv["max"] == 32767).all() and (lv["min"] == -32767).all()
    # sum_sq / n <= 2^30: the x3_level invariant the clamp is there for
    assert (lv["sum_sq"] // lv["n"] <= 1 << 30).all()


def test_a_band_with_no_bin_and_words_that_name_no_band():
    x = noise(64 * 4, 8)
    m = np.full(33, WILD, dtype=np.uint32)
    m[3], m[4], m[9] = 0, 2, 2                                 # band 1 has no bin; 30 bins are in no band
    lv = SL.levels_of(x, 64, 64, 2, m, 3)
    ms = S.power(x, 64, 64).astype(np.int64)
    assert lv.shape == (3, 2) and not lv["sum_sq"][1].any() and (lv["max"][1] == 0).all() and (lv["min"][1] == 0).all()
    assert (lv["n"] == 2).all()                                # an empty band still counts its frames
    assert lv["sum_sq"][0].tolist() == [int(ms[0:2, 3].sum()), int(ms[2:4, 3].sum())]
    assert lv["sum_sq"][2].tolist() == [int(ms[0:2, [4, 9]].sum()), int(ms[2:4, [4, 9]].sum())]
    every = SL.levels_of(x, 64, 64, 2, np.full(33, WILD, dtype=np.uint32), 1)
    assert not every["sum_sq"].any() and (every["n"] == 2).all()


def test_layouts_and_statuses_follow_the_rows_calls_rules():
    """the statuses, the row offsets and the total are spectra_ref.spectra_rows' on the same arguments when M = 1, and its
    rules with T(w) for R(w) otherwise; the records the call owns that hold no frame are the identity, the others keep the
    fill"""
    n_fft, hop = 64, 48
    lens = [64 + 2 * 48 + 3, 64 + 48, 63, 64 + 4 * 48, 64, 64 + 3 * 48 + 47]       # frames 3, 2, 0, 5, 1, 4
    offsets = np.concatenate([[1], 1 + np.cumsum(np.array(lens) + 1)])[:-1].tolist()
    x = noise(offsets[-1] + lens[-1] + 4, 11)
    m = some_map(33, 4, 1)
    ident = SL.IDENTITY
    for ins in (None, [0, 14, 0, 21, 0, 0]):
        for stride, cap in ((0, 15), (0, 14), (0, 4), (5, 31), (4, 24)):
            rows = S.spectra_rows(x, offsets, lens, ins, n_fft, hop, S.POWER, stride, cap)
            lv, off, st, total = SL.spectra_levels(x, offsets, lens, ins, n_fft, hop, 1, m, 4, stride, cap)
            assert np.array_equal(off, rows[1]) and np.array_equal(st, rows[2]) and total == rows[3]
    per_bin = 2
    bins = [2, 1, 0, 3, 1, 2]
    lv, off, st, total = SL.spectra_levels(x, offsets, lens, [0, 14, 0, 0, 0, 0], n_fft, hop, per_bin, m, 4, 0, 7, plane_stride=10)
    assert total == 9 and off.tolist() == [0, 2, 3, 3, 6, 7, 9] and st.tolist() == [0, 14, 0, 0, 0, S.ERR_BAD_ARG]
    assert lv.shape == (4, 10) and (lv[:, 7:].view(np.uint8) == 0x5A).all()        # between rows_cap and plane_stride: never touched
    assert (lv[:, 2] == ident).all()                                               # a range with a status
    assert np.array_equal(lv[:, 0:2], SL.levels_of(x[offsets[0]:offsets[0] + lens[0]], n_fft, hop, per_bin, m, 4))
    lv, off, st, total = SL.spectra_levels(x, offsets, lens, None, n_fft, hop, per_bin, m, 4, 0, 8)
    assert st.tolist() == [0, 0, 0, 0, 0, S.ERR_BAD_ARG] and (lv[:, 7] == ident).all()   # below rows_cap: the call's, no room for the range
    lv, off, st, total = SL.spectra_levels(x, offsets, lens, None, n_fft, hop, per_bin, m, 4, 2, 13)
    assert off.tolist() == [0, 2, 4, 6, 8, 10, 12] and st.tolist() == [0, 0, 0, S.ERR_BAD_ARG, 0, 0]
    assert (lv[:, 3] == ident).all() and (lv[:, 4:8] == ident).all() and (lv[:, 12:13].view(np.uint8) == 0x5A).all()
    wild = list(offsets)
    wild[1] = 2 ** 63
    assert SL.spectra_levels(x, wild, lens, None, n_fft, hop, per_bin, m, 4, 0, 9)[2].tolist() == [0, S.ERR_BAD_ARG, 0, 0, 0, 0]
    for bad in (dict(per_bin=0), dict(per_bin=1 << 31), dict(n_bands=0), dict(n_bands=34), dict(plane_stride=8), dict(rows_cap=0)):
        a = dict(per_bin=2, n_bands=4, plane_stride=0, rows_cap=9)
        a.update(bad)
        with pytest.raises(ValueError):
            SL.spectra_levels(x, offsets, lens, None, n_fft, hop, a["per_bin"], m, a["n_bands"], 0, a["rows_cap"], a["plane_stride"])
    with pytest.raises(ValueError):
        SL.spectra_levels(x, offsets, lens, None, n_fft, hop, 1, np.arange(33), 33, 0, (0x7FFFFFFF // 33) + 1)
