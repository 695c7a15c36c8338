"""spectra_ref.py (the definition of x3_spectra_rows_dev) against plain arithmetic, the kernels' 8-bit split against the
definition, and the identities include/x3hip.h states.  No GPU."""
import numpy as np
import pytest

import range_levels_ref as R
import spectra_ref as S
import tone_levels_ref as TL
import tone_range_levels_ref as TR

EXTREMES = [-32768, 32767, -129, -128, -1, 0, 127, 128, 255, 256]


def extreme_table(seed=2):
    rng = np.random.default_rng(seed)
    t = rng.choice(np.array(EXTREMES, dtype=np.int16), (S.PAIRS, 2))
    t[::7] = rng.integers(-32768, 32768, t[::7].shape)
    return t


def test_the_definition_against_a_plain_int64_matmul_and_a_loop():
    rng = np.random.default_rng(1)
    tab = TL.table()
    for n_fft, hop in ((64, 17), (128, 128), (1024, 300)):
        x = rng.integers(-32768, 32768, n_fft + 2 * hop + 5).astype(np.int16)
        got = S.sums(x, n_fft, hop)
        assert got.dtype == np.int64 and got.shape == (3, n_fft // 2 + 1, 2)
        n, k = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None, :]
        idx = ((n * k) % n_fft) * (1024 // n_fft)
        for r in range(3):
            fr = x[r * hop:r * hop + n_fft].astype(np.int64)
            assert np.array_equal(got[r, :, 0], fr @ tab[idx, 0].astype(np.int64))
            assert np.array_equal(got[r, :, 1], fr @ tab[idx, 1].astype(np.int64))
        # Python integers, one bin
        k1 = n_fft // 2 - 1
        want = sum(int(x[hop + i]) * int(tab[((i * k1) % n_fft) * (1024 // n_fft), 1]) for i in range(n_fft))
        assert int(got[1, k1, 1]) == want


@pytest.mark.parametrize("n_fft", [64, 256, 1024])
def test_the_8_bit_split_and_epilogue_equal_the_definition_at_the_extremes(n_fft):
    rng = np.random.default_rng(n_fft)
    tab = extreme_table()
    rows = [np.full(2 * n_fft, -32768), np.full(2 * n_fft, 32767), np.resize(np.array(EXTREMES), 2 * n_fft),
            rng.choice(np.array(EXTREMES), 2 * n_fft), rng.integers(-32768, 32768, 2 * n_fft)]
    for t in (tab, None, np.full((S.PAIRS, 2), -32768, dtype=np.int16), np.full((S.PAIRS, 2), 32767, dtype=np.int16)):
        for x in rows:
            x = x.astype(np.int16)
            assert np.array_equal(S.split_model(x, n_fft, n_fft // 2, t), S.sums(x, n_fft, n_fft // 2, t))
    hi, lo = S.split(np.array([-32768, 32767, -129, -128, -1, 0, 127, 128, 255, 256]))
    assert hi.tolist() == [-128, 127, -1, -1, -1, 0, 0, 0, 0, 1] and lo.tolist() == [-128, 127, -1, 0, 127, -128, -1, 0, 127, -128]
    assert abs(int(S.sums(np.full(n_fft, -32768, dtype=np.int16), n_fft, 1, np.full((S.PAIRS, 2), -32768, dtype=np.int16))[0, 0, 0])) == n_fft << 30


@pytest.mark.parametrize("n_fft", [64, 256, 1024])
def test_the_phase_identity(n_fft):
    """position i = 5 N + n of a stream under step = k * 2^32 / N has the pair ((n * k) mod N) * (1024 / N)"""
    n = np.arange(n_fft, dtype=np.int64)
    for k in (0, 1, 3, n_fft // 2 - 1, n_fft // 2):
        step = k * (2 ** 32 // n_fft)
        assert np.array_equal(TL.pair_index(5 * n_fft + n, step).astype(np.int64), ((n * k) % n_fft) * (1024 // n_fft))


def test_aligned_frames_equal_the_tone_range_levels_and_the_tone_power():
    rng = np.random.default_rng(4)
    n_fft, spf = 128, 400
    x = rng.integers(-20000, 20000, 2000).astype(np.int16)
    frames = [(0, x[a:a + spf]) for a in range(0, x.size, spf)]
    so = R.sample_offsets([spf] * (x.size // spf))
    p0 = 3 * n_fft
    got = S.sums(x[p0:p0 + 2 * n_fft], n_fft, n_fft)
    pw = S.power(x[p0:p0 + 2 * n_fft], n_fft, n_fft)
    for k in (0, 1, 17, 63, 64):
        rec, st = TR.one(frames, so, p0, 2 * n_fft, n_fft, k * (2 ** 32 // n_fft), TL.table())
        assert st == 0 and np.array_equal(rec["re"], got[:, k, 0]) and np.array_equal(rec["im"], got[:, k, 1])
        lev = TL.tone_power_levels(rec)
        assert np.array_equal(lev["sum_sq"] // lev["n"], pw[:, k].astype(np.uint64))


def test_a_table_of_ones_gives_the_frames_sums():
    x = np.random.default_rng(6).integers(-32768, 32768, 700).astype(np.int16)
    t = np.zeros((S.PAIRS, 2), dtype=np.int16)
    t[:, 0] = 1
    got = S.sums(x, 256, 100, t)
    assert got.shape[0] == 5 and not got[:, :, 1].any()
    for r in range(5):
        assert (got[r, :, 0] == int(x[100 * r:100 * r + 256].astype(np.int64).sum())).all()


def test_power_saturates_and_shifts_arithmetically():
    s = np.array([[-1, 0], [-(1 << 15), 1 << 15], [64 << 30, 0], [-(64 << 30), 64 << 30]], dtype=np.int64)
    assert S.power_of(s, 64).tolist() == [0, 0, 1 << 30, 1 << 30]     # -1 >> 15 == -1: 2 * 1 // 64 == 0
    assert S.power_of(np.array([[100 << 15, -(50 << 15)]], dtype=np.int64), 64).tolist() == [(2 * (100 * 100 + 50 * 50) // 64) // 64]


@pytest.mark.parametrize("n_fft, hop", [(64, 1), (64, 48), (256, 300), (1024, 1024)])
def test_rows_of_lengths_around_a_frame(n_fft, hop):
    lens = [0, n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop]
    assert [S.n_rows(v, n_fft, hop) for v in lens] == [0, 0, 1, 1, 2]
    x = np.arange(n_fft + hop, dtype=np.int16)
    for v in lens:
        assert S.sums(x[:v], n_fft, hop).shape[0] == S.n_rows(v, n_fft, hop)


def test_layouts_and_statuses():
    n_fft, hop = 64, 32
    x = np.random.default_rng(8).integers(-32768, 32768, 1000).astype(np.int16)
    offsets, lens = [1, 200, 400, 2 ** 63, 900], [64 + 32 * 2, 63, 64 + 32 * 4 + 5, 64, 101]      # rows 3, 0, 5, 1, 2
    out, off, st, total = S.spectra_rows(x, offsets, lens, None, n_fft, hop, S.SUMS, 0, 11)
    assert total == 11 and off.tolist() == [0, 3, 3, 8, 9, 11] and st.tolist() == [0, 0, 0, 24, 24]
    assert np.array_equal(out[0:3], S.sums(x[1:1 + lens[0]], n_fft, hop)) and np.array_equal(out[3:8], S.sums(x[400:400 + lens[2]], n_fft, hop))
    assert not out[8:11].any()                                 # the wild offset and the range past samples_cap: zeros
    out, off, st, total = S.spectra_rows(x, offsets, lens, [0, 7, 14, 0, 0], n_fft, hop, S.POWER, 0, 8)
    assert st.tolist() == [0, 7, 14, 24, 24] and total == 11 and not out[3:8].any()
    assert (out[8:].view(np.uint8) == 0x5A).all() if out.shape[0] > 8 else True
    out, off, st, total = S.spectra_rows(x, offsets[:3], lens[:3], None, n_fft, hop, S.POWER, 0, 7)
    assert st.tolist() == [0, 0, 24] and off.tolist() == [0, 3, 3, 8] and (out[3:].view(np.uint8) == 0x5A).all()
    out, off, st, total = S.spectra_rows(x, offsets[:3], lens[:3], None, n_fft, hop, S.POWER, 4, 13)
    assert st.tolist() == [0, 0, 24] and off.tolist() == [0, 4, 8, 12] and not out[3:12].any() and (out[12:].view(np.uint8) == 0x5A).all()
    assert np.array_equal(out[0:3], S.power(x[1:1 + lens[0]], n_fft, hop))
    for bad in (dict(n_fft=96), dict(hop=0), dict(fmt=2), dict(stride=5, rows_cap=14), dict(rows_cap=0)):
        a = dict(n_fft=n_fft, hop=hop, fmt=S.SUMS, stride=0, rows_cap=11)
        a.update(bad)
        with pytest.raises(ValueError):
            S.spectra_rows(x, offsets[:3], lens[:3], None, a["n_fft"], a["hop"], a["fmt"], a["stride"], a["rows_cap"])
