"""tone_bank_range_levels_ref (the definition of x3_tone_bank_range_levels_dev and its corpus form): the bank is one tone-range
call per step, plane by plane.  The properties that follow from that on tiny streams (57 samples in frames of 10), and
DESIGN.md section 27's example.  No GPU."""
import numpy as np
import pytest

import range_levels_ref as R
import tone_bank_levels_ref as B
import tone_bank_range_levels_ref as BR
import tone_levels_ref as TL
import tone_range_levels_ref as TR

ODD = 2_718_281_829
POOL = [0, 350_898_828, 1 << 31, (1 << 32) - 1, 1 << 22, ODD, 1, 1 << 30]
N = 57
BAD = TR.ERR_BAD_ARG


def _stream(n=N, seed=1, bad=()):
    """-> (frames as (status, samples), sample offsets, the samples)"""
    x = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)
    frames = [((13 + f if f in bad else 0), x[a:a + 10]) for f, a in enumerate(range(0, n, 10))]
    return frames, R.sample_offsets([len(w) for _, w in frames]), x


STARTS = [0, 1, 9, 10, 11, 30, 56, 57, 20, 0, 58]
LENS = [57, 1, 2, 10, 40, 0, 1, 0, 37, 58, 0]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_every_plane_is_the_single_definition(k):
    frames, so, _ = _stream(seed=k, bad=(2,) if k % 2 else ())
    tab = np.random.default_rng(k).integers(-32768, 32768, (1024, 2)).astype(np.int16) if k % 2 else None
    steps = POOL[:k]
    for bin_len in (0, 1, 7, 20, 21):
        rows = sum(TR.rows_of(v, bin_len) for v in LENS)
        for stride, cap in ((0, rows), (0, rows + 3), (3, 3 * len(LENS) + 2)):
            got, off, st = BR.range_levels(frames, so, STARTS, LENS, bin_len, stride, cap, steps, tab)
            assert got.shape == (k, cap, 32) and got.dtype == np.uint8
            for t, step in enumerate(steps):
                one, off1, st1 = TR.range_levels(frames, so, STARTS, LENS, bin_len, stride, cap, step, tab)
                assert got[t].tobytes() == one.tobytes() and np.array_equal(off, off1) and np.array_equal(st, st1)
                for f in ("min", "max", "n", "reserved"):                # the samples' fields are the same in every plane
                    assert np.array_equal(TR.view(got[t])[f], TR.view(got[0])[f])
            assert (st == BAD).any() and (st == 0).any()
            if k % 2 and not stride:
                assert (st == 15).any()                                  # the failed frame's status, whatever the bank


def test_a_plane_does_not_depend_on_the_other_steps_and_a_permutation_permutes_the_planes():
    frames, so, _ = _stream(seed=3)
    a = BR.range_levels(frames, so, STARTS, LENS, 7, 0, 40, [ODD, 1, 1 << 31, 5])[0]
    b = BR.range_levels(frames, so, STARTS, LENS, 7, 0, 40, [77, 1, 0, 9, 1 << 30])[0]
    assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() != b[0].tobytes()
    perm = [3, 0, 2, 1]
    c = BR.range_levels(frames, so, STARTS, LENS, 7, 0, 40, [[ODD, 1, 1 << 31, 5][i] for i in perm])[0]
    assert c.tobytes() == a[perm].tobytes()
    d = BR.range_levels(frames, so, STARTS, LENS, 7, 0, 40, [ODD, 5, ODD])[0]      # equal steps give equal planes
    assert d[0].tobytes() == d[2].tobytes() == a[0].tobytes() and d[1].tobytes() == a[3].tobytes()
    for bad in ([], list(range(9))):
        with pytest.raises(AssertionError):
            BR.range_levels(frames, so, STARTS, LENS, 7, 0, 40, bad)
    with pytest.raises(ValueError):
        BR.range_levels(frames, so, [], [], 7, 0, 4, [1, 2])


def test_ranges_without_room_are_untouched_in_every_plane():
    frames, so, _ = _stream(seed=4)
    steps = [ODD, 0, 1 << 31]
    rows = [TR.rows_of(v, 7) for v in LENS]
    cap = sum(rows) - 4                                                   # packed: the last ranges have no room
    got, off, st = BR.range_levels(frames, so, STARTS, LENS, 7, 0, cap, steps)
    full = BR.range_levels(frames, so, STARTS, LENS, 7, 0, sum(rows), steps)[0]
    fits = [int(off[w]) + rows[w] <= cap for w in range(len(LENS))]
    assert not all(fits) and any(fits)
    for t in range(3):
        for w in range(len(LENS)):
            a, b = int(off[w]), min(int(off[w]) + rows[w], cap)
            if fits[w]:
                assert got[t, a:b].tobytes() == full[t, a:b].tobytes()
            else:
                assert st[w] == BAD and (got[t, a:b] == 0x5A).all()
    # padded: the ranges longer than the stride are refused, the records behind n * stride are nobody's
    got, off, st = BR.range_levels(frames, so, STARTS, LENS, 7, 2, 2 * len(LENS) + 3, steps)
    for t in range(3):
        assert (got[t, 2 * len(LENS):] == 0x5A).all()
        for w in range(len(LENS)):
            mine = TR.view(got[t, 2 * w:2 * w + 2])
            if rows[w] > 2:
                assert st[w] == BAD and mine.tobytes() == TL.empty(2).tobytes()      # (the padded layout's identities)
            elif st[w] == 0:
                assert int(mine["n"].sum()) == LENS[w]
    assert got[0].tobytes() != got[1].tobytes()


def test_a_corpus_entry_starts_at_phase_0_in_every_plane():
    """an entry is a stream of its own: the same samples as two entries give the same planes, and the same samples further
    along ONE stream do not (the oscillators are not restarted at a range)"""
    x = np.random.default_rng(5).integers(-3000, 3000, 25).astype(np.int16)
    entry = [(0, x[:10]), (0, x[10:20]), (0, x[20:])]
    twice = entry + entry                                                 # one stream that holds the samples twice
    so1, so2 = R.sample_offsets([10, 10, 5]), R.sample_offsets([10, 10, 5] * 2)
    steps = [12_345_678, ODD, 12_345_678]
    a = BR.range_levels(entry, so1, [3], [20], 7, 0, 3, steps)[0]
    again = BR.range_levels(entry, so1, [3], [20], 7, 0, 3, steps)[0]    # the repeated entry
    later = BR.range_levels(twice, so2, [28], [20], 7, 0, 3, steps)[0]   # the same samples at positions 28 .. 47
    assert a.tobytes() == again.tobytes() and a[0].tobytes() == a[2].tobytes()
    for t in range(3):
        ra, rl = TR.view(a[t]), TR.view(later[t])
        for f in ("min", "max", "n"):
            assert np.array_equal(ra[f], rl[f])
        assert not np.array_equal(ra["re"], rl["re"])
    one, st = BR.one(entry, so1, 3, 20, 7, steps, TL.table())
    assert st == 0 and one.tobytes() == TR.view(a.reshape(-1, 32)).tobytes()


@pytest.mark.parametrize("bin_len", [0, 1, 7, 20, 21])
def test_the_whole_stream_equals_tone_bank_levels_ref(bin_len):
    for bad in ((), (0,), (3,), (5,)):
        frames, so, _ = _stream(seed=6, bad=bad)
        steps = POOL[:5]
        rows = TR.rows_of(N, bin_len)
        got, off, st = BR.range_levels(frames, so, [0], [N], bin_len, 0, rows, steps)
        want = B.tone_bank_levels([w if s == 0 else [] for s, w in frames], [s for s, _ in frames], so[:-1], bin_len, rows, steps)
        assert TR.view(got.reshape(-1, 32)).tobytes() == want.tobytes()
        assert st.tolist() == [13 + bad[0] if bad else 0]


EXAMPLE_RANGES = ([4_300, 11_900], [400, 400])          # section 26's two events, (4 400, 200) and (12 000, 200), padded by 100
EXAMPLE_BAND_MS = [                                     # [range][plane]: floor(sum_sq / n) of the four bins of 100
    [[10_465, 435_861, 920_106, 40_515], [14_975, 30_720, 23_159, 15_000], [23_820, 6_912, 119_925, 25_268],
     [42_650, 34_087, 45_468, 142_374]],
    [[84_708, 3_029, 47_439, 162_185], [235_688, 736_654, 343_400, 144_735], [35_304, 5_321, 52_827, 44_779],
     [484, 121_302, 19_092, 79_098]],
]


def example_band_ms(records):
    """uint8 [4, 8, 32] band records (LEVEL_DTYPE bytes) -> [range][plane] lists of floor(sum_sq / n)"""
    band = R.view(np.ascontiguousarray(records).reshape(-1, 32)).reshape(4, 8)
    ms = (band["sum_sq"] // band["n"]).astype(np.int64)
    return [[ms[t, 4 * w:4 * w + 4].tolist() for t in range(4)] for w in range(2)]


def test_the_example_two_events_looked_at_again_in_four_bands():
    """section 26's signal and bank; the two events found there, padded by 100 positions either side, at
    bins of 100.  435 861 and 920 106 are section 25's figures for the first burst in its own band."""
    w = B.example()
    frames, so = [(0, w[a:a + 2_000]) for a in range(0, 20_000, 2_000)], R.sample_offsets([2_000] * 10)
    starts, lens = EXAMPLE_RANGES
    rec, off, st = BR.range_levels(frames, so, starts, lens, 100, 0, 8, B.EXAMPLE_STEPS)
    assert off.tolist() == [0, 4, 8] and not st.any() and rec.shape == (4, 8, 32)
    band = np.stack([TL.tone_power_levels(TR.view(rec[t])) for t in range(4)])
    ms = example_band_ms(band.view(np.uint8).reshape(4, 8, 32))
    assert ms == EXAMPLE_BAND_MS
    loud = [(w_, t, r) for w_ in range(2) for t in range(4) for r in range(4) if ms[w_][t][r] >= 300_000]
    assert loud == [(0, 0, 1), (0, 0, 2), (1, 1, 1), (1, 1, 2)]
