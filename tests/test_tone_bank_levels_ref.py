"""tone_bank_levels_ref (the definition of x3_tone_bank_levels_dev and its corpus form): the bank is one tone call per step,
plane by plane.  The properties that follow from that, and DESIGN.md section 26's example.  No GPU."""
import numpy as np
import pytest

import events_ref as E
import levels_ref as LR
import test_tone_levels_ref as TRT
import tone_bank_levels_ref as B
import tone_levels_ref as TR

ODD = 2_718_281_829
POOL = [0, 1 << 30, 1 << 31, (1 << 32) - 1, ODD, 350_898_828, 1, 12_345_678]


def _stream(n, seed):
    x = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)
    return x, [x[a:a + 10] for a in range(0, n, 10)], list(range(0, n, 10))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_every_plane_is_the_single_call_and_big_integers(k):
    x, frames, so = _stream(57, k)
    tab = np.random.default_rng(k).integers(-32768, 32768, (1024, 2)).astype(np.int16) if k % 2 else None
    steps = POOL[:k]
    for bin_len in (0, 1, 7, 20, 21):
        nb = LR.n_bins_for(57, bin_len) + 1
        got = B.tone_bank_levels(frames, [0] * len(frames), so, bin_len, nb, steps, tab)
        assert got.shape == (k, nb) and got.dtype == B.TONE_DTYPE
        for t, step in enumerate(steps):
            assert got[t].tobytes() == TR.tone_levels(frames, [0] * len(frames), so, bin_len, nb, step, tab).tobytes()
            assert TRT.as_lists(got[t]) == TRT.slow_tone_levels(x, bin_len, nb, step, (TR.table() if tab is None else tab).tolist())
            for f in ("min", "max", "n"):                             # the samples' fields are the same in every plane
                assert np.array_equal(got[t][f], got[0][f])
            assert not got[t]["reserved"].any()
            assert got[t][-1].tobytes() == TR.empty(1).tobytes()      # the bin behind the stream


def test_a_plane_does_not_depend_on_the_other_steps_and_a_permutation_permutes_the_planes():
    _, frames, so = _stream(95, 3)
    ok = [0] * len(frames)
    a = B.tone_bank_levels(frames, ok, so, 7, 14, [ODD, 1, 1 << 31, 5])
    b = B.tone_bank_levels(frames, ok, so, 7, 14, [77, 1, 0, 9, 1 << 30])
    assert a[1].tobytes() == b[1].tobytes() and a[0].tobytes() != b[0].tobytes()
    perm = [3, 0, 2, 1]
    c = B.tone_bank_levels(frames, ok, so, 7, 14, [[ODD, 1, 1 << 31, 5][i] for i in perm])
    assert c.tobytes() == a[perm].tobytes()
    # equal steps give equal planes
    d = B.tone_bank_levels(frames, ok, so, 7, 14, [ODD, 5, ODD])
    assert d[0].tobytes() == d[2].tobytes() == a[0].tobytes() and d[1].tobytes() == a[3].tobytes()
    for bad in ([], list(range(9))):
        with pytest.raises(AssertionError):
            B.tone_bank_levels(frames, ok, so, 7, 14, bad)


def test_a_failed_frame_adds_to_no_plane_and_bins_behind_n_bins_are_dropped():
    x, frames, so = _stream(40, 4)
    got = B.tone_bank_levels(frames, [0, 2, 0, 0], so, 20, 2, [ODD, 0, 1 << 31])
    assert got["n"].tolist() == [[10, 20]] * 3
    step_zero = got[1]
    assert int(step_zero["re"][0]) == 32767 * int(x[:10].astype(np.int64).sum()) and not step_zero["im"].any()
    full = B.tone_bank_levels(frames, [0] * 4, so, 10, 4, [ODD, 3])
    short = B.tone_bank_levels(frames, [0] * 4, so, 10, 3, [ODD, 3])
    assert short.shape == (2, 3) and short.tobytes() == full[:, :3].tobytes()     # nothing spills into the next plane


def test_corpus_planes_restart_the_phase_and_share_row_first():
    rng = np.random.default_rng(5)
    a, b = rng.integers(-3000, 3000, 25).astype(np.int16), rng.integers(-3000, 3000, 31).astype(np.int16)
    ents = [([a[:20], a[20:]], [0, 0], [0, 20], 25), ([], [], [], 0), ([b[:20], b[20:]], [0, 0], [0, 20], 31), ([a[:20], a[20:]], [0, 0], [0, 20], 25)]
    steps = [12_345_678, ODD, 12_345_678]
    rows, rf = B.corpus_tone_bank_levels(ents, 10, steps)
    assert rf.tolist() == [0, 3, 4, 8, 11] and rows.shape == (3, 11)
    for t, step in enumerate(steps):
        one, rf1 = TR.corpus_tone_levels(ents, 10, step)
        assert np.array_equal(rf1, rf) and rows[t].tobytes() == one.tobytes()
        assert rows[t][0:3].tobytes() == rows[t][8:11].tobytes()          # the repeated entry: phase 0 at its start
        assert rows[t][0:3].tobytes() == TR.tone_levels([a[:20], a[20:]], [0, 0], [0, 20], 10, 3, step).tobytes()
        assert rows[t][3].tobytes() == TR.empty(1).tobytes()
    assert rows[0].tobytes() == rows[2].tobytes()


def band_mean_squares(planes):
    out = []
    for p in planes:
        band = TR.tone_power_levels(p)
        out.append((band, (band["sum_sq"] // band["n"]).astype(np.int64)))
    return out


def test_the_example_two_bursts_and_a_bank_of_four():
    """section 24's noise and burst at 0.0817 fs, a second burst at 0.2310 fs, bins of 200 and a bank at
    0.0817 / 0.2310 / 0.15 / 0.41 fs.  mean_sq_min = 400 000 finds each burst in its own plane and nothing in the others."""
    w = B.example()
    for f, s in zip(B.EXAMPLE_FREQS, B.EXAMPLE_STEPS):
        assert round(f * 2 ** 32) == s
    frames, so = [w[a:a + 2_000] for a in range(0, 20_000, 2_000)], range(0, 20_000, 2_000)
    planes = B.tone_bank_levels(frames, [0] * 10, so, 200, 100, B.EXAMPLE_STEPS)
    ms = [m for _, m in band_mean_squares(planes)]
    assert (int(ms[0].argmax()), int(ms[0].max()), int(np.delete(ms[0], 22).max())) == (22, 655_216, 150_707)
    assert (int(ms[1].argmax()), int(ms[1].max()), int(np.delete(ms[1], 60).max())) == (60, 518_188, 138_273)
    assert (int(ms[2].argmax()), int(ms[2].max())) == (19, 322_926)
    assert (int(ms[3].argmax()), int(ms[3].max())) == (34, 150_040)
    rule = E.Rule(mean_sq_min=400_000)
    found = [E.stream_events(band, 20_000, 200, rule)[0] for band, _ in band_mean_squares(planes)]
    assert found == [[(4_400, 200)], [(12_000, 200)], [], []]
