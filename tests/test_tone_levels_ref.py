"""tone_levels_ref (the definition of x3_tone_levels_dev and x3_tone_power_levels_dev) against an independent formulation:
Python big integers, position by position.  No GPU."""
import math

import numpy as np
import pytest

import levels_ref as LR
import tone_levels_ref as TR

STEPS = [0, 1, 1 << 30, 1 << 31, (1 << 32) - 1]


def slow_tone_levels(x, bin_len, n_bins, step, tab, first=0):
    """x at positions first .. : (re, im, min, max, n) per bin in Python integers"""
    out = [[0, 0, 32767, -32768, 0] for _ in range(n_bins)]
    for i, v in enumerate(x):
        pos = first + i
        b = pos // bin_len if bin_len else 0
        if b >= n_bins:
            continue
        k = ((pos * step) % (1 << 32)) >> 22
        r = out[b]
        r[0] += int(v) * int(tab[k][0])
        r[1] += int(v) * int(tab[k][1])
        r[2], r[3], r[4] = min(r[2], int(v)), max(r[3], int(v)), r[4] + 1
    return out


def as_lists(rec):
    return [[int(r["re"]), int(r["im"]), int(r["min"]), int(r["max"]), int(r["n"])] for r in rec]


def test_usual_table():
    t = TR.table()
    assert t.shape == (1024, 2) and t.dtype == np.int16
    assert t[0].tolist() == [32767, 0] and t[256].tolist() == [0, 32767] and t[512].tolist() == [-32767, 0]
    assert t[768].tolist() == [0, -32767]
    for k in (1, 100, 511, 1023):
        assert t[k].tolist() == [round(32767 * math.cos(2 * math.pi * k / 1024)), round(32767 * math.sin(2 * math.pi * k / 1024))]


@pytest.mark.parametrize("step", STEPS + [350892751])
@pytest.mark.parametrize("n", [0, 1, 19, 20, 21, 57])
def test_stream_against_big_integers(step, n):
    rng = np.random.default_rng(n * 7 + step % 1000)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    tab = rng.integers(-32768, 32768, (1024, 2)).astype(np.int16) if step % 2 else TR.table()
    # frames of 10 samples, the last one shorter; bins around a bin edge of 20
    frames = [x[a:a + 10] for a in range(0, n, 10)]
    so = list(range(0, n, 10))
    for bin_len in (0, 1, 7, 19, 20, 21):
        nb = LR.n_bins_for(n, bin_len)
        got = TR.tone_levels(frames, [0] * len(frames), so, bin_len, nb, step, tab)
        assert as_lists(got) == slow_tone_levels(x, bin_len, nb, step, tab.tolist()), (step, n, bin_len)
        assert not got["reserved"].any()


def test_failed_frames_add_nothing_and_far_positions_wrap():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, 40).astype(np.int16)
    frames = [x[0:10], x[10:20], x[20:30], x[30:40]]
    tab = TR.table()
    step = (1 << 32) - 1
    got = TR.tone_levels(frames, [0, 2, 0, 0], [0, 10, 20, 30], 20, 2, step)
    want0 = slow_tone_levels(x[0:10], 20, 2, step, tab.tolist())
    want1 = slow_tone_levels(x[20:40], 20, 2, step, tab.tolist(), first=20)
    assert as_lists(got) == [want0[0], want1[1]]
    # positions beyond 2^32: the phase is (i * step) mod 2^32 of the whole position
    base = (1 << 33) + 12345
    got = TR.tone_levels([x], [0], [base], 0, 1, 350892751)
    assert as_lists(got) == slow_tone_levels(x, 0, 1, 350892751, tab.tolist(), first=base)


def test_corpus_restarts_the_phase():
    rng = np.random.default_rng(5)
    a, b = rng.integers(-3000, 3000, 25).astype(np.int16), rng.integers(-3000, 3000, 31).astype(np.int16)
    ents = [([a[:20], a[20:]], [0, 0], [0, 20], 25), ([b[:20], b[20:]], [0, 0], [0, 20], 31)]
    rows, rf = TR.corpus_tone_levels(ents, 10, 12345678)
    assert rf.tolist() == [0, 3, 7]
    tab = TR.table().tolist()
    assert as_lists(rows) == slow_tone_levels(a, 10, 3, 12345678, tab) + slow_tone_levels(b, 10, 4, 12345678, tab)


def test_identities():
    rng = np.random.default_rng(9)
    x = rng.integers(-32768, 32768, 100).astype(np.int16)
    frames, so = [x[:50], x[50:]], [0, 50]
    lv = LR.levels(frames, [0, 0], so, 30, 4)
    ones = np.tile(np.array([[1, 0]], dtype=np.int16), (1024, 1))
    t = TR.tone_levels(frames, [0, 0], so, 30, 4, 987654321, ones)
    assert np.array_equal(t["re"], lv["sum"]) and not t["im"].any()
    for k in ("min", "max", "n"):
        assert np.array_equal(t[k], lv[k])
    t = TR.tone_levels(frames, [0, 0], so, 30, 4, 0)
    assert np.array_equal(t["re"], 32767 * lv["sum"]) and not t["im"].any()


def slow_power(re, im, n):
    """the adapter's record by its definition, written out once more with exact rational comparisons"""
    if n == 0:
        return (0, 0, 32767, -32768, 0)
    e = max(0, len(bin(n)) - 2 - 15)
    a = re // (1 << (15 + e))     # (floor division: the arithmetic shift)
    b = im // (1 << (15 + e))
    P = a * a + b * b
    m = n // (1 << e)
    ms = min(1 << 30, (2 * P // m) // m)
    peak = 0
    while (peak + 1) * (peak + 1) <= 2 * ms and peak < 32767:
        peak += 1
    return (ms * n, 0, -peak, peak, n)


@pytest.mark.parametrize("n", [0, 1, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 32) - 1])
def test_adapter_on_crafted_records(n):
    for sre in (1, -1):
        for sim in (1, -1, 0):
            re, im = sre * n * (1 << 30), sim * n * (1 << 30)
            got, P = TR.power_record(re, im, n)
            assert P < 1 << 62
            if n:   # peak is found by a loop in slow_power: only where it is small enough to walk
                assert got[0] == min(1 << 30, got[0] // n) * n and got[1] == 0 and got[4] == n
                assert got[0] // n <= 1 << 30 and -got[2] == got[3] <= 32767
            assert got == slow_power(re, im, n)
    # through the record form
    rec = np.zeros(1, dtype=TR.TONE_DTYPE)
    rec["re"], rec["im"], rec["n"] = -n * (1 << 30), n * (1 << 30), n
    out = TR.tone_power_levels(rec)
    want = slow_power(-n * (1 << 30), n * (1 << 30), n)
    assert (int(out["sum_sq"][0]), int(out["sum"][0]), int(out["min"][0]), int(out["max"][0]), int(out["n"][0])) == want
    assert int(out["reserved"][0]) == 0


def test_adapter_full_scale_clamps():
    # |re| = |im| = n * 2^30: ms would be 2 * 2^30, and is clamped to 2^30; peak to 32767
    for n in (1, 70000, (1 << 32) - 1):
        got, _ = TR.power_record(n << 30, -(n << 30), n)
        assert got == ((1 << 30) * n, 0, -32767, 32767, n)


SQUARE_ROOTS = [1, 2, 3, 100, 181, 32766, 32767]


def square_edge_records(r):
    """Records whose 2 * ms is r * r - 1, r * r or r * r + 1 -> [(target, re, im, n)].  2 * ms is even, so of the three
    targets the even ones can be reached, and every one of those is:
      even r: r * r, by n = 1 (e = 0, m = 1, ms = 2 * P) with a = r / 2, b = 0, so that 2 * ms = 4 * P = r * r;
      odd r:  n = 2 (e = 0, m = 2, ms = floor(P / 2)): a = r, b = 0 has P = r * r, odd, and 2 * ms = r * r - 1;
              a = r, b = 1 has P = r * r + 1, even, and 2 * ms = r * r + 1.
    |re|, |im| <= n * 2^30 holds (r <= 32767): records a tone call can write."""
    if r % 2 == 0:
        return [(r * r, (r // 2) << 15, 0, 1)]
    return [(r * r - 1, r << 15, 0, 2), (r * r + 1, -(r << 15), 1 << 15, 2)]


@pytest.mark.parametrize("r", SQUARE_ROOTS)
def test_adapter_at_perfect_squares(r):
    """2 * ms at r * r - 1, r * r and r * r + 1: every one of the three that is even, the floor square root on both sides of
    a square and the clamp of the peak at 32767"""
    recs = square_edge_records(r)
    assert sorted(t for t, _, _, _ in recs) == [t for t in (r * r - 1, r * r, r * r + 1) if t % 2 == 0]
    for target, re, im, n in recs:
        got, P = TR.power_record(re, im, n)
        ms = got[0] // n
        assert P < 1 << 62 and got[0] == ms * n and 2 * ms == target and got[1] == 0 and got[4] == n
        want = r if target >= r * r else r - 1             # isqrt(r * r - 1) = r - 1, isqrt(r * r) = isqrt(r * r + 1) = r
        assert got[3] == min(32767, want) == min(32767, TR.isqrt(target)) and got[2] == -got[3]
        assert got == slow_power(re, im, n)
    if r == 32767:                                          # next to the clamp: 32766 below the square, 32767 at and above it
        assert [TR.power_record(re, im, n)[0][3] for _, re, im, n in recs] == [32766, 32767]
    for x in (0, 1, 2, 3, 4, 15, 16, 17, r * r - 1, r * r, r * r + 1, (1 << 31) - 1, 1 << 31):
        s = TR.isqrt(x)
        assert s * s <= x < (s + 1) * (s + 1)


def test_every_even_square_edge_is_reached():
    hit = sum(len(square_edge_records(r)) for r in SQUARE_ROOTS)
    assert hit == sum(1 for r in SQUARE_ROOTS for t in (r * r - 1, r * r, r * r + 1) if t % 2 == 0) == 11


def test_adapter_estimates_a_tone():
    """amplitude A at the oscillator's frequency: ms about A * A / 2, peak about A"""
    A, n, step = 1000, 4000, round(0.0817 * 2 ** 32)
    t = np.arange(n)
    x = np.rint(A * np.sin(2 * np.pi * 0.0817 * t + 0.3)).astype(np.int16)
    rec = TR.tone_levels([x], [0], [0], 0, 1, step)
    out = TR.tone_power_levels(rec)
    ms = int(out["sum_sq"][0]) // n
    assert abs(ms - A * A // 2) < A * A // 2 * 0.02 and abs(int(out["max"][0]) - A) < A * 0.02
