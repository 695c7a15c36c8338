"""tests/events_ref.py, the serial definition the GPU events tests compare with, against hand-worked literal lists
(include/x3hip.h, "EVENTS").  Bins are 10 positions; '#' is a loud bin, '.' a quiet one, '0' a bin nothing was counted in."""
import numpy as np

import events_ref as E
from levels_ref import LEVEL_DTYPE, empty

BL = 10
PEAK = E.Rule(peak_min=100)


def rows(pattern):
    out = empty(len(pattern))
    for i, ch in enumerate(pattern):
        if ch == "#":
            out[i] = (1_000_000 + i, 10 + i, -5, 1000 + i, 10, 0)
        elif ch == ".":
            out[i] = (90, -2, -3 - i, 3, 10, 0)
    return out


def stream(pattern, rule, total=None):
    ev, lv = E.stream_events(rows(pattern), BL * len(pattern) if total is None else total, BL, rule)
    assert len(lv) == len(ev) and lv.dtype == LEVEL_DTYPE
    return ev


def test_gaps_of_join_bins_and_one_more():
    assert stream("#..#...#", PEAK._replace(join_bins=2)) == [(0, 40), (70, 10)]
    assert stream("#..#...#", PEAK._replace(join_bins=3)) == [(0, 80)]
    assert stream("#..#...#", PEAK._replace(join_bins=1)) == [(0, 10), (30, 10), (70, 10)]
    assert stream("##.#", PEAK) == [(0, 20), (30, 10)]
    assert stream("....", PEAK) == [] and stream("####", PEAK) == [(0, 40)]


def test_runs_at_the_first_and_last_row():
    assert stream("#....#", PEAK) == [(0, 10), (50, 10)]
    assert stream("#....#", PEAK._replace(join_bins=4)) == [(0, 60)]


def test_padding_is_clipped_at_both_ends():
    assert stream("#.....#", PEAK._replace(join_bins=4, pad_bins=2)) == [(0, 30), (40, 30)]
    assert stream("...#...", PEAK._replace(join_bins=4, pad_bins=2)) == [(10, 50)]
    # two padded runs keep a cold bin between them: gap 5 > join 4 >= 2 * pad
    assert stream(".#.....#.", PEAK._replace(join_bins=4, pad_bins=2)) == [(0, 40), (50, 40)]


def test_last_partial_bin_clips_len_to_the_samples():
    assert stream("......#", PEAK, total=65) == [(60, 5)]
    assert stream("......#", PEAK._replace(pad_bins=0, max_bins=1), total=61) == [(60, 1)]
    # fewer samples than rows given: the rows behind ceil(total / bin_len) do not count
    assert stream("#.....#", PEAK, total=60) == [(0, 10)]
    # more samples than rows given: the rows given count
    assert stream("#.....#", PEAK, total=1000) == [(0, 10), (60, 10)]


def test_min_bins_drops_before_padding():
    r = PEAK._replace(join_bins=2, pad_bins=1, min_bins=2)
    assert stream("..#..", r) == []                     # (padded it would span three bins)
    assert stream("..##..", r) == [(10, 40)]
    assert stream("..#.#..", r) == [(10, 50)]           # first hot .. last hot spans three
    # a dropped run does not exist: it neither joins nor blocks its neighbours
    assert stream("##...#...##", r) == [(0, 30), (80, 30)]


def test_cuts_at_max_bins():
    assert stream("######", PEAK._replace(max_bins=2)) == [(0, 20), (20, 20), (40, 20)]
    assert stream("######", PEAK._replace(max_bins=4)) == [(0, 40), (40, 20)]
    assert stream("######", PEAK._replace(max_bins=4), total=57) == [(0, 40), (40, 17)]
    assert stream("######", PEAK._replace(max_bins=1), total=57) == [(0, 10), (10, 10), (20, 10), (30, 10), (40, 10), (50, 7)]
    assert stream("######", PEAK._replace(max_bins=6)) == [(0, 60)] == stream("######", PEAK._replace(max_bins=7))


def test_entries_do_not_join_and_an_entry_of_one_row():
    lv = rows("#" + "#.#" + "#" + "..")
    ev, _ = E.corpus_events(lv, [5, 30, 10, 12], BL, PEAK._replace(join_bins=1))
    assert ev == [(0, 0, 5), (1, 0, 30), (2, 0, 10)]
    ev, _ = E.corpus_events(lv, [5, 30, 10, 12], BL, PEAK)
    assert ev == [(0, 0, 5), (1, 0, 10), (1, 20, 10), (2, 0, 10)]
    # an entry without samples has one row, which nothing is counted in
    ev, _ = E.corpus_events(rows("0#"), [0, 7], BL, PEAK)
    assert ev == [(1, 0, 7)]
    # rows clipped to those given
    ev, _ = E.corpus_events(rows("#.#"), [30, 30], BL, PEAK)
    assert ev == [(0, 0, 10), (0, 20, 10)]


def test_empty_bins_inside_a_run_and_the_merged_record():
    assert stream("#0#", PEAK._replace(join_bins=1)) == [(0, 30)]
    assert stream("#0#", PEAK) == [(0, 10), (20, 10)]
    ev, lv = E.stream_events(rows(".#0#."), 50, BL, PEAK._replace(join_bins=2, pad_bins=1))
    assert ev == [(0, 50)]
    assert lv[0].tolist() == (90 + 1_000_001 + 1_000_003 + 90, -2 + 11 + 13 - 2, -7, 1003, 40, 0)
    ev, lv = E.stream_events(rows(".#0#."), 50, BL, PEAK._replace(join_bins=2, pad_bins=1, max_bins=2))
    assert ev == [(0, 20), (20, 20), (40, 10)]
    assert [r.tolist() for r in lv] == [(90 + 1_000_001, 9, -5, 1001, 20, 0), (1_000_003, 13, -5, 1003, 10, 0),
                                        (90, -2, -7, 3, 10, 0)]
    # a bin with n == 0 is never hot, whatever its other fields say
    odd = rows("#")
    odd["n"] = 0
    assert E.stream_events(odd, 10, BL, PEAK)[0] == []
    # n counts modulo 2^32
    big = rows("##")
    big["n"] = 0x80000000
    assert int(E.stream_events(big, 20, BL, PEAK)[1][0]["n"]) == 0


def test_mean_square_at_equality_and_either_criterion():
    lv = empty(3)
    lv[0] = (1000, 0, -9, 9, 10, 0)     # sum_sq == 100 * n
    lv[1] = (999, 0, -9, 9, 10, 0)
    lv[2] = (10, 0, -200, 9, 10, 0)     # quiet on average, a peak of 200 on the negative side
    assert E.stream_events(lv, 30, BL, E.Rule(mean_sq_min=100))[0] == [(0, 10)]
    assert E.stream_events(lv, 30, BL, E.Rule(mean_sq_min=101))[0] == []
    assert E.stream_events(lv, 30, BL, E.Rule(peak_min=200))[0] == [(20, 10)]
    assert E.stream_events(lv, 30, BL, E.Rule(peak_min=201))[0] == []
    assert E.stream_events(lv, 30, BL, E.Rule(mean_sq_min=100, peak_min=200))[0] == [(0, 10), (20, 10)]


def test_slots_hold_the_first_events_and_the_filler():
    ev, lv = E.corpus_events(rows("#.#" + "#"), [30, 4], BL, PEAK)
    ent, st, ln, sl = E.slots(ev, lv, 5, True)
    assert ent.tolist() == [0, 0, 1, 0, 0] and st.tolist() == [0, 20, 0, 0, 0] and ln.tolist() == [10, 10, 4, 0, 0]
    assert sl[3].tolist() == (0, 0, 32767, -32768, 0, 0) == sl[4].tolist() and sl[2].tolist() == lv[2].tolist()
    ent, st, ln, sl = E.slots(ev, lv, 2, True)
    assert ent.tolist() == [0, 0] and st.tolist() == [0, 20] and np.array_equal(sl, lv[:2])
