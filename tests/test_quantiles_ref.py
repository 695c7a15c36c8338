"""tests/quantiles_ref.py, the serial definition the GPU quantiles tests compare with, against hand-worked literals
(include/x3hip.h, "LEVEL QUANTILES AND ADAPTIVE THRESHOLDS")."""
import numpy as np

import events_ref as E
import quantiles_ref as Q
from levels_ref import empty

BL = 10


def recs(peaks=(), mean_sqs=(), n=10):
    """records of n samples each with the given peaks (as max) or mean squares (sum_sq = m * n + n - 1: floors to m)"""
    count = max(len(peaks), len(mean_sqs))
    out = empty(count)
    out["n"] = n
    out["min"], out["max"] = -1, 1
    for i, p in enumerate(peaks):
        out["max"][i] = p
    for i, m in enumerate(mean_sqs):
        out["sum_sq"][i] = m * n + n - 1
    return out


def q_stream(lv, key, q_ppm, total=None):
    v, k = Q.stream_quantiles(lv, BL * len(lv) if total is None else total, BL, key, q_ppm)
    assert v.shape == (1, len(q_ppm)) and k.shape == (1,)
    return v[0].tolist(), int(k[0])


def test_k_of_0_1_and_2():
    lv = recs(peaks=[7, 9])
    lv["n"] = 0
    assert q_stream(lv, Q.PEAK, [0, 500_000, 1_000_000]) == ([0, 0, 0], 0)
    lv["n"][1] = 10
    assert q_stream(lv, Q.PEAK, [0, 500_000, 1_000_000]) == ([9, 9, 9], 1)
    lv["n"][0] = 10
    assert q_stream(lv, Q.PEAK, [0, 499_999, 500_000, 999_999, 1_000_000]) == ([7, 7, 7, 7, 9], 2)
    # rows behind ceil(total / bin_len) do not count; a total of 0 leaves none
    assert q_stream(lv, Q.PEAK, [1_000_000], total=10) == ([7], 1)
    assert q_stream(lv, Q.PEAK, [1_000_000], total=11) == ([9], 2)
    assert q_stream(lv, Q.PEAK, [1_000_000], total=0) == ([0], 0)


def test_a_rank_on_an_integer_and_just_below_it():
    lv = recs(peaks=[50, 10, 40, 20, 30])            # K = 5: rank = 4 q / 10^6
    assert q_stream(lv, Q.PEAK, [0, 249_999, 250_000, 500_000, 749_999, 750_000, 999_999, 1_000_000]) == \
        ([10, 10, 20, 30, 30, 40, 40, 50], 5)
    lv = recs(peaks=list(range(101, 0, -1)))          # K = 101: rank = q / 10^4
    assert q_stream(lv, Q.PEAK, [980_000, 979_999, 10_000, 9_999, 999_999])[0] == [99, 98, 2, 1, 100]


def test_all_keys_equal_and_the_maxima():
    assert q_stream(recs(peaks=[33] * 7), Q.PEAK, [0, 123_456, 1_000_000]) == ([33, 33, 33], 7)
    lv = recs(peaks=[5, 5, 5])
    lv["min"][1] = -32768                              # the peak 32768 comes from min alone
    assert q_stream(lv, Q.PEAK, [0, 1_000_000]) == ([5, 32768], 3)
    lv["min"][0] = -40_000                             # hand-made: clamped to the limit
    lv["max"][2], lv["min"][2] = -7, 9                 # hand-made: a negative peak is 0
    assert q_stream(lv, Q.PEAK, [0, 500_000, 1_000_000]) == ([0, 32768, 32768], 3)
    lv = recs(mean_sqs=[3, 1 << 30, 2])
    lv["sum_sq"][1] = (1 << 30) * 10                   # every sample -32768
    assert q_stream(lv, Q.MEAN_SQ, [0, 500_000, 1_000_000]) == ([2, 3, 1 << 30], 3)
    lv["sum_sq"][0] = (1 << 63) + 5                    # hand-made: clamped
    assert q_stream(lv, Q.MEAN_SQ, [500_000, 1_000_000])[0] == [1 << 30, 1 << 30]


def test_the_mean_square_key_floors_and_orders_by_the_quotient():
    lv = empty(3)
    lv["n"] = [10, 3, 1]
    lv["sum_sq"] = [109, 30, 9]                        # floors 10, 10, 9: sum_sq alone orders them the other way round
    assert q_stream(lv, Q.MEAN_SQ, [0, 500_000, 1_000_000]) == ([9, 10, 10], 3)
    for r in lv:                                       # the key is the largest mean_sq_min at which the row is still hot
        k = Q.key_of(r, Q.MEAN_SQ)
        assert E.is_hot(r, E.Rule(mean_sq_min=k)) and not E.is_hot(r, E.Rule(mean_sq_min=k + 1))
    lv = recs(peaks=[17])
    assert E.is_hot(lv[0], E.Rule(peak_min=17)) and not E.is_hot(lv[0], E.Rule(peak_min=18))


def test_corpus_entries_and_rows_that_do_not_count():
    # entries of 2, 1 (no samples: one row), 3 rows
    ns = [2 * BL - 1, 0, 3 * BL]
    lv = recs(peaks=[4, 8, 99, 6, 2, 9])
    lv["n"][2] = 0                                     # what the levels call leaves in the row of an entry without samples
    v, k = Q.corpus_quantiles(lv, ns, BL, Q.PEAK, [1_000_000, 0])
    assert v.tolist() == [[8, 4], [0, 0], [9, 2]] and k.tolist() == [2, 0, 3]
    assert Q.rows_by_table(ns, BL, 6) == [[0, 1], [2], [3, 4, 5]]
    assert Q.rows_by_table(ns, BL, 4) == [[0, 1], [2], [3]]                       # clipped to n_rows
    # a wild table: the prefix wraps, entries move past the rows or are emptied
    assert Q.rows_by_table([2 ** 64 - 1, 5, 5], 1, 4) == [[0, 1, 2, 3], [], []]
    tab = Q.rows_by_table([BL * 100, 0, 0], BL, 6)
    assert tab == [[0, 1, 2, 3, 4, 5], [], []]


def test_the_map_clamps_and_floors():
    lv = recs(peaks=[10, 20, 30], mean_sqs=[100, 200, 300])
    med = 500_000
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 3, 2, 1))) == [(0, 31, 3)]
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 1, 3, 0))) == [(0, 6, 3)]         # 20 / 3 floors
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 0, 1, 0))) == [(0, 1, 3)]         # clamped at 1
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 1, 21, 0))) == [(0, 1, 3)]
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 2000, 1, 0))) == [(0, 32768, 3)]  # ... and at the limit
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 1, 1, 2 ** 32 - 1))) == [(0, 32768, 3)]
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(mean_sq=(med, 4, 1, 0))) == [(800, 0, 3)]    # 6 dB over the median
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(mean_sq=(1_000_000, 2 ** 32 - 1, 1, 0))) == [(1 << 30, 0, 3)]
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(0, 1, 1, 0), mean_sq=(0, 7, 2, 5))) == [(355, 10, 3)]
    big = recs(mean_sqs=[1 << 30])
    big["sum_sq"][0] = (1 << 30) * 10
    assert Q.stream_thresholds(big, 10, BL, Q.TRule(mean_sq=(0, 2 ** 32 - 1, 2 ** 32 - 1, 0))) == [(1 << 30, 0, 1)]
    # K == 0, or a criterion whose div is 0: off
    lv["n"] = 0
    assert Q.stream_thresholds(lv, 30, BL, Q.TRule(peak=(med, 1, 1, 5), mean_sq=(med, 1, 1, 5))) == [(0, 0, 0)]
    assert Q.stream_thresholds(recs(peaks=[10]), 10, BL, Q.TRule(peak=(med, 1, 0, 5), mean_sq=(med, 1, 1, 0))) == [(1, 0, 1)]


def test_adaptive_hot_rows_feed_the_events_run_logic():
    lv = recs(peaks=[10, 50, 10, 10, 50, 50])
    ns = [3 * BL, 3 * BL]
    rule = E.Rule()
    # the same rows under two thresholds: 50 is hot in entry 0 only
    ev, _ = Q.corpus_adaptive_events(lv, ns, BL, [(0, 40), (0, 60)], rule)
    assert ev == [(0, 10, 10)]
    ev, _ = Q.corpus_adaptive_events(lv, ns, BL, [(0, 60), (0, 40)], rule)
    assert ev == [(1, 10, 20)]
    # both zero: no hot rows; a value above its limit: that criterion is never hot
    assert Q.corpus_adaptive_events(lv, ns, BL, [(0, 0), (0, 32769)], rule)[0] == []
    assert Q.corpus_adaptive_events(lv, ns, BL, [((1 << 30) + 1, 0), (2 ** 64 - 1, 50)], rule)[0] == [(1, 10, 20)]
    # equality at sum_sq == thr * n
    lv = recs(mean_sqs=[7])
    lv["sum_sq"][0] = 70
    assert Q.stream_adaptive_events(lv, BL, BL, (7, 0), rule)[0] == [(0, 10)]
    assert Q.stream_adaptive_events(lv, BL, BL, (8, 0), rule)[0] == []
    # equal thresholds are the plain events call
    lv = recs(peaks=[10, 50, 10, 10, 50, 50])
    assert Q.corpus_adaptive_events(lv, ns, BL, [(0, 40)] * 2, E.Rule(join_bins=2, pad_bins=1))[0] == \
        E.corpus_events(lv, ns, BL, E.Rule(peak_min=40, join_bins=2, pad_bins=1))[0]


def test_rows_by_table_is_the_sequential_layout_on_a_sound_table():
    rng = np.random.default_rng(5)
    for _ in range(50):
        ns = [int(v) for v in rng.integers(0, 60, int(rng.integers(1, 12)))]
        rows = [max(1, -(-v // BL)) for v in ns]
        want, at = [], 0
        for r in rows:
            want.append(list(range(at, at + r)))
            at += r
        assert Q.rows_by_table(ns, BL, at) == want
