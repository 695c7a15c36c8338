"""plane_events_ref (the definition of x3_plane_events_dev and its corpus form): the events of events_ref on one synthetic
row verdict, "at least min_planes planes are loud".  The identities that follow from that, and DESIGN.md section 28's
example with its numbers.  No GPU."""
import numpy as np

import events_ref as E
import levels_ref as R
import plane_events_ref as P
import quantiles_ref as Q
import tone_bank_levels_ref as B
import tone_levels_ref as TR

BL = 4


def random_planes(rng, k, n, p_hot=0.3):
    """K planes of n records: loud (peak 1500, mean square 750 000) with probability p_hot, a few rows with nothing counted"""
    lv = np.stack([R.empty(n) for _ in range(k)])
    for t in range(k):
        hot = rng.random(n) < p_hot
        lv[t]["n"] = np.where(rng.random(n) < 0.05, 0, BL)
        lv[t]["max"] = np.where(hot, 1500 + rng.integers(0, 9, n), 10)
        lv[t]["min"] = -rng.integers(1, 20, n)
        lv[t]["sum"] = rng.integers(-500, 500, n)
        lv[t]["sum_sq"] = np.where(hot, 3_000_000, 200).astype(np.uint64) + rng.integers(0, 50, n).astype(np.uint64)
    return lv


def random_rule(rng, k, min_planes=None):
    join = int(rng.choice([0, 1, 2, 5]))
    crit = rng.integers(0, 3, k)                                 # peak alone, mean square alone, both
    return P.PlaneRule(mean_sq_min=[0 if c == 0 else 500_000 for c in crit], peak_min=[0 if c == 1 else 1000 for c in crit],
                       min_planes=int(rng.integers(1, k + 1)) if min_planes is None else min_planes, join_bins=join,
                       min_bins=int(rng.choice([0, 1, 2])), pad_bins=int(rng.integers(0, join // 2 + 1)),
                       max_bins=int(rng.choice([0, 0, 1, 3])))


def single(rule, t=0):
    return E.Rule(rule.mean_sq_min[t], rule.peak_min[t], rule.join_bins, rule.min_bins, rule.pad_bins, rule.max_bins)


def whole(rule):
    """no run is cut: every event holds its run's hot rows.  A piece of a cut run may be padding or gap rows alone, and
    then no plane is loud in it: its mask is 0"""
    return rule.max_bins == 0


def loud_in(recs, start, ln, rule):
    return any(E.is_hot(r, rule) for r in recs[start // BL:-(-(start + ln) // BL)])


def test_one_plane_is_the_events_call():
    rng = np.random.default_rng(1)
    for case in range(40):
        n = int(rng.integers(1, 90))
        lv = random_planes(rng, 1, n)
        rule = random_rule(rng, 1)
        tot = int(rng.choice([BL * n, BL * n - 3, BL * (n // 2) + 1, 10 ** 9]))
        ev, elv = P.stream_plane_events(lv, tot, BL, rule)
        ev1, elv1 = E.stream_events(lv[0], tot, BL, single(rule))
        assert [e[:2] for e in ev] == ev1 and elv[0].tobytes() == elv1.tobytes()
        assert all(e[2] == int(whole(rule) or loud_in(lv[0], e[0], e[1], single(rule))) for e in ev)
        ns = [BL * 7 - 1, 0, BL * 3, 10 ** 6]
        ev, elv = P.corpus_plane_events(lv, ns, BL, rule)
        ev1, elv1 = E.corpus_events(lv[0], ns, BL, single(rule))
        assert [e[:3] for e in ev] == ev1 and all(e[3] <= 1 for e in ev) and elv[0].tobytes() == elv1.tobytes()
        assert not whole(rule) or all(e[3] == 1 for e in ev)
        # ... and with thresholds, the adaptive calls; a value above its limit is off, counted is ignored
        thr = [[(int(rng.choice([0, 500_000, (1 << 30) + 1])), int(rng.choice([0, 1000, 32769])), 77) for _ in ns]]
        rule0 = rule._replace(mean_sq_min=[0], peak_min=[0])
        ev, elv = P.corpus_plane_events(lv, ns, BL, rule0, thr)
        ev1, elv1 = Q.corpus_adaptive_events(lv[0], ns, BL, thr[0], single(rule0))
        assert [e[:3] for e in ev] == ev1 and elv[0].tobytes() == elv1.tobytes()
        ev, elv = P.stream_plane_events(lv, tot, BL, rule0, [thr[0][0]])
        ev1, elv1 = Q.stream_adaptive_events(lv[0], tot, BL, thr[0][0], single(rule0))
        assert [e[:2] for e in ev] == ev1 and elv[0].tobytes() == elv1.tobytes()


def test_equal_planes_are_the_single_plane():
    rng = np.random.default_rng(2)
    for case in range(20):
        n, k = int(rng.integers(1, 90)), int(rng.integers(2, 9))
        one = random_planes(rng, 1, n)
        r1 = random_rule(rng, 1)
        ev1, elv1 = E.stream_events(one[0], BL * n, BL, single(r1))
        for mp in range(1, k + 1):
            rule = r1._replace(mean_sq_min=r1.mean_sq_min * k, peak_min=r1.peak_min * k, min_planes=mp)
            ev, elv = P.stream_plane_events(np.concatenate([one] * k), BL * n, BL, rule)
            assert [e[:2] for e in ev] == ev1
            assert all(e[2] == ((1 << k) - 1) * int(whole(rule) or loud_in(one[0], e[0], e[1], single(r1))) for e in ev)
            assert all(elv[t].tobytes() == elv1.tobytes() for t in range(k))


def test_a_permutation_of_the_planes_permutes_mask_and_levels_alone():
    rng = np.random.default_rng(3)
    for case in range(20):
        n, k = int(rng.integers(1, 90)), int(rng.integers(2, 9))
        lv, rule = random_planes(rng, k, n), random_rule(rng, k)
        perm = rng.permutation(k)
        prule = rule._replace(mean_sq_min=[rule.mean_sq_min[j] for j in perm], peak_min=[rule.peak_min[j] for j in perm])
        ev, elv = P.stream_plane_events(lv, BL * n, BL, rule)
        pev, pelv = P.stream_plane_events(lv[perm], BL * n, BL, prule)
        assert [e[:2] for e in ev] == [e[:2] for e in pev]
        for e, pe in zip(ev, pev):                                   # plane i of the permuted call is plane perm[i]
            assert pe[2] == sum(((e[2] >> int(perm[i])) & 1) << i for i in range(k))
        assert pelv.tobytes() == elv[perm].tobytes()


def test_union_and_intersection():
    rng = np.random.default_rng(4)
    for case in range(20):
        n, k = int(rng.integers(1, 90)), int(rng.integers(2, 9))
        lv = random_planes(rng, k, n, p_hot=0.6)
        rule = random_rule(rng, k)._replace(join_bins=0, min_bins=0, pad_bins=0, max_bins=1)   # (an event per hot row)
        loud = np.array([[E.is_hot(lv[t][b], single(rule, t)) for b in range(n)] for t in range(k)])
        for mp, want in ((1, loud.any(axis=0)), (k, loud.all(axis=0))):
            ev, _ = P.stream_plane_events(lv, BL * n, BL, rule._replace(min_planes=mp))
            assert [e[0] // BL for e in ev] == np.flatnonzero(want).tolist()
            assert all(e[2] == sum(int(loud[t][e[0] // BL]) << t for t in range(k)) for e in ev)


def test_a_padding_row_sets_the_bits_of_the_planes_loud_there():
    lv = np.stack([R.empty(8) for _ in range(2)])
    for t in range(2):
        lv[t]["n"], lv[t]["max"], lv[t]["min"] = BL, 10, -10
    lv[0]["max"][[3, 4]] = 2000
    lv[1]["max"][[2, 4]] = 2000                                      # row 2: loud in plane 1 alone, row 3: in plane 0 alone
    rule = P.PlaneRule([0, 0], [1000, 1000], min_planes=2, join_bins=2, pad_bins=1)
    ev, elv = P.stream_plane_events(lv, BL * 8, BL, rule)
    assert ev == [(BL * 3, BL * 3, 3)] and elv[1][0]["max"] == 2000 and elv[0][0]["n"] == 3 * BL
    ev, _ = P.stream_plane_events(lv, BL * 8, BL, rule._replace(join_bins=0, pad_bins=0))
    assert ev == [(BL * 4, BL, 3)]
    sl = P.slots(*P.stream_plane_events(lv, BL * 8, BL, rule), 3, False)
    assert sl[0] is None and sl[3].tolist() == [3, 0, 0] and sl[4].shape == (2, 3)
    assert sl[4][:, 1:].tobytes() == np.stack([R.empty(2)] * 2).tobytes()


def test_the_example_a_step_between_bands_and_three_bands_at_once():
    """section 26's signal with five more bursts; bins of 200, a bank of four, the adapter,
    mean_sq_min = 400 000 in every plane"""
    w = P.example()
    frames, so = [w[a:a + 2_000] for a in range(0, 20_000, 2_000)], range(0, 20_000, 2_000)
    tone = B.tone_bank_levels(frames, [0] * 10, so, 200, 100, B.EXAMPLE_STEPS)
    planes = np.stack([TR.tone_power_levels(p) for p in tone])
    ms = [(p["sum_sq"] // p["n"]).astype(np.int64) for p in planes]
    loud = [{int(b): int(m[b]) for b in np.flatnonzero(m >= 400_000)} for m in ms]
    assert loud == [{22: 655_216, 40: 450_306, 80: 689_075}, {41: 685_978, 60: 518_188, 80: 685_892}, {80: 601_612}, {}]
    rest = [np.where(m >= 400_000, 0, m) for m in ms]
    assert max((int(r.max()), t, int(r.argmax())) for t, r in enumerate(rest)) == (322_926, 2, 19)
    rule = P.PlaneRule([400_000] * 4, [0] * 4)
    ev, elv = P.stream_plane_events(planes, 20_000, 200, rule)
    assert ev == [(4_400, 200, 1), (8_000, 400, 3), (12_000, 200, 2), (16_000, 200, 7)]
    assert [int(elv[t][1]["sum_sq"]) // int(elv[t][1]["n"]) for t in range(4)] == [236_813, 373_441, 13_655, 38_396]
    assert [int(elv[t][3]["sum_sq"]) // int(elv[t][3]["n"]) for t in range(4)] == [689_075, 685_892, 601_612, 6_780]
    for mp in (2, 3):
        assert P.stream_plane_events(planes, 20_000, 200, rule._replace(min_planes=mp))[0] == [(16_000, 200, 7)]
    assert P.stream_plane_events(planes, 20_000, 200, rule._replace(min_planes=4))[0] == []
    # plane by plane the step is two short events in two lists, never (8 000, 400)
    one = [E.stream_events(planes[t], 20_000, 200, E.Rule(mean_sq_min=400_000))[0] for t in range(4)]
    assert (8_000, 200) in one[0] and (8_200, 200) in one[1] and not any((8_000, 400) in o for o in one)
