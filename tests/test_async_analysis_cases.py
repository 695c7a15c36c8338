"""The preconditions of the stalled-stream cases of the analysis calls (async_analysis_cases.py), from the CPU references
alone: a case can only catch a call that reads early, or a kernel that runs in front of its producer, if the decoy A and the
content B give different answers in everything the case compares; it may only run on a shared GPU if A's and B's tables are
in bounds for the shapes the calls are given; and a corpus case needs a decoy of exactly B's geometry, because the corpus's
frame table is fixed at the build."""
import numpy as np
import pytest

import async_analysis_cases as AA
import async_cases as AC


@pytest.mark.parametrize("case", AA.CASES, ids=lambda c: c.name)
def test_decoy_and_content_differ_in_every_compared_output(case):
    AC.check_pair_differs(case)


def test_case_names_are_unique_and_disjoint_from_the_first_set():
    names = [c.name for c in AA.CASES]
    assert len(set(names)) == len(names)
    assert not set(names) & {c.name for c in AC.CASES}


def test_the_cases_the_contract_needs_are_all_there():
    names = {c.name for c in AA.CASES}
    want = {"levels_%s%s" % (s, d) for s in ("samples", "diff", "fir3", "fir8") for d in ("", "_damaged")}
    want |= {"range_levels_" + s for s in ("samples", "diff", "fir3", "fir3_damaged")}
    want |= {"events_from_records", "quantiles_from_records", "adaptive_from_records", "stream_chain"}
    want |= {"corpus_levels_" + s for s in ("samples", "diff", "fir3")} | {"corpus_range_levels_" + s for s in ("samples", "fir3")}
    want |= {"corpus_events_from_records", "corpus_adaptive_from_records", "corpus_ranges_pair", "corpus_chain"}
    assert names == want


@pytest.mark.parametrize("case", AA.CASES, ids=lambda c: c.name)
def test_same_ok_names_statuses_totals_and_sample_offsets_only(case):
    """never level records, event arrays, thresholds, quantiles, rows or a count of results"""
    assert set(case.same_ok) <= AA.SAME_OK_ALLOWED, case.same_ok


def test_the_corpus_decoy_has_the_contents_geometry():
    a, b = AA.corpus_content("A"), AA.corpus_content("B")
    assert a[0].size == b[0].size and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3])                                  # the frame offsets
    flipped = np.flatnonzero(a[0] != b[0])
    assert flipped.size == AA.NE                                       # one payload byte per entry
    frames = np.searchsorted(a[3], flipped, side="right") - 1
    first = np.concatenate([[0], np.cumsum([len(e[0]) for e in b[4]])])
    assert [int(f - first[e]) for e, f in enumerate(frames)] == [AA.damaged_frame(e) for e in range(AA.NE)]
    assert all(int(x) - int(a[3][f]) >= 20 for x, f in zip(flipped, frames))      # in the payload: headers as B's
    # the frames decode as the cases say: the oracle on every entry of A and of B
    for which, c in (("A", a), ("B", b)):
        for e, (fr, st, so) in enumerate(c[4]):
            s = c[0][c[1][e]:c[1][e] + c[2][e]]
            got = AA.RR.frames_of(s, AA.RR.frame_offsets(s), AA.c_oparams())
            assert [g[0] for g in got] == st.tolist(), (which, e)
            assert all(np.array_equal(g[1], w) for g, w, t in zip(got, fr, st) if t == 0), (which, e)
            assert int(so[-1]) == AA.ENTRY_SAMPLES[e] and 12 <= len(fr) <= 30


def test_the_stream_decoy_fails_where_the_cases_say():
    for kind in ("Ad", "Bd"):
        s, st = AA.stream(kind)
        got = AA.RR.frames_of(s, [int(v) for v in AA.offsets(kind)], AC.oparams())
        assert [g[0] for g in got] == st.tolist(), kind
        assert all(np.array_equal(g[1], w) for g, w, t in zip(got, AA.wav_frames(kind), st) if t == 0), kind
    assert np.flatnonzero(AA.stream("Ad")[1]).tolist() == [AA.AD_FRAME] and np.flatnonzero(AA.stream("Bd")[1]).tolist() == [9, 30]


@pytest.mark.parametrize("case", [c for c in AA.CASES if hasattr(c, "counts")], ids=lambda c: c.name)
def test_event_counts_differ_and_fit_the_capacity(case):
    a, b, cap, at_least = case.counts()
    assert a != b and a < cap and b < cap and b >= at_least, (a, b, cap)


@pytest.mark.parametrize("case", [c for c in AA.CASES if hasattr(c, "b_events")], ids=lambda c: c.name)
def test_a_run_of_the_content_spans_an_edge_of_the_events_tiles(case):
    """rows of one run in two tiles: only the scan between the tiles (x3_events_near_kernel) joins them, so a case without
    such a run could not tell whether that kernel ran in its place"""
    assert AA.spans_a_tile_edge(*case.b_events())


def test_the_fir_of_eight_taps_shifts():
    taps, shift = AA.FIRS["fir8"]
    assert len(taps) == 8 and shift > 0 and sum(abs(c) for c in taps) <= 32768
    assert AA.FIRS["fir3"] == ((1, -2, 1), 0)
