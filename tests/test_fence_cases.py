"""The preconditions of the exact-fit cases under guard pages (fence_cases.py), from the CPU references and the oracle alone:
a case can only catch an access behind a buffer if the buffer is exactly what include/x3hip.h asks for and the stream ends
where the case says it does, and it can only catch a kernel that leaves an output alone if the expectation is not what the
fresh buffer holds.  tests/test_gpu_fence_analysis.py runs the same tables on the GPU."""
import numpy as np
import pytest

import fence_cases as FC


@pytest.mark.parametrize("name", list(FC.STREAMS))
def test_streams_end_where_the_cases_say(name):
    s = FC.stream(name)
    bpf, k, kind = FC.STREAMS[name]
    assert (s.bpf, s.k, s.F, s.total) == (bpf, k, k + 1, FC.BL * bpf * k + 1)
    assert s.offs[-1] == s.bytes.size and s.bytes.size - s.offs[-2] == 22          # a header and one raw sample
    assert int(s.so[-1] - s.so[-2]) == 1 and all(int(b - a) == FC.BL * bpf for a, b in zip(s.so[:-2], s.so[1:-1]))
    if FC.RESIDUE[kind] is not None:
        assert s.bytes.size % 16 == FC.RESIDUE[kind]
    statuses = [st for st, _ in s.frames]
    assert statuses == [FC.CRC if kind == "crc" and f == k - 1 else 0 for f in range(k + 1)]
    assert s.n_index == 1 + s.F * (-(-bpf // s.seg_blocks) - 1) and s.n_index > 1


def test_no_stream_has_an_odd_size():
    """why "m2" and not 1 mod 16: every payload is whole 16-bit words, so is every frame and every stream"""
    for seed in range(40):
        for bpf, n in ((7, 141), (100, 2001)):
            rc, s, _ = FC.O.encode(FC._wav(seed, n), FC.oparams(bpf))
            assert rc == 0 and s.size % 2 == 0


def test_both_geometries_have_every_k_and_every_kind():
    for bpf in (7, 100):
        mine = [v for v in FC.STREAMS.values() if v[0] == bpf]
        assert sorted(v[1] for v in mine) == [1, 2, 3] and sorted(v[2] for v in mine) == ["crc", "m16", "m2"]


@pytest.mark.parametrize("bpf", list(FC.CORPORA))
def test_a_corpus_is_its_streams_back_to_back(bpf):
    c = FC.corpus(bpf)
    assert c.bytes.size == sum(c.lengths) and c.offsets[0] == 0
    for s, off, ln in zip(c.entries, c.offsets, c.lengths):
        assert np.array_equal(c.bytes[off:off + ln], s.bytes)
    assert c.offsets[-1] + c.lengths[-1] == c.bytes.size                           # the last one-sample frame ends the buffer
    assert sorted(s.kind for s in c.entries) == ["crc", "m16", "m2"] and c.F == sum(s.k + 1 for s in c.entries)


def test_the_groups_hold_the_cases_the_gpu_test_counts():
    names = [case.name for g in FC.GROUPS for _, cases in FC.group(g) for case in cases]
    assert len(set(names)) == len(names)
    for g in FC.GROUPS:
        assert FC.n_cases(g) == FC.COUNTS[g], g


def _cases(group):
    return [(src, case) for src, cases in FC.group(group) for case in cases]


@pytest.mark.parametrize("group", FC.GROUPS)
def test_every_size_is_the_references_own_need(group):
    for src, case in _cases(group):
        assert case.exact, case.name
        for what, given, need in case.exact:
            assert given == need, (case.name, what, given, need)
        n = len(case.inputs["starts"]) if "starts" in case.inputs else None
        if n is not None:                                # windows, ranges, range levels: 4 n of statuses, 8 (n + 1) of offsets
            assert FC.bytes_of(case.outputs["st"]).size == 4 * n, case.name
            assert "off" not in case.outputs or FC.bytes_of(case.outputs["off"]).size == 8 * (n + 1), case.name
        if "fst" in case.outputs:                        # levels: 4 F of frame statuses
            assert FC.bytes_of(case.outputs["fst"]).size == 4 * src.F, case.name
        for k, a in list(case.inputs.items()) + list(case.outputs.items()):
            assert FC.bytes_of(a).size > 0, (case.name, k)


@pytest.mark.parametrize("group", FC.GROUPS)
def test_no_expectation_is_what_a_fresh_buffer_holds(group):
    """every output array holds bytes other than the fill, and no status, offset, count, threshold or quantile is the fill
    in all of its bytes: an output the call leaves alone is seen"""
    for _, case in _cases(group):
        for k, a in case.outputs.items():
            b = FC.bytes_of(a)
            assert (b != FC.FILL).any(), (case.name, k)
            if k in case.control:
                per = np.ascontiguousarray(a).reshape(-1)
                assert not (b.reshape(per.size, -1) == FC.FILL).all(axis=1).any(), (case.name, k)


def test_levels_take_a_bin_that_divides_neither_frame_nor_block_and_0_and_1():
    assert set(FC.BINS) == {FC.BIN, 0, 1}
    assert all(FC.BL * bpf % FC.BIN for bpf in FC.CORPORA) and FC.BL % FC.BIN and FC.BIN % FC.BL
    assert FC.planes_of("bank3") == 3 and FC.planes_of("bank8") == 8 and len(FC.TAPS8) == 8


def test_range_tables_hold_the_ranges_the_edges_need():
    for name in FC.STREAMS:
        s = FC.stream(name)
        r = list(zip(*FC.stream_ranges(s)))
        assert (0, s.total) in r and (s.total, 0) in r and (s.total - 1, 1) in r
        assert any(a + n == s.total and n > 1 for a, n in r)                       # ends on the last sample
        assert all(a + n <= s.total for a, n in r)
        if s.kind == "crc":                                                        # the one-sample frame's lead frame failed
            assert s.frames[s.F - 2][0] == FC.CRC and int(s.so[-2]) == s.total - 1


def test_records_run_around_the_events_tile_and_reach_the_last_row():
    assert FC.N_ROWS == (FC.EVENTS_TILE - 1, FC.EVENTS_TILE, FC.EVENTS_TILE + 1)
    for n_rows in FC.N_ROWS:
        lv = FC.record_planes(n_rows, 1)[0]
        hot = [FC.E.is_hot(r, FC.EV_RULE) for r in lv]
        assert hot[n_rows - 1] and 4 <= sum(1 for a, b in zip([False] + hot, hot) if b and not a) <= 8
        for K in FC.PLANE_K:
            n = FC.loud_counts(FC.record_planes(n_rows, K), n_rows, FC.plane_rule(K, 1))
            assert (n == 1).any() and (n == 2).any() and (n == K).any(), (n_rows, K)
            assert n[n_rows - 1] == K


def test_plane_event_expectations_differ_between_the_three_min_planes():
    cases = {case.name: case for _, case in _cases("B4")}
    for n_rows in FC.N_ROWS:
        for form in ("", "corpus_"):
            for K in FC.PLANE_K:
                full = []
                for mp in (1, 2, K):
                    mine = [c for n, c in cases.items() if n.startswith("plane_events_%s%d_K%d_min%d_cap" % (form, n_rows, K, mp))]
                    assert len(mine) == 2
                    a, b = sorted(mine, key=lambda c: len(c.outputs["ev_st"]))
                    count = int(b.outputs["cnt"][0])
                    assert len(b.outputs["ev_st"]) == count and len(a.outputs["ev_st"]) == count - 1 >= 1   # d_count above cap
                    full.append(b)
                for i in range(3):
                    for j in range(i + 1, 3):
                        x, y = full[i].outputs, full[j].outputs
                        assert x["ev_st"].tobytes() != y["ev_st"].tobytes() or x["ev_mk"].tobytes() != y["ev_mk"].tobytes()
                        assert int(x["cnt"][0]) != int(y["cnt"][0]) or x["ev_ln"].tobytes() != y["ev_ln"].tobytes()


def test_caps_are_the_count_and_one_below_it():
    for _, case in _cases("B4"):
        if "cnt" in case.outputs:
            count, cap = int(case.outputs["cnt"][0]), len(case.outputs["ev_st"])
            assert cap in (count, count - 1) and cap >= 1, case.name
            assert FC.bytes_of(case.outputs["ev_st"]).size == 8 * cap and FC.bytes_of(case.outputs["ev_ln"]).size == 4 * cap
