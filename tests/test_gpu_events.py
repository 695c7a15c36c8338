"""Events (include/x3hip.h, "EVENTS"): x3_events_dev, x3_corpus_events_dev, x3_events_result and their Python mirrors.  Every
field of every slot -- entry, start, len, merged record, the filler behind the last event, the count -- is held with ==
against events_ref.py.  Most cases upload synthetic level records straight into d_levels (no decode): row counts and run
positions are laid around the kernels' tile (option "events_tile_rows"); the end-to-end cases run levels, events and ranges
back to back on the device with no wait in between."""
import ctypes as C

import numpy as np
import pytest

import events_ref as E
import levels_ref as R
import oracle_lib as O
import x3_cases as XC

pytestmark = pytest.mark.gpu

BAD = 24
CRC = 14
GUARD = 64
CANARY = 0x5A
BL = 4                      # bin length of the synthetic cases: an entry of r rows is a clip of at most 4 r samples
PEAK = E.Rule(peak_min=1000)


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.get_option("events_tile_rows")
    assert t >= 64 and t % 64 == 0
    return t


def rule_of(x3, r):
    return x3.EventRule.make(*r)


def records(hot, rng=None, empty_at=()):
    """level records: loud where `hot` is set (peak 1500), quiet elsewhere (peak 10), nothing counted at `empty_at` (whose
    other fields stay loud: n == 0 alone must keep them cold)"""
    hot = np.asarray(hot, dtype=bool)
    lv = R.empty(hot.size)
    k = np.arange(hot.size)
    lv["n"] = BL
    lv["max"] = np.where(hot, 1500 + k % 7, 10)
    lv["min"] = np.where(hot, -(20 + k % 5), -(3 + k % 3))
    lv["sum"] = np.where(hot, 100 + k, -k)
    lv["sum_sq"] = np.where(hot, 3_000_000 + k, 200 + k).astype(np.uint64)
    if rng is not None:
        lv["sum"] += rng.integers(-50, 50, hot.size)
    for i in empty_at:
        lv["n"][i] = 0
    return lv


class Guarded:
    """device arrays with a canary in front of and behind each"""

    def __init__(self, ctx, sizes):
        self.ctx, self.sizes = ctx, sizes
        self.base = [ctx.alloc(s + 2 * GUARD) for s in sizes]
        for q, s in zip(self.base, sizes):
            ctx.upload(q, np.full(s + 2 * GUARD, CANARY, dtype=np.uint8))
        self.ptr = [q + GUARD for q in self.base]

    def read(self):
        out = []
        for i, (q, s) in enumerate(zip(self.base, self.sizes)):
            raw = self.ctx.download(q, s + 2 * GUARD)
            assert (raw[:GUARD] == CANARY).all() and (raw[GUARD + s:] == CANARY).all(), "canary of array %d damaged" % i
            out.append(raw[GUARD:GUARD + s].copy())
        return out

    def close(self):
        for q in self.base:
            self.ctx.free(q)


def run(ctx, x3, lv, rule, cap, total=None, corpus=None, with_levels=True, bin_len=BL, n_rows=None):
    """one call on uploaded records -> (entries or None, starts, lens, event levels or None, count); the result call, the
    canaries round every output and "every slot is written" are checked"""
    n_rows = lv.size if n_rows is None else n_rows
    d_lv, d_tot = ctx.alloc(32 * lv.size), ctx.alloc(8)
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 32 * cap, 8])
    try:
        ctx.upload(d_lv, lv)
        ctx.upload(d_tot, np.array([0 if total is None else total], dtype=np.uint64))
        d_ent, d_st, d_ln, d_el, d_cnt = g.ptr
        r = rule_of(x3, rule)
        if corpus is None:
            rc = ctx.events_dev(d_lv, n_rows, bin_len, d_tot, r, d_st, d_ln, d_el if with_levels else None, cap, d_cnt)
        else:
            rc = corpus.events_into(d_lv, n_rows, bin_len, r, d_ent, d_st, d_ln, d_el if with_levels else None, cap, d_cnt)
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.events_result()
        ent, st, ln, el, cnt = g.read()
    finally:
        g.close()
        ctx.free(d_lv)
        ctx.free(d_tot)
    cnt = int(cnt.view(np.uint64)[0])
    assert res == (0, cnt), (res, cnt)
    if corpus is None:
        assert (ent == CANARY).all(), "a stream call has no entries to write"
    if not with_levels:
        assert (el == CANARY).all()
    return (ent.view(np.uint32) if corpus is not None else None, st.view(np.uint64), ln.view(np.uint32),
            el.view(R.LEVEL_DTYPE) if with_levels else None, cnt)


def check(ctx, x3, lv, rule, cap, total=None, corpus=None, n_samples=None, with_levels=True, what=None):
    got = run(ctx, x3, lv, rule, cap, total=total, corpus=corpus, with_levels=with_levels)
    if corpus is None:
        ev, elv = E.stream_events(lv, total, BL, rule)
    else:
        ev, elv = E.corpus_events(lv, n_samples, BL, rule)
    ent, st, ln, sl = E.slots(ev, elv, cap, corpus is not None)
    assert got[4] == len(ev), (what, got[4], len(ev))
    if corpus is not None:
        assert np.array_equal(got[0], ent), (what, np.flatnonzero(got[0] != ent)[:5])
    assert np.array_equal(got[1], st), (what, np.flatnonzero(got[1] != st)[:5], got[1][:8], st[:8])
    assert np.array_equal(got[2], ln), (what, np.flatnonzero(got[2] != ln)[:5], got[2][:8], ln[:8])
    if with_levels:
        for k in R.LEVEL_DTYPE.names:
            assert np.array_equal(got[3][k], sl[k]), (what, k, np.flatnonzero(got[3][k] != sl[k])[:5])
    return ev


# ------------------------------------------------------------------------------------------------ stream form, synthetic
def row_counts(T):
    return [1, T - 1, T, T + 1, 3 * T + 1]


def test_stream_patterns_round_the_tile(ctx, x3, T):
    for n in row_counts(T):
        tot = BL * n - 1
        k = np.arange(n)
        none, all_hot, alt = np.zeros(n, bool), np.ones(n, bool), k % 2 == 0
        assert check(ctx, x3, records(none), PEAK, 4, total=tot) == []
        assert check(ctx, x3, records(all_hot), PEAK, 4, total=tot) == [(0, tot)]
        ev = check(ctx, x3, records(alt), PEAK, n + 2, total=tot, what=("alt", n))
        assert len(ev) == (n + 1) // 2
        assert check(ctx, x3, records(alt), PEAK._replace(join_bins=1), 3, total=tot) == [(0, BL * (n - (n + 1) % 2) - (n % 2))]
        # max_bins 1: an event per bin of a run, padding included; without the merged records as well
        for with_levels in (True, False):
            ev = check(ctx, x3, records(k % 5 == 2), PEAK._replace(join_bins=2, pad_bins=1, max_bins=1), n + 1, total=tot,
                       with_levels=with_levels, what=("max_bins 1", n))
            assert all(e[1] <= BL for e in ev)
        # cap below, at and above the count: the filler in every unused slot, the full count
        hot = k % 3 == 0
        cnt = len(E.stream_events(records(hot), tot, BL, PEAK)[0])
        for cap in sorted({max(cnt - 1, 1), cnt, cnt + 5}):
            assert len(check(ctx, x3, records(hot), PEAK, cap, total=tot, what=("cap", n, cap))) == cnt
        # bins nothing was counted in: cold inside a run, whatever their other fields say
        if n >= 3:
            lv = records(all_hot, empty_at=range(1, n, 2))
            assert len(check(ctx, x3, lv, PEAK, n, total=tot)) == (n + 1) // 2
            assert len(check(ctx, x3, lv, PEAK._replace(join_bins=1), n, total=tot)) == 1


def test_runs_and_gaps_across_tile_edges(ctx, x3, T):
    n = 3 * T + 1
    tot = BL * n
    # a run that starts in one tile and ends two tiles on
    hot = np.zeros(n, bool)
    hot[T - 3:2 * T + 5] = True
    assert check(ctx, x3, records(hot), PEAK, 3, total=tot) == [(BL * (T - 3), BL * (T + 8))]
    # ... held together by single hot rows a tile apart (join_bins = T - 1), and not by one row less
    hot = np.zeros(n, bool)
    hot[[5, T + 5, 2 * T + 5]] = True
    assert check(ctx, x3, records(hot), PEAK._replace(join_bins=T - 1), 3, total=tot) == [(BL * 5, BL * (2 * T + 1))]
    assert len(check(ctx, x3, records(hot), PEAK._replace(join_bins=T - 2), 3, total=tot)) == 3
    # a gap of exactly join_bins across a tile edge, and one of join_bins + 1; at every edge and wave edge nearby
    for join in (0, 1, 2, 5, 70):
        for edge in (T, 2 * T, 3 * T, T + 64):
            for first in range(max(edge - join - 2, 0), edge, 1 if join < 10 else 9):
                hot = np.zeros(n, bool)
                hot[[first, min(first + join + 1, n - 1)]] = True
                ev = check(ctx, x3, records(hot), PEAK._replace(join_bins=join), 4, total=tot, what=(join, edge, first))
                assert len(ev) == 1
                if first + join + 2 < n:
                    hot = np.zeros(n, bool)
                    hot[[first, first + join + 2]] = True
                    assert len(check(ctx, x3, records(hot), PEAK._replace(join_bins=join), 4, total=tot)) == 2
    # padding and min_bins at the edges
    hot = np.zeros(n, bool)
    hot[[T - 1, T, 2 * T - 1, 3 * T]] = True
    for rule in (PEAK._replace(join_bins=4, pad_bins=2), PEAK._replace(join_bins=2, pad_bins=1, min_bins=2),
                 PEAK._replace(join_bins=T, pad_bins=T // 2, max_bins=7)):
        check(ctx, x3, records(hot), rule, 2 * n, total=tot, what=rule)


def test_more_tiles_and_runs_than_threads_of_the_scans(ctx, x3, T):
    """x3_events_count_kernel and x3_events_runs_kernel are one workgroup of 1 024 that walks a run of tiles, or of runs, per
    thread: 1 025 tiles with hot rows at the tile edges (two tiles a thread), 2 049 runs of one row (three runs a thread)"""
    n = 1025 * T
    k = np.arange(n)
    hot = (k % T == 0) | (k % T == T - 1)
    ev = check(ctx, x3, records(hot), PEAK, 1030, total=BL * n, what="1 025 tiles")
    assert len(ev) == 1026                                   # (the first row, 1 024 pairs across an edge, the last row)
    ev = check(ctx, x3, records(hot), PEAK._replace(join_bins=T - 2), 8, total=BL * n, what="1 025 tiles, one run")
    assert len(ev) == 1
    n = 2 * 2049 - 1
    ev = check(ctx, x3, records(np.arange(n) % 2 == 0), PEAK, 2049 + 3, total=BL * n, what="2 049 runs")
    assert len(ev) == 2049


def test_the_mean_square_criterion_at_equality(ctx, x3):
    lv = R.empty(4)
    lv["n"] = [10, 10, 10, 0]
    lv["sum_sq"] = [1000, 999, 10, 10 ** 12]
    lv["min"], lv["max"] = [-9, -9, -200, -9], [9, 9, 9, 9]
    assert check(ctx, x3, lv, E.Rule(mean_sq_min=100), 4, total=16) == [(0, 4)]
    assert check(ctx, x3, lv, E.Rule(mean_sq_min=101), 4, total=16) == []
    assert check(ctx, x3, lv, E.Rule(peak_min=200), 4, total=16) == [(8, 4)]
    assert check(ctx, x3, lv, E.Rule(mean_sq_min=100, peak_min=200), 4, total=16) == [(0, 4), (8, 4)]
    assert check(ctx, x3, lv, E.Rule(mean_sq_min=1 << 30, peak_min=32768), 4, total=16) == []


def test_an_untrusted_total(ctx, x3, T):
    n = T + 1
    hot = np.zeros(n, bool)
    hot[[0, T - 1, T]] = True
    lv = records(hot)
    # more samples than the rows given: the rows given count, the last len is a whole bin
    assert check(ctx, x3, lv, PEAK, 4, total=10 ** 15) == [(0, BL), (BL * (T - 1), 2 * BL)]
    assert check(ctx, x3, lv, PEAK, 4, total=2 ** 64 - 1) == [(0, BL), (BL * (T - 1), 2 * BL)]
    # fewer: the rows behind ceil(total / bin_len) do not count, the last bin is clipped
    assert check(ctx, x3, lv, PEAK, 4, total=BL * T - 1) == [(0, BL), (BL * (T - 1), BL - 1)]
    assert check(ctx, x3, lv, PEAK, 4, total=BL * (T - 1)) == [(0, BL)]
    assert check(ctx, x3, lv, PEAK, 4, total=1) == [(0, 1)]
    assert check(ctx, x3, lv, PEAK, 4, total=0) == []


# ------------------------------------------------------------------------------------------------ corpus form, synthetic
_CORPORA = {}


def layout_corpus(ctx, x3, rows):
    """a corpus whose entry e has rows[e] rows at bin length BL: clips of silence of 4 r - (e % 4) samples; rows 0: an
    entry of no bytes (it has one row all the same) -> (corpus, n_samples)"""
    key = tuple(rows)
    if key not in _CORPORA:
        ns = [max(BL * r - (e % BL), 0) for e, r in enumerate(rows)]
        parts = []
        for n in ns:
            rc, s, _ = O.encode(np.zeros(n, dtype=np.int16)) if n else (0, np.zeros(0, dtype=np.uint8), None)
            assert rc == 0
            parts.append(s)
        offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])[:-1]
        buf = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
        corpus = x3.Corpus(ctx, buf, offs, [p.size for p in parts], seg_blocks=0)
        assert corpus.entries["n_samples"].tolist() == ns
        assert corpus.levels_rows(BL).tolist() == np.concatenate([[0], np.cumsum([max(r, 1) for r in rows])]).tolist()
        _CORPORA[key] = (corpus, ns)
    return _CORPORA[key]


@pytest.fixture(scope="module", autouse=True)
def _close_corpora():
    yield
    for corpus, _ in _CORPORA.values():
        corpus.close()
    _CORPORA.clear()


def test_entries_do_not_join_at_tile_edges(ctx, x3, T):
    for cut in (T - 1, T, T + 1):
        rows = [cut, 2 * T + 1 - cut, 1, 1, 0, 1, T - 3]
        corpus, ns = layout_corpus(ctx, x3, rows)
        n = sum(max(r, 1) for r in rows)
        for hot in (np.ones(n, bool), np.isin(np.arange(n), [cut - 1, cut, 2 * T, 2 * T + 1, 2 * T + 2, 2 * T + 4])):
            for rule in (PEAK, PEAK._replace(join_bins=3, pad_bins=1), PEAK._replace(join_bins=2 * T, pad_bins=T, max_bins=50)):
                # (entry 4 has no samples: the levels call counts nothing into its row, which is then never hot)
                lv = records(hot, empty_at=[2 * T + 3])
                ev = check(ctx, x3, lv, rule, n, corpus=corpus, n_samples=ns, what=(cut, rule))
                ents = [e[0] for e in ev]
                assert 0 in ents and 1 in ents and 4 not in ents
                if rule.max_bins == 0 and hot.all():
                    assert ents == [0, 1, 2, 3, 5, 6]                  # one event an entry: nothing joined across


def test_entries_of_a_single_row(ctx, x3, T):
    rows = [1] * (T + 2)
    corpus, ns = layout_corpus(ctx, x3, rows)
    ev = check(ctx, x3, records(np.ones(T + 2, bool)), PEAK._replace(join_bins=5, pad_bins=2), T + 5, corpus=corpus, n_samples=ns)
    assert [e[0] for e in ev] == list(range(T + 2)) and all(e[1] == 0 for e in ev)
    for cap in (1, T + 1, T + 2):
        check(ctx, x3, records(np.arange(T + 2) % 3 != 1), PEAK, cap, corpus=corpus, n_samples=ns, with_levels=cap != 1)


def test_200_random_cases(ctx, x3, T):
    rng = np.random.default_rng(17)
    layouts = [None, [3 * T + 1], [T, T, T, 1], [T - 1, 2, T + 1, 0, 5], [1, 1, 7, 0, 0, 64, 63, 65, T - 70, 9],
               [int(v) for v in rng.integers(0, 40, 30)], [2 * T + 3, T - 2]]
    for case in range(200):
        lay = layouts[case % len(layouts)]
        join = int(rng.choice([0, 1, 2, 3, 8, 64, T]))
        rule = E.Rule(peak_min=1000 if case % 3 else 0, mean_sq_min=0 if case % 3 else int(rng.integers(1, 10 ** 6)),
                      join_bins=join, min_bins=int(rng.choice([0, 1, 2, 3, 9])), pad_bins=int(rng.integers(0, join // 2 + 1)),
                      max_bins=int(rng.choice([0, 0, 1, 2, 5, 100])))
        if lay is None:
            n = int(rng.integers(1, 3 * T + 2))
        else:
            corpus, ns = layout_corpus(ctx, x3, lay)
            n = sum(max(r, 1) for r in lay)
        hot = rng.random(n) < rng.choice([0.01, 0.1, 0.5, 0.95])
        lv = records(hot, rng, empty_at=np.flatnonzero(rng.random(n) < 0.05))
        if rule.mean_sq_min:       # loud and quiet rows on both sides of, and on, the threshold
            lv["sum_sq"] = (rule.mean_sq_min * lv["n"].astype(np.int64) + np.where(hot, rng.integers(0, 3, n), -1)).astype(np.uint64)
        cap = int(rng.choice([1, 2, 7, n, n + 3]))
        if lay is None:
            tot = int(rng.choice([BL * n, BL * n - 3, BL * (n // 2) + 1, 10 ** 12])) if n > 1 else 3
            check(ctx, x3, lv, rule, cap, total=tot, with_levels=bool(case % 4), what=(case, rule))
        else:
            check(ctx, x3, lv, rule, cap, corpus=corpus, n_samples=ns, with_levels=bool(case % 4), what=(case, rule))


def _device_entry_table(ctx, x3, corpus):
    """the device copy of a corpus's entry table (x3_corpus_entries_dev), believed only if its bytes ARE the entry table"""
    d_ent = corpus.d_entries
    assert d_ent
    back = ctx.download(d_ent, 32 * corpus.n_entries, x3.CORPUS_ENTRY_DTYPE)
    assert back.tobytes() == corpus.entries.tobytes()
    return d_ent


def test_an_entry_table_overwritten_after_the_build(ctx, x3, T):
    """nothing is trusted: whatever the device's entry table says, only the slots of the caller's arrays are written (run()
    brackets every output with canaries), and the rows read are the caller's n_rows"""
    rows = [T - 1, 2, T + 1, 0, 5]
    ns = [max(BL * r - (e % BL), 0) for e, r in enumerate(rows)]
    parts = [O.encode(np.zeros(n, dtype=np.int16))[1] if n else np.zeros(0, dtype=np.uint8) for n in ns]
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])[:-1]
    corpus = x3.Corpus(ctx, np.concatenate(parts), offs, [p.size for p in parts], seg_blocks=0)
    try:
        n = int(corpus.levels_rows(BL)[-1])
        d_ent = _device_entry_table(ctx, x3, corpus)
        rng = np.random.default_rng(3)
        lv = records(rng.random(n) < 0.5)
        for wild in ([0] * 5, [2 ** 64 - 1] * 5, [BL * 10 * n] * 5, [1, 2 ** 63, 7, 2 ** 64 - 5, 3], [BL * n, 0, 0, 0, 0],
                     [2 ** 33, 2 ** 34, 5, 5, 5]):
            tab = corpus.entries.copy()
            tab["n_samples"] = np.array(wild, dtype=np.uint64)
            tab["first_frame"] = rng.integers(0, 2 ** 62, 5)
            ctx.upload(d_ent, tab)
            for rule in (PEAK, PEAK._replace(join_bins=2 * T, pad_bins=T, max_bins=3), PEAK._replace(join_bins=1, max_bins=1)):
                for cap in (1, 5, 2 * n):
                    got = run(ctx, x3, lv, rule, cap, corpus=corpus)
                    assert (got[0] < 5).all()
        # the table as the build left it: the reference again
        ctx.upload(d_ent, corpus.entries)
        check(ctx, x3, lv, PEAK._replace(join_bins=2, pad_bins=1), n, corpus=corpus, n_samples=ns)
    finally:
        corpus.close()


# ------------------------------------------------------------------------------------------------ refusals and states
def test_refusals_enqueue_nothing_and_leave_the_earlier_result(ctx, x3, T):
    L = x3.lib()
    n, cap = T + 1, 8
    lv = records(np.arange(n) % 4 == 0)
    corpus, ns = layout_corpus(ctx, x3, [T, 1])
    d_lv, d_tot = ctx.alloc(32 * n), ctx.alloc(8)
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 32 * cap, 8])
    d_ent, d_st, d_ln, d_el, d_cnt = g.ptr
    try:
        ctx.upload(d_lv, lv)
        ctx.upload(d_tot, np.array([BL * n], dtype=np.uint64))
        good = dict(mean_sq_min=0, peak_min=1000, join_bins=2, min_bins=0, pad_bins=1, max_bins=0, reserved=0)

        def call(c=ctx._h, lv=d_lv, nb=n, bl=BL, tot=d_tot, st=d_st, ln=d_ln, el=d_el, cap=cap, cnt=d_cnt, k="use", ent=d_ent,
                 corpus_form=False, null_rule=False, **rule):
            r = x3.EventRule(**dict(good, **rule))
            rp = None if null_rule else C.byref(r)
            if corpus_form:
                return L.x3_corpus_events_dev(c, corpus._h if k == "use" else k, lv, nb, bl, rp, ent, st, ln, el, cap, cnt)
            return L.x3_events_dev(c, lv, nb, bl, tot, rp, st, ln, el, cap, cnt)

        # an earlier call whose result must survive every refusal
        assert call(cap=3) == 0
        before = [a.copy() for a in g.read()]
        want = len(E.stream_events(lv, BL * n, BL, PEAK._replace(join_bins=2, pad_bins=1))[0])
        refusals = [dict(bl=0), dict(bl=1 << 32), dict(peak_min=0), dict(peak_min=32769), dict(mean_sq_min=(1 << 30) + 1),
                    dict(pad_bins=2), dict(join_bins=0), dict(max_bins=1 << 30, bl=8), dict(max_bins=0xFFFFFFFF, bl=2),
                    dict(reserved=1), dict(cap=0), dict(cap=1 << 31), dict(nb=0), dict(nb=1 << 31), dict(c=None), dict(lv=None),
                    dict(tot=None), dict(st=None), dict(ln=None), dict(cnt=None), dict(null_rule=True), dict(lv=d_lv + 4),
                    dict(tot=d_tot + 4), dict(st=d_st + 4), dict(ln=d_ln + 2), dict(el=d_el + 4), dict(cnt=d_cnt + 4)]
        for bad in refusals:
            assert call(**bad) == BAD, bad
            if "tot" not in bad:                                     # (the corpus form has no d_total)
                assert call(corpus_form=True, **bad) == BAD, ("corpus", bad)
        for bad in (dict(k=None), dict(ent=None), dict(ent=d_ent + 2), dict(nb=n - 1), dict(nb=n + 1)):
            assert call(corpus_form=True, **bad) == BAD, bad
        ctx.graph_begin()
        try:
            assert call() == BAD and call(corpus_form=True) == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass
        ctx.sync()
        after = g.read()
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call wrote"
        assert ctx.events_result() == (0, want)                  # ... and the result is still the earlier call's
        assert ctx.events_result()[0] == BAD                     # read once
        # the limits themselves are fine; d_event_levels may be NULL
        assert call(mean_sq_min=1 << 30, peak_min=32768, el=None) == 0 and ctx.events_result() == (0, 0)
        assert call(max_bins=0xFFFFFFFF // BL) == 0 and ctx.events_result() == (0, want)
        assert call(corpus_form=True) == 0 and ctx.events_result()[0] == 0
    finally:
        g.close()
        ctx.free(d_lv)
        ctx.free(d_tot)


# ------------------------------------------------------------------------------------------------ end to end
def burst_wav(x3, kind, seed, n, bursts):
    """a quiet x3_synth clip with loud bursts (position, length) laid in"""
    w = (x3.synth(kind, seed, 0, n).astype(np.int32) >> 6).astype(np.int16)
    for a, ln in bursts:
        t = np.arange(min(ln, n - a))
        w[a:a + t.size] = (9000 * np.sin(t * 0.37)).astype(np.int16)
    return w


E2E_BIN = 250
E2E_RULE = E.Rule(mean_sq_min=4_000_000, peak_min=8000, join_bins=3, min_bins=0, pad_bins=1, max_bins=6)


def _frames_of(wav, spf):
    return [wav[i:i + spf] for i in range(0, wav.size, spf)]


@pytest.mark.parametrize("bl,bpf,index", [(20, 100, "decode"), (40, 50, "walk")])
def test_levels_events_ranges_back_to_back_on_a_stream(ctx, x3, bl, bpf, index):
    spf, n, cap, stride = bl * bpf, 9_300, 16, 6 * E2E_BIN
    bursts = [(0, 300), (1_990, 30), (2_600, 100), (4_000, 2_600), (9_200, 100)]
    wav = burst_wav(x3, 2, 31, n, bursts)
    p = x3.Params.make(bl, bpf)
    rc, stream, _ = O.encode(wav, O.Params.make(bl, bpf, (0, 1, 3)))
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8, index=index)
    n_bins = R.n_bins_for(n, E2E_BIN)
    d_lv = ctx.alloc(32 * n_bins)
    g = Guarded(ctx, [8 * cap, 4 * cap, 32 * cap, 8, 2 * cap * stride, 4 * cap])
    d_st, d_ln, d_el, d_cnt, d_out, d_status = g.ptr
    try:
        assert ws.n_frames == 5 and (index == "decode" or ws.seg_blocks == 8)
        # no wait between the three calls; the results are read afterwards, each by its own call
        assert ctx.levels_dev(ws.d_x3, ws.x3_len, ws.d_frame_offsets, ws.d_sample_offsets, ws.n_frames, p, E2E_BIN, d_lv, n_bins,
                              None, ws.d_seg_index, ws.seg_blocks) == 0
        assert ws.events_into(d_lv, n_bins, E2E_BIN, rule_of(x3, E2E_RULE), d_st, d_ln, d_el, cap, d_cnt) == 0
        assert ws.ranges_into(d_st, d_ln, cap, stride, d_out, cap * stride, 0, None, d_status) == 0
        assert ctx.decode_ranges_result()[:4] == (0, 0, cap, 0)
        rc, count = ctx.events_result()
        assert rc == 0 and ctx.levels_result() == (0, 0, ws.n_frames, 0)
        st, ln, el, cnt, out, status = g.read()
        st, ln, el, out = st.view(np.uint64), ln.view(np.uint32), el.view(R.LEVEL_DTYPE), out.view(np.int16).reshape(cap, stride)
        lv = R.levels(_frames_of(wav, spf), [0] * ws.n_frames, range(0, n, spf), E2E_BIN, n_bins)
        assert np.array_equal(ctx.download(d_lv, 32 * n_bins, R.LEVEL_DTYPE), lv)
        ev, elv = E.stream_events(lv, n, E2E_BIN, E2E_RULE)
        assert 4 <= len(ev) == count == int(cnt.view(np.uint64)[0]) < cap
        assert any(e[1] == 6 * E2E_BIN for e in ev) and ev[-1][0] + ev[-1][1] == n        # a cut event; the clipped last bin
        _, wst, wln, wlv = E.slots(ev, elv, cap, False)
        assert np.array_equal(st, wst) and np.array_equal(ln, wln) and np.array_equal(el, wlv)
        assert not status.view(np.int32).any()                                            # the filler ranges too
        for i in range(cap):
            a, k = int(st[i]), int(ln[i])
            assert np.array_equal(out[i, :k], wav[a:a + k]) and not out[i, k:].any(), i
        # the mirror: the same tensors, and ranges() takes them as they are
        t_st, t_ln, t_cnt, t_el = ws.events(E2E_BIN, rule_of(x3, E2E_RULE), cap)
        assert t_cnt.dim() == 0 and int(t_cnt) == count and t_st.is_cuda
        assert np.array_equal(t_st.cpu().numpy().view(np.uint64), wst) and np.array_equal(t_ln.cpu().numpy().view(np.uint32), wln)
        assert np.array_equal(x3.event_levels_view(t_el), wlv)
        rows, _, rst = ws.ranges(t_st, t_ln, padded_to=stride)
        assert np.array_equal(rows.cpu().numpy(), out) and not rst.cpu().numpy().any()
        small = ws.events(E2E_BIN, rule_of(x3, E2E_RULE), 2)
        assert int(small[2]) == count and np.array_equal(small[0].cpu().numpy().view(np.uint64), wst[:2])
    finally:
        g.close()
        ctx.free(d_lv)
        ws.close()


@pytest.mark.parametrize("bl,bpf,index", [(20, 100, "decode"), (40, 50, "walk")])
def test_levels_events_ranges_back_to_back_on_a_corpus(ctx, x3, bl, bpf, index):
    """five entries; the middle frame of entry 2 is damaged after encoding: its bins count nothing and stay cold, burst or not"""
    spf, cap, stride = bl * bpf, 24, 6 * E2E_BIN
    sizes = [3_100, 240, 6_000, 2_000, 4_999]
    bursts = [[(500, 700)], [(0, 240)], [(100, 300), (2_300, 900), (4_900, 600)], [], [(1_000, 2_900), (4_800, 199)]]
    clips = [burst_wav(x3, 1 + e % 3, 40 + e, n, b) for e, (n, b) in enumerate(zip(sizes, bursts))]
    p = x3.Params.make(bl, bpf)
    op = O.Params.make(bl, bpf, (0, 1, 3))
    parts = []
    for w in clips:
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        parts.append(s.copy())
    f2 = XC.frame_offsets(parts[2])
    parts[2][f2[1] + 20 + 33] ^= 0x10
    offs = np.concatenate([[0], np.cumsum([q.size for q in parts])])[:-1]
    corpus = x3.Corpus(ctx, np.concatenate(parts), offs, [q.size for q in parts], params=p, seg_blocks=8, index=index)
    rf = corpus.levels_rows(E2E_BIN)
    n_rows = int(rf[-1])
    d_lv, d_fst = ctx.alloc(32 * n_rows), ctx.alloc(4 * corpus.n_frames)
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 32 * cap, 8, 2 * cap * stride, 4 * cap])
    d_ent, d_st, d_ln, d_el, d_cnt, d_out, d_status = g.ptr
    try:
        assert corpus.entries["n_samples"].tolist() == sizes and (index == "decode" or corpus.seg_blocks == 8)
        assert ctx.corpus_levels_dev(corpus, E2E_BIN, d_lv, n_rows, d_fst) == 0
        assert corpus.events_into(d_lv, n_rows, E2E_BIN, rule_of(x3, E2E_RULE), d_ent, d_st, d_ln, d_el, cap, d_cnt) == 0
        assert corpus.ranges_into(d_ent, d_st, d_ln, cap, stride, d_out, cap * stride, 0, None, d_status) == 0
        assert ctx.decode_ranges_result()[:4] == (0, 0, cap, 0)
        rc, count = ctx.events_result()
        bad_frame = int(corpus.entries["first_frame"][2]) + 1
        assert rc == 0 and ctx.levels_result() == (0, 1, bad_frame, CRC)
        ent, st, ln, el, cnt, out, status = g.read()
        ent, st, ln = ent.view(np.uint32), st.view(np.uint64), ln.view(np.uint32)
        el, out = el.view(R.LEVEL_DTYPE), out.view(np.int16).reshape(cap, stride)
        ref_entries = []
        for e, w in enumerate(clips):
            fr = _frames_of(w, spf)
            ref_entries.append((fr, [CRC if (e == 2 and f == 1) else 0 for f in range(len(fr))], range(0, w.size, spf), w.size))
        lv, rf2 = R.corpus_levels(ref_entries, E2E_BIN)
        assert np.array_equal(rf, rf2) and np.array_equal(ctx.download(d_lv, 32 * n_rows, R.LEVEL_DTYPE), lv)
        a = int(rf[2]) + spf // E2E_BIN
        assert not lv["n"][a + 1:a + spf // E2E_BIN - 1].any()              # the damaged frame's bins count nothing
        ev, elv = E.corpus_events(lv, sizes, E2E_BIN, E2E_RULE)
        assert 6 <= len(ev) == count == int(cnt.view(np.uint64)[0]) < cap
        assert {e[0] for e in ev} == {0, 1, 2, 4}
        assert not any(e[0] == 2 and spf + E2E_BIN <= e[1] < 2 * spf - E2E_BIN for e in ev)   # ... and stay cold
        went, wst, wln, wlv = E.slots(ev, elv, cap, True)
        assert np.array_equal(ent, went) and np.array_equal(st, wst) and np.array_equal(ln, wln) and np.array_equal(el, wlv)
        assert not status.view(np.int32).any()
        for i in range(cap):
            e, s0, k = int(ent[i]), int(st[i]), int(ln[i])
            assert np.array_equal(out[i, :k], clips[e][s0:s0 + k]) and not out[i, k:].any(), i
        t_ent, t_st, t_ln, t_cnt, t_el = corpus.events(E2E_BIN, rule_of(x3, E2E_RULE), cap)
        assert int(t_cnt) == count and np.array_equal(t_ent.cpu().numpy().view(np.uint32), went)
        assert np.array_equal(t_st.cpu().numpy().view(np.uint64), wst) and np.array_equal(x3.event_levels_view(t_el), wlv)
        rows, _, rst = corpus.ranges(t_ent, t_st, t_ln, padded_to=stride)
        assert np.array_equal(rows.cpu().numpy(), out) and not rst.cpu().numpy().any()
    finally:
        g.close()
        ctx.free(d_lv)
        ctx.free(d_fst)
        corpus.close()
