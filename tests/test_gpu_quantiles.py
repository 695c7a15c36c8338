"""Level quantiles, thresholds from them and events with a threshold per entry (include/x3hip.h, "LEVEL QUANTILES AND
ADAPTIVE THRESHOLDS"): x3_level_quantiles_dev, x3_level_thresholds_dev, x3_events_adaptive_dev, their corpus forms and
x3_level_quantiles_result.  Every value, count, threshold and event slot is held with == against quantiles_ref.py.  Most
cases upload hand-made level records straight into d_levels (no decode), laid round the kernels' tile (option
"events_tile_rows") and round the digits of the select (8 bits each); the chain cases run levels, thresholds, adaptive events
and ranges back to back on the device with the result calls last."""
import ctypes as C

import numpy as np
import pytest

import events_ref as E
import levels_ref as R
import oracle_lib as O
import quantiles_ref as Q
import x3_cases as XC

pytestmark = pytest.mark.gpu

BAD = 24
CRC = 14
GUARD = 64
CANARY = 0x5A
BL = 4                      # bin length of the synthetic cases: an entry of r rows is a clip of at most 4 r samples
Q8 = [500_000, 0, 1_000_000, 999_999, 500_000, 1, 250_000, 1_000_000]     # unsorted, with duplicates, 0 and 1 000 000


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


def records(peak=None, mean_sq=None, n=None, size=None, rng=None, empty_at=()):
    """hand-made level records: peak[i] as max (as -min where i is odd), mean square mean_sq[i] as sum_sq = mean_sq * n +
    (something below n); nothing counted at `empty_at`, whose other fields stay as they are"""
    size = len(peak) if peak is not None else len(mean_sq) if mean_sq is not None else size
    lv = R.empty(size)
    k = np.arange(size)
    lv["n"] = BL if n is None else n
    peak = np.full(size, 10) if peak is None else np.asarray(peak, dtype=np.int64)
    lv["max"] = np.where(k % 2 == 0, peak, np.minimum(peak, 3))
    lv["min"] = np.where(k % 2 == 0, -np.minimum(peak, 2), -peak)
    ms = np.full(size, 50, dtype=np.uint64) if mean_sq is None else np.asarray(mean_sq, dtype=np.uint64)
    rem = (k % lv["n"].astype(np.int64)).astype(np.uint64) if rng is None else rng.integers(0, lv["n"].astype(np.int64)).astype(np.uint64)
    lv["sum_sq"] = ms * lv["n"].astype(np.uint64) + rem
    lv["sum"] = k
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


class Rows:
    """level records and a sample count on the device"""

    def __init__(self, ctx, lv, total=None):
        self.ctx = ctx
        self.d_lv, self.d_tot = ctx.alloc(32 * lv.size), ctx.alloc(8)
        ctx.upload(self.d_lv, lv)
        ctx.upload(self.d_tot, np.array([0 if total is None else total], dtype=np.uint64))

    def close(self):
        self.ctx.free(self.d_lv)
        self.ctx.free(self.d_tot)


def _empty_summary(counted):
    empty = np.flatnonzero(counted == 0)
    return (0, int(empty.size), int(empty[0]) if empty.size else int(counted.size))


def run_q(ctx, lv, key, q_ppm, total=None, corpus=None):
    """one quantiles call on uploaded records -> (values [n_ent, n_q], counted [n_ent]); the canaries round both outputs
    and the result call are checked"""
    n_ent = 1 if corpus is None else corpus.n_entries
    rows = Rows(ctx, lv, total)
    g = Guarded(ctx, [4 * n_ent * len(q_ppm), 4 * n_ent])
    try:
        if corpus is None:
            rc = ctx.level_quantiles_dev(rows.d_lv, lv.size, BL, rows.d_tot, key, q_ppm, g.ptr[0], g.ptr[1])
        else:
            rc = corpus.level_quantiles_into(rows.d_lv, lv.size, BL, key, q_ppm, g.ptr[0], g.ptr[1])
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.level_quantiles_result()
        values, counted = g.read()
    finally:
        g.close()
        rows.close()
    values, counted = values.view(np.uint32).reshape(n_ent, len(q_ppm)), counted.view(np.uint32)
    assert res == _empty_summary(counted), (res, counted[:8])
    return values, counted


def check_q(ctx, lv, key, q_ppm, total=None, corpus=None, n_samples=None, what=None):
    values, counted = run_q(ctx, lv, key, q_ppm, total=total, corpus=corpus)
    if corpus is None:
        wv, wk = Q.stream_quantiles(lv, total, BL, key, q_ppm)
    else:
        wv, wk = Q.corpus_quantiles(lv, n_samples, BL, key, q_ppm)
    assert np.array_equal(counted, wk), (what, np.flatnonzero(counted != wk)[:5], counted[:8], wk[:8])
    assert np.array_equal(values, wv), (what, np.argwhere(values != wv)[:5], values[:4], wv[:4])
    return values, counted


def run_thr(ctx, x3, lv, trule, total=None, corpus=None):
    """one thresholds call -> [(mean_sq_min, peak_min, counted)] per entry"""
    n_ent = 1 if corpus is None else corpus.n_entries
    rows = Rows(ctx, lv, total)
    g = Guarded(ctx, [16 * n_ent])
    try:
        r = x3.ThresholdRule.make(trule.peak, trule.mean_sq)
        if corpus is None:
            rc = ctx.level_thresholds_dev(rows.d_lv, lv.size, BL, rows.d_tot, r, g.ptr[0])
        else:
            rc = corpus.level_thresholds_into(rows.d_lv, lv.size, BL, r, g.ptr[0])
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.level_quantiles_result()
        thr = g.read()[0].view(x3.EVENT_THRESHOLD_DTYPE)
    finally:
        g.close()
        rows.close()
    assert res == _empty_summary(thr["counted"])
    return [tuple(int(v) for v in t) for t in thr.tolist()]


def check_thr(ctx, x3, lv, trule, total=None, corpus=None, n_samples=None, what=None):
    got = run_thr(ctx, x3, lv, trule, total=total, corpus=corpus)
    want = Q.stream_thresholds(lv, total, BL, trule) if corpus is None else Q.corpus_thresholds(lv, n_samples, BL, trule)
    assert got == want, (what, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:4])
    return got


def thr_array(x3, thrs):
    a = np.zeros(len(thrs), dtype=x3.EVENT_THRESHOLD_DTYPE)
    for i, t in enumerate(thrs):
        a[i] = (t[0], t[1], t[2] if len(t) > 2 else 0xABCD0000 + i)         # (counted is ignored: anything)
    return a


def run_ev(ctx, x3, lv, rule, cap, thrs=None, total=None, corpus=None, with_levels=True):
    """one events call, adaptive when thrs is given -> (entries or None, starts, lens, event levels or None, count)"""
    rows = Rows(ctx, lv, total)
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 32 * cap, 8] + ([16 * len(thrs)] if thrs is not None else []))
    try:
        d_ent, d_st, d_ln, d_el, d_cnt = g.ptr[:5]
        d_el = d_el if with_levels else None
        r = x3.EventRule.make(*rule)
        if thrs is not None:
            ctx.upload(g.ptr[5], thr_array(x3, thrs))
            if corpus is None:
                rc = ctx.events_adaptive_dev(rows.d_lv, lv.size, BL, rows.d_tot, r, g.ptr[5], d_st, d_ln, d_el, cap, d_cnt)
            else:
                rc = corpus.adaptive_events_into(rows.d_lv, lv.size, BL, r, g.ptr[5], d_ent, d_st, d_ln, d_el, cap, d_cnt)
        elif corpus is None:
            rc = ctx.events_dev(rows.d_lv, lv.size, BL, rows.d_tot, r, d_st, d_ln, d_el, cap, d_cnt)
        else:
            rc = corpus.events_into(rows.d_lv, lv.size, BL, r, d_ent, d_st, d_ln, d_el, cap, d_cnt)
        assert rc == 0, (rc, ctx.last_error())
        res = ctx.events_result()
        out = g.read()
    finally:
        g.close()
        rows.close()
    ent, st, ln, el, cnt = out[:5]
    cnt = int(cnt.view(np.uint64)[0])
    assert res == (0, cnt), (res, cnt)
    if thrs is not None:
        assert np.array_equal(out[5].view(x3.EVENT_THRESHOLD_DTYPE), thr_array(x3, thrs)), "d_thr is read-only"
    if corpus is None:
        assert (ent == CANARY).all(), "a stream call has no entries to write"
    return (ent.view(np.uint32) if corpus is not None else None, st.view(np.uint64), ln.view(np.uint32),
            el.view(R.LEVEL_DTYPE) if with_levels else None, cnt)


def same_slots(got, ev, elv, cap, with_entries, what=None):
    ent, st, ln, sl = E.slots(ev, elv, cap, with_entries)
    assert got[4] == len(ev), (what, got[4], len(ev))
    if with_entries:
        assert np.array_equal(got[0], ent), (what, np.flatnonzero(got[0] != ent)[:5])
    assert np.array_equal(got[1], st), (what, np.flatnonzero(got[1] != st)[:5], got[1][:8], st[:8])
    assert np.array_equal(got[2], ln), (what, np.flatnonzero(got[2] != ln)[:5], got[2][:8], ln[:8])
    if got[3] is not None:
        for k in R.LEVEL_DTYPE.names:
            assert np.array_equal(got[3][k], sl[k]), (what, k, np.flatnonzero(got[3][k] != sl[k])[:5])


def check_adaptive(ctx, x3, lv, thrs, rule, cap, total=None, corpus=None, n_samples=None, what=None):
    got = run_ev(ctx, x3, lv, rule, cap, thrs=thrs, total=total, corpus=corpus)
    if corpus is None:
        ev, elv = Q.stream_adaptive_events(lv, total, BL, thrs[0], rule)
    else:
        ev, elv = Q.corpus_adaptive_events(lv, n_samples, BL, thrs, rule)
    same_slots(got, ev, elv, cap, corpus is not None, what)
    return ev


# ------------------------------------------------------------------------------------------------ stream form
def row_counts(T):
    return [1, T - 1, T, T + 1, 2 * T + 1]


def test_stream_row_counts_and_totals(ctx, T):
    rng = np.random.default_rng(1)
    for n in row_counts(T):
        peak, ms = rng.integers(0, 32769, n), rng.integers(0, (1 << 30) + 1, n)
        lv = records(peak=peak, mean_sq=ms, rng=rng, empty_at=np.flatnonzero(rng.random(n) < 0.1))
        for total in sorted({0, 1, BL * n - 1, BL * n, BL * (n // 2) + 1, BL * n - BL, BL * n + 1, 10 ** 15, 2 ** 64 - 1}):
            for key in (Q.PEAK, Q.MEAN_SQ):
                for q_ppm in ([500_000], Q8):
                    _, k = check_q(ctx, lv, key, q_ppm, total=total, what=(n, total, key, len(q_ppm)))
                    assert int(k[0]) <= min(n, -(-total // BL))


def test_key_patterns(ctx, T):
    n = 2 * T + 1
    k = np.arange(n)
    qs = [0, 1_000_000, 500_000, 333_333, 999_999]

    def both(peak, ms, **kw):
        lv = records(peak=peak, mean_sq=ms, **kw)
        return (check_q(ctx, lv, Q.PEAK, qs, total=BL * n)[0][0].tolist(), check_q(ctx, lv, Q.MEAN_SQ, qs, total=BL * n)[0][0].tolist())

    # all equal
    assert both(np.full(n, 1234), np.full(n, 77_777)) == ([1234] * 5, [77_777] * 5)
    assert both(np.zeros(n), np.zeros(n)) == ([0] * 5, [0] * 5)
    # differing in the lowest digit only, and in the highest only
    p, m = both(0x1200 + k % 256, 0x12345600 + k % 256)
    assert p[:2] == [0x1200, 0x12FF] and m[:2] == [0x12345600, 0x123456FF]
    p, m = both((k % 128) << 8 | 0x5A, (k % 64) << 24 | 0x5A5A5A)
    assert p[:2] == [0x5A, 0x7F5A] and m[:2] == [0x5A5A5A, 0x3F5A5A5A]
    # two values either side of every digit boundary
    for hi in (1 << 8, 1 << 15, 1 << 16, 1 << 24, 1 << 30):
        pk = min(hi, 32768)
        p, m = both(np.where(k % 2 == 0, pk - 1, pk), np.where(k % 3 == 0, hi - 1, hi))
        assert p[:3] == [pk - 1, pk, pk - 1] and m[:3] == [hi - 1, hi, hi]
    # the maxima: min = -32768 alone gives the peak 32768; every sample -32768 gives sum_sq = 2^30 n
    lv = records(peak=np.full(n, 7), mean_sq=np.full(n, 1 << 30))
    lv["min"][1::2] = -32768
    lv["sum_sq"] = (1 << 30) * lv["n"].astype(np.uint64)
    assert check_q(ctx, lv, Q.PEAK, qs, total=BL * n)[0][0].tolist() == [7, 32768, 7, 7, 32768]
    assert check_q(ctx, lv, Q.MEAN_SQ, qs, total=BL * n)[0][0].tolist() == [1 << 30] * 5
    # n differing row to row: floor(sum_sq / n) orders differently from sum_sq
    rng = np.random.default_rng(2)
    nn = rng.integers(1, 2000, n)
    lv = records(mean_sq=rng.integers(0, 5000, n), n=nn, rng=rng)
    assert not np.array_equal(np.argsort(lv["sum_sq"], kind="stable"), np.argsort(lv["sum_sq"] // lv["n"], kind="stable"))
    check_q(ctx, lv, Q.MEAN_SQ, Q8, total=BL * n)
    # over-limit hand-made keys are clamped, a negative peak is 0
    lv = records(peak=np.full(n, 5), mean_sq=np.full(n, 9))
    lv["max"][::3], lv["min"][1::3] = 70_000, -(2 ** 31)
    lv["max"][2::3], lv["min"][2::3] = -4, 6
    lv["sum_sq"][::2] = 2 ** 64 - 1
    assert check_q(ctx, lv, Q.PEAK, [0, 1_000_000], total=BL * n)[0][0].tolist() == [0, 32768]
    assert check_q(ctx, lv, Q.MEAN_SQ, [0, 1_000_000], total=BL * n)[0][0].tolist() == [9, 1 << 30]


# ------------------------------------------------------------------------------------------------ corpus form
_CORPORA = {}


def layout_corpus(ctx, x3, rows):
    """a corpus whose entry e has rows[e] rows at bin length BL: clips of silence of 4 r - (e % 4) samples; rows 0: an
    entry of no bytes (it has one row all the same) -> (corpus, n_samples)"""
    key = tuple(rows)
    if key not in _CORPORA:
        ns = [max(BL * r - (e % BL), 0) for e, r in enumerate(rows)]
        enc = {}
        for n in set(ns):
            rc, s, _ = O.encode(np.zeros(n, dtype=np.int16)) if n else (0, np.zeros(0, dtype=np.uint8), None)
            assert rc == 0
            enc[n] = s
        parts = [enc[n] for n in ns]
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


def n_rows_of(lay):
    return sum(max(r, 1) for r in lay)


def first_rows(lay):
    return np.concatenate([[0], np.cumsum([max(r, 1) for r in lay])]).astype(int)


def test_corpus_layouts_round_the_tile(ctx, x3, T):
    rng = np.random.default_rng(3)
    layouts = [[1] * (3 * T),                                  # every tile holds many entries
               [T - 5, 10, T - 10, 7, T // 2, 3, T],           # entries that begin and end inside a tile
               [1, 3 * T - 2, 1, 1],                           # one entry over three tiles, neighbours of one row
               [T, T, 2 * T], [T - 1, T + 1, 1, 0, 5]]
    for lay in layouts:
        corpus, ns = layout_corpus(ctx, x3, lay)
        n = n_rows_of(lay)
        lv = records(peak=rng.integers(0, 32769, n), mean_sq=rng.integers(0, 1 << 20, n), rng=rng)
        for e in np.flatnonzero(np.asarray(lay) == 0):          # (an entry of no samples: the levels call counts nothing)
            lv["n"][first_rows(lay)[e]] = 0
        for key in (Q.PEAK, Q.MEAN_SQ):
            for q_ppm in ([1_000_000], Q8):
                check_q(ctx, lv, key, q_ppm, corpus=corpus, n_samples=ns, what=(lay[:4], key))
        check_thr(ctx, x3, lv, Q.TRule(peak=(998_000, 1, 1, 1), mean_sq=(500_000, 4, 1, 0)), corpus=corpus, n_samples=ns)


def test_entries_whose_rows_count_nothing(ctx, x3, T):
    lay = [T - 5, 10, T - 10, 7, T // 2, 3, T]
    corpus, ns = layout_corpus(ctx, x3, lay)
    n, rf = n_rows_of(lay), first_rows(lay)
    rng = np.random.default_rng(4)
    for dead in ([0], [2], [6], [0, 3, 6], list(range(7))):      # at the front, in the middle, last; all
        rows = np.concatenate([np.arange(rf[e], rf[e + 1]) for e in dead])
        lv = records(peak=rng.integers(1, 30_000, n), mean_sq=rng.integers(1, 1 << 29, n), rng=rng, empty_at=rows)
        for key in (Q.PEAK, Q.MEAN_SQ):
            v, k = check_q(ctx, lv, key, Q8, corpus=corpus, n_samples=ns, what=("dead", dead, key))
            assert [e for e in range(7) if k[e] == 0] == dead and not v[dead].any()
        thr = check_thr(ctx, x3, lv, Q.TRule(peak=(500_000, 2, 1, 0), mean_sq=(900_000, 1, 2, 3)), corpus=corpus, n_samples=ns)
        assert all(thr[e] == (0, 0, 0) for e in dead)


def test_200_random_cases(ctx, x3, T):
    rng = np.random.default_rng(18)
    layouts = [None, [2 * T + 1], [T, T, 1], [T - 1, 2, T + 1, 0, 5], [1, 1, 7, 0, 0, 64, 63, 65, T - 70, 9],
               [int(v) for v in rng.integers(0, 40, 30)], [T + 3, T - 2]]
    for case in range(200):
        lay = layouts[case % len(layouts)]
        n = int(rng.integers(1, 2 * T + 2)) if lay is None else n_rows_of(lay)
        spread = int(rng.choice([2, 300, 32769]))
        peak = rng.integers(0, spread, n) + int(rng.integers(0, 32769 - spread + 1))
        top = int(rng.choice([3, 1 << 9, 1 << 17, 1 << 30]))
        ms = rng.integers(0, top + 1, n)
        nn = rng.integers(1, 500, n) if case % 2 else None
        lv = records(peak=peak, mean_sq=ms, n=nn, rng=rng, empty_at=np.flatnonzero(rng.random(n) < rng.choice([0, 0.05, 0.6])))
        key = int(case % 3 == 0)
        q_ppm = [int(v) for v in rng.integers(0, 1_000_001, int(rng.integers(1, 9)))]
        if case % 5 == 0:
            q_ppm[0] = int(rng.choice([0, 1_000_000]))
        trule = Q.TRule(peak=(q_ppm[0], int(rng.integers(0, 5)), int(rng.integers(1, 4)), int(rng.integers(0, 50))) if case % 4 else None,
                        mean_sq=(q_ppm[-1], int(rng.integers(0, 2 ** 32)), int(rng.integers(1, 2 ** 32)), int(rng.integers(0, 9)))
                        if case % 4 != 1 else None)
        if lay is None:
            tot = int(rng.choice([BL * n, BL * n - 3, BL * (n // 2) + 1, 10 ** 12])) if n > 1 else 3
            check_q(ctx, lv, key, q_ppm, total=tot, what=(case, key, q_ppm))
            check_thr(ctx, x3, lv, trule, total=tot, what=(case, trule))
        else:
            corpus, ns = layout_corpus(ctx, x3, lay)
            for e in np.flatnonzero(np.asarray(lay) == 0):
                lv["n"][first_rows(lay)[e]] = 0
            check_q(ctx, lv, key, q_ppm, corpus=corpus, n_samples=ns, what=(case, key, q_ppm))
            check_thr(ctx, x3, lv, trule, corpus=corpus, n_samples=ns, what=(case, trule))


def _device_entry_table(ctx, x3, corpus):
    """the device copy of a corpus's entry table (x3_corpus_entries_dev), believed only if its bytes ARE the entry table"""
    d_ent = corpus.d_entries
    assert d_ent
    back = ctx.download(d_ent, 32 * corpus.n_entries, x3.CORPUS_ENTRY_DTYPE)
    assert back.tobytes() == corpus.entries.tobytes()
    return d_ent


def test_an_entry_table_overwritten_after_the_build(ctx, x3, T):
    """nothing is trusted: whatever the device's entry table says, the values are the reference's on THAT table, only the
    callers' n_entries slots are written (canaries), and the rows read are the caller's n_rows"""
    rows = [T - 1, 2, T + 1, 0, 5]
    ns = [max(BL * r - (e % BL), 0) for e, r in enumerate(rows)]
    parts = [O.encode(np.zeros(n, dtype=np.int16))[1] if n else np.zeros(0, dtype=np.uint8) for n in ns]
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])])[:-1]
    corpus = x3.Corpus(ctx, np.concatenate(parts), offs, [p.size for p in parts], seg_blocks=0)
    try:
        n = int(corpus.levels_rows(BL)[-1])
        d_ent = _device_entry_table(ctx, x3, corpus)
        rng = np.random.default_rng(3)
        lv = records(peak=rng.integers(0, 32769, n), mean_sq=rng.integers(0, 1 << 30, n), rng=rng,
                     empty_at=np.flatnonzero(rng.random(n) < 0.1))
        trule = Q.TRule(peak=(990_000, 1, 1, 1), mean_sq=(500_000, 3, 2, 0))
        thrs = [(1 << 20, 9000), (0, 20_000), (1 << 29, 0), (5, 5), (1 << 28, 30_000)]
        for wild in ([0] * 5,                                    # five entries of one row: the rest belongs to none
                     [2 ** 64 - 1] * 5,                          # a prefix that wraps
                     [BL * 10 * n] * 5,                          # entries moved past n_rows
                     [1, 2 ** 63, 7, 2 ** 64 - 5, 3], [BL * n, 0, 0, 0, 0], [2 ** 33, 2 ** 34, 5, 5, 5],
                     [0, 0, BL * 20, 0, BL * (n - 20)], [BL * 3, BL * 3, 2 ** 64 - BL * 5, BL * 40, BL * 7]):
            tab = corpus.entries.copy()
            tab["n_samples"] = np.array(wild, dtype=np.uint64)
            tab["first_frame"] = rng.integers(0, 2 ** 62, 5)
            ctx.upload(d_ent, tab)
            for key in (Q.PEAK, Q.MEAN_SQ):
                check_q(ctx, lv, key, Q8, corpus=corpus, n_samples=wild, what=("wild", wild, key))
            check_thr(ctx, x3, lv, trule, corpus=corpus, n_samples=wild, what=("wild", wild))
            for cap in (1, 2 * n):
                got = run_ev(ctx, x3, lv, E.Rule(join_bins=2, pad_bins=1, max_bins=3), cap, thrs=thrs, corpus=corpus)
                assert (got[0] < 5).all()
        # the table as the build left it: the reference again
        ctx.upload(d_ent, corpus.entries)
        check_q(ctx, lv, Q.MEAN_SQ, Q8, corpus=corpus, n_samples=ns)
        check_adaptive(ctx, x3, lv, thrs, E.Rule(join_bins=2, pad_bins=1), n, corpus=corpus, n_samples=ns)
    finally:
        corpus.close()


# ------------------------------------------------------------------------------------------------ thresholds
def test_the_map_clamps_and_floors(ctx, x3, T):
    n = T + 1
    lv = records(peak=np.full(n, 20), mean_sq=np.full(n, 200))
    med = 500_000
    cases = [(Q.TRule(peak=(med, 3, 2, 1)), (0, 31, n)), (Q.TRule(peak=(med, 1, 3, 0)), (0, 6, n)),
             (Q.TRule(peak=(med, 0, 1, 0)), (0, 1, n)), (Q.TRule(peak=(med, 1, 21, 0)), (0, 1, n)),
             (Q.TRule(peak=(med, 2000, 1, 0)), (0, 32768, n)), (Q.TRule(peak=(med, 1, 1, 2 ** 32 - 1)), (0, 32768, n)),
             (Q.TRule(peak=(med, 2 ** 32 - 1, 2 ** 32 - 1, 0)), (0, 20, n)),
             (Q.TRule(mean_sq=(med, 4, 1, 0)), (800, 0, n)), (Q.TRule(mean_sq=(med, 2 ** 32 - 1, 1, 2 ** 32 - 1)), (1 << 30, 0, n)),
             (Q.TRule(mean_sq=(med, 7, 2, 5)), (705, 0, n)), (Q.TRule(peak=(0, 1, 1, 0), mean_sq=(1_000_000, 1, 1, 0)), (200, 20, n)),
             (Q.TRule(peak=(med, 1, 0, 9), mean_sq=(med, 1, 1, 0)), (200, 0, n))]
    for trule, want in cases:
        assert check_thr(ctx, x3, lv, trule, total=BL * n, what=trule) == [want]
    big = records(peak=np.full(n, 32768), mean_sq=np.full(n, 1 << 30))
    big["sum_sq"] = (1 << 30) * big["n"].astype(np.uint64)
    assert check_thr(ctx, x3, big, Q.TRule(peak=(med, 2 ** 32 - 1, 1, 0), mean_sq=(med, 2 ** 32 - 1, 2 ** 32 - 1, 0)),
                     total=BL * n) == [(1 << 30, 32768, n)]
    assert check_thr(ctx, x3, lv, Q.TRule(peak=(med, 1, 1, 5), mean_sq=(med, 1, 1, 5)), total=0) == [(0, 0, 0)]


# ------------------------------------------------------------------------------------------------ adaptive events
def loud_records(hot, rng=None, empty_at=()):
    """records loud where `hot` is set (peak 1500 + i % 7, mean square 750 000) and quiet elsewhere (peak 10, 50)"""
    hot = np.asarray(hot, dtype=bool)
    k = np.arange(hot.size)
    return records(peak=np.where(hot, 1500 + k % 7, 10), mean_sq=np.where(hot, 750_000, 50), rng=rng, empty_at=empty_at)


def test_equal_thresholds_are_the_events_call(ctx, x3, T):
    rng = np.random.default_rng(6)
    lay = [T - 1, T + 1, 1, 0, 5, 2 * T]
    corpus, ns = layout_corpus(ctx, x3, lay)
    n = n_rows_of(lay)
    for m, p in ((0, 1000), (700_000, 0), (750_000, 1503), (1 << 30, 32768)):
        lv = loud_records(rng.random(n) < 0.3, rng, empty_at=np.flatnonzero(rng.random(n) < 0.05))
        for rule in (E.Rule(), E.Rule(join_bins=3, pad_bins=1, min_bins=2), E.Rule(join_bins=2 * T, pad_bins=T, max_bins=7)):
            for cap in (3, n):
                plain = run_ev(ctx, x3, lv, rule._replace(mean_sq_min=m, peak_min=p), cap, corpus=corpus)
                adaptive = run_ev(ctx, x3, lv, rule, cap, thrs=[(m, p)] * len(lay), corpus=corpus)
                for a, b in zip(plain[:4], adaptive[:4]):
                    assert a.tobytes() == b.tobytes()                 # fillers included
                assert plain[4] == adaptive[4]
        tot = BL * n - 2
        plain = run_ev(ctx, x3, lv, E.Rule(mean_sq_min=m, peak_min=p, join_bins=1), n, total=tot)
        adaptive = run_ev(ctx, x3, lv, E.Rule(join_bins=1), n, thrs=[(m, p)], total=tot)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[1:4], adaptive[1:4])) and plain[4] == adaptive[4]


def test_thresholds_per_entry(ctx, x3, T):
    rng = np.random.default_rng(7)
    lay = [T - 1, T + 1, 1, 0, 5, 2 * T, 9]
    corpus, ns = layout_corpus(ctx, x3, lay)
    n = n_rows_of(lay)
    lv = records(peak=rng.integers(0, 3000, n), mean_sq=rng.integers(0, 1 << 21, n), rng=rng,
                 empty_at=np.flatnonzero(rng.random(n) < 0.05))
    # over-limit values, both zero, one criterion zero, the limits themselves
    thrs = [(1 << 20, 2500), (0, 0), ((1 << 30) + 1, 32769), (2 ** 64 - 1, 2 ** 32 - 1), (0, 1500), (1 << 19, 0), (1 << 30, 32768)]
    for rule in (E.Rule(), E.Rule(join_bins=4, pad_bins=2), E.Rule(join_bins=1, min_bins=2, max_bins=3)):
        for cap in (2, n + 1):
            ev = check_adaptive(ctx, x3, lv, thrs, rule, cap, corpus=corpus, n_samples=ns, what=(rule, cap))
            assert {e[0] for e in ev} <= {0, 4, 5} and {0, 5} <= {e[0] for e in ev}
    # an over-limit value switches ITS criterion off, not the other one
    ev = check_adaptive(ctx, x3, lv, [((1 << 30) + 1, 1500)] * 7, E.Rule(), n, corpus=corpus, n_samples=ns)
    assert ev == Q.corpus_adaptive_events(lv, ns, BL, [(0, 1500)] * 7, E.Rule())[0] and len(ev) > 3
    # the stream form reads one record
    for thr in ((1 << 20, 0), (0, 2900), (0, 0), (2 ** 63, 40_000)):
        check_adaptive(ctx, x3, lv, [thr], E.Rule(join_bins=1), n, total=BL * n - 1)


def test_equality_at_the_mean_square_threshold(ctx, x3):
    lv = R.empty(4)
    lv["n"] = [10, 10, 10, 0]
    lv["sum_sq"] = [1000, 999, 10, 10 ** 12]
    lv["min"], lv["max"] = [-9, -9, -200, -9], [9, 9, 9, 9]
    rule = E.Rule()
    assert check_adaptive(ctx, x3, lv, [(100, 0)], rule, 4, total=16) == [(0, 4)]
    assert check_adaptive(ctx, x3, lv, [(101, 0)], rule, 4, total=16) == []
    assert check_adaptive(ctx, x3, lv, [(0, 200)], rule, 4, total=16) == [(8, 4)]
    assert check_adaptive(ctx, x3, lv, [(0, 201)], rule, 4, total=16) == []
    assert check_adaptive(ctx, x3, lv, [(100, 200)], rule, 4, total=16) == [(0, 4), (8, 4)]
    # the thresholds call's own value is the largest one that keeps the row hot
    lv2 = lv[:1].copy()
    thr = check_thr(ctx, x3, lv2, Q.TRule(mean_sq=(0, 1, 1, 0)), total=4)
    assert thr == [(100, 0, 1)]


def test_entries_meeting_at_a_tile_edge_keep_their_own_thresholds(ctx, x3, T):
    for cut in (T - 1, T, T + 1):
        lay = [cut, 2 * T + 1 - cut, 3]
        corpus, ns = layout_corpus(ctx, x3, lay)
        n = n_rows_of(lay)
        peak = np.full(n, 10)
        peak[cut - 2:cut] = 500                  # the last rows of entry 0: hot under entry 1's threshold, not its own
        peak[cut:cut + 2] = 2000                 # the first rows of entry 1: hot under both
        peak[n - 3:] = 500                       # entry 2: hot under its own
        lv = records(peak=peak)
        thrs = [(0, 1000), (0, 400), (0, 500)]
        for rule in (E.Rule(), E.Rule(join_bins=4, pad_bins=1)):
            ev = check_adaptive(ctx, x3, lv, thrs, rule, 8, corpus=corpus, n_samples=ns, what=(cut, rule))
            assert [e[0] for e in ev] == [1, 2] and ev[0][1] == 0 and ev[0][2] == BL * (2 + rule.pad_bins)
        ev = check_adaptive(ctx, x3, lv, [(0, 400), (0, 2001), (0, 501)], E.Rule(), 8, corpus=corpus, n_samples=ns)
        assert ev == [(0, BL * (cut - 2), ns[0] - BL * (cut - 2))]


# ------------------------------------------------------------------------------------------------ the chain on real data
CH_BIN = 250
CH_TRULE = Q.TRule(mean_sq=(500_000, 16, 1, 0))                     # 12 dB over the entry's median mean square
CH_RULE = E.Rule(join_bins=3, pad_bins=1)
CH_GLOBAL = CH_RULE._replace(mean_sq_min=40_000)
CH_GAINS = [1, 4, 16, 64]
CH_BURSTS = [[(700, 500), (4_100, 900)], [(250, 250), (2_500, 750), (5_250, 500)], [(500, 1_000), (4_500, 750)], [(3_000, 1_500)]]
CH_SIZES = [5_900, 6_000, 6_000, 5_555]


def gain_clip(e):
    """noise of +-8 and bursts of a sine of amplitude 100, times the clip's gain"""
    rng = np.random.default_rng(100 + e)
    w = rng.integers(-8, 9, CH_SIZES[e]).astype(np.int32)
    for a, ln in CH_BURSTS[e]:
        w[a:a + ln] = (100 * np.sin(np.arange(ln) * 0.37)).astype(np.int32)
    return (w * CH_GAINS[e]).astype(np.int16)


def _frames_of(wav, spf):
    return [wav[i:i + spf] for i in range(0, wav.size, spf)]


@pytest.mark.parametrize("bl,bpf,index", [(20, 100, "decode"), (40, 50, "walk")])
def test_levels_thresholds_adaptive_events_ranges_back_to_back(ctx, x3, bl, bpf, index):
    """four clips at gains 1 .. 64; the middle frame of clip 2 (no burst in it) is damaged after encoding"""
    spf, cap, stride = bl * bpf, 16, 8 * CH_BIN
    clips = [gain_clip(e) for e in range(4)]
    p, op = x3.Params.make(bl, bpf), O.Params.make(bl, bpf, (0, 1, 3))
    parts = []
    for w in clips:
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        rc, back, _, errs = O.decode_stream(s, op)
        assert rc == 0 and errs == 0 and np.array_equal(back, w)          # the oracle's samples are the clip's
        parts.append(s.copy())
    f2 = XC.frame_offsets(parts[2])
    parts[2][f2[1] + 20 + 33] ^= 0x10
    offs = np.concatenate([[0], np.cumsum([q.size for q in parts])])[:-1]
    corpus = x3.Corpus(ctx, np.concatenate(parts), offs, [q.size for q in parts], params=p, seg_blocks=8, index=index)
    rf = corpus.levels_rows(CH_BIN)
    n_rows = int(rf[-1])
    d_lv = ctx.alloc(32 * n_rows)
    g = Guarded(ctx, [16 * 4, 4 * cap, 8 * cap, 4 * cap, 32 * cap, 8, 2 * cap * stride, 4 * cap])
    d_thr, d_ent, d_st, d_ln, d_el, d_cnt, d_out, d_status = g.ptr
    try:
        assert corpus.entries["n_samples"].tolist() == CH_SIZES
        # no wait between the four calls; the results are read afterwards, each by its own call
        assert ctx.corpus_levels_dev(corpus, CH_BIN, d_lv, n_rows, None) == 0
        assert corpus.level_thresholds_into(d_lv, n_rows, CH_BIN, x3.ThresholdRule.make(mean_sq=CH_TRULE.mean_sq), d_thr) == 0
        assert corpus.adaptive_events_into(d_lv, n_rows, CH_BIN, x3.EventRule.make(*CH_RULE), d_thr, d_ent, d_st, d_ln, d_el, cap,
                                           d_cnt) == 0
        assert corpus.ranges_into(d_ent, d_st, d_ln, cap, stride, d_out, cap * stride, 0, None, d_status) == 0
        assert ctx.decode_ranges_result()[:4] == (0, 0, cap, 0)
        rc, count = ctx.events_result()
        assert rc == 0 and ctx.level_quantiles_result() == (0, 0, 4)
        bad_frame = int(corpus.entries["first_frame"][2]) + 1
        assert ctx.levels_result() == (0, 1, bad_frame, CRC)
        thr, ent, st, ln, el, cnt, out, status = g.read()
        thr = [tuple(int(v) for v in t) for t in thr.view(x3.EVENT_THRESHOLD_DTYPE).tolist()]
        ent, st, ln = ent.view(np.uint32), st.view(np.uint64), ln.view(np.uint32)
        el, out = el.view(R.LEVEL_DTYPE), out.view(np.int16).reshape(cap, stride)
        # the reference, on the clips' samples
        ref_entries = []
        for e, w in enumerate(clips):
            fr = _frames_of(w, spf)
            ref_entries.append((fr, [CRC if (e == 2 and f == 1) else 0 for f in range(len(fr))], range(0, w.size, spf), w.size))
        lv, rf2 = R.corpus_levels(ref_entries, CH_BIN)
        assert np.array_equal(rf, rf2) and np.array_equal(ctx.download(d_lv, 32 * n_rows, R.LEVEL_DTYPE), lv)
        want_thr = Q.corpus_thresholds(lv, CH_SIZES, CH_BIN, CH_TRULE)
        assert thr == want_thr
        assert want_thr[2][2] == int(rf[3] - rf[2]) - spf // CH_BIN               # the damaged frame's bins do not count
        assert all(want_thr[e][0] < want_thr[e + 1][0] for e in range(3))         # four noise floors, four thresholds
        ev, elv = Q.corpus_adaptive_events(lv, CH_SIZES, CH_BIN, want_thr, CH_RULE)
        assert len(ev) == count == int(cnt.view(np.uint64)[0]) < cap
        went, wst, wln, wlv = E.slots(ev, elv, cap, True)
        assert np.array_equal(ent, went) and np.array_equal(st, wst) and np.array_equal(ln, wln) and np.array_equal(el, wlv)
        # the adaptive call finds the bursts of every clip, and nothing else
        for e in range(4):
            mine = [(s0, k) for (en, s0, k) in ev if en == e]
            assert len(mine) == len(CH_BURSTS[e]), (e, mine)
            for (s0, k), (a, bn) in zip(mine, CH_BURSTS[e]):
                assert s0 <= a and a + bn <= s0 + k <= a + bn + 2 * CH_BIN and a - s0 <= 2 * CH_BIN, (e, s0, k, a, bn)
        assert not status.view(np.int32).any()
        for i in range(cap):
            e, s0, k = int(ent[i]), int(st[i]), int(ln[i])
            assert np.array_equal(out[i, :k], clips[e][s0:s0 + k]) and not out[i, k:].any(), i
        # one global rule, the parent's call: the loudest clip is one event end to end, the quietest has none
        g2 = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 8])
        try:
            assert corpus.events_into(d_lv, n_rows, CH_BIN, x3.EventRule.make(*CH_GLOBAL), g2.ptr[0], g2.ptr[1], g2.ptr[2], None, cap,
                                      g2.ptr[3]) == 0
            rc, gcount = ctx.events_result()
            gent, gst, gln, _ = g2.read()
        finally:
            g2.close()
        glob = [(int(a), int(b), int(c)) for a, b, c in zip(gent.view(np.uint32), gst.view(np.uint64), gln.view(np.uint32))][:gcount]
        assert rc == 0 and glob == E.corpus_events(lv, CH_SIZES, CH_BIN, CH_GLOBAL)[0]
        assert [x for x in glob if x[0] == 3] == [(3, 0, CH_SIZES[3])] and not [x for x in glob if x[0] == 0]
        # the mirror: the same tensors from one call
        t_ent, t_st, t_ln, t_cnt, t_el, t_thr = corpus.adaptive_events(CH_BIN, x3.ThresholdRule.make(mean_sq=CH_TRULE.mean_sq),
                                                                       x3.EventRule.make(*CH_RULE), cap)
        assert int(t_cnt) == count and np.array_equal(t_ent.cpu().numpy().view(np.uint32), went)
        assert np.array_equal(t_st.cpu().numpy().view(np.uint64), wst) and np.array_equal(x3.event_levels_view(t_el), wlv)
        assert [tuple(int(v) for v in t) for t in t_thr.cpu().numpy().reshape(-1).view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == want_thr
        v, k = corpus.level_quantiles(CH_BIN, x3.LEVEL_KEY_MEAN_SQ, [500_000, 1_000_000])
        wv, wk = Q.corpus_quantiles(lv, CH_SIZES, CH_BIN, Q.MEAN_SQ, [500_000, 1_000_000])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv) and np.array_equal(k.cpu().numpy().view(np.uint32), wk)
    finally:
        g.close()
        ctx.free(d_lv)
        corpus.close()


def test_the_stream_mirrors(ctx, x3):
    w = gain_clip(1)
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        n_bins = R.n_bins_for(w.size, CH_BIN)
        lv = R.levels(_frames_of(w, 2000), [0] * ws.n_frames, range(0, w.size, 2000), CH_BIN, n_bins)
        v, k = ws.level_quantiles(CH_BIN, x3.LEVEL_KEY_PEAK, [50_000, 500_000, 950_000])
        wv, wk = Q.stream_quantiles(lv, w.size, CH_BIN, Q.PEAK, [50_000, 500_000, 950_000])
        assert np.array_equal(v.cpu().numpy().view(np.uint32), wv) and np.array_equal(k.cpu().numpy().view(np.uint32), wk)
        st, ln, cnt, el, thr = ws.adaptive_events(CH_BIN, x3.ThresholdRule.make(mean_sq=CH_TRULE.mean_sq), x3.EventRule.make(*CH_RULE), 8)
        want_thr = Q.stream_thresholds(lv, w.size, CH_BIN, CH_TRULE)
        assert [tuple(int(x) for x in t) for t in thr.cpu().numpy().reshape(-1).view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == want_thr
        ev, elv = Q.stream_adaptive_events(lv, w.size, CH_BIN, want_thr[0], CH_RULE)
        _, wst, wln, wlv = E.slots(ev, elv, 8, False)
        assert int(cnt) == len(ev) == 3
        assert np.array_equal(st.cpu().numpy().view(np.uint64), wst) and np.array_equal(ln.cpu().numpy().view(np.uint32), wln)
        assert np.array_equal(x3.event_levels_view(el), wlv)
    finally:
        ws.close()


# ------------------------------------------------------------------------------------------------ refusals and states
def test_refusals_enqueue_nothing_and_leave_the_earlier_results(ctx, x3, T):
    L = x3.lib()
    n, cap, n_q = T + 1, 8, 3
    rng = np.random.default_rng(9)
    lv = records(peak=rng.integers(0, 3000, n), mean_sq=rng.integers(0, 1 << 20, n), rng=rng)
    lv["n"][:] = 0                                                   # the earlier quantiles result: one empty entry
    corpus, ns = layout_corpus(ctx, x3, [T, 1])
    rows = Rows(ctx, lv, BL * n)
    d_lv, d_tot = rows.d_lv, rows.d_tot
    g = Guarded(ctx, [4 * 2 * n_q, 4 * 2, 16 * 2, 4 * cap, 8 * cap, 4 * cap, 32 * cap, 8])
    d_val, d_k, d_thr, d_ent, d_st, d_ln, d_el, d_cnt = g.ptr
    u32p = C.POINTER(C.c_uint32)
    try:
        def quant(c=ctx._h, lv=d_lv, nb=n, bl=BL, tot=d_tot, key=0, q=(1, 500_000, 1_000_000), nq=None, val=d_val, k=d_k,
                  corp="use", corpus_form=False, null_q=False):
            arr = (C.c_uint32 * max(len(q), 1))(*q)
            qp = C.cast(None, u32p) if null_q else arr
            nq = len(q) if nq is None else nq
            if corpus_form:
                return L.x3_corpus_level_quantiles_dev(c, corpus._h if corp == "use" else corp, lv, nb, bl, key, qp, nq, val, k)
            return L.x3_level_quantiles_dev(c, lv, nb, bl, tot, key, qp, nq, val, k)

        def thresh(c=ctx._h, lv=d_lv, nb=n, bl=BL, tot=d_tot, thr=d_thr, corp="use", corpus_form=False, null_rule=False,
                   rule=(0, 0, 0, 0, 500_000, 4, 1, 0)):
            r = x3.ThresholdRule(*rule)
            rp = None if null_rule else C.byref(r)
            if corpus_form:
                return L.x3_corpus_level_thresholds_dev(c, corpus._h if corp == "use" else corp, lv, nb, bl, rp, thr)
            return L.x3_level_thresholds_dev(c, lv, nb, bl, tot, rp, thr)

        good = dict(mean_sq_min=0, peak_min=0, join_bins=2, min_bins=0, pad_bins=1, max_bins=0, reserved=0)

        def adapt(c=ctx._h, lv=d_lv, nb=n, bl=BL, tot=d_tot, thr=d_thr, st=d_st, ln=d_ln, el=d_el, cap=cap, cnt=d_cnt, corp="use",
                  ent=d_ent, corpus_form=False, null_rule=False, **rule):
            r = x3.EventRule(**dict(good, **rule))
            rp = None if null_rule else C.byref(r)
            if corpus_form:
                return L.x3_corpus_events_adaptive_dev(c, corpus._h if corp == "use" else corp, lv, nb, bl, rp, thr, ent, st, ln, el,
                                                       cap, cnt)
            return L.x3_events_adaptive_dev(c, lv, nb, bl, tot, rp, thr, st, ln, el, cap, cnt)

        # earlier calls whose results must survive every refusal: quantiles (an empty entry), adaptive events
        assert quant() == 0
        ctx.upload(d_thr, thr_array(x3, [(0, 1), (0, 1)]))
        ctx.upload(d_lv, records(peak=np.where(np.arange(n) % 4 == 0, 5, 0)))
        assert adapt(cap=3) == 0
        ctx.sync()
        before = [a.copy() for a in g.read()]
        want_events = -(-n // 4)

        shared = [dict(bl=0), dict(bl=1 << 32), dict(nb=0), dict(nb=1 << 31), dict(c=None), dict(lv=None), dict(lv=d_lv + 4),
                  dict(tot=None), dict(tot=d_tot + 4)]
        q_bad = shared + [dict(key=2), dict(key=-1), dict(nq=0), dict(nq=9, q=(0,) * 9), dict(q=(1_000_001,)),
                          dict(q=(0, 5, 1_000_001)), dict(q=(2 ** 32 - 1,)), dict(null_q=True), dict(val=None), dict(k=None),
                          dict(val=d_val + 2), dict(k=d_k + 1)]
        t_bad = shared + [dict(null_rule=True), dict(thr=None), dict(thr=d_thr + 4), dict(rule=(0,) * 8),
                          dict(rule=(5, 1, 0, 0, 5, 1, 0, 0)), dict(rule=(1_000_001, 1, 1, 0, 0, 0, 0, 0)),
                          dict(rule=(0, 1, 1, 0, 1_000_001, 1, 1, 0)), dict(rule=(0, 0, 0, 0, 2 ** 32 - 1, 1, 1, 0))]
        a_bad = shared + [dict(mean_sq_min=1), dict(peak_min=1), dict(mean_sq_min=5, peak_min=5), dict(thr=None), dict(thr=d_thr + 4),
                          dict(pad_bins=2), dict(max_bins=1 << 30, bl=8), dict(reserved=1), dict(cap=0), dict(cap=1 << 31),
                          dict(st=None), dict(ln=None), dict(cnt=None), dict(null_rule=True), dict(st=d_st + 4), dict(ln=d_ln + 2),
                          dict(el=d_el + 4), dict(cnt=d_cnt + 4)]
        for call, bads in ((quant, q_bad), (thresh, t_bad), (adapt, a_bad)):
            for bad in bads:
                assert call(**bad) == BAD, (call.__name__, bad)
                if "tot" not in bad:                                 # (the corpus forms have no d_total)
                    assert call(corpus_form=True, **bad) == BAD, ("corpus", call.__name__, bad)
            for bad in (dict(corp=None), dict(nb=n - 1), dict(nb=n + 1)):
                assert call(corpus_form=True, **bad) == BAD, (call.__name__, bad)
        for bad in (dict(ent=None), dict(ent=d_ent + 2)):
            assert adapt(corpus_form=True, **bad) == BAD, bad
        # (a q_ppm above 1 000 000 of a criterion that is off is not looked at)
        ctx.graph_begin()
        try:
            assert quant() == BAD and thresh() == BAD and adapt() == BAD
            assert quant(corpus_form=True) == BAD and thresh(corpus_form=True) == BAD and adapt(corpus_form=True) == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass
        ctx.sync()
        after = g.read()
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call wrote"
        assert ctx.level_quantiles_result() == (0, 1, 0)            # ... and the results are still the earlier calls'
        assert ctx.events_result() == (0, want_events)
        assert ctx.level_quantiles_result()[0] == BAD and ctx.events_result()[0] == BAD    # read once
        # the limits themselves are fine
        assert quant(q=(0, 1_000_000), key=1) == 0 and ctx.level_quantiles_result() == (0, 0, 1)
    finally:
        g.close()
        rows.close()


def test_a_quantiles_call_leaves_the_other_pending_results_alone(ctx, x3):
    w = gain_clip(0)
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    n_bins, cap = R.n_bins_for(w.size, CH_BIN), 4
    d_lv = ctx.alloc(32 * n_bins)
    g = Guarded(ctx, [4 * 2, 4, 16, 8 * cap, 4 * cap, 8, 2 * cap * 500, 4 * cap])
    d_val, d_k, d_thr, d_st, d_ln, d_cnt, d_out, d_status = g.ptr
    try:
        assert ctx.levels_dev(ws.d_x3, ws.x3_len, ws.d_frame_offsets, ws.d_sample_offsets, ws.n_frames, p, CH_BIN, d_lv, n_bins,
                              None, ws.d_seg_index, ws.seg_blocks) == 0
        ctx.upload(d_st, np.array([0, 100, 5_000, 0], dtype=np.uint64))
        ctx.upload(d_ln, np.array([10, 500, 7, 0], dtype=np.uint32))
        assert ws.ranges_into(d_st, d_ln, cap, 500, d_out, cap * 500, 0, None, d_status) == 0
        assert ws.level_quantiles_into(d_lv, n_bins, CH_BIN, x3.LEVEL_KEY_PEAK, [0, 1_000_000], d_val, d_k) == 0
        assert ws.level_thresholds_into(d_lv, n_bins, CH_BIN, x3.ThresholdRule.make(peak=(500_000, 2, 1, 0)), d_thr) == 0
        assert ctx.level_quantiles_result() == (0, 0, 1)
        assert ctx.decode_ranges_result()[:4] == (0, 0, cap, 0)
        assert ctx.levels_result() == (0, 0, ws.n_frames, 0)
        lv = R.levels(_frames_of(w, 2000), [0] * ws.n_frames, range(0, w.size, 2000), CH_BIN, n_bins)
        val, k, thr = g.read()[:3]
        wv, wk = Q.stream_quantiles(lv, w.size, CH_BIN, Q.PEAK, [0, 1_000_000])
        assert np.array_equal(val.view(np.uint32), wv[0]) and int(k.view(np.uint32)[0]) == int(wk[0]) == n_bins
        assert [tuple(int(x) for x in t) for t in thr.view(x3.EVENT_THRESHOLD_DTYPE).tolist()] == \
            Q.stream_thresholds(lv, w.size, CH_BIN, Q.TRule(peak=(500_000, 2, 1, 0)))
    finally:
        g.close()
        ctx.free(d_lv)
        ws.close()
