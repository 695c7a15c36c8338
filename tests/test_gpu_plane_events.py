"""Plane events (include/x3hip.h, "PLANE EVENTS"): x3_plane_events_dev, x3_corpus_plane_events_dev and their Python mirrors.
Every field of every slot -- entry, start, len, mask, the merged record of every plane, the fillers, the count -- is held with
== against plane_events_ref.py.  Cases upload synthetic level records straight into d_levels (no decode), laid round the
kernels' tile (option "events_tile_rows"); the rows between n_rows and plane_stride are loud and must change nothing; the
end-to-end cases run bank levels, plane events and bank range levels back to back on the device."""
import ctypes as C

import numpy as np
import pytest

import async_cases as AC
import events_ref as E
import levels_ref as R
import oracle_lib as O
import plane_events_ref as P
import quantiles_ref as Q
import tone_bank_levels_ref as B
import tone_levels_ref as TR

pytestmark = pytest.mark.gpu

BAD = 24
GUARD = 64
CANARY = 0x5A
BL = 4


@pytest.fixture(scope="module")
def x3():
    import torch  # noqa: F401  (torch first: its HIP runtime serves the library too)
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


def records(hot, rng=None, empty_at=()):
    """level records: loud where `hot` is set (peak 1500, mean square 750 000), quiet elsewhere, nothing counted at
    `empty_at` (whose other fields stay as they are: n == 0 alone must keep them from counting)"""
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


def planes_of(hots, rng=None, empty_at=()):
    return np.stack([records(h, rng, empty_at if t == 0 else ()) for t, h in enumerate(hots)])


def peak_rule(k, min_planes=1, **kw):
    return P.PlaneRule([0] * k, [1000] * k, min_planes, **kw)


def c_rule(x3, rule, k, thr=False):
    z = [0] * k
    return x3.PlaneEventRule.make(z if thr else list(rule.mean_sq_min), z if thr else list(rule.peak_min), rule.min_planes,
                                  rule.join_bins, rule.min_bins, rule.pad_bins, rule.max_bins)


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


def thr_array(x3, thr):
    """thr[t][e] = (mean_sq_min, peak_min, counted) -> records laid plane-major"""
    a = np.zeros(sum(len(t) for t in thr), dtype=x3.EVENT_THRESHOLD_DTYPE)
    a[:] = [v for t in thr for v in t]
    return a


def run(ctx, x3, lv, rule, cap, total=None, corpus=None, pad=0, thr=None, masks=True, levels=True, after_call=None):
    """one call on uploaded planes lv [K, n_rows] -> (entries or None, starts, lens, masks or None, event levels [K, cap] or
    None, count).  The planes lie plane_stride = n_rows + pad apart, the rows in between are loud; the result call, the
    canaries round every output and "every slot is written" are checked"""
    k, n_rows = lv.shape
    stride = n_rows + pad
    up = np.stack([records(np.ones(stride, bool)) for _ in range(k)])
    up[:, :n_rows] = lv
    d_lv, d_tot = ctx.alloc(32 * k * stride), ctx.alloc(8)
    d_thr = ctx.alloc(16 * sum(len(t) for t in thr)) if thr is not None else None
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 4 * cap, 32 * k * cap, 8])
    try:
        ctx.upload(d_lv, up)
        ctx.upload(d_tot, np.array([0 if total is None else total], dtype=np.uint64))
        if thr is not None:
            ctx.upload(d_thr, thr_array(x3, thr))
        d_ent, d_st, d_ln, d_mk, d_el, d_cnt = g.ptr
        r = c_rule(x3, rule, k, thr is not None)
        for t in range(k, 8):                       # values behind n_planes are never read
            r.mean_sq_min[t], r.peak_min[t] = (1 << 40) + t, 99_999
        args = (r, d_thr, d_st, d_ln, d_mk if masks else None, d_el if levels else None, cap, d_cnt)
        if corpus is None:
            rc = ctx.plane_events_dev(d_lv, stride, n_rows, BL, d_tot, *args)
        else:
            rc = corpus.plane_events_into(d_lv, stride, n_rows, BL, args[0], args[1], d_ent, *args[2:])
        assert rc == 0, (rc, ctx.last_error())
        if after_call:
            after_call(r, d_thr)
        res = ctx.events_result()
        ent, st, ln, mk, el, cnt = g.read()
    finally:
        g.close()
        for q in (d_lv, d_tot, d_thr):
            if q:
                ctx.free(q)
    cnt = int(cnt.view(np.uint64)[0])
    assert res == (0, cnt), (res, cnt)
    if corpus is None:
        assert (ent == CANARY).all(), "a stream call has no entries to write"
    if not masks:
        assert (mk == CANARY).all()
    if not levels:
        assert (el == CANARY).all()
    return (ent.view(np.uint32) if corpus is not None else None, st.view(np.uint64), ln.view(np.uint32),
            mk.view(np.uint32) if masks else None, el.view(R.LEVEL_DTYPE).reshape(k, cap) if levels else None, cnt)


def check(ctx, x3, lv, rule, cap, total=None, corpus=None, n_samples=None, what=None, **kw):
    got = run(ctx, x3, lv, rule, cap, total=total, corpus=corpus, **kw)
    thr = kw.get("thr")
    if corpus is None:
        ev, elv = P.stream_plane_events(lv, total, BL, rule, None if thr is None else [t[0] for t in thr])
    else:
        ev, elv = P.corpus_plane_events(lv, n_samples, BL, rule, thr)
    ent, st, ln, mk, sl = P.slots(ev, elv, cap, corpus is not None)
    assert got[5] == len(ev), (what, got[5], len(ev))
    if corpus is not None:
        assert np.array_equal(got[0], ent), (what, got[0][:8], ent[:8])
    assert np.array_equal(got[1], st), (what, got[1][:8], st[:8])
    assert np.array_equal(got[2], ln), (what, got[2][:8], ln[:8])
    if got[3] is not None:
        assert np.array_equal(got[3], mk), (what, got[3][:8], mk[:8])
    if got[4] is not None:
        for f in R.LEVEL_DTYPE.names:
            assert np.array_equal(got[4][f], sl[f]), (what, f, np.argwhere(got[4][f] != sl[f])[:5])
    return ev


# ------------------------------------------------------------------------------------------------ stream form
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_random_planes_round_the_tile(ctx, x3, T, k):
    rng = np.random.default_rng(100 + k)
    for n in (T - 1, T, T + 1, 2 * T + 1):
        for mp in sorted({1, min(2, k), k}):
            for pad in (0, 5):
                hots = [rng.random(n) < (0.5 if mp > 1 else 0.1) for _ in range(k)]
                lv = planes_of(hots, rng, empty_at=np.flatnonzero(rng.random(n) < 0.05))
                join = int(rng.choice([0, 1, 2, 5]))
                crit = rng.integers(0, 3, k)
                rule = P.PlaneRule([0 if c == 0 else 500_000 for c in crit], [0 if c == 1 else 1000 for c in crit], mp, join,
                                   int(rng.choice([0, 1, 2])), int(rng.integers(0, join // 2 + 1)), int(rng.choice([0, 0, 1, 3])))
                tot = int(rng.choice([BL * n, BL * n - 3, 10 ** 12]))
                cap = int(rng.choice([1, 7, n + 3]))
                check(ctx, x3, lv, rule, cap, total=tot, pad=pad, what=(k, n, mp, pad, rule))


def test_the_tile_edge_a_step_from_plane_to_plane(ctx, x3, T):
    n = 2 * T + 1
    h0, h1 = np.zeros(n, bool), np.zeros(n, bool)
    h0[T - 1], h1[T] = True, True
    lv = planes_of([h0, h1])
    assert check(ctx, x3, lv, peak_rule(2, 1), 4, total=BL * n, pad=5) == [(BL * (T - 1), 2 * BL, 3)]
    assert check(ctx, x3, lv, peak_rule(2, 2), 4, total=BL * n, pad=5) == []
    # the two single-plane events calls on the same records: two one-row events in two lists
    for t, row in ((0, T - 1), (1, T)):
        d_lv, d_tot = ctx.alloc(32 * n), ctx.alloc(8)
        g = Guarded(ctx, [8 * 4, 4 * 4, 8])
        try:
            ctx.upload(d_lv, lv[t])
            ctx.upload(d_tot, np.array([BL * n], dtype=np.uint64))
            assert ctx.events_dev(d_lv, n, BL, d_tot, x3.EventRule.make(peak_min=1000), g.ptr[0], g.ptr[1], None, 4, g.ptr[2]) == 0
            assert ctx.events_result() == (0, 1)
            st, ln, _ = g.read()
            assert (int(st.view(np.uint64)[0]), int(ln.view(np.uint32)[0])) == (BL * row, BL)
        finally:
            g.close()
            ctx.free(d_lv)
            ctx.free(d_tot)


def test_empty_records_and_off_planes(ctx, x3, T):
    n = T + 1
    h = np.zeros(n, bool)
    h[[3, T]] = True
    lv = planes_of([h, h, h], empty_at=[3])                       # plane 0 counts nothing at row 3, loud as its fields are
    ev = check(ctx, x3, lv, peak_rule(3, 3), 4, total=BL * n)
    assert ev == [(BL * T, BL, 7)]
    assert check(ctx, x3, lv, peak_rule(3, 2), 4, total=BL * n) == [(BL * 3, BL, 6), (BL * T, BL, 7)]
    off = P.PlaneRule([0, 0, 0], [1000, 0, 1000], 2)              # plane 1 is off: never loud, never in a mask
    assert check(ctx, x3, lv, off, 4, total=BL * n) == [(BL * T, BL, 5)]
    assert check(ctx, x3, lv, off._replace(min_planes=1), 4, total=BL * n) == [(BL * 3, BL, 4), (BL * T, BL, 5)]


def single_events(ctx, x3, lv, rule, cap, total=None, corpus=None, thr=None, levels=True):
    """x3_events_dev / x3_corpus_events_dev / the adaptive calls on one plane -> the raw bytes of (entries, starts, lens,
    event levels, count); levels=False: d_event_levels is NULL and its array must stay as it was"""
    n = lv.size
    d_lv, d_tot, d_thr = ctx.alloc(32 * n), ctx.alloc(8), ctx.alloc(16 * (len(thr) if thr else 1))
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 32 * cap, 8])
    try:
        ctx.upload(d_lv, lv)
        ctx.upload(d_tot, np.array([total or 0], dtype=np.uint64))
        if thr:
            ctx.upload(d_thr, thr_array(x3, [thr]))
        d_ent, d_st, d_ln, d_el, d_cnt = g.ptr
        if not levels:
            d_el = None
        r = x3.EventRule.make(0 if thr else rule.mean_sq_min[0], 0 if thr else rule.peak_min[0], rule.join_bins, rule.min_bins,
                              rule.pad_bins, rule.max_bins)
        if corpus is None and not thr:
            rc = ctx.events_dev(d_lv, n, BL, d_tot, r, d_st, d_ln, d_el, cap, d_cnt)
        elif corpus is None:
            rc = ctx.events_adaptive_dev(d_lv, n, BL, d_tot, r, d_thr, d_st, d_ln, d_el, cap, d_cnt)
        elif not thr:
            rc = corpus.events_into(d_lv, n, BL, r, d_ent, d_st, d_ln, d_el, cap, d_cnt)
        else:
            rc = corpus.adaptive_events_into(d_lv, n, BL, r, d_thr, d_ent, d_st, d_ln, d_el, cap, d_cnt)
        assert rc == 0 and ctx.events_result()[0] == 0
        out = g.read()
        assert levels or (out[3] == CANARY).all()
        return out
    finally:
        g.close()
        for q in (d_lv, d_tot, d_thr):
            ctx.free(q)


_CORPORA = {}


def layout_corpus(ctx, x3, rows):
    """a corpus whose entry e has rows[e] rows at bin length BL: clips of silence of 4 r - (e % 4) samples"""
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
        _CORPORA[key] = (corpus, ns)
    return _CORPORA[key]


@pytest.fixture(scope="module", autouse=True)
def _close_corpora():
    yield
    for corpus, _ in _CORPORA.values():
        corpus.close()
    _CORPORA.clear()


def test_one_plane_is_the_events_call_byte_for_byte(ctx, x3, T):
    # An events call IS a plane events call of one plane in the library (one descriptor, one launch set): both sides of this
    # comparison run the same flag instance, and differ only in the emit kernel the mask asks for.  What it still pins is the
    # host-side mapping of the two rule structs onto that descriptor.  The independent check of the kernels is
    # events_ref.py / plane_events_ref.py, which every check() here uses.
    rng = np.random.default_rng(5)
    n, cap = 2 * T + 1, 9
    lv = planes_of([rng.random(n) < 0.2], rng, empty_at=[7, T])
    rule = P.PlaneRule([500_000], [1000], 1, 2, 2, 1, 3)
    corpus, ns = layout_corpus(ctx, x3, [T - 1, 2, T])
    thr = [(500_000, 0, 5), (0, 1000, 6), (1 << 31, 1200, 7)]
    for form in ("stream", "corpus", "stream thr", "corpus thr"):
        c = corpus if "corpus" in form else None
        th = None if "thr" not in form else (thr if c else thr[:1])
        got = run(ctx, x3, lv, rule, cap, total=BL * n - 1, corpus=c, thr=None if th is None else [th])
        ent, st, ln, el, cnt = single_events(ctx, x3, lv[0], rule, cap, total=BL * n - 1, corpus=c, thr=th)
        assert got[5] == int(cnt.view(np.uint64)[0]) > 3, form
        assert got[1].tobytes() == st.tobytes() and got[2].tobytes() == ln.tobytes() and got[4].tobytes() == el.tobytes(), form
        assert c is None or got[0].tobytes() == ent.tobytes(), form
        assert set(got[3][:min(got[5], cap)].tolist()) <= {0, 1} and not got[3][min(got[5], cap):].any()
    # no run cut: every event holds a hot row, the mask is 1 in every event
    got = run(ctx, x3, lv, rule._replace(max_bins=0), cap, total=BL * n)
    assert got[5] > 3 and (got[3][:min(got[5], cap)] == 1).all()


def test_equal_planes_and_permuted_planes(ctx, x3, T):
    rng = np.random.default_rng(6)
    n, cap = T + 1, T + 4
    one = planes_of([rng.random(n) < 0.3], rng)
    r1 = P.PlaneRule([0], [1000], 1, 2, 0, 1, 0)
    base = run(ctx, x3, one, r1, cap, total=BL * n)
    for k in (2, 8):
        for mp in (1, 2, k):
            got = run(ctx, x3, np.concatenate([one] * k), peak_rule(k, mp, join_bins=2, pad_bins=1), cap, total=BL * n, pad=5)
            assert got[5] == base[5] and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
            assert (got[3][:got[5]] == (1 << k) - 1).all() and all(got[4][t].tobytes() == base[4][0].tobytes() for t in range(k))
    k = 3
    lv = planes_of([rng.random(n) < 0.3 for _ in range(k)], rng)
    rule = P.PlaneRule([0, 500_000, 0], [1000, 0, 1200], 2, 2, 0, 1, 0)
    a = run(ctx, x3, lv, rule, cap, total=BL * n)
    perm = [2, 0, 1]
    prule = rule._replace(mean_sq_min=[rule.mean_sq_min[j] for j in perm], peak_min=[rule.peak_min[j] for j in perm])
    b = run(ctx, x3, lv[perm], prule, cap, total=BL * n)
    assert a[5] == b[5] > 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    want = sum(((a[3] >> perm[i]) & 1) << i for i in range(k))
    assert np.array_equal(b[3], want) and b[4].tobytes() == a[4][perm].tobytes()


def test_a_padding_row_sets_its_bit(ctx, x3, T):
    n = T + 3
    h0, h1 = np.zeros(n, bool), np.zeros(n, bool)
    h0[[T - 1, T]] = True
    h1[[T - 2, T]] = True                                        # row T - 2: loud in plane 1 alone; row T: hot
    lv = planes_of([h0, h1])
    ev = check(ctx, x3, lv, peak_rule(2, 2, join_bins=2, pad_bins=1), 3, total=BL * n)
    assert ev == [(BL * (T - 1), 3 * BL, 3)]
    h1[T] = False
    h1[T + 1] = True                                             # plane 1 loud in padding rows alone: no hot row at all
    assert check(ctx, x3, planes_of([h0, h1]), peak_rule(2, 2, join_bins=2, pad_bins=1), 3, total=BL * n) == []
    h0[T + 1] = True                                             # hot at T + 1 only; row T is padding, loud in plane 0 alone
    h0[T - 1] = False
    h1[T - 2] = False
    ev = check(ctx, x3, planes_of([h0, h1]), peak_rule(2, 2, join_bins=2, pad_bins=1), 3, total=BL * n)
    assert ev == [(BL * T, 3 * BL, 3)]
    h0[T + 1], h0[T + 2] = False, True                           # now nothing is hot, though both planes are loud nearby
    assert check(ctx, x3, planes_of([h0, h1]), peak_rule(2, 2, join_bins=2, pad_bins=1), 3, total=BL * n) == []


def test_long_pieces_have_masks_and_levels_of_their_own(ctx, x3, T):
    n = T + 10
    h0, h1 = np.zeros(n, bool), np.zeros(n, bool)
    h0[20:220] = True
    h1[100:103] = True
    lv = planes_of([h0, h1], np.random.default_rng(8))
    ev = check(ctx, x3, lv, peak_rule(2, 1, max_bins=3), 80, total=BL * n, pad=5)
    assert len(ev) == 67 and [e[2] for e in ev].count(3) == 2 and ev[-1][1] == 2 * BL
    ev = check(ctx, x3, lv, peak_rule(2, 1, max_bins=150), 5, total=BL * n)       # pieces longer than a wave
    assert [(e[1], e[2]) for e in ev] == [(150 * BL, 3), (50 * BL, 1)]
    ev = check(ctx, x3, lv, peak_rule(2, 1), 5, total=BL * n)
    assert ev == [(20 * BL, 200 * BL, 3)]


def test_count_above_cap_and_null_outputs(ctx, x3, T):
    n = T + 1
    rng = np.random.default_rng(9)
    lv = planes_of([np.arange(n) % 3 == 0, rng.random(n) < 0.5, np.arange(n) % 4 == 0], rng)
    rule = peak_rule(3, 1)
    full = len(P.stream_plane_events(lv, BL * n, BL, rule)[0])
    for cap in (1, full - 1, full, full + 5):
        assert len(check(ctx, x3, lv, rule, cap, total=BL * n, what=cap)) == full
    for masks, levels in ((False, True), (True, False), (False, False)):
        check(ctx, x3, lv, rule, full + 2, total=BL * n, masks=masks, levels=levels)
        check(ctx, x3, lv, rule, 2, total=BL * n, masks=masks, levels=levels)


# ------------------------------------------------------------------------------------------------ the shared flag and emit steps
def check_single(ctx, x3, lv, rule, cap, total=None, corpus=None, n_samples=None, thr=None, levels=True, what=None):
    """the four events entry points on one plane against plane_events_ref with K = 1; thr: None or a record per entry"""
    ent, st, ln, el, cnt = single_events(ctx, x3, lv, rule, cap, total=total, corpus=corpus, thr=thr, levels=levels)
    if corpus is None:
        ev, elv = P.stream_plane_events(lv[None], total, BL, rule, None if thr is None else [thr[0]])
    else:
        ev, elv = P.corpus_plane_events(lv[None], n_samples, BL, rule, None if thr is None else [thr])
    w_ent, w_st, w_ln, _, w_el = P.slots(ev, elv, cap, corpus is not None)
    assert int(cnt.view(np.uint64)[0]) == len(ev), (what, len(ev))
    if corpus is None:
        assert (ent == CANARY).all(), what
    else:
        assert ent.tobytes() == w_ent.tobytes(), what
    assert st.tobytes() == w_st.tobytes() and ln.tobytes() == w_ln.tobytes(), what
    assert not levels or el.tobytes() == w_el[0].tobytes(), what
    return ev


@pytest.mark.parametrize("max_bins", [65, 130])
def test_one_plane_through_all_six_entry_points(ctx, x3, T, max_bins):
    """K = 1 where the piece walk, the wave join and the fillers are shared: pieces longer than one wave turn, every
    combination of NULL optional outputs, stream and corpus, the rule's values and d_thr's"""
    rows = [230, 2, 25]
    corpus, ns = layout_corpus(ctx, x3, rows)
    n = sum(rows)
    hot = np.zeros(n, bool)
    hot[10:215] = True                                               # 205 hot rows: pieces of 65 or 130 rows and a rest
    hot[[231, 240, 241, 256]] = True
    lv = planes_of([hot], np.random.default_rng(max_bins))
    rule = P.PlaneRule([0], [1000], 1, 1, 0, 0, max_bins)
    thr = [(0, 1000, 1), (2_000_000, 0, 2), (0, 1200, 3)]
    cap = 12
    for form in ("stream", "corpus", "stream thr", "corpus thr"):
        c = corpus if "corpus" in form else None
        th = None if "thr" not in form else (thr if c else thr[:1])
        kw = dict(total=None if c else BL * n - 1, corpus=c, n_samples=ns if c else None)
        for levels in (True, False):
            ev = check_single(ctx, x3, lv[0], rule, cap, thr=th, levels=levels, what=(form, levels), **kw)
            assert len(ev) >= 4 and max(e[-2] for e in ev) == max_bins * BL
            for masks in (True, False):
                check(ctx, x3, lv, rule, cap, thr=None if th is None else [th], masks=masks, levels=levels,
                      what=(form, masks, levels), **kw)
        check(ctx, x3, lv, rule, 2, thr=None if th is None else [th], what=(form, "cap 2"), **kw)   # the fillers' own start
        check_single(ctx, x3, lv[0], rule, 2, thr=th, what=(form, "cap 2"), **kw)


LIMIT_MS, LIMIT_PK = 1 << 30, 32768
# (mean_sq_min, peak_min) of a plane and the records that stand at its edge: hot rows meet the value exactly, the others
# miss it by one -- or would meet the criterion above its limit, had nobody tested the limit
EDGE_KINDS = {
    "ms at its limit": (LIMIT_MS, 0),
    "pk at its limit": (0, LIMIT_PK),
    "ms above its limit": (LIMIT_MS + 1, 1000),
    "pk above its limit": (500_000, LIMIT_PK + 1),
    "plain": (0, 1000),
}


def edge_records(hot, kind):
    lv = records(hot)
    if kind == "ms at its limit":
        lv["max"], lv["min"] = 10, -3
        lv["sum_sq"] = np.where(hot, LIMIT_MS * BL, LIMIT_MS * BL - 1).astype(np.uint64)
    elif kind == "pk at its limit":
        lv["max"] = 32767
        lv["min"] = np.where(hot, -32768, -32767)
    elif kind == "ms above its limit":                               # a cold row's sum_sq would pass (2^30 + 1) * n
        lv["sum_sq"] = np.where(hot, 200, (1 << 33) + np.arange(hot.size)).astype(np.uint64)
    elif kind == "pk above its limit":                               # a cold row's peak is the largest there is
        lv["max"] = 10
        lv["min"] = np.where(hot, -3, -32768)
        lv["sum_sq"] = np.where(hot, 500_000 * BL, 500_000 * BL - 1).astype(np.uint64)
    return lv


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("thr", [False, True], ids=["rule", "thr"])
def test_each_flag_instance_at_its_edges(ctx, x3, T, thr, k):
    """rule / d_thr x K in {1, 8} with min_planes = K, so that every plane's load and test decides the verdict: n_rows round
    the tile, a corpus whose entry edges fall inside a wave, values at their limits and (d_thr only: the host refuses them
    in a rule) above them"""
    kinds = list(EDGE_KINDS) if thr else ["ms at its limit", "pk at its limit", "plain"]
    corpus, ns = layout_corpus(ctx, x3, [1, T - 1, 2])
    for n, c in ((T - 1, None), (T, None), (T + 1, None), (T + 2, corpus)):
        for first in range(len(kinds) if k == 1 else 1):             # K = 1: every kind in its own call
            of = [kinds[(first + t) % len(kinds)] for t in range(k)]
            rng = np.random.default_rng(1000 * n + 10 * k + first)
            hots = [rng.random(n) < 0.85 for _ in range(k)]
            for t in range(k):                                       # plane t alone keeps row t + 2 cold; the edges are hot
                for u in range(k):
                    hots[u][t + 2] = u != t
                hots[t][[0, 1, n - 2, n - 1]] = True
            lv = np.stack([edge_records(hots[t], of[t]) for t in range(k)])
            vals = [EDGE_KINDS[kd] for kd in of]
            rule = P.PlaneRule([0] * k if thr else [v[0] for v in vals], [0] * k if thr else [v[1] for v in vals], k, 0, 0, 0, 0)
            th = None
            if thr:                                                  # the same values in every entry, counted garbage
                th = [[(v[0], v[1], 7 + e) for e in range(3 if c else 1)] for v in vals]
            ev = check(ctx, x3, lv, rule, n, total=None if c else BL * n, corpus=c, n_samples=ns if c else None, thr=th,
                       pad=3, what=(n, of))
            all_hot = np.logical_and.reduce(hots)
            assert len(ev) >= 2 and not all_hot[2:2 + k].any() and all_hot[[0, 1, n - 2, n - 1]].all()
            if k == 1 and c is None:
                check_single(ctx, x3, lv[0], rule, n, total=BL * n, thr=None if th is None else th[0], what=(n, of))


# ------------------------------------------------------------------------------------------------ corpus form
def test_corpus_entries_of_one_row_and_runs_that_stop_at_entries(ctx, x3, T):
    rows = [1] * (T + 2)
    corpus, ns = layout_corpus(ctx, x3, rows)
    n = T + 2
    lv = planes_of([np.ones(n, bool), np.arange(n) % 2 == 0])
    ev = check(ctx, x3, lv, peak_rule(2, 1, join_bins=5, pad_bins=2), n + 3, corpus=corpus, n_samples=ns, pad=5)
    assert [e[0] for e in ev] == list(range(n)) and [e[3] for e in ev] == [3, 1] * (n // 2)
    # runs never cross an entry, even when the neighbour's first row is loud in other planes
    for cut in (T - 1, T, T + 1):
        rows = [cut, 2 * T + 1 - cut, 1, 0, 3]
        corpus, ns = layout_corpus(ctx, x3, rows)
        n = sum(max(r, 1) for r in rows)
        h0, h1 = np.zeros(n, bool), np.zeros(n, bool)
        h0[[cut - 2, cut - 1]] = True
        h1[[cut, cut + 1, 2 * T + 1, 2 * T + 2]] = True          # (2 T + 2: the entry of no samples, whose row counts nothing)
        lv = planes_of([h0, h1])
        lv[1]["n"][2 * T + 2] = 0
        ev = check(ctx, x3, lv, peak_rule(2, 1, join_bins=4, pad_bins=2), 8, corpus=corpus, n_samples=ns, what=cut)
        assert [(e[0], e[3]) for e in ev] == [(0, 1), (1, 2), (2, 2)]
        rng = np.random.default_rng(cut)
        lv = planes_of([rng.random(n) < 0.4 for _ in range(3)], rng)
        for mp in (1, 2, 3):
            check(ctx, x3, lv, peak_rule(3, mp, join_bins=3, pad_bins=1, max_bins=5), n, corpus=corpus, n_samples=ns, pad=5)
    other = None
    import torch
    if torch.cuda.device_count() > 1:
        other = x3.Context(1)
        try:
            g = Guarded(ctx, [64] * 4)
            r = c_rule(x3, peak_rule(2, 1), 2)
            assert x3.lib().x3_corpus_plane_events_dev(other._h, corpus._h, g.ptr[0], n, n, BL, C.byref(r), None, g.ptr[0], g.ptr[1],
                                                       g.ptr[2], None, None, 2, g.ptr[3]) == BAD
            g.read()
            g.close()
        finally:
            other.close()


def test_thresholds_per_plane_and_entry(ctx, x3, T):
    rows = [T - 1, 2, T]
    corpus, ns = layout_corpus(ctx, x3, rows)
    n = sum(rows)
    rng = np.random.default_rng(11)
    lv = planes_of([rng.random(n) < 0.4 for _ in range(3)], rng)
    # distinct values per (plane, entry); one above its limit; both 0 for plane 1 of entry 2; counted garbage
    thr = [[(500_000, 0, 1), (0, 1000, 2), (3_000_001, 1501, 3)],
           [(0, 1503, 0xFFFFFFFF), ((1 << 30) + 1, 1000, 5), (0, 0, 6)],
           [(750_000, 32769, 7), (1, 0, 8), (0, 1500, 9)]]
    rule = P.PlaneRule([0] * 3, [0] * 3, 1, 2, 0, 1, 4)
    for mp in (1, 2, 3):
        check(ctx, x3, lv, rule._replace(min_planes=mp), n, corpus=corpus, n_samples=ns, thr=thr, pad=5, what=mp)
    check(ctx, x3, lv, rule, n, total=BL * n, thr=[t[:1] for t in thr])
    # the rule struct is copied at the call: overwritten behind it, nothing changes.  (That d_thr is read when the kernels
    # run, not at the call, is what test_behind_a_stalled_stream shows: its thresholds arrive behind the stall.)
    def scribble(r, d_thr):
        C.memset(C.byref(r), 0xFF, C.sizeof(r))
    check(ctx, x3, lv, rule._replace(min_planes=2), n, corpus=corpus, n_samples=ns, thr=thr, after_call=scribble)


# ------------------------------------------------------------------------------------------------ refusals and states
def test_refusals_enqueue_nothing_and_leave_the_earlier_result(ctx, x3, T):
    L = x3.lib()
    n, cap, k = T + 1, 8, 2
    lv = planes_of([np.arange(n) % 4 == 0, np.arange(n) % 6 == 0])
    corpus, ns = layout_corpus(ctx, x3, [T, 1])
    d_lv, d_tot, d_thr = ctx.alloc(32 * k * (n + 5)), ctx.alloc(8), ctx.alloc(16 * 2 * k + 8)
    g = Guarded(ctx, [4 * cap, 8 * cap, 4 * cap, 4 * cap, 32 * k * cap, 8])
    d_ent, d_st, d_ln, d_mk, d_el, d_cnt = g.ptr
    try:
        ctx.upload(d_lv, np.concatenate([lv[0], lv[1]]))
        ctx.upload(d_tot, np.array([BL * n], dtype=np.uint64))
        ctx.upload(d_thr, np.zeros(16 * 2 * k + 8, dtype=np.uint8))
        good = dict(n_planes=2, min_planes=1, join_bins=2, min_bins=0, pad_bins=1, max_bins=0)

        def call(c=ctx._h, lv=d_lv, ps=n, nb=n, bl=BL, tot=d_tot, thr=None, st=d_st, ln=d_ln, mk=d_mk, el=d_el, cap=cap, cnt=d_cnt,
                 kc="use", ent=d_ent, corpus_form=False, null_rule=False, ms=(0, 0), pk=(1000, 1000), reserved=(0, 0), **rule):
            r = x3.PlaneEventRule(**dict(good, **rule))
            r.reserved[0], r.reserved[1] = reserved
            for t in range(8):
                r.mean_sq_min[t], r.peak_min[t] = (ms[t], pk[t]) if t < len(ms) else ((1 << 40), 99_999)
            rp = None if null_rule else C.byref(r)
            if corpus_form:
                return L.x3_corpus_plane_events_dev(c, corpus._h if kc == "use" else kc, lv, ps, nb, bl, rp, thr, ent, st, ln, mk,
                                                    el, cap, cnt)
            return L.x3_plane_events_dev(c, lv, ps, nb, bl, tot, rp, thr, st, ln, mk, el, cap, cnt)

        assert call(cap=3) == 0                                       # an earlier call whose result must survive
        before = [a.copy() for a in g.read()]
        want = len(P.stream_plane_events(lv, BL * n, BL, peak_rule(2, 1, join_bins=2, pad_bins=1))[0])
        refusals = [dict(bl=0), dict(bl=1 << 32), dict(pk=(0, 0)), dict(pk=(32769, 1000)), dict(ms=((1 << 30) + 1, 0)),
                    dict(pad_bins=2), dict(join_bins=0), dict(max_bins=1 << 30, bl=8), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
                    dict(cap=0), dict(cap=1 << 31), dict(nb=0), dict(nb=1 << 31, ps=1 << 31), dict(c=None), dict(lv=None),
                    dict(tot=None), dict(st=None), dict(ln=None), dict(cnt=None), dict(null_rule=True), dict(lv=d_lv + 4),
                    dict(tot=d_tot + 4), dict(st=d_st + 4), dict(ln=d_ln + 2), dict(el=d_el + 4), dict(cnt=d_cnt + 4),
                    dict(mk=d_mk + 2), dict(n_planes=0), dict(n_planes=9), dict(min_planes=0), dict(min_planes=3), dict(ps=n - 1), dict(ps=1 << 31), dict(ps=1 << 59),
                    dict(pk=(1000, 0), min_planes=2),                  # an off plane leaves fewer than min_planes on
                    dict(thr=d_thr), dict(thr=d_thr, pk=(0, 0), ms=(0, 5)), dict(thr=d_thr + 4, pk=(0, 0))]
        for bad in refusals:
            assert call(**bad) == BAD, bad
            if "tot" not in bad:
                assert call(corpus_form=True, **bad) == BAD, ("corpus", bad)
        for bad in (dict(kc=None), dict(ent=None), dict(ent=d_ent + 2), dict(nb=n - 1), dict(nb=n + 1, ps=n + 1)):
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
        assert ctx.events_result() == (0, want)                      # ... and the result is still the earlier call's
        assert ctx.events_result()[0] == BAD                         # read once
        # the limits themselves are fine; the optional outputs may be NULL; thresholds with a rule of zeros
        assert call(ms=(1 << 30, 0), pk=(32768, 32768), el=None, mk=None) == 0 and ctx.events_result() == (0, 0)
        assert call(thr=d_thr, pk=(0, 0)) == 0 and ctx.events_result() == (0, 0)
        assert call(ps=n + 5) == 0 and ctx.events_result()[0] == 0
        assert call(corpus_form=True) == 0 and ctx.events_result()[0] == 0
    finally:
        g.close()
        for q in (d_lv, d_tot, d_thr):
            ctx.free(q)


# ------------------------------------------------------------------------------------------------ behind a stalled stream
class StalledPlaneEvents(AC.Case):
    """levels planes, the sample count and the thresholds arrive on the stream behind a stall; a decoy lies there when the
    host enqueues the call"""
    name = "plane_events"
    K, CAP = 3, 16

    def __init__(self, T):
        self.n = T + 7
        self.rule = P.PlaneRule([0] * 3, [0] * 3, 2, 2, 0, 1, 5)

    def content(self, which):
        rng = np.random.default_rng({"A": 1, "B": 2}[which])
        lv = planes_of([rng.random(self.n) < 0.6 for _ in range(self.K)], rng)
        thr = [[(0, 1000 + t, 3)] for t in range(self.K)] if which == "B" else [[(3_000_050, 0, 1)]] * self.K
        return lv, BL * self.n - (1 if which == "B" else 9), thr

    def inputs(self, which):
        import x3hip
        lv, tot, thr = self.content(which)
        return {"lv": lv, "tot": np.array([tot], dtype=np.uint64), "thr": thr_array(x3hip, thr)}

    def outputs(self):
        return {"st": 8 * self.CAP, "ln": 4 * self.CAP, "mk": 4 * self.CAP, "el": 32 * self.K * self.CAP, "cnt": 8}

    def enqueue(self, x3, ctx, d, which, probe):
        r = c_rule(x3, self.rule, self.K, True)
        assert ctx.plane_events_dev(d["lv"], self.n, self.n, BL, d["tot"], r, d["thr"], d["st"], d["ln"], d["mk"], d["el"],
                                    self.CAP, d["cnt"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"events": ctx.events_result()}

    def expect(self, which):
        lv, tot, thr = self.content(which)
        ev, elv = P.stream_plane_events(lv, tot, BL, self.rule, [t[0] for t in thr])
        _, st, ln, mk, sl = P.slots(ev, elv, self.CAP, False)
        out = {"st": [(0, st, False)], "ln": [(0, ln, False)], "mk": [(0, mk, False)], "el": [(0, sl, False)],
               "cnt": [(0, np.array([len(ev)], dtype=np.uint64), False)]}
        return {"out": out, "result": {"events": (0, len(ev))}}


def test_behind_a_stalled_stream(x3, T):
    import torch
    case = StalledPlaneEvents(T)
    AC.check_pair_differs(case)
    AC.run_stalled(x3, torch, case, AC.calibrate_sleep(torch))


# ------------------------------------------------------------------------------------------------ end to end
def _example_planes(w, n, bin_len=200):
    frames, so = [w[a:a + 2_000] for a in range(0, n, 2_000)], range(0, n, 2_000)
    tone = B.tone_bank_levels(frames, [0] * len(frames), so, bin_len, -(-n // bin_len), B.EXAMPLE_STEPS)
    return np.stack([TR.tone_power_levels(p) for p in tone])


def test_the_example_bank_events_then_bank_range_levels(ctx, x3):
    """DESIGN.md section 28's example through bank_events, and tone_bank_range_levels(..., band=True) on the tensors it
    returns as they are"""
    w = P.example()
    p = x3.Params.make(20, 100)
    rc, stream, _ = O.encode(w, O.Params.make(20, 100, (0, 1, 3)))
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        tones = [x3.Tone(s) for s in B.EXAMPLE_STEPS]
        planes = _example_planes(w, w.size)
        cap = 6
        want = {1: [(4_400, 200, 1), (8_000, 400, 3), (12_000, 200, 2), (16_000, 200, 7)], 2: [(16_000, 200, 7)],
                3: [(16_000, 200, 7)], 4: []}
        for mp in (1, 2, 3, 4):
            rule = P.PlaneRule([400_000] * 4, [0] * 4, mp)
            st, ln, cnt, mk, el = ws.bank_events(200, tones, c_rule(x3, rule, 4), cap)
            ev, elv = P.stream_plane_events(planes, w.size, 200, rule)
            assert ev == want[mp] and int(cnt) == len(ev) and st.is_cuda and cnt.dim() == 0
            _, wst, wln, wmk, wlv = P.slots(ev, elv, cap, False)
            assert np.array_equal(st.cpu().numpy().view(np.uint64), wst) and np.array_equal(ln.cpu().numpy().view(np.uint32), wln)
            assert np.array_equal(mk.cpu().numpy().view(np.uint32), wmk) and tuple(el.shape) == (4, cap, 32)
            got = np.stack([x3.event_levels_view(el[t]) for t in range(4)])
            assert got.tobytes() == wlv.tobytes()
            if mp == 1:
                ms = [[int(got[t][i]["sum_sq"]) // int(got[t][i]["n"]) for t in range(4)] for i in (1, 3)]
                assert ms == [[236_813, 373_441, 13_655, 38_396], [689_075, 685_892, 601_612, 6_780]]
                # the list goes to the bank range levels as it lies: one bin per event, fillers are identity rows
                rl, _, rst = ws.tone_bank_range_levels(st, ln, 0, tones, padded_to=1, band=True)
                assert not rst.cpu().numpy().any() and tuple(rl.shape)[:2] == (4, cap)
                rows = np.stack([x3.event_levels_view(rl[t]) for t in range(4)])
                assert (rows["n"][:, :4] == np.array([200, 400, 200, 200])).all() and not rows["n"][:, 4:].any()
        # records of any origin: the reference's planes through plane_events give the same list
        import torch
        t_lv = torch.from_numpy(planes.view(np.uint8).reshape(4, -1, 32).copy()).cuda()
        st, ln, cnt, mk, el = ws.plane_events(t_lv, 200, c_rule(x3, P.PlaneRule([400_000] * 4, [0] * 4, 1), 4), cap)
        assert int(cnt) == 4 and mk.cpu().numpy()[:4].tolist() == [1, 3, 2, 7]
    finally:
        ws.close()


def test_adaptive_bank_events_on_a_corpus_of_two_noise_floors(ctx, x3):
    rng = np.random.RandomState(3)
    clips = []
    for e, amp in enumerate((300, 3000)):
        w = rng.randint(-amp, amp + 1, 6_000).astype(np.int64)
        t = np.arange(2_000 + 1_000 * e, 2_200 + 1_000 * e)
        w[t] += np.rint(4 * amp * np.sin(2 * np.pi * B.EXAMPLE_FREQS[e] * t)).astype(np.int64)
        clips.append(np.clip(w, -32768, 32767).astype(np.int16))
    parts = []
    for w in clips:
        rc, s, _ = O.encode(w, O.Params.make(20, 100, (0, 1, 3)))
        assert rc == 0
        parts.append(s)
    offs = np.concatenate([[0], np.cumsum([q.size for q in parts])])[:-1]
    corpus = x3.Corpus(ctx, np.concatenate(parts + [np.zeros(16, dtype=np.uint8)]), offs, [q.size for q in parts],
                       params=x3.Params.make(20, 100), seg_blocks=8)
    try:
        tones = [x3.Tone(s) for s in B.EXAMPLE_STEPS[:2]]
        trule = Q.TRule(mean_sq=(500_000, 8, 1, 0))                   # 9 dB over the median band level, per plane and entry
        rule = P.PlaneRule([0, 0], [0, 0], 1)
        cap = 5
        ent, st, ln, cnt, mk, el, thr = corpus.adaptive_bank_events(200, tones, x3.ThresholdRule.make(mean_sq=trule.mean_sq),
                                                                    c_rule(x3, rule, 2, True), cap)
        planes = np.concatenate([_example_planes(w, w.size)[:2] for w in clips], axis=1)
        ns = [w.size for w in clips]
        want_thr = [Q.corpus_thresholds(planes[t], ns, 200, trule) for t in range(2)]
        got_thr = thr.cpu().numpy().view(x3.EVENT_THRESHOLD_DTYPE).reshape(2, 2)
        assert [[tuple(int(v) for v in got_thr[t][e]) for e in range(2)] for t in range(2)] == want_thr
        assert want_thr[0][1][0] > 20 * want_thr[0][0][0]             # two noise floors, two thresholds
        ev, elv = P.corpus_plane_events(planes, ns, 200, rule, want_thr)
        assert ev == [(0, 2_000, 200, 1), (1, 3_000, 200, 2)] and int(cnt) == 2
        went, wst, wln, wmk, wlv = P.slots(ev, elv, cap, True)
        assert np.array_equal(ent.cpu().numpy().view(np.uint32), went) and np.array_equal(st.cpu().numpy().view(np.uint64), wst)
        assert np.array_equal(ln.cpu().numpy().view(np.uint32), wln) and np.array_equal(mk.cpu().numpy().view(np.uint32), wmk)
        assert np.stack([x3.event_levels_view(el[t]) for t in range(2)]).tobytes() == wlv.tobytes()
    finally:
        corpus.close()
