"""Band levels (include/x3hip.h, "SPECTRA, BAND LEVELS"): x3_spectra_levels_dev and the Python surface on top of it.  Every
record, row offset and status is compared with == against spectra_levels_ref.py, the definition (integers: no tolerance
anywhere), and the tile-edge cases also against a torch reduction of the POWER rows that x3_spectra_rows_dev itself writes
from the same inputs.  Every output array is filled with 0x5A first and carries canary bytes behind its end, and what a
call may not write must keep its 0x5A.  The rule and fold structs are overwritten right behind every call: they were copied
at the call."""
import ctypes as C

import numpy as np
import pytest

import async_cases as AC
import spectra_levels_ref as SL
import spectra_ref as S
import test_gpu_spectra as TS
import tone_levels_ref as TL

pytestmark = pytest.mark.gpu

BAD = S.ERR_BAD_ARG
GUARD = TS.GUARD
WILD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def band_map(n_fft, kind):
    """(bin_band, K): "one": every bin in band 0; "eight": eight bands that are not contiguous, with bins in no band (a word
    of 8, 0x80000000 and 0xFFFFFFFF among them) and band 5 empty; "bins": a band per bin"""
    nb = S.n_bins(n_fft)
    if kind == "one":
        return np.zeros(nb, dtype=np.uint32), 1
    if kind == "bins":
        return np.arange(nb, dtype=np.uint32), nb
    m = (np.arange(nb, dtype=np.uint32) * 3) % 8
    m[m == 5] = 8
    m[1], m[7], m[nb - 1] = WILD, 0x80000000, WILD
    return m, 8


def run(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap, plane_stride=0,
        tab=None, in_place=False, null_offsets=False, samples_cap=None, tight=False):
    """one call -> (records as spectra_levels_ref lays them, row offsets, status, the result call's tuple); the canaries are
    checked.  tight: no canary bytes, every buffer allocated at its exact size (for a run under guard pages)."""
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    offsets = np.array([int(v) for v in offsets], dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    n, guard = lens.size, 0 if tight else GUARD
    cap_s = samples.size if samples_cap is None else samples_cap
    ps = plane_stride or rows_cap
    # (the last plane ends at its rows_cap: the records behind it up to plane_stride are not the call's, so not allocated)
    sizes = (32 * ((n_bands - 1) * ps + rows_cap), 8 * (n + 1), 4 * n)
    bufs = [ctx.alloc(s + guard) for s in sizes] + [ctx.alloc(max(2 * samples.size, 2)), ctx.alloc(8 * n), ctx.alloc(4 * n),
                                                    ctx.alloc(4 * n), ctx.alloc(4 * S.PAIRS), ctx.alloc(4 * S.n_bins(n_fft))]
    d_out, d_ro, d_st, d_x, d_off, d_len, d_in, d_tab, d_map = bufs
    try:
        for q, s in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(s + guard, 0x5A, dtype=np.uint8))
        if samples.size:
            ctx.upload(d_x, samples)
        ctx.upload(d_off, offsets)
        ctx.upload(d_len, lens)
        ctx.upload(d_tab, TL.table() if tab is None else np.ascontiguousarray(tab, dtype=np.int16))
        ctx.upload(d_map, np.ascontiguousarray(bin_band, dtype=np.uint32))
        if in_status is not None:
            ctx.upload(d_st if in_place else d_in, np.array(in_status, dtype=np.int32))
        rule = x3.SpectraRule(n_fft, hop, S.POWER, 0, d_tab)
        fold = x3.SpectraFold(per_bin, n_bands, plane_stride, d_map, 0)
        rc = ctx.spectra_levels_dev(d_x, cap_s, d_off, d_len, None if in_status is None else (d_st if in_place else d_in), n, rule,
                                    fold, stride, d_out, rows_cap, None if null_offsets else d_ro, d_st)
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        C.memset(C.byref(fold), 0xEE, C.sizeof(fold))
        assert rc == 0, ctx.last_error()
        res = ctx.spectra_result()
        raw = [ctx.download(q, s + guard) for q, s in zip(bufs[:3], sizes)]
    finally:
        for q in bufs:
            ctx.free(q)
    for name, a, s in zip(("d_levels", "d_row_offsets", "d_status"), raw, sizes):
        assert (a[s:] == 0x5A).all(), "the canary behind %s is damaged" % name
    out = np.full(n_bands * ps * 32, 0x5A, dtype=np.uint8)
    out[:sizes[0]] = raw[0][:sizes[0]]
    return out.view(SL.LEVEL).reshape(n_bands, ps), raw[1][:sizes[1]].view(np.uint64), raw[2][:sizes[2]].view(np.int32), res


def check(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap, plane_stride=0,
          tab=None, powers=None, **kw):
    """one call against the definition: every record of every plane (those the call leaves alone keep 0x5A -- the records
    between rows_cap and plane_stride among them), offsets, statuses, the result"""
    got = run(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap, plane_stride, tab, **kw)
    cap_s = kw.get("samples_cap")
    ref_samples = samples if cap_s is None else np.asarray(samples, dtype=np.int16)[:cap_s]
    want = SL.spectra_levels(ref_samples, offsets, lens, in_status, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap,
                             plane_stride, tab, powers=powers)
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    if not kw.get("null_offsets"):
        assert np.array_equal(got[1], want[1]), (got[1], want[1])
    else:
        assert (got[1].view(np.uint8) == 0x5A).all()
    if not np.array_equal(got[0], want[0]):
        b, r = [int(v[0]) for v in np.nonzero(got[0] != want[0])]
        raise AssertionError("N %d hop %d M %d K %d stride %d cap %d: %d records differ; plane %d row %d: got %s, want %s" % (
            n_fft, hop, per_bin, n_bands, stride, rows_cap, int((got[0] != want[0]).sum()), b, r, got[0][b, r], want[0][b, r]))
    bad = np.flatnonzero(want[2])
    assert got[3] == (0, bad.size, int(bad[0]) if bad.size else len(lens), int(want[2][bad[0]]) & 0xFF if bad.size else 0, want[3]), got[3]
    return got


def torch_fold(ms, counts, per_bin, bin_band, n_bands):
    """the second route: POWER rows [sum(counts), B] as x3_spectra_rows_dev wrote them (packed) -> LEVEL [K, sum of T], by
    torch's index_add and segment_reduce"""
    import torch
    ms = torch.from_numpy(ms.astype(np.int64))
    m = torch.from_numpy(np.asarray(bin_band, dtype=np.uint32).astype(np.int64))
    keep = m < n_bands
    bp = torch.zeros((ms.shape[0], n_bands), dtype=torch.int64).index_add_(1, m[keep], ms[:, keep]).clamp_(max=1 << 30)
    seg = []
    for r in counts:
        seg += [per_bin] * (r // per_bin) + ([r % per_bin] if r % per_bin else [])
    t = len(seg)
    out = np.zeros((n_bands, t), dtype=SL.LEVEL)
    if t == 0:
        return out
    seg_t = torch.tensor(seg, dtype=torch.int64)
    tot = torch.segment_reduce(bp.to(torch.float64), "sum", lengths=seg_t, axis=0)      # (below 2^53: exact in float64)
    top = torch.segment_reduce(bp.to(torch.float64), "max", lengths=seg_t, axis=0)
    peak = np.minimum(SL.isqrt(2 * top.numpy().astype(np.int64)), 32767)
    out["sum_sq"], out["max"], out["min"], out["n"] = tot.numpy().astype(np.uint64).T, peak.T, -peak.T, np.array(seg)[None, :]
    return out


# ------------------------------------------------------------------------------------------------ 1. tile edges
@pytest.mark.parametrize("n_fft", [64, 128, 1024])
@pytest.mark.parametrize("hop_of", ["1", "N/2", "N+5"])
def test_time_bins_at_the_tiles_and_the_ranges_edges(x3, ctx, n_fft, hop_of):
    """15, 16, 17 and 33 frames from several ranges (a tile holds 32 frames, 16 at n_fft 1 024), time bins of 1, 3, 7, 16 and 33
    frames: bins straddle tile edges, range edges fall inside a tile, the last bin of a range is partial; one band, eight
    and a band per bin.  Against the definition, and against the rows call's own POWER rows reduced by torch."""
    hop = {"1": 1, "N/2": n_fft // 2, "N+5": n_fft + 5}[hop_of]
    for total, counts in TS.SPLITS.items():
        offsets, lens, need = TS.rows_layout(counts, n_fft, hop)
        x = TS.noise(need, total)
        rows = TS.run(x3, ctx, x, offsets, lens, None, n_fft, hop, S.POWER, 0, total)[0]     # the parent's code
        powers = {}
        for per_bin in (1, 3, 7, 16, 33):
            cap = sum(SL.n_bins_of(r, per_bin) for r in counts)
            for kind in ("one", "eight", "bins"):
                m, k = band_map(n_fft, kind)
                got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, cap, powers=powers)
                assert np.array_equal(got[0], torch_fold(rows, counts, per_bin, m, k)), (total, per_bin, kind)
    m, k = band_map(n_fft, "bins")
    got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, 1, m, k, 0, total, powers=powers)
    assert np.array_equal(got[0]["sum_sq"].T, rows)                   # M = 1, a band per bin: sum_sq is the POWER word


def test_many_workgroups_into_one_record(x3, ctx):
    """20 000 frames of one range at time bins of 5 000: 157 tiles add into each record, the atomics' sums are exact"""
    n_fft, hop, frames, per_bin = 64, 16, 20_000, 5_000
    x = TS.noise(n_fft + (frames - 1) * hop, 31)
    for kind in ("one", "eight"):
        m, k = band_map(n_fft, kind)
        got = check(x3, ctx, x, [0], [x.size], None, n_fft, hop, per_bin, m, k, 0, 4)
        assert got[0]["n"].tolist() == [[per_bin] * 4] * k and got[3][4] == 4


def test_more_tiles_than_one_pass_of_the_grid(x3, ctx):
    """131 333 frames at n_fft 64, hop 1: more tiles of 32 than the 4 096 workgroups of the capped grid, so workgroups take a
    second tile and their accumulators must be zero again; time bins of 3 frames never align with a tile"""
    n_fft, frames, per_bin = 64, 4096 * 32 + 8 * 32 + 5, 3
    x = TS.noise(n_fft + frames - 1, 21)
    m, k = band_map(n_fft, "eight")
    cap = SL.n_bins_of(frames, per_bin)
    got = check(x3, ctx, x, [0], [x.size], None, n_fft, 1, per_bin, m, k, 0, cap)
    assert got[3][4] == cap and got[0]["n"][0, -1] == frames % per_bin


# ------------------------------------------------------------------------------------------------ 2. content
def clamp_table():
    t = np.zeros((S.PAIRS, 2), dtype=np.int16)
    t[:, 0] = 32767
    return t


@pytest.mark.parametrize("n_fft", [64, 256, 1024])
@pytest.mark.parametrize("table", ["usual", "clamp", "random"])
def test_content(x3, ctx, n_fft, table):
    """rows of -32768, of 32767 and of the eight values at which the byte split turns over; the usual table, the table of
    all (32767, 0) -- every bin of a full-scale row is at its clamp, so a band of all bins passes 2^30 before its own clamp
    -- and a random one; wild map words and an empty band ("eight")"""
    tab = {"usual": None, "clamp": clamp_table(), "random": TS.random_table()}[table]
    ln = 5 * n_fft + 7
    rows = [np.full(ln, -32768), np.full(ln, 32767), np.resize(np.array(TS.EDGE_VALUES), ln), np.resize(np.array(TS.EDGE_VALUES[::-1]), ln)]
    x = np.concatenate(rows).astype(np.int16)
    offsets, lens = [i * ln for i in range(4)], [ln] * 4
    for hop in (n_fft, 7):
        powers = {}
        for per_bin in (1, 3):
            cap = 4 * SL.n_bins_of(S.n_rows(ln, n_fft, hop), per_bin)
            for kind in ("one", "eight", "bins"):
                m, k = band_map(n_fft, kind)
                got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, cap, tab=tab, powers=powers)
                if kind == "eight":
                    assert not got[0]["sum_sq"][5].any() and (got[0]["max"][5] == 0).all() and got[0]["n"][5].all()   # the empty band
                if kind == "one" and table == "clamp":
                    ms = powers[(ln, ln)]                              # the row of 32767
                    assert int(ms[0].astype(np.int64).sum()) > 1 << 30                      # unclamped, the band passes 2^30
                    t1 = cap // 4
                    assert (got[0]["sum_sq"][0, t1:2 * t1] == (got[0]["n"][0, t1:2 * t1].astype(np.uint64) << 30)).all()
                    assert (got[0]["max"][0, t1:2 * t1] == 32767).all()


# ------------------------------------------------------------------------------------------------ 3. statuses and layouts
@pytest.mark.parametrize("n_fft, hop", [(64, 48), (1024, 100)])
def test_statuses_and_layouts(x3, ctx, n_fft, hop):
    counts, offsets, lens, x = TS._status_rows(n_fft, hop)           # frames 3, 2, 0, 5, 1, 4
    per_bin = 2
    bins = [SL.n_bins_of(r, per_bin) for r in counts]                # 2, 1, 0, 3, 1, 2
    total = sum(bins)
    m, k = band_map(n_fft, "eight")
    powers = {}
    ins = [0, 14, 0, 21, 0, 0]
    for in_place in (False, True):      # the in-status comes out, its records are the identity
        got = check(x3, ctx, x, offsets, lens, ins, n_fft, hop, per_bin, m, k, 0, total, powers=powers, in_place=in_place)
        assert got[2].tolist() == ins and (got[0][:, 3:6] == SL.IDENTITY).all() and got[0]["n"][:, 0:2].all()
        check(x3, ctx, x, offsets, lens, ins, n_fft, hop, per_bin, m, k, 4, 24, powers=powers, in_place=in_place)
    # wild offsets and lengths against samples_cap: the status, identity records, nothing read
    wild = list(offsets)
    wild[0], wild[3] = 2 ** 63 + 1, x.size - lens[3] + 1
    got = check(x3, ctx, x, wild, lens, None, n_fft, hop, per_bin, m, k, 0, total)
    assert got[2].tolist() == [BAD, 0, 0, BAD, 0, 0]
    got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, total, powers=powers, samples_cap=offsets[4] + lens[4])
    assert got[2].tolist() == [0, 0, 0, 0, 0, BAD]
    # packed past rows_cap: the range is refused, every record below rows_cap is still the call's (the identity), the total
    # says what all need
    for cap in (total - 1, 5, 4, 1):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, cap, powers=powers)
        assert got[3][4] == total and got[2].tolist() == [BAD if a + r > cap else 0 for a, r in zip(np.cumsum([0] + bins), bins)]
        assert (got[0].view(np.uint8) != 0x5A).reshape(k, cap, 32).any(axis=2).all()
    # padded: the identity behind T(w), T(w) > stride, no d_row_offsets
    for stride in (3, 2, 1):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, stride, 6 * stride + 1, powers=powers,
                    null_offsets=(stride == 2))
        assert got[2].tolist() == [BAD if r > stride else 0 for r in bins]
        assert (got[0][:, 6 * stride:].view(np.uint8) == 0x5A).all()   # the record behind n * stride is not the call's
    # planes further apart than rows_cap: the records in between keep their 0x5A (check compares them)
    for stride, cap, ps in ((0, total, total + 3), (0, 5, 11), (3, 18, 19)):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, stride, cap, ps, powers=powers)
        assert (got[0][:-1, cap:].view(np.uint8) == 0x5A).all()
    # lengths 0, N - 1, N and events' fillers (0, 0)
    lens2 = [0, n_fft - 1, n_fft, n_fft + hop, 0, 0]
    offs2 = [1, 3, 3 + n_fft, 5, 0, 0]
    got = check(x3, ctx, x, offs2, lens2, None, n_fft, hop, per_bin, m, k, 0, 2)
    assert not got[2].any() and got[1].tolist() == [0, 0, 0, 1, 2, 2, 2] and got[0]["n"][0].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_argument_refusals_enqueue_nothing(x3, ctx):
    n_fft, hop, per_bin = 64, 32, 2
    counts, offsets, lens, x = TS._status_rows(n_fft, hop)
    n, total = len(lens), sum(SL.n_bins_of(r, per_bin) for r in counts)
    m, k = band_map(n_fft, "eight")
    sizes = {"out": 32 * k * total, "ro": 8 * (n + 1), "st": 4 * n}
    d = {key: ctx.alloc(v + GUARD) for key, v in sizes.items()}
    d.update(x=ctx.alloc(2 * x.size), off=ctx.alloc(8 * n), ln=ctx.alloc(4 * n), tab=ctx.alloc(4 * S.PAIRS), map=ctx.alloc(4 * 33 + 4))
    try:
        ctx.upload(d["x"], x)
        ctx.upload(d["off"], np.array(offsets, dtype=np.uint64))
        ctx.upload(d["ln"], np.array(lens, dtype=np.uint32))
        ctx.upload(d["tab"], TL.table())
        ctx.upload(d["map"], m)

        def call(rule="ok", fold="ok", **kw):
            a = dict(d_samples=d["x"], samples_cap=x.size, d_offsets=d["off"], d_lens=d["ln"], d_in_status=None, n_ranges=n,
                     row_stride=0, d_out=d["out"], rows_cap=total, d_row_offsets=d["ro"], d_status=d["st"])
            a.update(kw)
            r = None if rule is None else x3.SpectraRule(n_fft, hop, S.POWER, 0, d["tab"])
            for key, v in ({} if rule in (None, "ok") else rule).items():
                setattr(r, key, v)
            f = None if fold is None else x3.SpectraFold(per_bin, k, 0, d["map"], 0)
            for key, v in ({} if fold in (None, "ok") else fold).items():
                setattr(f, key, v)
            return ctx.spectra_levels_dev(a["d_samples"], a["samples_cap"], a["d_offsets"], a["d_lens"], a["d_in_status"], a["n_ranges"],
                                          r, f, a["row_stride"], a["d_out"], a["rows_cap"], a["d_row_offsets"], a["d_status"])
        assert ctx.spectra_result()[0] == BAD                     # nothing pending yet
        assert call() == 0                                         # the earlier call, whose result stays to be served
        ctx.sync()
        want = {key: ctx.download(d[key], v + GUARD) for key, v in sizes.items()}
        for key, v in sizes.items():
            ctx.upload(d[key], np.full(v + GUARD, 0x5A, dtype=np.uint8))
        refused = [dict(rule=None)]
        refused += [dict(rule={"n_fft": v}) for v in (0, 32, 63, 65, 96, 2048, 1 << 31)]
        refused += [dict(rule={"hop": 0}), dict(rule={"hop": 1 << 31}), dict(rule={"format": 2}), dict(rule={"format": S.SUMS}),
                    dict(rule={"reserved": 1}), dict(rule={"d_table": None}), dict(rule={"d_table": d["tab"] + 2})]
        refused += [dict(fold=None), dict(fold={"frames_per_bin": 0}), dict(fold={"frames_per_bin": 1 << 31}), dict(fold={"n_bands": 0}),
                    dict(fold={"n_bands": 34}), dict(fold={"d_bin_band": None}), dict(fold={"d_bin_band": d["map"] + 2}),
                    dict(fold={"reserved": 1}), dict(fold={"plane_stride": total - 1}),
                    dict(fold={"plane_stride": (0x7FFFFFFF // k) + 1}), dict(fold={"n_bands": 33}, rows_cap=(0x7FFFFFFF // 33) + 1)]
        refused += [dict(n_ranges=0), dict(n_ranges=1 << 31), dict(rows_cap=0), dict(rows_cap=1 << 31)]
        refused += [dict(**{key: None}) for key in ("d_samples", "d_offsets", "d_lens", "d_out", "d_status", "d_row_offsets")]
        refused += [dict(d_samples=d["x"] + 1), dict(d_lens=d["ln"] + 2), dict(d_in_status=d["st"] + 2), dict(d_status=d["st"] + 2),
                    dict(d_offsets=d["off"] + 4), dict(d_out=d["out"] + 4), dict(d_row_offsets=d["ro"] + 4)]
        refused += [dict(row_stride=total // n + 1, d_row_offsets=None)]            # n_ranges * row_stride > rows_cap
        for kw in refused:
            assert call(**kw) == BAD, kw
        ctx.graph_begin()                                          # a context that is recording a graph: the good call itself
        try:
            assert call() == BAD
            assert call(row_stride=1, rows_cap=n, d_row_offsets=None) == BAD
        finally:
            try:
                ctx.graph_destroy(ctx.graph_end())
            except x3.X3Error:
                pass                                               # (a recording of nothing)
        ctx.sync()
        for key, v in sizes.items():
            assert (ctx.download(d[key], v + GUARD) == 0x5A).all(), "a refused call wrote to " + key
        res = ctx.spectra_result()                                 # the earlier call's result is still served
        assert res == (0, 0, n, 0, total), res
        assert ctx.spectra_result()[0] == BAD
        ref = SL.spectra_levels(x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, total)
        assert np.array_equal(want["out"][:sizes["out"]].view(SL.LEVEL).reshape(k, total), ref[0])
    finally:
        for q in d.values():
            ctx.free(q)


def test_a_rows_call_and_a_levels_call_alternate_on_one_context(x3, ctx):
    """the two calls share the pending slot and the workspace: each result is the call's own, whichever came before"""
    n_fft, hop = 128, 40
    counts = [3, 0, 9, 6]
    offsets, lens, need = TS.rows_layout(counts, n_fft, hop)
    x = TS.noise(need, 77)
    m, k = band_map(n_fft, "eight")
    powers = {}
    for per_bin in (2, 5, 1):
        cap = sum(SL.n_bins_of(r, per_bin) for r in counts)
        check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, cap, powers=powers)
        TS.check(x3, ctx, x, offsets, lens, None, n_fft, hop, S.POWER, 0, sum(counts))
        check(x3, ctx, x, offsets, lens, None, 1024, hop, per_bin, *band_map(1024, "bins"), 0, 1)   # (the workspace grows: no frame)
        TS.check(x3, ctx, x, offsets, lens, None, n_fft, hop, S.SUMS, 3, 12 + (per_bin == 5))


# ------------------------------------------------------------------------------------------------ 5. behind a stalled stream
class StalledSpectraLevels(TS.StalledSpectra):
    """TS.StalledSpectra's inputs and the band map arrive on the stream behind a stall; the rule and the fold structs are
    overwritten behind the call"""
    name = "spectra_levels"
    M, K = 4, 8

    def inputs(self, which):
        d = super().inputs(which)
        m = band_map(self.N, "eight")[0] if which == "A" else (np.arange(S.n_bins(self.N), dtype=np.uint32) % 11)
        return dict(d, map=m)

    def outputs(self):
        return {"out": 32 * self.K * self.CAP, "ro": 8 * 5, "st": 4 * 4}

    def enqueue(self, x3, ctx, d, which, probe):
        rule = x3.SpectraRule(self.N, self.HOP, S.POWER, 0, d["tab"])
        fold = x3.SpectraFold(self.M, self.K, 0, d["map"], 0)
        rc = ctx.spectra_levels_dev(d["x"], 4096, d["off"], d["ln"], d["in"] if which == "B" else None, 4, rule, fold, 0, d["out"],
                                    self.CAP, d["ro"], d["st"])
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        C.memset(C.byref(fold), 0xEE, C.sizeof(fold))
        assert rc == 0, ctx.last_error()

    def expect(self, which):
        x, offsets, lens, ins, tab = self.content(which)
        out, off, st, total = SL.spectra_levels(x, offsets, lens, ins, self.N, self.HOP, self.M, self.inputs(which)["map"], self.K, 0,
                                                self.CAP, 0, tab)
        bad = np.flatnonzero(st)
        res = (0, bad.size, int(bad[0]) if bad.size else 4, int(st[bad[0]]) if bad.size else 0, total)
        planes = [(32 * b * self.CAP, out[b, :total], False) for b in range(self.K)]
        return {"out": {"out": planes, "ro": [(0, off, False)], "st": [(0, st, False)]}, "result": {"spectra": res}}


def test_behind_a_stalled_stream(x3):
    import torch
    case = StalledSpectraLevels()
    AC.check_pair_differs(case)
    AC.run_stalled(x3, torch, case, AC.calibrate_sleep(torch))


# ------------------------------------------------------------------------------------------------ 6. end to end
def records(t):
    """uint8 [K, rows, 32] on the device -> LEVEL [K, rows]"""
    return t.cpu().numpy().view(SL.LEVEL).reshape(t.shape[0], t.shape[1])


def test_range_band_levels_over_a_damaged_frame(x3, ctx):
    import ranges_ref as RR
    wav, s, p = TS._stream(x3, hurt=2)                         # frame 2 (positions 800 .. 1199): its payload CRC fails
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        starts, lens = TS._base_ranges()
        covers = [a < 1200 and a + ln > 800 for a, ln in zip(starts, lens)]
        status = [RR.ERR_PAYLOAD_CRC if c else 0 for c in covers]
        edges = [0, 1, 4, 4, 20, 33]                           # five bands, the third without a bin
        m, k = x3.spectra_bin_band(64, edges)
        assert k == 5 and m.tolist()[:5] == [0, 1, 1, 1, 3] and m[32] == 4
        for per_bin in (1, 3):
            bins = [SL.n_bins_of(S.n_rows(v, 64, 48), per_bin) for v in lens]
            # the samples as the ranges call packs them, a damaged range's as zeros that are never transformed
            offs = np.concatenate([[0], np.cumsum(lens)])
            x = np.concatenate([wav[a:a + ln] for a, ln in zip(starts, lens)])
            for kw, stride in (({}, 0), ({"padded_to": 14}, 14)):
                cap = 14 * len(lens) if stride else sum(bins)
                lv, ro, st = src.range_band_levels(starts, lens, 64, 48, frames_per_bin=per_bin, bands=edges, **kw)
                want = SL.spectra_levels(x, offs[:-1], lens, status, 64, 48, per_bin, m, k, stride, cap)
                assert st.cpu().numpy().tolist() == status == want[2].tolist() and tuple(lv.shape) == (k, cap, 32) and lv.is_cuda
                assert np.array_equal(records(lv), want[0]) and np.array_equal(ro.cpu().numpy().view(np.uint64), want[1])
        lv, ro, st = src.range_band_levels(starts, lens, 64, 48, capacity=3)          # one band per bin; no room behind 3 rows
        assert tuple(lv.shape) == (33, 3, 32) and int(ro[-1]) == sum(S.n_rows(v, 64, 48) for v in lens) and BAD in st.cpu().numpy().tolist()
    finally:
        src.close()


def test_corpus_range_band_levels_on_two_entries(x3, ctx):
    (w0, s0, p), (w1, s1, _) = TS._stream(x3, 1500, 77), TS._stream(x3, 1000, 78)
    buf = np.concatenate([s0, np.zeros(2, dtype=np.uint8), s1, np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf, [0, s0.size + 2], [s0.size, s1.size], params=p, seg_blocks=4, index="walk")
    try:
        wavs = [w0, w1]
        entries, starts, lens = [0, 1, 0, 1], [0, 100, 333, 500], [400, 500, 128, 127]
        import torch
        m = (np.arange(65, dtype=np.uint32) * 7) % 9                    # a tensor of B band indices, 8 being "no band" at K = 8
        m[m == 8] = WILD
        lv, ro, st = corpus.range_band_levels(entries, starts, lens, 128, 64, frames_per_bin=2, bands=torch.from_numpy(m.view(np.int32)))
        assert not st.cpu().numpy().any() and lv.shape[0] == 8
        want = np.concatenate([SL.levels_of(wavs[e][a:a + ln], 128, 64, 2, m, 8) for e, a, ln in zip(entries, starts, lens)], axis=1)
        assert np.array_equal(records(lv), want)
    finally:
        corpus.close()


def test_band_levels_of_a_whole_stream_in_three_chunks(x3, ctx):
    """2 137 samples, n_fft 64, hop 32, time bins of 3 frames (96 positions), q = 2: ranges of 224 samples at multiples of
    192, twelve of them, the last one 25 samples long; chunk_samples 1 000 holds four ranges, so three chunks.  The planes
    equal one range_band_levels call over (0, total) where the rows hold all their frames, and the definition everywhere."""
    wav, s, p = TS._stream(x3)
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        n_fft, hop, per_bin, q = 64, 32, 3, 2
        bin_len = per_bin * hop
        edges = x3.band_edges_third_octave(n_fft, 16000, 800, 6400)
        m, k = x3.spectra_bin_band(n_fft, edges)
        lv = src.band_levels(n_fft, hop, frames_per_bin=per_bin, bands=edges, chunk_samples=1000, q=q)
        rows = -(-wav.size // bin_len)
        assert tuple(lv.shape) == (k, rows, 32) and rows == 23 and -(-wav.size // (q * bin_len)) == 12
        got = records(lv)
        want = np.full((k, rows), SL.IDENTITY, dtype=SL.LEVEL)
        for g in range(12):                                        # the definition: range g's rows at 2 g
            part = SL.levels_of(wav[g * q * bin_len:g * q * bin_len + (q * per_bin - 1) * hop + n_fft], n_fft, hop, per_bin, m, k)
            want[:, g * q:g * q + part.shape[1]] = part
        assert np.array_equal(got, want)
        one = records(src.range_band_levels([0], [wav.size], n_fft, hop, frames_per_bin=per_bin, bands=edges)[0])
        whole = one.shape[1] - 1                                   # (the single range's last bin may be partial)
        assert whole >= 20 and np.array_equal(got[:, :whole], one[:, :whole]) and (got["n"][:, :whole] == per_bin).all()
        assert (got[:, -1] == SL.IDENTITY).all()                  # the trailing row: 25 samples, no whole frame
    finally:
        src.close()


def test_band_levels_equal_the_tone_adapter_and_feed_plane_events(x3, ctx):
    """n_fft = hop = 64 and a frame per bin: every frame is aligned, so plane b of eight chosen bins holds what plane b of
    tone_bank_levels(band=True) at step k * 2^32 / 64 holds -- the same sum_sq / n (the adapter counts the 64 samples, this
    call the one frame), max and min; the planes through plane_events equal plane_events_ref on the definition's planes"""
    import plane_events_ref as P
    import test_gpu_plane_events as TP
    wav, s, p = TS._stream(x3)
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        n_fft = 64
        bins = [0, 1, 2, 5, 16, 31, 32, 7]
        m = np.full(33, WILD, dtype=np.uint32)
        m[bins] = np.arange(8)
        import torch
        lv = src.band_levels(n_fft, frames_per_bin=1, bands=torch.from_numpy(m.view(np.int32)))
        rows = -(-wav.size // n_fft)
        whole = wav.size // n_fft
        assert tuple(lv.shape) == (8, rows, 32) and whole == rows - 1
        tones = tuple(x3.Tone(kk * (2 ** 32 // n_fft)) for kk in bins)
        band = src.tone_bank_levels(n_fft, tones, band=True)[0][:, :whole]
        mine = records(lv)[:, :whole]
        assert (band["n"] == n_fft).all() and (mine["n"] == 1).all() and np.array_equal(mine["sum_sq"], band["sum_sq"] // n_fft)
        assert np.array_equal(mine["max"], band["max"]) and np.array_equal(mine["min"], band["min"]) and not mine["sum"].any()
        want = np.full((8, rows), SL.IDENTITY, dtype=SL.LEVEL)
        want[:, :whole] = SL.levels_of(wav, n_fft, n_fft, 1, m, 8)
        assert np.array_equal(records(lv), want)
        level = int(np.median(want["sum_sq"][:, :whole]))
        rule = P.PlaneRule([max(level, 1)] * 8, [0] * 8, 3)
        cap = rows
        st, ln, cnt, mk, el = src.plane_events(lv, n_fft, TP.c_rule(x3, rule, 8), cap)
        ev, elv = P.stream_plane_events(want.view(x3.LEVEL_DTYPE), wav.size, n_fft, rule)
        _, wst, wln, wmk, wlv = P.slots(ev, elv, cap, False)
        assert int(cnt) == len(ev) and len(ev) > 0
        assert np.array_equal(st.cpu().numpy().view(np.uint64), wst) and np.array_equal(ln.cpu().numpy().view(np.uint32), wln)
        assert np.array_equal(mk.cpu().numpy().view(np.uint32), wmk)
        assert np.array_equal(el.cpu().numpy().view(x3.LEVEL_DTYPE).reshape(8, cap), wlv)
    finally:
        src.close()


# ------------------------------------------------------------------------------------------------ 7. under guard pages
def fence_run(x3):
    """the body of the child of test_under_guard_pages: tile edges, statuses and layouts with buffers of exactly their bytes
    (X3HIP_FENCE_TIGHT ends every mapping at the buffer's last byte, the library's workspace included), each group on a
    Context of its own -> the calls made"""
    calls = 0
    for n_fft, hop in ((64, 1), (128, 48), (1024, 1029)):
        ctx = x3.Context(0)
        try:
            for total, counts in TS.SPLITS.items():
                offsets, lens, need = TS.rows_layout(counts, n_fft, hop)
                x = TS.noise(need, total)
                powers = {}
                for per_bin, kind in ((1, "bins"), (3, "eight"), (33, "one")):
                    m, k = band_map(n_fft, kind)
                    check(x3, ctx, x, offsets, lens, None, n_fft, hop, per_bin, m, k, 0, sum(SL.n_bins_of(r, per_bin) for r in counts),
                          powers=powers, tight=True)
                    calls += 1
        finally:
            ctx.close()
    for n_fft, hop in ((64, 48), (1024, 100)):
        ctx = x3.Context(0)
        try:
            counts, offsets, lens, x = TS._status_rows(n_fft, hop)
            x = x[:offsets[-1] + lens[-1]]                     # the last row ends the samples' mapping
            bins = [SL.n_bins_of(r, 2) for r in counts]
            total = sum(bins)
            m, k = band_map(n_fft, "eight")
            powers = {}
            check(x3, ctx, x, offsets, lens, [0, 14, 0, 21, 0, 0], n_fft, hop, 2, m, k, 0, total, powers=powers, in_place=True, tight=True)
            wild = list(offsets)
            wild[0], wild[3] = 2 ** 63 + 1, x.size - lens[3] + 1
            check(x3, ctx, x, wild, lens, None, n_fft, hop, 2, m, k, 0, total, tight=True)
            check(x3, ctx, x, offsets, lens, None, n_fft, hop, 2, m, k, 0, 5, powers=powers, tight=True)
            check(x3, ctx, x, offsets, lens, None, n_fft, hop, 2, m, k, 2, 12, powers=powers, null_offsets=True, tight=True)
            check(x3, ctx, x, offsets, lens, None, n_fft, hop, 2, m, k, 0, total, total + 5, powers=powers, tight=True)
            calls += 5
        finally:
            ctx.close()
    return calls


def test_under_guard_pages():
    """one child process under X3HIP_FENCE=16 X3HIP_FENCE_FILL=165 X3HIP_FENCE_TIGHT=1, started as
    test_gpu_fence_analysis.py starts its children: the cases above with exact-fit buffers, then 150 trials of the fuzz
    family (z) of tools/fuzz_parity.py in three runs of 50, each on a Context of its own"""
    import test_gpu_fence_analysis as FA
    out = FA._child("""
        import x3hip, test_gpu_spectra_levels as TSL
        print("calls", TSL.fence_run(x3hip), flush=True)
        import fuzz_parity as FZ
        total = 0
        for seed in (11, 12, 13):
            c = FZ.run(seed=seed, trials=50, families="z", context=None)
            assert sum(c.values()) == c["z"]
            total += c["z"]
        print("trials", total)
        """, timeout=240)
    assert int(out.split("calls")[1].split()[0]) == 3 * 4 * 3 + 2 * 5 and int(out.split("trials")[1]) == 150
