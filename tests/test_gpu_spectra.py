"""Spectra (include/x3hip.h, "SPECTRA"): x3_spectra_rows_dev, x3_spectra_result and the Python surface.  Every output word,
row offset and status is compared with == against spectra_ref.py, the definition (integers: no tolerance anywhere); every
output array is filled with 0x5A first and carries canary bytes behind its end, and what a call may not write must keep its
0x5A.  The rule struct is overwritten right behind every call: it was copied at the call.

The call transforms int16 rows that lie in HBM, so the cases that are about rows, tiles, statuses and layouts upload their
rows as they are; the end-to-end cases decode them from a stream of 2 137 samples in frames of
400 from the oracle's encoder, and from plane_events_ref.py's example signal."""
import ctypes as C

import numpy as np
import pytest

import async_cases as AC
import spectra_ref as S
import tone_levels_ref as TL

pytestmark = pytest.mark.gpu

BAD = S.ERR_BAD_ARG
GUARD = 64
EDGE_VALUES = [-129, -128, -1, 0, 127, 128, 255, 256]   # where the low byte and the high byte of the split turn over


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def ones_table():
    t = np.zeros((S.PAIRS, 2), dtype=np.int16)
    t[:, 0] = 1
    return t


def random_table(seed=5):
    t = np.random.default_rng(seed).integers(-32768, 32768, (S.PAIRS, 2)).astype(np.int16)
    t[0], t[1], t[511], t[512] = (-32768, 32767), (32767, -32768), (-129, 128), (128, -129)
    return t


def out_bytes(n_fft, fmt):
    return S.n_bins(n_fft) * (16 if fmt == S.SUMS else 4)


def run(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, fmt, stride, rows_cap, tab=None, in_place=False,
        null_offsets=False, samples_cap=None, tight=False):
    """one call -> (out as spectra_ref lays it, row offsets, status, the result call's tuple); the canaries are checked.
    tight: no canary bytes, every buffer allocated at its exact size (for a run under guard pages)."""
    samples = np.ascontiguousarray(samples, dtype=np.int16)
    offsets = np.array([int(v) for v in offsets], dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    n, guard = lens.size, 0 if tight else GUARD
    cap_s = samples.size if samples_cap is None else samples_cap
    sizes = (out_bytes(n_fft, fmt) * rows_cap, 8 * (n + 1), 4 * n)
    bufs = [ctx.alloc(s + guard) for s in sizes] + [ctx.alloc(max(2 * samples.size, 2)), ctx.alloc(8 * n), ctx.alloc(4 * n),
                                                    ctx.alloc(4 * n), ctx.alloc(4 * S.PAIRS)]
    d_out, d_ro, d_st, d_x, d_off, d_len, d_in, d_tab = bufs
    try:
        for q, s in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(s + guard, 0x5A, dtype=np.uint8))
        if samples.size:
            ctx.upload(d_x, samples)
        ctx.upload(d_off, offsets)
        ctx.upload(d_len, lens)
        ctx.upload(d_tab, TL.table() if tab is None else np.ascontiguousarray(tab, dtype=np.int16))
        if in_status is not None:
            ctx.upload(d_st if in_place else d_in, np.array(in_status, dtype=np.int32))
        rule = x3.SpectraRule(n_fft, hop, fmt, 0, d_tab)
        rc = ctx.spectra_rows_dev(d_x, cap_s, d_off, d_len, None if in_status is None else (d_st if in_place else d_in), n, rule,
                                  stride, d_out, rows_cap, None if null_offsets else d_ro, d_st)
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        assert rc == 0, ctx.last_error()
        res = ctx.spectra_result()
        raw = [ctx.download(q, s + guard) for q, s in zip(bufs[:3], sizes)]
    finally:
        for q in bufs:
            ctx.free(q)
    for name, a, s in zip(("d_out", "d_row_offsets", "d_status"), raw, sizes):
        assert (a[s:] == 0x5A).all(), "the canary behind %s is damaged" % name
    nb = S.n_bins(n_fft)
    out = raw[0][:sizes[0]].view(np.int64).reshape(rows_cap, nb, 2) if fmt == S.SUMS else raw[0][:sizes[0]].view(np.uint32).reshape(rows_cap, nb)
    return out, raw[1][:sizes[1]].view(np.uint64), raw[2][:sizes[2]].view(np.int32), res


def check(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, fmt, stride, rows_cap, tab=None, want=None, **kw):
    """one call against the definition: every word of the rows (those the call leaves alone keep 0x5A), offsets, statuses,
    the result"""
    got = run(x3, ctx, samples, offsets, lens, in_status, n_fft, hop, fmt, stride, rows_cap, tab, **kw)
    cap_s = kw.get("samples_cap")
    ref_samples = samples if cap_s is None else np.asarray(samples, dtype=np.int16)[:cap_s]
    want = want or S.spectra_rows(ref_samples, offsets, lens, in_status, n_fft, hop, fmt, stride, rows_cap, tab)
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    if not kw.get("null_offsets"):
        assert np.array_equal(got[1], want[1]), (got[1], want[1])
    else:
        assert (got[1].view(np.uint8) == 0x5A).all()
    if not np.array_equal(got[0], want[0]):
        rows = np.flatnonzero((got[0] != want[0]).reshape(rows_cap, -1).any(axis=1))
        r = int(rows[0])
        cols = np.flatnonzero((got[0][r] != want[0][r]).reshape(S.n_bins(n_fft), -1).any(axis=1))
        raise AssertionError("N %d hop %d fmt %d stride %d: rows %s differ; row %d bins %s: got %s, want %s" % (
            n_fft, hop, fmt, stride, rows[:8].tolist(), r, cols[:6].tolist(), got[0][r][cols[:3]].tolist(), want[0][r][cols[:3]].tolist()))
    bad = np.flatnonzero(want[2])
    assert got[3] == (0, bad.size, int(bad[0]) if bad.size else len(lens), int(want[2][bad[0]]) & 0xFF if bad.size else 0, want[3]), got[3]
    return got


def rows_layout(row_counts, n_fft, hop, first=1, gap=1, slack=3):
    """ranges with the given frame counts (0: a row one sample short of a frame), laid at odd sample offsets -> (offsets, lens,
    samples needed)"""
    offsets, lens, at = [], [], first
    for r in row_counts:
        ln = n_fft - 1 if r == 0 else n_fft + (r - 1) * hop + min(hop - 1, slack)
        offsets.append(at)
        lens.append(ln)
        at += ln + gap + (at + ln + gap + 1) % 2    # (the next offset is odd again)
    return offsets, lens, at


def noise(n, seed=3):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


SPLITS = {15: [4, 0, 7, 1, 3], 16: [5, 11], 17: [16, 1], 33: [9, 0, 13, 2, 9]}


# ------------------------------------------------------------------------------------------------ 1. rows at the tile's edge
@pytest.mark.parametrize("n_fft", [64, 128, 1024])
@pytest.mark.parametrize("hop_of", ["1", "48", "N/2", "N", "N+5"])
def test_rows_at_the_matrix_tiles_edge(x3, ctx, n_fft, hop_of):
    """15, 16, 17 and 33 rows from several ranges: a tile of 16 rows holds the end of one range and the start of the next"""
    hop = {"1": 1, "48": 48, "N/2": n_fft // 2, "N": n_fft, "N+5": n_fft + 5}[hop_of]
    for total, counts in SPLITS.items():
        assert sum(counts) == total
        offsets, lens, need = rows_layout(counts, n_fft, hop)
        x = noise(need, total)
        for fmt in (S.SUMS, S.POWER):
            check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, total)


def test_more_tiles_than_workgroups(x3, ctx):
    """the transform's grid is capped at 4 096 workgroups of 32 rows (16 at n_fft 1 024), which then walk the tiles grid-stride:
    one row of samples at hop 1 gives more rows than one pass of the grid holds, so workgroups take a second tile -- the
    barrier in front of the LDS planes' and the row flags' reuse, the frames' sums formed anew.  n_fft 64: every word;
    n_fft 1 024 (66 001 rows of 513 words): the first and last 48 rows and every 89th, with the same ==."""
    n_fft, rows = 64, 4096 * 32 + 8 * 32 + 5
    x = noise(n_fft + rows - 1, 21)
    for fmt in (S.POWER, S.SUMS):
        got = check(x3, ctx, x, [0], [x.size], None, n_fft, 1, fmt, 0, rows)
        assert got[3][4] == rows
    n_fft, rows = 1024, 4096 * 16 + 29 * 16 + 1
    x = noise(n_fft + rows - 1, 22)
    got = run(x3, ctx, x, [0], [x.size], None, n_fft, 1, S.POWER, 0, rows)
    assert got[3] == (0, 0, 1, 0, rows) and got[1].tolist() == [0, rows] and got[2].tolist() == [0]
    pick = np.unique(np.concatenate([np.arange(48), np.arange(0, rows, 89), np.arange(rows - 48, rows)]))
    frames = x.astype(np.int64)[pick[:, None] + np.arange(n_fft)[None, :]]
    want = S.power_of(np.einsum("rn,nkc->rkc", frames, S.basis(n_fft)), n_fft)
    assert np.array_equal(got[0][pick], want)
    assert pick[pick >= 4096 * 16].size > 48                      # rows of the second pass among them


# ------------------------------------------------------------------------------------------------ 2. lengths
@pytest.mark.parametrize("n_fft, hop", [(64, 1), (64, 48), (256, 128), (512, 517), (1024, 1024)])
def test_lengths_around_a_frame_at_odd_offsets(x3, ctx, n_fft, hop):
    lens = [0, n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop, 0, 0]
    offsets, at = [], 1
    for ln in lens[:5]:
        offsets.append(at)
        at = (at + ln + 1) | 1              # every offset is odd: the rows are 2-byte aligned, no more
    offsets += [0, 0]                       # events' fillers: (0, 0), zero rows and status 0
    x = noise(at + 4, n_fft + hop)
    assert [S.n_rows(v, n_fft, hop) for v in lens] == [0, 0, 1, 1, 2, 0, 0] and all(o % 2 for o in offsets[:5])
    for fmt in (S.SUMS, S.POWER):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, 4)
        assert not got[2].any() and got[1].tolist() == [0, 0, 0, 1, 2, 4, 4, 4]
        check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 2, 14)


# ------------------------------------------------------------------------------------------------ 3. content
@pytest.mark.parametrize("n_fft", [64, 256, 1024])
@pytest.mark.parametrize("table", ["usual", "ones", "random"])
def test_content_at_the_byte_splits_edges(x3, ctx, n_fft, table):
    tab = {"usual": None, "ones": ones_table(), "random": random_table()}[table]
    ln = 2 * n_fft + 7
    rows = [np.full(ln, -32768), np.full(ln, 32767), np.resize(np.array(EDGE_VALUES), ln), np.resize(np.array(EDGE_VALUES[::-1]), ln)]
    x = np.concatenate(rows).astype(np.int16)
    offsets, lens = [i * ln for i in range(4)], [ln] * 4
    for hop in (n_fft, 7):
        cap = 4 * S.n_rows(ln, n_fft, hop)
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, S.SUMS, 0, cap, tab)
        check(x3, ctx, x, offsets, lens, None, n_fft, hop, S.POWER, 0, cap, tab)
        if table == "ones":   # re == the frame's sum of samples, im == 0
            fr = np.concatenate([S.frames_of(r.astype(np.int16), n_fft, hop) for r in rows])
            assert np.array_equal(got[0][:, :, 0], np.repeat(fr.sum(axis=1)[:, None], S.n_bins(n_fft), axis=1)) and not got[0][:, :, 1].any()


# ------------------------------------------------------------------------------------------------ 4. statuses and layouts
def _status_rows(n_fft, hop):
    counts = [3, 2, 0, 5, 1, 4]
    offsets, lens, need = rows_layout(counts, n_fft, hop)
    return counts, offsets, lens, noise(need + 8, 11)


@pytest.mark.parametrize("n_fft, hop", [(64, 48), (1024, 100)])
@pytest.mark.parametrize("fmt", [S.SUMS, S.POWER])
def test_statuses(x3, ctx, n_fft, hop, fmt):
    counts, offsets, lens, x = _status_rows(n_fft, hop)
    total = sum(counts)
    ins = [0, 14, 0, 21, 0, 0]
    for in_place in (False, True):      # the in-status comes out, its rows are zeros
        got = check(x3, ctx, x, offsets, lens, ins, n_fft, hop, fmt, 0, total, in_place=in_place)
        assert got[2].tolist() == ins and not got[0][3:5].any() and got[0][0:3].any()
        check(x3, ctx, x, offsets, lens, ins, n_fft, hop, fmt, 6, 36, in_place=in_place)
    # wild offsets and lengths against samples_cap: the status, rows of zeros, nothing read
    wild = list(offsets)
    wild[0], wild[3] = 2 ** 63 + 1, x.size - lens[3] + 1
    got = check(x3, ctx, x, wild, lens, None, n_fft, hop, fmt, 0, total)
    assert got[2].tolist() == [BAD, 0, 0, BAD, 0, 0]
    got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, total, samples_cap=offsets[4] + lens[4])
    assert got[2].tolist() == [0, 0, 0, 0, 0, BAD]
    # packed past rows_cap: nothing of the range is written, the total says what all need
    for cap in (total - 1, 7, 4, 1):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, cap)
        assert got[3][4] == total and got[2].tolist() == [BAD if a + r > cap else 0 for a, r in zip(np.cumsum([0] + counts), counts)]
    # padded: zeros behind R(w), R(w) > stride, no d_row_offsets
    for stride in (5, 4, 1):
        got = check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, stride, 6 * stride + 1, null_offsets=(stride == 4))
        assert got[2].tolist() == [BAD if r > stride else 0 for r in counts]


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_argument_refusals_enqueue_nothing(x3, ctx):
    n_fft, hop, fmt = 64, 32, S.SUMS
    counts, offsets, lens, x = _status_rows(n_fft, hop)
    n, total = len(lens), sum(counts)
    sizes = {"out": out_bytes(n_fft, fmt) * total, "ro": 8 * (n + 1), "st": 4 * n}
    d = {k: ctx.alloc(v + GUARD) for k, v in sizes.items()}
    d.update(x=ctx.alloc(2 * x.size), off=ctx.alloc(8 * n), ln=ctx.alloc(4 * n), tab=ctx.alloc(4 * S.PAIRS))
    try:
        ctx.upload(d["x"], x)
        ctx.upload(d["off"], np.array(offsets, dtype=np.uint64))
        ctx.upload(d["ln"], np.array(lens, dtype=np.uint32))
        ctx.upload(d["tab"], TL.table())

        def call(rule="ok", **kw):
            a = dict(d_samples=d["x"], samples_cap=x.size, d_offsets=d["off"], d_lens=d["ln"], d_in_status=None, n_ranges=n,
                     row_stride=0, d_out=d["out"], rows_cap=total, d_row_offsets=d["ro"], d_status=d["st"])
            a.update(kw)
            r = None if rule is None else x3.SpectraRule(n_fft, hop, fmt, 0, d["tab"])
            for k, v in ({} if rule in (None, "ok") else rule).items():
                setattr(r, k, v)
            return ctx.spectra_rows_dev(a["d_samples"], a["samples_cap"], a["d_offsets"], a["d_lens"], a["d_in_status"], a["n_ranges"],
                                        r, a["row_stride"], a["d_out"], a["rows_cap"], a["d_row_offsets"], a["d_status"])
        assert ctx.spectra_result()[0] == BAD                     # nothing pending yet
        assert call() == 0                                         # the earlier call, whose result stays to be served
        ctx.sync()
        want = {k: ctx.download(d[k], v + GUARD) for k, v in sizes.items()}
        for k, v in sizes.items():
            ctx.upload(d[k], np.full(v + GUARD, 0x5A, dtype=np.uint8))
        refused = [dict(rule=None)]
        refused += [dict(rule={"n_fft": v}) for v in (0, 32, 63, 65, 96, 2048, 1 << 31)]
        refused += [dict(rule={"hop": 0}), dict(rule={"hop": 1 << 31}), dict(rule={"format": 2}), dict(rule={"reserved": 1}),
                    dict(rule={"d_table": None}), dict(rule={"d_table": d["tab"] + 2})]
        refused += [dict(n_ranges=0), dict(n_ranges=1 << 31), dict(rows_cap=0), dict(rows_cap=1 << 31)]
        refused += [dict(**{k: None}) for k in ("d_samples", "d_offsets", "d_lens", "d_out", "d_status", "d_row_offsets")]
        refused += [dict(d_samples=d["x"] + 1), dict(d_lens=d["ln"] + 2), dict(d_in_status=d["st"] + 2), dict(d_status=d["st"] + 2),
                    dict(d_offsets=d["off"] + 4), dict(d_out=d["out"] + 4), dict(d_row_offsets=d["ro"] + 4)]
        refused += [dict(row_stride=total // n + 1, d_row_offsets=None)]            # n_ranges * row_stride > rows_cap
        # the rule's checks come first: a bad rule with another bad argument is still the rule's refusal (the same code)
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
        for k, v in sizes.items():
            assert (ctx.download(d[k], v + GUARD) == 0x5A).all(), "a refused call wrote to " + k
        res = ctx.spectra_result()                                 # the earlier call's result is still served
        assert res == (0, 0, n, 0, total), res
        assert ctx.spectra_result()[0] == BAD
        ref = S.spectra_rows(x, offsets, lens, None, n_fft, hop, fmt, 0, total)
        assert np.array_equal(want["out"][:sizes["out"]].view(np.int64).reshape(total, -1, 2), ref[0])
    finally:
        for q in d.values():
            ctx.free(q)


def test_other_calls_states_are_left_alone(x3, ctx):
    """a spectra call between a ranges call and its result: both results are served, each its own"""
    import test_gpu_range_levels as T
    dev = T.base(ctx, x3)
    d_st, d_ln, d_out, d_off, d_s = (dev.alloc(8 * 2), dev.alloc(4 * 2), dev.alloc(2 * 900), dev.alloc(8 * 3), dev.alloc(4 * 2))
    try:
        ctx.upload(d_st, np.array([10, 401], dtype=np.uint64))
        ctx.upload(d_ln, np.array([300, 600], dtype=np.uint32))
        assert ctx.decode_ranges_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_st, d_ln, 2, 0, d_out, 900,
                                     x3.WINDOW_I16, d_off, d_s, dev.d_seg, dev.sb) == 0
        x = noise(300)
        check(x3, ctx, x, [1], [299], None, 64, 16, S.POWER, 0, S.n_rows(299, 64, 16))
        assert ctx.decode_ranges_result()[:2] == (0, 0)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 6. behind a stalled stream
class StalledSpectra(AC.Case):
    """samples, offsets, lengths, in-statuses and the table arrive on the stream behind a stall; a decoy lies there when the
    host enqueues the call, and the rule struct is overwritten behind it"""
    name = "spectra"
    N, HOP, CAP = 128, 40, 40

    def content(self, which):
        rng = np.random.default_rng({"A": 1, "B": 2}[which])
        counts = [3, 0, 9, 6] if which == "A" else [7, 2, 5, 11]
        offsets, lens, need = rows_layout(counts, self.N, self.HOP, first=3 if which == "A" else 1)
        x = rng.integers(-32768, 32768, 4096).astype(np.int16)
        assert need <= x.size
        ins = [0, 0, 0, 0] if which == "A" else [0, 13, 0, 0]
        tab = TL.table() if which == "A" else random_table(9)
        return x, offsets, lens, ins, tab

    def inputs(self, which):
        x, offsets, lens, ins, tab = self.content(which)
        return {"x": x, "off": np.array(offsets, dtype=np.uint64), "ln": np.array(lens, dtype=np.uint32),
                "in": np.array(ins if which == "B" else [1, 1, 1, 1], dtype=np.int32), "tab": tab}

    def outputs(self):
        return {"out": 4 * S.n_bins(self.N) * self.CAP, "ro": 8 * 5, "st": 4 * 4}

    def enqueue(self, x3, ctx, d, which, probe):
        rule = x3.SpectraRule(self.N, self.HOP, S.POWER, 0, d["tab"])
        rc = ctx.spectra_rows_dev(d["x"], 4096, d["off"], d["ln"], d["in"] if which == "B" else None, 4, rule, 0, d["out"], self.CAP,
                                  d["ro"], d["st"])
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"spectra": ctx.spectra_result()}

    def expect(self, which):
        x, offsets, lens, ins, tab = self.content(which)
        out, off, st, total = S.spectra_rows(x, offsets, lens, ins, self.N, self.HOP, S.POWER, 0, self.CAP, tab)
        bad = np.flatnonzero(st)
        res = (0, bad.size, int(bad[0]) if bad.size else 4, int(st[bad[0]]) if bad.size else 0, total)
        return {"out": {"out": [(0, out[:total], False)], "ro": [(0, off, False)], "st": [(0, st, False)]}, "result": {"spectra": res}}


def test_behind_a_stalled_stream(x3):
    import torch
    case = StalledSpectra()
    AC.check_pair_differs(case)
    AC.run_stalled(x3, torch, case, AC.calibrate_sleep(torch))


# ------------------------------------------------------------------------------------------------ 7. end to end
def _base_ranges():
    """ranges of the base stream, several with frames at multiples of N = 64 of the stream"""
    return [0, 384, 403, 64 * 7, 1210, 2000, 128], [400, 513, 131, 640, 300, 137, 63]   # (packed rows at odd and even offsets)


def _reference_rows(samples_of, starts, lens, status, n_fft, hop, power):
    rows = []
    for w, (s, ln) in enumerate(zip(starts, lens)):
        r = S.n_rows(ln, n_fft, hop)
        full = S.sums(samples_of(w)[s:s + ln], n_fft, hop) if status[w] == 0 else np.zeros((r, S.n_bins(n_fft), 2), dtype=np.int64)
        rows.append(S.power_of(full, n_fft).astype(np.int64) if power else full)
    return np.concatenate(rows)


def _stream(x3, n=2137, seed=1616, hurt=None):
    """n samples in frames of 400 from the oracle's encoder -> (samples, stream bytes, x3 params); hurt: the frame whose
    payload CRC fails"""
    import oracle_lib as O
    import ranges_ref as RR
    wav = x3.synth(2, seed, 0, n)
    rc, s, _ = O.encode(wav, O.Params.make(20, 20))
    assert rc == 0
    if hurt is not None:
        s = s.copy()
        s[RR.frame_offsets(s)[hurt] + 20 + 30] ^= 0x08
    return wav, s, x3.Params.make(block_len=20, blocks_per_frame=20)


def test_window_source_range_spectra_over_a_damaged_frame(x3, ctx):
    import torch
    import ranges_ref as RR
    wav, s, p = _stream(x3, hurt=2)                         # frame 2 (positions 800 .. 1199): its payload CRC fails
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        starts, lens = _base_ranges()
        rows = [S.n_rows(v, 64, 48) for v in lens]
        covers = [a < 1200 and a + ln > 800 for a, ln in zip(starts, lens)]
        assert any(covers) and not all(covers)
        for power in (True, False):
            for kw in ({}, {"padded_to": 14}):
                sp, ro, st, smp, so = src.range_spectra(starts, lens, 64, 48, power=power, **kw)
                st = st.cpu().numpy()
                assert st.tolist() == [RR.ERR_PAYLOAD_CRC if c else 0 for c in covers]
                want = _reference_rows(lambda w: wav, starts, lens, st, 64, 48, power)
                got = sp.cpu().numpy().astype(np.int64)
                if kw:
                    assert got.shape[0] == 14 * len(lens) and np.array_equal(ro.cpu().numpy(), 14 * np.arange(len(lens) + 1))
                    a = 0
                    for w, r in enumerate(rows):
                        assert np.array_equal(got[14 * w:14 * w + r], want[a:a + r]) and not got[14 * w + r:14 * (w + 1)].any()
                        a += r
                else:
                    assert np.array_equal(ro.cpu().numpy(), np.concatenate([[0], np.cumsum(rows)])) and np.array_equal(got, want)
                assert sp.dtype == (torch.int32 if power else torch.int64) and sp.is_cuda
                so = so.cpu().numpy()
                assert np.array_equal(so, np.concatenate([[0], np.cumsum(lens)]))
                for w in np.flatnonzero(st == 0):      # the caller gets the cut samples for free
                    a = int(so[w])
                    assert np.array_equal(smp[a:a + lens[w]].cpu().numpy(), wav[starts[w]:starts[w] + lens[w]])
        sp, ro, st, _, _ = src.range_spectra(starts, lens, 64, 48, capacity=rows[0] + rows[1])   # no room behind two ranges
        assert st.cpu().numpy().tolist()[:3] == [0, RR.ERR_PAYLOAD_CRC, BAD] and sp.shape[0] == rows[0] + rows[1] and int(ro[-1]) == sum(rows)
    finally:
        src.close()


@pytest.mark.parametrize("n_fft", [64, 128, 1024])
def test_tile_edges_on_rows_a_ranges_call_packed(x3, ctx, n_fft):
    """case 1's row counts on rows as x3_decode_ranges_dev lays them: ranges of the oracle-encoded stream with odd lengths,
    so the packed rows begin at odd and at even sample offsets, and the spectra call takes the ranges call's own offsets
    and statuses"""
    wav, s, p = _stream(x3)
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        for hop in (1, 48):
            for total, counts in SPLITS.items():
                _, lens, _ = rows_layout(counts, n_fft, hop)
                counts, lens = [0] + counts, [1] + lens            # (one sample in front: the next row begins at an odd offset)
                starts = [(37 * (w + 1) + 5 * total) % (wav.size - ln) for w, ln in enumerate(lens)]
                for power in (True, False):
                    sp, ro, st, smp, so = src.range_spectra(starts, lens, n_fft, hop, power=power)
                    so = so.cpu().numpy()
                    assert not st.cpu().numpy().any() and sp.shape[0] == total and any(int(v) % 2 for v in so[:-1])
                    assert np.array_equal(ro.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
                    want = _reference_rows(lambda w: wav, starts, lens, [0] * len(lens), n_fft, hop, power)
                    assert np.array_equal(sp.cpu().numpy().astype(np.int64), want), (n_fft, hop, total, power)
    finally:
        src.close()


def test_aligned_frames_equal_the_tone_bank_range_levels(x3, ctx):
    """frames at multiples of N of the stream: eight chosen bins == the planes of tone_bank_range_levels, and with band=True
    the POWER words == sum_sq // n"""
    wav, s, p = _stream(x3)
    src = x3.WindowSource(ctx, s, p, seg_blocks=4, index="walk")
    try:
        for n_fft in (64, 256):
            starts = [0, 3 * n_fft, 5 * n_fft]
            lens = [2 * n_fft, n_fft, 3 * n_fft]
            bins = [0, 1, 2, 5, n_fft // 4, n_fft // 2 - 1, n_fft // 2, 7]
            tones = tuple(x3.Tone(k * (2 ** 32 // n_fft)) for k in bins)
            sums = src.range_spectra(starts, lens, n_fft, power=False)[0].cpu().numpy()
            pw = src.range_spectra(starts, lens, n_fft, power=True)[0].cpu().numpy()
            lv, ro, st = src.tone_bank_range_levels(starts, lens, n_fft, tones)
            band = src.tone_bank_range_levels(starts, lens, n_fft, tones, band=True)[0]
            assert not st.cpu().numpy().any() and sums.shape[0] == 6
            for t, k in enumerate(bins):
                rec = lv[t].cpu().numpy().view(x3.TONE_DTYPE).reshape(-1)
                assert np.array_equal(sums[:, k, 0], rec["re"]) and np.array_equal(sums[:, k, 1], rec["im"]) and (rec["n"] == n_fft).all()
                lev = band[t].cpu().numpy().view(x3.LEVEL_DTYPE).reshape(-1)
                assert np.array_equal(pw[:, k].astype(np.uint64), lev["sum_sq"] // lev["n"])
    finally:
        src.close()


def test_corpus_range_spectra_on_two_entries(x3, ctx):
    (w0, s0, p), (w1, s1, _) = _stream(x3, 1500, 77), _stream(x3, 1000, 78)
    buf = np.concatenate([s0, np.zeros(2, dtype=np.uint8), s1, np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf, [0, s0.size + 2], [s0.size, s1.size], params=p, seg_blocks=4, index="walk")
    try:
        wavs = [w0, w1]
        entries, starts, lens = [0, 1, 0, 1], [0, 100, 333, 500], [400, 500, 128, 127]
        sp, ro, st, smp, so = corpus.range_spectra(entries, starts, lens, 128, 64, power=False)
        assert not st.cpu().numpy().any()
        want = np.concatenate([S.sums(wavs[e][a:a + ln], 128, 64) for e, a, ln in zip(entries, starts, lens)])
        assert np.array_equal(sp.cpu().numpy(), want)
        pw = corpus.range_spectra(entries, starts, lens, 128, 64)[0]
        assert np.array_equal(pw.cpu().numpy().view(np.uint32), S.power_of(want, 128))
    finally:
        corpus.close()


# ------------------------------------------------------------------------------------------------ 8. the example
def test_the_example_the_loudest_bins_of_the_two_bursts(x3, ctx):
    """DESIGN.md section 28's signal and its four plane events (min_planes 1), padded, n_fft = 256: the event (8 000, 400)
    holds the 0.0817 fs burst and then the 0.2310 fs burst, and at hop 144 it has two frames, one mostly inside each.  Their
    loudest bins are 21 (0.0817 * 256 = 20.9) and 59 (0.2310 * 256 = 59.1), by the reference on the CPU and by the call;
    the three events of 200 samples hold no whole frame of 256: rows of zeros."""
    import oracle_lib as O
    import plane_events_ref as P
    w = P.example()
    starts, lens = [4_400, 8_000, 12_000, 16_000], [200, 400, 200, 200]
    want = [S.power(w[a:a + ln], 256, 144) for a, ln in zip(starts, lens)]
    assert [v.shape[0] for v in want] == [0, 2, 0, 0] and [int(r.argmax()) for r in want[1]] == [21, 59]
    rc, stream, _ = O.encode(w, O.Params.make(20, 100, (0, 1, 3)))
    assert rc == 0
    ws = x3.WindowSource(ctx, stream, x3.Params.make(20, 100), seg_blocks=8)
    try:
        sp, ro, st, _, _ = ws.range_spectra(starts, lens, 256, 144, padded_to=2)
        got = sp.cpu().numpy().view(np.uint32)
        assert not st.cpu().numpy().any() and got.shape == (8, 129) and ro.cpu().numpy().tolist() == [0, 2, 4, 6, 8]
        assert np.array_equal(got[2:4], want[1]) and not got[:2].any() and not got[4:].any()
        assert got[2].argmax() == 21 and got[3].argmax() == 59
    finally:
        ws.close()


# ------------------------------------------------------------------------------------------------ 9. under guard pages
def fence_run(x3):
    """the body of the child of test_under_guard_pages: cases 1 and 4 with buffers of exactly their bytes (X3HIP_FENCE_TIGHT
    ends every mapping at the buffer's last byte, the library's workspace included), each group on a Context of its own
    -> the calls made"""
    calls = 0
    for n_fft, hop in ((64, 1), (128, 48), (1024, 1029)):
        ctx = x3.Context(0)
        try:
            for total, counts in SPLITS.items():
                offsets, lens, need = rows_layout(counts, n_fft, hop)
                x = noise(need, total)
                for fmt in (S.SUMS, S.POWER):
                    check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, total, tight=True)
                    calls += 1
        finally:
            ctx.close()
    for n_fft, hop in ((64, 48), (1024, 100)):
        ctx = x3.Context(0)
        try:
            counts, offsets, lens, x = _status_rows(n_fft, hop)
            x = x[:offsets[-1] + lens[-1]]                     # the last row ends the samples' mapping
            total = sum(counts)
            for fmt in (S.SUMS, S.POWER):
                check(x3, ctx, x, offsets, lens, [0, 14, 0, 21, 0, 0], n_fft, hop, fmt, 0, total, in_place=True, tight=True)
                wild = list(offsets)
                wild[0], wild[3] = 2 ** 63 + 1, x.size - lens[3] + 1
                check(x3, ctx, x, wild, lens, None, n_fft, hop, fmt, 0, total, tight=True)
                check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 0, 7, tight=True)
                check(x3, ctx, x, offsets, lens, None, n_fft, hop, fmt, 4, 24, null_offsets=True, tight=True)
                calls += 4
        finally:
            ctx.close()
    return calls


def test_under_guard_pages():
    """one child process under X3HIP_FENCE=16 X3HIP_FENCE_FILL=165 X3HIP_FENCE_TIGHT=1, started as
    test_gpu_fence_analysis.py starts its children: cases 1 and 4 with exact-fit buffers, then 150 trials of the fuzz family
    (y) of tools/fuzz_parity.py in three runs of 50, each on a Context of its own"""
    import test_gpu_fence_analysis as FA
    out = FA._child("""
        import x3hip, test_gpu_spectra as TS
        print("calls", TS.fence_run(x3hip), flush=True)
        import fuzz_parity as FZ
        total = 0
        for seed in (11, 12, 13):
            c = FZ.run(seed=seed, trials=50, families="y", context=None)
            assert sum(c.values()) == c["y"]
            total += c["y"]
        print("trials", total)
        """, timeout=240)
    assert int(out.split("calls")[1].split()[0]) == 3 * 4 * 2 + 2 * 2 * 4 and int(out.split("trials")[1]) == 150
