#!/usr/bin/env python3
"""Range levels (x3_range_levels_dev / x3_corpus_range_levels_dev) against the two routes a caller has without them, in one
process, the routes alternating rep by rep; medians of --reps, host time from the first call to the last synchronised result.
  route a   the ranges call into a sample buffer, then the five reductions in torch (min, max, sum and sum of squares in
            int64 over an int32 copy; the count is known)
  route b   the full levels call at that bin length (every frame of the stream, every entry of the corpus)
on
  config3   the stream kbench.py makes (691.2 M hydrophone samples at 192 kHz, block length 20, the encoder's index)
  corpus_a  tools/corpus_bench.py's corpus (a): 4 000 clips of 10-15 s at 44.1 kHz
Cases:
  1  1 024 ranges of 0.25-4 s at 1 ms bins (192 / 44 positions); starts and lengths are whole bins, so that route a's
     packed samples reshape to [rows, bin] and route b's records are the same bins
  2  one 10 s range at 2 000 bins
  3  the events of tools/events_bench.py (levels at 10 ms, its rule, --cap slots with fillers) at bin_len 0: one record an
     event; route a masks the tails of its padded rows, route b is the levels call plus the events call's own merged records
--signal diff: the same cases on the first difference (x3_signal_range_levels_dev / x3_corpus_signal_range_levels_dev with
X3_LEVEL_SIGNAL_DIFF).  Route a decodes every range with the sample in front of it (start - 1, len + 1; a range at its
entry's position 0 has none and its first position counts nothing), takes torch's difference, clamps it to 16 bits and
reduces; the index plan that drops each range's leading sample is made once, outside the timed part.  Route b is the DIFF
levels call, and case 3's events are found on the DIFF levels.
--signal fir [--taps 1,-2,1 --shift 0]: the same cases behind an integer FIR filter (x3_fir_range_levels_dev /
x3_corpus_fir_range_levels_dev).  Route a decodes every range with the T - 1 samples in front of it (fewer at its entry's
start, where the first positions count nothing), runs torch's conv1d in float64 over the packed buffer (exact: the sums stay
inside 2^30), shifts, clamps and reduces; case 3 sums T gathers of its padded rows instead.  Route b is the FIR levels call,
and case 3's events are found on the FIR levels.
--signal tone [--step 350898828]: the same cases against one oscillator (x3_tone_range_levels_dev /
x3_corpus_tone_range_levels_dev with the usual table), records x3_tone_level.  Route a decodes the ranges as they are and
forms, in torch's int64, every position's phase ((position in the stream or entry) * step mod 2^32 -- the positions are
made once, outside the timed part), gathers the table pair, multiplies and sums, with min and max of the samples.  Route b is
the tone levels call; case 3's events are found on the band's levels (the tone levels call and the adapter in place), and
its merged band records are no tone records, so case 3 compares the call with route a only.
--signal tone --tones K (2 .. 8): the tone bank call beside them (x3_tone_bank_range_levels_dev /
x3_corpus_tone_bank_range_levels_dev), K oscillators at BANK_FREQS[:K] (the first is --step's default):
  bank            one bank call of K tones, K planes of records
  singles         K single tone-range calls of the same build, one per plane
  range_levels    one single tone-range call (the first tone), as without --tones
  route_a         the ranges call once, then the torch reduction above once per tone
`bank` and `singles` alternate in order rep by rep.  The planes of `bank` are compared with == against `singles` (bytes) and
against route a (every plane).
Every route's records are compared with == at the end of every case and the tool fails otherwise.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/range_levels_bench.py ...`.  Prints one JSON line.
    python3 tools/range_levels_bench.py [--signal samples|diff|fir|tone] [--taps c0,c1,..] [--shift k] [--step s] [--tones K] [--samples N] [--reps 10] [--warmup 2] [--cap 4096]
                                        [--cases config3,corpus] [--no-route-a] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip

now = time.perf_counter
JOIN, MIN_BINS, PAD, MAX_BINS = 5, 1, 2, 25      # tools/events_bench.py's rule
BANK_FREQS = (0.0817, 0.2310, 0.15, 0.41, 0.02, 0.33, 0.275, 0.4999)   # --tones K: the first K, in units of fs (tone_levels_bench.py's)


class Source:
    """what a case needs of a stream or a corpus: the three calls, the entries' sample counts and their rows of a levels call"""

    def __init__(self, ctx, name, rate, n_samples, range_levels, ranges, levels, events, levels_rows, tone_call=None, bank_call=None):
        self.ctx, self.name, self.rate, self.n_samples = ctx, name, rate, n_samples
        self.tone_call, self.bank_call = tone_call, bank_call      # (--tones: range_levels' arguments and a Tone / the bank behind them)
        self.band = lambda d_lv, rows: ctx.tone_power_levels_dev(d_lv, rows, d_lv)      # (--signal tone: records -> band levels)
        self.range_levels, self.ranges, self.levels, self.events, self.levels_rows = range_levels, ranges, levels, events, levels_rows


def records(t):
    return t.cpu().numpy().view(x3hip.LEVEL_DTYPE).reshape(-1)


def as_records(mn, mx, sm, sq, n):
    out = np.zeros(len(n), dtype=x3hip.LEVEL_DTYPE)
    out["min"], out["max"], out["sum"], out["sum_sq"], out["n"] = mn, mx, sm, sq, n
    return out


def tone_records(re, im, mn, mx, n):
    out = np.zeros(len(n), dtype=x3hip.TONE_DTYPE)
    out["re"], out["im"], out["min"], out["max"], out["n"] = re, im, mn, mx, n
    out["min"][out["n"] == 0], out["max"][out["n"] == 0] = 32767, -32768
    return out


def tone_pairs(a, pos, step=None):
    """route a, tone: (cos, sin) int64 of the positions pos (int64, in the stream or entry)"""
    k = ((pos * (a.step if step is None else step)) & 0xFFFFFFFF) >> 22          # (pos < 2^31, step < 2^32: the product stays inside int64)
    return a.table[k, 0], a.table[k, 1]


def bank_sides(src, a, results, name, rep, args, rows, blv, slv, expect):
    """--tones: the bank call and the K single calls, timed in alternating order; args: the call's arguments in front of
    d_levels, (d_off, d_st) behind rows_cap"""
    ctx, (front, back) = src.ctx, args

    def bank():
        assert src.bank_call(*front, blv.data_ptr(), rows, *back) == 0, ctx.last_error()
        r = ctx.range_levels_result()
        assert r == expect, r

    def singles():
        for k, tone in enumerate(a.tones):
            assert src.tone_call(*front, slv.data_ptr() + 32 * rows * k, rows, *back, tone) == 0, ctx.last_error()
            r = ctx.range_levels_result()
            assert r == expect, r
    sides = [("bank", bank), ("singles", singles)]
    for side, fn in (sides if rep % 2 == 0 else sides[::-1]):
        t = now()
        fn()
        timed(results, name + "_" + side, rep, a.warmup, now() - t)


def bank_equal(a, blv, slv, reds, counts):
    """--tones: the bank's planes == the single calls' bytes and, where route a ran, == its records plane by plane"""
    same = bool(torch.equal(blv, slv))
    for k, red in enumerate(reds or []):
        want = tone_records(*(t.cpu().numpy() for t in red[:4]), counts)
        same = same and blv[k].cpu().numpy().tobytes() == want.tobytes()
    return same


def filtered(a, w):
    """route a's signal over a packed int32 buffer w: y[i] belongs to buffer index i + a.hist"""
    if a.signal == "diff":
        return torch.clamp(w[1:] - w[:-1], -32768, 32767)
    k = torch.tensor(a.taps[::-1], dtype=torch.float64, device="cuda")[None, None, :]      # (conv1d correlates: the taps reversed)
    acc = torch.nn.functional.conv1d(w.to(torch.float64)[None, None, :], k)[0, 0].to(torch.int64)
    return torch.clamp(acc >> a.shift, -32768, 32767)


def timed(results, key, rep, warmup, t):
    if rep >= warmup:
        results.setdefault(key, []).append(t * 1e3)


def bins_case(src, a, results, info, case, ent, starts, lens, bin_len):
    """cases 1 and 2: starts and lengths in whole bins, packed"""
    ctx, n = src.ctx, len(starts)
    name = "%s_case%d" % (src.name, case)
    rows = [v // bin_len for v in lens]
    total_rows, total = sum(rows), sum(lens)
    d_ent = torch.tensor(ent, dtype=torch.int32, device="cuda")
    d_st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    lv = torch.empty((total_rows, 32), dtype=torch.uint8, device="cuda")
    off, off2 = (torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    st, st2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    hist_on, hist = a.hist > 0, a.hist
    pre = [min(hist, s) for s in starts]          # route a, diff / fir: the samples in front of the range come with it
    total_a = total + sum(pre)
    buf = torch.empty(total_a, dtype=torch.int16, device="cuda")
    d_st_a = torch.tensor([s - k for s, k in zip(starts, pre)], dtype=torch.int64, device="cuda")
    d_ln_a = torch.tensor([v + k for v, k in zip(lens, pre)], dtype=torch.int32, device="cuda")
    if hist_on:   # where each range's own positions lie in route a's packed buffer; a range at position 0 has no first difference
        first = np.concatenate([[0], np.cumsum([v + k for v, k in zip(lens, pre)])[:-1]]) + np.array(pre)
        keep = torch.from_numpy(np.concatenate([f + np.arange(v) for f, v in zip(first, lens)]).astype(np.int64)).cuda()
        ok = np.ones(total, dtype=bool)
        for f, v, k in zip(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, pre):   # the positions without their history
            ok[f:f + min(hist - k, v)] = False
        valid = torch.from_numpy(ok).cuda().view(total_rows, bin_len)
    if a.tone:    # every sample's position in its stream or entry, in route a's packed order
        pos = torch.from_numpy(np.concatenate([s + np.arange(v, dtype=np.int64) for s, v in zip(starts, lens)])).cuda()
    rf = src.levels_rows(bin_len)
    full_rows = int(rf[-1])
    full = torch.empty((full_rows, 32), dtype=torch.uint8, device="cuda") if 64 * full_rows < a.levels_bytes else None
    if a.tones:
        blv, slv = (torch.empty((len(a.tones), total_rows, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    red = reds = None
    for rep in range(a.warmup + a.reps):
        if a.tones:
            bank_sides(src, a, results, name, rep, ((d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, bin_len, 0),
                                                    (off.data_ptr(), st.data_ptr())), total_rows, blv, slv, (0, 0, n, 0, total_rows))
        t0 = now()
        assert src.range_levels(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, bin_len, 0, lv.data_ptr(), total_rows,
                                off.data_ptr(), st.data_ptr()) == 0, ctx.last_error()
        r = ctx.range_levels_result()
        t1 = now()
        assert r == (0, 0, n, 0, total_rows), r
        if a.no_route_a:
            timed(results, name + "_range_levels", rep, a.warmup, t1 - t0)
            continue
        assert src.ranges(d_ent.data_ptr(), d_st_a.data_ptr(), d_ln_a.data_ptr(), n, 0, buf.data_ptr(), total_a, off2.data_ptr(),
                          st2.data_ptr()) == 0, ctx.last_error()
        r = ctx.decode_ranges_result()
        t2 = now()
        assert r[:2] == (0, 0), r
        if hist_on:
            w = buf.to(torch.int32)
            y = filtered(a, w)[(keep - hist).clamp(min=0)].view(total_rows, bin_len)
            red = (torch.where(valid, y, 32767).min(1).values, torch.where(valid, y, -32768).max(1).values,
                   torch.where(valid, y, 0).sum(1, dtype=torch.int64), torch.where(valid, y * y, 0).sum(1, dtype=torch.int64),
                   valid.sum(1))
        elif a.tone:
            x = buf.view(total_rows, bin_len)
            w = buf.to(torch.int64)
            reds = []
            for tone in a.tones or (a.tone,):
                cs, sn = tone_pairs(a, pos, tone.step)
                reds.append(((w * cs).view(total_rows, bin_len).sum(1), (w * sn).view(total_rows, bin_len).sum(1), x.min(1).values,
                             x.max(1).values))
            red = reds[0]
        else:
            x = buf.view(total_rows, bin_len)
            w = x.to(torch.int32)
            red = (x.min(1).values, x.max(1).values, w.sum(1, dtype=torch.int64), (w * w).sum(1, dtype=torch.int64))
        torch.cuda.synchronize()
        t3 = now()
        timed(results, name + "_range_levels", rep, a.warmup, t1 - t0)
        timed(results, name + "_route_a", rep, a.warmup, t3 - t1)
        timed(results, name + "_route_a_ranges", rep, a.warmup, t2 - t1)
        timed(results, name + "_route_a_torch", rep, a.warmup, t3 - t2)
        if full is not None:
            t4 = now()
            assert src.levels(bin_len, full.data_ptr(), full_rows) == 0, ctx.last_error()
            assert ctx.levels_result()[0] == 0
            timed(results, name + "_route_b", rep, a.warmup, now() - t4)
    got = records(lv)
    same = not st.cpu().numpy().any()
    if red is not None:
        counts = red[4].cpu().numpy().astype(np.uint32) if hist_on else np.full(total_rows, bin_len, dtype=np.uint32)
        want_a = (tone_records if a.tone else as_records)(*(t.cpu().numpy() for t in red[:4]), counts)
        same = same and got.tobytes() == want_a.tobytes()
    if a.tones:
        same = same and bank_equal(a, blv, slv, reds, counts if reds else None) and blv[0].cpu().numpy().tobytes() == got.tobytes()
    if full is not None and red is not None:
        frec = records(full)
        pick = np.concatenate([int(rf[e]) + s // bin_len + np.arange(k) for e, s, k in zip(ent, starts, rows)])
        same = same and np.array_equal(got, frec[pick])
    if not same:
        raise SystemExit("%s: the routes' records differ" % name)
    info[name] = {"signal": a.signal, "ranges": n, "bin_len": bin_len, "rows": total_rows, "samples": total, "levels_rows": full_rows,
                  "route_b": full is not None and red is not None, "equal": bool(same),
                  "replays": ctx.get_option("last_range_levels_replays"), "overflow": ctx.get_option("last_range_levels_overflow")}


def events_case(src, a, results, info, bin_len):
    """case 3: the slots of an events call, fillers included, at bin_len 0"""
    ctx, cap, name = src.ctx, a.cap, src.name + "_case3"
    stride = MAX_BINS * bin_len
    rf = src.levels_rows(bin_len)
    n_rows = int(rf[-1])
    full = torch.empty((n_rows, 32), dtype=torch.uint8, device="cuda")
    ent, st, ln = (torch.empty(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    ent.zero_()
    cnt = torch.zeros((), dtype=torch.int64, device="cuda")
    ev_lv, ev_lv2, lv = (torch.empty((cap, 32), dtype=torch.uint8, device="cuda") for _ in range(3))
    status, status2 = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    off = torch.empty(cap + 1, dtype=torch.int64, device="cuda")
    hist_on, hist = a.hist > 0, a.hist
    width = stride + hist                        # route a, diff / fir: columns for the samples in front of the range
    buf = torch.empty((cap, width), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert src.levels(bin_len, full.data_ptr(), n_rows) == 0 and (not a.tone or src.band(full.data_ptr(), n_rows) == 0)
    assert ctx.levels_result()[0] == 0
    ctx.sync()
    rec = records(full)
    q = 100.0 * (1.0 - min(0.002, cap / (4.0 * n_rows)))
    peak_min = int(min(max(np.percentile(np.maximum(rec["max"], -rec["min"])[rec["n"] != 0], q) + 1, 1), 32768))
    rule = x3hip.EventRule.make(0, peak_min, JOIN, MIN_BINS, PAD, MAX_BINS)
    assert src.events(full.data_ptr(), n_rows, bin_len, rule, ent.data_ptr(), st.data_ptr(), ln.data_ptr(), ev_lv.data_ptr(), cap,
                      cnt.data_ptr()) == 0
    rc, found = ctx.events_result()
    assert rc == 0 and found > 0 and (found <= cap or hist_on or a.tone), (rc, found)   # (diff: peaks saturate, ties at the
    # threshold can make more events than slots; the slots then hold the first `cap` of them and no filler)
    col = torch.arange(stride, device="cuda")[None, :]
    red = reds = None
    if a.tones:
        blv, slv = (torch.empty((len(a.tones), cap, 32), dtype=torch.uint8, device="cuda") for _ in range(2))
    for rep in range(a.warmup + a.reps):
        if a.tones:
            bank_sides(src, a, results, name, rep, ((ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, 0, 0),
                                                    (off.data_ptr(), status.data_ptr())), cap, blv, slv, (0, 0, cap, 0, cap))
        t0 = now()
        assert src.range_levels(ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, 0, 0, lv.data_ptr(), cap, off.data_ptr(),
                                status.data_ptr()) == 0, ctx.last_error()
        r = ctx.range_levels_result()
        t1 = now()
        assert r == (0, 0, cap, 0, cap), r
        if a.no_route_a:
            timed(results, name + "_range_levels", rep, a.warmup, t1 - t0)
            continue
        if hist_on:   # (start - 1, len + 1) where there is a sample in front; position r of the range is column r + pre
            pre = torch.where(ln > 0, st.clamp(max=hist), 0)
            st_a, ln_a = st - pre, ln + pre.to(torch.int32)
            torch.cuda.synchronize()
        else:
            st_a, ln_a = st, ln
        assert src.ranges(ent.data_ptr(), st_a.data_ptr(), ln_a.data_ptr(), cap, width, buf.data_ptr(), cap * width, None,
                          status2.data_ptr()) == 0, ctx.last_error()
        r = ctx.decode_ranges_result()
        t2 = now()
        assert r[:2] == (0, 0), r
        mask = col < ln[:, None]
        w = buf.to(torch.int32)
        if hist_on:
            at = col + pre[:, None]
            if a.signal == "diff":
                y = torch.clamp(w.gather(1, at) - w.gather(1, (at - 1).clamp(min=0)), -32768, 32767)
            else:
                acc = sum(c * w.gather(1, (at - t).clamp(min=0)).to(torch.int64) for t, c in enumerate(a.taps))
                y = torch.clamp(acc >> a.shift, -32768, 32767).to(torch.int32)
            mask = mask & (col + pre[:, None] >= hist)
            red = (torch.where(mask, y, 32767).min(1).values, torch.where(mask, y, -32768).max(1).values,
                   torch.where(mask, y, 0).sum(1, dtype=torch.int64), torch.where(mask, y * y, 0).sum(1, dtype=torch.int64),
                   mask.sum(1))
        elif a.tone:   # (the rows behind a range's length hold zeros: they add nothing)
            w64 = w.to(torch.int64)
            reds = []
            for tone in a.tones or (a.tone,):
                cs, sn = tone_pairs(a, st[:, None] + col, tone.step)
                reds.append(((w64 * cs).sum(1), (w64 * sn).sum(1), torch.where(mask, w, 32767).min(1).values,
                             torch.where(mask, w, -32768).max(1).values))
            red = reds[0]
        else:
            red = (torch.where(mask, w, 32767).min(1).values, torch.where(mask, w, -32768).max(1).values,
                   w.sum(1, dtype=torch.int64), (w * w).sum(1, dtype=torch.int64))
        torch.cuda.synchronize()
        t3 = now()
        assert src.levels(bin_len, full.data_ptr(), n_rows) == 0 and (not a.tone or src.band(full.data_ptr(), n_rows) == 0)
        assert src.events(full.data_ptr(), n_rows, bin_len, rule, ent.data_ptr(), st.data_ptr(), ln.data_ptr(), ev_lv2.data_ptr(),
                          cap, cnt.data_ptr()) == 0
        assert ctx.events_result()[0] == 0 and ctx.levels_result()[0] == 0
        t4 = now()
        timed(results, name + "_range_levels", rep, a.warmup, t1 - t0)
        timed(results, name + "_route_a", rep, a.warmup, t3 - t1)
        timed(results, name + "_route_a_ranges", rep, a.warmup, t2 - t1)
        timed(results, name + "_route_a_torch", rep, a.warmup, t3 - t2)
        timed(results, name + "_route_b", rep, a.warmup, t4 - t3)
    got = records(lv)
    same = not status.cpu().numpy().any()
    if red is not None:
        counts = red[4].cpu().numpy().astype(np.uint32) if hist_on else ln.cpu().numpy().view(np.uint32)
        want_a = (tone_records if a.tone else as_records)(*(t.cpu().numpy() for t in red[:4]), counts)
        same = same and got.tobytes() == want_a.tobytes()
        if a.tone:     # (the events' merged records are band records; both passes found the same events)
            same = same and np.array_equal(records(ev_lv), records(ev_lv2))
        else:
            same = same and np.array_equal(got, records(ev_lv)) and np.array_equal(got, records(ev_lv2))
    if a.tones:
        same = same and bank_equal(a, blv, slv, reds, counts if reds else None) and blv[0].cpu().numpy().tobytes() == got.tobytes()
    if not same:
        raise SystemExit("%s: the routes' records differ" % name)
    info[name] = {"signal": a.signal, "ranges": cap, "events": int(found), "bin_len": 0, "events_bin_len": bin_len, "peak_min": peak_min,
                  "samples": int(ln.sum().item()), "equal": bool(same),
                  "replays": ctx.get_option("last_range_levels_replays"), "overflow": ctx.get_option("last_range_levels_overflow")}


def cases(src, a, results, info):
    rng = np.random.default_rng(11)
    ms = src.rate // 1000                    # 1 ms in whole positions: 192, 44
    ns = src.n_samples
    ent, starts, lens = [], [], []
    for _ in range(1024):
        e = int(rng.integers(0, len(ns)))
        k = int(rng.integers(250, 4001))     # 0.25 - 4 s in bins of 1 ms
        k = min(k, ns[e] // ms)
        ent.append(e)
        lens.append(k * ms)
        starts.append(int(rng.integers(0, ns[e] // ms - k + 1)) * ms)
    bins_case(src, a, results, info, 1, ent, starts, lens, ms)
    e = int(np.argmax(ns))
    bl = (10 * src.rate) // 2000             # 10 s in 2 000 bins: 960, 220
    s0 = (ns[e] // bl - 2000) // 2 * bl
    bins_case(src, a, results, info, 2, [e], [s0], [2000 * bl], bl)
    events_case(src, a, results, info, src.rate // 100)
    torch.cuda.empty_cache()


def config3(ctx, a, results, info, run=None):
    """run: what to do with the source (default: this tool's cases); other tools take the source from here"""
    lib = x3hip.lib()
    n, p, sig = a.samples, x3hip.Params.default(), a.fir or a.tone or x3hip.level_signal(a.signal)
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    x = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off, so = (torch.empty(F + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, x.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    del wav
    assert ctx.sample_offsets_dev(x.data_ptr(), pos, off.data_ptr(), F, so.data_ptr()) == 0
    ctx.sync()
    s = (x.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p)
    src = Source(
        ctx, "config3", 192_000, [n],
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_off, d_st: ctx.fir_range_levels_dev(*s, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                             d_off, d_st, idx.data_ptr(), 32, sig))
        if a.fir else
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_off, d_st: ctx.tone_range_levels_dev(*s, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                              d_off, d_st, idx.data_ptr(), 32, sig))
        if a.tone else
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_off, d_st: ctx.signal_range_levels_dev(*s, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                                d_off, d_st, idx.data_ptr(), 32, sig)),
        lambda d_e, d_s, d_l, k, stride, d_out, oc, d_off, d_st: ctx.decode_ranges_dev(*s, d_s, d_l, k, stride, d_out, oc, 0, d_off,
                                                                                       d_st, idx.data_ptr(), 32),
        (lambda bl, d_lv, rows: ctx.fir_levels_dev(*s, bl, d_lv, rows, None, idx.data_ptr(), 32, sig)) if a.fir else
        (lambda bl, d_lv, rows: ctx.tone_levels_dev(*s, bl, d_lv, rows, None, idx.data_ptr(), 32, sig)) if a.tone else
        (lambda bl, d_lv, rows: ctx.signal_levels_dev(*s, bl, d_lv, rows, None, idx.data_ptr(), 32, sig)),
        lambda d_lv, rows, bl, rule, d_e, d_s, d_l, d_el, c, d_c: ctx.events_dev(d_lv, rows, bl, so.data_ptr() + 8 * F, rule, d_s, d_l,
                                                                                d_el, c, d_c),
        lambda bl: np.array([0, -(-n // bl)], dtype=np.uint64),
        lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_off, d_st, tone: ctx.tone_range_levels_dev(*s, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                                  d_off, d_st, idx.data_ptr(), 32, tone),
        lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_off, d_st: ctx.tone_bank_range_levels_dev(*s, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                                 d_off, d_st, idx.data_ptr(), 32, a.tones))
    (run or cases)(src, a, results, info)


def corpus_a(ctx, a, results, info, run=None):
    lib = x3hip.lib()
    rng = np.random.default_rng(7)
    ns = [int(v) for v in rng.integers(441_000, 661_500 + 1, 4000)]
    n_clips, total = len(ns), int(sum(ns))
    p = x3hip.Params.default()
    spf = p.block_len * p.blocks_per_frame
    base = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    so, sn, first = [], [], []
    for c, n in enumerate(ns):
        first.append(len(so))
        for s in range(0, n, spf):
            so.append(int(base[c]) + s)
            sn.append(min(spf, n - s))
    F = len(so)
    first.append(F)
    cap = sum(lib.x3_encode_bound(n, C.byref(p)) + 2 for n in ns) + 64
    d_wav, d_x3, d_off = ctx.alloc(2 * total), ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    ctx.synth_dev(x3hip.SYNTH_HYDROPHONE, 0x5336, 0, total, d_wav)
    assert ctx.encode_frames_dev(d_wav, so, sn, p, d_x3, cap, 0, d_off) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    ctx.free(d_wav)
    fo = ctx.download(d_off, 8 * (F + 1), np.uint64)
    offs = [int(fo[first[c]]) for c in range(n_clips)]
    lens = [int(fo[first[c + 1]]) - offs[c] for c in range(n_clips)]
    corpus = x3hip.Corpus(ctx, (d_x3, pos), offs, lens, seg_blocks=32)
    sig = a.fir or a.tone or x3hip.level_signal(a.signal)
    src = Source(
        ctx, "corpus_a", 44_100, ns,
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o, d_st: corpus.fir_range_levels_into(d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o,
                                                                                               d_st, sig))
        if a.fir else
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o, d_st: corpus.tone_range_levels_into(d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o,
                                                                                                d_st, sig))
        if a.tone else
        (lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o, d_st: corpus.range_levels_into(d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o,
                                                                                           d_st, signal=sig)),
        lambda d_e, d_s, d_l, k, stride, d_out, oc, d_o, d_st: corpus.ranges_into(d_e, d_s, d_l, k, stride, d_out, oc, 0, d_o, d_st),
        (lambda bl, d_lv, rows: ctx.corpus_fir_levels_dev(corpus, bl, d_lv, rows, None, sig)) if a.fir else
        (lambda bl, d_lv, rows: ctx.corpus_tone_levels_dev(corpus, bl, d_lv, rows, None, sig)) if a.tone else
        (lambda bl, d_lv, rows: ctx.corpus_signal_levels_dev(corpus, bl, d_lv, rows, None, sig)),
        lambda d_lv, rows, bl, rule, d_e, d_s, d_l, d_el, c, d_c: corpus.events_into(d_lv, rows, bl, rule, d_e, d_s, d_l, d_el, c, d_c),
        lambda bl: corpus.levels_rows(bl),
        lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o, d_st, tone: corpus.tone_range_levels_into(d_e, d_s, d_l, k, bl, stride, d_lv,
                                                                                                    c, d_o, d_st, tone),
        lambda d_e, d_s, d_l, k, bl, stride, d_lv, c, d_o, d_st: corpus.tone_bank_range_levels_into(d_e, d_s, d_l, k, bl, stride, d_lv, c,
                                                                                                   d_o, d_st, a.tones))
    (run or cases)(src, a, results, info)
    corpus.close()
    for q in (d_x3, d_off):
        ctx.free(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--signal", default="samples", choices=["samples", "diff", "fir", "tone"])
    ap.add_argument("--taps", default="1,-2,1", help="--signal fir: the taps c[0], c[1], ..")
    ap.add_argument("--shift", type=int, default=0)
    ap.add_argument("--step", type=int, default=350_898_828, help="--signal tone: the oscillator's step (0.0817 of the sample rate)")
    ap.add_argument("--tones", type=int, default=0, choices=[0, 2, 3, 4, 5, 6, 7, 8], help="--signal tone: the bank call of K tones beside it")
    ap.add_argument("--no-route-a", action="store_true", help="the calls alone: no ranges + torch, no levels call (for kernel traces)")
    ap.add_argument("--levels-bytes", type=float, default=16e9, help="route b runs where its records and workspace fit in this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.taps = [int(c) for c in a.taps.split(",")]
    a.fir = x3hip.Fir(a.taps, a.shift) if a.signal == "fir" else None
    a.hist = {"samples": 0, "diff": 1, "fir": len(a.taps) - 1, "tone": 0}[a.signal]      # samples in front of a position that its value takes
    torch.cuda.init()
    ctx = x3hip.Context(0)
    a.tone = x3hip.Tone(a.step) if a.signal == "tone" else None
    if a.tones and a.signal != "tone":
        ap.error("--tones goes with --signal tone")
    a.tones = x3hip.Tone.bank(BANK_FREQS[:a.tones], 1.0) if a.tones else None
    if a.tones:
        a.tone = a.tones[0]
        a.step = a.tone.step
    if a.tone:
        a.table = torch.from_numpy(x3hip.tone_table().astype(np.int64)).cuda()
    results, info = {}, {}
    if "config3" in a.cases:
        config3(ctx, a, results, info)
    if "corpus" in a.cases:
        corpus_a(ctx, a, results, info)
    out = {"samples": a.samples, "reps": a.reps, "signal": a.signal, "cases": info,
           **({"taps": a.taps, "shift": a.shift} if a.fir else {}), **({"step": a.step} if a.tone else {}),
           **({"tones": len(a.tones), "steps": [t.step for t in a.tones]} if a.tones else {}),
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
