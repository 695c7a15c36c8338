#!/usr/bin/env python3
"""Range spectra (x3_spectra_rows_dev behind the ranges calls) against the two routes a caller has without it, in one process,
the routes' order alternating rep by rep; medians of --reps (7) with minima and maxima, host time from the first call to the
last synchronised result.
  route a   range_spectra: the ranges call (packed int16) and the spectra call behind it, no host trip in between
  route b   the ranges call, then the frames gathered from the packed samples and ONE torch matmul against the same basis.
            torch has no integer matmul on the device; float64 is exact here -- every product is below 2^30 in size and a sum
            of n_fft <= 1 024 of them below 2^40 -- and the sums go back to int64.  Equal to route a on every frame
  route c   ceil(B / 8) tone_bank_range_levels calls at bin_len = n_fft, eight bins of the spectrum a call.  Equal to route a
            on the frames that sit at multiples of n_fft of their stream or entry (compared where hop == n_fft); timed on all
on tools/range_levels_bench.py's two sources and three cases: config 3 (691.2 M samples at 192 kHz) and
the corpus of 4 000 clips; 1 024 ranges of 0.25-4 s, one 10 s range, and the slots of an events call.  Starts are moved down
to multiples of n_fft, so that with hop == n_fft every frame is route c's.  The tool FAILS unless the routes agree with ==.
Kernel times: `rocprofv3 --kernel-trace --stats -- python3 tools/spectra_bench.py --no-routes ...`.  Prints one JSON line.
    python3 tools/spectra_bench.py [--n-fft 256] [--hop N] [--power | --sums] [--reps 7] [--warmup 1] [--samples N]
                                   [--cases config3,corpus] [--cap 4096] [--no-routes] [--no-route-c] [--out file.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import x3hip
import range_levels_bench as RB

now = time.perf_counter


def basis(n_fft):
    """float64 [N, 2 * B] on the device: cos columns, then sin columns, of the usual table"""
    tab = x3hip.tone_table().astype(np.float64)
    n, k = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None, :]
    idx = ((n * k) % n_fft) * (1024 // n_fft)
    return torch.from_numpy(np.concatenate([tab[idx, 0], tab[idx, 1]], axis=1)).cuda()


def power_of(re, im, n_fft):
    a, b = re >> 15, im >> 15
    return torch.clamp((2 * (a * a + b * b) // n_fft) // n_fft, max=1 << 30)


def spectra_case(src, a, results, info, case, ent, starts, lens):
    ctx, n, N, H = src.ctx, len(starts), a.n_fft, a.hop
    name = "%s_case%d" % (src.name, case)
    B = N // 2 + 1
    starts = [s - s % N for s in starts]
    rows = [x3hip.spectra_n_rows(v, N, H) for v in lens]
    total_rows, total = sum(rows), sum(lens)
    d_ent = torch.tensor(ent, dtype=torch.int32, device="cuda")
    d_st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    buf, buf2 = (torch.empty(max(total, 1), dtype=torch.int16, device="cuda") for _ in range(2))
    soff, soff2, roff, roff_c = (torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(4))
    st, st2, st_c = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    out = torch.empty((max(total_rows, 1), B) if a.power else (max(total_rows, 1), B, 2), dtype=torch.int32 if a.power else torch.int64,
                      device="cuda")
    rule = x3hip.SpectraRule(N, H, x3hip.SPECTRA_POWER if a.power else x3hip.SPECTRA_SUMS, 0, ctx.tone_table_dev())
    # route b: where every frame begins in the packed samples (made once, outside the timed part)
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    at = torch.from_numpy(np.concatenate([f + H * np.arange(r, dtype=np.int64) for f, r in zip(first, rows)] or [np.zeros(0, np.int64)])).cuda()
    col = torch.arange(N, device="cuda")[None, :]
    bs = basis(N)
    # route c: the bank's records, a bin of n_fft positions a record; frame r of range w is its record r when hop == n_fft
    rows_c = [max(1, -(-v // N)) for v in lens]
    total_c = sum(rows_c)
    groups = [list(range(k, min(k + 8, B))) for k in range(0, B, 8)]
    lv_c = torch.empty((len(groups), 8, total_c, 32), dtype=torch.uint8, device="cuda") if not a.no_route_c else None
    torch.cuda.synchronize()
    want_b = None

    def route_a():
        rc = src.ranges(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, 0, buf.data_ptr(), max(total, 1), soff.data_ptr(), st.data_ptr())
        assert rc == 0, ctx.last_error()
        rc = ctx.spectra_rows_dev(buf.data_ptr(), max(total, 1), soff.data_ptr(), d_ln.data_ptr(), st.data_ptr(), n, rule, 0, out.data_ptr(),
                                  max(total_rows, 1), roff.data_ptr(), st.data_ptr())
        assert rc == 0, ctx.last_error()
        r = ctx.decode_ranges_result()
        assert r[:2] == (0, 0), r
        r = ctx.spectra_result()
        assert r == (0, 0, n, 0, total_rows), r

    def route_b():
        nonlocal want_b
        rc = src.ranges(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, 0, buf2.data_ptr(), max(total, 1), soff2.data_ptr(), st2.data_ptr())
        assert rc == 0, ctx.last_error()
        r = ctx.decode_ranges_result()
        assert r[:2] == (0, 0), r
        parts = []
        for lo in range(0, total_rows, a.chunk_rows):      # (the frames as float64: 8 * n_fft bytes a row)
            fr = buf2[at[lo:lo + a.chunk_rows, None] + col].to(torch.float64)
            s = (fr @ bs).to(torch.int64)
            parts.append(power_of(s[:, :B], s[:, B:], N).to(torch.int32) if a.power else torch.stack([s[:, :B], s[:, B:]], dim=2))
        want_b = torch.cat(parts) if parts else None
        torch.cuda.synchronize()

    def route_c():
        for g, ks in enumerate(groups):
            a.source.tones = tuple(x3hip.Tone(k * (2 ** 32 // N)) for k in ks)      # (the bank of this call: eight bins)
            rc = src.bank_call(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, N, 0, lv_c[g].data_ptr(), total_c, roff_c.data_ptr(),
                               st_c.data_ptr())
            assert rc == 0, ctx.last_error()
            r = ctx.range_levels_result()
            assert r[:4] == (0, 0, n, 0), r

    routes = [("route_a", route_a)] + ([] if a.no_routes else [("route_b", route_b)] + ([] if a.no_route_c else [("route_c", route_c)]))
    for rep in range(a.warmup + a.reps):
        for key, fn in (routes if rep % 2 == 0 else routes[::-1]):
            t = now()
            fn()
            RB.timed(results, name + "_" + key, rep, a.warmup, now() - t)
    same = not st.cpu().numpy().any()
    got = out[:total_rows]
    if want_b is not None:
        same = same and bool(torch.equal(got, want_b))
    compared_c = 0
    if not a.no_routes and not a.no_route_c and H == N and total_rows:
        first_c = np.concatenate([[0], np.cumsum(rows_c)[:-1]])
        pick = torch.from_numpy(np.concatenate([f + np.arange(r, dtype=np.int64) for f, r in zip(first_c, rows)])).cuda()
        for g, ks in enumerate(groups):
            rec = lv_c[g][:len(ks), pick].contiguous().view(torch.int64).view(len(ks), total_rows, 4)     # re, im, (min, max), (n, 0)
            re, im = rec[:, :, 0].t(), rec[:, :, 1].t()
            if a.power:
                same = same and bool(torch.equal(got[:, ks[0]:ks[-1] + 1], power_of(re, im, N).to(torch.int32)))
            else:
                same = same and bool(torch.equal(got[:, ks[0]:ks[-1] + 1, 0], re)) and bool(torch.equal(got[:, ks[0]:ks[-1] + 1, 1], im))
        compared_c = total_rows
    if not same:
        raise SystemExit("%s: the routes' spectra differ" % name)
    info[name] = {"ranges": n, "rows": total_rows, "samples": total, "bins": B, "out_bytes": total_rows * B * (4 if a.power else 16),
                  "bank_calls": len(groups), "equal": bool(same), "route_b_compared": want_b is not None, "route_c_rows_compared": compared_c}
    del lv_c, want_b
    torch.cuda.empty_cache()


def cases(src, a, results, info, spectra_case=spectra_case):
    """tools/range_levels_bench.py's three cases: its 1 024 ranges, its 10 s range, the slots of its events call
    (spectra_case: what runs on each; tools/band_levels_bench.py brings its own)"""
    rng = np.random.default_rng(11)
    ms, ns = src.rate // 1000, src.n_samples
    ent, starts, lens = [], [], []
    for _ in range(1024):
        e = int(rng.integers(0, len(ns)))
        k = min(int(rng.integers(250, 4001)), ns[e] // ms)
        ent.append(e)
        lens.append(k * ms)
        starts.append(int(rng.integers(0, ns[e] // ms - k + 1)) * ms)
    spectra_case(src, a, results, info, 1, ent, starts, lens)
    e = int(np.argmax(ns))
    bl = (10 * src.rate) // 2000
    spectra_case(src, a, results, info, 2, [e], [(ns[e] // bl - 2000) // 2 * bl], [2000 * bl])
    # case 3: the events of levels at 10 ms under range_levels_bench's rule, as its events_case finds them
    ctx, cap, bin_len = src.ctx, a.cap, src.rate // 100
    n_rows = int(src.levels_rows(bin_len)[-1])
    full = torch.empty((n_rows, 32), dtype=torch.uint8, device="cuda")
    d_e, d_s, d_l = (torch.zeros(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    cnt = torch.zeros((), dtype=torch.int64, device="cuda")
    ev_lv = torch.empty((cap, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert src.levels(bin_len, full.data_ptr(), n_rows) == 0 and ctx.levels_result()[0] == 0
    rec = RB.records(full)
    q = 100.0 * (1.0 - min(0.002, cap / (4.0 * n_rows)))
    peak_min = int(min(max(np.percentile(np.maximum(rec["max"], -rec["min"])[rec["n"] != 0], q) + 1, 1), 32768))
    rule = x3hip.EventRule.make(0, peak_min, RB.JOIN, RB.MIN_BINS, RB.PAD, RB.MAX_BINS)
    assert src.events(full.data_ptr(), n_rows, bin_len, rule, d_e.data_ptr(), d_s.data_ptr(), d_l.data_ptr(), ev_lv.data_ptr(), cap,
                      cnt.data_ptr()) == 0
    rc, found = ctx.events_result()
    assert rc == 0 and found > 0, (rc, found)
    del full
    k = min(int(found), cap)
    spectra_case(src, a, results, info, 3, d_e.cpu().numpy()[:k].tolist(), d_s.cpu().numpy()[:k].tolist(), d_l.cpu().numpy()[:k].tolist())
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-fft", type=int, default=256, choices=list(x3hip.SPECTRA_NFFTS))
    ap.add_argument("--hop", type=int, default=0, help="0: n_fft")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--power", dest="power", action="store_true", default=True)
    g.add_argument("--sums", dest="power", action="store_false")
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--chunk-rows", type=int, default=1 << 19, help="route b: frames a matmul")
    ap.add_argument("--no-routes", action="store_true", help="route a alone (for kernel traces)")
    ap.add_argument("--no-route-c", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.hop = a.hop or a.n_fft
    # the arguments range_levels_bench's sources are built from: the plain signal; their bank call reads .tones when it runs
    a.source = argparse.Namespace(samples=a.samples, signal="samples", fir=None, tone=None, tones=None)
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, info = {}, {}
    run = lambda src, _, results, info: cases(src, a, results, info)
    if "config3" in a.cases:
        RB.config3(ctx, a.source, results, info, run)
    if "corpus" in a.cases:
        RB.corpus_a(ctx, a.source, results, info, run)
    out = {"samples": a.samples, "reps": a.reps, "n_fft": a.n_fft, "hop": a.hop, "format": "power" if a.power else "sums", "cases": info,
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
