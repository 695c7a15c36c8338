#!/usr/bin/env python3
"""Band levels (x3_spectra_levels_dev behind the ranges calls) against the route a caller had without it, in one process, the
routes' order reversed every other rep; medians of --reps (7) with minima and maxima, host time from the first call to the
last synchronised result.
  route a   range_band_levels: the ranges call (packed int16) and the levels call behind it, no host trip in between; no row
            per frame is stored
  route b   the ranges call, x3_spectra_rows_dev's POWER rows (a row per frame), then torch on the device: index_add of the
            bins into the bands, the clamp, index_add / scatter amax of the frames into the time bins.  Equal to route a in
            every record
  route c   (config 3 only) WindowSource.band_levels of the whole stream -- chunks of ranges, a sample buffer of
            --chunk-samples -- against x3_levels_dev of the same build at bin_len = frames_per_bin * hop, which reads the same
            stream once and forms no spectrum: what the spectra cost on top of a pass over the stream
on tools/spectra_bench.py's sources and three cases: config 3 (691.2 M samples at 192 kHz) and the
corpus of 4 000 clips; 1 024 ranges of 0.25-4 s, one 10 s range, and the slots of an events call.  n_fft = hop = 256, 32
frames a time bin, third-octave bands (band_edges_third_octave, 25 Hz .. 80 kHz) and one band per bin.  The tool FAILS unless
routes a and b agree with ==.  Kernel times: `rocprofv3 --kernel-trace --stats -- python3 tools/band_levels_bench.py
--no-routes ...`.  Prints one JSON line.
    python3 tools/band_levels_bench.py [--n-fft 256] [--hop N] [--frames-per-bin 32] [--reps 7] [--warmup 1] [--samples N]
                                       [--cases config3,corpus,stream] [--cap 4096] [--no-routes] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import x3hip
import range_levels_bench as RB
import spectra_bench as SB

now = time.perf_counter


def isqrt(v):
    """floor square roots of an int64 tensor of values below 2^32"""
    s = torch.sqrt(v.to(torch.float64)).to(torch.int64)
    s = s - (s * s > v).to(torch.int64)
    return s + ((s + 1) * (s + 1) <= v).to(torch.int64)


def band_case(src, a, results, info, case, ent, starts, lens):
    ctx, n, N, H, M = src.ctx, len(starts), a.n_fft, a.hop, a.frames_per_bin
    B = N // 2 + 1
    starts = [s - s % N for s in starts]
    rows = [x3hip.spectra_n_rows(v, N, H) for v in lens]
    bins = [-(-r // M) for r in rows]
    total_rows, total_bins, total = sum(rows), sum(bins), sum(lens)
    d_ent = torch.tensor(ent, dtype=torch.int32, device="cuda")
    d_st = torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_ln = torch.tensor(lens, dtype=torch.int32, device="cuda")
    buf, buf2 = (torch.empty(max(total, 1), dtype=torch.int16, device="cuda") for _ in range(2))
    soff, soff2, roff, roff2 = (torch.empty(n + 1, dtype=torch.int64, device="cuda") for _ in range(4))
    st, st2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    power = torch.empty((max(total_rows, 1), B), dtype=torch.int32, device="cuda")
    rule = x3hip.SpectraRule(N, H, x3hip.SPECTRA_POWER, 0, ctx.tone_table_dev())
    # route b: the time bin of every frame (made once, outside the timed part)
    first = np.concatenate([[0], np.cumsum(bins)[:-1]]).astype(np.int64)
    seg = torch.from_numpy(np.concatenate([f + np.arange(r, dtype=np.int64) // M for f, r in zip(first, rows)] or [np.zeros(0, np.int64)])).cuda()
    maps = {"third_octave": x3hip.spectra_bin_band(N, x3hip.band_edges_third_octave(N, src.rate, 25, 80_000)),
            "per_bin": x3hip.spectra_bin_band(N, None)}
    for tag, (m, K) in maps.items():
        name = "%s_case%d_%s" % (src.name, case, tag)
        d_map = torch.from_numpy(m.view(np.int32)).cuda()
        idx = torch.from_numpy(m.astype(np.int64)).cuda()
        keep = idx < K
        fold = x3hip.SpectraFold(M, K, 0, d_map.data_ptr(), 0)
        levels = torch.empty((K, max(total_bins, 1), 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        want_b = None

        def route_a():
            rc = src.ranges(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, 0, buf.data_ptr(), max(total, 1), soff.data_ptr(), st.data_ptr())
            assert rc == 0, ctx.last_error()
            rc = ctx.spectra_levels_dev(buf.data_ptr(), max(total, 1), soff.data_ptr(), d_ln.data_ptr(), st.data_ptr(), n, rule, fold, 0,
                                        levels.data_ptr(), max(total_bins, 1), roff.data_ptr(), st.data_ptr())
            assert rc == 0, ctx.last_error()
            r = ctx.decode_ranges_result()
            assert r[:2] == (0, 0), r
            r = ctx.spectra_result()
            assert r == (0, 0, n, 0, total_bins), r

        def route_b():
            nonlocal want_b
            rc = src.ranges(d_ent.data_ptr(), d_st.data_ptr(), d_ln.data_ptr(), n, 0, buf2.data_ptr(), max(total, 1), soff2.data_ptr(), st2.data_ptr())
            assert rc == 0, ctx.last_error()
            rc = ctx.spectra_rows_dev(buf2.data_ptr(), max(total, 1), soff2.data_ptr(), d_ln.data_ptr(), st2.data_ptr(), n, rule, 0,
                                      power.data_ptr(), max(total_rows, 1), roff2.data_ptr(), st2.data_ptr())
            assert rc == 0, ctx.last_error()
            r = ctx.decode_ranges_result()
            assert r[:2] == (0, 0), r
            r = ctx.spectra_result()
            assert r == (0, 0, n, 0, total_rows), r
            ms = power[:total_rows].to(torch.int64)
            bp = torch.zeros((total_rows, K), dtype=torch.int64, device="cuda").index_add_(1, idx[keep], ms[:, keep]).clamp_(max=1 << 30)
            sums = torch.zeros((total_bins, K), dtype=torch.int64, device="cuda").index_add_(0, seg, bp)
            top = torch.zeros((total_bins, K), dtype=torch.int64, device="cuda").scatter_reduce_(0, seg[:, None].expand(-1, K), bp, "amax")
            cnt = torch.zeros(total_bins, dtype=torch.int64, device="cuda").index_add_(0, seg, torch.ones_like(seg))
            peak = isqrt(2 * top).clamp_(max=32767)
            rec = torch.zeros((K, total_bins, 4), dtype=torch.int64, device="cuda")      # sum_sq, sum, (min, max), (n, reserved)
            rec[:, :, 0] = sums.t()
            rec[:, :, 2] = ((-peak.t()) & 0xFFFFFFFF) | (peak.t() << 32)
            rec[:, :, 3] = cnt[None, :]
            want_b = rec
            torch.cuda.synchronize()

        routes = [("route_a", route_a)] + ([] if a.no_routes else [("route_b", route_b)])
        for rep in range(a.warmup + a.reps):
            for key, fn in (routes if rep % 2 == 0 else routes[::-1]):
                t = now()
                fn()
                RB.timed(results, name + "_" + key, rep, a.warmup, now() - t)
        same = not st.cpu().numpy().any()
        if want_b is not None:
            same = same and bool(torch.equal(levels[:, :total_bins].contiguous().view(torch.int64).view(K, total_bins, 4), want_b))
        if not same:
            raise SystemExit("%s: the routes' records differ" % name)
        info[name] = {"ranges": n, "frames": total_rows, "time_bins": total_bins, "samples": total, "bands": K,
                      "out_bytes": total_bins * K * 32, "rows_bytes": total_rows * B * 4, "equal": bool(same),
                      "route_b_compared": want_b is not None}
        del levels, want_b
        torch.cuda.empty_cache()


def whole_stream(ctx, a, results, info):
    """route c: config 3's stream as a WindowSource; band_levels against the levels call at the same bin length"""
    lib = x3hip.lib()
    n, p = a.samples, x3hip.Params.default()
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    x = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, x.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    del wav
    torch.cuda.empty_cache()
    ws = x3hip.WindowSource(ctx, (x.data_ptr(), pos), p, seg_blocks=32, frame_offsets=off.data_ptr(), n_frames=F, seg_index=idx.data_ptr())
    N, H, M, q = a.n_fft, a.hop, a.frames_per_bin, 4           # (q: band_levels' default, rows a range)
    bin_len = M * H
    n_bins = -(-n // bin_len)
    edges = x3hip.band_edges_third_octave(N, 192_000, 25, 80_000)
    plain = torch.empty((n_bins, 32), dtype=torch.uint8, device="cuda")
    sig = x3hip.level_signal("samples")
    planes = None

    def band():
        nonlocal planes
        planes = ws.band_levels(N, H, frames_per_bin=M, bands=edges, chunk_samples=a.chunk_samples, q=q)
        torch.cuda.synchronize()

    def levels():
        rc = ctx.signal_levels_dev(ws.d_x3, ws.x3_len, ws.d_frame_offsets, ws.d_sample_offsets, F, p, bin_len, plain.data_ptr(), n_bins,
                                   None, idx.data_ptr(), 32, sig)
        assert rc == 0, ctx.last_error()
        assert ctx.levels_result()[0] == 0

    routes = [("band_levels", band), ("levels", levels)]
    for rep in range(a.warmup + a.reps):
        for key, fn in (routes if rep % 2 == 0 else routes[::-1]):
            t = now()
            fn()
            RB.timed(results, "config3_stream_" + key, rep, a.warmup, now() - t)
    rec, lv = RB.records(planes[0]), RB.records(plain)
    whole = (n - N) // bin_len                                  # rows whose M frames all lie in the stream
    assert tuple(planes.shape) == (len(edges) - 1, n_bins, 32) and (rec["n"][:whole] == M).all()
    assert (lv["n"][:n_bins - 1] == bin_len).all()
    range_len = (q * M - 1) * H + N                            # band_levels' ranges and chunks, by its own rule
    n_ranges, per_chunk = -(-n // (q * bin_len)), max(1, a.chunk_samples // range_len)
    info["config3_stream"] = {"samples": n, "time_bins": n_bins, "bands": len(edges) - 1, "chunk_samples": a.chunk_samples, "q": q,
                              "ranges": n_ranges, "chunks": -(-n_ranges // per_chunk), "out_bytes": n_bins * (len(edges) - 1) * 32}
    ws.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-fft", type=int, default=256, choices=list(x3hip.SPECTRA_NFFTS))
    ap.add_argument("--hop", type=int, default=0, help="0: n_fft")
    ap.add_argument("--frames-per-bin", type=int, default=32)
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--cases", default="config3,corpus,stream")
    ap.add_argument("--chunk-samples", type=int, default=1 << 26)
    ap.add_argument("--no-routes", action="store_true", help="route a alone (for kernel traces)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.hop = a.hop or a.n_fft
    a.source = argparse.Namespace(samples=a.samples, signal="samples", fir=None, tone=None, tones=None)
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, info = {}, {}
    run = lambda src, _, results, info: SB.cases(src, a, results, info, band_case)
    picked = a.cases.split(",")
    if "config3" in picked:
        RB.config3(ctx, a.source, results, info, run)
    if "corpus" in picked:
        RB.corpus_a(ctx, a.source, results, info, run)
    if "stream" in picked:
        whole_stream(ctx, a, results, info)
    out = {"samples": a.samples, "reps": a.reps, "n_fft": a.n_fft, "hop": a.hop, "frames_per_bin": a.frames_per_bin, "cases": info,
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
