#!/usr/bin/env python3
"""Levels behind an integer FIR filter (x3_fir_levels_dev / x3_corpus_fir_levels_dev) on tools/levels_bench.py's cases, the
sides alternating rep by rep in one process; medians of --reps, host time from the call to the synchronised result:
  fir3            the FIR call with {1, -2, 1}
  fir8            the FIR call with eight taps of mixed signs and shift 7
  diff            the DIFF call of the same build (x3_signal_levels_dev)
  decode_torch3 / decode_torch8
                  the status quo: decode into a sample buffer (x3_decode_dev_seg / x3_decode_streams_dev), then in torch
                  conv1d (float64: sums below 2^30 are exact), shift, clamp and the same five reductions
Cases: config3_20_<bin> -- the stream kbench.py makes (691.2 M hydrophone samples, block length 20, the encoder's segment
index), bin_len 1920 and 0; corpus_a_0 -- 4 000 clips of 10-15 s at 44.1 kHz, one record per clip.  The records of the FIR
calls and of decode_torch are compared with == (every field, n included).  Device memory of both sides goes into the line.
Kernel times (the seam kernel's among them): run it with --no-torch under
`rocprofv3 --kernel-trace --stats -- python3 tools/fir_levels_bench.py --no-torch ...`.  Prints one JSON line.
    python3 tools/fir_levels_bench.py [--samples N] [--clips N] [--reps 10] [--warmup 2] [--cases config3,corpus] [--no-torch]
                                      [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip

now = time.perf_counter
FIRS = {"3": x3hip.Fir([1, -2, 1]), "8": x3hip.Fir([-3000, 9000, -200, 7, 5000, -8000, 1, 6560], 7)}
CHUNK = 1 << 26   # samples per conv1d call of the flat case: 0.5 GB of float64 in, as much out


def fir_flat(x, fir):
    """x: int16 [n] -> y int32 [n]: the filter's output at positions T - 1 .. n - 1, position T - 1's value in front of it"""
    T, n = len(fir.taps), x.numel()
    w = torch.tensor(fir.taps[::-1], dtype=torch.float64, device=x.device).view(1, 1, T)
    y = torch.empty(n, dtype=torch.int32, device=x.device)
    for a in range(T - 1, n, CHUNK):
        b = min(n, a + CHUNK)
        acc = torch.nn.functional.conv1d(x[a - (T - 1):b].to(torch.float64).view(1, 1, -1), w).view(-1).to(torch.int64)
        y[a:b] = (acc >> fir.shift).clamp_(-32768, 32767).to(torch.int32)
    y[:T - 1] = y[T - 1]
    return y


def reduce_flat(x, bin_len, fir):
    """(min, max, sum, sum_sq, n) of the filter's output per bin of bin_len positions (whole bins; bin_len >= T - 1) or over
    everything.  The T - 1 positions in front hold no value: they were given position T - 1's, which leaves min and max alone,
    and are taken out of the first bin's sums again."""
    T = len(fir.taps)
    y = fir_flat(x, fir)
    first = y[0].to(torch.int64)
    if bin_len:
        r = y[: y.numel() // bin_len * bin_len].view(-1, bin_len)
        mn, mx, sm, sq = r.min(1).values, r.max(1).values, r.sum(1, dtype=torch.int64), (r * r).sum(1, dtype=torch.int64)
        cnt = torch.full((r.shape[0],), bin_len, dtype=torch.int64, device=x.device)
    else:
        mn, mx, sm, sq = y.min().view(1), y.max().view(1), y.sum(dtype=torch.int64).view(1), (y * y).sum(dtype=torch.int64).view(1)
        cnt = torch.full((1,), y.numel(), dtype=torch.int64, device=x.device)
    sm[0] -= (T - 1) * first
    sq[0] -= (T - 1) * first * first
    cnt[0] -= T - 1
    torch.cuda.synchronize()
    return mn, mx, sm, sq, cnt


def equal(rec, red, rows):
    return bool(np.array_equal(rec["min"][:rows], red[0].cpu().numpy()) and np.array_equal(rec["max"][:rows], red[1].cpu().numpy()) and
                np.array_equal(rec["sum"][:rows], red[2].cpu().numpy()) and
                np.array_equal(rec["sum_sq"][:rows].astype(np.int64), red[3].cpu().numpy()) and
                np.array_equal(rec["n"][:rows].astype(np.int64), red[4].cpu().numpy()))


def config3(ctx, a, results, mem, checks):
    lib = x3hip.lib()
    n = a.samples
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    back = torch.empty(n, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    p = x3hip.Params.make(20, 500)
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    nseg = (ne - 1) // F + 1
    out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    so = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, out.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    assert ctx.sample_offsets_dev(out.data_ptr(), pos, off.data_ptr(), F, so.data_ptr()) == 0
    ctx.sync()
    del wav
    for bin_len in (1920, 0):
        n_bins = -(-n // bin_len) if bin_len else 1
        lv = {k: torch.empty(4 * n_bins, dtype=torch.int64, device="cuda") for k in ("diff", "3", "8")}
        name = "config3_20_%d" % bin_len
        peak, red = 0, {}
        for rep in range(a.warmup + a.reps):
            t = {}
            t0 = now()
            assert ctx.signal_levels_dev(out.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, bin_len, lv["diff"].data_ptr(), n_bins,
                                         None, idx.data_ptr(), 32, x3hip.LEVEL_SIGNAL_DIFF) == 0
            r = ctx.levels_result()
            t["diff"] = now() - t0
            assert r[:2] == (0, 0), r
            for k, fir in FIRS.items():
                t0 = now()
                assert ctx.fir_levels_dev(out.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, bin_len, lv[k].data_ptr(), n_bins,
                                          None, idx.data_ptr(), 32, fir) == 0
                r = ctx.levels_result()
                t["fir" + k] = now() - t0
                assert r[:2] == (0, 0), r
                assert ctx.get_option("last_levels_replays") == 0
            for k, fir in FIRS.items() if not a.no_torch else ():
                red.pop(k, None)
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = now()
                assert ctx.decode_dev_seg(out.data_ptr(), pos, off.data_ptr(), F, p, back.data_ptr(), n, idx.data_ptr(), 32, n_per_clip=n) == 0
                assert ctx.decode_result()[0] == 0
                red[k] = reduce_flat(back, bin_len, fir)
                t["decode_torch" + k] = now() - t0
                peak = max(peak, torch.cuda.max_memory_allocated() - base)
            if rep >= a.warmup:
                for side, v in t.items():
                    results.setdefault(name + "_" + side, []).append(v * 1e3)
        for k in red:
            checks[name + "_fir" + k] = equal(lv[k].cpu().numpy().view(x3hip.LEVEL_DTYPE), red[k], n // bin_len if bin_len else 1)
        mem[name] = {"levels_bytes": 32 * n_bins + 32 * (n_bins + F) + 48 * F, "fir_edge_bytes": 32 * F * nseg,
                     "decode_torch_bytes": 2 * n + int(peak), "stream_bytes": int(pos), "frames": int(F)}
        del lv, red
    del out, off, so, idx, back
    torch.cuda.empty_cache()


def corpus_a(ctx, a, results, mem, checks):
    lib = x3hip.lib()
    rng = np.random.default_rng(7)
    ns = [int(v) for v in rng.integers(441_000, 661_500 + 1, a.clips)]
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
    nseg = (corpus.seg_index_words - 1) // F + 1 if corpus.seg_index_words else 1
    n_rows = int(corpus.levels_rows(0)[-1])
    lv = {k: torch.empty(4 * n_rows, dtype=torch.int64, device="cuda") for k in ("diff", "3", "8")}
    row_len = (max(ns) + 3) // 4 * 4
    rows = torch.empty(n_clips * row_len, dtype=torch.int16, device="cuda")
    res = torch.empty(24 * n_clips, dtype=torch.uint8, device="cuda")
    t_ns = torch.tensor(ns, device="cuda").view(-1, 1)
    peak, red = 0, {}
    for rep in range(a.warmup + a.reps):
        t = {}
        t0 = now()
        assert ctx.corpus_signal_levels_dev(corpus, 0, lv["diff"].data_ptr(), n_rows, None, x3hip.LEVEL_SIGNAL_DIFF) == 0
        r = ctx.levels_result()
        t["diff"] = now() - t0
        assert r[:2] == (0, 0), r
        for k, fir in FIRS.items():
            t0 = now()
            assert ctx.corpus_fir_levels_dev(corpus, 0, lv[k].data_ptr(), n_rows, None, fir) == 0
            r = ctx.levels_result()
            t["fir" + k] = now() - t0
            assert r[:2] == (0, 0), r
        for k, fir in FIRS.items() if not a.no_torch else ():
            T = len(fir.taps)
            red.pop(k, None)
            torch.cuda.reset_peak_memory_stats()
            base_mem = torch.cuda.memory_allocated()
            t0 = now()
            assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, rows.data_ptr(), row_len, 0, res.data_ptr()) == 0
            assert ctx.decode_streams_result()[0] == 0
            w = torch.tensor(fir.taps[::-1], dtype=torch.float64, device="cuda").view(1, 1, T)
            col = torch.arange(T - 1, row_len, device="cuda").view(1, -1)
            parts = []
            for c0 in range(0, n_clips, 250):          # (250 clips: 1.3 GB of float64 in, as much out)
                x = rows.view(n_clips, row_len)[c0:c0 + 250]
                acc = torch.nn.functional.conv1d(x.to(torch.float64).unsqueeze(1), w).squeeze(1).to(torch.int64)
                y = (acc >> fir.shift).clamp_(-32768, 32767)
                inside = col < t_ns[c0:c0 + 250]       # (position i of a clip holds a value for T - 1 <= i < its samples)
                mn = torch.where(inside, y, torch.full_like(y, 32767)).min(1).values
                mx = torch.where(inside, y, torch.full_like(y, -32768)).max(1).values
                y = torch.where(inside, y, torch.zeros_like(y))
                parts.append((mn, mx, y.sum(1), (y * y).sum(1)))
                del x, acc, y, inside
            red[k] = tuple(torch.cat([q[j] for q in parts]) for j in range(4)) + (torch.tensor(ns, dtype=torch.int64) - (T - 1),)
            torch.cuda.synchronize()
            t["decode_torch" + k] = now() - t0
            peak = max(peak, torch.cuda.max_memory_allocated() - base_mem)
        if rep >= a.warmup:
            for side, v in t.items():
                results.setdefault("corpus_a_0_" + side, []).append(v * 1e3)
    for k in red:
        checks["corpus_a_0_fir" + k] = equal(lv[k].cpu().numpy().view(x3hip.LEVEL_DTYPE), red[k], n_rows)
    mem["corpus_a_0"] = {"levels_bytes": 32 * n_rows + 32 * (n_rows + F) + 48 * F + 8 * (n_clips + 1), "fir_edge_bytes": 32 * F * nseg,
                         "decode_torch_bytes": 2 * n_clips * row_len + int(peak), "stream_bytes": int(pos), "frames": int(F),
                         "clips": n_clips, "samples": total}
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, mem, checks = {}, {}, {}
    if "config3" in a.cases:
        config3(ctx, a, results, mem, checks)
    if "corpus" in a.cases:
        corpus_a(ctx, a, results, mem, checks)
    out = {"samples": a.samples, "clips": a.clips, "reps": a.reps, "fir_equal_to_torch": checks, "memory": mem,
           "taps": {k: {"taps": list(f.taps), "shift": f.shift} for k, f in FIRS.items()},
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    if not all(checks.values()):
        sys.exit("records differ: %s" % checks)


if __name__ == "__main__":
    main()
