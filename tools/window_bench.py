#!/usr/bin/env python3
"""Random access against the whole decode: batches of random one-second windows (x3_decode_windows_dev) of config 3's stream
(1 h of hydrophone synth at 192 kHz, 691.2 M samples, encoded with x3_encode_dev_seg, seg_blocks 32), with and without the
segment index, in both formats, and the full x3_decode_dev_seg of the same stream -- in one process, the cases alternating
rep by rep.  Host time of a call: from the call to its x3_*_result (synchronised).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/window_bench.py --reps 5` (the x3_window_* kernels against
x3_decode_split_kernel).  Prints one JSON line.
    python3 tools/window_bench.py [--reps 20] [--warmup 3] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import x3hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L, sb, seed = a.samples, 192_000, 32, 0x58330003
    ctx = x3hip.Context(0)
    p = x3hip.Params.default()
    lib = x3hip.lib()
    F = lib.x3_num_frames(n, C.byref(p))
    cap = lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), sb)
    nmax = 256
    d_wav, d_x3, d_off, d_seg = ctx.alloc(2 * n), ctx.alloc(cap), ctx.alloc(8 * (F + 1)), ctx.alloc(8 * ne)
    d_so, d_st, d_out, d_status = ctx.alloc(8 * (F + 1)), ctx.alloc(8 * nmax), ctx.alloc(4 * nmax * L), ctx.alloc(4 * nmax)
    ctx.synth_dev(x3hip.SYNTH_HYDROPHONE, seed, 0, n, d_wav)
    assert ctx.encode_dev_seg(d_wav, n, p, d_x3, cap, d_seg, sb, 0, d_off) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    assert ctx.sample_offsets_dev(d_x3, pos, d_off, F, d_so) == 0
    ctx.sync()
    rng = np.random.default_rng(1)
    cases = [(nw, idx, fmt) for nw in (1, 16, 256) for idx in (True, False) for fmt in (0, 1)]
    times = {c: [] for c in cases}
    full = []

    def run_windows(nw, idx, fmt):
        ctx.upload(d_st, np.sort(rng.integers(0, n - L + 1, nw)).astype(np.uint64))
        ctx.sync()
        t0 = time.perf_counter()
        rc = ctx.decode_windows_dev(d_x3, pos, d_off, d_so, F, p, d_st, nw, L, d_out, fmt, d_status,
                                    d_seg if idx else None, sb if idx else 0)
        res = ctx.decode_windows_result()
        t = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and res == (0, 0, nw, 0), (rc, res)
        return t

    def run_full():
        t0 = time.perf_counter()
        rc = ctx.decode_dev_seg(d_x3, pos, d_off, F, p, d_wav, n, d_seg, sb, n_per_clip=n)
        res = ctx.decode_result()
        t = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and res == (0, F, 0, n), (rc, res)
        return t

    for rep in range(a.warmup + a.reps):
        order = list(cases)
        rng.shuffle(order)
        for c in order:
            t = run_windows(*c)
            if rep >= a.warmup:
                times[c].append(t)
        t = run_full()
        if rep >= a.warmup:
            full.append(t)
    # spot check: the last batch against the samples the stream was encoded from
    starts = np.sort(rng.integers(0, n - L + 1, 4)).astype(np.uint64)
    ctx.upload(d_st, starts)
    assert ctx.decode_windows_dev(d_x3, pos, d_off, d_so, F, p, d_st, 4, L, d_out, 0, d_status, d_seg, sb) == 0
    assert ctx.decode_windows_result() == (0, 0, 4, 0)
    rows = ctx.download(d_out, 2 * 4 * L, np.int16).reshape(4, L)
    for r, s in zip(rows, starts):
        assert np.array_equal(r, x3hip.synth(x3hip.SYNTH_HYDROPHONE, seed, int(s), L))
    med = lambda v: float(np.median(v))
    out = {"metric": "window_decode_host_ms_median", "samples": n, "window_len": L, "seg_blocks": sb, "reps": a.reps,
           "full_decode_dev_seg_ms": med(full)}
    for (nw, idx, fmt), v in times.items():
        out["w%d_%s_%s_ms" % (nw, "index" if idx else "noindex", "f32" if fmt else "i16")] = med(v)
    out["speedup_256_index_i16_vs_full"] = out["full_decode_dev_seg_ms"] / out["w256_index_i16_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for q in (d_wav, d_x3, d_off, d_seg, d_so, d_st, d_out, d_status):
        ctx.free(q)
    ctx.close()


if __name__ == "__main__":
    main()
