#!/usr/bin/env python3
"""Parameter tuning: the tuning pass against one encode of the same samples, and what tuning gains.

usage: tune_bench.py [--samples N] [--clips C] [--kind K] [--steps S] [--no-gains]

  * timing: x3_tuner_add_dev over N samples of synthetic kind K (default config 3: 691.2 M samples of the hydrophone kind),
    C clips of N / C samples for a config-5 style batch, against x3_encode_dev + x3_encode_result of the same buffer, and
    the tuning pass on all-zero samples (the content X3 is for: it must not be the slow case).  Wall time per call,
    synchronized, median of S; the kernel's own time comes from a run under `rocprofv3 --kernel-trace --stats`.
    The read roofline is 2 N bytes at 6.29 TB/s (MI355X, measured float4 copy).
  * gains: 400 000 samples of each synthetic kind (seed 0x58330001, frames of 10 000), the default set's bytes against the
    chosen set's -- the table of the tuning issue.  Byte counts, not timings: they hold on any machine.
One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import x3hip  # noqa: E402

HBM_TBS = 6.29


def median_ms(fn, steps):
    fn()  # warm
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--kind", type=int, default=x3hip.SYNTH_HYDROPHONE)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-gains", action="store_true")
    a = ap.parse_args()
    ctx = x3hip.Context(0)
    L = x3hip.lib()
    npc = a.samples // a.clips
    n = npc * a.clips
    out = {"samples": n, "clips": a.clips, "kind": a.kind}
    d_wav = ctx.alloc(2 * n)
    ctx.synth_dev(a.kind, 0x58330001, 0, n, d_wav)
    p = x3hip.Params.default()
    cap = int(L.x3_encode_bound(npc, C.byref(p))) * a.clips
    d_out = ctx.alloc(cap)
    tuner = x3hip.Tuner(ctx)

    def tune_step():
        tuner.reset()
        assert tuner.add_dev(d_wav, npc, npc, a.clips) == 0
        rc, _, _, _ = tuner.result()
        assert rc == 0

    def encode_step():
        assert ctx.encode_dev(d_wav, npc, p, d_out, cap, n_clips=a.clips, clip_stride=npc) == 0
        assert ctx.encode_result()[0] == 0

    out["tune_ms"] = median_ms(tune_step, a.steps)
    out["encode_ms"] = median_ms(encode_step, a.steps)
    out["roofline_ms"] = 2 * n / (HBM_TBS * 1e12) * 1e3
    out["tune_roofline_share"] = out["roofline_ms"] / out["tune_ms"]
    rc, best, bb, sizes = tuner.result()
    out["chosen"] = [best.block_len] + list(best.thresholds)
    out["chosen_bytes"], out["default_bytes"] = int(bb), int(sizes[x3hip.TUNE_DEFAULT_INDEX])
    ctx.synth_dev(x3hip.SYNTH_ZEROS, 0, 0, n, d_wav)
    out["tune_zeros_ms"] = median_ms(tune_step, a.steps)
    tuner.close()
    ctx.free(d_out)
    ctx.free(d_wav)
    print("tune pass %.3f ms (all zeros %.3f), encode %.3f ms, read roofline %.3f ms (%.0f %% of it)"
          % (out["tune_ms"], out["tune_zeros_ms"], out["encode_ms"], out["roofline_ms"], 100 * out["tune_roofline_share"]))

    if not a.no_gains:
        gains = {}
        for name, kind in (("hydrophone", x3hip.SYNTH_HYDROPHONE), ("walk", x3hip.SYNTH_WALK), ("sine", x3hip.SYNTH_SINE),
                           ("white", x3hip.SYNTH_WHITE)):
            w = x3hip.synth(kind, 0x58330001, 0, 400_000)
            bp, bb, sizes = ctx.tune(w)
            d = int(sizes[x3hip.TUNE_DEFAULT_INDEX])
            gains[name] = {"default": d, "best": int(bb), "gain_pct": round(100.0 * (int(bb) - d) / d, 2),
                           "set": [bp.block_len] + list(bp.thresholds)}
            print("%-10s default %8d  best %8d (%+.1f %%)  block length %d; %d, %d, %d"
                  % ((name, d, bb, gains[name]["gain_pct"], bp.block_len) + tuple(bp.thresholds)))
        out["gains"] = gains
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
