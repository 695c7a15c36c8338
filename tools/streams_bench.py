#!/usr/bin/env python3
"""Batches of streams (x3_decode_streams_dev) against what a loader can do without it, on one batch of clips encoded back to
back by x3_encode_frames_dev, in one process, the cases alternating rep by rep:
  streams_i16 / streams_f32   x3_decode_streams_dev .. x3_decode_streams_result, int16 / float32 rows
  floor                       x3_decode_dev with the encoder's own frame table and row offsets (what only the encoder knows)
  loop                        x3_decode_stream_dev once per clip (what a loader does today)
Host time of a call: from the call to its result (synchronised).  Shapes: --shape a = 4 000 clips of 10-15 s at 44.1 kHz of
varied lengths, --shape b = 1 000 one-minute clips at 96 kHz (config 5's shape).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/streams_bench.py ...`.  Prints one JSON line.
    python3 tools/streams_bench.py [--shape a|b] [--reps 10] [--warmup 2] [--loop-reps 2] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import x3hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("a", "b"), default="a")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    if a.shape == "a":
        ns = rng.integers(441_000, 661_500 + 1, 4000)
        ns = (ns // 4) * 4 + rng.integers(0, 4, ns.size)   # (varied: not all multiples of four)
    else:
        ns = np.full(1000, 60 * 96_000)
    ns = [int(v) for v in ns]
    n_clips, total = len(ns), int(sum(ns))
    row_len = (max(ns) + 3) // 4 * 4
    ctx = x3hip.Context(0)
    p = x3hip.Params.default()
    lib = x3hip.lib()
    spf = p.block_len * p.blocks_per_frame
    starts = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.uint64)
    so, sn, first = [], [], []
    for c, n in enumerate(ns):
        first.append(len(so))
        for s in range(0, n, spf):
            so.append(int(starts[c]) + s)
            sn.append(min(spf, n - s))
    F = len(so)
    first.append(F)
    cap = sum(lib.x3_encode_bound(n, C.byref(p)) + 2 for n in ns) + 64
    d_wav, d_x3, d_off = ctx.alloc(2 * total), ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    d_rows = ctx.alloc(4 * n_clips * row_len)
    d_res, d_woff = ctx.alloc(24 * n_clips), ctx.alloc(8 * F)
    ctx.synth_dev(x3hip.SYNTH_HYDROPHONE, 0x5335, 0, total, d_wav)
    assert ctx.encode_frames_dev(d_wav, so, sn, p, d_x3, cap, 0, d_off) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    fo = ctx.download(d_off, 8 * (F + 1), np.uint64)
    offs = [int(fo[first[c]]) for c in range(n_clips)]
    lens = [int(fo[first[c + 1]]) - offs[c] for c in range(n_clips)]
    woff = np.empty(F, dtype=np.uint64)   # the floor's row offsets: clip c's frames at c * row_len + k * spf
    for c in range(n_clips):
        k = first[c + 1] - first[c]
        woff[first[c]:first[c + 1]] = c * row_len + spf * np.arange(k, dtype=np.uint64)
    ctx.upload(d_woff, woff)
    x4 = ctx.get_option("wav_offsets_x4")

    def streams(fmt):
        assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, d_rows, row_len, fmt, d_res) == 0
        r = ctx.decode_streams_result()
        assert r[:2] == (0, 0), r

    def floor():
        ctx.set_option("wav_offsets_x4", 1)
        assert ctx.decode_dev(d_x3, pos, d_off, F, p, d_rows, n_clips * row_len, d_wav_offsets=d_woff) == 0
        r = ctx.decode_result()
        ctx.set_option("wav_offsets_x4", x4)
        assert r[:2] == (0, F), r

    cases = {"streams_i16": lambda: streams(0), "streams_f32": lambda: streams(1), "floor": floor}
    # the loop needs its clips on 4-byte boundaries (x3_decode_stream_dev): the encoder's even offsets mostly are not
    aligned = all(o % 4 == 0 for o in offs)
    times = {k: [] for k in list(cases) + ["loop"]}
    for k, f in cases.items():
        for _ in range(a.warmup):
            f()
    # correctness of what is timed: the rows equal the clips
    streams(0)
    for c in list(range(0, n_clips, max(1, n_clips // 50))) + [n_clips - 1]:
        got = ctx.download(d_rows + 2 * c * row_len, 2 * row_len, np.int16)
        ref = ctx.download(d_wav + 2 * int(starts[c]), 2 * ns[c], np.int16)
        assert np.array_equal(got[:ns[c]], ref) and not got[ns[c]:].any(), c
    general = ctx.get_option("last_streams_general_walks")
    for _ in range(a.reps):
        for k, f in cases.items():
            ctx.sync()
            t = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t) * 1e3)
    if not aligned:   # copy the clips to 4-byte boundaries once (not timed), then loop over them
        offs4, pos4 = [], 0
        for c in range(n_clips):
            offs4.append(pos4)
            pos4 += (lens[c] + 3) // 4 * 4
        d_x3b = ctx.alloc(pos4 + 64)
        for c in range(n_clips):
            ctx.upload(d_x3b + offs4[c], ctx.download(d_x3 + offs[c], lens[c]))
        d_src, offs_loop = d_x3b, offs4
    else:
        d_src, offs_loop = d_x3, offs

    def loop2():
        for c in range(n_clips):
            assert ctx.decode_stream_dev(d_src + offs_loop[c], lens[c], p, d_rows + 2 * c * row_len, row_len)[0] == 0

    loop2()
    for _ in range(a.loop_reps):
        ctx.sync()
        t = time.perf_counter()
        loop2()
        times["loop"].append((time.perf_counter() - t) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"shape": a.shape, "clips": n_clips, "samples": total, "stream_bytes": int(pos), "row_len": row_len, "frames": F,
           "general_walks": general, "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in times.items()},
           "streams_i16_vs_floor": med["streams_i16"] / med["floor"], "loop_vs_streams_i16": med["loop"] / med["streams_i16"],
           "reps": a.reps, "loop_reps": a.loop_reps}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
