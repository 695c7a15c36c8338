#!/usr/bin/env python3
"""Ranges (x3_corpus_ranges_dev: a length per range, rows packed or padded) against the fixed-length window call of the same
total and against whole-entry decoding, on tools/corpus_bench.py's corpus, in one process, the cases alternating rep by rep:
  ranges_<k>_<packed|padded>_<i16|f32>   k ranges, entries at random, lengths uniform in 0.25 - 4 s, starts at random
  windows_<k>_<i16|f32>                  the fair measure of what the variable geometry costs: x3_corpus_windows_dev with k
                                         windows of L = the mean drawn length at the same entries -- the same total of
                                         samples and covering frames to within rounding
  drawn_<k>                              the loader's way today: x3_decode_streams_dev (int16) of just the drawn entries;
                                         the slicing behind it is not timed
Host time of a call: from the call to its result (synchronised).  Shapes: --shape a = 4 000 clips of 10-15 s at 44.1 kHz,
--shape b = 1 000 one-minute clips at 96 kHz.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3
tools/ranges_bench.py ...`.  Prints one JSON line.
    python3 tools/ranges_bench.py [--shape a|b] [--reps 10] [--warmup 2] [--out file.json]"""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    rate = 44_100 if a.shape == "a" else 96_000
    ns = rng.integers(441_000, 661_500 + 1, 4000) if a.shape == "a" else np.full(1000, 60 * 96_000)
    ns = [int(v) for v in ns]
    n_clips, total = len(ns), int(sum(ns))
    ctx = x3hip.Context(0)
    p = x3hip.Params.default()
    lib = x3hip.lib()
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
    lo, hi = rate // 4, 4 * rate
    K = (1, 256, 1024)
    kmax = max(K)
    row_len = (max(ns) + 3) // 4 * 4
    d_ent, d_st, d_wst, d_len = ctx.alloc(4 * kmax), ctx.alloc(8 * kmax), ctx.alloc(8 * kmax), ctx.alloc(4 * kmax)
    d_out, d_status, d_ooff = ctx.alloc(4 * kmax * hi), ctx.alloc(4 * kmax), ctx.alloc(8 * (kmax + 1))
    d_rows, d_res = ctx.alloc(2 * n_clips * row_len), ctx.alloc(24 * n_clips)
    now = time.perf_counter
    results, drawn = {}, {}

    def add(name, v):
        results.setdefault(name, []).append(v * 1e3)

    for rep in range(a.warmup + a.reps):
        keep = rep >= a.warmup
        for k in K:
            ents = rng.integers(0, n_clips, k).astype(np.uint32)
            ln = rng.integers(lo, hi + 1, k).astype(np.uint32)
            st = np.array([int(rng.integers(0, ns[e] - int(n) + 1)) for e, n in zip(ents, ln)], dtype=np.uint64)
            L = int(round(float(ln.mean())))
            wst = np.array([int(rng.integers(0, ns[e] - L + 1)) for e in ents], dtype=np.uint64)
            tot = int(ln.astype(np.int64).sum())
            for d, v in ((d_ent, ents), (d_st, st), (d_wst, wst), (d_len, ln)):
                ctx.upload(d, v)
            for fmt, fn in ((0, "i16"), (1, "f32")):
                for stride, sname in ((0, "packed"), (hi, "padded")):
                    t0 = now()
                    assert corpus.ranges_into(d_ent, d_st, d_len, k, stride, d_out, k * stride if stride else tot, fmt, d_ooff,
                                              d_status) == 0
                    r = ctx.decode_ranges_result()
                    dt = now() - t0
                    assert r == (0, 0, k, 0, tot), r
                    if keep:
                        add("ranges_%d_%s_%s" % (k, sname, fn), dt)
                t0 = now()
                assert corpus.decode_into(d_ent, d_wst, k, L, d_out, fmt, d_status) == 0
                r = ctx.decode_windows_result()
                dt = now() - t0
                assert r[:2] == (0, 0), r
                if keep:
                    add("windows_%d_%s" % (k, fn), dt)
            idx = sorted(set(int(e) for e in ents))
            t0 = now()
            assert ctx.decode_streams_dev(d_x3, pos, [offs[i] for i in idx], [lens[i] for i in idx], p, d_rows, row_len, 0, d_res) == 0
            assert ctx.decode_streams_result()[0] == 0
            dt = now() - t0
            if keep:
                add("drawn_%d" % k, dt)
                drawn.setdefault(k, []).append((tot, L))
    out = {"shape": a.shape, "clips": n_clips, "frames": F, "samples": total, "bytes": pos, "len_lo": lo, "len_hi": hi,
           "reps": a.reps, "mean_total_samples": {str(k): int(np.mean([t for t, _ in v])) for k, v in drawn.items()},
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    corpus.close()
    ctx.close()


if __name__ == "__main__":
    main()
