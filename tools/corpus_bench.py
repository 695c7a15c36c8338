#!/usr/bin/env python3
"""Corpus windows (x3_corpus_build / x3_corpus_windows_dev) against single-stream windows and whole-entry decoding, on one
corpus of clips encoded back to back by x3_encode_frames_dev, in one process, the cases alternating rep by rep:
  build_32 / build_0        x3_corpus_build with seg_blocks 32 / 0 (synchronous; index bytes reported)
  streams_all               x3_decode_streams_dev int16 of every clip (the build's yardstick)
  corpus_<k>_<sb>           k random one-second windows per call, seg_blocks 32 / 0
  single_<k>_<sb>           the fair baseline: the same buffer as ONE stream (the encoder's frame table) and
                            x3_decode_windows_dev at the same global positions -- the same work but for the plan step
  drawn_<k>                 the loader's alternative today: x3_decode_streams_dev of just the drawn entries
Host time of a call: from the call to its result (synchronised).  Shapes: --shape a = 4 000 clips of 10-15 s at 44.1 kHz,
--shape b = 1 000 one-minute clips at 96 kHz.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3
tools/corpus_bench.py ...`.  Prints one JSON line.
    python3 tools/corpus_bench.py [--shape a|b] [--reps 10] [--warmup 2] [--out file.json]"""
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
    if a.shape == "a":
        ns = rng.integers(441_000, 661_500 + 1, 4000)
    else:
        ns = np.full(1000, 60 * 96_000)
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
    # the single-stream baseline: the encoder's frame table over the whole buffer, its sample offsets, and a segment index
    # recorded as the corpus records it -- every frame's samples at a multiple of four in a scratch of its own (the clips'
    # positions are not, and the recording decoder takes only such rows)
    ws32 = x3hip.WindowSource(ctx, (d_x3, pos), seg_blocks=0, frame_offsets=d_off, n_frames=F)
    assert ws32.total == total
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    d_idx, d_back, d_woff = ctx.alloc(8 * ne), ctx.alloc(2 * F * spf), ctx.alloc(8 * F)
    ctx.upload(d_woff, np.arange(F, dtype=np.uint64) * np.uint64(spf))
    x4 = ctx.get_option("wav_offsets_x4")
    ctx.set_option("wav_offsets_x4", 1)
    assert ctx.decode_dev_seg(d_x3, pos, d_off, F, p, d_back, F * spf, d_idx, 32, record=True, d_wav_offsets=d_woff) == 0
    assert ctx.decode_result()[0] == 0
    ctx.set_option("wav_offsets_x4", x4)
    ctx.free(d_back)
    L = rate
    K = (1, 256, 1024)
    row_len = (max(ns) + 3) // 4 * 4
    kmax = max(K)
    d_ent, d_st, d_gst = ctx.alloc(4 * kmax), ctx.alloc(8 * kmax), ctx.alloc(8 * kmax)
    d_out, d_status = ctx.alloc(2 * kmax * L), ctx.alloc(4 * kmax)
    d_rows = ctx.alloc(2 * n_clips * row_len)
    d_res = ctx.alloc(24 * n_clips)
    now = time.perf_counter

    def t_streams(idx):
        o = [offs[i] for i in idx]
        ln = [lens[i] for i in idx]
        t0 = now()
        assert ctx.decode_streams_dev(d_x3, pos, o, ln, p, d_rows, row_len, 0, d_res) == 0
        assert ctx.decode_streams_result()[0] == 0
        return now() - t0

    corpora, index_bytes, results = {}, {}, {}

    def add(name, v):
        results.setdefault(name, []).append(v * 1e3)

    for rep in range(a.warmup + a.reps):
        keep = rep >= a.warmup
        for sb in (32, 0):
            old = corpora.pop(sb, None)
            if old is not None:
                old.close()
            t0 = now()
            c = x3hip.Corpus(ctx, (d_x3, pos), offs, lens, seg_blocks=sb)
            dt = now() - t0
            if keep:
                add("build_%d" % sb, dt)
            corpora[sb] = c
            index_bytes[sb] = 8 * lib.x3_seg_index_entries(F, C.byref(p), sb) if c.seg_blocks else 0
        dt = t_streams(range(n_clips))
        if keep:
            add("streams_all", dt)
        for k in K:
            ents = rng.integers(0, n_clips, k).astype(np.uint32)
            st = np.array([int(rng.integers(0, ns[e] - L + 1)) for e in ents], dtype=np.uint64)
            gst = (base[ents] + st.astype(np.int64)).astype(np.uint64)
            ctx.upload(d_ent, ents)
            ctx.upload(d_st, st)
            ctx.upload(d_gst, gst)
            for sb in (32, 0):
                c = corpora[sb]
                t0 = now()
                assert c.decode_into(d_ent, d_st, k, L, d_out, 0, d_status) == 0
                r = ctx.decode_windows_result()
                dt = now() - t0
                assert r[:2] == (0, 0), r
                if keep:
                    add("corpus_%d_%d" % (k, sb), dt)
                t0 = now()
                assert ctx.decode_windows_dev(d_x3, pos, d_off, ws32.d_sample_offsets, F, p, d_gst, k, L, d_out, 0, d_status,
                                              d_idx if sb else None, sb) == 0
                r = ctx.decode_windows_result()
                dt = now() - t0
                assert r[:2] == (0, 0), r
                if keep:
                    add("single_%d_%d" % (k, sb), dt)
            dt = t_streams(sorted(set(int(e) for e in ents)))
            if keep:
                add("drawn_%d" % k, dt)
    out = {"shape": a.shape, "clips": n_clips, "frames": F, "samples": total, "bytes": pos, "window_len": L,
           "reps": a.reps, "index_bytes_32": index_bytes[32],
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for c in corpora.values():
        c.close()
    ws32.close()
    ctx.close()


if __name__ == "__main__":
    main()
