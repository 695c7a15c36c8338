#!/usr/bin/env python3
"""The segment index by a walk (x3_seg_index_build_dev) against the two ways there were before it, in one process, the
cases alternating rep by rep.  Host time of a call: from the call to its result (synchronised).  Prints one JSON line.

--case stream   one stream of --samples hydrophone samples at the default parameters (default: BASELINE config 3):
  walk_<sb>       x3_seg_index_build_dev + x3_ctx_sync
  record_<sb>     x3_decode_dev_seg(record = 1) + x3_decode_result -- the only way to index a foreign stream before; its
                  output buffer (2 bytes a sample) is reported as sample_buffer_bytes, the walk needs none
--case corpus   tools/corpus_bench.py's corpora (--shape a | b) encoded at --block-len 20 or 40:
  build_walk / build_record / build_none    x3_corpus_build with X3_CORPUS_INDEX_WALK, without it, with seg_blocks 0
  index_walk      x3_seg_index_build_dev alone over the corpus's frame table (the build's step 3)
  streams_all     x3_decode_streams_dev int16 of every clip (the build's yardstick)
  windows_<k>_walk / windows_<k>_none       k random one-second windows by the walk-built index / without an index
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3 tools/segindex_bench.py ...`.
    python3 tools/segindex_bench.py --case stream|corpus [--shape a|b] [--block-len 20|40] [--reps 10] [--warmup 2] [--out f]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import x3hip

now = time.perf_counter


def summary(results):
    return {"ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
            "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}


def case_stream(a, ctx, lib):
    p = x3hip.Params.default()
    n = a.samples
    F = lib.x3_num_frames(n, C.byref(p))
    cap = lib.x3_encode_bound(n, C.byref(p))
    d_wav, d_x3, d_off = ctx.alloc(2 * n), ctx.alloc(cap + 16), ctx.alloc(8 * (F + 1))
    ctx.synth_dev(x3hip.SYNTH_HYDROPHONE, 0x58330001, 0, n, d_wav)
    assert ctx.encode_dev(d_wav, n, p, d_x3, cap, 0, d_off) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    results, words = {}, {}
    idx = {sb: (ctx.alloc(8 * lib.x3_seg_index_entries(F, C.byref(p), sb)), ctx.alloc(8 * lib.x3_seg_index_entries(F, C.byref(p), sb)))
           for sb in (32, 64)}
    for rep in range(a.warmup + a.reps):
        for sb, (d_walk, d_rec) in idx.items():
            t0 = now()
            assert ctx.seg_index_build_dev(d_x3, pos, d_off, F, p, d_walk, sb) == 0
            ctx.sync()
            t1 = now()
            assert ctx.decode_dev_seg(d_x3, pos, d_off, F, p, d_wav, n, d_rec, sb, record=True, n_per_clip=n) == 0
            assert ctx.decode_result()[:2] == (0, F)
            t2 = now()
            if rep >= a.warmup:
                results.setdefault("walk_%d" % sb, []).append((t1 - t0) * 1e3)
                results.setdefault("record_%d" % sb, []).append((t2 - t1) * 1e3)
    for sb, (d_walk, d_rec) in idx.items():
        ne = lib.x3_seg_index_entries(F, C.byref(p), sb)
        assert np.array_equal(ctx.download(d_walk, 8 * ne, np.uint64), ctx.download(d_rec, 8 * ne, np.uint64))
        words[sb] = ne
    assert ctx.get_option("last_seg_index_irregular") == 0
    out = {"case": "stream", "samples": n, "frames": F, "bytes": pos, "reps": a.reps, "sample_buffer_bytes": 2 * n,
           "index_bytes": {str(sb): 8 * w for sb, w in words.items()}}
    out.update(summary(results))
    return out


def case_corpus(a, ctx, lib):
    rng = np.random.default_rng(7)
    rate = 44_100 if a.shape == "a" else 96_000
    ns = [int(v) for v in (rng.integers(441_000, 661_500 + 1, 4000) if a.shape == "a" else np.full(1000, 60 * 96_000))]
    n_clips, total = len(ns), int(sum(ns))
    p = x3hip.Params.make(a.block_len, 10_000 // a.block_len)
    spf = p.block_len * p.blocks_per_frame
    so, sn, first = [], [], []
    pos_s = 0
    for n in ns:
        first.append(len(so))
        for s in range(0, n, spf):
            so.append(pos_s + s)
            sn.append(min(spf, n - s))
        pos_s += n
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
    L, K = rate, (1, 256, 1024)
    row_len = (max(ns) + 3) // 4 * 4
    d_ent, d_st = ctx.alloc(4 * max(K)), ctx.alloc(8 * max(K))
    d_out, d_status = ctx.alloc(2 * max(K) * L), ctx.alloc(4 * max(K))
    d_rows, d_res = ctx.alloc(2 * n_clips * row_len), ctx.alloc(24 * n_clips)
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    d_idx = ctx.alloc(8 * ne)
    results, corpora, in_use = {}, {}, {}
    kinds = {"walk": dict(seg_blocks=32, index="walk"), "record": dict(seg_blocks=32), "none": dict(seg_blocks=0)}
    for rep in range(a.warmup + a.reps):
        keep = rep >= a.warmup

        def add(name, dt):
            if keep:
                results.setdefault(name, []).append(dt * 1e3)
        for kind, kw in kinds.items():
            old = corpora.pop(kind, None)
            if old is not None:
                old.close()
            t0 = now()
            corpora[kind] = x3hip.Corpus(ctx, (d_x3, pos), offs, lens, params=p, **kw)
            add("build_" + kind, now() - t0)
            in_use[kind] = corpora[kind].seg_blocks
        fr = corpora["walk"]
        t0 = now()
        assert ctx.seg_index_build_dev(d_x3, pos, d_off, F, p, d_idx, 32) == 0
        ctx.sync()
        add("index_walk", now() - t0)
        t0 = now()
        assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, d_rows, row_len, 0, d_res) == 0
        assert ctx.decode_streams_result()[0] == 0
        add("streams_all", now() - t0)
        for k in K:
            ents = rng.integers(0, n_clips, k).astype(np.uint32)
            st = np.array([int(rng.integers(0, ns[e] - L + 1)) for e in ents], dtype=np.uint64)
            ctx.upload(d_ent, ents)
            ctx.upload(d_st, st)
            for kind in ("walk", "none"):
                t0 = now()
                assert corpora[kind].decode_into(d_ent, d_st, k, L, d_out, 0, d_status) == 0
                r = ctx.decode_windows_result()
                add("windows_%d_%s" % (k, kind), now() - t0)
                assert r[:2] == (0, 0), r
                if kind == "walk":
                    assert ctx.get_option("last_window_replays") == 0
        assert fr.n_frames == F
    out = {"case": "corpus", "shape": a.shape, "block_len": a.block_len, "clips": n_clips, "frames": F, "samples": total,
           "bytes": pos, "window_len": L, "reps": a.reps, "index_bytes_32": 8 * ne, "seg_blocks_in_use": in_use}
    out.update(summary(results))
    for c in corpora.values():
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("stream", "corpus"), default="stream")
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--shape", choices=("a", "b"), default="a")
    ap.add_argument("--block-len", type=int, choices=(20, 40), default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = x3hip.Context(0)
    out = (case_stream if a.case == "stream" else case_corpus)(a, ctx, x3hip.lib())
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
