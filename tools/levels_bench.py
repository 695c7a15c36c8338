#!/usr/bin/env python3
"""Levels (x3_levels_dev / x3_corpus_levels_dev) against the status quo, decode into a sample buffer and reduce it, in one
process, the two alternating rep by rep; medians of --reps, host time from the call to the synchronised result.
  config3_<bl>_<bin>   the stream kbench.py makes (691.2 M hydrophone samples), bin_len 1920 (10 ms at 192 kHz) and 0:
                       block length 20 with the encoder's segment index, block length 40 with a walk-built one
                       (x3_seg_index_build_dev); status quo: x3_decode_dev_seg (20) / x3_decode_dev (40) + torch reductions
  corpus_a_0           tools/corpus_bench.py's corpus (a): 4 000 clips of 10-15 s at 44.1 kHz, one record per clip;
                       status quo: x3_decode_streams_dev into padded rows + torch reductions over the rows
The torch reductions are the same five quantities (min, max, sum, sum of squares in int64; the count is known).  Device
memory of each side: the levels workspace and records, against the sample buffer plus torch's peak.  Kernel times: run it
under `rocprofv3 --kernel-trace --stats -- python3 tools/levels_bench.py ...`.  Prints one JSON line.
    python3 tools/levels_bench.py [--samples N] [--reps 10] [--warmup 2] [--cases config3,corpus] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip

now = time.perf_counter


def reduce_flat(x, bin_len):
    """the five reductions of a decoded buffer (int16 tensor), per bin of bin_len samples or over everything"""
    if bin_len:
        r = x[: x.numel() // bin_len * bin_len].view(-1, bin_len)
        w = r.to(torch.int32)
        out = (r.min(1).values, r.max(1).values, w.sum(1, dtype=torch.int64), (w * w).sum(1, dtype=torch.int64))
    else:
        w = x.to(torch.int32)
        out = (x.min(), x.max(), w.sum(dtype=torch.int64), (w * w).sum(dtype=torch.int64))
    torch.cuda.synchronize()
    return out


def config3(ctx, a, results, mem, checks):
    lib = x3hip.lib()
    n = a.samples
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    back = torch.empty(n, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    for bl, bpf in ((20, 500), (40, 250)):
        p = x3hip.Params.make(bl, bpf)
        F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
        ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
        out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
        off = torch.empty(F + 1, dtype=torch.int64, device="cuda")
        so = torch.empty(F + 1, dtype=torch.int64, device="cuda")
        idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
        if bl == 20:
            assert ctx.encode_dev_seg(wav.data_ptr(), n, p, out.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
        else:
            assert ctx.encode_dev(wav.data_ptr(), n, p, out.data_ptr(), cap, 0, off.data_ptr()) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        if bl != 20:
            assert ctx.seg_index_build_dev(out.data_ptr(), pos, off.data_ptr(), F, p, idx.data_ptr(), 32) == 0
        assert ctx.sample_offsets_dev(out.data_ptr(), pos, off.data_ptr(), F, so.data_ptr()) == 0
        ctx.sync()
        for bin_len in (1920, 0):
            n_bins = -(-n // bin_len) if bin_len else 1
            lv = torch.empty(4 * n_bins, dtype=torch.int64, device="cuda")
            name = "config3_%d_%d" % (bl, bin_len)
            for rep in range(a.warmup + a.reps):
                t0 = now()
                assert ctx.levels_dev(out.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, bin_len, lv.data_ptr(), n_bins,
                                      None, idx.data_ptr(), 32) == 0
                r = ctx.levels_result()
                t1 = now()
                assert r[:2] == (0, 0), r
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t2 = now()
                if bl == 20:
                    assert ctx.decode_dev_seg(out.data_ptr(), pos, off.data_ptr(), F, p, back.data_ptr(), n, idx.data_ptr(), 32,
                                              n_per_clip=n) == 0
                else:
                    assert ctx.decode_dev(out.data_ptr(), pos, off.data_ptr(), F, p, back.data_ptr(), n, n_per_clip=n) == 0
                assert ctx.decode_result()[0] == 0
                red = reduce_flat(back, bin_len)
                t3 = now()
                if rep >= a.warmup:
                    results.setdefault(name + "_levels", []).append((t1 - t0) * 1e3)
                    results.setdefault(name + "_decode_reduce", []).append((t3 - t2) * 1e3)
                peak = torch.cuda.max_memory_allocated() - base
            assert ctx.get_option("last_levels_replays") == 0
            rec = lv.cpu().numpy().view(x3hip.LEVEL_DTYPE)
            full = n // bin_len if bin_len else 1      # (the bins the torch side reduces: the whole ones)
            checks[name] = bool(np.array_equal(rec["min"][:full], np.atleast_1d(red[0].cpu().numpy())) and
                                np.array_equal(rec["max"][:full], np.atleast_1d(red[1].cpu().numpy())) and
                                np.array_equal(rec["sum"][:full], np.atleast_1d(red[2].cpu().numpy())) and
                                np.array_equal(rec["sum_sq"][:full].astype(np.int64), np.atleast_1d(red[3].cpu().numpy())))
            mem[name] = {"levels_bytes": 32 * n_bins + 32 * (n_bins + F) + 48 * F, "decode_reduce_bytes": 2 * n + int(peak),
                         "stream_bytes": int(pos), "frames": int(F)}
            del lv, red
        del out, off, so, idx
    del wav, back
    torch.cuda.empty_cache()


def corpus_a(ctx, a, results, mem, checks):
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
    rf = corpus.levels_rows(0)
    n_rows = int(rf[-1])
    lv = torch.empty(4 * n_rows, dtype=torch.int64, device="cuda")
    row_len = (max(ns) + 3) // 4 * 4
    rows = torch.empty(n_clips * row_len, dtype=torch.int16, device="cuda")
    res = torch.empty(24 * n_clips, dtype=torch.uint8, device="cuda")
    t_ns = torch.tensor(ns, device="cuda").view(-1, 1)
    col = torch.arange(row_len, device="cuda").view(1, -1)
    for rep in range(a.warmup + a.reps):
        t0 = now()
        assert ctx.corpus_levels_dev(corpus, 0, lv.data_ptr(), n_rows) == 0
        r = ctx.levels_result()
        t1 = now()
        assert r[:2] == (0, 0), r
        torch.cuda.reset_peak_memory_stats()
        base_mem = torch.cuda.memory_allocated()
        t2 = now()
        assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, rows.data_ptr(), row_len, 0, res.data_ptr()) == 0
        assert ctx.decode_streams_result()[0] == 0
        x = rows.view(n_clips, row_len)
        inside = col < t_ns                      # (rows are padded with zeros: they count for the sums, not for min / max)
        mn = torch.where(inside, x, torch.full_like(x, 32767)).min(1).values
        mx = torch.where(inside, x, torch.full_like(x, -32768)).max(1).values
        w = x.to(torch.int32)
        sm, sq = w.sum(1, dtype=torch.int64), (w * w).sum(1, dtype=torch.int64)
        torch.cuda.synchronize()
        t3 = now()
        if rep >= a.warmup:
            results.setdefault("corpus_a_0_levels", []).append((t1 - t0) * 1e3)
            results.setdefault("corpus_a_0_decode_reduce", []).append((t3 - t2) * 1e3)
        peak = torch.cuda.max_memory_allocated() - base_mem
    rec = lv.cpu().numpy().view(x3hip.LEVEL_DTYPE)
    checks["corpus_a_0"] = bool(np.array_equal(rec["min"], mn.cpu().numpy()) and np.array_equal(rec["max"], mx.cpu().numpy()) and
                                np.array_equal(rec["sum"], sm.cpu().numpy()) and
                                np.array_equal(rec["sum_sq"].astype(np.int64), sq.cpu().numpy()) and
                                np.array_equal(rec["n"], np.array(ns, dtype=np.uint32)))
    mem["corpus_a_0"] = {"levels_bytes": 32 * n_rows + 32 * (n_rows + F) + 48 * F + 8 * (n_clips + 1),
                         "decode_reduce_bytes": 2 * n_clips * row_len + int(peak), "stream_bytes": int(pos), "frames": int(F),
                         "clips": n_clips, "samples": total}
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, mem, checks = {}, {}, {}
    if "config3" in a.cases:
        config3(ctx, a, results, mem, checks)
    if "corpus" in a.cases:
        corpus_a(ctx, a, results, mem, checks)
    out = {"samples": a.samples, "reps": a.reps, "equal_to_torch": checks, "memory": mem,
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
