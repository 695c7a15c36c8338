#!/usr/bin/env python3
"""Per-entry adaptive thresholds in the chain levels -> thresholds -> adaptive events -> ranges, all on the device
(x3_level_thresholds_dev, x3_events_adaptive_dev and their corpus forms), against today's route -- levels, download the
records, per-entry quantiles in numpy, a vectorised detector with a threshold per entry, upload (entry,) start, len, ranges
-- in one process, the two alternating rep by rep; medians of --reps, host time from the first call to the last synchronised
result.  The cases are tools/events_bench.py's (its stream and corpus, its detector, its join / pad / piece rule):
  config3   691.2 M hydrophone samples, bins of 1920 positions: one entry of 360 000 records
  corpus_a  4 000 clips of 10-15 s at 44.1 kHz, bins of 441 positions: 4 000 entries of 1 000 - 1 500 records
The threshold of an entry is its peak at 99.8 % (rank floor((K - 1) * 0.998) of its counting bins) plus 1.  The device route
decodes `cap` ranges (the slots behind the events are zero-length), today's route exactly as many as it found; both sides'
thresholds, events and rows are compared with == at the end of every case, and the tool fails otherwise.  The quantiles call
alone is timed for 1 and 8 quantiles of both keys.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/thresholds_bench.py ...`.  Prints one JSON line.
    python3 tools/thresholds_bench.py [--samples N] [--reps 10] [--warmup 2] [--cap 4096] [--corpus-cap 16384]
                                      [--cases config3,corpus] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import x3hip
from events_bench import JOIN, MIN_BINS, PAD, MAX_BINS, detect

now = time.perf_counter
Q_PPM = 998_000
Q8 = [50_000, 100_000, 250_000, 500_000, 750_000, 900_000, 950_000, 998_000]


def entry_thresholds(lv, row_first):
    """per entry the key of rank (K - 1) * Q_PPM // 10^6 among the peaks of its counting rows, plus 1, at most 32768; 0 for an
    entry without one -> (thresholds per entry, K per entry)"""
    n_ent = row_first.size - 1
    ent = np.repeat(np.arange(n_ent), np.diff(row_first.astype(np.int64)))
    counts = lv["n"] != 0
    key = np.clip(np.maximum(lv["max"], -lv["min"]), 0, 32768)[counts]
    ent = ent[counts]
    order = np.lexsort((key, ent))
    k = np.bincount(ent, minlength=n_ent)
    first = np.cumsum(k) - k
    rank = (np.maximum(k, 1) - 1) * Q_PPM // 1_000_000
    value = key[order][np.minimum(first + rank, max(key.size - 1, 0))] if key.size else np.zeros(n_ent, np.int64)
    return np.where(k > 0, np.minimum(value + 1, 32768), 0), k


def bench(ctx, a, cap, name, results, info, bin_len, n_rows, row_first, n_samples, levels, thresholds, events, ranges, quantiles,
          with_entries):
    """levels(d_lv) / thresholds(d_lv, trule, d_thr) / events(d_lv, rule, d_thr, d_ent, d_st, d_ln, cap, d_cnt) /
    ranges(d_ent, d_st, d_ln, n, stride, d_out, out_cap, d_status) / quantiles(d_lv, key, q_ppm, d_val, d_k) enqueue the calls
    of the case"""
    stride, n_ent = MAX_BINS * bin_len, row_first.size - 1
    lv = torch.empty(4 * n_rows, dtype=torch.int64, device="cuda")
    thr = torch.empty(2 * n_ent, dtype=torch.int64, device="cuda")
    ent, st, ln = (torch.empty(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    ent2, st2, ln2 = (torch.empty(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    cnt = torch.zeros((), dtype=torch.int64, device="cuda")
    out, out2 = (torch.empty(cap * stride, dtype=torch.int16, device="cuda") for _ in range(2))
    status, status2 = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    val, kk = torch.empty(8 * n_ent, dtype=torch.int32, device="cuda"), torch.empty(n_ent, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    trule = x3hip.ThresholdRule.make(peak=(Q_PPM, 1, 1, 1))
    rule = x3hip.EventRule.make(0, 0, JOIN, MIN_BINS, PAD, MAX_BINS)
    rows_ent = np.repeat(np.arange(n_ent), np.diff(row_first.astype(np.int64)))
    for rep in range(a.warmup + a.reps):
        t0 = now()
        assert levels(lv.data_ptr()) == 0
        assert thresholds(lv.data_ptr(), trule, thr.data_ptr()) == 0
        assert events(lv.data_ptr(), rule, thr.data_ptr(), ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, cnt.data_ptr()) == 0
        assert ranges(ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, stride, out.data_ptr(), cap * stride, status.data_ptr()) == 0
        r = ctx.decode_ranges_result()
        t1 = now()
        assert r[:2] == (0, 0), r
        rc, found = ctx.events_result()
        assert rc == 0 and ctx.levels_result()[0] == 0 and ctx.level_quantiles_result()[0] == 0 and found <= cap, (rc, found)
        t2 = now()
        assert levels(lv.data_ptr()) == 0 and ctx.levels_result()[0] == 0
        rec = ctx.download(lv.data_ptr(), 32 * n_rows, x3hip.LEVEL_DTYPE)
        t3 = now()
        hthr, hk = entry_thresholds(rec, row_first)
        t4 = now()
        he, hs, hl = detect(rec, row_first, n_samples, bin_len, np.where(hthr > 0, hthr, 1 << 20)[rows_ent])
        t5 = now()
        n = hs.size
        assert 0 < n <= cap, n
        if with_entries:
            ctx.upload(ent2.data_ptr(), he)
        ctx.upload(st2.data_ptr(), hs)
        ctx.upload(ln2.data_ptr(), hl)
        assert ranges(ent2.data_ptr(), st2.data_ptr(), ln2.data_ptr(), n, stride, out2.data_ptr(), cap * stride, status2.data_ptr()) == 0
        r = ctx.decode_ranges_result()
        t6 = now()
        assert r[:2] == (0, 0), r
        if rep >= a.warmup:
            results.setdefault(name + "_device", []).append((t1 - t0) * 1e3)
            results.setdefault(name + "_host_route", []).append((t6 - t2) * 1e3)
            results.setdefault(name + "_host_route_levels_download", []).append((t3 - t2) * 1e3)
            results.setdefault(name + "_host_route_quantiles", []).append((t4 - t3) * 1e3)
            results.setdefault(name + "_host_route_detector", []).append((t5 - t4) * 1e3)
            results.setdefault(name + "_host_route_upload_ranges", []).append((t6 - t5) * 1e3)
    dthr = thr.cpu().numpy().view(x3hip.EVENT_THRESHOLD_DTYPE)
    same = (np.array_equal(dthr["peak_min"], hthr) and np.array_equal(dthr["counted"], hk) and not dthr["mean_sq_min"].any() and
            found == n and np.array_equal(st.cpu().numpy()[:n].view(np.uint64), hs) and
            np.array_equal(ln.cpu().numpy()[:n].view(np.uint32), hl) and not ln.cpu().numpy()[n:].any() and
            (not with_entries or np.array_equal(ent.cpu().numpy()[:n].view(np.uint32), he)) and
            torch.equal(out[:n * stride], out2[:n * stride]) and not status.cpu().numpy().any())
    if not same:
        raise SystemExit("%s: the two routes' thresholds, events or rows differ (found %d on the device, %d on the host)" % (name, found, n))
    # the quantiles call alone, from the call to its synchronised result; the levels are in lv
    for key, kname in ((x3hip.LEVEL_KEY_PEAK, "peak"), (x3hip.LEVEL_KEY_MEAN_SQ, "mean_sq")):
        for q_ppm in ([Q_PPM], Q8):
            for rep in range(a.warmup + a.reps):
                t0 = now()
                assert quantiles(lv.data_ptr(), key, q_ppm, val.data_ptr(), kk.data_ptr()) == 0
                assert ctx.level_quantiles_result()[0] == 0
                if rep >= a.warmup:
                    results.setdefault("%s_quantiles_%s_nq%d" % (name, kname, len(q_ppm)), []).append((now() - t0) * 1e3)
    info[name] = {"rows": int(n_rows), "entries": int(n_ent), "events": int(n), "cap": cap, "row_stride": int(stride),
                  "peak_min_lowest": int(hthr[hthr > 0].min()), "peak_min_highest": int(hthr.max()), "equal": bool(same)}


def config3(ctx, a, results, info):
    lib = x3hip.lib()
    n, p = a.samples, x3hip.Params.default()
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    x = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off, so = (torch.empty(F + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, x.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    del wav
    assert ctx.sample_offsets_dev(x.data_ptr(), pos, off.data_ptr(), F, so.data_ptr()) == 0
    ctx.sync()
    bin_len = 1920
    n_bins = -(-n // bin_len)
    d_total = so.data_ptr() + 8 * F
    bench(ctx, a, a.cap, "config3", results, info, bin_len, n_bins, np.array([0, n_bins]), [n],
          lambda d_lv: ctx.levels_dev(x.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, bin_len, d_lv, n_bins, None,
                                      idx.data_ptr(), 32),
          lambda d_lv, trule, d_thr: ctx.level_thresholds_dev(d_lv, n_bins, bin_len, d_total, trule, d_thr),
          lambda d_lv, rule, d_thr, d_e, d_s, d_l, c, d_c: ctx.events_adaptive_dev(d_lv, n_bins, bin_len, d_total, rule, d_thr, d_s,
                                                                                   d_l, None, c, d_c),
          lambda d_e, d_s, d_l, k, stride, d_out, oc, d_status: ctx.decode_ranges_dev(
              x.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, d_s, d_l, k, stride, d_out, oc, 0, None, d_status,
              idx.data_ptr(), 32),
          lambda d_lv, key, q_ppm, d_v, d_k: ctx.level_quantiles_dev(d_lv, n_bins, bin_len, d_total, key, q_ppm, d_v, d_k), False)
    torch.cuda.empty_cache()


def corpus_a(ctx, a, results, info):
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
    bin_len = 441
    rf = corpus.levels_rows(bin_len)
    n_rows = int(rf[-1])
    bench(ctx, a, a.corpus_cap, "corpus_a", results, info, bin_len, n_rows, rf, ns,
          lambda d_lv: ctx.corpus_levels_dev(corpus, bin_len, d_lv, n_rows),
          lambda d_lv, trule, d_thr: corpus.level_thresholds_into(d_lv, n_rows, bin_len, trule, d_thr),
          lambda d_lv, rule, d_thr, d_e, d_s, d_l, c, d_c: corpus.adaptive_events_into(d_lv, n_rows, bin_len, rule, d_thr, d_e, d_s,
                                                                                       d_l, None, c, d_c),
          lambda d_e, d_s, d_l, k, stride, d_out, oc, d_status: corpus.ranges_into(d_e, d_s, d_l, k, stride, d_out, oc, 0, None,
                                                                                 d_status),
          lambda d_lv, key, q_ppm, d_v, d_k: corpus.level_quantiles_into(d_lv, n_rows, bin_len, key, q_ppm, d_v, d_k), True)
    corpus.close()
    for q in (d_x3, d_off):
        ctx.free(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--corpus-cap", type=int, default=16384)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, info = {}, {}
    if "config3" in a.cases:
        config3(ctx, a, results, info)
    if "corpus" in a.cases:
        corpus_a(ctx, a, results, info)
    out = {"samples": a.samples, "reps": a.reps, "q_ppm": Q_PPM, "cases": info,
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
