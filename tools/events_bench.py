#!/usr/bin/env python3
"""Events (x3_events_dev / x3_corpus_events_dev) in the chain levels -> events -> ranges, all on the device, against today's
route -- levels, download the records, a numpy detector, upload (entry,) start, len, ranges -- in one process, the two
alternating rep by rep; medians of --reps, host time from the first call to the last synchronised result.
  config3   the stream kbench.py makes (691.2 M hydrophone samples, block length 20, the encoder's index), bins of 1920
            positions (10 ms at 192 kHz): 360 000 records
  corpus_a  tools/corpus_bench.py's corpus (a): 4 000 clips of 10-15 s at 44.1 kHz, bins of 441 positions (10 ms)
One rule each: a peak threshold at a high percentile of the bins' peaks (99.8, or what keeps the hot bins below a quarter of
--cap; taken from a first levels call, outside the timing), join 5 bins, 2 bins of padding, pieces of 25 bins.  The device route decodes `--cap` ranges
(the slots behind the events are zero-length), today's route exactly as many as it found.  The numpy detector is the
vectorised one a user writes (tests/events_ref.py is the same definition as a serial loop: minutes at this size); both
sides' events, and the rows of the events, are compared with == at the end of every case.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/events_bench.py ...`.  Prints one JSON line.
    python3 tools/events_bench.py [--samples N] [--reps 10] [--warmup 2] [--cap 4096] [--cases config3,corpus] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip

now = time.perf_counter
JOIN, MIN_BINS, PAD, MAX_BINS = 5, 1, 2, 25


def detect(lv, row_first, n_samples, bin_len, peak_min):
    """the events of level records (np, LEVEL_DTYPE) whose entries' rows are [row_first[e], row_first[e + 1]) -> entries,
    starts, lens: the definition of include/x3hip.h ("EVENTS") for a peak rule, vectorised"""
    hot = np.flatnonzero((lv["n"] != 0) & (np.maximum(lv["max"], -lv["min"]) >= peak_min)).astype(np.int64)
    if hot.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    rf = row_first.astype(np.int64)
    ent = np.searchsorted(rf, hot, side="right") - 1
    new = np.ones(hot.size, dtype=bool)
    new[1:] = (hot[1:] - hot[:-1] - 1 > JOIN) | (ent[1:] != ent[:-1])
    first, e = hot[new], ent[new]
    last = hot[np.append(np.flatnonzero(new)[1:] - 1, hot.size - 1)]
    keep = last - first + 1 >= MIN_BINS
    first, last, e = first[keep], last[keep], e[keep]
    b0, b1 = np.maximum(first - PAD, rf[e]), np.minimum(last + 1 + PAD, rf[e + 1])
    pieces = -(-(b1 - b0) // MAX_BINS)
    run = np.repeat(np.arange(first.size), pieces)
    j = np.arange(run.size) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    p0 = b0[run] + j * MAX_BINS
    p1 = np.minimum(p0 + MAX_BINS, b1[run])
    lo, ns = rf[e[run]], np.asarray(n_samples, dtype=np.int64)[e[run]]
    start = (p0 - lo) * bin_len
    return e[run].astype(np.uint32), start.astype(np.uint64), (np.minimum((p1 - lo) * bin_len, ns) - start).astype(np.uint32)


def bench(ctx, a, name, results, info, bin_len, n_rows, row_first, n_samples, levels, events, ranges, with_entries):
    """levels(d_lv) / events(d_lv, rule, d_ent, d_st, d_ln, cap, d_cnt) / ranges(d_ent, d_st, d_ln, n, stride, d_out, out_cap,
    d_status) enqueue the three calls of the case"""
    cap, stride = a.cap, MAX_BINS * bin_len
    lv = torch.empty(4 * n_rows, dtype=torch.int64, device="cuda")
    ent, st, ln = (torch.empty(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    ent2, st2, ln2 = (torch.empty(cap, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
    cnt = torch.zeros((), dtype=torch.int64, device="cuda")
    out, out2 = (torch.empty(cap * stride, dtype=torch.int16, device="cuda") for _ in range(2))
    status, status2 = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    assert levels(lv.data_ptr()) == 0 and ctx.levels_result()[0] == 0
    rec = lv.cpu().numpy().view(x3hip.LEVEL_DTYPE)
    q = 100.0 * (1.0 - min(0.002, cap / (4.0 * n_rows)))
    peak_min = int(min(max(np.percentile(np.maximum(rec["max"], -rec["min"])[rec["n"] != 0], q) + 1, 1), 32768))
    rule = x3hip.EventRule.make(0, peak_min, JOIN, MIN_BINS, PAD, MAX_BINS)
    for rep in range(a.warmup + a.reps):
        t0 = now()
        assert levels(lv.data_ptr()) == 0
        assert events(lv.data_ptr(), rule, ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, cnt.data_ptr()) == 0
        assert ranges(ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, stride, out.data_ptr(), cap * stride, status.data_ptr()) == 0
        r = ctx.decode_ranges_result()
        t1 = now()
        assert r[:2] == (0, 0), r
        rc, found = ctx.events_result()
        assert rc == 0 and ctx.levels_result()[0] == 0 and found <= cap, (rc, found)
        t2 = now()
        assert levels(lv.data_ptr()) == 0 and ctx.levels_result()[0] == 0
        rec = ctx.download(lv.data_ptr(), 32 * n_rows, x3hip.LEVEL_DTYPE)
        t3 = now()
        he, hs, hl = detect(rec, row_first, n_samples, bin_len, peak_min)
        t4 = now()
        n = hs.size
        assert 0 < n <= cap
        if with_entries:
            ctx.upload(ent2.data_ptr(), he)
        ctx.upload(st2.data_ptr(), hs)
        ctx.upload(ln2.data_ptr(), hl)
        assert ranges(ent2.data_ptr(), st2.data_ptr(), ln2.data_ptr(), n, stride, out2.data_ptr(), cap * stride, status2.data_ptr()) == 0
        r = ctx.decode_ranges_result()
        t5 = now()
        assert r[:2] == (0, 0), r
        if rep >= a.warmup:
            results.setdefault(name + "_device", []).append((t1 - t0) * 1e3)
            results.setdefault(name + "_host_route", []).append((t5 - t2) * 1e3)
            results.setdefault(name + "_host_route_levels_download", []).append((t3 - t2) * 1e3)
            results.setdefault(name + "_host_route_detector", []).append((t4 - t3) * 1e3)
            results.setdefault(name + "_host_route_upload_ranges", []).append((t5 - t4) * 1e3)
    same = (found == n and np.array_equal(st.cpu().numpy()[:n].view(np.uint64), hs) and
            np.array_equal(ln.cpu().numpy()[:n].view(np.uint32), hl) and not ln.cpu().numpy()[n:].any() and
            (not with_entries or np.array_equal(ent.cpu().numpy()[:n].view(np.uint32), he)) and
            torch.equal(out[:n * stride], out2[:n * stride]) and not status.cpu().numpy().any())
    if not same:
        raise SystemExit("%s: the two routes' events or rows differ (found %d on the device, %d on the host)" % (name, found, n))
    info[name] = {"rows": int(n_rows), "events": int(n), "peak_min": peak_min, "cap": cap, "row_stride": int(stride),
                  "equal": bool(same)}


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
    bench(ctx, a, "config3", results, info, bin_len, n_bins, np.array([0, n_bins]), [n],
          lambda d_lv: ctx.levels_dev(x.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, bin_len, d_lv, n_bins, None,
                                      idx.data_ptr(), 32),
          lambda d_lv, rule, d_e, d_s, d_l, c, d_c: ctx.events_dev(d_lv, n_bins, bin_len, so.data_ptr() + 8 * F, rule, d_s, d_l,
                                                                  None, c, d_c),
          lambda d_e, d_s, d_l, k, stride, d_out, oc, d_status: ctx.decode_ranges_dev(
              x.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p, d_s, d_l, k, stride, d_out, oc, 0, None, d_status,
              idx.data_ptr(), 32), False)
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
    bench(ctx, a, "corpus_a", results, info, bin_len, n_rows, rf, ns,
          lambda d_lv: ctx.corpus_levels_dev(corpus, bin_len, d_lv, n_rows),
          lambda d_lv, rule, d_e, d_s, d_l, c, d_c: corpus.events_into(d_lv, n_rows, bin_len, rule, d_e, d_s, d_l, None, c, d_c),
          lambda d_e, d_s, d_l, k, stride, d_out, oc, d_status: corpus.ranges_into(d_e, d_s, d_l, k, stride, d_out, oc, 0, None,
                                                                                 d_status), True)
    corpus.close()
    for q in (d_x3, d_off):
        ctx.free(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=4096)
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
    out = {"samples": a.samples, "reps": a.reps, "cases": info,
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
