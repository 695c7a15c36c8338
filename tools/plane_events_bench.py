#!/usr/bin/env python3
"""Plane events (x3_plane_events_dev / x3_corpus_plane_events_dev) in the chain tone bank levels -> plane events -> tone bank
range levels, on --planes K band planes, three routes in one process, the sides alternating rep by rep (the order of the
routes is reversed in every other rep); medians of --reps (at least 7), host time from the first call to the last
synchronised result.
  (a) device      bank levels with the adapter, plane events, bank range levels of `--cap` padded ranges: no host trip
  (b) host route  today's: bank levels, their result, download of the K planes, a vectorised numpy detector over planes,
                  upload of (entry,) start, len, bank range levels of exactly the ranges found
  (c) K calls     bank levels, then K x3_events_dev / x3_corpus_events_dev calls, one per plane.  FOR TIME ONLY: K unrelated
                  lists do NOT compute what (a) and (b) compute -- no union in front of the runs, no "k of K", no one list
(a) and (b) are compared with == at the end of every case -- count, entries, starts, lens, masks, and every record of every
plane of the events' range-levels rows -- or the tool fails.
  config3   the stream kbench.py makes (691.2 M hydrophone samples, block length 20, the encoder's index), bins of 1920
  corpus_a  tools/corpus_bench.py's corpus (a): 4 000 clips of 10-15 s at 44.1 kHz, bins of 441 positions
The bank is K tones spread over the band; the rule is mean_sq_min per plane at a high percentile of that plane's band mean
squares (taken from a first levels call outside the timing, so that the hot rows stay below a quarter of --cap),
min_planes = --min-planes, join 5 bins, 2 bins of padding, pieces of 25 bins; the range levels are at bin_len / 8.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3 tools/plane_events_bench.py ...`; with --single the
device route also runs x3_events_dev on plane 0 once per rep, so that the one-plane instance x3_events_flag_kernel<false, 1>
and x3_events_emit_kernel stand in the same trace as the yardstick.  Prints one JSON line.
    python3 tools/plane_events_bench.py [--planes 4] [--min-planes 1] [--samples N] [--reps 9] [--warmup 2] [--cap 4096]
                                        [--cases config3,corpus] [--single] [--only-device] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip

now = time.perf_counter
JOIN, MIN_BINS, PAD, MAX_BINS, FINER = 5, 1, 2, 25, 8


def detect(planes, row_first, n_samples, bin_len, mean_sq_min, min_planes):
    """the plane events of K planes of level records (np, LEVEL_DTYPE [K, rows]) whose entries' rows are [row_first[e],
    row_first[e + 1]) -> entries, starts, lens, masks: include/x3hip.h ("PLANE EVENTS") for mean-square rules, vectorised"""
    loud = np.stack([(p["n"] != 0) & (p["sum_sq"] >= np.uint64(m) * p["n"].astype(np.uint64)) for p, m in zip(planes, mean_sq_min)])
    hot = np.flatnonzero(loud.sum(axis=0) >= min_planes).astype(np.int64)
    if hot.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
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
    mask = np.zeros(run.size, dtype=np.uint32)
    for t in range(loud.shape[0]):          # bit t: plane t is loud in some row of [p0, p1)
        c = np.concatenate([[0], np.cumsum(loud[t])])
        mask |= ((c[p1] - c[p0]) > 0).astype(np.uint32) << np.uint32(t)
    return e[run].astype(np.uint32), start.astype(np.uint64), (np.minimum((p1 - lo) * bin_len, ns) - start).astype(np.uint32), mask


def bench(ctx, a, name, results, info, src, tones, bin_len, n_rows, row_first, n_samples, with_entries):
    """src: a WindowSource or a Corpus; both have tone_bank_levels_into, plane_events_into, events_into and
    tone_bank_range_levels_into, the Corpus's with d_entries"""
    K, cap, rbin = len(tones), a.cap, max(bin_len // FINER, 1)
    stride = -(-MAX_BINS * bin_len // rbin)
    dev = lambda n, dt: torch.empty(n, dtype=dt, device="cuda")
    lv = dev(4 * K * n_rows, torch.int64)
    ent, st, ln, mk = dev(cap, torch.int32), dev(cap, torch.int64), dev(cap, torch.int32), dev(cap, torch.int32)
    ent2, st2, ln2 = dev(cap, torch.int32), dev(cap, torch.int64), dev(cap, torch.int32)
    cnt = torch.zeros((), dtype=torch.int64, device="cuda")
    rows, rows2 = dev(4 * K * cap * stride, torch.int64), dev(4 * K * cap * stride, torch.int64)
    status, status2 = dev(cap, torch.int32), dev(cap, torch.int32)
    torch.cuda.synchronize()
    e_arg = lambda d_e: (d_e,) if with_entries else ()

    def levels():
        return src.tone_bank_levels_into(bin_len, tones, lv.data_ptr(), n_rows, band=True)

    def range_levels(d_e, d_s, d_l, n, d_rows, d_status):
        return src.tone_bank_range_levels_into(*e_arg(d_e), d_s, d_l, n, rbin, stride, d_rows, cap * stride, None, d_status, tones)

    assert levels() == 0 and ctx.levels_result()[0] == 0
    rec = ctx.download(lv.data_ptr(), 32 * K * n_rows, x3hip.LEVEL_DTYPE).reshape(K, n_rows)
    q = 100.0 * (1.0 - min(0.002, cap / (4.0 * n_rows * K)))
    ms = []
    for t in range(K):
        keys = (rec[t]["sum_sq"] // np.maximum(rec[t]["n"], 1))[rec[t]["n"] != 0]
        ms.append(int(min(max(np.percentile(keys, q) + 1, 1), 1 << 30)))
    rule = x3hip.PlaneEventRule.make(ms, None, a.min_planes, JOIN, MIN_BINS, PAD, MAX_BINS)
    one = x3hip.EventRule.make(ms[0], 0, JOIN, MIN_BINS, PAD, MAX_BINS)
    found = n = 0
    he = hs = hl = hm = None

    def route_a():
        nonlocal found
        t0 = now()
        assert levels() == 0
        assert src.plane_events_into(lv.data_ptr(), n_rows, n_rows, bin_len, rule, None, *e_arg(ent.data_ptr()), st.data_ptr(),
                                     ln.data_ptr(), mk.data_ptr(), None, cap, cnt.data_ptr()) == 0
        assert range_levels(ent.data_ptr(), st.data_ptr(), ln.data_ptr(), cap, rows.data_ptr(), status.data_ptr()) == 0
        r = ctx.range_levels_result()
        ctx.sync()                        # (the adapter-free tone records are final behind the result; nothing else is pending)
        t1 = now()
        assert r[:2] == (0, 0), r
        rc, found = ctx.events_result()
        assert rc == 0 and ctx.levels_result()[0] == 0 and found <= cap, (rc, found)
        if a.single:                      # the yardstick kernels in the same trace; outside the timing
            assert src.events_into(lv.data_ptr(), n_rows, bin_len, one, *e_arg(ent2.data_ptr()), st2.data_ptr(), ln2.data_ptr(),
                                   rows2.data_ptr(), cap, cnt.data_ptr()) == 0
            assert ctx.events_result()[0] == 0
        return {"device": t1 - t0}

    def route_b():
        nonlocal n, he, hs, hl, hm
        t2 = now()
        assert levels() == 0 and ctx.levels_result()[0] == 0
        rec = ctx.download(lv.data_ptr(), 32 * K * n_rows, x3hip.LEVEL_DTYPE).reshape(K, n_rows)
        t3 = now()
        he, hs, hl, hm = detect(rec, row_first, n_samples, bin_len, ms, a.min_planes)
        t4 = now()
        n = hs.size
        assert 0 < n <= cap, n
        if with_entries:
            ctx.upload(ent2.data_ptr(), he)
        ctx.upload(st2.data_ptr(), hs)
        ctx.upload(ln2.data_ptr(), hl)
        assert range_levels(ent2.data_ptr(), st2.data_ptr(), ln2.data_ptr(), n, rows2.data_ptr(), status2.data_ptr()) == 0
        r = ctx.range_levels_result()
        ctx.sync()
        t5 = now()
        assert r[:2] == (0, 0), r
        return {"host_route": t5 - t2, "host_route_levels_download": t3 - t2, "host_route_detector": t4 - t3,
                "host_route_upload_range_levels": t5 - t4}

    def route_c():
        t6 = now()
        assert levels() == 0
        for t in range(K):
            r1 = x3hip.EventRule.make(ms[t], 0, JOIN, MIN_BINS, PAD, MAX_BINS)
            assert src.events_into(lv.data_ptr() + 32 * t * n_rows, n_rows, bin_len, r1, *e_arg(ent2.data_ptr()), st2.data_ptr(),
                                   ln2.data_ptr(), None, cap, cnt.data_ptr()) == 0
        rc = ctx.events_result()[0]
        t7 = now()
        assert rc == 0 and ctx.levels_result()[0] == 0
        return {"k_events_calls_not_equivalent": t7 - t6}

    routes = [route_a] if a.only_device else [route_a, route_b, route_c]
    for rep in range(a.warmup + a.reps):
        for route in (routes if rep % 2 == 0 else routes[::-1]):
            for k, v in route().items():
                if rep >= a.warmup:
                    results.setdefault(name + "_" + k, []).append(v * 1e3)
    if a.only_device:
        info[name] = {"rows": int(n_rows), "planes": K, "events": int(found), "cap": cap}
        return
    # (a) against (b): the events, the masks, and the events' rows in every plane
    assert route_a() and route_b()
    rows_a = rows.view(K, cap * stride, 4)[:, :n * stride]
    rows_b = rows2.view(K, cap * stride, 4)[:, :n * stride]
    same = (found == n and np.array_equal(st.cpu().numpy()[:n].view(np.uint64), hs) and
            np.array_equal(ln.cpu().numpy()[:n].view(np.uint32), hl) and not ln.cpu().numpy()[n:].any() and
            np.array_equal(mk.cpu().numpy()[:n].view(np.uint32), hm) and not mk.cpu().numpy()[n:].any() and
            (not with_entries or np.array_equal(ent.cpu().numpy()[:n].view(np.uint32), he)) and
            torch.equal(rows_a, rows_b) and not status.cpu().numpy().any())
    if not same:
        raise SystemExit("%s: routes (a) and (b) differ in events, masks or rows (found %d on the device, %d on the host)"
                         % (name, found, n))
    info[name] = {"rows": int(n_rows), "planes": K, "min_planes": a.min_planes, "events": int(n), "mean_sq_min": ms, "cap": cap,
                  "masks_seen": sorted(set(int(v) for v in hm)), "range_bin": int(rbin), "row_stride": int(stride),
                  "equal": bool(same)}


def config3(ctx, a, tones, results, info):
    lib = x3hip.lib()
    n, p = a.samples, x3hip.Params.default()
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    x = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, x.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    del wav
    src = x3hip.WindowSource(ctx, (x.data_ptr(), pos), p, seg_blocks=32, frame_offsets=off.data_ptr(), n_frames=F,
                             seg_index=idx.data_ptr())
    bin_len = 1920
    n_bins = -(-n // bin_len)
    bench(ctx, a, "config3", results, info, src, tones, bin_len, n_bins, np.array([0, n_bins]), [n], False)
    src.close()
    torch.cuda.empty_cache()


def corpus_a(ctx, a, tones, results, info):
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
    bin_len = 441
    rf = corpus.levels_rows(bin_len)
    bench(ctx, a, "corpus_a", results, info, corpus, tones, bin_len, int(rf[-1]), rf, ns, True)
    corpus.close()
    for q in (d_x3, d_off):
        ctx.free(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--min-planes", type=int, default=1)
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--single", action="store_true", help="also x3_events_dev on plane 0 in every rep (the yardstick kernels)")
    ap.add_argument("--only-device", action="store_true", help="route (a) alone, no comparison: for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not 1 <= a.min_planes <= a.planes <= x3hip.EVENT_PLANES_MAX or (a.reps < 7 and not a.only_device):
        raise SystemExit("1 <= --min-planes <= --planes <= %d, and medians of at least 7 reps" % x3hip.EVENT_PLANES_MAX)
    torch.cuda.init()
    ctx = x3hip.Context(0)
    tones = [x3hip.Tone(int((t + 1) * (1 << 31) // (a.planes + 1))) for t in range(a.planes)]   # spread over (0, fs / 2)
    results, info = {}, {}
    if "config3" in a.cases:
        config3(ctx, a, tones, results, info)
    if "corpus" in a.cases:
        corpus_a(ctx, a, tones, results, info)
    out = {"samples": a.samples, "planes": a.planes, "reps": a.reps, "cases": info,
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
