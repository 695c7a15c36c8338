#!/usr/bin/env python3
"""Tone levels (x3_tone_levels_dev / x3_corpus_tone_levels_dev, x3_tone_power_levels_dev) on tools/levels_bench.py's cases, the
sides alternating rep by rep in one process; medians of --reps, host time from the call to the synchronised result:
  tone            the tone call at 0.0817 fs with the usual table
  tone_power      the tone call and the adapter in place behind it, to the synchronised records
  samples         the levels call of the same build (x3_levels_dev / x3_corpus_levels_dev)
  fir3            the FIR call of the same build with {1, -2, 1}
  decode_torch    the status quo: decode into a sample buffer (x3_decode_dev_seg / x3_decode_streams_dev), then in torch in
                  int64 the phase of every position, the table gather, the two products and the reshaped sums, with min,
                  max and n
Cases: config3_20_<bin> -- the stream kbench.py makes (691.2 M hydrophone samples, block length 20, the encoder's segment
index), bin_len 1920 and 0; corpus_a_0 -- 4 000 clips of 10-15 s at 44.1 kHz, one record per clip.  The records of the tone
call and of decode_torch are compared with == (every field).  Device memory of both sides goes into the line.  Kernel times:
run it with --no-torch under `rocprofv3 --kernel-trace --stats -- python3 tools/tone_levels_bench.py --no-torch ...`.
--tones K (2 .. 8): the tone bank call (x3_tone_bank_levels_dev / x3_corpus_tone_bank_levels_dev) on
the same cases instead, K oscillators at BANK_FREQS[:K]:
  bank            one bank call of K tones
  singles         K single-tone calls of the same build, one per plane
  tone            one single-tone call (the first tone)
  decode_torch    decode into a sample buffer once, then the torch reduction above once per tone
The planes of `bank` are compared with == against `singles` (bytes) and against decode_torch (every field, every plane).
Prints one JSON line.   (X3HIP_LIB=/path/to/variant.so to measure another build)
    python3 tools/tone_levels_bench.py [--samples N] [--clips N] [--reps 10] [--warmup 2] [--cases config3,corpus] [--no-torch]
                                       [--tones K] [--out file.json]"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
import numpy as np
import torch
import x3hip
if os.environ.get("X3HIP_LIB"):
    x3hip.LIB_PATH = os.environ["X3HIP_LIB"]

now = time.perf_counter
TONE = x3hip.Tone.at(0.0817, 1.0)
FIR3 = x3hip.Fir([1, -2, 1])
BANK_FREQS = (0.0817, 0.2310, 0.15, 0.41, 0.02, 0.33, 0.275, 0.4999)   # --tones K: the first K, in units of fs
CHUNK = 1 << 25   # positions per pass of the flat case: a few int64 temporaries of 256 MB each


def tone_flat(x, bin_len, tab, step=TONE.step):
    """x: int16 [n] -> (re, im, min, max, n) per bin of bin_len positions (whole bins) or over everything"""
    n = x.numel()
    if bin_len:
        rows = n // bin_len
        per = max(1, CHUNK // bin_len)
        re, im = torch.empty(rows, dtype=torch.int64, device=x.device), torch.empty(rows, dtype=torch.int64, device=x.device)
        mn, mx = torch.empty(rows, dtype=torch.int16, device=x.device), torch.empty(rows, dtype=torch.int16, device=x.device)
        for r0 in range(0, rows, per):
            r1 = min(rows, r0 + per)
            pos = torch.arange(r0 * bin_len, r1 * bin_len, dtype=torch.int64, device=x.device)
            k = ((pos * step) & 0xFFFFFFFF) >> 22
            v = x[r0 * bin_len:r1 * bin_len]
            v64 = v.to(torch.int64)
            re[r0:r1] = (v64 * tab[k, 0]).view(-1, bin_len).sum(1)
            im[r0:r1] = (v64 * tab[k, 1]).view(-1, bin_len).sum(1)
            mn[r0:r1], mx[r0:r1] = v.view(-1, bin_len).min(1).values, v.view(-1, bin_len).max(1).values
        cnt = torch.full((rows,), bin_len, dtype=torch.int64, device=x.device)
    else:
        re, im = torch.zeros(1, dtype=torch.int64, device=x.device), torch.zeros(1, dtype=torch.int64, device=x.device)
        for a in range(0, n, CHUNK):
            b = min(n, a + CHUNK)
            pos = torch.arange(a, b, dtype=torch.int64, device=x.device)
            k = ((pos * step) & 0xFFFFFFFF) >> 22
            v64 = x[a:b].to(torch.int64)
            re += (v64 * tab[k, 0]).sum()
            im += (v64 * tab[k, 1]).sum()
        mn, mx = x.min().view(1), x.max().view(1)
        cnt = torch.full((1,), n, dtype=torch.int64, device=x.device)
    torch.cuda.synchronize()
    return re, im, mn, mx, cnt


def equal(rec, red, rows):
    return bool(np.array_equal(rec["re"][:rows], red[0].cpu().numpy()) and np.array_equal(rec["im"][:rows], red[1].cpu().numpy()) and
                np.array_equal(rec["min"][:rows], red[2].cpu().numpy().astype(np.int32)) and
                np.array_equal(rec["max"][:rows], red[3].cpu().numpy().astype(np.int32)) and
                np.array_equal(rec["n"][:rows].astype(np.int64), red[4].cpu().numpy()))


def config3(ctx, a, results, mem, checks):
    lib = x3hip.lib()
    n = a.samples
    wav = torch.empty(n + 32, dtype=torch.int16, device="cuda")
    back = torch.empty(n, dtype=torch.int16, device="cuda")
    ctx.synth_dev(2, 0x58330003, 0, n, wav.data_ptr())
    ctx.sync()
    p = x3hip.Params.make(20, 500)
    F, cap = lib.x3_num_frames(n, C.byref(p)), lib.x3_encode_bound(n, C.byref(p))
    ne = lib.x3_seg_index_entries(F, C.byref(p), 32)
    out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    off = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    so = torch.empty(F + 1, dtype=torch.int64, device="cuda")
    idx = torch.zeros(ne, dtype=torch.int64, device="cuda")
    assert ctx.encode_dev_seg(wav.data_ptr(), n, p, out.data_ptr(), cap, idx.data_ptr(), 32, 0, off.data_ptr()) == 0
    rc, pos, _ = ctx.encode_result()
    assert rc == 0
    assert ctx.sample_offsets_dev(out.data_ptr(), pos, off.data_ptr(), F, so.data_ptr()) == 0
    ctx.sync()
    del wav
    tab = torch.from_numpy(x3hip.tone_table().astype(np.int64)).cuda()
    src = (out.data_ptr(), pos, off.data_ptr(), so.data_ptr(), F, p)
    for bin_len in (1920, 0) if a.tones else ():
        n_bins = -(-n // bin_len) if bin_len else 1
        K, tones = a.tones, x3hip.Tone.bank(BANK_FREQS[:a.tones], 1.0)
        lv = {k: torch.empty(4 * K * n_bins, dtype=torch.int64, device="cuda") for k in ("bank", "singles")}
        one = torch.empty(4 * n_bins, dtype=torch.int64, device="cuda")
        name = "config3_20_%d" % bin_len
        peak, red = 0, None
        for rep in range(a.warmup + a.reps):
            t = {}

            def bank():
                assert ctx.tone_bank_levels_dev(*src, bin_len, lv["bank"].data_ptr(), n_bins, None, idx.data_ptr(), 32, tones) == 0
                r = ctx.levels_result()
                assert r[:2] == (0, 0) and ctx.get_option("last_levels_replays") == 0, r

            def singles():
                for k, tone in enumerate(tones):
                    assert ctx.tone_levels_dev(*src, bin_len, lv["singles"].data_ptr() + 32 * n_bins * k, n_bins, None, idx.data_ptr(), 32, tone) == 0
                    r = ctx.levels_result()
                    assert r[:2] == (0, 0), r

            def tone():
                assert ctx.tone_levels_dev(*src, bin_len, one.data_ptr(), n_bins, None, idx.data_ptr(), 32, tones[0]) == 0
                r = ctx.levels_result()
                assert r[:2] == (0, 0), r
            sides = [("bank", bank), ("singles", singles), ("tone", tone)]
            for side, fn in (sides if rep % 2 == 0 else sides[::-1]):      # (the sides alternate rep by rep)
                t0 = now()
                fn()
                t[side] = now() - t0
            if not a.no_torch:
                red = None
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = now()
                assert ctx.decode_dev_seg(out.data_ptr(), pos, off.data_ptr(), F, p, back.data_ptr(), n, idx.data_ptr(), 32, n_per_clip=n) == 0
                assert ctx.decode_result()[0] == 0
                red = [tone_flat(back, bin_len, tab, tn.step) for tn in tones]
                t["decode_torch"] = now() - t0
                peak = max(peak, torch.cuda.max_memory_allocated() - base)
            if rep >= a.warmup:
                for side, v in t.items():
                    results.setdefault(name + "_" + side, []).append(v * 1e3)
        checks[name + "_bank_is_singles"] = bool(torch.equal(lv["bank"], lv["singles"]))
        if red is not None:
            rec = lv["bank"].cpu().numpy().view(x3hip.TONE_DTYPE).reshape(K, n_bins)
            checks[name + "_bank"] = all(equal(rec[k], red[k], n // bin_len if bin_len else 1) for k in range(K))
        mem[name] = {"bank_workspace_bytes": 32 * K * (n_bins + F) + 48 * F, "bank_records_bytes": 32 * K * n_bins,
                     "single_workspace_bytes": 32 * (n_bins + F) + 48 * F, "tone_table_bytes": 4096,
                     "decode_torch_bytes": 2 * n + int(peak), "stream_bytes": int(pos), "frames": int(F)}
        del lv, red, one
    for bin_len in () if a.tones else (1920, 0):
        n_bins = -(-n // bin_len) if bin_len else 1
        lv = {k: torch.empty(4 * n_bins, dtype=torch.int64, device="cuda") for k in ("samples", "fir3", "tone", "tone_power")}
        name = "config3_20_%d" % bin_len
        peak, red = 0, None
        for rep in range(a.warmup + a.reps):
            t = {}
            t0 = now()
            assert ctx.levels_dev(*src, bin_len, lv["samples"].data_ptr(), n_bins, None, idx.data_ptr(), 32) == 0
            r = ctx.levels_result()
            t["samples"] = now() - t0
            assert r[:2] == (0, 0), r
            t0 = now()
            assert ctx.fir_levels_dev(*src, bin_len, lv["fir3"].data_ptr(), n_bins, None, idx.data_ptr(), 32, FIR3) == 0
            r = ctx.levels_result()
            t["fir3"] = now() - t0
            assert r[:2] == (0, 0), r
            t0 = now()
            assert ctx.tone_levels_dev(*src, bin_len, lv["tone"].data_ptr(), n_bins, None, idx.data_ptr(), 32, TONE) == 0
            r = ctx.levels_result()
            t["tone"] = now() - t0
            assert r[:2] == (0, 0), r
            assert ctx.get_option("last_levels_replays") == 0
            t0 = now()
            assert ctx.tone_levels_dev(*src, bin_len, lv["tone_power"].data_ptr(), n_bins, None, idx.data_ptr(), 32, TONE) == 0
            assert ctx.tone_power_levels_dev(lv["tone_power"].data_ptr(), n_bins, lv["tone_power"].data_ptr()) == 0
            r = ctx.levels_result()
            ctx.sync()
            t["tone_power"] = now() - t0
            assert r[:2] == (0, 0), r
            if not a.no_torch:
                red = None
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = now()
                assert ctx.decode_dev_seg(out.data_ptr(), pos, off.data_ptr(), F, p, back.data_ptr(), n, idx.data_ptr(), 32, n_per_clip=n) == 0
                assert ctx.decode_result()[0] == 0
                red = tone_flat(back, bin_len, tab)
                t["decode_torch"] = now() - t0
                peak = max(peak, torch.cuda.max_memory_allocated() - base)
            if rep >= a.warmup:
                for side, v in t.items():
                    results.setdefault(name + "_" + side, []).append(v * 1e3)
        if red is not None:
            checks[name + "_tone"] = equal(lv["tone"].cpu().numpy().view(x3hip.TONE_DTYPE), red, n // bin_len if bin_len else 1)
        mem[name] = {"levels_bytes": 32 * n_bins + 32 * (n_bins + F) + 48 * F, "tone_table_bytes": 4096,
                     "decode_torch_bytes": 2 * n + int(peak), "stream_bytes": int(pos), "frames": int(F)}
        del lv, red
    del out, off, so, idx, back
    torch.cuda.empty_cache()


def corpus_a(ctx, a, results, mem, checks):
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
    n_rows = int(corpus.levels_rows(0)[-1])
    lv = {k: torch.empty(4 * n_rows, dtype=torch.int64, device="cuda") for k in ("samples", "fir3", "tone", "tone_power")}
    if a.tones:
        return corpus_bank(ctx, a, results, mem, checks, corpus, ns, p, d_x3, pos, offs, lens, F)
    row_len = (max(ns) + 3) // 4 * 4
    rows = torch.empty(n_clips * row_len, dtype=torch.int16, device="cuda")
    res = torch.empty(24 * n_clips, dtype=torch.uint8, device="cuda")
    t_ns = torch.tensor(ns, device="cuda").view(-1, 1)
    tab = torch.from_numpy(x3hip.tone_table().astype(np.int64)).cuda()
    peak, red = 0, None
    for rep in range(a.warmup + a.reps):
        t = {}
        t0 = now()
        assert ctx.corpus_levels_dev(corpus, 0, lv["samples"].data_ptr(), n_rows, None) == 0
        r = ctx.levels_result()
        t["samples"] = now() - t0
        assert r[:2] == (0, 0), r
        t0 = now()
        assert ctx.corpus_fir_levels_dev(corpus, 0, lv["fir3"].data_ptr(), n_rows, None, FIR3) == 0
        r = ctx.levels_result()
        t["fir3"] = now() - t0
        assert r[:2] == (0, 0), r
        t0 = now()
        assert ctx.corpus_tone_levels_dev(corpus, 0, lv["tone"].data_ptr(), n_rows, None, TONE) == 0
        r = ctx.levels_result()
        t["tone"] = now() - t0
        assert r[:2] == (0, 0), r
        t0 = now()
        assert ctx.corpus_tone_levels_dev(corpus, 0, lv["tone_power"].data_ptr(), n_rows, None, TONE) == 0
        assert ctx.tone_power_levels_dev(lv["tone_power"].data_ptr(), n_rows, lv["tone_power"].data_ptr()) == 0
        r = ctx.levels_result()
        ctx.sync()
        t["tone_power"] = now() - t0
        assert r[:2] == (0, 0), r
        if not a.no_torch:
            red = None
            torch.cuda.reset_peak_memory_stats()
            base_mem = torch.cuda.memory_allocated()
            t0 = now()
            assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, rows.data_ptr(), row_len, 0, res.data_ptr()) == 0
            assert ctx.decode_streams_result()[0] == 0
            col = torch.arange(row_len, dtype=torch.int64, device="cuda")
            k = ((col * TONE.step) & 0xFFFFFFFF) >> 22              # (every clip starts at phase 0)
            wc, wsn = tab[k, 0].view(1, -1), tab[k, 1].view(1, -1)
            parts = []
            for c0 in range(0, n_clips, 100):          # (100 clips: 0.5 GB of int64 per temporary)
                x = rows.view(n_clips, row_len)[c0:c0 + 100]
                inside = col.view(1, -1) < t_ns[c0:c0 + 100]
                v = torch.where(inside, x.to(torch.int64), torch.zeros((), dtype=torch.int64, device="cuda"))
                mn = torch.where(inside, x, torch.full_like(x, 32767)).min(1).values
                mx = torch.where(inside, x, torch.full_like(x, -32768)).max(1).values
                parts.append(((v * wc).sum(1), (v * wsn).sum(1), mn, mx))
                del x, v, inside
            red = tuple(torch.cat([q[j] for q in parts]) for j in range(4)) + (torch.tensor(ns, dtype=torch.int64),)
            torch.cuda.synchronize()
            t["decode_torch"] = now() - t0
            peak = max(peak, torch.cuda.max_memory_allocated() - base_mem)
        if rep >= a.warmup:
            for side, v in t.items():
                results.setdefault("corpus_a_0_" + side, []).append(v * 1e3)
    if red is not None:
        checks["corpus_a_0_tone"] = equal(lv["tone"].cpu().numpy().view(x3hip.TONE_DTYPE), red, n_rows)
    mem["corpus_a_0"] = {"levels_bytes": 32 * n_rows + 32 * (n_rows + F) + 48 * F + 8 * (n_clips + 1), "tone_table_bytes": 4096,
                         "decode_torch_bytes": 2 * n_clips * row_len + int(peak), "stream_bytes": int(pos), "frames": int(F),
                         "clips": n_clips, "samples": total}
    corpus.close()


def corpus_bank(ctx, a, results, mem, checks, corpus, ns, p, d_x3, pos, offs, lens, F):
    """--tones K on corpus_a's corpus: one record per clip and tone"""
    n_clips, total = len(ns), int(sum(ns))
    n_rows = int(corpus.levels_rows(0)[-1])
    K, tones = a.tones, x3hip.Tone.bank(BANK_FREQS[:a.tones], 1.0)
    lv = {k: torch.empty(4 * K * n_rows, dtype=torch.int64, device="cuda") for k in ("bank", "singles")}
    one = torch.empty(4 * n_rows, dtype=torch.int64, device="cuda")
    row_len = (max(ns) + 3) // 4 * 4
    rows = torch.empty(n_clips * row_len, dtype=torch.int16, device="cuda")
    res = torch.empty(24 * n_clips, dtype=torch.uint8, device="cuda")
    t_ns = torch.tensor(ns, device="cuda").view(-1, 1)
    tab = torch.from_numpy(x3hip.tone_table().astype(np.int64)).cuda()
    col = torch.arange(row_len, dtype=torch.int64, device="cuda")

    def reduce(step):
        k = ((col * step) & 0xFFFFFFFF) >> 22              # (every clip starts at phase 0)
        wc, wsn = tab[k, 0].view(1, -1), tab[k, 1].view(1, -1)
        parts = []
        for c0 in range(0, n_clips, 100):          # (100 clips: 0.5 GB of int64 per temporary)
            x = rows.view(n_clips, row_len)[c0:c0 + 100]
            inside = col.view(1, -1) < t_ns[c0:c0 + 100]
            v = torch.where(inside, x.to(torch.int64), torch.zeros((), dtype=torch.int64, device="cuda"))
            mn = torch.where(inside, x, torch.full_like(x, 32767)).min(1).values
            mx = torch.where(inside, x, torch.full_like(x, -32768)).max(1).values
            parts.append(((v * wc).sum(1), (v * wsn).sum(1), mn, mx))
            del x, v, inside
        return tuple(torch.cat([q[j] for q in parts]) for j in range(4)) + (torch.tensor(ns, dtype=torch.int64),)
    peak, red = 0, None
    for rep in range(a.warmup + a.reps):
        t = {}

        def bank():
            assert ctx.corpus_tone_bank_levels_dev(corpus, 0, lv["bank"].data_ptr(), n_rows, None, tones) == 0
            r = ctx.levels_result()
            assert r[:2] == (0, 0), r

        def singles():
            for k, tone in enumerate(tones):
                assert ctx.corpus_tone_levels_dev(corpus, 0, lv["singles"].data_ptr() + 32 * n_rows * k, n_rows, None, tone) == 0
                r = ctx.levels_result()
                assert r[:2] == (0, 0), r

        def tone():
            assert ctx.corpus_tone_levels_dev(corpus, 0, one.data_ptr(), n_rows, None, tones[0]) == 0
            r = ctx.levels_result()
            assert r[:2] == (0, 0), r
        sides = [("bank", bank), ("singles", singles), ("tone", tone)]
        for side, fn in (sides if rep % 2 == 0 else sides[::-1]):
            t0 = now()
            fn()
            t[side] = now() - t0
        if not a.no_torch:
            red = None
            torch.cuda.reset_peak_memory_stats()
            base_mem = torch.cuda.memory_allocated()
            t0 = now()
            assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, rows.data_ptr(), row_len, 0, res.data_ptr()) == 0
            assert ctx.decode_streams_result()[0] == 0
            red = [reduce(tn.step) for tn in tones]
            torch.cuda.synchronize()
            t["decode_torch"] = now() - t0
            peak = max(peak, torch.cuda.max_memory_allocated() - base_mem)
        if rep >= a.warmup:
            for side, v in t.items():
                results.setdefault("corpus_a_0_" + side, []).append(v * 1e3)
    checks["corpus_a_0_bank_is_singles"] = bool(torch.equal(lv["bank"], lv["singles"]))
    if red is not None:
        rec = lv["bank"].cpu().numpy().view(x3hip.TONE_DTYPE).reshape(K, n_rows)
        checks["corpus_a_0_bank"] = all(equal(rec[k], red[k], n_rows) for k in range(K))
    mem["corpus_a_0"] = {"bank_workspace_bytes": 32 * K * (n_rows + F) + 48 * F + 8 * (n_clips + 1), "bank_records_bytes": 32 * K * n_rows,
                         "single_workspace_bytes": 32 * (n_rows + F) + 48 * F + 8 * (n_clips + 1), "tone_table_bytes": 4096,
                         "decode_torch_bytes": 2 * n_clips * row_len + int(peak), "stream_bytes": int(pos), "frames": int(F),
                         "clips": n_clips, "samples": total}
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=691_200_000)
    ap.add_argument("--clips", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="config3,corpus")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--tones", type=int, default=0, choices=[0, 2, 3, 4, 5, 6, 7, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = x3hip.Context(0)
    results, mem, checks = {}, {}, {}
    if "config3" in a.cases:
        config3(ctx, a, results, mem, checks)
    if "corpus" in a.cases:
        corpus_a(ctx, a, results, mem, checks)
    out = {"samples": a.samples, "clips": a.clips, "reps": a.reps, "tone_equal_to_torch": checks, "memory": mem,
           "step": TONE.step, "tones": a.tones, "steps": [t.step for t in x3hip.Tone.bank(BANK_FREQS[:a.tones], 1.0)], "library": os.path.basename(os.path.dirname(os.environ["X3HIP_LIB"])) if os.environ.get("X3HIP_LIB") else "tree",
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in results.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in results.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in results.items()}}
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()
    if not all(checks.values()):
        sys.exit("records differ: %s" % checks)


if __name__ == "__main__":
    main()
