#!/usr/bin/env python3
"""bench.py -- encode+decode round trip of BASELINE config 3 (1 h of 192 kHz mono, 691.2 M samples)
on N MI355X GPUs, one process per GPU.

    python bench.py [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch of synthetic audio already resident in HBM:
x3_encode_dev (single-pass encode + compaction into the final stream) followed by x3_decode_dev
(header + payload CRC check + decode) of the stream just produced.  With N > 1 the frames are
sharded -- weak scaling by default: every rank owns its own hour of audio (= BASELINE config 4 at
N = 8); --strong: one stream of --total-samples cut into N frame ranges -- and the step ALSO holds
the path's exchange: the RCCL all-gather of the sub-stream lengths (x3_shard_exchange_lengths) and
the reassembly of the whole .x3a byte stream on rank 0 (x3_shard_gather: grouped ncclSend/ncclRecv,
one xGMI link per peer), both through libx3hip.so's C ABI (librccl directly; torch.distributed only
starts the ranks, hands the communicator id round and takes the max of the ranks' times).  The
gather is also timed alone ("gather"), and --no-gather leaves it out of the step.

Rank 0 prints ONE JSON line (see the contract in the task statement), with
  roofline     -- the encode kernel: algorithmic bytes (2 B/sample read + stream bytes written)
                  / mean launch time from HIP events on the launch stream, vs 8 TB/s HBM
  cpu_baseline -- the CPU oracle (C port of the reference algorithm, 1 thread) on a bounded
                  sample of the same signal, timed in this run on this box's host cores.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
N_SAMPLES = 691_200_000  # config 3: 1 h @ 192 kHz mono
SEED = 0x58330003


def measure_traffic(n, kind, timeout=180):
    """HBM bytes per launch and kernel from two rocprofv3 PMC passes over tools/kbench.py (the same kernels on the same
    workload, three steps each) -> ({kernel: {...}}, source) or ({}, why not).  Counter units and the gfx950 correction
    as in tools/make_traffic.py: KiB; FETCH_SIZE counts a 128-byte request of a 16-byte-per-lane read as 64 bytes."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    from collections import defaultdict
    if shutil.which("rocprofv3") is None:
        return {}, "rocprofv3 not found"
    if any(k.startswith("ROCPROF") or k.startswith("ROCP_") for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return {}, "this run is itself under a profiler"
    d = tempfile.mkdtemp(prefix="x3pmc_", dir="/tmp")
    vals = {}
    sq_counters = ("SQ_BUSY_CYCLES", "SQ_WAVES", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE")
    try:
        # (one counter group per run, no other trace domain: MI355X_MICROARCH.md; the third pass is the SQ's view of the
        # same launches -- busy cycles, waves, vector instructions -- and the GRBM's active cycles: VERDICT r3, item 3)
        for tag, counters in (("FETCH_SIZE", ("FETCH_SIZE",)), ("WRITE_SIZE", ("WRITE_SIZE",)), ("SQ", sq_counters)):
            cmd = ["rocprofv3", "--kernel-trace", "--pmc"] + list(counters) + ["-d", os.path.join(d, tag), "-o", "pmc",
                   "--output-format", "csv", "--", sys.executable, os.path.join(ROOT, "tools", "kbench.py"),
                   "--steps", "3", "--samples", str(n), "--kind", str(kind)]
            try:
                subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=timeout, check=True)
            except Exception:
                if tag == "SQ":
                    break          # (the traffic passes are what the contract needs; the SQ pass is extra)
                raise
            for counter in counters:
                acc = defaultdict(list)
                for f in glob.glob(os.path.join(d, tag, "**", "*counter_collection.csv"), recursive=True):
                    for r in csv.DictReader(open(f)):
                        if r["Counter_Name"] == counter:
                            acc[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
                vals[counter] = {k: sum(v) / len(v) for k, v in acc.items()}
    except Exception as e:
        return {}, "PMC pass failed: %s" % type(e).__name__
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = {}
    for k in set(vals["FETCH_SIZE"]) | set(vals["WRITE_SIZE"]):
        if k.startswith("x3_"):
            fb = vals["FETCH_SIZE"].get(k, 0.0) * 1024 * 2
            wb = vals["WRITE_SIZE"].get(k, 0.0) * 1024
            out[k] = {"hbm_bytes_per_launch": int(fb + wb), "fetch_bytes": int(fb), "write_bytes": int(wb)}
            sq = {c: round(vals[c][k]) for c in sq_counters if k in vals.get(c, {})}
            if sq:
                out[k]["sq_per_launch"] = sq
    if not out:
        return {}, "the PMC passes returned no x3 kernels"
    return out, ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes) over "
                 "tools/kbench.py on the same workload; KiB x 1024, FETCH_SIZE x 2 (gfx950 128-byte requests)")


def native_oracle(params_type):
    """the CPU baseline's oracle: oracle/x3_oracle.c built for THIS host by oracle/Makefile's `native` target (-O3
    -march=native -flto), in a temporary directory -- the tree the benchmark runs from may be read-only, and a build made on
    another host is not native to this one.  Only x3o_time_roundtrip is bound (params_type: the oracle's parameter struct)."""
    import shutil
    import subprocess
    import tempfile
    d = tempfile.mkdtemp(prefix="x3oracle_")
    try:
        for f in ("Makefile", "x3_oracle.c", "x3_oracle.h"):
            shutil.copy(os.path.join(ROOT, "oracle", f), d)
        subprocess.run(["make", "-s", "-C", d, "native"], check=True)
        L = C.CDLL(os.path.join(d, "libx3oracle_native.so"))
    finally:
        shutil.rmtree(d, ignore_errors=True)   # (a loaded library stays mapped)
    L.x3o_time_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(params_type), C.c_int, C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.x3o_init.restype = None
    L.x3o_init()
    return L


COMPACT_MAX = 4000   # characters of the contract line (tests/test_bench_contract.py holds it to this)


def compact_line(res):
    """the contract's JSON line cut down to what the driver and the judge read (everything else: the bench_details line)"""
    def short(s, n=150):
        return s if len(s) <= n else s[:n - 3] + "..."

    def roof(r, full):
        keys = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "avg_launch_ms") if full else \
               ("kernel", "frac", "avg_launch_ms", "traffic")
        o = {k: r[k] for k in keys if k in r}
        v = r.get("valu_issue")
        if v:
            o["valu"] = {"insts": v["insts"], "per_sample": v["lane_insts_per_sample"], "frac_of_issue_peak": v.get("frac_of_peak", v.get("frac"))}
        return o
    c = {k: res[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                             "vs_baseline", "dtype", "data")}
    cfg = res["config"]
    c["config"] = {k: cfg[k] for k in ("workload", "samples_per_gpu", "frames_per_gpu", "stream_bytes_per_gpu", "bytes_per_sample",
                                       "frames_verified_vs_oracle", "settle_steps", "sharding") if k in cfg}
    c["config"]["workload"] = short(c["config"]["workload"], 120)
    c["config"]["sharding"] = short(c["config"]["sharding"], 120)
    c["roofline"] = roof(res["roofline"], True)
    c["roofline_all"] = {k: roof(v, False) for k, v in res["roofline_all"].items()}
    c["encode_read_frac"] = res["encode_read_frac"]
    c["kernels_ms"] = {k: v for k, v in res["kernels_ms"].items() if v}
    st = res.get("kernels_ms_stats", {})
    c["kernels_ms_p90_over_min"] = {k: round(v["p90"] / v["min"], 3) for k, v in st.items() if v and v.get("min")}
    c["clocks_mhz"] = {k[:-len("_kernel_mhz")]: v.get("median") for k, v in (res.get("clocks") or {}).items() if k.endswith("_kernel_mhz")}
    cb = res.get("cpu_baseline")
    if isinstance(cb, dict):    # (None: --no-cpu-baseline, or a rank count above one -- the baseline is timed at N = 1 only)
        c["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind") if k in cb}
        c["cpu_baseline"]["sample"] = short(cb.get("sample", ""), 130)
        for k in ("encode_msamples_s", "decode_msamples_s"):
            if k in cb:
                c["cpu_baseline"][k] = cb[k]
        if isinstance(cb.get("all_cores"), dict):
            c["cpu_baseline"]["all_cores"] = {k: cb["all_cores"][k] for k in ("value", "cores") if k in cb["all_cores"]}
    else:
        c["cpu_baseline"] = None
    c["value_without_kernel_events"] = res.get("value_without_kernel_events")
    c["value_with_all_kernel_events"] = res.get("value_with_all_kernel_events")
    for k in ("decoder_kernels",):
        if k in res:
            c[k] = res[k]
    if "cold" in res:
        c["cold_ms_per_step"] = res["cold"]["ms_per_step"]
        c["value_with_frame_walk"] = res.get("value_with_frame_walk")
        ex = res.get("extremes", {})
        c["extremes_ms_per_step"] = {k: v["ms_per_step"] for k, v in ex.items() if isinstance(v, dict) and "ms_per_step" in v}
    if "configs" in res:
        c["configs"] = {}
        for cn in ("config2", "config5"):
            v = res["configs"].get(cn)
            if isinstance(v, dict):
                c["configs"][cn] = {"skipped": short(v["skipped"], 60)} if "skipped" in v else \
                    {"step": v.get("step"), "step_with_segment_index": (v.get("with_segment_index") or {}).get("step")}
    if "gather" in res:
        g = res["gather"]
        c["gather"] = {k: g[k] for k in ("mode", "ms", "in_timed_region", "value_without_gather") if k in g}
        c["rccl"] = res.get("rccl")
    if res.get("placement"):
        pl = res["placement"]
        c["placement"] = {"candidates_per_buffer": pl["candidates_per_buffer"], "step_ms": pl["step_ms"]}
    c["details"] = "bench_details.json beside this run (--details): notes, per-step arrays, layouts, host-buffer and per-frame APIs"
    # never longer than the tail the driver keeps: drop the least important keys first
    for k in ("extremes_ms_per_step", "kernels_ms_p90_over_min", "configs", "decoder_kernels", "cold_ms_per_step"):
        if len(json.dumps(c)) <= COMPACT_MAX:
            break
        c.pop(k, None)
    return c


# --dump-outputs: an output longer than its share of the budget is written as a seeded sample of windows of DUMP_WINDOW
# consecutive elements (the first and the last window always among them), so that two builds can be compared output for output
DUMP_MAX_BYTES = 64_000_000      # all files of one dump together
DUMP_WINDOW = 4096
DUMP_STREAM_ELEMS = 4 << 20      # float32: 16 MiB
DUMP_DECODED_ELEMS = 4 << 20     # float32: 16 MiB
DUMP_OFFSETS_ELEMS = 2 << 20     # float64: 16 MiB (config 3 has 69 121 offsets: all of them)


def dump_sample(t, max_elems):
    """a 1-D device tensor -> (a copy of it on the device, None), or (its sampled windows, shape (windows, DUMP_WINDOW), the
    windows' first indexes) when it is longer than max_elems.  The windows depend on the length alone."""
    import numpy as np
    import torch
    m = t.numel()
    if m <= max_elems:
        return t.clone(), None
    rng = np.random.default_rng([SEED, m])
    last = m - DUMP_WINDOW
    starts = np.unique(np.concatenate([[0, last], rng.integers(0, last + 1, max_elems // DUMP_WINDOW - 2)])).astype(np.int64)
    idx = torch.from_numpy(starts).to(t.device)[:, None] + torch.arange(DUMP_WINDOW, dtype=torch.int64, device=t.device)
    return t[idx], starts


def write_dump(d, arrays):
    """{name: (device tensor or numpy array, window starts or None)} -> d/<name>.npy (+ d/<name>_window_starts.npy) in float32
    (8- and 16-bit integers) or float64 (wider ones, exact below 2**53); returns what was written"""
    import numpy as np
    import torch
    files = {}
    for name, (a, starts) in arrays.items():
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.dtype.itemsize <= 2:
            files[name] = a.astype(np.float32)
        else:
            assert a.size == 0 or np.abs(a.astype(np.float64)).max() < 2 ** 53, name
            files[name] = a.astype(np.float64)
        if starts is not None:
            files[name + "_window_starts"] = starts.astype(np.float64)
    total = sum(v.nbytes for v in files.values())
    assert total <= DUMP_MAX_BYTES, total
    if not os.path.isdir(d):
        os.makedirs(d)
        # (a directory this run creates stays out of version control wherever it lies)
        with open(os.path.join(d, ".gitignore"), "w") as fh:
            fh.write("*\n")
    for name, v in files.items():
        np.save(os.path.join(d, name + ".npy"), v)
    return {"dir": d, "bytes": int(total),
            "arrays": {name: {"shape": list(arrays[name][0].shape), "sampled": arrays[name][1] is not None} for name in arrays}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--samples", type=int, default=N_SAMPLES, help="samples per GPU (default: config 3)")
    ap.add_argument("--kind", type=int, default=2, help="synthetic signal (2 = hydrophone noise)")
    ap.add_argument("--cpu-sample", type=int, default=100_000_000, help="samples timed on the CPU baseline")
    ap.add_argument("--cpu-reps", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--details", default="bench_details.json",
                    help="file that takes everything the one-line record leaves out ('-': stderr, '': nowhere)")
    ap.add_argument("--no-gather", action="store_true", help="= --gather none")
    ap.add_argument("--gather", choices=("in-step", "overlapped", "sharded", "none"), default="in-step",
                    help="N > 1: the reassembly of the whole stream -- on rank 0 inside every step on the context's stream (the "
                         "contract's `value`: where north_star puts it), on rank 0 beside the next steps on the shard's own stream "
                         "and communicator, SHARDED (no rank takes in the whole stream: every rank writes its sub-stream at its "
                         "own offset of one file, x3_shard_write_at), or not at all; the other modes are timed as well (gather_modes)")
    ap.add_argument("--gather-file", default=None,
                    help="--gather sharded: the file all ranks write into (default: /dev/shm/x3_bench_<MASTER_PORT>.x3a, removed at the end)")
    ap.add_argument("--mode-steps", type=int, default=10, help="timed steps for each of the gather modes that is not --gather")
    ap.add_argument("--verify-gather", action="store_true",
                    help="rank 0 compares the reassembled stream with the oracle's encoding of the whole signal (small totals)")
    ap.add_argument("--strong", action="store_true", help="strong scaling: --total-samples cut into N frame ranges")
    ap.add_argument("--total-samples", type=int, default=8 * N_SAMPLES, help="--strong: the whole stream (config 4: 8 h)")
    ap.add_argument("--no-verify-all", action="store_true", help="compare only sampled frames with the CPU oracle")
    ap.add_argument("--settle", type=int, default=0,
                    help="extra untimed steps in front of the warm-up (0: none -- a context's first launch is paced from the data)")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the cold-context, frame-walk and extreme-content measurements that ride on the line")
    ap.add_argument("--no-measure-traffic", action="store_true",
                    help="roofline.traffic from profiles/traffic.json instead of two rocprofv3 PMC passes run here")
    ap.add_argument("--settle-ms", type=float, default=500.0,
                    help="upper bound of the time-based settle in front of the warm-up: steps are run until the shader clock "
                         "the kernels log has stayed within 2.5 %% of its running maximum for 8 launches (0: no settle)")
    ap.add_argument("--place", type=int, default=8,
                    help="candidates per buffer for the placement probe (x3hip.place_buffers: the pair of stream / sample buffers "
                         "the round trip runs best on is kept; 1 = take the first allocation as it comes)")
    ap.add_argument("--no-configs", action="store_true", help="skip the timing of BASELINE configs 2 and 5 (`configs` in the line)")
    ap.add_argument("--spawn", action="store_true",
                    help="start the ranks as a child process (torch.distributed.run) even for --gpus 1; --gpus N > 1 without "
                         "WORLD_SIZE in the environment does so by itself")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step handed its caller (the stream, its frame offsets, the encoder's "
                         "block-type counts, the decoded samples) as DIR/<name>.npy in float32 / float64, at most 64 MB in all: "
                         "an output longer than its share is a seeded sample of windows (DIR/<name>_window_starts.npy says "
                         "where they start).  Rank 0's outputs with --gpus N > 1")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # `python3 bench.py --gpus N` outside torch.distributed.run: start the N ranks ourselves, as a CHILD process and before
    # anything here has touched the GPU (a process that has initialised HIP must never be replaced by another program);
    # the child's JSON line goes to our stdout as it is, its return code becomes ours.
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.spawn):
        import socket
        import subprocess
        s_ = socket.socket()
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
        s_.close()
        child_args = [a for a in sys.argv[1:] if a != "--spawn"]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + child_args
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.stdout.flush()
        sys.exit(subprocess.run(cmd, env=env).returncode)

    import numpy as np
    import torch
    import x3hip

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        args.gpus = world    # (the launcher decides; an unset WORLD_SIZE with --gpus N > 1 has started its own ranks above)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    # X3_BENCH_FORCE_DIST=1: take the distributed path (RCCL init, length exchange, gather, barriers) with one rank
    # too -- a way to exercise it on a one-GPU box (launch through torch.distributed.run --nproc-per-node 1)
    if world > 1 or os.environ.get("X3_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", "29531")   # (X3_BENCH_FORCE_DIST=1 without a launcher)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    p = x3hip.Params.default()
    L = x3hip.lib()
    if args.strong:
        first_sample, n = x3hip.shard_sample_range(args.total_samples, p, rank, world)
    else:
        first_sample, n = rank * args.samples, args.samples  # every rank owns a different hour of the same signal
    F = L.x3_num_frames(n, C.byref(p))
    cap = L.x3_encode_bound(n, C.byref(p))

    stream = torch.cuda.current_stream(dev)
    ctx = x3hip.Context(local_rank, stream=stream.cuda_stream)

    wav = torch.empty(n, dtype=torch.int16, device=dev)
    out = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
    off = torch.empty(F + 1, dtype=torch.int64, device=dev)
    back = torch.empty(n, dtype=torch.int16, device=dev)
    ctx.synth_dev(args.kind, SEED, first_sample, n, wav.data_ptr())
    torch.cuda.synchronize(dev)

    # ---- placement (round 6): where the stream and the decoded samples lie in HBM decides the decode
    # phase's pace by up to 10 % -- per pair of buffers, reproducibly within a process (profiles/r6/decoder_modes.txt).  As a
    # pipeline that keeps its buffers would: a few candidates, a short probe of every pair, the best pair stays.
    placement = None
    if args.place > 1:
        cand_out, cand_back, pads = [out], [back], []
        for k in range(args.place - 1):
            # (odd-sized allocations between the candidates: so that they do not all lie alike)
            try:
                pads.append(torch.empty((k + 1) * 1237 * 1024, dtype=torch.uint8, device=dev))
                o_k = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
                b_k = torch.empty(n, dtype=torch.int16, device=dev)
            except RuntimeError:   # (a GPU that has no room for more candidates: the probe makes do with what it has)
                break
            cand_out.append(o_k)
            cand_back.append(b_k)
        ms = x3hip.place_buffers(ctx, p, wav.data_ptr(), n, [t.data_ptr() for t in cand_out], cap, off.data_ptr(),
                                 [t.data_ptr() for t in cand_back])
        flat = [(ms[i][j], i, j) for i in range(len(cand_out)) for j in range(len(cand_back))]
        best = min(flat)
        placement = {"candidates_per_buffer": len(cand_out), "probe": "4 untimed + 8 timed round trips per pair, host wall time",
                     "step_ms": {"first_allocation": round(ms[0][0], 4), "best": round(best[0], 4), "worst": round(max(flat)[0], 4)},
                     "kept": {"stream": best[1], "samples": best[2]},
                     "ms_per_step": [[round(v, 4) for v in row] for row in ms],
                     "stream_buffers": ["%x" % t.data_ptr() for t in cand_out], "sample_buffers": ["%x" % t.data_ptr() for t in cand_back]}
        out, back = cand_out[best[1]], cand_back[best[2]]
        del cand_out, cand_back, pads
        torch.cuda.empty_cache()

    # ---- the group of ranks: librccl through the library's own C ABI (x3_shard_*)
    rccl = None
    shard_obj = None
    lens = torch.zeros(world, dtype=torch.int64, device=dev)
    if dist is not None:
        idt = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            idt.copy_(torch.frombuffer(bytearray(x3hip.shard_unique_id()), dtype=torch.uint8))
        dist.broadcast(idt, src=0)
        shard_obj = x3hip.Shard(ctx, bytes(idt.cpu().numpy().tobytes()), rank, world)
        # (ranks_seen: what the communicator itself says, x3_shard_world -- so that a SCALE record answers "did RCCL see N ranks")
        rccl = {"ranks_seen": int(x3hip.lib().x3_shard_world(shard_obj._h)),
                "via": "librccl through x3_shard_* (ncclAllGather of %d lengths; grouped ncclSend/ncclRecv to rank 0)" % world}

    if args.no_gather:
        args.gather = "none"
    gather_mode = args.gather if dist is not None else "none"
    gather_in_step = gather_mode in ("in-step", "sharded")

    # The overlapped reassembly needs the sub-stream of step k-1 to stay put while step k+1 is encoded: three output
    # buffers (and frame indexes, length vectors) in rotation; the other modes use the first one only.
    NB = 3 if dist is not None else 1
    outs = [out] + [torch.empty(cap + 16, dtype=torch.uint8, device=dev) for _ in range(NB - 1)]
    offs_b = [off] + [torch.empty(F + 1, dtype=torch.int64, device=dev) for _ in range(NB - 1)]
    lens_b = [lens] + [torch.zeros(world, dtype=torch.int64, device=dev) for _ in range(NB - 1)]
    lens_pin = [torch.zeros(world, dtype=torch.int64).pin_memory() for _ in range(NB)] if dist is not None else []
    lens_ev = [torch.cuda.Event() for _ in range(NB)] if dist is not None else []
    pipe = {"k": 0, "issued": -1}   # steps enqueued so far in overlapped mode; the last step whose reassembly was issued

    # --gather sharded: ONE file, every rank its own descriptor (rank 0 creates it; the others open it behind a barrier)
    shard_file = {"fd": -1, "path": None}

    def open_shard_file():
        if shard_file["fd"] >= 0 or dist is None:
            return
        path = args.gather_file or "/dev/shm/x3_bench_%s.x3a" % os.environ.get("MASTER_PORT", "0")
        if rank == 0:
            fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o600)
        dist.barrier()
        if rank != 0:
            fd = os.open(path, os.O_RDWR)
        shard_file["fd"], shard_file["path"] = fd, path

    def one_step(mode, b=0):
        """encode + decode (+ the exchange of the lengths, + the reassembly as `mode` says) with output buffer b"""
        rc = ctx.encode_dev(wav.data_ptr(), n, p, outs[b].data_ptr(), cap, 0, offs_b[b].data_ptr())
        assert rc == 0, (rc, ctx.last_error())
        rc = ctx.decode_dev(outs[b].data_ptr(), cap, offs_b[b].data_ptr(), F, p, back.data_ptr(), n, n_per_clip=n)
        assert rc == 0, (rc, ctx.last_error())
        if shard_obj is not None:
            # exchange step 1: sub-stream lengths -> global byte offsets (8 bytes per rank; no rank's decode needs
            # another rank's length, so it is enqueued behind the decoder rather than in front of it)
            shard_obj.exchange_lengths(offs_b[b].data_ptr() + 8 * F, lens_b[b].data_ptr())
        if mode == "in-step":
            # exchange step 2: the whole .x3a byte stream on rank 0.  The lengths have to reach the host first
            # (they are the send/recv sizes): one small copy + sync per step, part of the path's cost
            lens_h = lens_b[b].cpu().tolist()
            wb = whole_buf(sum(lens_h))
            shard_obj.gather(outs[b].data_ptr(), lens_h, 0, wb.data_ptr() if rank == 0 else None, wb.numel())
        elif mode == "sharded":
            # exchange step 2, sharded: nobody takes in the whole stream -- this rank's sub-stream goes down its own host link
            # and into the file at its own offset (x3_shard_write_at; returns when the bytes are written)
            lens_h = lens_b[b].cpu().tolist()
            shard_obj.write_at(outs[b].data_ptr(), lens_h, shard_file["fd"], 0)

    def issue_gather(j):
        """overlapped mode: the reassembly of step j on the shard's own stream (its lengths are on the host by now)"""
        bj = j % NB
        lens_ev[bj].synchronize()            # step j has run (the steps behind it go on)
        lens_h = lens_pin[bj].tolist()
        shard_obj.gather_wait(on_stream=True)   # one in flight; what is enqueued from here on may reuse ITS buffers
        wb = whole_buf(sum(lens_h))
        shard_obj.gather(outs[bj].data_ptr(), lens_h, 0, wb.data_ptr() if rank == 0 else None, wb.numel(), overlapped=True)
        pipe["issued"] = j

    def step_overlapped():
        k = pipe["k"]
        b = k % NB
        one_step("overlapped", b)
        lens_pin[b].copy_(lens_b[b], non_blocking=True)
        lens_ev[b].record(stream)
        if k >= 1:
            issue_gather(k - 1)              # beside step k (and k + 1 ...), out of the buffer step k + 2 will write to
        pipe["k"] = k + 1

    def drain_overlapped():
        """the last step's reassembly, and the end of all of them"""
        if pipe["k"] >= 1 and pipe["issued"] < pipe["k"] - 1:
            issue_gather(pipe["k"] - 1)
        shard_obj.gather_wait(on_stream=False)
        pipe["k"], pipe["issued"] = 0, -1

    def step():
        if gather_mode == "overlapped":
            step_overlapped()
        else:
            one_step(gather_mode)

    whole_holder = {}

    def whole_buf(total):
        # (every rank sizes it alike, so that every rank passes the same capacity to the reassembly; only rank 0's is written)
        t = whole_holder.get("t")
        if t is None or t.numel() < total:
            t = torch.empty((int(total * 1.05) + 4096) if rank == 0 else 16, dtype=torch.uint8, device=dev)
            whole_holder["t"] = t
            whole_holder["cap"] = int(total * 1.05) + 4096
        class _W:   # what the callers use: pointer and the ROOT's capacity
            def __init__(self, t, cap): self.t, self.cap = t, cap
            def data_ptr(self): return self.t.data_ptr()
            def numel(self): return self.cap
        return _W(t, whole_holder["cap"])

    def barrier():
        if dist is not None:
            dist.barrier()

    if gather_mode == "sharded":
        open_shard_file()
    # (--settle: extra untimed launches in front of the contract's W warm-up steps, reported as config.settle_steps.
    # Round 2 needed twelve for the kernels' pace controllers; a first launch is now paced from the data: 0.)
    for _ in range(args.settle):
        step()
    # Time-based settle: a fresh box ramps its shader clock over the first tens of milliseconds of
    # load, and W = 5 warm-up steps are 6 ms.  Steps are run, eight at a time, until the clock the DECODE kernel logs for
    # itself (workgroup 0's s_memtime against s_memrealtime) has stayed within 2.5 % of its running maximum for eight
    # launches, bounded by --settle-ms; the trace goes into the line (config.settle_*).  Untimed, in front of the warm-up.
    settle = {"steps": 0, "ms": 0.0, "clock_mhz": [], "settled": None}
    if args.settle_ms > 0:
        t_s = time.perf_counter()
        run_max = 0.0
        while True:
            for _ in range(8):
                step()
            if gather_mode == "overlapped":
                drain_overlapped()
            torch.cuda.synchronize(dev)
            settle["steps"] += 8
            last8 = [e["clock_mhz"] for e in ctx.launch_log(1)[-8:]]
            settle["clock_mhz"] += [round(c) for c in last8]
            run_max = max([run_max] + last8)
            ok = len(last8) == 8 and min(last8) >= 0.975 * run_max and settle["steps"] >= 16
            settle["ms"] = (time.perf_counter() - t_s) * 1e3
            late = settle["ms"] >= args.settle_ms
            if dist is not None:   # all ranks leave together: settled everywhere, or out of time anywhere
                tt = torch.tensor([0 if ok else 1, 1 if late else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                ok, late = int(tt[0].item()) == 0, int(tt[1].item()) == 1
            if ok or late:
                settle["settled"] = bool(ok)
                break
    for _ in range(args.warmup):
        step()
    if gather_mode == "overlapped":
        drain_overlapped()
    rc, pos, stats = ctx.encode_result()
    assert rc == 0, (rc, ctx.last_error())
    rc, first_bad, st, before = ctx.decode_result()
    assert (rc, first_bad, st, before) == (0, F, 0, n), (rc, first_bad, st, before)

    # The timed region carries the HIP events of the DECODE PHASE's two kernels -- the decoder, whose launch duration over exactly
    # these K steps is `roofline`, as the contract asks, and the check kernel that runs beside it (both or neither: with events
    # on the decoder alone its dispatch is held back behind the marker, the check kernel's workgroups take the CUs first and
    # the decoder runs in 0.92 ms instead of 0.64 -- measured).  The encoder's, the dense pass's and the merge kernel's events
    # (a marker packet behind each kernel: five a step, 24 us, 2 % of a step) ride on a second pass of the same K steps right
    # behind it (`kernels_ms` for them, and that pass's rate as `value_with_all_kernel_events`: what `value` was until round
    # 5); a third pass has none (`value_without_kernel_events`).
    def timed_pass():
        barrier()
        torch.cuda.synchronize(dev)
        t0_ = time.perf_counter()
        for _ in range(args.steps):
            step()
        if gather_mode == "overlapped":
            drain_overlapped()   # (the last reassembly is part of the K steps)
        torch.cuda.synchronize(dev)
        barrier()
        el = time.perf_counter() - t0_
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        rc_, pos_, stats_ = ctx.encode_result()
        assert rc_ == 0, (rc_, ctx.last_error())
        r_ = ctx.decode_result()
        assert r_ == (0, F, 0, n), r_
        return el, pos_, stats_
    ctx.set_option("kernel_timing_mask", int(os.environ.get("X3_BENCH_MASK", str((1 << 1) | (1 << 4))), 0))
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_time()
    elapsed, pos, stats = timed_pass()
    decode_ts, check_ts = ctx.kernel_times(1), ctx.kernel_times(4)
    ctx.set_option("kernel_timing_mask", 0xFFFFFFFF)
    ctx.reset_kernel_time()
    elapsed_all_events, pos_a, _ = timed_pass()
    assert pos_a == pos
    # every timed launch's own HIP-event time (the events ride on the kernels' dispatch packets): mean, minimum, median and
    # p90 over the K timed steps, and the K values themselves
    def kstats(ts):
        v = sorted(ts)
        return {"n": len(v), "mean": round(sum(v) / len(v), 4), "min": round(v[0], 4), "median": round(v[len(v) // 2], 4),
                "p90": round(v[min(len(v) - 1, (9 * len(v)) // 10)], 4), "max": round(v[-1], 4)}
    ktimes, ksteps = {}, {}
    for name, which in (("encode", 0), ("decode", 1), ("frame_sizes", 2), ("scan", 3), ("frame_check", 4), ("encode_dense_pass", 5)):
        ts = decode_ts if which == 1 else (check_ts if which == 4 else ctx.kernel_times(which))   # (the decode phase's: those of the timed region itself)
        ktimes[name] = sum(ts) / max(len(ts), 1)
        if ts:
            ksteps[name] = ts
    ctx.enable_kernel_timing(False)
    enc_gen = int(ctx.get_option("enc_gen_in_use"))
    # the kernels' own launch log: the shader clock each launch ran at (workgroup 0's shader ticks against the constant
    # 100 MHz clock over its life) and, for the decoder, the pace it aimed at and the pace its slowest group achieved
    dlog = ctx.launch_log(1)[-args.steps:]
    elog = ctx.launch_log(0)[-args.steps:]
    # The same K steps once more without any events: what a caller who does not time kernels gets.  Reported beside `value`
    # (K steps with the dominant kernel's events inside the timed region).
    barrier()
    torch.cuda.synchronize(dev)
    t0u = time.perf_counter()
    for _ in range(args.steps):
        step()
    if gather_mode == "overlapped":
        drain_overlapped()
    torch.cuda.synchronize(dev)
    barrier()
    elapsed_untimed = time.perf_counter() - t0u
    if dist is not None:
        t = torch.tensor([elapsed_untimed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_untimed = float(t.item())
    rc, pos_u, stats_u = ctx.encode_result()
    assert rc == 0 and pos_u == pos, (rc, pos_u, pos)
    rc, first_bad, st, before = ctx.decode_result()
    assert (rc, first_bad, st, before) == (0, F, 0, n), (rc, first_bad, st, before)
    def med(v):
        v = sorted(v)
        return v[len(v) // 2] if v else None
    clocks = {"device_max_mhz": torch.cuda.get_device_properties(dev).clock_rate / 1000.0 if hasattr(torch.cuda.get_device_properties(dev), "clock_rate") else None,
              "decode_kernel_mhz": {"median": med([e["clock_mhz"] for e in dlog]), "min": min([e["clock_mhz"] for e in dlog], default=None),
                                    "max": max([e["clock_mhz"] for e in dlog], default=None)},
              "encode_kernel_mhz": {"median": med([e["clock_mhz"] for e in elog]), "min": min([e["clock_mhz"] for e in elog], default=None),
                                    "max": max([e["clock_mhz"] for e in elog], default=None)},
              "note": "shader clock DURING the kernel: workgroup 0's s_memtime ticks / s_memrealtime ticks x 100 MHz over its "
                      "whole life, logged by the kernel itself for every launch (x3_ctx_launch_log); the pool's boxes differ "
                      "by 9 % in the decoder's time, and this says whether a line comes from a slow box"}
    # pace: 10 ns ticks per 16 blocks -> us per block; target = what the launch aimed at, achieved = its slowest group
    decoder_pace = {"target_us_per_block": [round(e["target_ticks16"] / 1600.0, 4) for e in dlog],
                    "achieved_us_per_block": [round(e["achieved_ticks16"] / 1600.0, 4) for e in dlog],
                    "note": "per timed step: the decoder's pace controller (x3_decode_split_kernel.h); a launch that misses its "
                            "target by more than a few per cent has all its waves at one priority = the unpaced kernel"}
    # --dump-outputs: what the last timed step (the last of the pass above) handed its caller, before anything else
    # overwrites the buffers
    dump_info = None
    if args.dump_outputs and rank == 0:
        # (the buffer the last step wrote: only the overlapped mode rotates them, and every pass of it starts at the first)
        lb = (args.steps - 1) % NB if gather_mode == "overlapped" else 0
        dump_info = write_dump(args.dump_outputs, {"stream": dump_sample(outs[lb][:pos], DUMP_STREAM_ELEMS),
                                                   "frame_offsets": dump_sample(offs_b[lb][:F + 1], DUMP_OFFSETS_ELEMS),
                                                   "decoded": dump_sample(back[:n], DUMP_DECODED_ELEMS),
                                                   "encode_stats": (stats_u, None)})

    # ---- bit-exactness of the timed output: decode(encode(x)) == x, and the stream == the CPU oracle's
    assert torch.equal(back, wav), "decode(encode(x)) != x"
    import oracle_lib as O
    offs = off.cpu().numpy()
    assert int(offs[-1]) == pos
    verified = 0
    if rank != 0:
        # every rank checks a sample of its own frames against the oracle (rank 0: all of them, below)
        for fr in sorted({0, F // 3, (2 * F) // 3, F - 1}):
            a_, b_ = fr * p.spf, min(n, (fr + 1) * p.spf)
            enc = O.encode(wav[a_:b_].cpu().numpy())[1]
            assert np.array_equal(enc, out[int(offs[fr]):int(offs[fr + 1])].cpu().numpy()), "rank %d frame %d differs from the CPU oracle" % (rank, fr)
    if rank == 0:
        import concurrent.futures as cf
        frames = list(range(F)) if not args.no_verify_all else [0, F // 3, F - 1]
        host_wav = wav.cpu().numpy()
        host_out = out[:pos].cpu().numpy()
        chunk = 256 if not args.no_verify_all else 1
        jobs = [(f0, min(F, f0 + chunk)) for f0 in range(0, F, chunk)] if not args.no_verify_all else [(f, f + 1) for f in frames]

        def vwork(j):
            a, b = j
            enc = O.encode(host_wav[a * p.spf:min(n, b * p.spf)])[1]
            return np.array_equal(enc, host_out[int(offs[a]):int(offs[b])]), j
        with cf.ThreadPoolExecutor(max_workers=min(64, os.cpu_count() or 1)) as ex:
            for ok, j in ex.map(vwork, jobs):
                assert ok, "frames %d..%d differ from the CPU oracle" % j
                verified += j[1] - j[0]
        del host_wav, host_out

    # ---- the reassembly on rank 0 alone (and its result: the ranks' sub-streams back to back)
    gather = None
    gather_modes = None
    if shard_obj is not None:
        lens_h = lens.cpu().tolist()
        starts = x3hip.shard_offsets(lens_h)
        assert lens_h[rank] == pos and all(v % 2 == 0 for v in starts)
        wb = whole_buf(starts[-1])
        torch.cuda.synchronize(dev)
        barrier()
        g0 = time.perf_counter()
        greps = 3
        for _ in range(greps):
            shard_obj.gather(out.data_ptr(), lens_h, 0, wb.data_ptr() if rank == 0 else None, wb.numel())
        torch.cuda.synchronize(dev)
        barrier()
        g1 = time.perf_counter()
        whole_ok = None
        if rank == 0:
            wt = wb.t
            assert torch.equal(wt[starts[0]:starts[1]], out[:pos]), "rank 0's own part of the gathered stream"
            if args.verify_gather:
                # the whole reassembled stream against the oracle's encoding of the whole signal (the ranks' signals are
                # consecutive stretches of one generator: weak -- every rank n samples -- and strong alike)
                tot_n = args.total_samples if args.strong else n * world
                full = x3hip.synth(args.kind, SEED, 0, tot_n)
                rc_o, ref, _ = O.encode(full)
                whole_ok = bool(rc_o == 0 and ref.size == starts[-1] and np.array_equal(ref, wt[:starts[-1]].cpu().numpy()))
                assert whole_ok, "the reassembled stream differs from the oracle's encoding of the whole signal"
        gather = {"ms": round((g1 - g0) / greps * 1e3, 3), "bytes": int(starts[-1]),
                  "gb_s": round(starts[-1] / ((g1 - g0) / greps) / 1e9, 1),
                  "pattern": "x3_shard_gather: grouped ncclSend/ncclRecv to rank 0 (one xGMI link per peer)",
                  "in_timed_region": bool(gather_in_step), "mode": gather_mode,
                  "whole_stream_verified_vs_oracle": whole_ok,
                  "note": "What the curve over N has to look like (DESIGN.md, multi-GPU).  A rank's compute step is ~1.15 ms for "
                          "691.2 M samples and leaves a 363 MB sub-stream.  in-step (the default, where north_star puts the "
                          "reassembly): all of it lands on ONE GPU per step, over at most seven xGMI links at ~55 GB/s each -- "
                          "~6.5 ms whatever N is -- so value ~ N x 691.2 M / (1.2 + 6.5 ms): 0.3 x one GPU at N = 2, 1.2 x at "
                          "N = 8; overlapped hides the compute behind it (1.4 x at N = 8: the root's ingest is the bound).  "
                          "sharded: nobody takes in the whole stream, every rank writes its sub-stream at its own offset of one "
                          "file over its own host link (x3_shard_write_at; ~56 GB/s per rank: ~6.5 ms per step, but N of them "
                          "side by side), so value ~ N x 691.2 M / 7.7 ms -- linear in N, 1.2 x one no-output GPU at N = 8.  "
                          "none = gather_modes.none is the N x figure of the independent shards.  north_star's >= 6 x at "
                          "8 GPUs is met by none, approached by no mode that delivers the bytes once per step."}
        # ---- the other two ways of placing the reassembly, timed like the headline (barrier + synchronize on both sides,
        # maximum over the ranks): in the step, beside the following steps, not at all
        gather_modes = {}
        for mode in ("in-step", "overlapped", "sharded", "none"):
            if mode == "sharded":
                open_shard_file()
            if mode == gather_mode:
                gather_modes[mode] = {"ms_per_step": round(elapsed / args.steps * 1e3, 4),
                                      "value": round(n * world * args.steps / elapsed / 1e6, 2), "steps": args.steps, "is_value": True}
                continue
            def mstep():
                if mode == "overlapped":
                    step_overlapped()
                else:
                    one_step(mode)
            for _ in range(3):
                mstep()
            if mode == "overlapped":
                drain_overlapped()
            barrier()
            torch.cuda.synchronize(dev)
            m0 = time.perf_counter()
            for _ in range(args.mode_steps):
                mstep()
            if mode == "overlapped":
                drain_overlapped()
            torch.cuda.synchronize(dev)
            barrier()
            mt = torch.tensor([time.perf_counter() - m0], dtype=torch.float64, device=dev)
            dist.all_reduce(mt, op=dist.ReduceOp.MAX)
            mt = float(mt.item())
            rc_m = ctx.encode_result()[0]
            assert rc_m == 0 and ctx.decode_result()[:3] == (0, F, 0), mode
            gather_modes[mode] = {"ms_per_step": round(mt / args.mode_steps * 1e3, 4),
                                  "value": round(n * world * args.mode_steps / mt / 1e6, 2), "steps": args.mode_steps, "is_value": False}
        if rank == 0 and gather_mode not in ("none", "sharded"):
            # (the reassembled stream of the last mode run is rank 0's sub-stream followed by the others')
            assert torch.equal(whole_buf(starts[-1]).t[starts[0]:starts[1]], out[:pos])
        # ---- the sharded file: every rank finds its own sub-stream at its own offset; rank 0 holds the whole file against
        # the oracle's encoding of the whole signal (--verify-gather)
        if shard_file["fd"] >= 0:
            barrier()
            mine = np.frombuffer(os.pread(shard_file["fd"], lens_h[rank], starts[rank]), dtype=np.uint8)
            assert mine.size == lens_h[rank] and np.array_equal(mine, out[:pos].cpu().numpy()), "rank %d: its part of the sharded file" % rank
            sharded_ok = None
            if rank == 0:
                assert os.fstat(shard_file["fd"]).st_size == starts[-1], (os.fstat(shard_file["fd"]).st_size, starts[-1])
                if args.verify_gather:
                    tot_n = args.total_samples if args.strong else n * world
                    rc_o, ref, _ = O.encode(x3hip.synth(args.kind, SEED, 0, tot_n))
                    whole_f = np.frombuffer(os.pread(shard_file["fd"], starts[-1], 0), dtype=np.uint8)
                    sharded_ok = bool(rc_o == 0 and np.array_equal(ref, whole_f))
                    assert sharded_ok, "the sharded file differs from the oracle's encoding of the whole signal"
            gather["sharded_file"] = {"bytes": int(starts[-1]), "every_rank_verified_its_part": True,
                                      "whole_file_verified_vs_oracle": sharded_ok,
                                      "pattern": "x3_shard_write_at: D2H over each rank's own host link + pwrite at x3_shard_offsets[rank]"}
            barrier()
            os.close(shard_file["fd"])
            if rank == 0 and not args.gather_file:
                os.unlink(shard_file["path"])

    # ---- CPU baseline: the oracle (port of the reference algorithm), 1 thread, bounded sample
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        m = min(args.cpu_sample, n)
        sample = wav[:m].cpu().numpy()
        OL = native_oracle(O.Params)
        po = O.Params.default()
        es, ds, sl = C.c_double(0), C.c_double(0), C.c_uint64(0)
        rc = OL.x3o_time_roundtrip(sample.ctypes.data, m, C.byref(po), args.cpu_reps, C.byref(es), C.byref(ds),
                                   C.byref(sl))
        assert rc == 0, rc
        tot = es.value + ds.value
        cpu = {"value": round(m * args.cpu_reps / tot / 1e6, 2), "unit": "Msamples/s", "cores": 1, "kind": "port",
               "sample": "first %d samples of the same signal, %d reps, encode %.2f s + decode %.2f s; "
                         "oracle/x3_oracle.c -O3 -march=native -flto" % (m, args.cpu_reps, es.value, ds.value),
               "encode_msamples_s": round(m * args.cpu_reps / es.value / 1e6, 2),
               "decode_msamples_s": round(m * args.cpu_reps / ds.value / 1e6, 2)}
        # the generous baseline: the same port, frame-parallel over all host cores -- every
        # thread round-trips its own slice of whole frames (ctypes releases the GIL)
        import threading
        ncores = os.cpu_count() or 1
        if ncores > 1 and args.cpu_reps > 0:
            spf = 10000
            per = max(spf, (m // ncores) // spf * spf)
            parts = [sample[i * per:(i + 1) * per] for i in range(ncores) if (i + 1) * per <= m]
            rcs = [0] * len(parts)
            # a few seconds of wall time: assume the whole machine manages ~16x the single-thread rate just
            # measured (memory-bound port, SMT siblings), never more than the thread count
            agg = cpu["value"] * 1e6 * min(ncores, 16)
            reps_mt = max(1, int(4.0 * agg / (len(parts) * per) + 0.5))

            def work(i):
                e, d, l = C.c_double(0), C.c_double(0), C.c_uint64(0)
                rcs[i] = OL.x3o_time_roundtrip(parts[i].ctypes.data, parts[i].size, C.byref(po), reps_mt,
                                               C.byref(e), C.byref(d), C.byref(l))
            th = [threading.Thread(target=work, args=(i,)) for i in range(len(parts))]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            wall = time.perf_counter() - t0
            assert not any(rcs), rcs
            cpu["all_cores"] = {"value": round(sum(q.size for q in parts) * reps_mt / wall / 1e6, 2),
                                "unit": "Msamples/s", "cores": len(parts),
                                "sample": "%d slices of %d samples, %d reps, %.2f s wall" % (len(parts), per, reps_mt, wall)}

    # ---- the host-buffer entry points (x3_encode / x3_decode_stream): pageable host memory in, PCIe both ways,
    # internal staging; reported beside the headline, never as `value`
    host_api = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # caller-owned pageable buffers, allocated and touched beforehand (a caller that streams audio has
        # them already); first call = cold (device scratch is allocated), second = steady state
        L = x3hip.lib()
        hwav = wav.cpu().numpy()
        hcap = L.x3_encode_bound(n, C.byref(p))
        hout = np.zeros(hcap, dtype=np.uint8); hout[::4096] = 1
        hback = np.zeros(n, dtype=np.int16); hback[::2048] = 1
        hpos, hn, hok, herr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        hstats = np.zeros(6, dtype=np.uint64)
        def host_round_trip():
            t0 = time.perf_counter()
            rc = L.x3_encode(ctx._h, hwav.ctypes.data, n, 1, C.byref(p), hout.ctypes.data, hcap, 0, C.byref(hpos),
                             hstats.ctypes.data)
            t1 = time.perf_counter()
            rc2 = L.x3_decode_stream(ctx._h, hout.ctypes.data, hpos.value, C.byref(p), hback.ctypes.data, n, C.byref(hn),
                                     C.byref(hok), C.byref(herr))
            t2 = time.perf_counter()
            assert rc == 0 and rc2 == 0 and hn.value == n, (rc, rc2, hn.value)
            return (t1 - t0, t2 - t1)
        # first call = cold (device scratch is allocated); then four steady calls, the median one is reported (long
        # buffers go through in chunks, uploads beside downloads, and one decode call in three is 5 ms slower than the
        # others: DESIGN.md section 5); last, one call with the buffers in one piece (option host_chunk_frames = -1)
        times = [host_round_trip() for _ in range(5)]
        assert np.array_equal(hback, hwav)
        ctx.set_option("host_chunk_frames", -1)
        host_round_trip()
        one_piece = host_round_trip()
        ctx.set_option("host_chunk_frames", 0)
        assert np.array_equal(hback, hwav)
        steady = sorted(times[1:], key=lambda t: t[0] + t[1])
        te, td = steady[len(steady) // 2]
        host_api = {"samples": n, "encode_ms": round(te * 1e3, 2), "decode_ms": round(td * 1e3, 2),
                    "encode_msamples_s": round(n / te / 1e6, 1), "decode_msamples_s": round(n / td / 1e6, 1),
                    "msamples_s": round(n / (te + td) / 1e6, 1),
                    "calls_ms": [[round(a * 1e3, 2), round(b * 1e3, 2)] for a, b in times[1:]],
                    "cold_call_ms": [round(times[0][0] * 1e3, 2), round(times[0][1] * 1e3, 2)],
                    "one_piece_ms": [round(one_piece[0] * 1e3, 2), round(one_piece[1] * 1e3, 2)],
                    "pcie_gb_s": round((2 * n + hpos.value) / te / 1e9, 1),
                    "note": "x3_encode + x3_decode_stream on caller-owned pageable host buffers, taken in chunks of whole "
                            "frames (uploads, kernels and downloads side by side on three host threads): the median of "
                            "four steady calls (calls_ms: encode, decode); cold_call_ms: the first call (device scratch "
                            "is allocated); one_piece_ms: the same buffers in one piece (option host_chunk_frames = -1)"}
        # ---- the reference's incremental reader (X3aReader::decode_next_frame, one frame per call) over the same
        # stream as an .x3a archive in host memory: x3_reader_* decodes a window of frames ahead per launch set and
        # hands them out one by one (the loop below is a Python loop over the C entry point: ~1 us of ctypes per call)
        rc_h, ahdr = x3hip.archive_header_write(192000, p)
        assert rc_h == 0
        x3a = np.concatenate([ahdr, hout[:hpos.value]])
        rd = C.c_void_p()
        assert L.x3_reader_open_mem(ctx._h, x3a.ctypes.data, x3a.size, C.byref(rd)) == 0
        fbuf = np.zeros(65536, dtype=np.int16)
        fn_ = C.c_uint64(0)
        nf = tot = 0
        nxt, fptr, fcap, fref = L.x3_reader_next_frame, fbuf.ctypes.data, fbuf.size, C.byref(fn_)
        t0 = time.perf_counter()
        while True:
            rc = nxt(rd, fptr, fcap, fref)
            if rc or fn_.value == 0:
                break
            nf += 1
            tot += fn_.value
        t1 = time.perf_counter()
        assert rc == 0 and tot == n and nf == F and L.x3_reader_frame_errors(rd) == 0, (rc, tot, nf)
        assert np.array_equal(fbuf[:p.spf], hwav[n - p.spf:]) if n % p.spf == 0 else True
        L.x3_reader_close(rd)
        per_frame = {"frames": nf, "ms": round((t1 - t0) * 1e3, 2), "msamples_s": round(n / (t1 - t0) / 1e6, 1),
                     "us_per_call": round((t1 - t0) / max(nf, 1) * 1e6, 3),
                     "note": "x3_reader_open_mem + a loop of x3_reader_next_frame (= decode_next_frame, decodefile.rs:105-136) "
                             "over the whole stream from host memory into a host frame buffer; windows of %d frames are "
                             "checked and decoded ahead on the GPU" % ctx.get_option("reader_window_frames")}
        # ---- a FOREIGN stream resident in HBM (frame offsets unknown): GPU frame walk + check + decode
        # (the host-buffer calls above decoded the stream in chunks of other sizes: the decoder's pace controller takes a few
        # launches of THIS size to settle again -- five untimed calls, then the median of ten)
        fs_ms = []
        for _ in range(15):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r4 = ctx.decode_stream_dev(out.data_ptr(), pos, p, back.data_ptr(), n)
            fs_ms.append((time.perf_counter() - t0) * 1e3)
            assert r4 == (0, n, F, 0), r4
        assert torch.equal(back, wav)
        foreign = {"ms": round(sorted(fs_ms[5:])[5], 3), "min_ms": round(min(fs_ms[5:]), 3), "first_call_ms": round(fs_ms[0], 3),
                   "index_fast_walks": int(ctx.get_option("index_fast_walks")), "index_general_walks": int(ctx.get_option("index_general_walks")),
                   "note": "x3_decode_stream_dev on the device-resident stream: frame walk on the GPU (every byte offset "
                           "tested for a header; a clean chain is numbered by two scans and checked in one kernel, anything "
                           "else goes through the hash table and pointer doubling) + header/payload-CRC check + decode, "
                           "host wall time incl. the trips back (index summary, decode result)"}
        del hwav, hout, hback

    # ---- what the headline does not say: a fresh context's first step, the round trip with the frame walk
    # in it, and the two adversarial contents of SURVEY 8(d) -- all timed here, in this run
    cold = with_walk = extremes = layouts = None
    if rank == 0 and world == 1 and not args.no_extras:
        def timed_steps(c, fn, k):
            c.enable_kernel_timing(True); c.reset_kernel_time()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / k
            kt = {}
            for name, which in (("encode", 0), ("decode", 1), ("frame_sizes", 2), ("scan", 3), ("frame_check", 4), ("encode_dense_pass", 5)):
                ms, cnt = c.kernel_time(which)
                if cnt:
                    kt[name] = round(ms / cnt, 4)
            c.enable_kernel_timing(False)
            return dt, kt
        # (a) cold: a NEW context (own stream, no history: no pace words, no scratch), ONE step.  (Two steps of the old
        # context first: the verification above kept the host busy for seconds and the GPU's clocks have dropped.)
        step(); step()
        assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F, 0)
        # (three fresh contexts, the median one is reported: the step is dominated by the allocator, 1.5 - 4 ms by run)
        colds = []
        for _ in range(3):
            c2 = x3hip.Context(local_rank)
            def step2():
                assert c2.encode_dev(wav.data_ptr(), n, p, out.data_ptr(), cap, 0, off.data_ptr()) == 0
                assert c2.decode_dev(out.data_ptr(), cap, off.data_ptr(), F, p, back.data_ptr(), n, n_per_clip=n) == 0
                c2.sync()
            back.zero_()
            dt, kt = timed_steps(c2, step2, 1)
            assert c2.encode_result()[0] == 0 and c2.decode_result()[:3] == (0, F, 0) and torch.equal(back, wav)
            colds.append((dt, kt))
            c2.close()
        colds.sort(key=lambda x: x[0])
        dt, kt = colds[1]
        cold = {"ms_per_step": round(dt * 1e3, 4), "value": round(n / dt / 1e6, 2), "kernels_ms": kt,
                "all_ms_per_step": [round(x[0] * 1e3, 4) for x in colds],
                "note": "first encode+decode of a fresh context (scratch allocation, no launch history) on a GPU that is awake, "
                        "the median of three fresh contexts; ms_per_step is host wall time incl. the allocations, kernels_ms "
                        "the kernels alone"}
        # (b) the round trip when the decoder does not get the encoder's frame index: x3_encode_dev + x3_decode_stream_dev
        def step_walk():
            assert ctx.encode_dev(wav.data_ptr(), n, p, out.data_ptr(), cap, 0, off.data_ptr()) == 0
            r4 = ctx.decode_stream_dev(out.data_ptr(), pos, p, back.data_ptr(), n)
            assert r4 == (0, n, F, 0), r4
        for _ in range(5):   # (as above: the pace controller settles on this launch size again)
            step_walk()
        dt, kt = timed_steps(ctx, step_walk, 10)
        assert ctx.encode_result()[0] == 0 and torch.equal(back, wav)
        with_walk = {"ms_per_step": round(dt * 1e3, 4), "value": round(n / dt / 1e6, 2), "kernels_ms": kt,
                     "note": "x3_encode_dev + x3_decode_stream_dev (frame walk on the GPU, check, decode; the call returns the "
                             "summary, so every step ends with a trip to the host)"}
        # (b2) round 6: the block-per-lane decoder (x3_decode_blocks_kernel.h, option decode_blocks) beside the default
        # three-wave kernel, same stream, same step -- the design VERDICT r5 asked for, built, bit-exact, and slower
        def step_plain():
            assert ctx.encode_dev(wav.data_ptr(), n, p, out.data_ptr(), cap, 0, off.data_ptr()) == 0
            assert ctx.decode_dev(out.data_ptr(), cap, off.data_ptr(), F, p, back.data_ptr(), n, n_per_clip=n) == 0
        decoder_kernels = {}
        for name, opt in (("three_wave", 0), ("block_per_lane", 1)):
            ctx.set_option("decode_blocks", opt)
            back.zero_()
            for _ in range(5):
                step_plain()
            dt, kt = timed_steps(ctx, step_plain, 10)
            assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F, 0) and torch.equal(back, wav)
            decoder_kernels[name] = {"decode_ms": kt.get("decode"), "ms_per_step": round(dt * 1e3, 4)}
        ctx.set_option("decode_blocks", 0)
        for _ in range(5):
            step_plain()
        ctx.decode_result()
        decoder_kernels["note"] = ("x3_decode_dev with option decode_blocks = 0 / 1; block_per_lane: a walker wave finds the block "
                                   "boundaries, three decoder waves decode a block per lane (every frame walked twice: 363 M vector "
                                   "instructions against 238 M, profiles/r6)")
        # (c) SURVEY 8(d)'s extremes on the same 691.2 M samples: minimum and maximum output
        # ... and `mixed`: config 3 with every hundredth frame full-scale noise (a ship passing the hydrophone): such frames
        # do not fit the wave encoder's LDS image and take the dense pass behind it
        extremes = {}
        for kind, name in ((0, "zeros"), (1, "white_noise"), (2, "mixed")):
            ctx.synth_dev(kind, SEED, 0, n, wav.data_ptr())
            if name == "mixed":
                for fr in range(50, F, 100):
                    lo = fr * p.spf
                    ctx.synth_dev(1, SEED + fr, lo, min(p.spf, n - lo), wav.data_ptr() + 2 * lo)
            torch.cuda.synchronize(dev)
            # (the first calls on new content run before the timed ones: the context's generation hint follows the content)
            for _ in range(3):
                step()
            rc_e, pos_e, _ = ctx.encode_result()
            assert rc_e == 0 and ctx.decode_result()[:3] == (0, F, 0)
            dt, kt = timed_steps(ctx, step, 10)
            rc_e, pos_e, _ = ctx.encode_result()
            assert rc_e == 0 and ctx.decode_result()[:3] == (0, F, 0) and torch.equal(back, wav), name
            offs_e = off.cpu().numpy()
            for fr in sorted({0, F // 2, F - 1}):   # sampled frames against the oracle
                enc = O.encode(wav[fr * p.spf:min(n, (fr + 1) * p.spf)].cpu().numpy())[1]
                assert np.array_equal(enc, out[int(offs_e[fr]):int(offs_e[fr + 1])].cpu().numpy()), (name, fr)
            extremes[name] = {"ms_per_step": round(dt * 1e3, 4), "value": round(n / dt / 1e6, 2), "kernels_ms": kt,
                              "bytes_per_sample": round(pos_e / n, 4), "encoder_generation": int(ctx.get_option("enc_gen_in_use")),
                              "dense_frames": int(ctx.get_option("last_dense_frames"))}
        extremes["encoder"] = {"dense_reruns": int(ctx.get_option("encode_dense_reruns")),
                               "note": "frames whose payload does not fit the wave encoder's LDS image (> 9 728 bytes) are written by the "
                                       "dense pass behind it in the same stream (kernels_ms.encode_dense_pass; mixed: every hundredth "
                                       "frame); no call is encoded twice.  A call with more than a quarter of such frames makes the "
                                       "context's next call start on the second-generation kernel (white noise: encoder_generation 2)"}

        # (d) layouts one step away from config 3's (round 4): the same samples in frames of 501 blocks (every other frame
        # on an 8-byte boundary) and 256 blocks, and as a batch of fifteen-second 44.1 kHz clips side by side (661 500 samples
        # each: a short last frame per clip, groups of 64 frames that span clips, rows on 8-byte boundaries)
        layouts = {}
        ctx.synth_dev(args.kind, SEED, 0, n, wav.data_ptr())
        torch.cuda.synchronize(dev)
        for name, bpf, npc in (("blocks_501", 501, n), ("blocks_256", 256, n), ("clips_15s_44k1", 500, 661_500)):
            pl_ = x3hip.Params.make(20, bpf)
            n_clips = n // npc
            n_l = npc * n_clips
            F_l = L.x3_num_frames(npc, C.byref(pl_)) * n_clips
            cap_l = L.x3_encode_bound(npc, C.byref(pl_)) * n_clips
            out_l = out if cap_l <= cap else torch.empty(cap_l + 16, dtype=torch.uint8, device=dev)
            off_l = off if F_l <= F else torch.empty(F_l + 1, dtype=torch.int64, device=dev)

            def step_l():
                assert ctx.encode_dev(wav.data_ptr(), npc, pl_, out_l.data_ptr(), cap_l, 0, off_l.data_ptr(), n_clips=n_clips,
                                      clip_stride=npc) == 0
                assert ctx.decode_dev(out_l.data_ptr(), cap_l, off_l.data_ptr(), F_l, pl_, back.data_ptr(), n_l, n_per_clip=npc,
                                      n_clips=n_clips, clip_stride=npc) == 0
            back.zero_()
            for _ in range(3):
                step_l()
            assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F_l, 0)
            dt, kt = timed_steps(ctx, step_l, 10)
            assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F_l, 0) and torch.equal(back[:n_l], wav[:n_l]), name
            layouts[name] = {"ms_per_step": round(dt * 1e3, 4), "value": round(n_l / dt / 1e6, 2), "kernels_ms": kt, "frames": int(F_l),
                             "encoder_generation": int(ctx.get_option("enc_gen_in_use"))}
        layouts["note"] = ("config 3's samples in other layouts, encode + decode per step as in `value`: frames of 501 / 256 blocks "
                           "instead of 500; 1 044 clips of 661 500 samples (15 s at 44.1 kHz) side by side at stride = length")

    # ---- BASELINE configs 2 and 5, timed (they had parity tests and no number anywhere): the same entry
    # points as the step (x3_encode_dev, x3_decode_dev from the encoder's frame index) and the foreign-stream decode
    # (x3_decode_stream_dev), wall time per call over back-to-back calls between two synchronisations, the kernels' own
    # HIP-event times beside it, the round trip checked for identity and sampled frames against the oracle.
    configs = None
    if rank == 0 and world == 1 and not args.no_extras and not args.no_configs:
        configs = {}
        for cname, n_per, n_clips, reps in (("config2", 26_460_000, 1, 20), ("config5", 5_760_000, 1000, 5)):
            n_c = n_per * n_clips
            free_b, _tot = torch.cuda.mem_get_info(dev)
            if free_b < 5.2 * n_c + (2 << 30):
                configs[cname] = {"skipped": "needs %.1f GB of free HBM, %.1f free" % (5.2 * n_c / 1e9, free_b / 1e9)}
                continue
            F_c = L.x3_num_frames(n_per, C.byref(p)) * n_clips
            cap_c = int(n_c * 0.75) + 4096 if n_clips > 1 else L.x3_encode_bound(n_per, C.byref(p))
            wav_c = torch.empty(n_c, dtype=torch.int16, device=dev)
            out_c = torch.empty(cap_c + 16, dtype=torch.uint8, device=dev)
            off_c = torch.empty(F_c + 1, dtype=torch.int64, device=dev)
            back_c = torch.zeros(n_c, dtype=torch.int16, device=dev)
            if n_clips == 1:
                ctx.synth_dev(args.kind, 0x58330002, 0, n_per, wav_c.data_ptr())
            else:
                for c_ in range(n_clips):   # (the clips of tests/test_gpu_parity.py::test_full_size_config5_batch)
                    ctx.synth_dev(2 if c_ % 7 else 4, 0x58330005 + c_, 0, n_per, wav_c.data_ptr() + 2 * c_ * n_per)
            torch.cuda.synchronize(dev)

            def enc_c():
                assert ctx.encode_dev(wav_c.data_ptr(), n_per, p, out_c.data_ptr(), cap_c, 0, off_c.data_ptr(), n_clips=n_clips) == 0

            def dec_c():
                assert ctx.decode_dev(out_c.data_ptr(), cap_c, off_c.data_ptr(), F_c, p, back_c.data_ptr(), n_c, n_per_clip=n_per,
                                      n_clips=n_clips) == 0
            enc_c()
            rc_c, pos_c, _ = ctx.encode_result()
            assert rc_c == 0, (cname, rc_c, ctx.last_error())

            def fs_c():
                r4 = ctx.decode_stream_dev(out_c.data_ptr(), pos_c, p, back_c.data_ptr(), n_c)
                assert r4 == (0, n_c, F_c, 0), (cname, r4)

            def timed_calls(fn, k, kernel_ids):
                for _ in range(3):
                    fn()
                ctx.enable_kernel_timing(True); ctx.reset_kernel_time()
                torch.cuda.synchronize(dev)
                t0_ = time.perf_counter()
                for _ in range(k):
                    fn()
                torch.cuda.synchronize(dev)
                dt_ = (time.perf_counter() - t0_) / k
                kt_ = {}
                for nm_, which in kernel_ids:
                    ms_, cnt_ = ctx.kernel_time(which)
                    if cnt_:
                        kt_[nm_] = round(ms_ / cnt_, 4)
                ctx.enable_kernel_timing(False)
                return {"ms": round(dt_ * 1e3, 4), "gsamples_s": round(n_c / dt_ / 1e9, 1), "kernels_ms": kt_}
            # ... and with the SEGMENT INDEX (include/x3hip.h): the encoder leaves, for every 32nd block of every frame, the bit
            # position it begins at and the sample in front of it; the decoder then takes as many stretches of a frame side by
            # side as fill the GPU (a hint that every stretch checks against the next one's entry; frames alone fill the GPU in
            # config 5 and the index is not used there)
            SEG_SB = 32
            seg_c = torch.zeros(int(L.x3_seg_index_entries(F_c, C.byref(p), SEG_SB)) + 1, dtype=torch.int64, device=dev)

            def enc_seg_c():
                assert ctx.encode_dev_seg(wav_c.data_ptr(), n_per, p, out_c.data_ptr(), cap_c, seg_c.data_ptr(), SEG_SB, 0,
                                          off_c.data_ptr(), n_clips=n_clips) == 0

            def dec_seg_c():
                assert ctx.decode_dev_seg(out_c.data_ptr(), cap_c, off_c.data_ptr(), F_c, p, back_c.data_ptr(), n_c, seg_c.data_ptr(),
                                          SEG_SB, n_per_clip=n_per, n_clips=n_clips) == 0
            r_enc = timed_calls(enc_c, reps, (("encode", 0), ("encode_dense_pass", 5), ("frame_sizes", 2), ("scan", 3)))
            assert ctx.encode_result()[0] == 0
            r_dec = timed_calls(dec_c, reps, (("decode", 1), ("frame_check", 4)))
            assert ctx.decode_result()[:3] == (0, F_c, 0) and torch.equal(back_c, wav_c), cname
            back_c.zero_()
            r_fs = timed_calls(fs_c, reps, (("decode", 1), ("frame_check", 4)))
            assert torch.equal(back_c, wav_c), cname
            def step_c():
                enc_c(); dec_c()

            def step_seg_c():
                enc_seg_c(); dec_seg_c()
            r_step = timed_calls(step_c, reps, (("encode", 0), ("decode", 1)))
            assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F_c, 0)
            r_enc_seg = timed_calls(enc_seg_c, reps, (("encode", 0), ("encode_dense_pass", 5)))
            assert ctx.encode_result()[0] == 0
            back_c.zero_()
            r_dec_seg = timed_calls(dec_seg_c, reps, (("decode", 1), ("frame_check", 4)))
            r_dec_seg["stretches_per_frame"] = int(ctx.get_option("last_seg_stretches"))
            assert ctx.decode_result()[:3] == (0, F_c, 0) and torch.equal(back_c, wav_c), cname
            back_c.zero_()
            r_step_seg = timed_calls(step_seg_c, reps, (("encode", 0), ("decode", 1)))
            assert ctx.encode_result()[0] == 0 and ctx.decode_result()[:3] == (0, F_c, 0) and torch.equal(back_c, wav_c), cname
            # sampled frames against the oracle (first, last, a spread; config 5: frames of the first, a middle and the last clip)
            offs_c = off_c.cpu().numpy()
            assert int(offs_c[-1]) == pos_c
            fpc_c = F_c // n_clips
            sampled = sorted({0, 1, fpc_c - 1, F_c // 2, F_c - fpc_c, F_c - 1} | set(range(7, F_c, max(1, F_c // 24))))
            for fr in sampled:
                clip_, idx_ = divmod(fr, fpc_c)
                a_ = clip_ * n_per + idx_ * p.spf
                b_ = min(clip_ * n_per + n_per, a_ + p.spf)
                enc = O.encode(wav_c[a_:b_].cpu().numpy())[1]
                assert np.array_equal(enc, out_c[int(offs_c[fr]):int(offs_c[fr + 1])].cpu().numpy()), (cname, fr)
            configs[cname] = {"samples": n_c, "clips": n_clips, "frames": int(F_c), "stream_bytes": int(pos_c),
                              "bytes_per_sample": round(pos_c / n_c, 4),
                              "encode": r_enc, "decode": r_dec, "decode_stream_dev": r_fs,
                              "round_trip_ms": round(r_enc["ms"] + r_dec["ms"], 4),
                              "round_trip_gsamples_s": round(n_c / (r_enc["ms"] + r_dec["ms"]) / 1e6, 1),
                              "step": r_step,     # encode + decode per step, steps back to back (as the headline is timed)
                              "with_segment_index": {"seg_blocks": SEG_SB, "index_bytes": int(seg_c.numel() * 8),
                                                     "encode": r_enc_seg, "decode": r_dec_seg,
                                                     "round_trip_ms": round(r_enc_seg["ms"] + r_dec_seg["ms"], 4),
                                                     "round_trip_gsamples_s": round(n_c / (r_enc_seg["ms"] + r_dec_seg["ms"]) / 1e6, 1),
                                                     "step": r_step_seg},
                              "frames_verified_vs_oracle": len(sampled), "round_trip_is_identity": True}
            del wav_c, out_c, off_c, back_c, seg_c
            torch.cuda.empty_cache()
        configs["note"] = ("BASELINE configs 2 (10 min 44.1 kHz: 26.46 M samples, 2 646 frames) and 5 (1000 x 1 min 96 kHz clips in one "
                           "launch set: 5.76 G samples) on the entry points of the step: ms = host wall time per call over "
                           "back-to-back calls between two synchronisations, kernels_ms = the kernels' HIP-event times; step = encode + "
                           "decode per step, steps back to back, as `value` is timed.  A stream "
                           "of few frames cannot be faster than ONE frame's serial decode (a frame is one bit stream): 0.41 ms "
                           "from the frame index alone (DESIGN.md section 4); with_segment_index: x3_encode_dev_seg + "
                           "x3_decode_dev_seg, the frames' stretches decoded side by side")
    if rank == 0:
        total_samples = n * world
        value = total_samples * args.steps / elapsed / 1e6
        # algorithmic HBM bytes per launch (DESIGN.md "Kernels"): 2 B per sample + P stream bytes for
        # the encoder and the decoder; the size pass re-reads the samples; the check pass reads the stream
        alg = {"encode": 2 * n + pos, "decode": 2 * n + pos, "frame_sizes": 2 * n, "frame_check": pos}
        ktimes.setdefault("frame_sizes", 0.0)
        kname = {"encode": ("x3_encode_wave_kernel<false>" if enc_gen == 3 else "x3_encode_stream2_kernel<false, false>") if ktimes.get("frame_sizes", 0.0) == 0.0 else "x3_encode_frames_kernel<false, false>",
                 "decode": "x3_decode_split_kernel",
                 "frame_sizes": "x3_encode_frames_kernel<true, false>", "frame_check": "x3_frame_check_kernel"}
        alg = {k: v for k, v in alg.items() if ktimes.get(k, 0.0) > 0.0}  # the two-pass fallback kernels may not run
        # the dominant kernel of the step's critical path: the frame check runs BESIDE the decoder on a second
        # stream (its co-running time is stretched by the decoder's waves), so it is reported but not a candidate
        dominant = max((k for k in alg if k != "frame_check"), key=lambda k: ktimes[k])
        # HBM bytes per launch: two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE -- separate runs, MI355X_MICROARCH.md)
        # of the same kernels on the same workload, run here as child processes once the timing is done; the recorded
        # profiles/traffic.json when that is not possible (no rocprofv3, N > 1, already under a profiler)
        traffic, traffic_source = {}, None
        if world == 1 and not args.no_measure_traffic:
            traffic, traffic_source = measure_traffic(n, args.kind)
        if not traffic:
            why = traffic_source
            try:
                traffic = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
                traffic_source = "profiles/traffic.json (rocprofv3 PMC passes of this workload, recorded; not measured in this run%s)" % (
                    ": " + why if why else "")
            except Exception:
                traffic, traffic_source = {}, "none"

        def roof(k):
            t = ktimes[k] / 1e3
            ach = alg[k] / t / 1e9
            r = {"bound": "hbm", "kernel": kname[k], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                 "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                 "traffic": traffic.get(kname[k], {}).get("hbm_bytes_per_launch"),
                 "traffic_source": traffic_source,
                 "sq_per_launch": traffic.get(kname[k], {}).get("sq_per_launch"),
                 "algorithmic_bytes": int(alg[k]), "avg_launch_ms": round(ktimes[k], 4)}
            # the wall these kernels actually stand at: vector-instruction issue.  MEASURED (tools/ubench/valu_rate, profiles/r2/
            # valu_rate.txt): a full SIMD retires one 64-bit-encoded vector instruction (VOP3 / VOP3P: v_alignbit, v_bfe, v_mad, v_bfi,
            # v_perm, v_pk_*) per 1.8 ns and one 32-bit-encoded (VOP1 / VOP2) per 1.27 ns, at six waves per SIMD; one wave alone gets one
            # per ~3.8 ns, a dependent chain one per ~8.5 clocks (tools/ubench/issue_cost).  These kernels are ~80 % 64-bit encodings.
            insts = (r["sq_per_launch"] or {}).get("SQ_INSTS_VALU")
            mhz = (clocks.get("decode_kernel_mhz" if k in ("decode", "frame_check") else "encode_kernel_mhz") or {}).get("median")
            if insts and mhz:
                clk = t * mhz * 1e6 * 1024.0        # SIMD-clocks of the launch
                r["valu_issue"] = {"insts": int(insts), "lane_insts_per_sample": round(insts * 64.0 / n, 2),
                                   "simd_clocks_per_inst": round(clk / insts, 2),
                                   "frac_of_peak": round(insts * 1.8e-9 / (1024.0 * t), 4),
                                   "peak": "one 64-bit-encoded vector instruction per 1.8 ns and SIMD (measured, profiles/r2/valu_rate.txt), 1 024 SIMDs",
                                   "note": "frac_of_peak = SQ_INSTS_VALU x 1.8 ns / (1 024 SIMDs x launch time): the share of the SIMDs' "
                                           "measured vector issue rate the kernel uses.  The decode kernels are bound by it and by the "
                                           "LATENCY of one frame's serial walk (a lone wave: one dependent instruction per ~8.5 clocks), "
                                           "not by HBM: round 6 measured both walls (profiles/r6/decoder_blocks_kernel.txt)"}
            return r
        secs = n / 192000.0
        kinds = {0: "all zeros", 1: "white noise", 2: "hydrophone-like noise", 3: "sine", 4: "random walk"}
        if n == N_SAMPLES:
            workload = "config 3: 1 h 192 kHz mono %s, encode+decode round trip per GPU" % kinds.get(args.kind, "?")
        else:
            workload = "%d samples (%.1f s at 192 kHz) mono %s, encode+decode round trip per GPU -- NOT config 3's size" % (
                n, secs, kinds.get(args.kind, "?"))
        if world == 1:
            sharding = "one GPU"
        elif args.strong:
            sharding = "strong: one stream of %d samples cut into %d contiguous frame ranges (config 4 = 8 h over 8 GPUs)" % (args.total_samples, world)
        else:
            sharding = "weak: every rank encodes+decodes its own hour (N = 8 is config 4)"
        if world > 1:
            sharding += "; per step: all-gather of the sub-stream lengths" + ("" if not gather_in_step else " + reassembly of the whole stream on rank 0")
        res = {
            "metric": "Msamples/s encode+decode (bit-exact), 1h 192kHz mono; % HBM-read roofline",
            "value": round(value, 2),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak",
            "vs_baseline": None,
            "dtype": "i16",
            "data": "synthetic",
            "config": {"workload": workload,
                       "samples_per_gpu": n, "frames_per_gpu": int(F), "stream_bytes_per_gpu": int(pos),
                       "bytes_per_sample": round(pos / n, 4), "block_len": 20, "blocks_per_frame": 500,
                       "signal_kind": args.kind, "frames_verified_vs_oracle": int(verified),
                       "settle_steps": args.settle + settle["steps"],  # extra untimed launches in front of the warm-up
                       "settle_ms": round(settle["ms"], 1), "settle_settled": settle["settled"],
                       "settle_clock_mhz": settle["clock_mhz"][-64:],
                       "settle_note": "time-based settle in front of the W warm-up steps: steps in batches of eight until the "
                                      "shader clock the decode kernel logs has stayed within 2.5 % of its running maximum for "
                                      "eight launches, bounded by --settle-ms (default 500); untimed",
                       "sharding": sharding},
            "roofline": roof(dominant),
            "roofline_all": {k: roof(k) for k in alg},
            "encode_read_frac": round(2 * n / (ktimes["encode"] / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
            "value_without_kernel_events": round(n * world / elapsed_untimed * args.steps / 1e6, 2),
            "value_with_all_kernel_events": round(n * world / elapsed_all_events * args.steps / 1e6, 2),
            "ms_per_step_without_kernel_events": round(elapsed_untimed / args.steps * 1e3, 4),
            "kernels_ms": {k: round(v, 4) for k, v in ktimes.items()},
            "kernels_ms_stats": {k: kstats(v) for k, v in ksteps.items()},
            "kernels_ms_steps": {k: [round(x, 4) for x in v] for k, v in ksteps.items() if k in ("encode", "decode", "frame_check")},
            "clocks": clocks,
            "decoder_pace": decoder_pace,
            "cpu_baseline": cpu,
        }
        if cold is not None:
            res["decoder_kernels"] = decoder_kernels
            res["cold"] = cold
            res["value_with_frame_walk"] = with_walk["value"]
            res["with_frame_walk"] = with_walk
            res["extremes"] = extremes
            res["layouts"] = layouts
        if configs is not None:
            res["configs"] = configs
        if host_api is not None:
            res["host_buffer_api"] = host_api
            res["per_frame_api"] = per_frame
            res["foreign_stream"] = foreign
            res["foreign_stream_ms"] = foreign["ms"]
        if gather is not None:
            if gather["in_timed_region"]:
                # derived, for the reader who wants the compute alone beside the contract's `value`: one rank cannot take in
                # N sub-streams as fast as N GPUs produce them (a stream leaves a GPU at ~270 GB/s, an xGMI link carries ~60)
                rest = max(elapsed / args.steps - gather["ms"] / 1e3, 1e-9)
                gather["step_ms_without_gather"] = round(rest * 1e3, 4)
                gather["value_without_gather"] = round(total_samples / rest / 1e6, 2)
            res["gather"] = gather
            res["gather_modes"] = gather_modes
            res["rccl_ranks"] = world
            res["rccl"] = rccl
        if placement is not None:
            res["placement"] = placement
        if dump_info is not None:
            res["dump_outputs"] = dump_info
        # ONE line on stdout, as the contract says, and short (<= 4 KB, so that the tail of the driver's
        # record holds every number it judges by: kernels_ms, encode_read_frac, roofline_all, the clocks, the CPU baseline,
        # configs 2 and 5); everything else -- notes, per-step arrays, the wider measurements -- goes to a FILE beside it
        # (--details, default bench_details.json in the working directory; "-" = a second line on stderr).
        if args.details == "-":
            print(json.dumps({"bench_details": res}), file=sys.stderr, flush=True)
        elif args.details:
            try:
                with open(args.details, "w") as fh:
                    json.dump({"bench_details": res}, fh)
            except OSError as e:
                print("bench.py: cannot write %s: %s" % (args.details, e), file=sys.stderr)
        print(json.dumps(compact_line(res)), flush=True)

    if shard_obj is not None:
        shard_obj.close()
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
