"""bench.py is what the driver runs at the end of a round: keep it runnable.

CPU: the script compiles and no function uses a name as a local before binding it (the classic way an
`import x as C` inside a function breaks an earlier use of the module-level C).
GPU: one small run end to end, and the JSON line carries every key of the contract."""
import ast
import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bench_has_no_function_local_shadowing_of_module_imports():
    tree = ast.parse(open(BENCH).read())
    top = set()
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            top.update((a.asname or a.name).split(".")[0] for a in node.names)
    for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]:
        for node in ast.walk(fn):
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                for a in node.names:
                    name = (a.asname or a.name).split(".")[0]
                    assert name not in top, "bench.py: %s() re-imports module-level name %r (makes it a local)" % (fn.name, name)


@pytest.mark.gpu
def test_bench_small_run_prints_the_contract_line():
    details = os.path.join(tempfile.mkdtemp(), "bench_details.json")
    r = subprocess.run([sys.executable, BENCH, "--steps", "2", "--warmup", "1", "--samples", "20000000", "--cpu-sample",
                        "2000000", "--cpu-reps", "1", "--details", details], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    # ONE line on stdout, short enough for the tail the driver keeps of a run; the rest in a file
    assert len(lines) == 1
    last = json.loads(lines[0])
    assert len(lines[0]) <= 4000, len(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "kernels_ms", "encode_read_frac", "roofline_all"):
        assert k in last, k
    assert last["kernels_ms"]["encode"] > 0 and last["kernels_ms"]["decode"] > 0
    assert last["roofline_all"]["encode"]["frac"] > 0 and "avg_launch_ms" in last["roofline_all"]["decode"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms"):
        assert k in last["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in last["cpu_baseline"], k
    assert last["clocks_mhz"]["decode"] > 500 and last["clocks_mhz"]["encode"] > 500
    assert "step" in last["configs"]["config2"] or "skipped" in last["configs"]["config2"]
    assert last["decoder_kernels"]["three_wave"]["decode_ms"] > 0 and last["decoder_kernels"]["block_per_lane"]["decode_ms"] > 0
    # the placement probe (round 6): what it saw is in the line, the whole matrix in the details
    sm = last["placement"]["step_ms"]
    assert last["placement"]["candidates_per_buffer"] == 8 and 0 < sm["best"] <= sm["first_allocation"] <= sm["worst"]
    j = json.load(open(details))["bench_details"]
    for k in ("metric", "value", "ms_per_step"):
        assert j[k] == last[k], k
    assert len(j["placement"]["ms_per_step"]) == 8 and all(len(r) == 8 for r in j["placement"]["ms_per_step"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0 and j["vs_baseline"] is None
    assert "workload" in j["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in j["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in j["cpu_baseline"], k
    assert j["host_buffer_api"]["encode_msamples_s"] > 0
    # per-launch statistics, the kernels' own clock measurement and the decoder's pace per step
    for k in ("encode", "decode", "frame_check"):
        st = j["kernels_ms_stats"][k]
        assert st["n"] == 2 and st["min"] <= st["median"] <= st["p90"] <= st["max"] and len(j["kernels_ms_steps"][k]) == 2, (k, st)
    assert 500 < j["clocks"]["decode_kernel_mhz"]["median"] < 3000 and 500 < j["clocks"]["encode_kernel_mhz"]["median"] < 3000, j["clocks"]
    assert len(j["decoder_pace"]["target_us_per_block"]) == 2 and min(j["decoder_pace"]["achieved_us_per_block"]) > 0
    # every hundredth frame loud: the dense pass writes them, the wave encoder keeps the call
    assert j["extremes"]["mixed"]["encoder_generation"] == 3 and j["extremes"]["mixed"]["dense_frames"] == 20
    assert j["extremes"]["encoder"]["dense_reruns"] == 0
    # configs 2 and 5 are timed in the line
    for cn, frames in (("config2", 2646), ("config5", 576000)):
        c = j["configs"][cn]
        if "skipped" in c:
            continue
        assert c["frames"] == frames and c["round_trip_is_identity"] and c["frames_verified_vs_oracle"] >= 20, c
        for leg in ("encode", "decode", "decode_stream_dev"):
            assert c[leg]["ms"] > 0 and c[leg]["gsamples_s"] > 0, (cn, leg, c[leg])
        ws = c["with_segment_index"]
        assert ws["decode"]["ms"] > 0 and ws["decode"]["stretches_per_frame"] == (16 if cn == "config2" else 0), ws
    assert j["configs"]["config2"]["with_segment_index"]["decode"]["ms"] < 0.5 * j["configs"]["config2"]["decode"]["ms"]
    assert j["config"]["settle_steps"] >= 16 and j["config"]["settle_ms"] > 0
    # the same K steps without the kernels' HIP events, beside `value` (which has them in the timed region, as the contract asks)
    assert j["value_without_kernel_events"] > 0 and j["ms_per_step_without_kernel_events"] > 0
    # (the timed region carries the events of the decode phase's two kernels; the pass behind it all five kernels': what `value` was until round 5)
    assert j["value_with_all_kernel_events"] > 0 and last["value_with_all_kernel_events"] == j["value_with_all_kernel_events"]
    # roofline.traffic is measured by the run itself (two rocprofv3 PMC passes as child processes) where rocprofv3 exists
    import shutil
    if shutil.which("rocprofv3"):
        assert j["roofline"]["traffic_source"].startswith("measured in this run"), j["roofline"]["traffic_source"]
        alg = j["roofline"]["algorithmic_bytes"]
        assert 0.9 * alg < j["roofline"]["traffic"] < 1.3 * alg, (j["roofline"]["traffic"], alg)


@pytest.mark.gpu
def test_bench_distributed_path_with_one_rank():
    """the N > 1 code path (torch.distributed start-up, x3_shard over librccl: all-gather of the lengths + gather to
    rank 0 inside the step) on the one GPU a test box has: launched through torch.distributed.run with one rank"""
    env = dict(os.environ, X3_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    details = os.path.join(tempfile.mkdtemp(), "bench_details.json")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), BENCH, "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--samples", "20000000", "--no-cpu-baseline", "--no-measure-traffic", "--details", details],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    last = json.loads(lines[-1])
    assert len(lines) == 1 and len(lines[-1]) <= 4000
    # (the contract line says by itself whether RCCL saw N ranks: VERDICT r5, item 9)
    assert last["rccl"]["ranks_seen"] == 1 and last["gather"]["in_timed_region"] is True and last["kernels_ms"]["decode"] > 0
    j = json.load(open(details))["bench_details"]
    assert j["rccl_ranks"] == 1 and "x3_shard" in j["rccl"]["via"] and j["rccl"]["ranks_seen"] == 1
    assert j["gather"]["in_timed_region"] is True and j["gather"]["bytes"] == j["config"]["stream_bytes_per_gpu"]
    assert set(j["gather_modes"]) == {"in-step", "overlapped", "sharded", "none"} and j["gather_modes"]["in-step"]["is_value"] is True
    assert j["gather"]["sharded_file"]["bytes"] == j["gather"]["bytes"] and j["gather"]["sharded_file"]["every_rank_verified_its_part"]
    assert "6.5 ms" in j["gather"]["note"]
    assert j["config"]["frames_verified_vs_oracle"] == j["config"]["frames_per_gpu"]


@pytest.mark.gpu
def test_bench_starts_its_own_ranks():
    """`python3 bench.py --gpus N` without WORLD_SIZE starts torch.distributed.run as a child process before it touches the
    GPU and relays the child's line and return code; --spawn forces that path for N = 1"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--spawn", "--gpus", "1", "--steps", "2", "--warmup", "1", "--samples", "20000000",
                        "--no-cpu-baseline", "--no-measure-traffic", "--no-extras", "--place", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4000     # (the contract line, relayed from the child)
    last = json.loads(lines[0])
    assert "placement" not in last      # (--place 1: the first allocation as it comes)
    assert last["kernels_ms"]["encode"] > 0 and last["kernels_ms"]["decode"] > 0
    j = last
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["value"] > 0


def test_bench_spawn_builds_the_launcher_command(monkeypatch):
    """CPU: the self-launch happens before torch or the library is imported and hands the arguments on unchanged"""
    import importlib.util
    import subprocess as sp
    spec = importlib.util.spec_from_file_location("x3_bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}

    class _R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return _R()
    monkeypatch.setattr(sp, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "4", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("x3_bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_dump_samples_windows_within_the_budget(tmp_path):
    """CPU: --dump-outputs keeps a short output whole and a long one as seeded windows that depend on its length alone (the
    first and the last among them); outputs at every cap together stay within 64 MB, in float32 / float64"""
    import numpy as np
    import torch
    b = _bench_module()
    short = torch.arange(1000, dtype=torch.int16)
    v, starts = b.dump_sample(short, b.DUMP_DECODED_ELEMS)
    assert starts is None and torch.equal(v, short)
    g = torch.Generator().manual_seed(3)
    stream = torch.randint(0, 256, (b.DUMP_STREAM_ELEMS + 12345,), dtype=torch.uint8, generator=g)
    v, starts = b.dump_sample(stream, b.DUMP_STREAM_ELEMS)
    assert v.shape == (starts.size, b.DUMP_WINDOW) and starts.size * b.DUMP_WINDOW <= b.DUMP_STREAM_ELEMS
    assert starts[0] == 0 and starts[-1] == stream.numel() - b.DUMP_WINDOW and np.all(np.diff(starts) > 0)
    for i in (0, starts.size // 2, starts.size - 1):
        assert torch.equal(v[i], stream[starts[i]:starts[i] + b.DUMP_WINDOW])
    assert np.array_equal(b.dump_sample(stream.clone(), b.DUMP_STREAM_ELEMS)[1], starts)
    arrays = {"stream": (v, starts),
              "frame_offsets": b.dump_sample(torch.arange(b.DUMP_OFFSETS_ELEMS + 1, dtype=torch.int64) << 20, b.DUMP_OFFSETS_ELEMS),
              "decoded": b.dump_sample(torch.zeros(b.DUMP_DECODED_ELEMS + 1, dtype=torch.int16) - 7, b.DUMP_DECODED_ELEMS),
              "encode_stats": (np.arange(6, dtype=np.uint64), None)}
    info = b.write_dump(str(tmp_path / "d"), arrays)
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == [".gitignore", "decoded.npy", "decoded_window_starts.npy", "encode_stats.npy", "frame_offsets.npy",
                     "frame_offsets_window_starts.npy", "stream.npy", "stream_window_starts.npy"]
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in files) <= 64_000_000 and info["bytes"] <= 64_000_000
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in files if f.endswith(".npy")}
    assert got["stream"].dtype == np.float32 and np.array_equal(got["stream"], v.numpy().astype(np.float32))
    assert got["decoded"].dtype == np.float32 and np.all(got["decoded"] == -7)
    assert got["frame_offsets"].dtype == np.float64 and got["encode_stats"].dtype == np.float64
    assert np.array_equal(got["frame_offsets"], arrays["frame_offsets"][0].numpy().astype(np.float64))
    assert np.array_equal(got["stream_window_starts"], starts.astype(np.float64))


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_steps_outputs(tmp_path):
    """--dump-outputs: two runs with the same arguments write the same arrays, and they are what the timed path computed --
    the oracle's stream, frame offsets and block-type counts of the seeded input, and that input decoded back; --steps is the
    number of timed steps and ms_per_step is in the line"""
    import numpy as np
    import oracle_lib as O
    import x3hip
    b = _bench_module()
    n, steps = 20_000_000, 3
    dumps = []
    for run in ("a", "b"):
        d = str(tmp_path / run)
        r = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--warmup", "1", "--samples", str(n), "--no-cpu-baseline",
                            "--no-measure-traffic", "--no-extras", "--place", "1", "--details", "", "--dump-outputs", d],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        last = json.loads(lines[-1])
        assert len(lines) == 1 and last["steps"] == steps and len(last["kernels_ms"]) and last["ms_per_step"] > 0
        files = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64_000_000
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in files})
    a, b2 = dumps
    assert sorted(a) == sorted(b2) == ["decoded", "decoded_window_starts", "encode_stats", "frame_offsets", "stream",
                                       "stream_window_starts"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b2[k]), k
    wav = x3hip.synth(x3hip.SYNTH_HYDROPHONE, b.SEED, 0, n)
    rc, ref, stats = O.encode(wav)
    assert rc == 0
    offs = a["frame_offsets"].astype(np.int64)
    assert offs.size == n // 10000 + 1 and offs[0] == 0 and offs[-1] == ref.size
    assert np.array_equal(a["encode_stats"], stats.astype(np.float64))
    for name, full in (("stream", ref), ("decoded", wav)):
        starts = a[name + "_window_starts"].astype(np.int64)
        assert starts[0] == 0 and starts[-1] == full.size - b.DUMP_WINDOW
        want = full[starts[:, None] + np.arange(b.DUMP_WINDOW)]
        assert np.array_equal(a[name], want.astype(np.float32)), name


def test_bench_builds_its_cpu_baseline_outside_the_tree():
    """CPU: the CPU baseline's native oracle is compiled in a temporary directory, so that bench.py runs from a tree it
    cannot write to; oracle/ is left as it was, and the library times a round trip of the default parameters"""
    import ctypes as C
    import numpy as np
    import oracle_lib as O
    b = _bench_module()
    odir = os.path.join(ROOT, "oracle")
    before = {f: os.path.getmtime(os.path.join(odir, f)) for f in os.listdir(odir)}
    L = b.native_oracle(O.Params)
    assert {f: os.path.getmtime(os.path.join(odir, f)) for f in os.listdir(odir)} == before
    wav = (np.arange(30000) % 200 - 100).astype(np.int16)
    p = O.Params.default()
    es, ds, sl = C.c_double(0), C.c_double(0), C.c_uint64(0)
    assert L.x3o_time_roundtrip(wav.ctypes.data, wav.size, C.byref(p), 2, C.byref(es), C.byref(ds), C.byref(sl)) == 0
    assert es.value > 0 and ds.value > 0 and sl.value == O.encode(wav)[1].size
