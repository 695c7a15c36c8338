"""Which kernel a decode or encode call takes, on the CPU: tests/host_cpp/test_routes.cpp calls the library's decode_route
and encode_route (x3_internal.h) over a grid of Rice code sets, thresholds, block lengths, frame lengths, clip strides,
pointer alignments, offsets, segment-index modes and options, and checks each answer against the rules it writes out
(those of expected_kernel and expected_gen in tests/test_gpu_code_sets.py, extended to layouts and options).  The
library's translation units are compiled as tests/test_host_sanitized.py compiles them (the registration of their kernels
needs the code objects) and linked with the driver, which is host code only; nothing creates a context."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "x3-rust_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ["x3_ctx", "x3_encode", "x3_decode", "x3_files", "x3_mgpu"]
DRIVER = os.path.join(ROOT, "tests", "host_cpp", "test_routes.cpp")
FLAGS = ["--offload-arch=gfx950", "-O1", "-g0", "-std=c++17", "-Wno-unused-function", "-pthread"]


def _newest_source(driver):
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "include", "x3hip.h"), driver]
    return max(os.path.getmtime(s) for s in srcs)


def build_driver(driver, name):
    """The library's units and a host-only driver, linked to tests/host_cpp/_routes/<name>: rebuilt when a source is newer.
    (Every driver links unit objects of its own, <name>_<unit>.o, so two drivers built side by side share no file.)"""
    out = os.path.join(ROOT, "tests", "host_cpp", "_routes")     # (git-ignored)
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < _newest_source(driver):
        objs = [os.path.join(out, "%s_%s.o" % (name, u)) for u in UNITS]

        def cc(u, o):
            subprocess.run([HIPCC] + FLAGS + ["-c", "-o", o, os.path.join(CSRC, u + ".hip")], check=True, capture_output=True)
        with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
            list(ex.map(cc, UNITS, objs))
        drv = os.path.join(out, name + "_driver.o")
        subprocess.run([HIPCC] + FLAGS + ["--cuda-host-only", "-x", "hip", "-I", CSRC, "-c", "-o", drv, driver],
                       check=True, capture_output=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-pthread", "-o", exe, drv] + objs, check=True, capture_output=True)
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_decode_and_encode_routes():
    exe = build_driver(DRIVER, "test_routes")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok decode="), (r.stdout[-4000:], r.stderr[-2000:])
    counts = dict(kv.split("=") for kv in r.stdout.split()[1:])
    assert int(counts["decode"]) >= 100000 and int(counts["encode"]) >= 1000000, counts
