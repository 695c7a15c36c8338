"""The C++ mirror of the tone bank range-levels calls (x3-rust_amd/host/x3.hpp: device::tone_bank_range_levels,
device::Corpus::tone_bank_range_levels), by tests/host_cpp/test_tone_bank_range_levels_hpp.cpp against a loop over positions on
the host and against device::tone_range_levels plane by plane."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x3_hpp_tone_bank_range_levels(tmp_path):
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_tone_bank_range_levels_hpp.cpp")
    exe = str(tmp_path / "test_tone_bank_range_levels_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
