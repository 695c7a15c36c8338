"""tests/host_cpp/test_spectra_levels_hpp.cpp: device::spectra_levels, device::range_band_levels and
device::Corpus::range_band_levels of the C++ mirror, built and run as tests/test_gpu_spectra_hpp.py builds its neighbour."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x3_hpp_spectra_levels(tmp_path):
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_spectra_levels_hpp.cpp")
    exe = str(tmp_path / "test_spectra_levels_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
