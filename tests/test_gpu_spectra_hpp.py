"""tests/host_cpp/test_spectra_hpp.cpp: device::spectra_rows, device::range_spectra and device::Corpus::range_spectra of the
C++ mirror, built and run as tests/test_gpu_events_hpp.py builds its neighbour."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x3_hpp_spectra(tmp_path):
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_spectra_hpp.cpp")
    exe = str(tmp_path / "test_spectra_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
