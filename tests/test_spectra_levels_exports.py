"""The band levels entry point in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the
layout of x3_spectra_fold in all of them.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import x3hip
from test_binding_widths import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_spectra_levels_dev"]
FIELDS = [("frames_per_bin", 0, 4), ("n_bands", 4, 4), ("plane_stride", 8, 8), ("d_bin_band", 16, 8), ("reserved", 24, 8)]


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_library_exports_the_new_entry_point():
    L = x3hip.lib()
    for name in NEW:
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    vp, u64 = C.c_void_p, C.c_uint64
    # ctx, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, rule, fold, row_stride, d_levels, rows_cap,
    # d_row_offsets, d_status
    assert L.x3_spectra_levels_dev.argtypes == [vp, vp, u64, vp, vp, vp, u64, C.POINTER(x3hip.SpectraRule),
                                                C.POINTER(x3hip.SpectraFold), u64, vp, u64, vp, vp]


def test_the_argument_widths_are_the_headers():
    L, protos = x3hip.lib(), prototypes()
    for name in NEW:
        assert [C.sizeof(t) for t in getattr(L, name).argtypes] == protos[name], name
    assert protos["x3_spectra_levels_dev"] == [8] * 14


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "SPECTRA, BAND LEVELS" in header
    body = re.search(r"typedef\s+struct\s+x3_spectra_fold\s*\{(.*?)\}\s*x3_spectra_fold\s*;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == [
        "uint32_t frames_per_bin, n_bands", "uint64_t plane_stride", "const uint32_t* d_bin_band", "uint64_t reserved"]
    F = x3hip.SpectraFold
    assert C.sizeof(F) == 32
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == FIELDS
    # the library holds the same layout with a static_assert of its own
    hip = text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert "sizeof(x3_spectra_fold) == 32" in hip and "offsetof(x3_spectra_fold, d_bin_band) == 16" in hip
    assert "offsetof(x3_spectra_fold, plane_stride) == 8" in hip and "offsetof(x3_spectra_fold, reserved) == 24" in hip
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_spectra_fold\s*\{(.*?)\}", rust, flags=re.S)
    assert rm and [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()] == \
        ["pub frames_per_bin: u32", "pub n_bands: u32", "pub plane_stride: u64", "pub d_bin_band: *const u32", "pub reserved: u64"]


def test_the_mirrors_declare_it():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
    assert re.search(r"x3_spectra_levels_dev\([^;]*const int32_t\* d_in_status, uint64_t n_ranges, const x3_spectra_rule\* rule,\s+"
                     r"const x3_spectra_fold\* fold, uint64_t row_stride, x3_level\* d_levels, uint64_t rows_cap,\s+"
                     r"uint64_t\* d_row_offsets, int32_t\* d_status\);", header)
    assert re.search(r"pub fn x3_spectra_levels_dev\([^;]*rule: \*const x3_spectra_rule,\s+fold: \*const x3_spectra_fold,[^;]*\) -> c_int;", rust)
    assert "struct SpectraFold {" in hpp and "inline X3Error spectra_levels(" in hpp and "inline X3Error range_band_levels(" in hpp
    assert "X3Error range_band_levels(Context& ctx, const uint32_t* d_entries" in hpp
    assert "pub fn spectra_levels<'g>(" in rust and "pub fn range_band_levels<'g>(" in rust and "pub struct SpectraFold<" in rust
    # the kernels are part of the decode unit, in a header beside the rows call's: the build is unchanged
    hip = text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert '#include "x3_spectra_levels_kernel.h"' in hip and '#include "x3_spectra_kernel.h"' in hip
    kernels = text("x3-rust_amd", "csrc", "x3_spectra_levels_kernel.h")
    assert "x3sp_transform_tiles<MT>" in kernels and "x3sp_plan(" in kernels and "x3sp_power(" in kernels   # shared, not forked


def test_the_python_mirror():
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("range_band_levels_into", "range_band_levels"):
            assert callable(getattr(cls, method)), (cls, method)
        p = inspect.signature(cls.range_band_levels).parameters
        lead = ["starts", "lens", "n_fft", "hop"] if cls is x3hip.WindowSource else ["entries", "starts", "lens", "n_fft", "hop"]
        assert list(p)[1:1 + len(lead)] == lead and p["hop"].default is None
        for name, default in (("frames_per_bin", 1), ("bands", None), ("table", None), ("padded_to", None), ("capacity", None),
                              ("sample_capacity", None)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    p = inspect.signature(x3hip.WindowSource.band_levels).parameters
    assert list(p)[1:3] == ["n_fft", "hop"] and p["frames_per_bin"].default is inspect.Parameter.empty
    assert p["frames_per_bin"].kind is inspect.Parameter.KEYWORD_ONLY and p["chunk_samples"].default == 1 << 26 and p["q"].default >= 1
    assert list(inspect.signature(x3hip.Context.spectra_levels_dev).parameters)[1:] == [
        "d_samples", "samples_cap", "d_offsets", "d_lens", "d_in_status", "n_ranges", "rule", "fold", "row_stride", "d_levels",
        "rows_cap", "d_row_offsets", "d_status"]


def test_the_band_maps():
    m, k = x3hip.spectra_bin_band(64, None)
    assert k == 33 and m.dtype == np.uint32 and m.tolist() == list(range(33))
    m, k = x3hip.spectra_bin_band(64, [2, 5, 5, 9])                        # edges: three bands, the second without a bin
    assert k == 3 and m.tolist() == [0xFFFFFFFF] * 2 + [0] * 3 + [2] * 4 + [0xFFFFFFFF] * 24
    wild = np.full(33, 0xFFFFFFFF, dtype=np.uint32)
    wild[4], wild[30] = 6, 1
    m, k = x3hip.spectra_bin_band(64, wild)                                # an array of B words: as it is
    assert k == 7 and np.array_equal(m, wild)
    assert x3hip.spectra_bin_band(64, wild.view(np.int32))[1] == 7         # (the bits of a torch tensor)
    for bad in ([3], [5, 2], [0, 34], [-1, 4], list(range(35)), np.zeros((2, 33), dtype=np.int32), [0.5, 2.0],
                np.full(33, 0xFFFFFFFF, dtype=np.uint32)):
        with pytest.raises(ValueError):
            x3hip.spectra_bin_band(64, bad)


def test_third_octave_edges():
    """centres 1 000 * 2^(i / 3) Hz; a bin belongs to the band that holds its centre frequency"""
    for n_fft, rate, lo, hi in ((256, 48000, 200, 20000), (1024, 96000, 100, 40000), (64, 16000, 800, 6400)):
        e = x3hip.band_edges_third_octave(n_fft, rate, lo, hi)
        assert e == sorted(e) and 0 <= e[0] and e[-1] <= n_fft // 2 + 1 and len(e) >= 2
        df = rate / n_fft
        i0 = int(np.ceil(3 * np.log2(lo / 1000) - 1e-9))
        for b in range(len(e) - 1):
            f_lo, f_hi = 1000 * 2 ** ((2 * (i0 + b) - 1) / 6), 1000 * 2 ** ((2 * (i0 + b) + 1) / 6)
            for k in range(e[b], e[b + 1]):
                assert f_lo - 1e-6 <= k * df < f_hi + 1e-6, (n_fft, b, k)
        m, k = x3hip.spectra_bin_band(n_fft, e)
        assert k == len(e) - 1
    e = x3hip.band_edges_third_octave(256, 48000, 1000, 1000)              # one band: 891 .. 1 122 Hz, bins 5 (937.5 Hz) only
    assert e == [5, 6]
    with pytest.raises(ValueError):
        x3hip.band_edges_third_octave(256, 48000, 30000, 40000)
    with pytest.raises(ValueError):
        x3hip.band_edges_third_octave(256, 48000, 0, 100)


def test_the_call_refuses_a_bad_rule_without_a_device():
    """the first checks need no GPU: a NULL context, rule or fold is X3_ERR_BAD_ARG"""
    L = x3hip.lib()
    assert L.x3_spectra_levels_dev(None, None, 0, None, None, None, 1, None, None, 0, None, 1, None, None) == x3hip.ERR_BAD_ARG
