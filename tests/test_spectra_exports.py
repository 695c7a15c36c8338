"""The spectra entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the layout
of x3_spectra_rule in all of them.  CPU only."""
import ctypes as C
import inspect
import os
import re


import x3hip
from test_binding_widths import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_spectra_rows_dev", "x3_spectra_result"]
FIELDS = [("n_fft", 0, 4), ("hop", 4, 4), ("format", 8, 4), ("reserved", 12, 4), ("d_table", 16, 8)]


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW:
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    vp, u64 = C.c_void_p, C.c_uint64
    # ctx, d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, rule, row_stride, d_out, rows_cap, d_row_offsets, d_status
    assert L.x3_spectra_rows_dev.argtypes == [vp, vp, u64, vp, vp, vp, u64, C.POINTER(x3hip.SpectraRule), u64, vp, u64, vp, vp]
    assert L.x3_spectra_result.argtypes == L.x3_range_levels_result.argtypes


def test_the_argument_widths_are_the_headers():
    L, protos = x3hip.lib(), prototypes()
    for name in NEW:
        assert [C.sizeof(t) for t in getattr(L, name).argtypes] == protos[name], name
    assert protos["x3_spectra_rows_dev"] == [8] * 13 and protos["x3_spectra_result"] == protos["x3_range_levels_result"]


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "SPECTRA" in header and re.search(r"#define\s+X3_SPECTRA_SUMS\s+0\b", header) and re.search(r"#define\s+X3_SPECTRA_POWER\s+1\b", header)
    assert (x3hip.SPECTRA_SUMS, x3hip.SPECTRA_POWER) == (0, 1) and x3hip.SPECTRA_NFFTS == (64, 128, 256, 512, 1024)
    body = re.search(r"typedef\s+struct\s+x3_spectra_rule\s*\{(.*?)\}\s*x3_spectra_rule\s*;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    assert [" ".join(d.split()) for d in body.split(";") if d.strip()] == ["uint32_t n_fft, hop, format, reserved", "const int16_t* d_table"]
    R = x3hip.SpectraRule
    assert C.sizeof(R) == 24
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == FIELDS
    # the library holds the same layout with a static_assert of its own
    hip = text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert "sizeof(x3_spectra_rule) == 24" in hip and "offsetof(x3_spectra_rule, d_table) == 16" in hip
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_spectra_rule\s*\{(.*?)\}", rust, flags=re.S)
    assert rm and [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()] == \
        ["pub n_fft: u32", "pub hop: u32", "pub format: u32", "pub reserved: u32", "pub d_table: *const i16"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
    assert re.search(r"x3_spectra_rows_dev\([^;]*const int32_t\* d_in_status, uint64_t n_ranges, const x3_spectra_rule\* rule,\s+"
                     r"uint64_t row_stride, void\* d_out, uint64_t rows_cap, uint64_t\* d_row_offsets, int32_t\* d_status\);", header)
    assert re.search(r"pub fn x3_spectra_rows_dev\([^;]*rule: \*const x3_spectra_rule,[^;]*\) -> c_int;", rust)
    assert "struct SpectraRule {" in hpp and "inline X3Error spectra_rows(" in hpp and "inline X3Error range_spectra(" in hpp
    assert "X3Error range_spectra(Context& ctx, const uint32_t* d_entries" in hpp
    assert "pub fn spectra_rows<'g>(" in rust and "pub fn range_spectra<'g>(" in rust and "pub struct SpectraRule<" in rust
    # the kernels are part of the decode unit: the build is unchanged
    assert '#include "x3_spectra_kernel.h"' in text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert "v_mfma_i32_16x16x64_i8" in text("x3-rust_amd", "csrc", "x3_spectra_kernel.h")


def test_the_python_mirror():
    assert x3hip.spectra_n_rows(63, 64, 1) == 0 and x3hip.spectra_n_rows(64, 64, 7) == 1 and x3hip.spectra_n_rows(64 + 13, 64, 7) == 2
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("range_spectra_into", "range_spectra"):
            assert callable(getattr(cls, method)), (cls, method)
        p = inspect.signature(cls.range_spectra).parameters
        lead = ["starts", "lens", "n_fft", "hop"] if cls is x3hip.WindowSource else ["entries", "starts", "lens", "n_fft", "hop"]
        assert list(p)[1:1 + len(lead)] == lead and p["hop"].default is None
        for name, default in (("power", True), ("table", None), ("padded_to", None), ("capacity", None), ("sample_capacity", None)):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is default
    assert list(inspect.signature(x3hip.Context.spectra_rows_dev).parameters)[1:] == [
        "d_samples", "samples_cap", "d_offsets", "d_lens", "d_in_status", "n_ranges", "rule", "row_stride", "d_out", "rows_cap",
        "d_row_offsets", "d_status"]
    assert callable(x3hip.Context.spectra_result)


def test_the_call_refuses_a_bad_rule_without_a_device():
    """the rule's checks need no GPU: a NULL context or rule is X3_ERR_BAD_ARG"""
    L = x3hip.lib()
    assert L.x3_spectra_rows_dev(None, None, 0, None, None, None, 1, None, 0, None, 1, None, None) == x3hip.ERR_BAD_ARG
    assert L.x3_spectra_result(None, None, None, None, None) == x3hip.ERR_BAD_ARG
