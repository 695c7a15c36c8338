"""The plane events entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the
layout of x3_plane_event_rule in all of them.  CPU only."""
import ctypes as C
import inspect
import os
import re

import pytest

import x3hip
from test_binding_widths import prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_plane_events_dev", "x3_corpus_plane_events_dev"]
FIELDS = [("n_planes", 0, 4), ("min_planes", 4, 4), ("join_bins", 8, 4), ("min_bins", 12, 4), ("pad_bins", 16, 4),
          ("max_bins", 20, 4), ("reserved", 24, 8), ("mean_sq_min", 32, 64), ("peak_min", 96, 32)]


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_events_result"]:                                   # (x3_events_result serves the new calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    vp, u64 = C.c_void_p, C.c_uint64
    rule = C.POINTER(x3hip.PlaneEventRule)
    # ctx, d_levels, plane_stride, n_bins, bin_len, d_total, rule, d_thr, d_starts, d_lens, d_event_planes, d_event_levels, cap, d_count
    assert L.x3_plane_events_dev.argtypes == [vp, vp, u64, u64, u64, vp, rule, vp, vp, vp, vp, vp, u64, vp]
    # ctx, corpus, d_levels, plane_stride, n_rows, bin_len, rule, d_thr, d_entries, d_starts, d_lens, d_event_planes, ...
    assert L.x3_corpus_plane_events_dev.argtypes == [vp, vp, vp, u64, u64, u64, rule, vp, vp, vp, vp, vp, vp, u64, vp]


def test_the_argument_widths_are_the_headers():
    L, protos = x3hip.lib(), prototypes()
    for name in NEW:
        assert [C.sizeof(t) for t in getattr(L, name).argtypes] == protos[name], name
    # the events call's arguments with plane_stride, d_thr and d_event_planes laid in
    ev, pe = protos["x3_events_dev"], protos["x3_plane_events_dev"]
    assert len(pe) == len(ev) + 3 and pe == [8] * 14
    assert len(protos["x3_corpus_plane_events_dev"]) == len(protos["x3_corpus_events_dev"]) + 3


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "PLANE EVENTS" in header and re.search(r"#define\s+X3_EVENT_PLANES_MAX\s+8\b", header)
    assert x3hip.EVENT_PLANES_MAX == 8
    body = re.search(r"typedef\s+struct\s+x3_plane_event_rule\s*\{(.*?)\}\s*x3_plane_event_rule\s*;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert fields == ["uint32_t n_planes", "uint32_t min_planes", "uint32_t join_bins, min_bins, pad_bins, max_bins",
                      "uint32_t reserved[2]", "uint64_t mean_sq_min[X3_EVENT_PLANES_MAX]", "uint32_t peak_min[X3_EVENT_PLANES_MAX]"]
    R = x3hip.PlaneEventRule
    assert C.sizeof(R) == 128
    assert [(n, getattr(R, n).offset, getattr(R, n).size) for n, _ in R._fields_] == FIELDS
    # the library holds the same layout with a static_assert of its own
    hip = text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert "sizeof(x3_plane_event_rule) == 128" in hip and "offsetof(x3_plane_event_rule, peak_min) == 96" in hip
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_plane_event_rule\s*\{(.*?)\}", rust, flags=re.S)
    assert rm and [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()] == \
        ["pub n_planes: u32", "pub min_planes: u32", "pub join_bins: u32", "pub min_bins: u32", "pub pad_bins: u32",
         "pub max_bins: u32", "pub reserved: [u32; 2]", "pub mean_sq_min: [u64; 8]", "pub peak_min: [u32; 8]"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_plane_event_rule\* rule,\s+const x3_event_threshold\* d_thr,[^;]*"
                         r"uint32_t\* d_event_planes, x3_level\* d_event_levels,\s+uint64_t cap, uint64_t\* d_count\);" % name,
                         header), name
        assert re.search(r"pub fn %s\([^;]*rule: \*const x3_plane_event_rule,[^;]*\) -> c_int;" % name, rust), name
    assert "struct PlaneEventRule {" in hpp and "inline X3Error plane_events(" in hpp and "X3Error plane_events(Context& ctx" in hpp
    assert "pub fn plane_events<'g>(" in rust and "pub fn corpus_plane_events<'g>(" in rust
    assert "pub type PlaneEventRule = ffi::x3_plane_event_rule;" in rust


def test_the_rule_and_the_python_mirror():
    r = x3hip.PlaneEventRule.make(mean_sq_min=[5, 0, 7], peak_min=[0, 9, 0], min_planes=2, join_bins=4, min_bins=1, pad_bins=2,
                                  max_bins=6)
    assert (r.n_planes, r.min_planes, r.join_bins, r.min_bins, r.pad_bins, r.max_bins) == (3, 2, 4, 1, 2, 6)
    assert list(r.mean_sq_min) == [5, 0, 7, 0, 0, 0, 0, 0] and list(r.peak_min) == [0, 9, 0, 0, 0, 0, 0, 0]
    assert list(r.reserved) == [0, 0]
    r = x3hip.PlaneEventRule.make(peak_min=[1] * 8)
    assert r.n_planes == 8 and r.min_planes == 1 and not any(r.mean_sq_min)
    r = x3hip.PlaneEventRule.make(n_planes=4, min_planes=3)                      # a rule for thresholds per entry
    assert r.n_planes == 4 and not any(r.mean_sq_min) and not any(r.peak_min)
    for bad in (dict(), dict(peak_min=[1] * 9), dict(mean_sq_min=[1, 2], peak_min=[1]), dict(peak_min=[1], n_planes=2)):
        with pytest.raises(ValueError):
            x3hip.PlaneEventRule.make(**bad)
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("plane_events_into", "plane_events", "bank_events", "adaptive_bank_events"):
            assert callable(getattr(cls, method)), (cls, method)
        p = inspect.signature(cls.plane_events).parameters
        assert list(p)[1:5] == ["levels", "bin_len", "rule", "capacity"] and p["thresholds"].kind is inspect.Parameter.KEYWORD_ONLY
        assert list(inspect.signature(cls.bank_events).parameters)[1:] == ["bin_len", "tones", "rule", "capacity"]
        assert list(inspect.signature(cls.adaptive_bank_events).parameters)[1:] == ["bin_len", "tones", "threshold_rule", "rule",
                                                                                   "capacity"]
    for name in ("plane_events_dev", "corpus_plane_events_dev"):
        assert "plane_stride" in inspect.signature(getattr(x3hip.Context, name)).parameters
