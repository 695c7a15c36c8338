"""The FIR levels entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the
Python mirror's Fir value and keyword.  CPU only."""
import ctypes as C
import inspect
import os
import re

import pytest

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_fir_levels_dev", "x3_corpus_fir_levels_dev"]


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_levels_result"]:                                   # (x3_levels_result serves the new calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    # x3_levels_dev's / x3_corpus_levels_dev's arguments and a pointer to the taps
    assert L.x3_fir_levels_dev.argtypes[:-1] == L.x3_levels_dev.argtypes
    assert L.x3_corpus_fir_levels_dev.argtypes[:-1] == L.x3_corpus_levels_dev.argtypes
    for name in NEW:
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelFir)


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "FIR LEVELS" in header and "THE HISTORY RULE" in header and "2^30" in header
    body = re.search(r"typedef\s+struct\s+x3_level_fir\s*\{(.*?)\}\s*x3_level_fir\s*;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert fields == ["uint32_t n_taps", "uint32_t shift", "int16_t taps[8]"]
    assert [(n, t) for n, t in x3hip.LevelFir._fields_] == [("n_taps", C.c_uint32), ("shift", C.c_uint32), ("taps", C.c_int16 * 8)]
    assert C.sizeof(x3hip.LevelFir) == 24
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_level_fir\s*\{(.*?)\}", rust, flags=re.S)
    assert rm and [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()] == \
        ["pub n_taps: u32", "pub shift: u32", "pub taps: [i16; 8]"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_level_fir\* fir\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*fir: \*const x3_level_fir\) -> c_int;" % name, rust), name
    assert "struct Fir {" in hpp and len(re.findall(r"WindowsResult\* res,\s+const Fir& fir\)", hpp)) == 2      # device::levels, Corpus::levels
    assert "pub fn fir_levels<'g>(" in rust and "pub fn fir_levels(&self" in rust and "pub type Fir = ffi::x3_level_fir;" in rust
    # the option table is untouched: no option speaks of the filter
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "fir" in w.split("_")]


def test_fir_and_the_keyword():
    f = x3hip.Fir([1, -2, 1])
    assert (f.taps, f.shift) == ((1, -2, 1), 0) and x3hip.level_signal(f) is f
    assert x3hip.Fir([4096] * 8, 15).c_struct().n_taps == 8 and x3hip.Fir([-32768]).taps == (-32768,)
    for taps, shift in (([], 0), ([1] * 9, 0), ([1], 16), ([1], -1), ([16384, -16384, 1], 0), ([32768], 0), ([0.5], 0)):
        with pytest.raises(ValueError):
            x3hip.Fir(taps, shift)
    with pytest.raises(AttributeError):
        f.taps = (1,)
    with pytest.raises(ValueError, match="not built yet"):
        x3hip.level_signal(f, fir=False)
    for cls in (x3hip.WindowSource, x3hip.Corpus):                       # ... and in front of any other work in the _into forms
        obj = cls.__new__(cls)
        obj._h = 1
        n_args = len(inspect.signature(cls.range_levels_into).parameters) - 2
        with pytest.raises(ValueError, match="not built yet"):
            obj.range_levels_into(*([0] * n_args), signal=f)
    assert [x3hip.level_signal(s, fir=False) for s in ("samples", "diff")] == [0, 1]
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("levels", "events", "level_quantiles", "adaptive_events", "range_levels"):
            p = inspect.signature(getattr(cls, method)).parameters["signal"]
            assert p.default == "samples" and p.kind is inspect.Parameter.KEYWORD_ONLY, (cls, method)
    for name in ("fir_levels_dev", "corpus_fir_levels_dev"):
        assert "fir" in inspect.signature(getattr(x3hip.Context, name)).parameters
