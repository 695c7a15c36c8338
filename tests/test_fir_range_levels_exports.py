"""The FIR range levels entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, the
Python mirror's methods, and the old keyword's refusal.  CPU only."""
import ctypes as C
import inspect
import os
import re

import pytest

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_fir_range_levels_dev", "x3_corpus_fir_range_levels_dev"]


def text(*path):
    with open(os.path.join(ROOT, *path)) as fh:
        return fh.read()


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_range_levels_result"]:                              # (x3_range_levels_result serves the new calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    # x3_range_levels_dev's / x3_corpus_range_levels_dev's arguments and a pointer to the taps
    assert L.x3_fir_range_levels_dev.argtypes[:-1] == L.x3_range_levels_dev.argtypes
    assert L.x3_corpus_fir_range_levels_dev.argtypes[:-1] == L.x3_corpus_range_levels_dev.argtypes
    for name in NEW:
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelFir)


def test_the_header_and_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    assert "FIR RANGE LEVELS" in header and "LEAD FRAMES" in header and "it does not filter the cut" in header
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_level_fir\* fir\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*fir: \*const x3_level_fir\) -> c_int;" % name, rust), name
    # the Fir goes in front of the result pointer: device::fir_range_levels and Corpus::fir_range_levels
    assert len(re.findall(r"const Fir& fir,\s+RangeLevelsResult\* res\)", hpp)) == 2
    assert "inline X3Error fir_range_levels(" in hpp and "  X3Error fir_range_levels(" in hpp
    assert "pub fn fir_range_levels<'g>(" in rust and "pub fn fir_range_levels(&self" in rust
    # the option table is untouched: no option speaks of the filter
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "fir" in w.split("_")]


def test_the_python_methods():
    for name in ("fir_range_levels_dev", "corpus_fir_range_levels_dev"):
        assert "fir" in inspect.signature(getattr(x3hip.Context, name)).parameters
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        sig = inspect.signature(cls.fir_range_levels).parameters
        names = list(sig)
        assert names[-3:] == ["fir", "padded_to", "capacity"] and names[-4] == "bin_len", cls
        assert sig["fir"].default is inspect.Parameter.empty
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None for k in ("padded_to", "capacity"))
        into, old = inspect.signature(cls.fir_range_levels_into).parameters, inspect.signature(cls.range_levels_into).parameters
        assert list(into) == list(old)[:-1] + ["fir"], cls
        with pytest.raises(ValueError, match="a Fir"):
            cls.fir_range_levels(cls.__new__(cls), *([0] * (len(names) - 4)), "diff")


def test_the_old_keyword_still_raises():
    f = x3hip.Fir([1, 0, -1])
    with pytest.raises(ValueError, match="not built yet on this keyword: call fir_range_levels"):
        x3hip.level_signal(f, fir=False)
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        obj = cls.__new__(cls)
        obj._h = 1
        n_args = len(inspect.signature(cls.range_levels_into).parameters) - 2
        with pytest.raises(ValueError, match="not built yet"):
            obj.range_levels_into(*([0] * n_args), signal=f)
        n_args = len(inspect.signature(cls.range_levels).parameters) - 4          # (self, padded_to, capacity, signal)
        with pytest.raises(ValueError, match="not built yet"):
            obj.range_levels(*([0] * n_args), signal=f)
