"""The tone range levels entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, the
Python mirror's methods, the refusal order (the tone first) and the old keyword's refusal.  CPU only."""
import ctypes as C
import inspect
import os
import re

import pytest

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_tone_range_levels_dev", "x3_corpus_tone_range_levels_dev"]


def text(*path):
    with open(os.path.join(ROOT, *path)) as fh:
        return fh.read()


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_range_levels_result", "x3_tone_power_levels_dev"]:   # (both serve the new calls as they are)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    # x3_range_levels_dev's / x3_corpus_range_levels_dev's arguments, width for width, and a pointer to the oscillator
    assert L.x3_tone_range_levels_dev.argtypes[:-1] == L.x3_range_levels_dev.argtypes
    assert L.x3_corpus_tone_range_levels_dev.argtypes[:-1] == L.x3_corpus_range_levels_dev.argtypes
    assert [C.sizeof(t) for t in L.x3_tone_range_levels_dev.argtypes] == [8, 8, 8, 8, 8, 8, 8, 8, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8]
    assert [C.sizeof(t) for t in L.x3_corpus_tone_range_levels_dev.argtypes] == [8] * 13
    for name in NEW:
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelTone)


def test_the_header_and_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    assert "TONE RANGE LEVELS" in header and "it does NOT restart the oscillator at the range" in header
    assert "THE PHASE IS THE STREAM'S" in header and "never the raw sums" in header          # what a caller may compare
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*x3_tone_level\* d_levels,[^;]*const x3_level_tone\* tone\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*d_levels: \*mut x3_tone_level,[^;]*tone: \*const x3_level_tone\) -> c_int;" % name, rust), name
    # packed or padded tone range records go through the adapter unchanged: said at both places
    adapter = header[header.index("THE ADAPTER"):header.index("int x3_tone_power_levels_dev(")]
    assert "x3_tone_range_levels_dev" in adapter and "packed or padded" in adapter
    new = header[header.index("TONE RANGE LEVELS"):header.index("int x3_tone_range_levels_dev(")]
    assert "x3_tone_power_levels_dev unchanged" in new
    # the Tone goes in front of the result pointer: device::tone_range_levels and Corpus::tone_range_levels
    assert len(re.findall(r"const Tone& tone,\s+RangeLevelsResult\* res\)", hpp)) == 2
    assert "inline X3Error tone_range_levels(" in hpp and "  X3Error tone_range_levels(" in hpp
    assert "pub fn tone_range_levels<'g>(" in rust and "pub fn tone_range_levels(&self" in rust
    # the option table is untouched: no option speaks of the tone
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "tone" in w.split("_")]


def test_the_tone_is_refused_first():
    """without a device only the order in the source can be read: each entry point tests the context and the tone, and
    nothing else, in front of the call that tests every other argument (the GPU file makes the calls)"""
    src = text("x3-rust_amd", "csrc", "x3_decode.hip")
    for name, inner in zip(NEW, ("stream_range_levels_call", "corpus_range_levels_call")):
        body = src[src.index('extern "C" int %s(' % name):]
        body = body[body.index("{"):body.index("\n}\n")]
        lines = [ln.strip() for ln in body.split("\n")[1:] if ln.strip()]
        assert lines[0] == "X3LevToneTail t;"
        assert lines[1] == "if (!c || !levels_tone_arg(tone, &t)) return X3_ERR_BAD_ARG;"
        assert lines[2].startswith("return %s(" % inner)
    L = x3hip.lib()
    for name in NEW:          # (no context: refused, nothing touched)
        fn = getattr(L, name)
        assert fn(*[0 if t in (C.c_uint64, C.c_uint32, C.c_int) else None for t in fn.argtypes]) == x3hip.ERR_BAD_ARG


def test_the_python_methods():
    for name in ("tone_range_levels_dev", "corpus_tone_range_levels_dev"):
        assert "tone" in inspect.signature(getattr(x3hip.Context, name)).parameters
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        sig = inspect.signature(cls.tone_range_levels).parameters
        names = list(sig)
        assert names[-4:] == ["tone", "padded_to", "capacity", "band"] and names[-5] == "bin_len", cls
        assert sig["tone"].default is inspect.Parameter.empty
        assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("padded_to", "capacity", "band"))
        assert sig["padded_to"].default is None and sig["capacity"].default is None and sig["band"].default is False
        into, old = inspect.signature(cls.tone_range_levels_into).parameters, inspect.signature(cls.range_levels_into).parameters
        assert list(into) == list(old)[:-1] + ["tone"], cls
        with pytest.raises(ValueError, match="a Tone"):
            cls.tone_range_levels(cls.__new__(cls), *([0] * (len(names) - 5)), 12345)


def test_the_old_keyword_still_raises():
    t = x3hip.Tone(12345)
    with pytest.raises(ValueError, match="not built yet on this keyword: call tone_range_levels"):
        x3hip.level_signal(t, fir=False)
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        obj = cls.__new__(cls)
        obj._h = 1
        n_args = len(inspect.signature(cls.range_levels_into).parameters) - 2
        with pytest.raises(ValueError, match="not built yet"):
            obj.range_levels_into(*([0] * n_args), signal=t)
        n_args = len(inspect.signature(cls.range_levels).parameters) - 4          # (self, padded_to, capacity, signal)
        with pytest.raises(ValueError, match="not built yet"):
            obj.range_levels(*([0] * n_args), signal=t)
