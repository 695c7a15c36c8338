"""The tone levels entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the
Python mirror's Tone value, table and keyword.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tone_levels_ref as TR
import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_tone_levels_dev", "x3_corpus_tone_levels_dev"]
ADAPTER = "x3_tone_power_levels_dev"


def text(*path):
    return open(os.path.join(ROOT, *path)).read()


def struct_fields(header, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + [ADAPTER, "x3_levels_result"]:                          # (x3_levels_result serves the new calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    # x3_levels_dev's / x3_corpus_levels_dev's arguments and a pointer to the oscillator
    assert L.x3_tone_levels_dev.argtypes[:-1] == L.x3_levels_dev.argtypes
    assert L.x3_corpus_tone_levels_dev.argtypes[:-1] == L.x3_corpus_levels_dev.argtypes
    for name in NEW:
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelTone)
    assert [C.sizeof(t) for t in L.x3_tone_power_levels_dev.argtypes] == [8, 8, 8, 8]


def test_the_structs_are_the_headers():
    header = text("include", "x3hip.h")
    assert "TONE LEVELS" in header and "THE ADAPTER" in header and "Nyquist" in header and "Two identities" in header
    assert struct_fields(header, "x3_level_tone") == ["uint32_t step", "uint32_t reserved", "const int16_t* d_table"]
    assert struct_fields(header, "x3_tone_level") == ["int64_t re", "int64_t im", "int32_t min, max", "uint32_t n",
                                                      "uint32_t reserved"]
    assert [(n, t) for n, t in x3hip.LevelTone._fields_] == [("step", C.c_uint32), ("reserved", C.c_uint32),
                                                             ("d_table", C.c_void_p)]
    assert C.sizeof(x3hip.LevelTone) == 16
    # the record: x3_level's layout slot for slot
    assert x3hip.TONE_DTYPE.itemsize == x3hip.LEVEL_DTYPE.itemsize == 32 and x3hip.TONE_DTYPE == TR.TONE_DTYPE
    assert x3hip.TONE_DTYPE.names == ("re", "im", "min", "max", "n", "reserved")
    for a, b in zip(x3hip.TONE_DTYPE.names, x3hip.LEVEL_DTYPE.names):
        assert x3hip.TONE_DTYPE.fields[a][1] == x3hip.LEVEL_DTYPE.fields[b][1]
        assert x3hip.TONE_DTYPE.fields[a][0].itemsize == x3hip.LEVEL_DTYPE.fields[b][0].itemsize
    assert x3hip.TONE_DTYPE.fields["re"][0] == np.int64 and x3hip.TONE_DTYPE.fields["im"][0] == np.int64
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")

    def rust_fields(name):
        rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+%s\s*\{(.*?)\}" % name, rust, flags=re.S)
        return rm and [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()]
    assert rust_fields("x3_level_tone") == ["pub step: u32", "pub reserved: u32", "pub d_table: *const i16"]
    assert rust_fields("x3_tone_level") == ["pub re: i64", "pub im: i64", "pub min: i32", "pub max: i32", "pub n: u32",
                                            "pub reserved: u32"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_level_tone\* tone\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*tone: \*const x3_level_tone\) -> c_int;" % name, rust), name
    assert "int %s(x3_ctx* ctx, const x3_tone_level* d_tone, uint64_t n_rows, x3_level* d_levels);" % ADAPTER in header
    assert ADAPTER + "(" in hpp and "pub fn %s(" % ADAPTER in rust
    assert "struct Tone {" in hpp and "inline X3Error tone_levels(" in hpp and "inline X3Error tone_power_levels(" in hpp
    assert len(re.findall(r"WindowsResult\* res,\s+const Tone& tone\)", hpp)) == 2       # device::tone_levels, Corpus::tone_levels
    assert "pub fn tone_levels<'g>(" in rust and "pub fn tone_levels(&self" in rust and "pub fn tone_power_levels<'g>(" in rust
    assert "pub type ToneLevel = ffi::x3_tone_level;" in rust
    # the option table is untouched: no option speaks of the tone
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "tone" in w.split("_")]


def test_the_table():
    t = x3hip.tone_table()
    assert t.dtype == np.int16 and t.shape == (1024, 2) and t.nbytes == 4096 and np.array_equal(t, TR.table())
    assert t[0].tolist() == [32767, 0] and t[256].tolist() == [0, 32767]


def test_tone_and_the_keyword():
    t = x3hip.Tone(step=12345)
    assert t.step == 12345 and x3hip.level_signal(t) is t and t == x3hip.Tone(12345) and hash(t) == hash(x3hip.Tone(12345))
    assert x3hip.Tone(0).step == 0 and x3hip.Tone((1 << 32) - 1).step == (1 << 32) - 1
    assert x3hip.Tone.at(0.0817, 1.0).step == round(0.0817 * 2 ** 32)
    assert x3hip.Tone.at(4000, 16000).step == 1 << 30 and x3hip.Tone.at(0, 16000).step == 0
    # just below the sample rate the rounded step is 2^32: the last step below it, not DC
    assert x3hip.Tone.at(1.0 - 2.0 ** -34, 1.0).step == (1 << 32) - 1 and x3hip.Tone.at(47999.99999, 48000).step == (1 << 32) - 1
    assert x3hip.Tone.at(1.0 - 2.0 ** -32, 1.0).step == (1 << 32) - 1 and x3hip.Tone.at(0.5, 1.0).step == 1 << 31
    for bad in (-1, 1 << 32, 0.5, True, "1", None):
        with pytest.raises(ValueError):
            x3hip.Tone(bad)
    for f, fs in ((-1, 16000), (16000, 16000), (1, 0)):
        with pytest.raises(ValueError):
            x3hip.Tone.at(f, fs)
    with pytest.raises(AttributeError):
        t.step = 1
    with pytest.raises(AttributeError):
        del t.step
    with pytest.raises(ValueError, match="not built yet"):
        x3hip.level_signal(t, fir=False)
    for cls in (x3hip.WindowSource, x3hip.Corpus):       # range_levels(signal=Tone(...)) raises in front of any other work
        obj = cls.__new__(cls)
        obj._h = 1
        with pytest.raises(ValueError, match="not built yet"):
            if cls is x3hip.Corpus:
                obj.range_levels(None, None, None, 100, signal=t)
            else:
                obj.range_levels(None, None, 100, signal=t)
        with pytest.raises(ValueError, match="a Tone"):
            obj.tone_levels(100, 12345)
    assert [x3hip.level_signal(s) for s in ("samples", "diff")] == [0, 1]
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("levels", "events", "level_quantiles", "adaptive_events", "range_levels"):
            p = inspect.signature(getattr(cls, method)).parameters["signal"]
            assert p.default == "samples" and p.kind is inspect.Parameter.KEYWORD_ONLY, (cls, method)
        assert list(inspect.signature(cls.tone_levels).parameters)[1:3] == ["bin_len", "tone"]
        assert "tone" in inspect.signature(cls.tone_levels_into).parameters
    assert list(inspect.signature(x3hip.WindowSource.tone_levels).parameters)[3] == "n_bins"
    for name in ("tone_levels_dev", "corpus_tone_levels_dev"):
        assert "tone" in inspect.signature(getattr(x3hip.Context, name)).parameters
    assert list(inspect.signature(x3hip.Context.tone_power_levels_dev).parameters) == ["self", "d_tone", "n_rows", "d_levels"]
