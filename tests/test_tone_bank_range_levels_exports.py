"""The tone bank range-levels entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors,
and the Python mirror's methods.  CPU only."""
import ctypes as C
import inspect
import re

import pytest

import x3hip
from test_tone_levels_exports import struct_fields, text

NEW = ["x3_tone_bank_range_levels_dev", "x3_corpus_tone_bank_range_levels_dev"]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW:
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelToneBank)
    # the single call's arguments, and a pointer to the bank where its pointer to the oscillator is
    assert L.x3_tone_bank_range_levels_dev.argtypes[:-1] == L.x3_tone_range_levels_dev.argtypes[:-1] == L.x3_range_levels_dev.argtypes
    assert L.x3_corpus_tone_bank_range_levels_dev.argtypes[:-1] == L.x3_corpus_tone_range_levels_dev.argtypes[:-1]
    assert L.x3_corpus_tone_bank_range_levels_dev.argtypes[:-1] == L.x3_corpus_range_levels_dev.argtypes


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "TONE BANK RANGE LEVELS" in header and "DESIGN.md section 27" in header and "plane stride rows_cap" in header
    assert struct_fields(header, "x3_level_tone_bank") == ["uint32_t n_tones", "uint32_t reserved", "const int16_t* d_table",
                                                           "uint32_t steps[X3_TONE_BANK_MAX]"]
    assert C.sizeof(x3hip.LevelToneBank) == 48 == 8 + 8 + 4 * x3hip.TONE_BANK_MAX     # sizeof(x3_level_tone_bank)
    assert [n for n, _ in x3hip.LevelToneBank._fields_] == ["n_tones", "reserved", "d_table", "steps"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_level_tone_bank\* bank\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*bank: \*const x3_level_tone_bank\) -> c_int;" % name, rust), name

    def params(decl, name):                     # the C parameter list up to the last argument, names and types
        m = re.search(r"int %s\((.*?)\);" % name, decl, flags=re.S)
        return [" ".join(a.split()) for a in m.group(1).split(",")][:-1]
    assert params(header, "x3_tone_bank_range_levels_dev") == params(header, "x3_tone_range_levels_dev")
    assert params(header, "x3_corpus_tone_bank_range_levels_dev") == params(header, "x3_corpus_tone_range_levels_dev")
    assert "inline X3Error tone_bank_range_levels(" in hpp
    assert len(re.findall(r"const ToneBank& bank,\s+RangeLevelsResult\* res\)", hpp)) == 2     # device::, Corpus::
    assert "pub fn tone_bank_range_levels<'g>(" in rust and "pub fn tone_bank_range_levels(&self" in rust
    # the launcher has no hole left, and the option table is untouched
    decode = text("x3-rust_amd", "csrc", "x3_decode.hip")
    assert "case LevSignal::BANK: return X3_ERR_BAD_ARG" not in decode
    # (the range launcher runs the bank signal's instances: the behaviour is the GPU tests')
    launcher = decode[decode.index("static int range_levels_launch("):]
    assert re.search(r"X3LevToneBank<\s*2\s*>", launcher[:launcher.index("\n}\n")])
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "tone" in w.split("_")]


def test_the_python_methods_and_the_tones_argument():
    bank = x3hip.Tone.bank([0.0817, 0.2310, 0.15, 0.41], 1.0)
    for cls, lead in ((x3hip.WindowSource, ["starts", "lens", "bin_len", "tones"]),
                      (x3hip.Corpus, ["entries", "starts", "lens", "bin_len", "tones"])):
        obj = cls.__new__(cls)
        obj._h = 1
        for bad in ((), [x3hip.Tone(1)] * 9, x3hip.Tone(1), None):      # `tones` is checked in front of any other work
            with pytest.raises(ValueError, match="1 .. 8 Tone"):
                obj.tone_bank_range_levels(*([[0]] * (len(lead) - 2)), 100, bad)
        sig = inspect.signature(cls.tone_bank_range_levels).parameters
        assert list(sig)[1:1 + len(lead)] == lead
        for kw, default in (("padded_to", None), ("capacity", None), ("band", False)):
            assert sig[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig[kw].default is default
        assert [p for p in sig if p not in ("self", "tones")] == \
            [p for p in inspect.signature(cls.tone_range_levels).parameters if p not in ("self", "tone")]
        into = list(inspect.signature(cls.tone_bank_range_levels_into).parameters)
        assert into[:-1] == list(inspect.signature(cls.tone_range_levels_into).parameters)[:-1] and into[-1] == "tones"
    for name in ("tone_bank_range_levels_dev", "corpus_tone_bank_range_levels_dev"):
        mine = list(inspect.signature(getattr(x3hip.Context, name)).parameters)
        assert mine[-1] == "tones" and mine[:-1] == list(inspect.signature(getattr(x3hip.Context, name.replace("_bank", ""))).parameters)[:-1]
    assert "planes" in inspect.signature(x3hip._range_levels_torch).parameters          # one helper, with a plane count
    # the keyword `signal` of range_levels takes no bank and names the call that does
    for bad in (bank, list(bank), x3hip.LevelToneBank()):
        with pytest.raises(ValueError, match="call tone_bank_range_levels"):
            x3hip.level_signal(bad, fir=False)
    with pytest.raises(ValueError):
        x3hip.level_signal(bank)                                                          # (the levels keyword: as it was)
