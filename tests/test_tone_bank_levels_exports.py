"""The tone bank entry points in the header, the built library, the ctypes binding and the C++ and Rust mirrors, and the
Python mirror's LevelToneBank, Tone.bank and `tones` argument.  CPU only."""
import ctypes as C
import inspect
import re

import pytest

import x3hip
from test_tone_levels_exports import struct_fields, text

NEW = ["x3_tone_bank_levels_dev", "x3_corpus_tone_bank_levels_dev"]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW:
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes[-1] is C.POINTER(x3hip.LevelToneBank)
    # the single call's arguments, and a pointer to the bank where its pointer to the oscillator is
    assert L.x3_tone_bank_levels_dev.argtypes[:-1] == L.x3_tone_levels_dev.argtypes[:-1] == L.x3_levels_dev.argtypes
    assert L.x3_corpus_tone_bank_levels_dev.argtypes[:-1] == L.x3_corpus_tone_levels_dev.argtypes[:-1]


def test_the_struct_is_the_headers():
    header = text("include", "x3hip.h")
    assert "TONE BANK LEVELS" in header and "PLANE BY PLANE" in header and "DESIGN.md section 26" in header
    assert re.search(r"#define\s+X3_TONE_BANK_MAX\s+8\b", header) and x3hip.TONE_BANK_MAX == 8
    assert struct_fields(header, "x3_level_tone_bank") == ["uint32_t n_tones", "uint32_t reserved", "const int16_t* d_table",
                                                           "uint32_t steps[X3_TONE_BANK_MAX]"]
    assert [(n, t) for n, t in x3hip.LevelToneBank._fields_] == [("n_tones", C.c_uint32), ("reserved", C.c_uint32),
                                                                 ("d_table", C.c_void_p), ("steps", C.c_uint32 * 8)]
    assert C.sizeof(x3hip.LevelToneBank) == 48 and x3hip.LevelToneBank.steps.offset == 16
    assert x3hip.LevelToneBank.d_table.offset == x3hip.LevelTone.d_table.offset == 8
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    rm = re.search(r"#\[repr\(C\)\][^{]*?pub\s+struct\s+x3_level_tone_bank\s*\{(.*?)\}", rust, flags=re.S)
    assert [" ".join(f.split()) for f in rm.group(1).split(",\n") if f.strip()] == [
        "pub n_tones: u32", "pub reserved: u32", "pub d_table: *const i16", "pub steps: [u32; 8]"]


def test_the_mirrors_declare_them():
    header, hpp, rust = text("include", "x3hip.h"), text("x3-rust_amd", "host", "x3.hpp"), text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
        assert re.search(r"%s\([^;]*const x3_level_tone_bank\* bank\);" % name, header), name
        assert re.search(r"pub fn %s\([^;]*bank: \*const x3_level_tone_bank\) -> c_int;" % name, rust), name

    def params(decl, name):                     # the C parameter list up to the last argument, names and types
        m = re.search(r"int %s\((.*?)\);" % name, decl, flags=re.S)
        return [" ".join(a.split()) for a in m.group(1).split(",")][:-1]
    assert params(header, "x3_tone_bank_levels_dev") == params(header, "x3_tone_levels_dev")
    assert params(header, "x3_corpus_tone_bank_levels_dev") == params(header, "x3_corpus_tone_levels_dev")
    assert "struct ToneBank {" in hpp and "inline X3Error tone_bank_levels(" in hpp
    assert len(re.findall(r"WindowsResult\* res,\s+const ToneBank& bank\)", hpp)) == 2     # device::, Corpus::
    assert "pub fn tone_bank_levels<'g>(" in rust and "pub fn tone_bank_levels(&self" in rust and "pub struct ToneBank<" in rust
    # the option table is untouched, and the kernels' bank is the header's
    assert not [w for w in re.findall(r'"([a-z_0-9]+)"', text("x3-rust_amd", "csrc", "x3_ctx.hip")) if "tone" in w.split("_")]
    assert re.search(r"#define\s+X3L_TONE_BANK\s+8\b", text("x3-rust_amd", "csrc", "x3_levels_kernel.h"))
    assert "X3_TONE_BANK_MAX == X3L_TONE_BANK" in text("x3-rust_amd", "csrc", "x3_decode.hip")


def test_tone_bank_and_the_tones_argument():
    bank = x3hip.Tone.bank([0.0817, 0.2310, 0.15, 0.41], 1.0)
    assert isinstance(bank, tuple) and [t.step for t in bank] == [350_898_828, 992_137_445, 644_245_094, 1_760_936_591]
    assert bank == tuple(x3hip.Tone.at(f, 1.0) for f in (0.0817, 0.2310, 0.15, 0.41))
    assert x3hip.Tone.bank([4000], 16000) == (x3hip.Tone(1 << 30),) and x3hip.Tone.bank([], 16000) == ()
    with pytest.raises(ValueError):
        x3hip.Tone.bank([16000], 16000)
    assert x3hip.tone_bank(list(bank)) == bank and x3hip.tone_bank(t for t in bank) == bank
    for bad in ((), [x3hip.Tone(1)] * 9, x3hip.Tone(1), [1, 2], None, 5, [x3hip.Tone(1), None]):
        with pytest.raises(ValueError, match="1 .. 8 Tone"):
            x3hip.tone_bank(bad)
    for cls in (x3hip.WindowSource, x3hip.Corpus):       # the host methods check `tones` in front of any other work
        obj = cls.__new__(cls)
        obj._h = 1
        for bad in ((), [x3hip.Tone(1)] * 9, x3hip.Tone(1)):
            with pytest.raises(ValueError, match="1 .. 8 Tone"):
                obj.tone_bank_levels(100, bad)
        sig = inspect.signature(cls.tone_bank_levels).parameters
        assert list(sig)[1:3] == ["bin_len", "tones"] and sig["band"].default is False
        assert sig["band"].kind is inspect.Parameter.KEYWORD_ONLY
        into = inspect.signature(cls.tone_bank_levels_into).parameters
        assert "tones" in into and into["band"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "signal" not in sig                      # a bank returns K planes, which levels() cannot
    assert list(inspect.signature(x3hip.WindowSource.tone_bank_levels).parameters)[3] == "n_bins"
    for name in ("tone_bank_levels_dev", "corpus_tone_bank_levels_dev"):
        assert "tones" in inspect.signature(getattr(x3hip.Context, name)).parameters
    with pytest.raises(ValueError):
        x3hip.level_signal(bank)                         # the keyword `signal` stays as it is
