"""The built library exports the signal-range-levels entry points, the Python mirror carries their keyword, and the C++ and
Rust mirrors name the calls."""
import inspect
import os

import x3hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["x3_signal_range_levels_dev", "x3_corpus_signal_range_levels_dev"]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_range_levels_result", "x3_range_levels_dev", "x3_corpus_range_levels_dev"]:   # (the result call is shared)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    assert len(L.x3_signal_range_levels_dev.argtypes) == len(L.x3_range_levels_dev.argtypes) + 1
    assert len(L.x3_corpus_signal_range_levels_dev.argtypes) == len(L.x3_corpus_range_levels_dev.argtypes) + 1


def test_the_keyword_and_the_context_methods():
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        p = inspect.signature(cls.range_levels).parameters["signal"]
        assert p.default == "samples" and p.kind is inspect.Parameter.KEYWORD_ONLY, cls
        p = inspect.signature(cls.range_levels_into).parameters["signal"]
        assert p.default == x3hip.LEVEL_SIGNAL_SAMPLES, cls
    for method in ("signal_range_levels_dev", "corpus_signal_range_levels_dev"):
        p = inspect.signature(getattr(x3hip.Context, method)).parameters["signal"]
        assert p.default == x3hip.LEVEL_SIGNAL_SAMPLES, method


def test_the_header_and_the_mirrors_name_the_calls():
    def text(*path):
        with open(os.path.join(ROOT, *path)) as fh:
            return fh.read()
    header = text("include", "x3hip.h")
    hpp = text("x3-rust_amd", "host", "x3.hpp")
    rust = text("x3-rust_amd", "rust", "src", "lib.rs")
    for name in NEW:
        assert "int %s(" % name in header and name + "(" in hpp and "pub fn %s(" % name in rust, name
    assert hpp.count("RangeLevelsResult* res, LevelSignal signal = LevelSignal::Samples") == 1            # device::range_levels
    assert "RangeLevelsResult* res,\n                       LevelSignal signal = LevelSignal::Samples) const" in hpp   # Corpus
    assert "pub fn signal_range_levels<'g>(" in rust and "pub fn signal_range_levels(&self" in rust
