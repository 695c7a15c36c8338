"""The built library exports the signal-levels entry points, and the Python mirror carries their constants and keyword."""
import inspect

import pytest

import x3hip

NEW = ["x3_signal_levels_dev", "x3_corpus_signal_levels_dev"]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_levels_result", "x3_levels_dev", "x3_corpus_levels_dev"]:   # (x3_levels_result serves the new calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name
    assert len(L.x3_signal_levels_dev.argtypes) == len(L.x3_levels_dev.argtypes) + 1
    assert len(L.x3_corpus_signal_levels_dev.argtypes) == len(L.x3_corpus_levels_dev.argtypes) + 1


def test_constants_and_the_keyword():
    assert (x3hip.LEVEL_SIGNAL_SAMPLES, x3hip.LEVEL_SIGNAL_DIFF) == (0, 1)
    assert x3hip.LEVEL_SIGNALS == {"samples": 0, "diff": 1}
    assert [x3hip.level_signal(s) for s in ("samples", "diff", 0, 1)] == [0, 1, 0, 1]
    for bad in ("second", 2, -1, None, True):
        with pytest.raises(ValueError):
            x3hip.level_signal(bad)
    for cls in (x3hip.WindowSource, x3hip.Corpus):
        for method in ("levels", "events", "level_quantiles", "adaptive_events"):
            p = inspect.signature(getattr(cls, method)).parameters["signal"]
            assert p.default == "samples" and p.kind is inspect.Parameter.KEYWORD_ONLY, (cls, method)
