"""The built library exports the level-quantile, threshold and adaptive-events entry points, and the ctypes mirrors of their
two structures have the sizes include/x3hip.h states."""
import ctypes as C

import numpy as np

import x3hip

NEW = ["x3_level_quantiles_dev", "x3_corpus_level_quantiles_dev", "x3_level_quantiles_result", "x3_level_thresholds_dev",
       "x3_corpus_level_thresholds_dev", "x3_events_adaptive_dev", "x3_corpus_events_adaptive_dev"]


def test_the_library_exports_the_new_entry_points():
    L = x3hip.lib()
    for name in NEW + ["x3_events_result"]:          # (x3_events_result, not new, serves the adaptive calls)
        assert name in x3hip.SYMBOLS and hasattr(L, name), name


def test_structure_sizes():
    assert C.sizeof(x3hip.ThresholdRule) == 32 and C.sizeof(x3hip.EventRule) == 32
    assert x3hip.EVENT_THRESHOLD_DTYPE.itemsize == 16
    assert [x3hip.EVENT_THRESHOLD_DTYPE.fields[k][1] for k in ("mean_sq_min", "peak_min", "counted")] == [0, 8, 12]
    r = x3hip.ThresholdRule.make(mean_sq=(500_000, 4, 1, 0))
    assert (r.peak_div, r.mean_sq_q_ppm, r.mean_sq_mul, r.mean_sq_div) == (0, 500_000, 4, 1)
    assert np.frombuffer(bytes(r), dtype="<u4").tolist() == [0, 0, 0, 0, 500_000, 4, 1, 0]
    assert (x3hip.LEVEL_KEY_PEAK, x3hip.LEVEL_KEY_MEAN_SQ) == (0, 1)
