"""numpy reference of x3_tone_bank_range_levels_dev / x3_corpus_tone_bank_range_levels_dev (include/x3hip.h, "TONE BANK RANGE
LEVELS"; not a test module).  This file is the definition, and it is one rule: the bank is one tone-range call per step, laid
plane by plane with plane stride `cap`.  Row offsets and statuses exist once and are the single call's; records a call does
not write keep the fill in every plane.  Integers only (tone_range_levels_ref's).  An entry of a corpus is a stream of its
own, as there: the phase is 0 at every entry's first position in every plane."""
import numpy as np

import tone_range_levels_ref as TR

TONE_DTYPE = TR.TONE_DTYPE
BANK_MAX = 8


def one(frames, so, start, length, bin_len, steps, tab):
    """the single range (start, length) -> (TONE_DTYPE [len(steps), R], status): tone_range_levels_ref.one per plane"""
    assert 1 <= len(steps) <= BANK_MAX
    planes = [TR.one(frames, so, start, length, bin_len, int(step), tab) for step in steps]
    assert len({st for _, st in planes}) == 1                 # the status never depends on the bank
    return np.stack([p[0] for p in planes]), planes[0][1]


def range_levels(frames, so, starts, lens, bin_len, stride, cap, steps, tab=None, fill=0x5A):
    """tone_range_levels_ref.range_levels' arguments with 1 .. 8 steps -> (records uint8 [len(steps), cap, 32], row offsets,
    status); ValueError where the call is refused"""
    assert 1 <= len(steps) <= BANK_MAX
    planes = [TR.range_levels(frames, so, starts, lens, bin_len, stride, cap, int(step), tab, fill) for step in steps]
    for p in planes[1:]:
        assert np.array_equal(p[1], planes[0][1]) and np.array_equal(p[2], planes[0][2])
    return np.stack([p[0] for p in planes]), planes[0][1], planes[0][2]
