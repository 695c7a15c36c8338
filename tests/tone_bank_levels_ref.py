"""numpy reference of x3_tone_bank_levels_dev / x3_corpus_tone_bank_levels_dev (include/x3hip.h, "TONE BANK LEVELS"; not a
test module).  This file is the definition, and it is one rule: the bank is one tone call per step, laid plane by plane.
Integers only (tone_levels_ref's)."""
import numpy as np

import tone_levels_ref as TR

TONE_DTYPE = TR.TONE_DTYPE
BANK_MAX = 8


def tone_bank_levels(frames, statuses, so, bin_len, n_bins, steps, tab=None):
    """tone_levels_ref.tone_levels' arguments with 1 .. 8 steps -> TONE_DTYPE[len(steps), n_bins]"""
    assert 1 <= len(steps) <= BANK_MAX
    return np.stack([TR.tone_levels(frames, statuses, so, bin_len, n_bins, int(step), tab) for step in steps])


def corpus_tone_bank_levels(entries, bin_len, steps, tab=None):
    """tone_levels_ref.corpus_tone_levels' arguments with 1 .. 8 steps -> (TONE_DTYPE[len(steps), rows], row_first): the
    plane stride is the corpus's rows, row_first is the single call's"""
    assert 1 <= len(steps) <= BANK_MAX
    planes = [TR.corpus_tone_levels(entries, bin_len, int(step), tab) for step in steps]
    return np.stack([p[0] for p in planes]), planes[0][1]


def example():
    """DESIGN.md section 26's signal: section 24's noise and burst (0.0817 fs on [4 400, 4 600)) and a second burst of
    amplitude 1 000 at 0.2310 fs with phase 1.1 on [12 000, 12 200)"""
    w = np.random.RandomState(7).randint(-3000, 3001, 20_000).astype(np.int64)
    t = np.arange(4_400, 4_600)
    w[4_400:4_600] += np.rint(1_000 * np.sin(2 * np.pi * 0.0817 * t + 0.3)).astype(np.int64)
    t = np.arange(12_000, 12_200)
    w[12_000:12_200] += np.rint(1_000 * np.sin(2 * np.pi * 0.2310 * t + 1.1)).astype(np.int64)
    return np.clip(w, -32768, 32767).astype(np.int16)


EXAMPLE_FREQS = (0.0817, 0.2310, 0.15, 0.41)
EXAMPLE_STEPS = (350_898_828, 992_137_445, 644_245_094, 1_760_936_591)
