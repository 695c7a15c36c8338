"""signal_range_levels_ref.py, the numpy statement of x3_signal_range_levels_dev's definition, against a per-position loop and
its siblings (diff_levels_ref, range_levels_ref) on the oracle's decode of the base stream of tests/test_gpu_range_levels.py:
2 137 samples in frames of 400 (block length 20, 20 blocks a frame)."""
import numpy as np
import pytest

import diff_levels_ref as D
import levels_ref as LR
import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR
import signal_range_levels_ref as S

BAD, CRC = S.ERR_BAD_ARG, RR.ERR_PAYLOAD_CRC
N = 2137
BINS = [0, 1, 7, 20, 399, 400, 401, 1000, 2 ** 32, 2 ** 40]


@pytest.fixture(scope="module")
def base():
    """(frames, sample offsets, wav, stream, frame offsets, op) of the intact stream"""
    import x3hip
    wav = x3hip.synth(2, 1616, 0, N)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    assert rc == 0
    offs = RR.frame_offsets(s)
    frames = RR.frames_of(s, offs, op)
    so = R.sample_offsets([len(w) for _, w in frames])
    assert so.tolist() == [0, 400, 800, 1200, 1600, 2000, 2137]
    return frames, so, wav, s, offs, op


def _hurt(base, f):
    """the frames with a payload byte of frame f flipped"""
    frames, so, wav, s, offs, op = base
    h = s.copy()
    h[offs[f] + 20 + 30] ^= 0x08
    damaged = RR.frames_of(h, offs, op)
    assert [st for st, _ in damaged] == [CRC if g == f else 0 for g in range(6)]
    return damaged


def _brute(wav, so, bad, start, length, bin_len):
    """a loop over the positions; bad: the frames with a status other than 0"""
    out = LR.empty(S.rows_of(length, bin_len))
    edges = [int(v) for v in so]
    frame_of = lambda g: max(f for f in range(len(edges) - 1) if edges[f] <= g)   # noqa: E731
    for g in range(start, start + length):
        if g == 0 or frame_of(g) in bad or frame_of(g - 1) in bad:
            continue
        v = min(max(int(wav[g]) - int(wav[g - 1]), -32768), 32767)
        r = out[(g - start) // bin_len if bin_len else 0]
        r["sum_sq"] += v * v
        r["sum"] += v
        r["min"], r["max"] = min(r["min"], v), max(r["max"], v)
        r["n"] += 1
    return out


RANGES = [(0, N), (0, 1), (1, 1), (399, 3), (400, 400), (400, 1), (401, 1000), (1, 2136), (2000, 137), (800, 400), (799, 2),
          (2136, 1), (81, 40), (481, 700), (5, 0), (395, 30)]


@pytest.mark.parametrize("bad", [(), (0,), (2,), (5,), (1, 2)])
def test_the_reference_against_a_loop_over_the_positions(base, bad):
    frames, so, wav = base[:3]
    fr = [(BAD if f == 1 else 13 + f, None) if f in bad else fw for f, fw in enumerate(frames)]   # (a frame's status may be BAD_ARG too)
    for start, ln in RANGES:
        for b in (0, 1, 7, 400):
            got, st = S.one(fr, so, start, ln, b)
            assert np.array_equal(got, _brute(wav, so, bad, start, ln, b)), (start, ln, b)
            assert st == R.one(fr, so, start, ln, b)[1]          # the status is the SAMPLES call's


def test_what_n_counts(base):
    frames, so, wav = base[:3]
    assert int(S.one(frames, so, 0, N, 0)[0]["n"][0]) == N - 1            # the entry's first position has no difference
    for start, ln in ((1, 2136), (399, 3), (400, 400), (800, 1), (2136, 1), (401, 7)):
        assert int(S.one(frames, so, start, ln, 0)[0]["n"][0]) == ln     # ... every other clean range has one per position
    hurt = _hurt(base, 1)                                                # a failed lead frame: the seam is gone, the status is 0
    got, st = S.one(hurt, so, 800, 400, 0)
    assert st == 0 and int(got["n"][0]) == 399
    got, st = S.one(hurt, so, 400, 400, 0)                               # ... and as a covering frame it is the status
    assert st == CRC and int(got["n"][0]) == 0
    got, st = S.one(hurt, so, 0, N, 400)                                 # both of its seams are gone
    assert st == CRC and got["n"].tolist() == [399, 0, 399, 400, 400, 137]


def _signal_levels(frames, so, bin_len, n_bins):
    return D.signal_levels([w if st == 0 else [] for st, w in frames], [st for st, _ in frames], so[:-1], bin_len, n_bins, D.DIFF)


@pytest.mark.parametrize("bin_len", BINS)
def test_the_whole_stream_equals_diff_levels_ref(base, bin_len):
    frames, so = base[:2]
    for fr in (frames, _hurt(base, 0), _hurt(base, 2), _hurt(base, 5)):
        got, st = S.one(fr, so, 0, N, bin_len)
        assert np.array_equal(got, _signal_levels(fr, so, bin_len, S.rows_of(N, bin_len)))


@pytest.mark.parametrize("hurt", [None, 0, 2, 5])
def test_bin_aligned_ranges_are_slices_of_the_signal_levels(base, hurt):
    frames, so = base[:2]
    fr = frames if hurt is None else _hurt(base, hurt)
    for b in (1, 7, 20, 100, 400):
        whole = _signal_levels(fr, so, b, S.rows_of(N, b))
        for first, count in ((0, 1), (1, 3), (400 // b, 800 // b), (N // b - 1, 1), (3, N // b - 3)):
            if count < 1:
                continue
            start, ln = first * b, count * b
            got, _ = S.one(fr, so, start, ln, b)
            assert np.array_equal(got, whole[first:first + count]), (b, first, count)
        # ... and the last record cut to the range's length: its n only holds what lies in front of the cut
        start, ln = b, min(3 * b + b // 2 + 1, N - b)
        got, _ = S.one(fr, so, start, ln, b)
        full = ln // b
        assert np.array_equal(got[:full], whole[1:1 + full])
        if ln % b:
            assert np.array_equal(got[full:], S.one(fr, so, start + full * b, ln % b, 0)[0])


def test_samples_is_range_levels_ref(base):
    frames, so = base[:2]
    hurt = _hurt(base, 2)
    starts, lens = [0, 399, 2000, N, 900, 1, N + 1, 5, 400, 800], [400, 3, 137, 0, 1000, N, 0, 61, 400, 1]
    for bin_len, stride, cap in ((0, 0, 10), (7, 0, 400), (7, 0, 100), (400, 3, 30), (100, 25, 250)):
        for fr in (frames, hurt):
            want = R.range_levels(fr, so, starts, lens, bin_len, stride, cap)
            got = S.range_levels(fr, so, starts, lens, bin_len, stride, cap, S.SAMPLES)
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            diff = S.range_levels(fr, so, starts, lens, bin_len, stride, cap, S.DIFF)
            assert np.array_equal(diff[1], want[1]) and np.array_equal(diff[2], want[2])      # offsets and statuses
            rec_d, rec_s = S.view(diff[0]), S.view(want[0])
            assert np.array_equal(rec_d["n"] == 0x5A5A5A5A, rec_s["n"] == 0x5A5A5A5A)          # the same records are written
    with pytest.raises(ValueError):
        S.range_levels(frames, so, [], [], 7, 0, 4)
