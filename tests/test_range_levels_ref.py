"""range_levels_ref.py, the numpy statement of x3_range_levels_dev's definition, against itself and its siblings
(levels_ref, events_ref, ranges_ref) on the oracle's decode of the base stream of tests/test_gpu_range_levels.py: 2 137
samples in frames of 400 (block length 20, 20 blocks a frame)."""
import numpy as np
import pytest

import events_ref as E
import levels_ref as LR
import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR

BAD = R.ERR_BAD_ARG
N = 2137
BINS = [0, 1, 7, 20, 399, 400, 401, 1000, 2 ** 32, 2 ** 40]


@pytest.fixture(scope="module")
def base():
    """(frames, sample offsets, wav) of the intact stream, and the frames with a payload byte of frame 2 flipped"""
    import x3hip
    wav = x3hip.synth(2, 1616, 0, N)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    assert rc == 0
    offs = RR.frame_offsets(s)
    frames = RR.frames_of(s, offs, op)
    so = R.sample_offsets([len(w) for _, w in frames])
    assert so.tolist() == [0, 400, 800, 1200, 1600, 2000, 2137] and np.array_equal(np.concatenate([w for _, w in frames]), wav)
    hurt = s.copy()
    hurt[offs[2] + 20 + 30] ^= 0x08
    damaged = RR.frames_of(hurt, offs, op)
    assert [st for st, _ in damaged] == [0, 0, RR.ERR_PAYLOAD_CRC, 0, 0, 0]
    return frames, so, wav, damaged


def _levels_of(frames, so, bin_len, n_bins):
    return LR.levels([w if st == 0 else [] for st, w in frames], [st for st, _ in frames], so[:-1], bin_len, n_bins)


def _brute(wav, start, length, bin_len, skip=()):
    """a loop over the samples; skip: positions [a, b) of frames that add nothing"""
    out = LR.empty(R.rows_of(length, bin_len))
    for g in range(start, start + length):
        if any(a <= g < b for a, b in skip):
            continue
        r, v = out[(g - start) // bin_len if bin_len else 0], int(wav[g])
        r["sum_sq"] += v * v
        r["sum"] += v
        r["min"], r["max"] = min(r["min"], v), max(r["max"], v)
        r["n"] += 1
    return out


def test_rows_of_is_the_corpus_levels_rule():
    for ln in (0, 1, 19, 20, 21, 2137, 2 ** 32 - 1):
        for b in BINS:
            assert R.rows_of(ln, b) == LR.n_bins_for(ln, b)
    assert [R.rows_of(ln, 20) for ln in (0, 1, 20, 21)] == [1, 1, 1, 2] and R.rows_of(2 ** 32 - 1, 2 ** 32) == 1


@pytest.mark.parametrize("bin_len", BINS)
def test_the_whole_stream_equals_levels_ref(base, bin_len):
    frames, so, wav, damaged = base
    for fr in (frames, damaged):
        got, st = R.one(fr, so, 0, N, bin_len)
        assert np.array_equal(got, _levels_of(fr, so, bin_len, R.rows_of(N, bin_len)))
        assert st == (0 if fr is frames else RR.ERR_PAYLOAD_CRC)
        assert int(got["n"].sum()) == (N if fr is frames else N - 400)


@pytest.mark.parametrize("bin_len", [1, 7, 20, 399, 400, 401, 1000])
def test_bin_len_0_is_the_merge_of_the_fine_bins(base, bin_len):
    frames, so, wav, damaged = base
    for fr in (frames, damaged):
        for start, ln in ((0, N), (399, 3), (401, 1000), (1, 2136), (2000, 137), (800, 400), (5, 0)):
            fine, st = R.one(fr, so, start, ln, bin_len)
            whole, st0 = R.one(fr, so, start, ln, 0)
            assert st == st0 and len(whole) == 1 and whole[0] == E.merge(fine)


def test_bins_are_counted_from_the_range_start(base):
    frames, so, wav, damaged = base
    for start, ln, b in ((0, 400, 7), (399, 3, 1), (395, 30, 7), (1, 2136, 401), (1999, 138, 20), (777, 1000, 399)):
        got, st = R.one(frames, so, start, ln, b)
        assert st == 0 and np.array_equal(got, _brute(wav, start, ln, b))
        hurt, st = R.one(damaged, so, start, ln, b)
        covers = start < 1200 and start + ln > 800
        assert st == (RR.ERR_PAYLOAD_CRC if covers else 0)
        assert np.array_equal(hurt, _brute(wav, start, ln, b, skip=[(800, 1200)]))


def test_a_bad_frame_adds_nothing_and_sets_the_status(base):
    frames, so, wav, damaged = base
    got, st = R.one(damaged, so, 700, 600, 100)              # frames 1, 2, 3: 100 samples, the bad frame, 100 samples
    assert st == RR.ERR_PAYLOAD_CRC and got["n"].tolist() == [100, 0, 0, 0, 0, 100]
    assert np.array_equal(got[1:5], LR.empty(4)) and np.array_equal(got[[0, 5]], _brute(wav, 700, 600, 100)[[0, 5]])
    got, st = R.one(damaged, so, 900, 100, 0)                # inside it
    assert st == RR.ERR_PAYLOAD_CRC and np.array_equal(got, LR.empty(1))
    assert R.one(damaged, so, 0, 800, 400)[1] == 0 and R.one(damaged, so, 1200, 937, 400)[1] == 0
    two = [(0, w) if f not in (1, 4) else (13 + f, None) for f, (_, w) in enumerate(frames)]
    assert R.one(two, so, 0, N, 0)[1] == 14 and int(R.one(two, so, 0, N, 0)[0]["n"][0]) == N - 800   # the first in frame order


def test_off_the_end_and_a_length_of_0(base):
    frames, so, wav, _ = base
    for start, ln in ((N + 1, 0), (N, 1), (1, N), (2 ** 63, 5), (0, N + 1)):
        got, st = R.one(frames, so, start, ln, 20)
        assert st == BAD and np.array_equal(got, LR.empty(R.rows_of(ln, 20)))
    for start in (0, 400, N):
        got, st = R.one(frames, so, start, 0, 20)
        assert st == 0 and np.array_equal(got, LR.empty(1))


def test_packed_and_padded_hold_the_same_records(base):
    frames, so, wav, damaged = base
    starts, lens = [0, 399, 2000, N, 900, 1, N + 1, 5], [400, 3, 137, 0, 1000, N, 0, 61]
    for bin_len in (0, 7, 400, 2 ** 32):
        rows = [R.rows_of(ln, bin_len) for ln in lens]
        total, stride = sum(rows), max(rows)
        packed, off, st = R.range_levels(damaged, so, starts, lens, bin_len, 0, total + 3)
        padded, poff, pst = R.range_levels(damaged, so, starts, lens, bin_len, stride, len(lens) * stride + 2)
        assert off.tolist() == np.concatenate([[0], np.cumsum(rows)]).tolist() and poff.tolist() == [w * stride for w in range(9)]
        assert np.array_equal(st, pst) and st.tolist() == [0, 0, 0, 0, RR.ERR_PAYLOAD_CRC, BAD, BAD, 0]
        assert (packed[total:] == 0x5A).all() and (padded[len(lens) * stride:] == 0x5A).all()
        for w, r in enumerate(rows):
            a, b = int(off[w]), int(poff[w])
            assert np.array_equal(packed[a:a + r], padded[b:b + r])
            assert np.array_equal(R.view(padded[b + r:b + stride]), LR.empty(stride - r))
            assert np.array_equal(R.view(packed[a:a + r]), R.one(damaged, so, starts[w], lens[w], bin_len)[0])


def test_layout_refusals_and_rows_without_room(base):
    frames, so, wav, _ = base
    starts, lens = [0, 400, 5, 800], [400, 400, 0, 400]
    out, off, st = R.range_levels(frames, so, starts, lens, 100, 0, 6)          # rows 4, 4, 1, 4; the second is cut
    assert off.tolist() == [0, 4, 8, 9, 13] and st.tolist() == [0, BAD, BAD, BAD]
    assert np.array_equal(R.view(out[:4]), _brute(wav, 0, 400, 100)) and (out[4:] == 0x5A).all()
    out, off, st = R.range_levels(frames, so, starts, lens, 100, 2, 9)          # a stride below R(w): a row of identities
    assert st.tolist() == [BAD, BAD, 0, BAD] and np.array_equal(R.view(out[:8]), LR.empty(8)) and (out[8:] == 0x5A).all()
    for bad_call in (([], [], 0, 4), (starts, lens, 4, 15), (starts, lens, 0, 0)):
        with pytest.raises(ValueError):
            R.range_levels(frames, so, bad_call[0], bad_call[1], 100, bad_call[2], bad_call[3])
