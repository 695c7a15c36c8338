"""ranges_ref.py, the numpy statement of x3_decode_ranges_dev's definition, on hand-made frames."""
import numpy as np
import pytest

import ranges_ref as R

FILL = 0x5A5A
BAD = R.ERR_BAD_ARG


def _frames(lengths, bad=()):
    """frames whose sample at position g is g + 1 (never 0, never the fill)"""
    so = R.sample_offsets(lengths)
    frames = [(14, None) if f in bad else (0, np.arange(int(so[f]) + 1, int(so[f + 1]) + 1, dtype=np.int16))
              for f in range(len(lengths))]
    return frames, so


def _i16(v):
    return np.array(v, dtype=np.int16)


def test_single_windows_prefix_zeros_and_first_failing_frame():
    frames, so = _frames([4, 4, 3], bad=(1,))
    assert R.one(frames, so, 0, 4)[1] == 0 and R.one(frames, so, 0, 4)[0].tolist() == [1, 2, 3, 4]
    row, st = R.one(frames, so, 2, 7)                      # covers frames 0, 1, 2: exact in front of frame 1, zeros behind
    assert st == 14 and row.tolist() == [3, 4, 0, 0, 0, 0, 0]
    row, st = R.one(frames, so, 5, 2)                      # inside the failing frame
    assert st == 14 and not row.any()
    row, st = R.one(frames, so, 8, 3)                      # behind it: clean
    assert st == 0 and row.tolist() == [9, 10, 11]
    assert R.one(frames, so, 8, 4)[1] == BAD and R.one(frames, so, 2 ** 63, 1)[1] == BAD
    assert R.one(frames, so, 11, 0)[1] == 0 and R.one(frames, so, 12, 0)[1] == BAD   # a length of 0: start <= total


def test_packed_rows_lie_at_the_sum_of_all_lengths():
    frames, so = _frames([5, 5])
    starts, lens = [0, 9, 3, 10, 4], [3, 2, 0, 0, 6]       # (9, 2) is off the end: BAD, zeros, and its length counts
    out, off, st = R.ranges(frames, so, starts, lens, 0, 12, FILL)
    assert off.tolist() == [0, 3, 5, 5, 5, 11] and st.tolist() == [0, BAD, 0, 0, 0]
    assert out.tolist() == [1, 2, 3, 0, 0, 5, 6, 7, 8, 9, 10, FILL]


def test_packed_capacity_refuses_rows_without_room_and_writes_nothing_of_them():
    frames, so = _frames([5, 5])
    out, off, st = R.ranges(frames, so, [0, 2, 0, 7, 1], [4, 5, 1, 0, 1], 0, 6, FILL)
    assert off.tolist() == [0, 4, 9, 10, 10, 11]           # complete, whatever fits
    assert st.tolist() == [0, BAD, BAD, BAD, BAD]          # row 1 is cut by the capacity; rows behind the capacity too
    assert out.tolist() == [1, 2, 3, 4, FILL, FILL]
    out, off, st = R.ranges(frames, so, [0, 2, 9], [4, 5, 0], 0, 9, FILL)
    assert st.tolist() == [0, 0, 0] and out.tolist() == [1, 2, 3, 4, 3, 4, 5, 6, 7]   # a length of 0 at the capacity fits


def test_padded_rows_tails_and_a_length_above_the_stride():
    frames, so = _frames([5, 5], bad=(1,))
    out, off, st = R.ranges(frames, so, [0, 3, 0, 8, 10], [2, 4, 5, 1, 0], 4, 21, FILL)
    assert off.tolist() == [0, 4, 8, 12, 16, 20] and st.tolist() == [0, 14, BAD, 14, 0]
    assert out.tolist() == [1, 2, 0, 0, 4, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, FILL]
    with pytest.raises(ValueError):
        R.ranges(frames, so, [0, 0], [1, 1], 4, 7, FILL)   # n * stride > capacity: the call is refused
    with pytest.raises(ValueError):
        R.ranges(frames, so, [], [], 0, 7, FILL)


def test_frames_of_checks_crcs_and_sample_offsets_on_an_encoded_stream():
    import oracle_lib as O
    wav = (np.arange(950) % 37 - 18).astype(np.int16)
    op = O.Params.make(20, 20)
    rc, s, _ = O.encode(wav, op)
    assert rc == 0
    offs = R.frame_offsets(s)
    assert len(offs) == 4
    fr = R.frames_of(s, offs, op)
    so = R.sample_offsets([len(w) for _, w in fr])
    assert so.tolist() == [0, 400, 800, 950] and np.array_equal(np.concatenate([w for _, w in fr]), wav)
    out, off, st = R.ranges(fr, so, [390, 0], [20, 950], 0, 970)
    assert not st.any() and np.array_equal(out[:20], wav[390:410]) and np.array_equal(out[20:], wav)
    bad = s.copy()
    bad[offs[1] + 25] ^= 1
    bad[offs[2] + 2] ^= 1
    assert [a for a, _ in R.frames_of(bad, offs, op)] == [0, R.ERR_PAYLOAD_CRC, R.ERR_HEADER_CRC]
    so2 = so.copy()
    so2[1] += 1
    assert [a for a, _ in R.frames_of(s, offs, op, so2)] == [BAD, BAD, 0]
    assert np.array_equal(R.f32_bits(_i16([-32768, 1])), np.array([-1.0, 2.0 ** -15], dtype=np.float32).view(np.uint32))
