"""FIR range levels (include/x3hip.h, "FIR RANGE LEVELS"): x3_fir_range_levels_dev, x3_corpus_fir_range_levels_dev and the
Python surface.  Every record, offset and status is compared with == against fir_range_levels_ref.py, the definition written
from the CPU oracle's decode (all five fields are integers: no tolerance anywhere); every output array is filled with 0x5A
first and carries canary bytes behind its end (test_gpu_range_levels.py's run(), whose helpers these tests use).

The base stream is that file's: 2 137 samples in frames of 400 (block length 20, seg_blocks 4: five stretches a frame, the
second from sample 81), five whole frames and one of 137."""
import ctypes as C

import numpy as np
import pytest

import fir_range_levels_ref as FR
import levels_ref as LR
import oracle_lib as O
import ranges_ref as RR
import seg_index_ref as SR
import signal_range_levels_ref as S
import test_gpu_range_levels as T
from x3_cases import refresh_crcs

pytestmark = pytest.mark.gpu

BAD, CRC, N, SB, REC = T.BAD, T.CRC, T.N, T.SB, T.REC
STARTS = [0, 1, 6, 7, 8, 80, 81, 87, 88, 399, 400, 401, 406, 407, 408, 799, 800, 2136]
BINS = [0, 1, 7, 20, 400, 401, 2 ** 32]
EIGHT = ((3, -5, 7, -11, 13, -17, 19, -23), 7)
FIRS = [((1,), 0), ((1, -1), 0), ((1, -2, 1), 0), ((1, 0, -1), 0), EIGHT, ((-3, 2), 15)]     # (the last: negative sums, floor)


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def call(dev, fir, seg=True, d_so=None):
    """the enqueue function of T.run: x3_fir_range_levels_dev on dev's stream (d_so: other sample offsets than its own)"""
    idx = dev.d_seg if seg else None
    f = dev.x3.Fir(*fir)

    def enqueue(d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status):
        return dev.ctx.fir_range_levels_dev(dev.d_x3, dev.len, dev.d_off, d_so or dev.d_so, dev.F, dev.p, d_starts, d_lens, n,
                                            bin_len, stride, d_levels, cap, d_off, d_status, idx, dev.sb if idx else 0, f)
    return enqueue


def compare(got, want, lens, bin_len, what=""):
    assert np.array_equal(got[2], want[2]), (what, np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
    assert np.array_equal(got[1], want[1])
    T.same(got[0], want[0], what)
    assert got[3] == T.rows_total(lens, bin_len)


def check(ctx, dev, frames, starts, lens, bin_len, stride, cap, fir, seg=True, so=None, d_so=None, want=None):
    got = T.run(ctx, call(dev, fir, seg, d_so), starts, lens, bin_len, stride, cap)
    if want is None:
        want = FR.range_levels(frames, dev.so if so is None else so, starts, lens, bin_len, stride, cap, *fir)
    compare(got, want, lens, bin_len, (fir, bin_len, stride))
    return got


def grid(starts=STARTS, lens=T.LENS):
    """every length at every start (those off the end are ERR_BAD_ARG), in an order that is not sorted"""
    tab = [(s, ln) for s in starts for ln in lens]
    np.random.default_rng(5).shuffle(tab)
    return [s for s, _ in tab], [ln for _, ln in tab]


def layouts(lens, bin_len):
    """packed with room for all, padded to a stride that refuses the longest ranges: (stride, cap)"""
    stride = min(max(FR.rows_of(v, bin_len) for v in lens), 25)
    return (0, T.rows_total(lens, bin_len)), (stride, len(lens) * stride + 3)


def both_layouts(ctx, dev, frames, starts, lens, bin_len, fir, seg=True):
    out = None
    for stride, cap in reversed(layouts(lens, bin_len)):
        out = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, fir, seg)
    return out                                                # (the packed one)


# ------------------------------------------------------------------------------------------------ starts, lengths, bins, layouts

@pytest.mark.parametrize("bin_len", BINS)
@pytest.mark.parametrize("fir", FIRS, ids=lambda f: "T%d" % len(f[0]) + ("s%d" % f[1] if f[1] else ""))
def test_every_length_at_every_start_at_every_bin_length(ctx, x3, fir, bin_len):
    """starts at a frame's and a stretch's first sample and T - 1 either side of them (0, 400, 800; 81; 6 / 7 / 8, 87 / 88,
    406 / 407 / 408), at a frame's last sample (399, 799, 2 136); the encoder's index, a walk-built one and none give the
    same bytes, the reference is computed once for the three"""
    starts, lens = grid()
    wants = None
    for index in ("ref", "walk", None):
        dev = T.base(ctx, x3, index)
        assert dev.total == N and dev.F == 6
        frames = dev.frames()
        if wants is None:
            wants = [FR.range_levels(frames, dev.so, starts, lens, bin_len, stride, cap, *fir) for stride, cap in layouts(lens, bin_len)]
        for (stride, cap), want in zip(layouts(lens, bin_len), wants):
            out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, fir, seg=index is not None, want=want)
            assert ctx.get_option("last_range_levels_replays") == 0 and ctx.get_option("last_range_levels_overflow") == 0
        dev.close()
    out, off, st = wants[0]
    assert (st == BAD).any() and (st == 0).any()
    need = len(fir[0]) - 1
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # n counts filter outputs: one per position from T - 1 on
        if st[w] == 0:
            assert int(FR.view(out[int(off[w]):int(off[w + 1])])["n"].sum()) == max(0, ln - max(0, need - s0)), (s0, ln)


@pytest.mark.parametrize("bl, bpf, codes", [(10, 40, (0, 1, 3)), (40, 10, (0, 1, 3)), (20, 20, (1, 1, 3))])
def test_block_lengths_and_code_sets(ctx, x3, bl, bpf, codes):
    for index in ("walk", None):
        dev = T.base(ctx, x3, index, bl, bpf, codes)
        assert dev.F == 6 and dev.so[1] == 400
        first = 1 + SB * bl                                   # the second stretch's first sample
        starts, lens = grid([0, 1, 7, first - 1, first, first + 6, first + 7, 400, 400 + first, 406, 800, 2136], [0, 1, 21, 400, 401, N])
        for bin_len, fir in ((0, EIGHT), (7, FIRS[2]), (400, EIGHT)):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, fir, seg=index is not None)
            if not any(st for st, _ in dev.frames()):             # (with codes (1, 1, 3) frames fail to decode: the reader's)
                assert ctx.get_option("last_range_levels_replays") == 0
        dev.close()


def _short_frames(values, per, op):
    parts = []
    for i in range(0, len(values), per):
        rc, s, _ = O.encode(np.array(values[i:i + per], dtype=np.int16), op)
        assert rc == 0
        parts.append(s)
    return np.concatenate(parts)


VALUES = [5, -32768, 32767, 0, -7, 32767, -32768, 11, 12, -300, 4000, -32768, 32767, 32767, -1, 77, 31000, -31000, 9, 8, 7]


@pytest.mark.parametrize("per, lead", [(1, 7), (3, 3)])
def test_short_frames_and_eight_taps(ctx, x3, per, lead):
    """frames of one sample: seven lead frames in front of a range far enough in; frames of three: three lead frames, and every
    stretch is shorter than T - 1.  Every counted position takes samples of up to eight frames"""
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    dev = T.Dev(ctx, x3, _short_frames(VALUES, per, op), p, op, None)
    assert dev.F == len(VALUES) // per and dev.total == len(VALUES)
    starts, lens = grid(list(range(len(VALUES) + 1)), [0, 1, 2, 3, 9, len(VALUES)])
    for fir in (EIGHT, ((16384, -16384), 0), ((1, 0, -1), 0), ((1, 1, 1, 1), 2)):
        for bin_len in (0, 1, 2, 4):
            out, off, st, _ = both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, fir, seg=False)
    assert ctx.get_option("last_range_levels_replays") == 0
    # a range that starts 7 or more positions in has an output at every position, all of them from the frames in front
    s0 = 3 * lead if per == 3 else 9
    out, off, st, _ = check(ctx, dev, dev.frames(), [s0, s0], [1, 5], 0, 0, 2, EIGHT, seg=False)
    assert st.tolist() == [0, 0] and FR.view(out)["n"].tolist() == [1, 5]
    dev.close()


def test_a_stream_of_one_sample(ctx, x3):
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    dev = T.Dev(ctx, x3, _short_frames([-4321], 1, op), p, op, None)
    for fir in (EIGHT, FIRS[1]):
        for bin_len in (0, 1):
            out, off, st, _ = check(ctx, dev, dev.frames(), [0, 0, 1, 1], [1, 0, 0, 1], bin_len, 0, 4, fir, seg=False)
            assert st.tolist() == [0, 0, 0, BAD] and np.array_equal(FR.view(out), LR.empty(4))     # n == 0 everywhere
    out, off, st, _ = check(ctx, dev, dev.frames(), [0], [1], 0, 0, 1, FIRS[0], seg=False)
    assert FR.view(out)["n"].tolist() == [1] and FR.view(out)["min"].tolist() == [-4321]
    dev.close()


def test_a_saturating_pair_on_a_full_scale_alternation(ctx, x3):
    """{16384, -16384} on +-32767 alternating: every sum is +-2^30 less a little, every output clamps"""
    w = np.where(np.arange(900) % 2 == 0, 32767, -32768).astype(np.int16)
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    rc, s, _ = O.encode(w, op)
    assert rc == 0
    words = SR.build(s, RR.frame_offsets(s)[:-1], op, SB)[0]
    dev = T.Dev(ctx, x3, s, p, op, words)
    fir = ((16384, -16384), 0)
    starts, lens = [0, 1, 399, 400, 401, 80, 81, 82, 500], [900, 899, 3, 400, 20, 3, 3, 3, 400]
    for bin_len in (0, 1, 7, 400):
        out, off, st, _ = both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, fir)
    rec = FR.view(out[int(off[0]):int(off[1])])
    assert rec["n"].sum() == 899 and rec["min"].min() == -32768 and rec["max"].max() == 32767
    dev.close()


# ------------------------------------------------------------------------------------------------ against existing GPU paths

def _fir_levels(dev, bin_len, n_bins, fir):
    d_lv, d_st = dev.alloc(REC * n_bins), dev.alloc(4 * dev.F)
    assert dev.ctx.fir_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, dev.d_seg,
                                  dev.sb, dev.x3.Fir(*fir)) == 0
    assert dev.ctx.levels_result()[0] == 0
    return dev.ctx.download(d_lv, REC * n_bins, LR.LEVEL_DTYPE), dev.ctx.download(d_st, 4 * dev.F, np.int32)


def _hurt(ctx, x3, f, at=30):
    """the base stream with a payload byte of frame f flipped, under the intact stream's index"""
    clean = T.base(ctx, x3)
    s = clean.stream.copy()
    s[clean.offs[f] + 20 + at] ^= 0x08
    dev = T.Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    clean.close()
    assert [st for st, _ in dev.frames()] == [CRC if g == f else 0 for g in range(6)]
    return dev


@pytest.mark.parametrize("hurt", [None, 0, 2, 5])
def test_the_whole_stream_equals_x3_fir_levels_dev(ctx, x3, hurt):
    dev = T.base(ctx, x3) if hurt is None else _hurt(ctx, x3, hurt)
    for fir in (FIRS[3], EIGHT):
        for bin_len in BINS:
            n_bins = FR.rows_of(N, bin_len)
            lv, fst = _fir_levels(dev, bin_len, n_bins, fir)
            out, off, st, total = T.run(ctx, call(dev, fir), [0], [N], bin_len, 0, n_bins)
            assert total == n_bins and st.tolist() == [0 if hurt is None else CRC]
            assert np.array_equal(FR.view(out), lv), (fir, bin_len)
        if hurt is None:
            assert int(lv["n"].sum()) == N - (len(fir[0]) - 1)
        # ... and bin-aligned ranges are slices of those records, the last one cut to the range's length
        lv, _ = _fir_levels(dev, 100, 22, fir)
        starts, lens = [0, 400, 800, 300, 2000, 1900, 100], [400, 400, 1337, 250, 137, 200, 2037]
        out, off, st, _ = T.run(ctx, call(dev, fir), starts, lens, 100, 0, T.rows_total(lens, 100))
        for w, (s0, ln) in enumerate(zip(starts, lens)):
            got = FR.view(out[int(off[w]):int(off[w + 1])])
            assert np.array_equal(got[:ln // 100], lv[s0 // 100:(s0 + ln) // 100]), (s0, ln)
            if s0 + ln == N:
                assert np.array_equal(got[-1], lv[-1])
    dev.close()


def test_one_tap_is_x3_range_levels_dev_and_the_pair_is_the_difference_byte_for_byte(ctx, x3):
    dev = _hurt(ctx, x3, 2)
    starts, lens = T.base_ranges(seed=7)
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 25)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len) - 5        # (packed: the last ranges have no room)
        old = T.run(ctx, dev.call, starts, lens, bin_len, stride, cap)
        new = T.run(ctx, call(dev, ((1,), 0)), starts, lens, bin_len, stride, cap)
        assert all(np.array_equal(a, b) for a, b in zip(new[:3], old[:3])) and new[3] == old[3]

        def diff(d_starts, d_lens, n, bl, st, d_levels, c, d_off, d_status):
            return ctx.signal_range_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_starts, d_lens, n, bl, st,
                                               d_levels, c, d_off, d_status, dev.d_seg, dev.sb, S.DIFF)
        old = T.run(ctx, diff, starts, lens, bin_len, stride, cap)
        new = T.run(ctx, call(dev, ((1, -1), 0)), starts, lens, bin_len, stride, cap)
        assert all(np.array_equal(a, b) for a, b in zip(new[:3], old[:3])) and new[3] == old[3]
    dev.close()


# ------------------------------------------------------------------------------------------------ damage

DAMAGE_RANGES = ([0, 100, 799, 800, 900, 1199, 700, 0, 799, 1200, 1201, 1600, 1199, 400, 800, 1200, 1200, 81, 1206, 1207, 1203],
                 [800, 50, 1, 400, 100, 1, 600, N, 402, 400, 936, 537, 2, 400, 1, 1, 937, 1500, 10, 10, 3])


def _damage_check(ctx, dev, frames, fir=EIGHT):
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(DAMAGE_RANGES[0]) + starts, list(DAMAGE_RANGES[1]) + lens
    got = None
    for bin_len, stride in ((7, 0), (400, 0), (0, 0), (100, 25)):
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len), fir)
    return starts, lens, got


@pytest.mark.parametrize("f", [0, 2, 5])
def test_a_payload_crc_failure_takes_the_frame_and_the_positions_behind_it(ctx, x3, f):
    dev = _hurt(ctx, x3, f)
    frames = dev.frames()
    a, b = int(dev.so[f]), int(dev.so[f + 1])
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # the status is the SAMPLES call's: covering frames only
        covers = ln and s0 < b and s0 + ln > a and s0 <= N and ln <= N - s0
        assert (st[w] == CRC) == bool(covers), (s0, ln, st[w])
    assert ctx.get_option("last_range_levels_replays") == 0
    # the whole stream in one bin: the frame's positions and the T - 1 behind it are missing, and the entry's first T - 1
    for fir in (FIRS[3], EIGHT):
        need = len(fir[0]) - 1
        one = check(ctx, dev, frames, [0], [N], 0, 0, 1, fir)
        lost = (b - a) + (need if b < N else 0) + (need if a else 0)
        assert int(FR.view(one[0])["n"][0]) == N - lost
    dev.close()


def test_a_damaged_lead_frame_costs_the_positions_whose_taps_reach_it_and_not_the_status(ctx, x3):
    dev = _hurt(ctx, x3, 0)
    clean = T.base(ctx, x3)
    starts, lens = [400, 400, 0, 401, 400, 402, 403], [400, 1, 400, 399, 0, 10, 10]
    fir = FIRS[3]                                              # {1, 0, -1}: two positions
    out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, 0, 0, 7, fir)
    assert st.tolist() == [0, 0, CRC, 0, 0, 0, 0] and FR.view(out)["n"].tolist() == [398, 0, 0, 398, 0, 10, 10]
    ref, _, rst, _ = check(ctx, clean, clean.frames(), starts, lens, 0, 0, 7, fir)
    assert not rst.any() and FR.view(ref)["n"].tolist() == [400, 1, 398, 399, 0, 10, 10]
    assert np.array_equal(out[5], ref[5])                      # (402, 10) never looks at frame 0
    out, off, st, _ = check(ctx, dev, dev.frames(), [400, 406, 407], [400, 10, 10], 0, 0, 3, EIGHT)
    assert st.tolist() == [0, 0, 0] and FR.view(out)["n"].tolist() == [393, 9, 10]
    dev.close()
    clean.close()


def test_the_second_of_three_lead_frames_is_damaged(ctx, x3):
    """frames of three samples, eight taps: a range at frame 4's first sample (12) has lead frames 1, 2 and 3; frame 2 (samples
    6 .. 8) fails: the positions 12 .. 15, whose taps reach sample 8 or further back, are gone, the status is 0"""
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    s = _short_frames(VALUES, 3, op)
    offs = RR.frame_offsets(s)
    s[offs[2] + 20] ^= 0x10
    dev = T.Dev(ctx, x3, s, p, op, None)
    frames = dev.frames()
    assert [st for st, _ in frames] == [CRC if f == 2 else 0 for f in range(7)]
    starts, lens = [12, 12, 16, 15, 9, 6, 0], [9, 4, 5, 6, 12, 3, 21]
    for bin_len in (0, 1, 4):
        out, off, st, _ = both_layouts(ctx, dev, frames, starts, lens, bin_len, EIGHT, seg=False)
    out, off, st, _ = check(ctx, dev, frames, starts, lens, 0, 0, 7, EIGHT, seg=False)
    assert st.tolist() == [0, 0, 0, 0, 0, CRC, CRC] and FR.view(out)["n"].tolist() == [5, 0, 5, 5, 5, 0, 5]
    assert ctx.get_option("last_range_levels_replays") == 0
    dev.close()


def _late_error(ctx, x3):
    clean = T.base(ctx, x3)
    s = clean.stream.copy()
    o = clean.offs[2]
    plen = int(s[o + 6]) << 8 | int(s[o + 7])
    payload = s[o + 20:o + 20 + plen].copy()
    rc2 = 0
    for at in range(40, plen - 16, 37):                       # (test_gpu_range_levels.py: a zero run until the frame fails)
        s[o + 20:o + 20 + plen] = payload
        s[o + 20 + at:o + 20 + at + 12] = 0
        rc2 = O.decode_frame(s[o + 20:o + 20 + plen], 400, clean.op)[0]
        if rc2:
            break
    assert rc2, "no zero run made frame 2 fail to decode"
    refresh_crcs(s, o)
    dev = T.Dev(ctx, x3, s, clean.p, clean.op, ctx.download(clean.d_seg, 8 * SR.n_words(6, clean.op, SB), np.uint64))
    clean.close()
    return dev, rc2


def test_a_late_decode_error_goes_through_the_reader_and_the_fixup_takes_the_fronts(ctx, x3):
    dev, rc2 = _late_error(ctx, x3)
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, rc2, 0, 0, 0] and rc2 not in (CRC, BAD)
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    assert ctx.get_option("last_range_levels_replays") > 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == rc2) == bool(covers), (s0, ln, st[w])
    out, off, st, _ = check(ctx, dev, frames, [1200, 0], [400, N], 0, 0, 2, EIGHT)     # frame 2 as a lead frame that fails late
    assert st.tolist() == [0, rc2] and FR.view(out)["n"].tolist() == [393, N - 7 - 400 - 7]
    assert ctx.get_option("last_range_levels_replays") == 2
    dev.close()


@pytest.mark.parametrize("how", ["bit", "sample"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """frame 2, entry 2: a bit position one late, or a last sample with its lowest bit flipped.  The FIR signal takes no seed
    from the index, but x3w_stretch's proof does read it: the stretch in front ends on another sample than the entry names (and
    the stretch behind predicts from the entry's), so the frame is flagged either way, goes through the reader in the fix-up,
    which forms its positions and the front of frame 3 from the history it carries, and the bytes are the same"""
    dev = T.base(ctx, x3)
    frames = dev.frames()
    nw = SR.n_words(6, dev.op, SB)
    good = ctx.download(dev.d_seg, 8 * nw, np.uint64)
    per = (nw - 1) // 6
    bad = good.copy()
    bad[1 + 2 * per + 1] = bad[1 + 2 * per + 1] + np.uint64(1) if how == "bit" else bad[1 + 2 * per + 1] ^ np.uint64(1 << 32)
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(DAMAGE_RANGES[0]) + starts, list(DAMAGE_RANGES[1]) + lens
    for bin_len, stride in ((7, 0), (0, 0), (100, 25)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        ctx.upload(dev.d_seg, good)
        want = T.run(ctx, call(dev, EIGHT), starts, lens, bin_len, stride, cap)
        assert ctx.get_option("last_range_levels_replays") == 0
        ctx.upload(dev.d_seg, bad)
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, EIGHT)
        assert ctx.get_option("last_range_levels_replays") > 0
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    dev.close()


def test_sample_offsets_of_another_stream(ctx, x3):
    """frames of 300 by the caller's offsets: five frames fail their check with ERR_BAD_ARG; the last frame agrees and counts,
    without its first T - 1 positions"""
    dev = T.base(ctx, x3)
    so = np.array([0, 300, 600, 900, 1200, 1500, 1637], dtype=np.uint64)
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    frames = dev.frames(so)
    assert [st for st, _ in frames] == [BAD] * 5 + [0]
    starts, lens = [0, 1200, 1500, 1501, 1400, 1637, 1500, 1638], [1637, 437, 137, 136, 200, 0, 138, 0]
    for bin_len, stride in ((0, 0), (7, 0), (100, 20)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, FIRS[3], so=so, d_so=d_so)
        assert st.tolist() == [BAD, BAD, 0, 0, BAD, 0, BAD, BAD]
    one = check(ctx, dev, frames, starts, lens, 0, 0, len(starts), FIRS[3], so=so, d_so=d_so)[0]
    assert FR.view(one)["n"].tolist() == [135, 135, 135, 135, 98, 0, 0, 0]
    dev.close()


# ------------------------------------------------------------------------------------------------ shared frames

@pytest.mark.parametrize("n, overflow", [(2, 0), (40, 16)])
def test_ranges_that_all_cover_all_six_frames(ctx, x3, n, overflow):
    """40 ranges over 6 frames are 240 pairs against P = min(40 * 6, 4 * (6 + 40) + (T - 1) * 40): all 240 with three taps,
    224 with two, 184 with one.  The pairs beyond go through the reader, their positions and the fronts next to them are the
    fix-up's, and the records are the same"""
    dev = T.base(ctx, x3)
    starts = [w % 3 for w in range(n)]
    lens = [N - 2 - (w % 5) for w in range(n)]
    for bin_len in (0, 7, 400):
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), FIRS[3])
        assert ctx.get_option("last_range_levels_overflow") == 0 and ctx.get_option("last_range_levels_replays") == 0
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), FIRS[0])
        over = max(0, n * 6 - 4 * (6 + n))
        assert ctx.get_option("last_range_levels_overflow") == over and ctx.get_option("last_range_levels_replays") == over
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), FIRS[1])
        assert ctx.get_option("last_range_levels_overflow") == overflow and ctx.get_option("last_range_levels_replays") == overflow
    dev.close()


def test_lead_frames_beyond_the_pairs_the_workspace_holds(ctx, x3):
    """60 ranges (400, 1737) with two taps: a lead frame and five covering frames each, 360 pairs against P = min(360, 4 * 66 +
    60) = 324; the fix-up replays the 36 pairs beyond and forms the fronts next to them"""
    dev = T.base(ctx, x3)
    starts, lens = [400] * 60, [1737 - (w % 4) for w in range(60)]
    for bin_len in (0, 400):
        out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), FIRS[1])
        assert ctx.get_option("last_range_levels_overflow") == 36 and ctx.get_option("last_range_levels_replays") == 36
        assert not st.any()
    dev.close()


def test_two_ranges_share_a_frame_that_is_a_lead_frame_of_one_only(ctx, x3):
    for dev, want_st in ((T.base(ctx, x3), [0, 0, 0, 0, 0]), (_hurt(ctx, x3, 0), [0, CRC, CRC, 0, 0])):
        starts, lens = [400, 0, 100, 403, 407], [400, 400, 500, 401, 30]
        for bin_len in (0, 100):
            out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), EIGHT)
            assert st.tolist() == want_st
        dev.close()


def test_more_ranges_than_threads_of_the_scans(ctx, x3):
    dev = T.base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 60, 3000).tolist()
    starts = (rng.integers(0, (N - 60) // 20, 3000) * 20 + rng.integers(0, 8, 3000)).tolist()   # many near frame and stretch starts
    check(ctx, dev, dev.frames(), starts, lens, 7, 0, T.rows_total(lens, 7), EIGHT)
    check(ctx, dev, dev.frames(), starts, lens, 0, 2, 6000, FIRS[2])
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

ENTRY_SAMPLES = (1, 399, N, 0, 1000, 400, 5)


def _corpus(ctx, x3, index):
    """a one-sample, a one-frame, a six-frame, an empty entry, one with a payload-CRC failure in its frame 1, one more frame,
    and an entry shorter than T - 1"""
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    ents, parts, offsets, pos = [], [], [], 0
    for e, n in enumerate(ENTRY_SAMPLES):
        s = np.zeros(0, dtype=np.uint8)
        if n:
            rc, s, _ = O.encode(x3.synth(2, 700 + e, 0, n), op)
            assert rc == 0
        if e == 4:
            s = s.copy()
            s[RR.frame_offsets(s)[1] + 20 + 11] ^= 0x40
        pad = np.zeros(1 if pos % 2 == 0 else 2, dtype=np.uint8)
        parts += [pad, s]
        offsets.append(pos + pad.size)
        pos += pad.size + s.size
        ents.append(s)
    buf = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf, offsets, [s.size for s in ents], params=p, seg_blocks=SB, index=index)
    assert corpus.entries["n_samples"].tolist() == list(ENTRY_SAMPLES)
    return corpus, [T.Dev(ctx, x3, s, p, op, None) if s.size else None for s in ents]


@pytest.mark.parametrize("index", ["decode", "walk"])
def test_corpus_ranges_equal_the_stream_form_on_each_entry(ctx, x3, index):
    corpus, devs = _corpus(ctx, x3, index)
    ne = len(ENTRY_SAMPLES)
    tab = [(e, 0, n) for e, n in enumerate(ENTRY_SAMPLES)] + [(e, 0, 1) for e in range(ne)] + [(e, 0, 0) for e in range(ne + 1)]
    tab += [(2, 400, 400), (2, 800, 1337), (2, 81, 1000), (2, 401, 5), (2, 6, 3), (2, 7, 3), (4, 400, 400), (4, 800, 200), (4, 0, 400),
            (4, 399, 2), (4, 803, 9), (4, 0, 1000), (1, 398, 1), (1, 0, 8), (5, 399, 1), (5, 1, 399), (5, 0, 7), (6, 0, 5), (6, 4, 1),
            (ne, 0, 1), (2 ** 32 - 1, 0, 0), (3, 1, 0), (0, 1, 0), (1, 399, 1), (2, N, 1), (5, 2 ** 63, 1)]
    np.random.default_rng(2).shuffle(tab)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    seen = set()
    fir = x3.Fir(*EIGHT)
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 22)):
        cap = len(tab) * stride or T.rows_total(lens, bin_len)
        out, off, st, total = T.run(ctx, lambda *a: corpus.fir_range_levels_into(*a, fir), starts, lens, bin_len, stride, cap,
                                    entries=ent)
        assert total == T.rows_total(lens, bin_len)
        for w, (e, s0, ln) in enumerate(tab):
            rows = stride or FR.rows_of(ln, bin_len)
            mine = out[int(off[w]):int(off[w]) + rows]
            if e >= ne or devs[e] is None:
                assert st[w] == BAD, (e, s0, ln)             # not in the corpus, or an entry without frames
                assert np.array_equal(FR.view(mine), LR.empty(rows)), (e, s0, ln)
                continue
            d = devs[e]
            want = FR.range_levels(d.frames(), d.so, [s0], [ln], bin_len, stride, rows, *EIGHT)
            one = T.run(ctx, call(d, EIGHT, seg=False), [s0], [ln], bin_len, stride, rows)     # the stream form, on that entry alone
            assert st[w] == one[2][0] == want[2][0], (e, s0, ln, st[w])
            T.same(mine, one[0], (e, s0, ln))
            T.same(one[0], want[0], (e, s0, ln))
            seen.add(int(st[w]))
            if s0 == 0 and ln == ENTRY_SAMPLES[e] and e != 4:      # no history crosses an entry's start
                assert int(FR.view(mine)["n"].sum()) == max(0, ln - 7)
    assert seen == {0, BAD, CRC}
    assert ctx.get_option("last_range_levels_replays") == 0
    for d in devs:
        if d is not None:
            d.close()
    corpus.close()


# ------------------------------------------------------------------------------------------------ refusals, pending state

def test_refusals_and_pending_states(ctx, x3):
    L = x3.lib()
    dev = _hurt(ctx, x3, 2)
    n, cap = 4, 64
    sizes = {"lv": REC * cap, "off": 8 * (n + 1), "st": 4 * n}
    d = {k: dev.alloc(v) for k, v in sizes.items()}
    d_starts, d_lens = dev.alloc(8 * n), dev.alloc(4 * n)
    ctx.upload(d_starts, np.array([0, 400, 800, 1200], dtype=np.uint64))
    ctx.upload(d_lens, np.full(n, 400, dtype=np.uint32))
    for k, v in sizes.items():
        ctx.upload(d[k], np.full(v, 0x5A, dtype=np.uint8))
    ok = x3.Fir([1, 0, -1]).c_struct()

    def raw(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=SB, starts=d_starts,
            lens=d_lens, nr=n, bl=100, stride=0, lv=d["lv"], rows=cap, off=d["off"], st=d["st"], fir=ok):
        return L.x3_fir_range_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, starts, lens, nr, bl, stride, lv,
                                         rows, off, st, C.byref(fir) if fir is not None else None)
    bad_firs = [None, x3.LevelFir(0, 0, (C.c_int16 * 8)()), x3.LevelFir(9, 0, (C.c_int16 * 8)(1)),
                x3.LevelFir(1, 16, (C.c_int16 * 8)(1)), x3.LevelFir(3, 0, (C.c_int16 * 8)(16384, -16384, 1))]
    for fir in bad_firs:                                        # a NULL or invalid fir is refused first: whatever else is wrong
        assert raw(fir=fir) == BAD and raw(fir=fir, x=None, nr=0) == BAD
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert raw(fir=None, params=bad_p) == BAD and raw(params=bad_p) != 0
    for r in (dict(c=None), dict(nr=0), dict(nr=2 ** 31), dict(rows=0), dict(rows=2 ** 31), dict(starts=None), dict(lens=None),
              dict(lv=None), dict(st=None), dict(off=None), dict(starts=d_starts + 4), dict(lens=d_lens + 2), dict(lv=d["lv"] + 4),
              dict(off=d["off"] + 4), dict(st=d["st"] + 2), dict(sb=3), dict(sb=0), dict(stride=17), dict(stride=2 ** 63),
              dict(x=None), dict(fo=dev.d_off + 4), dict(so=dev.d_so + 4)):
        assert raw(**r) == BAD, r
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, bin_len=100, row_stride=0, d_levels=d["lv"], rows_cap=cap,
               d_row_offsets=d["off"], d_status=d["st"], fir=ok)
    for r in [dict(fir=f) for f in bad_firs] + [dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(rows_cap=0),
                                                 dict(d_starts=None), dict(d_levels=d["lv"] + 4), dict(d_row_offsets=None),
                                                 dict(row_stride=17)]:
        assert corpus.fir_range_levels_into(**dict(cok, **r)) == BAD, r
    assert L.x3_corpus_fir_range_levels_dev(ctx._h, None, d_ent, d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"],
                                            C.byref(ok)) == BAD
    ctx.graph_begin()
    try:
        assert raw() == BAD and corpus.fir_range_levels_into(**cok) == BAD      # a context that records a graph
    finally:
        try:
            ctx.graph_destroy(ctx.graph_end())
        except x3.X3Error:
            pass                                                                 # (a recording of nothing)
    assert ctx.range_levels_result()[0] == BAD                               # nothing is pending
    ctx.sync()
    for k, v in sizes.items():
        assert (ctx.download(d[k], v) == 0x5A).all(), k                      # ... and nothing was enqueued
    # beside the levels, events and ranges calls: four pending slots, each result call answers its own
    bin_len, ecap = 50, 16
    n_bins = FR.rows_of(N, bin_len)
    rule = x3.EventRule.make(peak_min=1, join_bins=0, pad_bins=0, max_bins=4)
    d_l, d_es, d_el, d_ev, d_cnt = (dev.alloc(REC * n_bins), dev.alloc(8 * ecap), dev.alloc(4 * ecap), dev.alloc(REC * ecap),
                                    dev.alloc(8))
    d_out, d_ooff, d_ost = dev.alloc(2 * ecap * 200), dev.alloc(8 * (ecap + 1)), dev.alloc(4 * ecap)
    assert ctx.fir_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_l, n_bins, None, dev.d_seg, SB,
                              x3.Fir([1, 0, -1])) == 0
    assert ctx.events_dev(d_l, n_bins, bin_len, dev.d_so + 8 * dev.F, rule, d_es, d_el, d_ev, ecap, d_cnt) == 0
    assert raw() == 0
    assert ctx.decode_ranges_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_es, d_el, ecap, 200, d_out, ecap * 200, 0,
                                 d_ooff, d_ost, dev.d_seg, SB) == 0
    assert ctx.decode_ranges_result()[:2] == (0, 0)
    assert ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    assert ctx.events_result()[0] == 0
    assert ctx.levels_result() == (0, 1, 2, CRC)
    want = FR.range_levels(dev.frames(), dev.so, [0, 400, 800, 1200], [400] * 4, 100, 0, cap, (1, 0, -1))
    T.same(ctx.download(d["lv"], REC * cap).reshape(cap, REC), want[0])
    assert FR.view(want[0][:16])["n"].tolist() == [98] + [100] * 7 + [0] * 4 + [98] + [100] * 3     # frame 2 and two positions behind it
    for r in (ctx.decode_ranges_result, ctx.range_levels_result, ctx.events_result, ctx.levels_result):
        assert r()[0] == BAD                                                 # nothing is pending any more
    # the three forms share the slot: the second call's summary replaces the first's
    assert dev.call(d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"]) == 0 and raw(nr=2) == 0
    assert ctx.range_levels_result() == (0, 0, 2, 0, 8) and ctx.range_levels_result()[0] == BAD
    assert corpus.fir_range_levels_into(**cok) == 0 and ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ what it is for

def test_the_burst_found_behind_the_filter_is_looked_at_again_behind_the_filter(ctx, x3):
    """test_gpu_fir_levels.py's burst -- a tone of amplitude 12 000 and period 2 000 with a burst of amplitude 600 at fs/4 on
    [4 300, 4 400) -- closed into a loop: events(signal=Fir([1, 0, -1])) -> fir_range_levels(bin_len=10) on the returned
    tensors as they are.  The fillers give one identity row and status 0, the burst's ten records are the definition's"""
    import torch
    i = np.arange(8_000)
    w = np.round(12_000 * np.sin(2 * np.pi * i / 2_000)).astype(np.int64)
    w[4_300:4_400] += np.round(600 * np.cos(np.pi * i[4_300:4_400] / 2)).astype(np.int64)
    w = w.astype(np.int16)
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    offs = RR.frame_offsets(stream)
    frames, so = RR.frames_of(stream, offs, op), S.R.sample_offsets([2_000] * 4)
    fir = x3.Fir([1, 0, -1])
    rule = x3.EventRule.make(mean_sq_min=100_000)
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        starts, lens, cnt, el = ws.events(100, rule, 4, signal=fir)
        assert int(cnt) == 1 and starts.tolist() == [4_300, 0, 0, 0] and lens.tolist() == [100, 0, 0, 0]
        lv, off, st = ws.fir_range_levels(starts, lens, 10, fir)
        assert isinstance(lv, torch.Tensor) and off.tolist() == [0, 10, 11, 12, 13] and st.tolist() == [0, 0, 0, 0]
        want = FR.range_levels(frames, so, [4_300, 0, 0, 0], [100, 0, 0, 0], 10, 0, 13, (1, 0, -1))
        T.same(lv.cpu().numpy(), want[0])
        rec = x3.event_levels_view(lv)
        y = w.astype(np.int64)[2:] - w.astype(np.int64)[:-2]                 # y[i] = x[i] - x[i - 2] at position i = index + 2
        assert np.array_equal(rec[10:], LR.empty(3)) and rec["n"][:10].tolist() == [10] * 10
        assert rec["sum_sq"][:10].tolist() == [int((y[4_298 + 10 * b:4_308 + 10 * b] ** 2).sum()) for b in range(10)]
        one, _, _ = ws.fir_range_levels(starts, lens, 0, fir)             # one bin a range: the events' own records
        assert torch.equal(one, el)
        with pytest.raises(ValueError, match="not built yet"):
            ws.range_levels(starts, lens, 10, signal=fir)
        with pytest.raises(ValueError):
            ws.fir_range_levels(starts, lens, 10, "diff")
    finally:
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], params=p, seg_blocks=8,
                       index="walk")
    try:
        ent, starts, lens, cnt, el = corpus.events(100, rule, 4, signal=fir)
        assert int(cnt) == 2 and ent.tolist() == [0, 1, 0, 0] and starts.tolist() == [4_300, 4_300, 0, 0]
        clv, off, st = corpus.fir_range_levels(ent, starts, lens, 10, fir)
        assert off.tolist() == [0, 10, 20, 21, 22] and not st.any()
        assert torch.equal(clv[:10], lv[:10]) and torch.equal(clv[10:20], lv[:10]) and torch.equal(clv[20:], lv[10:12])
        with pytest.raises(ValueError, match="not built yet"):
            corpus.range_levels(ent, starts, lens, 10, signal=fir)
    finally:
        corpus.close()
