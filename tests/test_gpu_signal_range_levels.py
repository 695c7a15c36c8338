"""Signal range levels (include/x3hip.h, "SIGNAL RANGE LEVELS"): x3_signal_range_levels_dev, x3_corpus_signal_range_levels_dev
and the Python surface.  Every record, offset and status is compared with == against signal_range_levels_ref.py, the
definition written from the CPU oracle's decode (all five fields are integers: no tolerance anywhere); every output array is
filled with 0x5A first and carries canary bytes behind its end (test_gpu_range_levels.py's run(), whose helpers these tests
use).

The base stream is that file's: 2 137 samples in frames of 400 (block length 20, seg_blocks 4: five stretches a frame, the
second from sample 81), five whole frames and one of 137."""
import ctypes as C

import numpy as np
import pytest

import events_ref as E
import levels_ref as LR
import oracle_lib as O
import ranges_ref as RR
import seg_index_ref as SR
import signal_range_levels_ref as S
import test_gpu_range_levels as T
from x3_cases import refresh_crcs

pytestmark = pytest.mark.gpu

BAD, CRC, N, SB, REC = T.BAD, T.CRC, T.N, T.SB, T.REC
SAMPLES, DIFF = S.SAMPLES, S.DIFF
STARTS = [0, 1, 81, 399, 400, 401, 481, 799, 800, 2136]
BINS = [0, 1, 7, 20, 400, 401, 2 ** 32]


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def call(dev, signal=DIFF, seg=True, d_so=None):
    """the enqueue function of T.run: x3_signal_range_levels_dev on dev's stream (d_so: other sample offsets than its own)"""
    idx = dev.d_seg if seg else None

    def enqueue(d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status):
        return dev.ctx.signal_range_levels_dev(dev.d_x3, dev.len, dev.d_off, d_so or dev.d_so, dev.F, dev.p, d_starts, d_lens, n,
                                               bin_len, stride, d_levels, cap, d_off, d_status, idx, dev.sb if idx else 0, signal)
    return enqueue


def check(ctx, dev, frames, starts, lens, bin_len, stride, cap, seg=True, so=None, d_so=None):
    got = T.run(ctx, call(dev, DIFF, seg, d_so), starts, lens, bin_len, stride, cap)
    want = S.range_levels(frames, dev.so if so is None else so, starts, lens, bin_len, stride, cap)
    assert np.array_equal(got[2], want[2]), (np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
    assert np.array_equal(got[1], want[1])
    T.same(got[0], want[0], (bin_len, stride))
    assert got[3] == T.rows_total(lens, bin_len)
    return got


def grid(starts=STARTS, lens=T.LENS):
    """every length at every start (those off the end are ERR_BAD_ARG), in an order that is not sorted"""
    tab = [(s, ln) for s in starts for ln in lens]
    np.random.default_rng(5).shuffle(tab)
    return [s for s, _ in tab], [ln for _, ln in tab]


def both_layouts(ctx, dev, frames, starts, lens, bin_len, seg=True):
    """packed with room for all, padded to a stride that refuses the longest ranges"""
    out = check(ctx, dev, frames, starts, lens, bin_len, 0, T.rows_total(lens, bin_len), seg)
    most = max(S.rows_of(v, bin_len) for v in lens)
    stride = min(most, 25)
    check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride + 3, seg)
    return out


# ------------------------------------------------------------------------------------------------ starts, lengths, bins, layouts

@pytest.mark.parametrize("bin_len", BINS)
@pytest.mark.parametrize("index", ["ref", None, "walk"])
def test_every_length_at_every_start_at_every_bin_length(ctx, x3, index, bin_len):
    """starts at 0 (a frame start without a frame in front), 400 and 800 (the lead frame), 1 and 401 (seeded by the sample in
    front of the cut inside the frame), 81 and 481 (a stretch's first sample: seeded from the index), 399 / 799 / 2 136 (a
    frame's last sample)"""
    dev = T.base(ctx, x3, index)
    assert dev.total == N and dev.F == 6
    starts, lens = grid()
    frames = dev.frames()
    out, off, st, _ = both_layouts(ctx, dev, frames, starts, lens, bin_len, seg=index is not None)
    assert (st == BAD).any() and (st == 0).any()
    assert ctx.get_option("last_range_levels_replays") == 0 and ctx.get_option("last_range_levels_overflow") == 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # n counts differences: one per position, but for position 0
        if st[w] == 0:
            assert int(S.view(out[int(off[w]):int(off[w + 1])])["n"].sum()) == ln - (1 if s0 == 0 and ln else 0), (s0, ln)
    dev.close()


@pytest.mark.parametrize("bl, bpf, codes", [(10, 40, (0, 1, 3)), (40, 10, (0, 1, 3)), (20, 20, (1, 1, 3))])
def test_block_lengths_and_code_sets(ctx, x3, bl, bpf, codes):
    for index in ("walk", None):
        dev = T.base(ctx, x3, index, bl, bpf, codes)
        assert dev.F == 6 and dev.so[1] == 400
        first = 1 + SB * bl                                   # the second stretch's first sample
        starts, lens = grid([0, 1, first, 400, 400 + first, 401, 800, 2136], [0, 1, 21, 400, 401, N])
        for bin_len in (0, 7, 400):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, seg=index is not None)
            if not any(st for st, _ in dev.frames()):             # (with codes (1, 1, 3) frames fail to decode: the reader's)
                assert ctx.get_option("last_range_levels_replays") == 0
        dev.close()


def _one_sample_frames(values, op):
    parts = []
    for v in values:
        rc, s, _ = O.encode(np.array([v], dtype=np.int16), op)
        assert rc == 0
        parts.append(s)
    return np.concatenate(parts)


def test_frames_of_one_sample_and_a_stream_of_one_sample(ctx, x3):
    """every start is a frame's first sample: every range but those at 0 has a lead frame, every counted position is a seam"""
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    values = [5, -32768, 32767, 0, -7, 32767, -32768, 11, 12]
    dev = T.Dev(ctx, x3, _one_sample_frames(values, op), p, op, None)
    assert dev.F == 9 and dev.total == 9
    starts, lens = grid(list(range(10)), [0, 1, 2, 3, 9])
    for bin_len in (0, 1, 2, 4):
        out, off, st, _ = both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, seg=False)
    w = next(i for i, (s0, ln) in enumerate(zip(starts, lens)) if (s0, ln) == (1, 3))
    rec = S.view(out[int(off[w]):int(off[w + 1])])          # (bins of 4) -32768 - 5 and 32767 - -32768 clamp; 0 - 32767
    assert rec["n"].tolist() == [3] and rec["min"].tolist() == [-32768] and rec["max"].tolist() == [32767]
    dev.close()
    dev = T.Dev(ctx, x3, _one_sample_frames([-4321], op), p, op, None)
    for bin_len in (0, 1):
        out, off, st, _ = check(ctx, dev, dev.frames(), [0, 0, 1, 1], [1, 0, 0, 1], bin_len, 0, 4, seg=False)
        assert st.tolist() == [0, 0, 0, BAD] and np.array_equal(S.view(out), LR.empty(4))     # one sample: no difference
    dev.close()


# ------------------------------------------------------------------------------------------------ against existing GPU paths

def _signal_levels(dev, bin_len, n_bins, signal=DIFF):
    d_lv, d_st = dev.alloc(REC * n_bins), dev.alloc(4 * dev.F)
    assert dev.ctx.signal_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, dev.d_seg,
                                     dev.sb, signal) == 0
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
def test_the_whole_stream_equals_x3_signal_levels_dev(ctx, x3, hurt):
    dev = T.base(ctx, x3) if hurt is None else _hurt(ctx, x3, hurt)
    for bin_len in BINS:
        n_bins = S.rows_of(N, bin_len)
        lv, fst = _signal_levels(dev, bin_len, n_bins)
        out, off, st, total = T.run(ctx, call(dev), [0], [N], bin_len, 0, n_bins)
        assert total == n_bins and st.tolist() == [0 if hurt is None else CRC]
        assert np.array_equal(S.view(out), lv), bin_len
    if hurt is None:
        assert int(lv["n"].sum()) == N - 1
    # ... and bin-aligned ranges are slices of those records, the last one cut to the range's length
    lv, _ = _signal_levels(dev, 100, 22)
    starts, lens = [0, 400, 800, 300, 2000, 1900, 100], [400, 400, 1337, 250, 137, 200, 2037]
    out, off, st, _ = T.run(ctx, call(dev), starts, lens, 100, 0, T.rows_total(lens, 100))
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        got = S.view(out[int(off[w]):int(off[w + 1])])
        assert np.array_equal(got[:ln // 100], lv[s0 // 100:(s0 + ln) // 100]), (s0, ln)
        if s0 + ln == N:
            assert np.array_equal(got[-1], lv[-1])
    dev.close()


def test_samples_is_x3_range_levels_dev_byte_for_byte(ctx, x3):
    dev = _hurt(ctx, x3, 2)
    starts, lens = T.base_ranges(seed=7)
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 25)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len) - 5        # (packed: the last ranges have no room)
        new = T.run(ctx, call(dev, SAMPLES), starts, lens, bin_len, stride, cap)
        old = T.run(ctx, dev.call, starts, lens, bin_len, stride, cap)
        assert all(np.array_equal(a, b) for a, b in zip(new[:3], old[:3])) and new[3] == old[3]
        want = S.range_levels(dev.frames(), dev.so, starts, lens, bin_len, stride, cap, SAMPLES)
        T.same(new[0], want[0], "samples")
    dev.close()


# ------------------------------------------------------------------------------------------------ damage

DAMAGE_RANGES = ([0, 100, 799, 800, 900, 1199, 700, 0, 799, 1200, 1201, 1600, 1199, 400, 800, 1200, 1200, 81],
                 [800, 50, 1, 400, 100, 1, 600, N, 402, 400, 936, 537, 2, 400, 1, 1, 937, 1500])


def _damage_check(ctx, dev, frames):
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(DAMAGE_RANGES[0]) + starts, list(DAMAGE_RANGES[1]) + lens
    got = None
    for bin_len, stride in ((7, 0), (400, 0), (0, 0), (100, 25)):
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len))
    return starts, lens, got


@pytest.mark.parametrize("f", [0, 2, 5])
def test_a_payload_crc_failure_takes_the_frame_and_both_of_its_seams(ctx, x3, f):
    dev = _hurt(ctx, x3, f)
    frames = dev.frames()
    a, b = int(dev.so[f]), int(dev.so[f + 1])
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # the status is the SAMPLES call's: covering frames only
        covers = ln and s0 < b and s0 + ln > a and s0 <= N and ln <= N - s0
        assert (st[w] == CRC) == bool(covers), (s0, ln, st[w])
    assert ctx.get_option("last_range_levels_replays") == 0
    # the whole stream in one bin: the frame's positions and the seam behind it are missing, and the one in front
    one = T.run(ctx, call(dev), [0], [N], 0, 0, 1)
    lost = (b - a) + (1 if b < N else 0) - (1 if a == 0 else 0)
    assert int(S.view(one[0])["n"][0]) == N - 1 - lost
    dev.close()


def test_a_damaged_lead_frame_costs_the_seam_and_not_the_status(ctx, x3):
    dev = _hurt(ctx, x3, 0)
    clean = T.base(ctx, x3)
    starts, lens = [400, 400, 0, 401, 400], [400, 1, 400, 399, 0]
    out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, 0, 0, 5)
    assert st.tolist() == [0, 0, CRC, 0, 0] and S.view(out)["n"].tolist() == [399, 0, 0, 399, 0]
    ref, _, rst, _ = check(ctx, clean, clean.frames(), starts, lens, 0, 0, 5)
    assert not rst.any() and S.view(ref)["n"].tolist() == [400, 1, 399, 399, 0]
    assert np.array_equal(out[3], ref[3])                      # (401, 399) never looks at frame 0
    dev.close()
    clean.close()


def test_a_late_decode_error_goes_through_the_reader_and_the_fixup_takes_the_seams(ctx, x3):
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
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, rc2, 0, 0, 0] and rc2 not in (CRC, BAD)
    starts, lens, (out, off, st, _) = _damage_check(ctx, dev, frames)
    assert ctx.get_option("last_range_levels_replays") > 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == rc2) == bool(covers), (s0, ln, st[w])
    out, off, st, _ = check(ctx, dev, frames, [1200, 0], [400, N], 0, 0, 2)     # frame 2 as a lead frame that fails late
    assert st.tolist() == [0, rc2] and S.view(out)["n"].tolist() == [399, N - 1 - 400 - 1]
    assert ctx.get_option("last_range_levels_replays") == 2
    clean.close()
    dev.close()


@pytest.mark.parametrize("how", ["bit", "sample"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """frame 2, entry 2: a bit position one late, or a last sample with its lowest bit flipped -- the seed of the stretch
    behind it; the stretch in front contradicts the entry, the frame goes through the reader, the bytes are the same"""
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
        want = T.run(ctx, call(dev), starts, lens, bin_len, stride, cap)
        assert ctx.get_option("last_range_levels_replays") == 0
        ctx.upload(dev.d_seg, bad)
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, cap)
        assert ctx.get_option("last_range_levels_replays") > 0
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    dev.close()


def test_sample_offsets_of_another_stream(ctx, x3):
    """frames of 300 by the caller's offsets: five frames fail their check with ERR_BAD_ARG, a status a range off the end has
    too; the last frame agrees and counts, without the seam in front of it"""
    dev = T.base(ctx, x3)
    so = np.array([0, 300, 600, 900, 1200, 1500, 1637], dtype=np.uint64)
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    frames = dev.frames(so)
    assert [st for st, _ in frames] == [BAD] * 5 + [0]
    starts, lens = [0, 1200, 1500, 1501, 1400, 1637, 1500, 1638], [1637, 437, 137, 136, 200, 0, 138, 0]
    for bin_len, stride in ((0, 0), (7, 0), (100, 20)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, so=so, d_so=d_so)
        assert st.tolist() == [BAD, BAD, 0, 0, BAD, 0, BAD, BAD]
    one = check(ctx, dev, frames, starts, lens, 0, 0, len(starts), so=so, d_so=d_so)[0]
    assert S.view(one)["n"].tolist() == [136, 136, 136, 136, 99, 0, 0, 0]      # frame 5 less its first position, where covered
    dev.close()


# ------------------------------------------------------------------------------------------------ shared frames

@pytest.mark.parametrize("n, overflow", [(2, 0), (40, 16)])
def test_ranges_that_all_cover_all_six_frames(ctx, x3, n, overflow):
    """40 ranges over 6 frames are 240 pairs against P = min(40 * 6, 4 * (6 + 40) + 40) = 224: the pairs beyond go through the
    reader, their seams and those next to them are the fix-up's, and the records are the same"""
    dev = T.base(ctx, x3)
    starts = [w % 3 for w in range(n)]
    lens = [N - 2 - (w % 5) for w in range(n)]
    for bin_len in (0, 7, 400):
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len))
        assert ctx.get_option("last_range_levels_overflow") == overflow
        assert ctx.get_option("last_range_levels_replays") == overflow
    dev.close()


def test_lead_frames_beyond_the_pairs_the_workspace_holds(ctx, x3):
    """60 ranges (400, 1737): a lead frame and five covering frames each, 360 pairs against P = min(360, 4 * 66 + 60) = 324"""
    dev = T.base(ctx, x3)
    starts, lens = [400] * 60, [1737 - (w % 4) for w in range(60)]
    for bin_len in (0, 400):
        out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len))
        assert ctx.get_option("last_range_levels_overflow") == 36 and ctx.get_option("last_range_levels_replays") == 36
        assert not st.any()
    dev.close()


def test_two_ranges_share_a_frame_that_is_the_lead_frame_of_one_only(ctx, x3):
    for dev, want_st in ((T.base(ctx, x3), [0, 0, 0, 0]), (_hurt(ctx, x3, 0), [0, CRC, CRC, 0])):
        starts, lens = [400, 0, 100, 400], [400, 400, 500, 401]
        for bin_len in (0, 100):
            out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len))
            assert st.tolist() == want_st
        dev.close()


def test_more_ranges_than_threads_of_the_scans(ctx, x3):
    dev = T.base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 60, 3000).tolist()
    starts = (rng.integers(0, (N - 60) // 20, 3000) * 20 + rng.integers(0, 2, 3000)).tolist()   # many at frame and stretch starts
    check(ctx, dev, dev.frames(), starts, lens, 7, 0, T.rows_total(lens, 7))
    check(ctx, dev, dev.frames(), starts, lens, 0, 2, 6000)
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

ENTRY_SAMPLES = (1, 399, N, 0, 1000, 400)


def _corpus(ctx, x3, index):
    """a one-sample, a one-frame, a six-frame, an empty entry, one with a payload-CRC failure in its frame 1, one more frame"""
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
    tab = [(e, 0, n) for e, n in enumerate(ENTRY_SAMPLES)] + [(e, 0, 1) for e in range(6)] + [(e, 0, 0) for e in range(7)]
    tab += [(2, 400, 400), (2, 800, 1337), (2, 81, 1000), (2, 401, 5), (4, 400, 400), (4, 800, 200), (4, 0, 400), (4, 399, 2),
            (4, 0, 1000), (1, 398, 1), (5, 399, 1), (5, 1, 399), (6, 0, 1), (2 ** 32 - 1, 0, 0), (3, 1, 0), (0, 1, 0), (1, 399, 1), (2, N, 1),
            (5, 2 ** 63, 1)]
    np.random.default_rng(2).shuffle(tab)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    seen = set()
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 22)):
        cap = len(tab) * stride or T.rows_total(lens, bin_len)
        out, off, st, total = T.run(ctx, lambda *a: corpus.range_levels_into(*a, signal=DIFF), starts, lens, bin_len, stride, cap,
                                    entries=ent)
        assert total == T.rows_total(lens, bin_len)
        for w, (e, s0, ln) in enumerate(tab):
            rows = stride or S.rows_of(ln, bin_len)
            mine = out[int(off[w]):int(off[w]) + rows]
            if e >= 6 or devs[e] is None:
                assert st[w] == BAD, (e, s0, ln)             # not in the corpus, or an entry without frames
                assert np.array_equal(S.view(mine), LR.empty(rows)), (e, s0, ln)
                continue
            d = devs[e]
            want = S.range_levels(d.frames(), d.so, [s0], [ln], bin_len, stride, rows)
            one = T.run(ctx, call(d, DIFF, seg=False), [s0], [ln], bin_len, stride, rows)     # the stream form, on that entry alone
            assert st[w] == one[2][0] == want[2][0], (e, s0, ln, st[w])
            T.same(mine, one[0], (e, s0, ln))
            T.same(one[0], want[0], (e, s0, ln))
            seen.add(int(st[w]))
            if s0 == 0 and ln == ENTRY_SAMPLES[e] and e != 4:      # position 0 has no seam into the entry in front of it
                assert int(S.view(mine)["n"].sum()) == ln - 1
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

    def raw(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=SB, starts=d_starts,
            lens=d_lens, nr=n, bl=100, stride=0, lv=d["lv"], rows=cap, off=d["off"], st=d["st"], sig=DIFF):
        return L.x3_signal_range_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, starts, lens, nr, bl, stride, lv,
                                            rows, off, st, sig)
    for sig in (2, -1, 1 << 16):                                # an unknown signal is refused first: whatever else is wrong
        assert raw(sig=sig) == BAD and raw(sig=sig, x=None, nr=0) == BAD
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert raw(sig=2, params=bad_p) == BAD and raw(params=bad_p) != 0
    for r in (dict(c=None), dict(nr=0), dict(nr=2 ** 31), dict(rows=0), dict(rows=2 ** 31), dict(starts=None), dict(lens=None),
              dict(lv=None), dict(st=None), dict(off=None), dict(starts=d_starts + 4), dict(lens=d_lens + 2), dict(lv=d["lv"] + 4),
              dict(off=d["off"] + 4), dict(st=d["st"] + 2), dict(sb=3), dict(sb=0), dict(stride=17), dict(stride=2 ** 63),
              dict(x=None), dict(fo=dev.d_off + 4), dict(so=dev.d_so + 4)):
        for sig in (SAMPLES, DIFF):
            assert raw(**dict(dict(sig=sig), **r)) == BAD, r
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, bin_len=100, row_stride=0, d_levels=d["lv"], rows_cap=cap,
               d_row_offsets=d["off"], d_status=d["st"], signal=DIFF)
    for r in (dict(signal=2), dict(signal=-1), dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(rows_cap=0),
              dict(d_starts=None), dict(d_levels=d["lv"] + 4), dict(d_row_offsets=None), dict(row_stride=17)):
        assert corpus.range_levels_into(**dict(cok, **r)) == BAD, r
    assert L.x3_corpus_signal_range_levels_dev(ctx._h, None, d_ent, d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"],
                                               DIFF) == BAD
    ctx.graph_begin()
    try:
        assert raw() == BAD and corpus.range_levels_into(**cok) == BAD      # a context that records a graph
    finally:
        try:
            ctx.graph_destroy(ctx.graph_end())
        except x3.X3Error:
            pass                                                             # (a recording of nothing)
    assert ctx.range_levels_result()[0] == BAD                               # nothing is pending
    ctx.sync()
    for k, v in sizes.items():
        assert (ctx.download(d[k], v) == 0x5A).all(), k                      # ... and nothing was enqueued
    # beside the levels, events and ranges calls: four pending slots, each result call answers its own
    bin_len, ecap = 50, 16
    n_bins = S.rows_of(N, bin_len)
    rule = x3.EventRule.make(peak_min=1, join_bins=0, pad_bins=0, max_bins=4)
    d_l, d_es, d_el, d_ev, d_cnt = (dev.alloc(REC * n_bins), dev.alloc(8 * ecap), dev.alloc(4 * ecap), dev.alloc(REC * ecap),
                                    dev.alloc(8))
    d_out, d_ooff, d_ost = dev.alloc(2 * ecap * 200), dev.alloc(8 * (ecap + 1)), dev.alloc(4 * ecap)
    assert ctx.signal_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_l, n_bins, None, dev.d_seg, SB,
                                 DIFF) == 0
    assert ctx.events_dev(d_l, n_bins, bin_len, dev.d_so + 8 * dev.F, rule, d_es, d_el, d_ev, ecap, d_cnt) == 0
    assert raw() == 0
    assert ctx.decode_ranges_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_es, d_el, ecap, 200, d_out, ecap * 200, 0,
                                 d_ooff, d_ost, dev.d_seg, SB) == 0
    assert ctx.decode_ranges_result()[:2] == (0, 0)
    assert ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    assert ctx.events_result()[0] == 0
    assert ctx.levels_result() == (0, 1, 2, CRC)
    want = S.range_levels(dev.frames(), dev.so, [0, 400, 800, 1200], [400] * 4, 100, 0, cap)
    T.same(ctx.download(d["lv"], REC * cap).reshape(cap, REC), want[0])
    assert S.view(want[0][:16])["n"].tolist() == [99] + [100] * 7 + [0] * 4 + [99] + [100] * 3     # frame 2 and both its seams
    for r in (ctx.decode_ranges_result, ctx.range_levels_result, ctx.events_result, ctx.levels_result):
        assert r()[0] == BAD                                                 # nothing is pending any more
    # the SAMPLES and the DIFF form share the slot: the second call's summary replaces the first's
    assert raw(sig=SAMPLES) == 0 and raw(sig=DIFF, nr=2) == 0
    assert ctx.range_levels_result() == (0, 0, 2, 0, 8) and ctx.range_levels_result()[0] == BAD
    assert corpus.range_levels_into(**cok) == 0 and ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ what it is for

def test_the_burst_found_on_the_difference_is_looked_at_again_on_the_difference(ctx, x3):
    """test_gpu_signal_levels.py's burst -- a tone of amplitude 12 000 and period 2 000 with +-600 alternating on [4 300,
    4 400) -- closed into a loop: events(signal="diff") -> range_levels(bin_len=10, signal="diff") on the returned tensors as
    they are.  The fillers give one identity row and status 0, the burst's ten records are the definition's"""
    import torch
    i = np.arange(8_000)
    w = np.round(12_000 * np.sin(2 * np.pi * i / 2_000)).astype(np.int64)
    w[4_300:4_400] += 600 * (-1) ** i[4_300:4_400]
    w = w.astype(np.int16)
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    offs = RR.frame_offsets(stream)
    frames, so = RR.frames_of(stream, offs, op), S.R.sample_offsets([2_000] * 4)
    d = np.clip(np.diff(w.astype(np.int64)), -32768, 32767)
    rule = x3.EventRule.make(mean_sq_min=100_000)
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        starts, lens, cnt, el = ws.events(100, rule, 4, signal="diff")
        assert int(cnt) == 1 and starts.tolist() == [4_300, 0, 0, 0] and lens.tolist() == [100, 0, 0, 0]
        lv, off, st = ws.range_levels(starts, lens, 10, signal="diff")
        assert isinstance(lv, torch.Tensor) and off.tolist() == [0, 10, 11, 12, 13] and st.tolist() == [0, 0, 0, 0]
        want = S.range_levels(frames, so, [4_300, 0, 0, 0], [100, 0, 0, 0], 10, 0, 13)
        T.same(lv.cpu().numpy(), want[0])
        rec = x3.event_levels_view(lv)
        assert np.array_equal(rec[10:], LR.empty(3)) and rec["n"][:10].tolist() == [10] * 10
        assert rec["sum_sq"][:10].tolist() == [int((d[4_299 + 10 * b:4_309 + 10 * b] ** 2).sum()) for b in range(10)]
        assert E.merge(rec[:10]) == x3.event_levels_view(el)[0]                  # ... and together they are the event's record
        one, _, _ = ws.range_levels(starts, lens, 0, signal="diff")
        assert torch.equal(one, el)
        same, _, _ = ws.range_levels(starts, lens, 10, signal="samples")
        old, _, _ = ws.range_levels(starts, lens, 10)
        assert torch.equal(same, old) and not torch.equal(same, lv)
        with pytest.raises(ValueError):
            ws.range_levels(starts, lens, 10, signal="second")
    finally:
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], params=p, seg_blocks=8,
                       index="walk")
    try:
        ent, starts, lens, cnt, el = corpus.events(100, rule, 4, signal="diff")
        assert int(cnt) == 2 and ent.tolist() == [0, 1, 0, 0] and starts.tolist() == [4_300, 4_300, 0, 0]
        clv, off, st = corpus.range_levels(ent, starts, lens, 10, signal="diff")
        assert off.tolist() == [0, 10, 20, 21, 22] and not st.any()
        assert torch.equal(clv[:10], lv[:10]) and torch.equal(clv[10:20], lv[:10]) and torch.equal(clv[20:], lv[10:12])
        with pytest.raises(ValueError):
            corpus.range_levels(ent, starts, lens, 10, signal=2)
    finally:
        corpus.close()
