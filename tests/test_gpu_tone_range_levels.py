"""Tone range levels (include/x3hip.h, "TONE RANGE LEVELS"): x3_tone_range_levels_dev, x3_corpus_tone_range_levels_dev and the
Python surface.  Every record, offset and status is compared with == against tone_range_levels_ref.py, the definition written
from the CPU oracle's decode (all fields are integers: no tolerance anywhere); every output array is filled with 0x5A first
and carries canary bytes behind its end (test_gpu_range_levels.py's run(), whose helpers these tests use, with the damaged
streams, the corpus and the range tables of test_gpu_fir_range_levels.py).

The base stream is that file's: 2 137 samples in frames of 400 (block length 20, seg_blocks 4: five stretches a frame, the
second from sample 81), five whole frames and one of 137.  What is under test beside the records themselves is THE PHASE: it
is the stream's or entry's, so every lane's seed (its first sample's position) and the fix-up's (the frame's sample 0) show
in re and im of every range that does not start at a multiple of the oscillator's period."""
import ctypes as C

import numpy as np
import pytest

import async_cases as AC
import levels_ref as LR
import oracle_lib as O
import range_levels_ref as R
import ranges_ref as RR
import seg_index_ref as SR
import test_gpu_fir_range_levels as TF
import test_gpu_range_levels as T
import tone_levels_ref as TL
import tone_range_levels_ref as TR

pytestmark = pytest.mark.gpu

BAD, CRC, N, SB, REC = T.BAD, T.CRC, T.N, T.SB, T.REC
STARTS = [0, 1, 80, 81, 82, 399, 400, 401, 800, 2136]     # first, last and neighbour samples of frames and stretches
BINS = [0, 1, 7, 20, 400, 401, 2 ** 32]
EXAMPLE_STEP = 350_898_828                                  # round(0.0817 * 2^32)
STEPS = [0, EXAMPLE_STEP, 2 ** 31, 2 ** 32 - 1, 2 ** 22]   # (2^22: a period of 1 024 positions)
ONES = np.tile(np.array([[1, 0]], dtype=np.int16), (1024, 1))


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _random_table(seed=11):
    return np.random.default_rng(seed).integers(-32768, 32768, (1024, 2)).astype(np.int16)


def _table(dev, tab):
    """the device pointer of a table: None is the context's usual one, an array is uploaded (and freed with dev)"""
    if tab is None:
        return dev.ctx.tone_table_dev()
    d = dev.alloc(4096)
    dev.ctx.upload(d, np.ascontiguousarray(tab, dtype=np.int16))
    return d


def call(dev, step, d_tab=None, seg=True, d_so=None):
    """the enqueue function of T.run: x3_tone_range_levels_dev on dev's stream (d_so: other sample offsets than its own)"""
    idx = dev.d_seg if seg else None

    def enqueue(d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status):
        tone = dev.x3.LevelTone(step, 0, d_tab or dev.ctx.tone_table_dev())
        rc = dev.ctx.tone_range_levels_dev(dev.d_x3, dev.len, dev.d_off, d_so or dev.d_so, dev.F, dev.p, d_starts, d_lens, n,
                                           bin_len, stride, d_levels, cap, d_off, d_status, idx, dev.sb if idx else 0, tone)
        tone.step, tone.d_table = 0xDEAD, 8                    # (the struct was copied at the call)
        return rc
    return enqueue


def same(got, want, what=""):
    """records (uint8 [rows, 32]) equal, byte for byte; the first rows that differ are named as tone records"""
    if not np.array_equal(got, want):
        rows = np.flatnonzero((got != want).any(axis=1))[:4]
        raise AssertionError("%s records %s: got %s, want %s" % (what, rows.tolist(), [TR.view(got[r:r + 1])[0] for r in rows],
                                                                  [TR.view(want[r:r + 1])[0] for r in rows]))


def compare(got, want, lens, bin_len, what=""):
    assert np.array_equal(got[2], want[2]), (what, np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
    assert np.array_equal(got[1], want[1])
    same(got[0], want[0], what)
    assert got[3] == T.rows_total(lens, bin_len)


def check(ctx, dev, frames, starts, lens, bin_len, stride, cap, step, tab=None, d_tab=None, seg=True, so=None, d_so=None, want=None):
    """one call against the reference; tab: the table's contents (None: the usual one), d_tab: where it lies on the device"""
    got = T.run(ctx, call(dev, step, d_tab, seg, d_so), starts, lens, bin_len, stride, cap)
    if want is None:
        want = TR.range_levels(frames, dev.so if so is None else so, starts, lens, bin_len, stride, cap, step, tab)
    compare(got, want, lens, bin_len, (step, bin_len, stride))
    return got


grid, layouts = TF.grid, TF.layouts


def both_layouts(ctx, dev, frames, starts, lens, bin_len, step, tab=None, d_tab=None, seg=True):
    out = None
    for stride, cap in reversed(layouts(lens, bin_len)):
        out = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, step, tab, d_tab, seg)
    return out                                                # (the packed one)


# ------------------------------------------------------------------------------------------------ starts, lengths, bins, layouts

@pytest.mark.parametrize("bin_len", BINS)
@pytest.mark.parametrize("step", STEPS)
def test_every_length_at_every_start_at_every_bin_length(ctx, x3, step, bin_len):
    """packed, and padded to a stride that refuses the longest ranges; the encoder's index, a walk-built one and none give the
    same bytes, the reference is computed once for the three"""
    starts, lens = grid(STARTS)
    wants = None
    for index in ("ref", "walk", None):
        dev = T.base(ctx, x3, index)
        assert dev.total == N and dev.F == 6
        frames = dev.frames()
        if wants is None:
            wants = [TR.range_levels(frames, dev.so, starts, lens, bin_len, stride, cap, step) for stride, cap in layouts(lens, bin_len)]
        for (stride, cap), want in zip(layouts(lens, bin_len), wants):
            check(ctx, dev, frames, starts, lens, bin_len, stride, cap, step, seg=index is not None, want=want)
            assert ctx.get_option("last_range_levels_replays") == 0 and ctx.get_option("last_range_levels_overflow") == 0
        dev.close()
    out, off, st = wants[0]
    assert (st == BAD).any() and (st == 0).any()
    if bin_len in (1, 7, 20):
        assert (wants[1][2] == BAD).sum() > (st == BAD).sum()          # the stride of 25 rows refuses the longest ranges
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # n counts samples: one per position, whatever the tone
        if st[w] == 0:
            assert int(TR.view(out[int(off[w]):int(off[w + 1])])["n"].sum()) == ln, (s0, ln)


@pytest.mark.parametrize("bl, bpf, codes", [(10, 40, (0, 1, 3)), (40, 10, (0, 1, 3)), (20, 20, (1, 1, 3))])
def test_block_lengths_and_code_sets(ctx, x3, bl, bpf, codes):
    for index in ("walk", None):
        dev = T.base(ctx, x3, index, bl, bpf, codes)
        assert dev.F == 6 and dev.so[1] == 400
        first = 1 + SB * bl                                   # the second stretch's first sample
        starts, lens = grid([0, 1, first - 1, first, first + 1, 399, 400, 400 + first, 401, 800, 2136], [0, 1, 21, 400, 401, N])
        for bin_len, step in ((0, EXAMPLE_STEP), (7, 2 ** 32 - 1), (400, 2 ** 22)):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, step, seg=index is not None)
            if not any(st for st, _ in dev.frames()):             # (with codes (1, 1, 3) frames fail to decode: the reader's)
                assert ctx.get_option("last_range_levels_replays") == 0
        dev.close()


def test_a_random_table(ctx, x3):
    """any contents are legal: 1 024 random int16 pairs, full scale among them"""
    tab = _random_table()
    tab[5], tab[1023] = (-32768, 32767), (32767, -32768)
    for index in ("ref", None):
        dev = T.base(ctx, x3, index)
        d_tab = _table(dev, tab)
        starts, lens = grid(STARTS)
        for bin_len, step in ((0, EXAMPLE_STEP), (7, 2 ** 32 - 1), (401, 2 ** 22), (1, 2 ** 31)):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, step, tab, d_tab, seg=index is not None)
        dev.close()


def test_two_ranges_over_identical_samples_differ_by_the_phase(ctx, x3):
    """a constant stream: equal lengths at different starts have equal min, max and n and other re and im -- the phase is
    the stream's; a start one period (1 024 positions at step 2^22) later gives the same record"""
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    rc, s, _ = O.encode(np.full(N, 1000, dtype=np.int16), op)
    assert rc == 0
    dev = T.Dev(ctx, x3, s, p, op, SR.build(s, RR.frame_offsets(s)[:-1], op, SB)[0])
    out, off, st, _ = check(ctx, dev, dev.frames(), [0, 333, 1024, 333 + 1024, 81], [200] * 5, 0, 0, 5, 2 ** 22)
    rec = TR.view(out)
    assert not st.any() and rec["n"].tolist() == [200] * 5 and rec["min"].tolist() == rec["max"].tolist() == [1000] * 5
    assert rec[0] == rec[2] and rec[1] == rec[3] and rec["re"][0] != rec["re"][1] and rec["im"][0] != rec["im"][1]
    assert len({(int(r["re"]), int(r["im"])) for r in rec}) == 3
    dev.close()


# ------------------------------------------------------------------------------------------------ against existing GPU paths

def _tone_levels(dev, bin_len, n_bins, step, d_tab=None):
    d_lv, d_st = dev.alloc(REC * n_bins), dev.alloc(4 * dev.F)
    tone = dev.x3.LevelTone(step, 0, d_tab or dev.ctx.tone_table_dev())
    assert dev.ctx.tone_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, dev.d_seg,
                                   dev.sb, tone) == 0
    assert dev.ctx.levels_result()[0] == 0
    return dev.ctx.download(d_lv, REC * n_bins, TL.TONE_DTYPE), dev.ctx.download(d_st, 4 * dev.F, np.int32)


def _whole_stream(ctx, dev, status, steps=STEPS):
    for step in steps:
        for bin_len in BINS:
            n_bins = TR.rows_of(N, bin_len)
            lv, fst = _tone_levels(dev, bin_len, n_bins, step)
            out, off, st, total = T.run(ctx, call(dev, step), [0], [N], bin_len, 0, n_bins)
            assert total == n_bins and st.tolist() == [status]
            assert np.array_equal(TR.view(out), lv), (step, bin_len)
        # ... and bin-aligned ranges are slices of those records, the last one cut to the range's length
        lv, _ = _tone_levels(dev, 100, 22, step)
        starts, lens = [0, 400, 800, 300, 2000, 1900, 100], [400, 400, 1337, 250, 137, 200, 2037]
        out, off, st, _ = T.run(ctx, call(dev, step), starts, lens, 100, 0, T.rows_total(lens, 100))
        for w, (s0, ln) in enumerate(zip(starts, lens)):
            got = TR.view(out[int(off[w]):int(off[w + 1])])
            assert np.array_equal(got[:ln // 100], lv[s0 // 100:(s0 + ln) // 100]), (s0, ln)
            if s0 + ln == N:
                assert np.array_equal(got[-1], lv[-1])


@pytest.mark.parametrize("hurt", [None, 0, 2, 5])
def test_the_whole_stream_equals_x3_tone_levels_dev(ctx, x3, hurt):
    dev = T.base(ctx, x3) if hurt is None else TF._hurt(ctx, x3, hurt)
    _whole_stream(ctx, dev, 0 if hurt is None else CRC)
    assert ctx.get_option("last_range_levels_replays") == 0
    dev.close()


def test_the_whole_stream_with_a_late_decode_error_goes_through_the_reader(ctx, x3):
    """frame 2 fails late in its payload under a valid CRC: its stretches flag it and the fix-up replays it through the
    reader for its status; it adds nothing, and the frames either side of it keep their own phase.  (A frame the fix-up
    replays to status 0, where its phase seed -- the frame's sample 0 -- decides the sums, is the wrong index entry's and
    the forty ranges' below.)"""
    dev, rc2 = TF._late_error(ctx, x3)
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, rc2, 0, 0, 0] and rc2 not in (CRC, BAD)
    _whole_stream(ctx, dev, rc2, STEPS[1:4])
    assert ctx.get_option("last_range_levels_replays") > 0
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(TF.DAMAGE_RANGES[0]) + starts, list(TF.DAMAGE_RANGES[1]) + lens
    for bin_len, stride in ((7, 0), (400, 0), (0, 0), (100, 25)):
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len),
                                EXAMPLE_STEP)
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == rc2) == bool(covers), (s0, ln, st[w])
    dev.close()


@pytest.mark.parametrize("how", ["bit", "sample"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """frame 2, entry 2: a bit position one late, or a last sample with its lowest bit flipped.  The tone takes nothing from
    the index, but x3w_stretch's proof reads it: the frame is flagged, goes through the reader in the fix-up -- every range
    that covers it seeds the phase with the position of the frame's sample 0 and skips to its cut -- and the bytes are the
    same"""
    dev = T.base(ctx, x3)
    frames = dev.frames()
    nw = SR.n_words(6, dev.op, SB)
    good = ctx.download(dev.d_seg, 8 * nw, np.uint64)
    per = (nw - 1) // 6
    bad = good.copy()
    bad[1 + 2 * per + 1] = bad[1 + 2 * per + 1] + np.uint64(1) if how == "bit" else bad[1 + 2 * per + 1] ^ np.uint64(1 << 32)
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(TF.DAMAGE_RANGES[0]) + starts, list(TF.DAMAGE_RANGES[1]) + lens
    for (bin_len, stride), step in zip(((7, 0), (0, 0), (100, 25)), (EXAMPLE_STEP, 2 ** 32 - 1, 2 ** 22)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        ctx.upload(dev.d_seg, good)
        want = T.run(ctx, call(dev, step), starts, lens, bin_len, stride, cap)
        assert ctx.get_option("last_range_levels_replays") == 0
        ctx.upload(dev.d_seg, bad)
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, step)
        assert ctx.get_option("last_range_levels_replays") > 0
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    dev.close()


def test_a_table_of_ones_gives_the_bytes_of_x3_range_levels_dev(ctx, x3):
    """all (1, 0): re is the SAMPLES record's sum, im is 0, min, max, n, row offsets and statuses are its bytes, whatever
    the step; and step 0 with the usual table gives 32 767 times the sum"""
    dev = TF._hurt(ctx, x3, 2)
    d_ones = _table(dev, ONES)
    starts, lens = T.base_ranges(seed=7)
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 25)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len) - 5        # (packed: the last ranges have no room)
        old = T.run(ctx, dev.call, starts, lens, bin_len, stride, cap)
        plain = R.view(old[0])
        written = plain["reserved"] == 0                                    # (what no call may write keeps its 0x5A)
        assert written.any() and (old[2] == BAD).any()
        for step, d_tab, mul in [(s, d_ones, 1) for s in STEPS] + [(0, None, 32767)]:
            new = T.run(ctx, call(dev, step, d_tab), starts, lens, bin_len, stride, cap)
            assert np.array_equal(new[1], old[1]) and np.array_equal(new[2], old[2]) and new[3] == old[3]
            rec = TR.view(new[0])
            assert np.array_equal(new[0][~written], old[0][~written])
            assert np.array_equal(rec["re"][written], mul * plain["sum"][written]) and not rec["im"][written].any()
            for name in ("min", "max", "n", "reserved"):
                assert np.array_equal(rec[name], plain[name]), name
    dev.close()


@pytest.mark.parametrize("f", [0, 2, 5])
def test_a_payload_crc_failure_takes_the_frame_only(ctx, x3, f):
    dev = TF._hurt(ctx, x3, f)
    frames = dev.frames()
    a, b = int(dev.so[f]), int(dev.so[f + 1])
    starts, lens = T.base_ranges(seed=4)
    starts, lens = list(TF.DAMAGE_RANGES[0]) + starts, list(TF.DAMAGE_RANGES[1]) + lens
    for bin_len, stride in ((7, 0), (400, 0), (0, 0), (100, 25)):
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len),
                                EXAMPLE_STEP)
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # the status is the SAMPLES call's
        covers = ln and s0 < b and s0 + ln > a and s0 <= N and ln <= N - s0
        assert (st[w] == CRC) == bool(covers), (s0, ln, st[w])
    assert ctx.get_option("last_range_levels_replays") == 0
    one = check(ctx, dev, frames, [0], [N], 0, 0, 1, EXAMPLE_STEP)
    assert int(TR.view(one[0])["n"][0]) == N - (b - a)
    dev.close()


def test_sample_offsets_of_another_stream(ctx, x3):
    """frames of 300 by the caller's offsets: five frames fail their check with ERR_BAD_ARG; the last frame agrees and counts,
    at the phase of the positions the caller's offsets give it"""
    dev = T.base(ctx, x3)
    so = np.array([0, 300, 600, 900, 1200, 1500, 1637], dtype=np.uint64)
    d_so = dev.alloc(8 * so.size)
    ctx.upload(d_so, so)
    frames = dev.frames(so)
    assert [st for st, _ in frames] == [BAD] * 5 + [0]
    starts, lens = [0, 1200, 1500, 1501, 1400, 1637, 1500, 1638], [1637, 437, 137, 136, 200, 0, 138, 0]
    for bin_len, stride in ((0, 0), (7, 0), (100, 20)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, EXAMPLE_STEP, so=so, d_so=d_so)
        assert st.tolist() == [BAD, BAD, 0, 0, BAD, 0, BAD, BAD]
    dev.close()


# ------------------------------------------------------------------------------------------------ shared frames

@pytest.mark.parametrize("n", [2, 40])
def test_ranges_that_all_cover_all_six_frames(ctx, x3, n):
    """40 ranges over 6 frames are 240 pairs against P = min(40 * 6, 4 * (6 + 40)) = 184, the SAMPLES form's (no lead frames):
    the 56 pairs beyond go through the reader in the fix-up, seeded with their frame's sample 0, and the records are the same"""
    dev = T.base(ctx, x3)
    starts = [w % 3 for w in range(n)]
    lens = [N - 2 - (w % 5) for w in range(n)]
    over = max(0, n * 6 - 4 * (6 + n))
    assert over == (56 if n == 40 else 0)
    for bin_len, step in ((0, EXAMPLE_STEP), (7, 2 ** 32 - 1), (400, 2 ** 22)):
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), step)
        assert ctx.get_option("last_range_levels_overflow") == over and ctx.get_option("last_range_levels_replays") == over
    dev.close()


def test_more_ranges_than_threads_of_the_scans(ctx, x3):
    dev = T.base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 60, 3000).tolist()
    starts = (rng.integers(0, (N - 60) // 20, 3000) * 20 + rng.integers(0, 8, 3000)).tolist()   # many near frame and stretch starts
    check(ctx, dev, dev.frames(), starts, lens, 7, 0, T.rows_total(lens, 7), EXAMPLE_STEP)
    check(ctx, dev, dev.frames(), starts, lens, 0, 2, 6000, 2 ** 32 - 1)
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

@pytest.mark.parametrize("index", ["decode", "walk"])
def test_corpus_ranges_equal_the_stream_form_on_each_entry(ctx, x3, index):
    """entries of 1, 399, 2 137, 0, 1 000, 400 and 5 samples: none but the first begins at a multiple of any period in the
    corpus's own positions, so records equal to the stream form's on each entry alone prove phase 0 at every entry"""
    corpus, devs = TF._corpus(ctx, x3, index)
    ES = TF.ENTRY_SAMPLES
    ne = len(ES)
    tab = [(e, 0, n) for e, n in enumerate(ES)] + [(e, 0, 1) for e in range(ne)] + [(e, 0, 0) for e in range(ne + 1)]
    tab += [(2, 400, 400), (2, 800, 1337), (2, 81, 1000), (2, 401, 5), (2, 1, 3), (2, 82, 3), (4, 400, 400), (4, 800, 200), (4, 0, 400),
            (4, 399, 2), (4, 803, 9), (4, 0, 1000), (1, 398, 1), (1, 0, 8), (5, 399, 1), (5, 1, 399), (5, 0, 7), (6, 0, 5), (6, 4, 1),
            (ne, 0, 1), (2 ** 32 - 1, 0, 0), (3, 1, 0), (0, 1, 0), (1, 399, 1), (2, N, 1), (5, 2 ** 63, 1)]
    np.random.default_rng(2).shuffle(tab)
    ent, starts, lens = [t[0] for t in tab], [t[1] for t in tab], [t[2] for t in tab]
    seen = set()
    tone = x3.LevelTone(EXAMPLE_STEP, 0, ctx.tone_table_dev())
    for bin_len, stride in ((0, 0), (7, 0), (400, 0), (100, 22)):
        cap = len(tab) * stride or T.rows_total(lens, bin_len)
        out, off, st, total = T.run(ctx, lambda *a: corpus.tone_range_levels_into(*a, tone), starts, lens, bin_len, stride, cap,
                                    entries=ent)
        assert total == T.rows_total(lens, bin_len)
        for w, (e, s0, ln) in enumerate(tab):
            rows = stride or TR.rows_of(ln, bin_len)
            mine = out[int(off[w]):int(off[w]) + rows]
            if e >= ne or devs[e] is None:
                assert st[w] == BAD, (e, s0, ln)             # not in the corpus, or an entry without frames
                assert np.array_equal(TR.view(mine), TL.empty(rows)), (e, s0, ln)
                continue
            d = devs[e]
            want = TR.range_levels(d.frames(), d.so, [s0], [ln], bin_len, stride, rows, EXAMPLE_STEP)
            one = T.run(ctx, call(d, EXAMPLE_STEP, seg=False), [s0], [ln], bin_len, stride, rows)   # the stream form, on that entry alone
            assert st[w] == one[2][0] == want[2][0], (e, s0, ln, st[w])
            same(mine, one[0], (e, s0, ln))
            same(one[0], want[0], (e, s0, ln))
            seen.add(int(st[w]))
    assert seen == {0, BAD, CRC}
    assert ctx.get_option("last_range_levels_replays") == 0
    for d in devs:
        if d is not None:
            d.close()
    corpus.close()


# ------------------------------------------------------------------------------------------------ refusals, pending state

def test_refusals_and_pending_states(ctx, x3):
    L = x3.lib()
    dev = TF._hurt(ctx, x3, 2)
    n, cap = 4, 64
    sizes = {"lv": REC * cap, "off": 8 * (n + 1), "st": 4 * n}
    d = {k: dev.alloc(v) for k, v in sizes.items()}
    d_starts, d_lens = dev.alloc(8 * n), dev.alloc(4 * n)
    ctx.upload(d_starts, np.array([0, 400, 800, 1200], dtype=np.uint64))
    ctx.upload(d_lens, np.full(n, 400, dtype=np.uint32))
    for k, v in sizes.items():
        ctx.upload(d[k], np.full(v, 0x5A, dtype=np.uint8))
    d_tab = ctx.tone_table_dev()
    ok = x3.LevelTone(EXAMPLE_STEP, 0, d_tab)

    def raw(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=SB, starts=d_starts,
            lens=d_lens, nr=n, bl=100, stride=0, lv=d["lv"], rows=cap, off=d["off"], st=d["st"], tone=ok):
        return L.x3_tone_range_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, starts, lens, nr, bl, stride, lv,
                                          rows, off, st, C.byref(tone) if tone is not None else None)
    bad_tones = [None, x3.LevelTone(EXAMPLE_STEP, 0, None), x3.LevelTone(EXAMPLE_STEP, 0, d_tab + 2),
                 x3.LevelTone(EXAMPLE_STEP, 1, d_tab)]
    for tone in bad_tones:                                      # a NULL or invalid tone is refused first: whatever else is wrong
        assert raw(tone=tone) == BAD and raw(tone=tone, x=None, nr=0) == BAD
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert raw(tone=None, params=bad_p) == BAD and raw(params=bad_p) != 0
    for r in (dict(c=None), dict(nr=0), dict(nr=2 ** 31), dict(rows=0), dict(rows=2 ** 31), dict(starts=None), dict(lens=None),
              dict(lv=None), dict(st=None), dict(off=None), dict(starts=d_starts + 4), dict(lens=d_lens + 2), dict(lv=d["lv"] + 4),
              dict(off=d["off"] + 4), dict(st=d["st"] + 2), dict(sb=3), dict(sb=0), dict(stride=17), dict(stride=2 ** 63),
              dict(x=None), dict(fo=dev.d_off + 4), dict(so=dev.d_so + 4)):
        assert raw(**r) == BAD, r
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, bin_len=100, row_stride=0, d_levels=d["lv"], rows_cap=cap,
               d_row_offsets=d["off"], d_status=d["st"], tone=ok)
    for r in [dict(tone=t) for t in bad_tones] + [dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(rows_cap=0),
                                                  dict(d_starts=None), dict(d_levels=d["lv"] + 4), dict(d_row_offsets=None),
                                                  dict(row_stride=17)]:
        assert corpus.tone_range_levels_into(**dict(cok, **r)) == BAD, r
    assert L.x3_corpus_tone_range_levels_dev(ctx._h, None, d_ent, d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"],
                                             C.byref(ok)) == BAD
    ctx.graph_begin()
    try:
        assert raw() == BAD and corpus.tone_range_levels_into(**cok) == BAD      # a context that records a graph
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
    n_bins = TR.rows_of(N, bin_len)
    rule = x3.EventRule.make(peak_min=1, join_bins=0, pad_bins=0, max_bins=4)
    d_l, d_es, d_el, d_ev, d_cnt = (dev.alloc(REC * n_bins), dev.alloc(8 * ecap), dev.alloc(4 * ecap), dev.alloc(REC * ecap),
                                    dev.alloc(8))
    d_out, d_ooff, d_ost = dev.alloc(2 * ecap * 200), dev.alloc(8 * (ecap + 1)), dev.alloc(4 * ecap)
    assert ctx.tone_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_l, n_bins, None, dev.d_seg, SB,
                               ok) == 0
    assert ctx.tone_power_levels_dev(d_l, n_bins, d_l) == 0
    assert ctx.events_dev(d_l, n_bins, bin_len, dev.d_so + 8 * dev.F, rule, d_es, d_el, d_ev, ecap, d_cnt) == 0
    assert raw() == 0
    assert ctx.decode_ranges_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, d_es, d_el, ecap, 200, d_out, ecap * 200, 0,
                                 d_ooff, d_ost, dev.d_seg, SB) == 0
    assert ctx.decode_ranges_result()[0] == 0
    assert ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    assert ctx.events_result()[0] == 0
    assert ctx.levels_result() == (0, 1, 2, CRC)
    want = TR.range_levels(dev.frames(), dev.so, [0, 400, 800, 1200], [400] * 4, 100, 0, cap, EXAMPLE_STEP)
    same(ctx.download(d["lv"], REC * cap).reshape(cap, REC), want[0])
    assert TR.view(want[0][:16])["n"].tolist() == [100] * 8 + [0] * 4 + [100] * 4     # frame 2 and nothing else
    for r in (ctx.decode_ranges_result, ctx.range_levels_result, ctx.events_result, ctx.levels_result):
        assert r()[0] == BAD                                                 # nothing is pending any more
    # the forms share the slot: the second call's summary replaces the first's
    assert dev.call(d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"]) == 0 and raw(nr=2) == 0
    assert ctx.range_levels_result() == (0, 0, 2, 0, 8) and ctx.range_levels_result()[0] == BAD
    assert corpus.tone_range_levels_into(**cok) == 0 and ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ behind a stall

def test_one_call_behind_a_stalled_caller_stream(x3):
    """the context runs on the caller's stream, which is stalled (test_gpu_async_analysis.py's helper: torch.cuda._sleep,
    calibrated by async_cases.calibrate_sleep, proven by an event behind it that has not completed when the enqueue has
    returned).  At the call the device table and the device starts still hold a decoy -- their content is copied behind the
    stall -- and the host x3_level_tone is overwritten right after the call: the records are those of the table and starts
    as they are when the kernels run and of the struct as it was at the call"""
    import torch
    cycles_per_ms = AC.calibrate_sleep(torch)
    op, p = O.Params.make(20, 20), x3.Params.make(block_len=20, blocks_per_frame=20)
    rc, s, _ = O.encode(T.base_wav(x3), op)
    assert rc == 0
    offs = RR.frame_offsets(s)
    frames, F = RR.frames_of(s, offs, op), len(offs) - 1
    so = R.sample_offsets([len(w) for _, w in frames])
    words = SR.build(s, offs[:-1], op, SB)[0]
    starts, lens = [401, 0, 81, 799, 1200, 333], [700, N, 40, 3, 937, 0]
    tab = _random_table(21)
    n, bin_len = len(starts), 100
    cap = T.rows_total(lens, bin_len)
    want = TR.range_levels(frames, so, starts, lens, bin_len, 0, cap, EXAMPLE_STEP, tab)
    decoy = TR.range_levels(frames, so, [0] * n, lens, bin_len, 0, cap, 12345, ONES)
    assert not np.array_equal(want[0], decoy[0])
    S = torch.cuda.Stream()
    ctx = x3.Context(0, stream=S.cuda_stream)
    try:
        with torch.cuda.stream(S):
            def dev(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
            d_x3, d_off, d_seg = dev(s), dev(np.array(offs, dtype=np.uint64)), dev(words)
            d_so = torch.empty(8 * (F + 1), dtype=torch.uint8, device="cuda")
            src_tab, src_starts, d_lens = dev(tab), dev(np.array(starts, dtype=np.uint64)), dev(np.array(lens, dtype=np.uint32))
            decoy_tab, decoy_starts = dev(ONES), dev(np.zeros(n, dtype=np.uint64))
            d_tab, d_starts = torch.empty_like(src_tab), torch.empty_like(src_starts)
            outs = {"lv": torch.empty(REC * cap + 64, dtype=torch.uint8, device="cuda"),
                    "off": torch.empty(8 * (n + 1) + 64, dtype=torch.uint8, device="cuda"),
                    "st": torch.empty(4 * n + 64, dtype=torch.uint8, device="cuda")}
            assert ctx.sample_offsets_dev(d_x3.data_ptr(), s.size, d_off.data_ptr(), F, d_so.data_ptr()) == 0
            stall_ms = 0.0          # (the first pass warms the workspace up without a stall; it proves nothing)
            for attempt in range(5):
                for t in outs.values():
                    t.fill_(AC.CANARY)
                d_tab.copy_(decoy_tab)
                d_starts.copy_(decoy_starts)
                S.synchronize()
                tone, other = x3.LevelTone(EXAMPLE_STEP, 0, d_tab.data_ptr()), x3.LevelTone(12345, 0, decoy_tab.data_ptr())
                if stall_ms:
                    torch.cuda._sleep(int(stall_ms * cycles_per_ms))
                behind = torch.cuda.Event()
                behind.record(S)
                d_tab.copy_(src_tab, non_blocking=True)                      # the content arrives behind the stall
                d_starts.copy_(src_starts, non_blocking=True)
                assert ctx.tone_range_levels_dev(d_x3.data_ptr(), s.size, d_off.data_ptr(), d_so.data_ptr(), F, p, d_starts.data_ptr(),
                                                 d_lens.data_ptr(), n, bin_len, 0, outs["lv"].data_ptr(), cap, outs["off"].data_ptr(),
                                                 outs["st"].data_ptr(), d_seg.data_ptr(), SB, tone) == 0, ctx.last_error()
                C.memmove(C.byref(tone), C.byref(other), C.sizeof(tone))    # the host struct, overwritten right after the call
                proven = bool(stall_ms) and not behind.query()
                S.synchronize()
                if not stall_ms:
                    stall_ms = 5.0
                    continue
                if proven:
                    break
                stall_ms *= 2
            else:
                raise AssertionError("the stall was never proven: the event behind it had completed when the enqueue returned")
            assert tone.step == 12345                                        # (the overwrite took place)
            res = ctx.range_levels_result()
            assert res == (0, 0, n, 0, cap), res
            lv, off, st = (outs[k].cpu().numpy() for k in ("lv", "off", "st"))
            for a, size in ((lv, REC * cap), (off, 8 * (n + 1)), (st, 4 * n)):
                assert (a[size:] == AC.CANARY).all()
            same(lv[:REC * cap].reshape(cap, REC), want[0], "behind the stall")
            assert np.array_equal(off[:8 * (n + 1)].view(np.uint64), want[1]) and not st[:4 * n].any()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ what it is for

def test_the_burst_found_in_the_band_is_looked_at_again_in_the_band(ctx, x3):
    """test_gpu_tone_levels.py's example -- uniform noise of +-3 000 with a 200-sample tone of amplitude 1 000 at 0.0817 fs on
    [4 400, 4 600) -- closed into a loop: events(signal=tone) at bins of 200 finds (4 400, 200); tone_range_levels of the event
    with 200 positions either side, (4 200, 600), at bins of 100 with band=True gives six records of the band's level.  By
    tone_range_levels_ref.py and tone_levels_ref.tone_power_levels on the CPU the band mean squares (sum_sq / n) are
        34 091, 10 465, 435 861, 920 106, 40 515, 169 058:
    the two burst bins exceed every other bin, by 2.57 x at the least.  The bin length is 100 and not 50 for that reason: at
    50 the same definition gives 564 558, 503 712, 465 615 and 1 532 858 inside the burst against 422 618 at most outside, a
    margin of 1.10 x, where half a bin of noise decides (the figures quoted with the request for this call, 597 518 and
    872 189 inside at 100 and 220 929 inside at 50, are not this signal's: its outside figures 169 058 and 422 618 are).
    The GPU's records are held with == against the reference's, not against a threshold"""
    import torch
    import test_gpu_tone_levels as TT
    w = TT._example()
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [(0, w[a:a + 2_000]) for a in range(0, 20_000, 2_000)], R.sample_offsets([2_000] * 10)
    tone = x3.Tone(EXAMPLE_STEP)

    def band_ms(records):
        b = R.view(records)
        return (b["sum_sq"] // np.maximum(b["n"], 1)).astype(np.int64).tolist()
    want = TR.range_levels(frames, so, [4_200], [600], 100, 0, 6, EXAMPLE_STEP)
    want_band = TL.tone_power_levels(TR.view(want[0]))
    assert band_ms(want_band) == [34_091, 10_465, 435_861, 920_106, 40_515, 169_058]
    at50 = band_ms(TL.tone_power_levels(TR.one(frames, so, 4_200, 600, 50, EXAMPLE_STEP, TL.table())[0]))
    assert min(at50[4:8]) == 465_615 and max(at50[:4] + at50[8:]) == 422_618
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    try:
        starts, lens, cnt, el = ws.events(200, x3.EventRule.make(mean_sq_min=400_000), 4, signal=tone)
        assert int(cnt) == 1 and starts.tolist() == [4_400, 0, 0, 0] and lens.tolist() == [200, 0, 0, 0]
        zs, zl = starts[:1] - 200, lens[:1] + 400                                # the event with 200 positions either side
        lv, off, st = ws.tone_range_levels(zs, zl, 100, tone, band=True)
        assert isinstance(lv, torch.Tensor) and off.tolist() == [0, 6] and st.tolist() == [0]
        assert lv.cpu().numpy().tobytes() == want_band.tobytes()
        ms = band_ms(lv.cpu().numpy())
        assert min(ms[2:4]) > max(ms[:2] + ms[4:]) and 100 * min(ms[2:4]) >= 257 * max(ms[:2] + ms[4:])
        raw, off, st = ws.tone_range_levels(zs, zl, 100, tone)                   # the quadrature sums themselves
        same(raw.cpu().numpy(), want[0])
        # the events' own tensors go in as they are: the fillers give one identity row and status 0; at one bin a range the
        # band records are the events' own
        one, off, st = ws.tone_range_levels(starts, lens, 0, tone, band=True)
        assert off.tolist() == [0, 1, 2, 3, 4] and not st.any() and torch.equal(one, el)
        # padded to a stride that refuses the range: its rows are the identity after the adapter, not zeros
        none, off, st = ws.tone_range_levels(zs, zl, 100, tone, padded_to=4, band=True)
        assert st.tolist() == [BAD] and np.array_equal(R.view(none.cpu().numpy()), LR.empty(4))
        # packed without room: the call does not write the records, the wrapper's zeros become the identity too
        none, off, st = ws.tone_range_levels(zs, zl, 100, tone, capacity=4, band=True)
        assert st.tolist() == [BAD] and np.array_equal(R.view(none.cpu().numpy()), LR.empty(4))
        with pytest.raises(ValueError, match="not built yet on this keyword: call tone_range_levels"):
            ws.range_levels(starts, lens, 100, signal=tone)
        with pytest.raises(ValueError):
            ws.tone_range_levels(starts, lens, 100, "tone")
    finally:
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], params=p, seg_blocks=8,
                       index="walk")
    try:
        ent, starts, lens, cnt, el = corpus.events(200, x3.EventRule.make(mean_sq_min=400_000), 4, signal=tone)
        assert int(cnt) == 2 and ent.tolist() == [0, 1, 0, 0] and starts.tolist() == [4_400, 4_400, 0, 0]
        clv, off, st = corpus.tone_range_levels(ent[:2], starts[:2] - 200, lens[:2] + 400, 100, tone, band=True)
        assert off.tolist() == [0, 6, 12] and not st.any()                   # the phase is 0 at each entry: the same records twice
        assert torch.equal(clv[:6], lv) and torch.equal(clv[6:], lv)
        craw, off, st = corpus.tone_range_levels(ent[:2], starts[:2] - 200, lens[:2] + 400, 100, tone)
        assert torch.equal(craw[:6], raw) and torch.equal(craw[6:], raw)
        with pytest.raises(ValueError, match="not built yet"):
            corpus.range_levels(ent, starts, lens, 100, signal=tone)
    finally:
        corpus.close()
