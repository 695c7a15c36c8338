"""Tone bank range levels (include/x3hip.h, "TONE BANK RANGE LEVELS"): x3_tone_bank_range_levels_dev,
x3_corpus_tone_bank_range_levels_dev and the Python surface.  ONE RULE: the bank is n_tones tone-range calls laid plane by
plane with plane stride rows_cap.  Every plane is compared with == against tone_bank_range_levels_ref.py (the definition) and
against the bytes x3_tone_range_levels_dev writes for that step; offsets, statuses, the result and the two counters
(last_range_levels_replays / _overflow) against the single call's.  All fields are integers: no tolerance anywhere.  Every
output array is filled with 0x5A first and carries canary bytes behind its end -- the records' canary lies behind the LAST
plane, and what no call may write must keep its 0x5A in every plane.

The base stream, the damaged streams, the corpus and the range tables are those of test_gpu_range_levels.py,
test_gpu_fir_range_levels.py and test_gpu_tone_range_levels.py: 2 137 samples in frames of 400 (block length 20, seg_blocks 4),
five whole frames and one of 137.  Banks are the first K steps of POOL: K = 2 runs the accumulate instance of two slots, 3 and
4 that of four (3: a spare slot), 5 and 8 that of eight (5: three spare slots), 1 the single call's kernels."""
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
import test_gpu_tone_range_levels as TT
import test_tone_bank_range_levels_ref as EX
import tone_bank_levels_ref as B
import tone_bank_range_levels_ref as BR
import tone_levels_ref as TL
import tone_range_levels_ref as TR

pytestmark = pytest.mark.gpu

BAD, CRC, N, SB, REC = T.BAD, T.CRC, T.N, T.SB, T.REC
STARTS, BINS, EXAMPLE_STEP, ONES = TT.STARTS, TT.BINS, TT.EXAMPLE_STEP, TT.ONES
ODD = 2_718_281_829
POOL = TT.STEPS + [ODD, 1, 2 ** 30, 12_345_678]      # [0, EXAMPLE_STEP, 2^31, 2^32 - 1, 2^22, ...]: nine, so POOL[1:9] is a bank
KS = [1, 2, 3, 4, 5, 8]
GUARD = T.GUARD


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def bank_of(x3, ctx, steps, d_tab=None, spare=0xDEADBEEF, **kw):
    """an x3_level_tone_bank of `steps` with `spare` in the slots behind them; kw: fields set to other values"""
    b = x3.LevelToneBank(len(steps), 0, d_tab or ctx.tone_table_dev(), (C.c_uint32 * 8)(*(list(steps) + [spare] * (8 - len(steps)))))
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def call(dev, steps, d_tab=None, seg=True, d_so=None, spare=0xDEADBEEF):
    """the enqueue function of run(): x3_tone_bank_range_levels_dev on dev's stream; the spare steps hold garbage and the
    struct is overwritten right behind the call (it was copied at the call)"""
    idx = dev.d_seg if seg else None

    def enqueue(d_starts, d_lens, n, bin_len, stride, d_levels, cap, d_off, d_status):
        bank = bank_of(dev.x3, dev.ctx, steps, d_tab, spare)
        rc = dev.ctx.tone_bank_range_levels_dev(dev.d_x3, dev.len, dev.d_off, d_so or dev.d_so, dev.F, dev.p, d_starts, d_lens, n,
                                                bin_len, stride, d_levels, cap, d_off, d_status, idx, dev.sb if idx else 0, bank)
        C.memset(C.byref(bank), 0xEE, C.sizeof(bank))
        return rc
    return enqueue


def run(ctx, enqueue, k, starts, lens, bin_len, stride, cap, entries=None):
    """T.run for k planes -> (records uint8 [k, cap, 32], offsets, status, total rows); the result call and the canaries
    are checked"""
    starts = np.array([int(s) for s in starts], dtype=np.uint64)
    lens = np.array(lens, dtype=np.uint32)
    n = starts.size
    sizes = (REC * k * cap, 8 * (n + 1), 4 * n)
    bufs = [ctx.alloc(max(s + GUARD, 8)) for s in sizes] + [ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)]
    d_lv, d_off, d_status, d_starts, d_lens, d_ent = bufs
    try:
        for q, s in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(s + GUARD, 0x5A, dtype=np.uint8))
        ctx.upload(d_starts, starts)
        ctx.upload(d_lens, lens)
        args = (d_starts, d_lens, n, bin_len, stride, d_lv, cap, d_off, d_status)
        if entries is not None:
            ctx.upload(d_ent, np.array(entries, dtype=np.uint32))
            args = (d_ent,) + args
        rc = enqueue(*args)
        assert rc == 0, ctx.last_error()
        res = ctx.range_levels_result()
        raw = [ctx.download(q, s + GUARD) for q, s in zip(bufs[:3], sizes)]
    finally:
        for q in bufs:
            ctx.free(q)
    for name, a, s in zip(("d_levels", "d_row_offsets", "d_status"), raw, sizes):
        assert (a[s:] == 0x5A).all(), "the canary behind %s is damaged" % name
    out = raw[0][:sizes[0]].reshape(k, cap, REC)
    off, st = raw[1][:sizes[1]].view(np.uint64), raw[2][:sizes[2]].view(np.int32)
    bad = np.nonzero(st)[0]
    assert res[:4] == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0), res
    return out, off, st, res[4]


def counters(ctx):
    return ctx.get_option("last_range_levels_replays"), ctx.get_option("last_range_levels_overflow")


_WANTS = {}


def single_want(key, frames, so, starts, lens, bin_len, stride, cap, step, tab=None):
    """the definition of one plane, computed once per (key: the stream and the ranges by name, call, step)"""
    k = (key, bin_len, stride, cap, step)
    if key is None or k not in _WANTS:
        w = TR.range_levels(frames, so, starts, lens, bin_len, stride, cap, step, tab)
        if key is None:
            return w
        for a in w:
            a.setflags(write=False)
        _WANTS[k] = w
    return _WANTS[k]


def check(ctx, dev, frames, starts, lens, bin_len, stride, cap, steps, tab=None, d_tab=None, seg=True, so=None, d_so=None, key=None,
          singles=True):
    """one bank call: every plane == the definition and == the single call's bytes (one call per distinct step); offsets,
    statuses, total and both counters are the single call's"""
    k = len(steps)
    assert 1 <= k <= 8
    got = run(ctx, call(dev, steps, d_tab, seg, d_so), k, starts, lens, bin_len, stride, cap)
    mine = counters(ctx)
    assert got[0].shape == (k, cap, REC) and got[3] == T.rows_total(lens, bin_len)
    seen = {}
    for t, step in enumerate(steps):
        want = single_want(key, frames, dev.so if so is None else so, starts, lens, bin_len, stride, cap, step, tab)
        assert np.array_equal(got[2], want[2]), (t, np.flatnonzero(got[2] != want[2])[:8], got[2][:16], want[2][:16])
        assert np.array_equal(got[1], want[1])
        TT.same(got[0][t], want[0], ("plane", t, step, bin_len, stride))
        if singles and step not in seen:
            one = T.run(ctx, TT.call(dev, step, d_tab, seg, d_so), starts, lens, bin_len, stride, cap)
            assert counters(ctx) == mine, (counters(ctx), mine)
            assert np.array_equal(one[1], got[1]) and np.array_equal(one[2], got[2]) and one[3] == got[3]
            seen[step] = one[0]
        if singles:
            assert got[0][t].tobytes() == seen[step].tobytes(), ("plane is not the single call's bytes", t, step)
    return got


def both_layouts(ctx, dev, frames, starts, lens, bin_len, steps, tab=None, d_tab=None, seg=True):
    out = None
    for stride, cap in reversed(TF.layouts(lens, bin_len)):
        out = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, steps, tab, d_tab, seg)
    return out                                                # (the packed one)


def damage_ranges():
    starts, lens = T.base_ranges(seed=4)
    return list(TF.DAMAGE_RANGES[0]) + starts, list(TF.DAMAGE_RANGES[1]) + lens


# ------------------------------------------------------------------------------------------------ starts, lengths, bins, layouts

@pytest.mark.parametrize("bin_len", BINS)
@pytest.mark.parametrize("k", KS)
def test_every_length_at_every_start_at_every_bin_length(ctx, x3, k, bin_len):
    """packed, and padded to a stride that refuses the longest ranges; the encoder's index, a walk-built one and none give the
    same bytes.  One tone IS the single call"""
    starts, lens = TF.grid(STARTS)
    steps = POOL[:k]
    for index in ("ref", "walk", None):
        dev = T.base(ctx, x3, index)
        assert dev.total == N and dev.F == 6
        for stride, cap in TF.layouts(lens, bin_len):
            out, off, st, _ = check(ctx, dev, dev.frames(), starts, lens, bin_len, stride, cap, steps, seg=index is not None,
                                    key="base-grid", singles=index != "walk")
            assert counters(ctx) == (0, 0)
        dev.close()
    assert (st == BAD).any() and (st == 0).any()


@pytest.mark.parametrize("k", [3, 5])
def test_spare_steps_and_an_overwritten_struct_change_nothing(ctx, x3, k):
    """steps[n_tones ..] are never read: garbage, zeros and a live step there give the same bytes in the same planes, and the
    plane count is n_tones' (the canary behind plane k - 1 holds)"""
    dev = T.base(ctx, x3)
    starts, lens = T.base_ranges(seed=7)
    steps = POOL[1:1 + k]
    cap = T.rows_total(lens, 7)
    outs = [run(ctx, call(dev, steps, spare=spare), k, starts, lens, 7, 0, cap) for spare in (0xDEADBEEF, 0, EXAMPLE_STEP, 2 ** 32 - 1)]
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o[:3], outs[0][:3]))
    check(ctx, dev, dev.frames(), starts, lens, 7, 0, cap, steps)
    dev.close()


@pytest.mark.parametrize("bl, bpf, codes", [(10, 40, (0, 1, 3)), (40, 10, (0, 1, 3)), (20, 20, (1, 1, 3))])
def test_block_lengths_and_code_sets(ctx, x3, bl, bpf, codes):
    for index in ("walk", None):
        dev = T.base(ctx, x3, index, bl, bpf, codes)
        assert dev.F == 6 and dev.so[1] == 400
        first = 1 + SB * bl                                   # the second stretch's first sample
        starts, lens = TF.grid([0, 1, first - 1, first, first + 1, 399, 400, 400 + first, 401, 800, 2136], [0, 1, 21, 400, 401, N])
        for bin_len, k in ((0, 3), (7, 8), (400, 2)):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, POOL[:k], seg=index is not None)
            if not any(st for st, _ in dev.frames()):             # (with codes (1, 1, 3) frames fail to decode: the reader's)
                assert ctx.get_option("last_range_levels_replays") == 0
        dev.close()


def test_a_random_table(ctx, x3):
    tab = TT._random_table()
    tab[5], tab[1023] = (-32768, 32767), (32767, -32768)
    for index in ("ref", None):
        dev = T.base(ctx, x3, index)
        d_tab = TT._table(dev, tab)
        starts, lens = TF.grid(STARTS)
        for bin_len, k in ((0, 4), (7, 5), (401, 2), (1, 3)):
            both_layouts(ctx, dev, dev.frames(), starts, lens, bin_len, POOL[:k], tab, d_tab, seg=index is not None)
        dev.close()


def test_a_table_of_ones_gives_the_sums_of_x3_range_levels_dev_in_every_plane(ctx, x3):
    """all (1, 0): re is the SAMPLES record's sum and im is 0 in every plane, whatever the steps; min, max, n, row offsets and
    statuses are its bytes"""
    dev = TF._hurt(ctx, x3, 2)
    d_ones = TT._table(dev, ONES)
    starts, lens = T.base_ranges(seed=7)
    for (bin_len, stride), k in zip(((0, 0), (7, 0), (400, 0), (100, 25)), (8, 3, 2, 5)):
        cap = len(starts) * stride or T.rows_total(lens, bin_len) - 5        # (packed: the last ranges have no room)
        old = T.run(ctx, dev.call, starts, lens, bin_len, stride, cap)
        plain = R.view(old[0])
        written = plain["reserved"] == 0                                    # (what no call may write keeps its 0x5A)
        assert written.any() and (old[2] == BAD).any()
        new = run(ctx, call(dev, POOL[:k], d_ones), k, starts, lens, bin_len, stride, cap)
        assert np.array_equal(new[1], old[1]) and np.array_equal(new[2], old[2]) and new[3] == old[3]
        for t in range(k):
            rec = TR.view(new[0][t])
            assert np.array_equal(new[0][t][~written], old[0][~written])
            assert np.array_equal(rec["re"][written], plain["sum"][written]) and not rec["im"][written].any()
            for name in ("min", "max", "n", "reserved"):
                assert np.array_equal(rec[name], plain[name]), name
    dev.close()


# ------------------------------------------------------------------------------------------------ planes not written

@pytest.mark.parametrize("k", [2, 3, 8])
def test_records_no_call_writes_keep_their_bytes_in_every_plane(ctx, x3, k):
    """packed with rows_cap one above, at and one below the rows drawn, and far below; padded with rows_cap above
    n * stride: the records of ranges without room and those behind n * stride carry 0x5A in every plane, and plane t's last
    written record lies in front of plane t + 1's first"""
    dev = T.base(ctx, x3)
    frames = dev.frames()
    starts, lens = T.base_ranges(seed=3)
    steps = POOL[:k]
    drawn = T.rows_total(lens, 20)
    for cap in (drawn + 1, drawn, drawn - 1, drawn // 2):
        out, off, st, total = check(ctx, dev, frames, starts, lens, 20, 0, cap, steps)
        assert total == drawn
        rows = [TR.rows_of(v, 20) for v in lens]
        room = np.array([int(off[w]) + rows[w] <= cap for w in range(len(lens))])
        assert ((st == BAD) >= ~room).all() and (cap >= drawn or (~room).any())
        for t in range(k):
            assert (out[t, min(drawn, cap):] == 0x5A).all()                  # behind the rows drawn: nobody's, in no plane
            for w in np.flatnonzero(~room):
                assert (out[t, int(off[w]):min(int(off[w]) + rows[w], cap)] == 0x5A).all(), (t, w)
    n = len(starts)
    for stride, extra in ((5, 1), (5, 7), (1, 0)):
        out, off, st, _ = check(ctx, dev, frames, starts, lens, 20, stride, n * stride + extra, steps)
        for t in range(k):
            assert (out[t, n * stride:] == 0x5A).all() and not (out[t, :n * stride] == 0x5A).all(axis=1).any()
    dev.close()


# ------------------------------------------------------------------------------------------------ damage

@pytest.mark.parametrize("f", [0, 2, 5])
def test_a_payload_crc_failure_adds_to_no_plane(ctx, x3, f):
    dev = TF._hurt(ctx, x3, f)
    frames = dev.frames()
    a, b = int(dev.so[f]), int(dev.so[f + 1])
    starts, lens = damage_ranges()
    for (bin_len, stride), k in zip(((7, 0), (400, 0), (0, 0), (100, 25)), (3, 8, 2, 5)):
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len),
                                POOL[1:1 + k])
        assert ctx.get_option("last_range_levels_replays") == 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):          # the status is the SAMPLES call's
        covers = ln and s0 < b and s0 + ln > a and s0 <= N and ln <= N - s0
        assert (st[w] == CRC) == bool(covers), (s0, ln, st[w])
    one = check(ctx, dev, frames, [0], [N], 0, 0, 1, POOL[:4])
    assert [int(TR.view(one[0][t])["n"][0]) for t in range(4)] == [N - (b - a)] * 4
    dev.close()


def test_a_late_decode_error_goes_through_the_fixup_of_eight_slots(ctx, x3):
    """frame 2 fails late in its payload under a valid CRC: its stretches flag it, the fix-up (the NT = 8 instance for every
    bank) replays it through the reader for its status; it adds to no plane"""
    dev, rc2 = TF._late_error(ctx, x3)
    frames = dev.frames()
    assert [st for st, _ in frames] == [0, 0, rc2, 0, 0, 0] and rc2 not in (CRC, BAD)
    starts, lens = damage_ranges()
    for (bin_len, stride), k in zip(((7, 0), (400, 0), (0, 0), (100, 25)), (2, 5, 8, 3)):
        out, off, st, _ = check(ctx, dev, frames, starts, lens, bin_len, stride, len(starts) * stride or T.rows_total(lens, bin_len),
                                POOL[1:1 + k])
        assert ctx.get_option("last_range_levels_replays") > 0
    for w, (s0, ln) in enumerate(zip(starts, lens)):
        covers = ln and s0 < 1200 and s0 + ln > 800 and s0 + ln <= N
        assert (st[w] == rc2) == bool(covers), (s0, ln, st[w])
    dev.close()


@pytest.mark.parametrize("how", ["bit", "sample"])
def test_a_wrong_index_entry_changes_nothing(ctx, x3, how):
    """frame 2, entry 2: a bit position one late, or a last sample with its lowest bit flipped.  The frame is flagged and
    replayed to status 0 in the fix-up, whose eight phases are seeded with the position of the frame's sample 0 and stepped
    to the range's cut: every plane is the same bytes as with the right index"""
    dev = T.base(ctx, x3)
    frames = dev.frames()
    nw = SR.n_words(6, dev.op, SB)
    good = ctx.download(dev.d_seg, 8 * nw, np.uint64)
    per = (nw - 1) // 6
    bad = good.copy()
    bad[1 + 2 * per + 1] = bad[1 + 2 * per + 1] + np.uint64(1) if how == "bit" else bad[1 + 2 * per + 1] ^ np.uint64(1 << 32)
    starts, lens = damage_ranges()
    for (bin_len, stride), k in zip(((7, 0), (0, 0), (100, 25)), (8, 2, 3)):
        steps = POOL[1:1 + k]
        cap = len(starts) * stride or T.rows_total(lens, bin_len)
        ctx.upload(dev.d_seg, good)
        want = run(ctx, call(dev, steps), k, starts, lens, bin_len, stride, cap)
        assert ctx.get_option("last_range_levels_replays") == 0
        ctx.upload(dev.d_seg, bad)
        got = check(ctx, dev, frames, starts, lens, bin_len, stride, cap, steps)
        assert ctx.get_option("last_range_levels_replays") > 0
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    dev.close()


# ------------------------------------------------------------------------------------------------ shared frames

@pytest.mark.parametrize("n", [2, 40])
def test_ranges_that_all_cover_all_six_frames(ctx, x3, n):
    """40 ranges over 6 frames are 240 pairs against P = min(40 * 6, 4 * (6 + 40)) = 184, the SAMPLES form's: the 56 pairs
    beyond have no rows in any plane and go through the reader in the fix-up; every plane is right"""
    dev = T.base(ctx, x3)
    starts = [w % 3 for w in range(n)]
    lens = [N - 2 - (w % 5) for w in range(n)]
    over = max(0, n * 6 - 4 * (6 + n))
    assert over == (56 if n == 40 else 0)
    for bin_len, k in ((0, 8), (7, 3), (400, 2), (20, 5)):
        check(ctx, dev, dev.frames(), starts, lens, bin_len, 0, T.rows_total(lens, bin_len), POOL[1:1 + k])
        assert counters(ctx) == (over, over)
    dev.close()


def test_more_ranges_than_threads_of_the_scans(ctx, x3):
    dev = T.base(ctx, x3)
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 60, 3000).tolist()
    starts = (rng.integers(0, (N - 60) // 20, 3000) * 20 + rng.integers(0, 8, 3000)).tolist()   # many near frame and stretch starts
    check(ctx, dev, dev.frames(), starts, lens, 7, 0, T.rows_total(lens, 7), POOL[1:4])
    check(ctx, dev, dev.frames(), starts, lens, 0, 2, 6000, POOL[1:6], singles=False)
    dev.close()


# ------------------------------------------------------------------------------------------------ against the bank levels call

def _bank_levels(dev, bin_len, n_bins, steps):
    k = len(steps)
    d_lv, d_st = dev.alloc(REC * k * n_bins), dev.alloc(4 * dev.F)
    assert dev.ctx.tone_bank_levels_dev(dev.d_x3, dev.len, dev.d_off, dev.d_so, dev.F, dev.p, bin_len, d_lv, n_bins, d_st, dev.d_seg,
                                        dev.sb, bank_of(dev.x3, dev.ctx, steps)) == 0
    assert dev.ctx.levels_result()[0] == 0
    return dev.ctx.download(d_lv, REC * k * n_bins, TL.TONE_DTYPE).reshape(k, n_bins)


@pytest.mark.parametrize("hurt", [None, 0, 2, 5])
def test_the_whole_stream_equals_x3_tone_bank_levels_dev(ctx, x3, hurt):
    dev = T.base(ctx, x3) if hurt is None else TF._hurt(ctx, x3, hurt)
    for k in (2, 4, 5):
        steps = POOL[1:1 + k]
        for bin_len in BINS:
            n_bins = TR.rows_of(N, bin_len)
            lv = _bank_levels(dev, bin_len, n_bins, steps)
            out, off, st, total = run(ctx, call(dev, steps), k, [0], [N], bin_len, 0, n_bins)
            assert total == n_bins and st.tolist() == [0 if hurt is None else CRC]
            assert out.tobytes() == lv.tobytes(), (k, bin_len)
    assert ctx.get_option("last_range_levels_replays") == 0
    dev.close()


# ------------------------------------------------------------------------------------------------ corpus

@pytest.mark.parametrize("index", ["decode", "walk"])
def test_corpus_ranges_equal_the_stream_form_on_each_entry(ctx, x3, index):
    """TF's corpus (entries of 1, 399, 2 137, 0, 1 000, 400 and 5 samples): every range's records equal, in every plane, the
    stream form's on that entry alone -- phase 0 at every entry -- and the single corpus call's bytes"""
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
    for (bin_len, stride), k in zip(((0, 0), (7, 0), (400, 0), (100, 22)), (5, 3, 2, 8)):
        steps = POOL[1:1 + k]
        bank = bank_of(x3, ctx, steps)
        cap = len(tab) * stride or T.rows_total(lens, bin_len)
        out, off, st, total = run(ctx, lambda *a: corpus.tone_bank_range_levels_into(*a, bank), k, starts, lens, bin_len, stride, cap,
                                  entries=ent)
        assert total == T.rows_total(lens, bin_len)
        for t, step in enumerate(steps):                      # the single corpus call's bytes, offsets and statuses
            tone = x3.LevelTone(step, 0, ctx.tone_table_dev())
            one = T.run(ctx, lambda *a: corpus.tone_range_levels_into(*a, tone), starts, lens, bin_len, stride, cap, entries=ent)
            assert out[t].tobytes() == one[0].tobytes() and np.array_equal(one[1], off) and np.array_equal(one[2], st)
        for w, (e, s0, ln) in enumerate(tab):
            rows = stride or TR.rows_of(ln, bin_len)
            mine = out[:, int(off[w]):int(off[w]) + rows]
            if e >= ne or devs[e] is None:
                assert st[w] == BAD, (e, s0, ln)             # not in the corpus, or an entry without frames
                for t in range(k):
                    assert np.array_equal(TR.view(mine[t]), TL.empty(rows)), (e, s0, ln)
                continue
            d = devs[e]
            want = BR.range_levels(d.frames(), d.so, [s0], [ln], bin_len, stride, rows, steps)
            alone = run(ctx, call(d, steps, seg=False), k, [s0], [ln], bin_len, stride, rows)     # the stream form, on that entry alone
            assert st[w] == alone[2][0] == want[2][0], (e, s0, ln, st[w])
            assert mine.tobytes() == alone[0].tobytes() == want[0].tobytes(), (e, s0, ln)
            seen.add(int(st[w]))
    assert seen == {0, BAD, CRC}
    assert ctx.get_option("last_range_levels_replays") == 0
    for d in devs:
        if d is not None:
            d.close()
    corpus.close()


def test_a_repeated_entry_and_an_empty_one(ctx, x3):
    """the base stream as entries 0 and 2 with an empty entry between them: the same ranges in both give the same bytes in
    every plane (phase 0 at each entry's start), equal to the stream form's; the empty entry refuses its ranges"""
    dev = T.base(ctx, x3)
    s = dev.stream
    pad = np.zeros(s.size % 2, dtype=np.uint8)
    buf = np.concatenate([s, pad, s, np.zeros(16, dtype=np.uint8)])
    at = s.size + pad.size
    corpus = x3.Corpus(ctx, buf, [0, at, at], [s.size, 0, s.size], params=dev.p, seg_blocks=SB, index="walk")
    assert corpus.entries["n_samples"].tolist() == [N, 0, N]
    starts, lens = [0, 81, 399, 801, 2000, 0, 5], [N, 400, 3, 1000, 137, 1, 0]
    n = len(starts)
    steps = POOL[1:6]
    bank = bank_of(x3, ctx, steps)
    for bin_len, stride in ((7, 0), (0, 0), (100, 22)):
        cap = 3 * n * stride or 3 * T.rows_total(lens, bin_len)
        out, off, st, _ = run(ctx, lambda *a: corpus.tone_bank_range_levels_into(*a, bank), 5, starts * 3, lens * 3, bin_len, stride, cap,
                              entries=[0] * n + [2] * n + [1] * n)
        alone = run(ctx, call(dev, steps), 5, starts, lens, bin_len, stride, cap // 3)
        rows = int(off[n])
        assert not st[:2 * n].any() and (st[2 * n:] == BAD).all()
        assert np.array_equal(out[:, :rows], alone[0][:, :rows]) and np.array_equal(out[:, rows:2 * rows], alone[0][:, :rows])
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ refusals, pending state

def test_refusals_and_pending_states(ctx, x3):
    L = x3.lib()
    dev = TF._hurt(ctx, x3, 2)
    n, cap, K = 4, 64, 3
    steps = POOL[1:1 + K]
    sizes = {"lv": REC * K * cap, "off": 8 * (n + 1), "st": 4 * n}
    d = {k: dev.alloc(v) for k, v in sizes.items()}
    d_starts, d_lens = dev.alloc(8 * n), dev.alloc(4 * n)
    ctx.upload(d_starts, np.array([0, 400, 800, 1200], dtype=np.uint64))
    ctx.upload(d_lens, np.full(n, 400, dtype=np.uint32))

    def poison():
        for k, v in sizes.items():
            ctx.upload(d[k], np.full(v, 0x5A, dtype=np.uint8))
    poison()
    d_tab = ctx.tone_table_dev()
    ok = bank_of(x3, ctx, steps)

    def raw(c=ctx._h, x=dev.d_x3, fo=dev.d_off, so=dev.d_so, nf=dev.F, params=dev.p, idx=dev.d_seg, sb=SB, starts=d_starts,
            lens=d_lens, nr=n, bl=100, stride=0, lv=d["lv"], rows=cap, off=d["off"], st=d["st"], bank=ok):
        return L.x3_tone_bank_range_levels_dev(c, x, dev.len, fo, so, nf, C.byref(params), idx, sb, starts, lens, nr, bl, stride, lv,
                                               rows, off, st, C.byref(bank) if bank is not None else None)
    # a pending call first: every refusal below leaves its slot as it is
    assert dev.call(d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"]) == 0
    ctx.sync()
    pending = {k: ctx.download(d[k], v) for k, v in sizes.items()}
    bad_banks = [None, bank_of(x3, ctx, steps, n_tones=0), bank_of(x3, ctx, steps, n_tones=9), bank_of(x3, ctx, steps, n_tones=2 ** 31),
                 bank_of(x3, ctx, steps, reserved=1), bank_of(x3, ctx, steps, d_table=None), bank_of(x3, ctx, steps, d_table=d_tab + 2),
                 bank_of(x3, ctx, steps[:1], n_tones=0), bank_of(x3, ctx, steps[:1], reserved=1), bank_of(x3, ctx, steps[:1], d_table=None)]
    for bank in bad_banks:                                       # an invalid bank is refused first: whatever else is wrong
        assert raw(bank=bank) == BAD and raw(bank=bank, x=None, nr=0, rows=0) == BAD
    # n_tones * rows_cap above 2^31 - 1 with rows_cap itself legal, by argument only (the records lie in the 64-row buffer):
    # 2 * 2^30 = 2^31, 3 * 715 827 883 = 2^31 + 1, 8 * 2^28 = 2^31; one tone is bound by rows_cap alone (2^31 is refused
    # there as everywhere).  The largest legal products -- 0x7FFFFFFF itself with one tone, 2 * 0x3FFFFFFF -- would size a
    # workspace of 64 GiB, so no call is made with them; the bound is held from above
    for rows, bank in ((2 ** 30, bank_of(x3, ctx, steps[:2])), (715_827_883, ok), (2 ** 28, bank_of(x3, ctx, POOL[:8])),
                       (2 ** 31, bank_of(x3, ctx, steps[:1])), (0x7FFFFFFF, bank_of(x3, ctx, steps[:2]))):
        assert raw(rows=rows, bank=bank) == BAD and raw(rows=rows, bank=bank, stride=1) == BAD, rows
    bad_p = x3.Params.make(block_len=20, blocks_per_frame=20)
    bad_p.block_len = 0
    assert raw(bank=None, params=bad_p) == BAD and raw(params=bad_p) != 0
    for r in (dict(c=None), dict(nr=0), dict(nr=2 ** 31), dict(rows=0), dict(rows=2 ** 31), dict(starts=None), dict(lens=None),
              dict(lv=None), dict(st=None), dict(off=None), dict(starts=d_starts + 4), dict(lens=d_lens + 2), dict(lv=d["lv"] + 4),
              dict(off=d["off"] + 4), dict(st=d["st"] + 2), dict(sb=3), dict(sb=0), dict(stride=17), dict(stride=2 ** 63),
              dict(x=None), dict(fo=dev.d_off + 4), dict(so=dev.d_so + 4)):
        assert raw(**r) == BAD, r
    corpus = x3.Corpus(ctx, dev.stream, [0], [dev.len], params=dev.p, seg_blocks=SB, index="walk")
    d_ent = dev.alloc(4 * n + 4)
    ctx.upload(d_ent, np.zeros(n + 1, dtype=np.uint32))
    cok = dict(d_entries=d_ent, d_starts=d_starts, d_lens=d_lens, n=n, bin_len=100, row_stride=0, d_levels=d["lv"], rows_cap=cap,
               d_row_offsets=d["off"], d_status=d["st"], tones=ok)
    for r in [dict(tones=b) for b in bad_banks[1:]] + [dict(d_entries=None), dict(d_entries=d_ent + 2), dict(n=0), dict(rows_cap=0),
                                                       dict(rows_cap=715_827_883), dict(d_starts=None), dict(d_levels=d["lv"] + 4),
                                                       dict(d_row_offsets=None), dict(row_stride=17)]:
        assert corpus.tone_bank_range_levels_into(**dict(cok, **r)) == BAD, r
    for bank in (None, ok):
        assert L.x3_corpus_tone_bank_range_levels_dev(ctx._h, None if bank else corpus._h, d_ent, d_starts, d_lens, n, 100, 0, d["lv"],
                                                      cap, d["off"], d["st"], C.byref(bank) if bank else None) == BAD
    ctx.graph_begin()
    try:
        assert raw() == BAD and corpus.tone_bank_range_levels_into(**cok) == BAD      # a context that records a graph
    finally:
        try:
            ctx.graph_destroy(ctx.graph_end())
        except x3.X3Error:
            pass                                                                 # (a recording of nothing)
    ctx.sync()
    for k, v in sizes.items():
        assert np.array_equal(ctx.download(d[k], v), pending[k]), k           # nothing was enqueued by any refusal ...
    assert ctx.range_levels_result() == (0, 1, 2, CRC, 16)                    # ... and the pending call's result is intact
    assert ctx.range_levels_result()[0] == BAD                                # nothing else is pending
    # the call itself, beside a SAMPLES call and a tone call on the same slot: the last call's summary is the one pending
    poison()
    frames = dev.frames()
    want = BR.range_levels(frames, dev.so, [0, 400, 800, 1200], [400] * 4, 100, 0, cap, steps)
    assert dev.call(d_starts, d_lens, n, 100, 0, d["lv"], cap, d["off"], d["st"]) == 0 and raw(nr=2) == 0
    assert ctx.range_levels_result() == (0, 0, 2, 0, 8) and ctx.range_levels_result()[0] == BAD
    poison()
    assert raw() == 0 and ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    got = ctx.download(d["lv"], REC * K * cap).reshape(K, cap, REC)
    for t in range(K):
        TT.same(got[t], want[0][t], ("plane", t))
    assert TR.view(want[0][1][:16])["n"].tolist() == [100] * 8 + [0] * 4 + [100] * 4     # frame 2 and nothing else, in a plane
    poison()
    assert corpus.tone_bank_range_levels_into(**cok) == 0 and ctx.range_levels_result() == (0, 1, 2, CRC, 16)
    assert ctx.download(d["lv"], REC * K * cap).tobytes() == got.tobytes()
    # a table at an address that is 4-byte aligned and no more
    d_odd = dev.alloc(4096 + 4)
    ctx.upload(d_odd + 4, TL.table())
    poison()
    assert raw(bank=bank_of(x3, ctx, steps, d_odd + 4)) == 0 and ctx.range_levels_result()[0] == 0
    assert ctx.download(d["lv"], REC * K * cap).tobytes() == got.tobytes()
    corpus.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ behind a stall

def test_one_call_behind_a_stalled_caller_stream(x3):
    """as test_gpu_tone_range_levels.py's: the context runs on the caller's stream, which is stalled.  At the call the device
    table and the device starts still hold a decoy -- their content is copied behind the stall -- and the host
    x3_level_tone_bank is overwritten right after the call: every plane is that of the table and starts as they are when the
    kernels run and of the struct as it was at the call"""
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
    tab = TT._random_table(21)
    steps = [EXAMPLE_STEP, 2 ** 32 - 1, ODD]
    K, n, bin_len = len(steps), len(starts), 100
    cap = T.rows_total(lens, bin_len)
    want = BR.range_levels(frames, so, starts, lens, bin_len, 0, cap, steps, tab)
    decoy = BR.range_levels(frames, so, [0] * n, lens, bin_len, 0, cap, [12345, 1, 2], ONES)
    assert not any(np.array_equal(want[0][t], decoy[0][t]) for t in range(K))
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
            outs = {"lv": torch.empty(REC * K * cap + 64, dtype=torch.uint8, device="cuda"),
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
                bank = x3.LevelToneBank(K, 0, d_tab.data_ptr(), (C.c_uint32 * 8)(*(steps + [7] * 5)))
                other = x3.LevelToneBank(2, 0, decoy_tab.data_ptr(), (C.c_uint32 * 8)(*([12345] * 8)))
                if stall_ms:
                    torch.cuda._sleep(int(stall_ms * cycles_per_ms))
                behind = torch.cuda.Event()
                behind.record(S)
                d_tab.copy_(src_tab, non_blocking=True)                      # the content arrives behind the stall
                d_starts.copy_(src_starts, non_blocking=True)
                assert ctx.tone_bank_range_levels_dev(d_x3.data_ptr(), s.size, d_off.data_ptr(), d_so.data_ptr(), F, p,
                                                      d_starts.data_ptr(), d_lens.data_ptr(), n, bin_len, 0, outs["lv"].data_ptr(), cap,
                                                      outs["off"].data_ptr(), outs["st"].data_ptr(), d_seg.data_ptr(), SB,
                                                      bank) == 0, ctx.last_error()
                C.memmove(C.byref(bank), C.byref(other), C.sizeof(bank))    # the host struct, overwritten right after the call
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
            assert bank.n_tones == 2 and bank.steps[0] == 12345                  # (the overwrite took place)
            res = ctx.range_levels_result()
            assert res == (0, 0, n, 0, cap), res
            lv, off, st = (outs[k].cpu().numpy() for k in ("lv", "off", "st"))
            for a, size in ((lv, REC * K * cap), (off, 8 * (n + 1)), (st, 4 * n)):
                assert (a[size:] == AC.CANARY).all()
            got = lv[:REC * K * cap].reshape(K, cap, REC)
            for t in range(K):
                TT.same(got[t], want[0][t], "behind the stall, plane %d" % t)
            assert np.array_equal(off[:8 * (n + 1)].view(np.uint64), want[1]) and not st[:4 * n].any()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ what it is for

def test_two_events_found_by_the_bank_are_looked_at_again_in_all_four_bands(ctx, x3):
    """DESIGN.md section 27's example end to end: tone_bank_levels(200, tones, band=True) on section 26's signal, events on every
    plane as it lies, the ranges found -- (4 400, 200) in plane 0, (12 000, 200) in plane 1 -- padded by 100 positions either
    side into tone_bank_range_levels(..., 100, tones, band=True): a [4, 8, 32] tensor whose band mean squares are the table of
    test_tone_bank_range_levels_ref.py; at a threshold of 300 000 exactly rows 1 and 2 of plane 0 in range 0 and rows 1 and 2 of
    plane 1 in range 1 are loud"""
    import torch
    w = B.example()
    p, op = x3.Params.make(20, 100), O.Params.make(20, 100, (0, 1, 3))
    rc, stream, _ = O.encode(w, op)
    assert rc == 0
    frames, so = [(0, w[a:a + 2_000]) for a in range(0, 20_000, 2_000)], R.sample_offsets([2_000] * 10)
    tones = x3.Tone.bank(B.EXAMPLE_FREQS, 1.0)
    assert tuple(t.step for t in tones) == B.EXAMPLE_STEPS
    rule = x3.EventRule.make(mean_sq_min=400_000)
    dev = torch.device("cuda", torch.cuda.current_device())
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=8)
    d_lv = ctx.alloc(32 * 4 * 100)
    try:
        lv, fst = ws.tone_bank_levels(200, tones, band=True)
        assert lv.shape == (4, 100) and not fst.any()
        assert ws.tone_bank_levels_into(200, tones, d_lv, 100, band=True) == 0 and ctx.levels_result() == (0, 0, 10, 0)
        found_s, found_l = [], []
        for t in range(4):                                                   # events on every plane as it lies
            h_st, h_ln = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
            h_el, h_cnt = torch.empty((4, 32), dtype=torch.uint8, device=dev), torch.empty((), dtype=torch.int64, device=dev)
            torch.cuda.current_stream().synchronize()
            assert ws.events_into(d_lv + 32 * 100 * t, 100, 200, rule, h_st.data_ptr(), h_ln.data_ptr(), h_el.data_ptr(), 4,
                                  h_cnt.data_ptr()) == 0
            assert ctx.events_result()[0] == 0
            found_s.append(h_st[:int(h_cnt)])
            found_l.append(h_ln[:int(h_cnt)])
        assert [v.tolist() for v in found_s] == [[4_400], [12_000], [], []] and [v.tolist() for v in found_l] == [[200], [200], [], []]
        starts, lens = torch.cat(found_s) - 100, torch.cat(found_l) + 200
        assert (starts.tolist(), lens.tolist()) == EX.EXAMPLE_RANGES
        band, off, st = ws.tone_bank_range_levels(starts, lens, 100, tones, band=True)
        assert isinstance(band, torch.Tensor) and tuple(band.shape) == (4, 8, 32) and off.tolist() == [0, 4, 8] and st.tolist() == [0, 0]
        want = BR.range_levels(frames, so, [4_300, 11_900], [400, 400], 100, 0, 8, B.EXAMPLE_STEPS)
        want_band = np.stack([TL.tone_power_levels(TR.view(want[0][t])) for t in range(4)])
        assert band.cpu().numpy().tobytes() == want_band.tobytes()
        ms = EX.example_band_ms(band.cpu().numpy())
        assert ms == EX.EXAMPLE_BAND_MS
        assert [(r, t, b) for r in range(2) for t in range(4) for b in range(4) if ms[r][t][b] >= 300_000] == \
            [(0, 0, 1), (0, 0, 2), (1, 1, 1), (1, 1, 2)]
        raw, off, st = ws.tone_bank_range_levels(starts, lens, 100, tones)       # the quadrature sums themselves
        assert tuple(raw.shape) == (4, 8, 32) and raw.cpu().numpy().tobytes() == want[0].tobytes()
        for t in range(4):                                                       # plane t is the single call's tensor
            one, _, _ = ws.tone_range_levels(starts, lens, 100, tones[t])
            assert torch.equal(raw[t], one)
        one, _, _ = ws.tone_bank_range_levels(starts, lens, 100, tones[:1])
        assert tuple(one.shape) == (1, 8, 32) and torch.equal(one[0], raw[0])
        # padded to a stride that refuses the ranges, and packed without room: identities after the adapter in every plane
        for kw in (dict(padded_to=3), dict(capacity=3)):
            none, off, st = ws.tone_bank_range_levels(starts, lens, 100, tones, band=True, **kw)
            rows = 6 if "padded_to" in kw else 3
            assert st.tolist() == [BAD, BAD] and tuple(none.shape) == (4, rows, 32)
            assert np.array_equal(R.view(none.cpu().numpy().reshape(-1, 32)), LR.empty(4 * rows))
        with pytest.raises(ValueError, match="call tone_bank_range_levels"):
            ws.range_levels(starts, lens, 100, signal=tones)
        for bad in ((), tones + tones + tones, tones[0], None):
            with pytest.raises(ValueError, match="1 .. 8 Tone"):
                ws.tone_bank_range_levels(starts, lens, 100, bad)
    finally:
        ctx.free(d_lv)
        ws.close()
    corpus = x3.Corpus(ctx, np.concatenate([stream, stream]), [0, stream.size], [stream.size, stream.size], params=p, seg_blocks=8,
                       index="walk")
    try:
        ent = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=dev)
        cs, cl = torch.cat([starts, starts]), torch.cat([lens, lens])
        cband, off, st = corpus.tone_bank_range_levels(ent, cs, cl, 100, tones, band=True)
        assert tuple(cband.shape) == (4, 16, 32) and off.tolist() == [0, 4, 8, 12, 16] and not st.any()
        assert torch.equal(cband[:, :8], band) and torch.equal(cband[:, 8:], band)       # phase 0 at each entry
        craw, off, st = corpus.tone_bank_range_levels(ent, cs, cl, 100, tones)
        assert torch.equal(craw[:, :8], raw) and torch.equal(craw[:, 8:], raw)
        with pytest.raises(ValueError, match="call tone_bank_range_levels"):
            corpus.range_levels(ent, cs, cl, 100, signal=list(tones))
    finally:
        corpus.close()
