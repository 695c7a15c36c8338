"""The stalled-stream cases of the analysis calls (not a test module): levels, events, quantiles, thresholds, range levels
and x3_corpus_ranges_dev behind async_cases.run_stalled, which is used as it is.

include/x3hip.h says of every one of these calls "Asynchronous on the context's stream: one launch set, no host trip".  Their
own tests upload, wait, call and fetch, so the GPU never lags behind the host in them.  Here the stream bytes, the frame
offsets and every device table (starts, lens, entries, level records, totals, thresholds) hold a decoy A when the host
enqueues, the content B arrives behind the stall, and x3_sample_offsets_dev / x3_seg_index_build_dev are enqueued inside
the case in front of the calls under test, so that the sample offsets and the index are device data of the same pass.

The stream content is async_cases': 48 frames of 10 000 samples with loud frames.
    "A" / "B"   AC.encoded(which)                "Bd"  AC.damaged_b(): frames 9 (payload CRC) and 30 (decode error)
    "Ad"        A with a payload-CRC failure in frame 8, the frame behind the loud frame 7 -- the decoy of every stream case:
                its frame statuses and result calls differ from clean B's as well as from Bd's
The corpus content: six entries in frames of 1 000 samples (12 .. 30 frames each); one entry is white noise, the others hold
two or three bursts, each inside one frame, over a floor of +-8.  The corpus references the harness's work buffer and its
frame table is fixed at the build, so the decoy is B's bytes with one payload byte flipped in the frame of each entry's first
burst: B's geometry exactly, and failed frames add nothing, so records, statuses and events differ in every entry.

Every expectation comes from the CPU references of tests/ (levels_ref, diff_levels_ref, fir_levels_ref, events_ref,
quantiles_ref, range_levels_ref, signal_range_levels_ref, fir_range_levels_ref, ranges_ref, seg_index_ref)."""
import functools

import numpy as np

import async_cases as AC
import diff_levels_ref as DL
import events_ref as E
import fir_levels_ref as FL
import fir_range_levels_ref as FR
import levels_ref as L
import oracle_lib as O
import quantiles_ref as Q
import range_levels_ref as RL
import ranges_ref as RR
import seg_index_ref as SI
import signal_range_levels_ref as SR
from x3_cases import frame_offsets

CANARY, SPF, F0, N0 = AC.CANARY, AC.SPF, AC.F0, AC.N0
CANARY16 = CANARY << 8 | CANARY
CRC = AC.ERR_PAYLOAD_CRC
SB = 32                      # seg_blocks of x3_seg_index_build_dev and of every call that takes the index
BIN = 641                    # divides neither the frame (10 000) nor the block (20)
NB = L.n_bins_for(N0, BIN)
SO = np.arange(F0 + 1, dtype=np.uint64) * np.uint64(SPF)
NW = SI.n_words(F0, AC.oparams(), SB)
AD_FRAME = 8

# name -> (taps, shift) of a FIR signal, or the `signal` of the signal calls
FIRS = {"fir3": ((1, -2, 1), 0), "fir8": ((-1000, 2900, -5000, 7400, -7400, 5000, -2900, 1000), 7),
        "fir4": ((1, 1, 1, 1), 2), "fir121": ((1, 2, 1), 2)}
SIGNALS = {"samples": DL.SAMPLES, "diff": DL.DIFF}
assert all(FL.check(t, s) for t, s in FIRS.values())

# the one result that no single-entry content can make differ: no entry is without counting rows in A or in B
NONE_EMPTY = "n_empty is 0 and first_empty the entry count by construction: every entry of A and of B has counting rows"
CLEAN_RANGES = "statuses of clean content: no event of A or B covers a damaged frame"


# ------------------------------------------------------------------------------------------------ stream content

@functools.lru_cache(maxsize=None)
def stream(kind):
    """-> (stream bytes, per-frame status)"""
    if kind == "Bd":
        return AC.damaged_b()
    s, offs, _ = AC.encoded(kind[0])
    st = np.zeros(F0, dtype=np.int32)
    if kind == "Ad":
        s = s.copy()
        s[int(offs[AD_FRAME]) + 20 + 77] ^= 0x20
        st[AD_FRAME] = CRC
    return s, st


def offsets(kind):
    return AC.encoded(kind[0])[1]


@functools.lru_cache(maxsize=None)
def x3_bytes():
    kinds = ("A", "Ad", "B", "Bd")
    return dict(zip(kinds, AC.padded([stream(k)[0] for k in kinds])))


def x3_len():
    return x3_bytes()["B"].size


def wav_frames(kind):
    w = AC.wav(kind[0])
    return [w[f * SPF:(f + 1) * SPF] for f in range(F0)]


@functools.lru_cache(maxsize=None)
def frames(kind):
    """ranges_ref.frames_of's form: per frame (status, samples or None)"""
    return [(int(st), w if st == 0 else None) for st, w in zip(stream(kind)[1], wav_frames(kind))]


def summary(st):
    """what x3_levels_result / the range result calls say about statuses: (rc, n_bad, first_bad, its status)"""
    bad = np.flatnonzero(st)
    return (0, int(bad.size), int(bad[0]) if bad.size else len(st), int(st[bad[0]]) if bad.size else 0)


def levels_of(fr, st, so, bin_len, n_bins, signal):
    if signal in SIGNALS:
        return DL.signal_levels(fr, st, so, bin_len, n_bins, SIGNALS[signal])
    taps, shift = FIRS[signal]
    return FL.fir_levels(fr, st, so, bin_len, n_bins, taps, shift)


@functools.lru_cache(maxsize=None)
def stream_levels(kind, signal):
    lv = levels_of(wav_frames(kind), stream(kind)[1], SO[:-1], BIN, NB, signal)
    lv.setflags(write=False)
    return lv


@functools.lru_cache(maxsize=None)
def seg_segments(kind):
    """the index words of the frames that decode (seg_index_ref.build takes intact frames only): the header word and a
    segment per good frame; what the walk leaves in a failed frame's words is compared between clone and original only"""
    words = SI.build(AC.encoded(kind[0])[0], offsets(kind)[:-1], AC.oparams(), SB)[0]
    per = (NW - 1) // F0
    segs = [(0, words[:1], False)]
    for f in np.flatnonzero(stream(kind)[1] == 0):
        segs.append((8 * (1 + int(f) * per), words[1 + int(f) * per:1 + (int(f) + 1) * per], False))
    return segs


def range_levels_of(fr, so, starts, lens, bin_len, stride, cap, signal):
    """-> (records uint8 [cap, 32] with CANARY where no call writes, row offsets, statuses)"""
    if signal in SIGNALS:
        return SR.range_levels(fr, so, starts, lens, bin_len, stride, cap, SIGNALS[signal], fill=CANARY)
    taps, shift = FIRS[signal]
    return FR.range_levels(fr, so, starts, lens, bin_len, stride, cap, taps, shift, fill=CANARY)


def fir_of(x3, name):
    return x3.Fir(*FIRS[name])


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def word(v):
    return np.array([v], dtype=np.uint64)


class StreamCase(AC.Case):
    """the stream bytes and frame offsets as inputs; x3_sample_offsets_dev and x3_seg_index_build_dev in front"""
    decoy, content = "Ad", "B"
    same_ok = {"so": "both contents are cut into the same full frames"}

    def kind(self, which):
        return self.decoy if which == "A" else self.content

    def inputs(self, which):
        return dict({"x3": x3_bytes()[self.kind(which)], "off": offsets(self.kind(which))}, **self.tables(which))

    def tables(self, which):
        return {}

    def outputs(self):
        return dict({"so": 8 * (F0 + 1), "seg": 8 * NW}, **self.own_outputs())

    def prelude(self, x3, ctx, d):
        assert ctx.sample_offsets_dev(d["x3"], x3_len(), d["off"], F0, d["so"]) == 0
        assert ctx.seg_index_build_dev(d["x3"], x3_len(), d["off"], F0, x3.Params.default(), d["seg"], SB) == 0, ctx.last_error()
        return (d["x3"], x3_len(), d["off"], d["so"], F0, x3.Params.default())

    def expect(self, which):
        out, res = self.own_expect(which)
        return {"out": dict({"so": [(0, SO, False)], "seg": seg_segments(self.kind(which))}, **out), "result": res}

    def valid(self, which):
        offs = offsets(self.kind(which))
        assert int(offs[-1]) <= x3_len() and np.all(np.diff(offs.astype(np.int64)) >= 22) and offs.size == F0 + 1
        self.own_valid(which)

    def own_valid(self, which):
        pass


class LevelsCase(StreamCase):
    """x3_levels_dev (samples), x3_signal_levels_dev (diff) or x3_fir_levels_dev with the frame statuses: every record,
    d_frame_status and x3_levels_result.  ("last_levels_replays" is not compared: no reference computes it)"""

    def __init__(self, signal, damaged):
        self.name = "levels_%s%s" % (signal, "_damaged" if damaged else "")
        self.signal = signal
        self.content = "Bd" if damaged else "B"

    def own_outputs(self):
        return {"lv": 32 * NB, "fst": 4 * F0}

    def enqueue(self, x3, ctx, d, which, probe):
        src = self.prelude(x3, ctx, d)
        a = src + (BIN, d["lv"], NB, d["fst"], d["seg"], SB)
        if self.signal == "samples":
            rc = ctx.levels_dev(*a)
        elif self.signal in SIGNALS:
            rc = ctx.signal_levels_dev(*a, signal=SIGNALS[self.signal])
        else:
            rc = ctx.fir_levels_dev(*a, fir=fir_of(x3, self.signal))
        assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"levels": tuple(ctx.levels_result())}

    def own_expect(self, which):
        k = self.kind(which)
        st = stream(k)[1]
        return {"lv": [(0, stream_levels(k, self.signal), False)], "fst": [(0, st, False)]}, {"levels": summary(st)}


def stream_table(which, n=64, max_len=25_000):
    """64 ranges inside the stream: random ones, and around frame f0 (A and B: another frame, other lengths) a zero length, a
    range inside one block, ranges that begin on a frame's first position and one behind it (their history lies in the
    frame in front), one over more than three frames; the first and the last positions of the stream; around each
    content's failed frames ranges whose lead frame, whose middle and whose only frame fails"""
    rng = np.random.default_rng({"A": 51, "B": 62}[which])
    lens = rng.integers(1, 6000, size=n).astype(np.uint32)
    starts = np.array([rng.integers(0, N0 - int(k) + 1) for k in lens], dtype=np.uint64)
    f0, k = (11, 3) if which == "A" else (17, 5)
    bad = (AD_FRAME, AD_FRAME) if which == "A" else (9, 30)
    special = [(12_345 + k, 0), (N0, 0), (f0 * SPF + 1 + 20 * k + 3, 9 + k), (f0 * SPF, 5000 + k), (f0 * SPF, 1),
               (f0 * SPF + 1, 30 + k), (f0 * SPF - 700 - k, max_len - k), (0, 10 + k), (N0 - 3000 - k, 3000 + k),
               ((bad[0] + 1) * SPF, 2000 + k), ((bad[0] - 1) * SPF + 500, 12_000 + k), (bad[1] * SPF + 1, 50 + k),
               ((bad[1] + 1) * SPF + 1, 20 + k), ((bad[1] + 1) * SPF, 2)]
    at = rng.permutation(n)[:len(special)]
    for i, (s, ln) in zip(at, special):
        starts[i], lens[i] = s, ln
    return starts, lens


class RangeLevelsCase(StreamCase):
    """x3_range_levels_dev (samples), x3_signal_range_levels_dev (diff) or x3_fir_range_levels_dev, packed and then padded
    to a stride, over 64 ranges that differ between A and B: rows, row offsets, statuses and x3_range_levels_result"""
    W, STRIDE = 64, 40

    def __init__(self, signal, damaged=False):
        self.name = "range_levels_%s%s" % (signal, "_damaged" if damaged else "")
        self.signal = signal
        self.content = "Bd" if damaged else "B"
        self.cap = self.W * self.STRIDE

    def tables(self, which):
        s, n = stream_table(which, self.W, self.STRIDE * BIN - 700)
        return {"starts": s, "lens": n}

    def own_outputs(self):
        return {"rows1": 32 * self.cap, "off1": 8 * (self.W + 1), "st1": 4 * self.W, "rows2": 32 * self.cap, "st2": 4 * self.W}

    def enqueue(self, x3, ctx, d, which, probe):
        src = self.prelude(x3, ctx, d)
        for stride, rows, off, st in ((0, "rows1", d["off1"], "st1"), (self.STRIDE, "rows2", None, "st2")):
            a = src + (d["starts"], d["lens"], self.W, BIN, stride, d[rows], self.cap, off, d[st], d["seg"], SB)
            if self.signal == "samples":
                rc = ctx.range_levels_dev(*a)
            elif self.signal in SIGNALS:
                rc = ctx.signal_range_levels_dev(*a, signal=SIGNALS[self.signal])
            else:
                rc = ctx.fir_range_levels_dev(*a, fir=fir_of(x3, self.signal))
            assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"range_levels": tuple(ctx.range_levels_result())}

    def own_expect(self, which):
        starts, lens = stream_table(which, self.W, self.STRIDE * BIN - 700)
        fr = frames(self.kind(which))
        r1, off1, st1 = range_levels_of(fr, SO, starts, lens, BIN, 0, self.cap, self.signal)
        r2, _, st2 = range_levels_of(fr, SO, starts, lens, BIN, self.STRIDE, self.cap, self.signal)
        out = {"rows1": [(0, r1, False)], "off1": [(0, off1, False)], "st1": [(0, st1, False)], "rows2": [(0, r2, False)],
               "st2": [(0, st2, False)]}
        return out, {"range_levels": summary(st2) + (int(off1[-1]),)}

    def own_valid(self, which):
        starts, lens = stream_table(which, self.W, self.STRIDE * BIN - 700)
        assert all(int(s) + int(n) <= N0 for s, n in zip(starts, lens))
        rows = [RL.rows_of(n, BIN) for n in lens]
        assert max(rows) <= self.STRIDE and sum(rows) <= self.cap
        f = [(int(s) // SPF, (int(s) + int(n) - 1) // SPF) for s, n in zip(starts, lens) if n]
        assert (lens == 0).any() and any(b - a >= 3 for a, b in f) and any(int(s) % SPF == 0 and n for s, n in zip(starts, lens))
        at = [(int(s) % SPF, int(n)) for s, n in zip(starts, lens)]      # (sample i of a frame lies in block (i - 1) // 20)
        assert any(n and i and (i - 1) // 20 == (i + n - 2) // 20 for i, n in at)


# ---- from records: no decode; the inputs are the level records of the CPU reference and the word d_total points to.  A's
# total is one frame short, so that the totals differ too; the rows behind it are not A's to count.

TOTALS = {"A": N0 - SPF, "B": N0}
EV_CAP = 16
# join_bins 250: B's loud frames 5-6 and 20 (bins 78 .. 109 and 312 .. 327) are ONE run, which spans the tile edge at row
# 256: only x3_events_near_kernel's scan tells row 312 that row 109 is near.  A's loud frames (7, 31) stay two runs.
EVENTS_TILE = 256            # the option "events_tile_rows"
EV_RULE = E.Rule(mean_sq_min=200_000_000, join_bins=250, min_bins=2, pad_bins=1, max_bins=40)     # the white-noise frames
AD_RULE = E.Rule(join_bins=250, min_bins=2, pad_bins=1, max_bins=64)
TRULE = Q.TRule(peak=(900_000, 3, 2, 5), mean_sq=(500_000, 16, 1, 0))
TRULE_M = Q.TRule(mean_sq=(500_000, 16, 1, 0))                                                  # 12 dB over the median
Q_PPM = [100_000, 500_000, 990_000]
THR_DTYPE = np.dtype([("mean_sq_min", "<u8"), ("peak_min", "<u4"), ("counted", "<u4")])


def thr_records(thrs):
    a = np.zeros(len(thrs), dtype=THR_DTYPE)
    for i, t in enumerate(thrs):
        a[i] = t
    return a


def event_rule(x3, rule):
    return x3.EventRule.make(*rule)


def threshold_rule(x3, trule):
    return x3.ThresholdRule.make(trule.peak, trule.mean_sq)


def slot_outputs(cap, with_entries=False):
    o = {"ev_st": 8 * cap, "ev_ln": 4 * cap, "ev_lv": 32 * cap, "cnt": 8}
    if with_entries:
        o["ev_ent"] = 4 * cap
    return o


def slot_expect(ev, elv, cap, with_entries=False):
    ent, st, ln, lv = E.slots(ev, elv, cap, with_entries)
    out = {"ev_st": [(0, st, False)], "ev_ln": [(0, ln, False)], "ev_lv": [(0, lv, False)], "cnt": [(0, word(len(ev)), False)]}
    if with_entries:
        out["ev_ent"] = [(0, ent, False)]
    return out


def spans_a_tile_edge(events, bin_len, first_rows=None):
    """True when consecutive pieces of one run (they adjoin) cover rows on both sides of a multiple of EVENTS_TILE with at
    least two rows on either side (one may be padding): the run's hot rows lie in two tiles of the events kernels"""
    spans = []
    for ev in events:
        base = int(first_rows[ev[0]]) if first_rows is not None else 0
        a, b = base + ev[-2] // bin_len, base + -(-(ev[-2] + ev[-1]) // bin_len)
        if spans and spans[-1][1] == a:
            spans[-1][1] = b
        else:
            spans.append([a, b])
    return any(a <= k - 2 and k + 2 <= b for a, b in spans for k in range(EVENTS_TILE, b, EVENTS_TILE))


def empty_summary(counted):
    empty = [e for e, k in enumerate(counted) if k == 0]
    return (0, len(empty), empty[0] if empty else len(counted))


class RecordsCase(AC.Case):
    signal = "samples"

    def records(self, which):
        return stream_levels("Ad" if which == "A" else "B", self.signal)

    def inputs(self, which):
        return {"lv": u8(self.records(which)), "tot": word(TOTALS[which])}

    def valid(self, which):
        assert self.records(which).size == NB and TOTALS[which] <= N0


class EventsFromRecords(RecordsCase):
    """x3_events_dev with a join / pad / min / max rule: all cap slots, the count and x3_events_result"""
    name = "events_from_records"

    def outputs(self):
        return slot_outputs(EV_CAP)

    def enqueue(self, x3, ctx, d, which, probe):
        assert ctx.events_dev(d["lv"], NB, BIN, d["tot"], event_rule(x3, EV_RULE), d["ev_st"], d["ev_ln"], d["ev_lv"], EV_CAP,
                              d["cnt"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"events": tuple(ctx.events_result())}

    def events(self, which):
        return E.stream_events(self.records(which), TOTALS[which], BIN, EV_RULE)

    def expect(self, which):
        ev, elv = self.events(which)
        return {"out": slot_expect(ev, elv, EV_CAP), "result": {"events": (0, len(ev))}}

    def counts(self):
        return len(self.events("A")[0]), len(self.events("B")[0]), EV_CAP, 5

    def b_events(self):
        return self.events("B")[0], BIN, None


class QuantilesFromRecords(RecordsCase):
    """x3_level_quantiles_dev with three quantiles for either key, then x3_level_thresholds_dev of both criteria"""
    name = "quantiles_from_records"
    signal = "diff"
    same_ok = {"empty": NONE_EMPTY}

    def outputs(self):
        return {"v_peak": 4 * 3, "k_peak": 4, "v_msq": 4 * 3, "k_msq": 4, "thr": 16}

    def enqueue(self, x3, ctx, d, which, probe):
        for key, v, k in ((x3.LEVEL_KEY_PEAK, "v_peak", "k_peak"), (x3.LEVEL_KEY_MEAN_SQ, "v_msq", "k_msq")):
            assert ctx.level_quantiles_dev(d["lv"], NB, BIN, d["tot"], key, Q_PPM, d[v], d[k]) == 0, ctx.last_error()
        assert ctx.level_thresholds_dev(d["lv"], NB, BIN, d["tot"], threshold_rule(x3, TRULE), d["thr"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"empty": tuple(ctx.level_quantiles_result())}

    def expect(self, which):
        lv, tot = self.records(which), TOTALS[which]
        vp, kp = Q.stream_quantiles(lv, tot, BIN, Q.PEAK, Q_PPM)
        vm, km = Q.stream_quantiles(lv, tot, BIN, Q.MEAN_SQ, Q_PPM)
        thr = Q.stream_thresholds(lv, tot, BIN, TRULE)
        out = {"v_peak": [(0, vp, False)], "k_peak": [(0, kp, False)], "v_msq": [(0, vm, False)], "k_msq": [(0, km, False)],
               "thr": [(0, thr_records(thr), False)]}
        return {"out": out, "result": {"empty": empty_summary([t[2] for t in thr])}}


class AdaptiveFromRecords(RecordsCase):
    """x3_level_thresholds_dev, then x3_events_adaptive_dev on its record"""
    name = "adaptive_from_records"
    signal = "fir3"
    same_ok = {"empty": NONE_EMPTY}

    def outputs(self):
        return dict(slot_outputs(EV_CAP), thr=16)

    def enqueue(self, x3, ctx, d, which, probe):
        assert ctx.level_thresholds_dev(d["lv"], NB, BIN, d["tot"], threshold_rule(x3, TRULE_M), d["thr"]) == 0, ctx.last_error()
        assert ctx.events_adaptive_dev(d["lv"], NB, BIN, d["tot"], event_rule(x3, AD_RULE), d["thr"], d["ev_st"], d["ev_ln"],
                                       d["ev_lv"], EV_CAP, d["cnt"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"empty": tuple(ctx.level_quantiles_result()), "events": tuple(ctx.events_result())}

    def events(self, which):
        lv, tot = self.records(which), TOTALS[which]
        thr = Q.stream_thresholds(lv, tot, BIN, TRULE_M)
        return Q.stream_adaptive_events(lv, tot, BIN, thr[0], AD_RULE) + (thr,)

    def expect(self, which):
        ev, elv, thr = self.events(which)
        return {"out": dict(slot_expect(ev, elv, EV_CAP), thr=[(0, thr_records(thr), False)]),
                "result": {"empty": empty_summary([t[2] for t in thr]), "events": (0, len(ev))}}

    def counts(self):
        return len(self.events("A")[0]), len(self.events("B")[0]), EV_CAP, 3

    def b_events(self):
        return self.events("B")[0], BIN, None


# ---- the stream chain

CH_CAP = 8
CH_FINE = 97                                        # the second look's bin
CH_ROWS = CH_CAP * RL.rows_of(AD_RULE.max_bins * BIN, CH_FINE)
CH_OUT = CH_CAP * AD_RULE.max_bins * BIN


@functools.lru_cache(maxsize=None)
def stream_chain_ref(kind, signal="fir3"):
    """levels -> thresholds -> adaptive events -> FIR range levels and ranges of the events' slots, fillers included"""
    lv = stream_levels(kind, signal)
    thr = Q.stream_thresholds(lv, N0, BIN, TRULE_M)
    ev, elv = Q.stream_adaptive_events(lv, N0, BIN, thr[0], AD_RULE)
    _, starts, lens, _ = E.slots(ev, elv, CH_CAP, False)
    rl = range_levels_of(frames(kind), SO, starts, lens, CH_FINE, 0, CH_ROWS, signal)
    rg = RR.ranges(frames(kind), SO, starts, lens, 0, CH_OUT, CANARY16)
    return lv, thr, ev, elv, rl, rg


class StreamChain(StreamCase):
    """sample offsets, index, x3_fir_levels_dev, x3_level_thresholds_dev, x3_events_adaptive_dev, x3_fir_range_levels_dev and
    x3_decode_ranges_dev on the events' arrays as they are: nothing is waited for in between, every intermediate buffer is
    compared, and the five result calls are read behind the wait, each its own call's"""
    name = "stream_chain"
    same_ok = dict(StreamCase.same_ok, empty=NONE_EMPTY)

    def own_outputs(self):
        return dict(slot_outputs(CH_CAP), lv=32 * NB, fst=4 * F0, thr=16, rl=32 * CH_ROWS, rl_off=8 * (CH_CAP + 1),
                    rl_st=4 * CH_CAP, rg=2 * CH_OUT, rg_off=8 * (CH_CAP + 1), rg_st=4 * CH_CAP)

    def enqueue(self, x3, ctx, d, which, probe):
        src = self.prelude(x3, ctx, d)
        fir, tot = fir_of(x3, "fir3"), d["so"] + 8 * F0
        assert ctx.fir_levels_dev(*src, BIN, d["lv"], NB, d["fst"], d["seg"], SB, fir=fir) == 0, ctx.last_error()
        assert ctx.level_thresholds_dev(d["lv"], NB, BIN, tot, threshold_rule(x3, TRULE_M), d["thr"]) == 0, ctx.last_error()
        assert ctx.events_adaptive_dev(d["lv"], NB, BIN, tot, event_rule(x3, AD_RULE), d["thr"], d["ev_st"], d["ev_ln"],
                                       d["ev_lv"], CH_CAP, d["cnt"]) == 0, ctx.last_error()
        assert ctx.fir_range_levels_dev(*src, d["ev_st"], d["ev_ln"], CH_CAP, CH_FINE, 0, d["rl"], CH_ROWS, d["rl_off"],
                                        d["rl_st"], d["seg"], SB, fir=fir) == 0, ctx.last_error()
        assert ctx.decode_ranges_dev(*src, d["ev_st"], d["ev_ln"], CH_CAP, 0, d["rg"], CH_OUT, x3.WINDOW_I16, d["rg_off"],
                                     d["rg_st"], d["seg"], SB) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"ranges": tuple(ctx.decode_ranges_result()), "range_levels": tuple(ctx.range_levels_result()),
                "events": tuple(ctx.events_result()), "empty": tuple(ctx.level_quantiles_result()),
                "levels": tuple(ctx.levels_result())}

    def own_expect(self, which):
        k = self.kind(which)
        lv, thr, ev, elv, (rl, rl_off, rl_st), (rg, rg_off, rg_st) = stream_chain_ref(k)
        out = dict(slot_expect(ev, elv, CH_CAP), lv=[(0, lv, False)], fst=[(0, stream(k)[1], False)],
                   thr=[(0, thr_records(thr), False)], rl=[(0, rl, False)], rl_off=[(0, rl_off, False)], rl_st=[(0, rl_st, False)],
                   rg=[(0, rg, False)], rg_off=[(0, rg_off, False)], rg_st=[(0, rg_st, False)])
        res = {"levels": summary(stream(k)[1]), "empty": empty_summary([t[2] for t in thr]), "events": (0, len(ev)),
               "range_levels": summary(rl_st) + (int(rl_off[-1]),), "ranges": summary(rg_st) + (int(rg_off[-1]),)}
        return out, res

    def counts(self):
        return len(stream_chain_ref("Ad")[2]), len(stream_chain_ref("B")[2]), CH_CAP, 3

    def b_events(self):
        return stream_chain_ref("B")[2], BIN, None


# ------------------------------------------------------------------------------------------------ corpus content

C_BL, C_BPF, C_SPF = 20, 50, 1000
ENTRY_SAMPLES = AC.ENTRY_SAMPLES
NE = len(ENTRY_SAMPLES)
LOUD_ENTRY = 4
C_GAINS = (1, 4, 16, 2, 0, 8)
C_BURSTS = ([(3_200, 600), (17_100, 800)], [(2_300, 500), (8_150, 700)], [(1_100, 700), (14_200, 600), (26_050, 900)],
            [(4_400, 500), (10_100, 800)], [(7_000, 1_000)], [(6_250, 600), (12_100, 650), (15_300, 500)])
C_BIN = 130                                          # divides neither the frame (1 000) nor the block
C_FINE = 37
C_CAP = 24
C_EV_RULE = E.Rule(mean_sq_min=1000, join_bins=2, min_bins=2, pad_bins=1, max_bins=40)
C_AD_RULE = E.Rule(join_bins=2, min_bins=2, pad_bins=1, max_bins=20)


def c_oparams():
    return O.Params.make(C_BL, C_BPF, (0, 1, 3), (3, 8, 20))


def c_params(x3):
    return x3.Params.make(C_BL, C_BPF)


@functools.lru_cache(maxsize=None)
def corpus_wavs():
    out = []
    for e, n in enumerate(ENTRY_SAMPLES):
        rng = np.random.default_rng(500 + e)
        if e == LOUD_ENTRY:
            w = rng.integers(-32768, 32768, size=n).astype(np.int16)
        else:
            w = rng.integers(-8, 9, size=n).astype(np.int32)
            for a, ln in C_BURSTS[e]:
                assert a // C_SPF == (a + ln - 1) // C_SPF          # a burst lies inside one frame
                w[a:a + ln] = (100 * C_GAINS[e] * np.sin(np.arange(ln) * 0.37)).astype(np.int32)
            w = w.astype(np.int16)
        w.setflags(write=False)
        out.append(w)
    return out


def damaged_frame(e):
    """the frame of entry e that fails in the decoy: the one that holds its first burst"""
    return C_BURSTS[e][0][0] // C_SPF


@functools.lru_cache(maxsize=None)
def corpus_content(which):
    """-> (buffer with 16 bytes of slack, entry offsets, entry lengths, frame offsets in the buffer [F + 1],
    per entry (frames, statuses, sample offsets relative to the entry [n + 1]))"""
    parts, ents, foffs, pos = [], [], [], 0
    for e, w in enumerate(corpus_wavs()):
        rc, s, _ = O.encode(w, c_oparams())
        assert rc == 0
        offs = frame_offsets(s) + [s.size]
        nf = len(offs) - 1
        assert nf == -(-w.size // C_SPF)
        st = np.zeros(nf, dtype=np.int32)
        if which == "A":
            f = damaged_frame(e)
            s = s.copy()
            s[offs[f] + 20 + 40] ^= 0x04
            st[f] = CRC
        parts.append(s)
        foffs += [pos + o for o in offs[:-1]]
        pos += s.size
        so = np.minimum(np.arange(nf + 1, dtype=np.uint64) * np.uint64(C_SPF), np.uint64(w.size))
        ents.append(([w[f * C_SPF:(f + 1) * C_SPF] for f in range(nf)], st, so))
    lens = [int(s.size) for s in parts]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    buf = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
    return buf, offs, lens, np.array(foffs + [pos], dtype=np.uint64), ents


def c_frames(which, e):
    fr, st, _ = corpus_content(which)[4][e]
    return [(int(s), w if s == 0 else None) for s, w in zip(st, fr)]


def c_statuses(which):
    return np.concatenate([st for _, st, _ in corpus_content(which)[4]])


@functools.lru_cache(maxsize=None)
def corpus_levels(which, signal, bin_len=C_BIN):
    """-> (LEVEL_DTYPE [rows], row_first)"""
    rf = L.corpus_row_first(ENTRY_SAMPLES, bin_len)
    out = L.empty(int(rf[-1]))
    for e, (fr, st, so) in enumerate(corpus_content(which)[4]):
        a, b = int(rf[e]), int(rf[e + 1])
        out[a:b] = levels_of(fr, st, so[:-1], bin_len, b - a, signal)
    out.setflags(write=False)
    return out, rf


C_ROWS = int(L.corpus_row_first(ENTRY_SAMPLES, C_BIN)[-1])


def per_entry(fn, which, ent, span):
    """a corpus call's arrays from the stream reference on each entry alone: fn(frames, sample offsets) -> (out [cap, ...],
    offsets, statuses) over ALL ranges; range w takes its rows (span(w) elements at its offset) and status from entry ent[w]"""
    assert int(np.max(ent)) < NE
    out = off = st = None
    for e in range(NE):
        o, f, s = fn(c_frames(which, e), corpus_content(which)[4][e][2])
        if out is None:
            out, off, st = o.copy(), f, s.copy()
        for w in np.flatnonzero(np.asarray(ent) == e):
            a = int(f[w])
            out[a:a + span(w)] = o[a:a + span(w)]
            st[w] = s[w]
    return out, off, st


class CorpusCase(AC.Case):
    """a corpus over the harness's work buffer "x3", built in the warm-up pass's first enqueue: the clean bytes go up with
    the upload that waits, x3_corpus_build (synchronous) walks them, the decoy is put back"""
    corpus = None
    own_buffer = False          # the cases that decode nothing keep the corpus's bytes in a buffer of their own

    def inputs(self, which):
        i = {} if self.own_buffer else {"x3": corpus_content(which)[0]}
        return dict(i, **self.tables(which))

    def tables(self, which):
        return {}

    def corpus_of(self, x3, ctx, d):
        if self.corpus is None:
            buf, offs, lens = corpus_content("B")[:3]
            self.ctx, self.d_own = ctx, None
            if self.own_buffer:
                self.d_own = ctx.alloc(buf.size)
            ptr = self.d_own or d["x3"]
            ctx.upload(ptr, buf)
            self.corpus = x3.Corpus(ctx, (ptr, buf.size - 16), offs, lens, c_params(x3), seg_blocks=SB)
            assert self.corpus.entries["n_samples"].tolist() == list(ENTRY_SAMPLES)
            assert self.corpus.n_frames == corpus_content("B")[3].size - 1
            if not self.own_buffer:
                ctx.upload(ptr, corpus_content("A")[0])
        return self.corpus

    def cleanup(self):
        if self.corpus is not None:
            self.corpus.close()
            if self.d_own:
                self.ctx.free(self.d_own)
            self.corpus = None

    def valid(self, which):
        buf, offs, lens, foffs, ents = corpus_content(which)
        b = corpus_content("B")
        assert buf.size == b[0].size and offs == b[1] and lens == b[2] and np.array_equal(foffs, b[3])
        assert all(12 <= len(fr) <= 30 for fr, _, _ in ents)
        self.own_valid(which)

    def own_valid(self, which):
        pass


class CorpusLevels(CorpusCase):
    """x3_corpus_levels_dev (samples), x3_corpus_signal_levels_dev (diff) or x3_corpus_fir_levels_dev"""

    def __init__(self, signal):
        self.name = "corpus_levels_" + signal
        self.signal = signal

    def outputs(self):
        return {"lv": 32 * C_ROWS, "fst": 4 * c_statuses("B").size}

    def enqueue(self, x3, ctx, d, which, probe):
        k = self.corpus_of(x3, ctx, d)
        if self.signal == "samples":
            rc = ctx.corpus_levels_dev(k, C_BIN, d["lv"], C_ROWS, d["fst"])
        elif self.signal in SIGNALS:
            rc = ctx.corpus_signal_levels_dev(k, C_BIN, d["lv"], C_ROWS, d["fst"], SIGNALS[self.signal])
        else:
            rc = ctx.corpus_fir_levels_dev(k, C_BIN, d["lv"], C_ROWS, d["fst"], fir_of(x3, self.signal))
        assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"levels": tuple(ctx.levels_result())}

    def expect(self, which):
        st = c_statuses(which)
        return {"out": {"lv": [(0, corpus_levels(which, self.signal)[0], False)], "fst": [(0, st, False)]},
                "result": {"levels": summary(st)}}


class CorpusRecordsCase(CorpusCase):
    own_buffer = True
    signal = "samples"

    def records(self, which):
        return corpus_levels(which, self.signal)[0]

    def tables(self, which):
        return {"lv": u8(self.records(which))}

    def own_valid(self, which):
        assert self.records(which).size == C_ROWS


class CorpusEventsFromRecords(CorpusRecordsCase):
    """x3_corpus_events_dev: entries, starts, lens, merged records, the count"""
    name = "corpus_events_from_records"

    def outputs(self):
        return slot_outputs(C_CAP, True)

    def enqueue(self, x3, ctx, d, which, probe):
        k = self.corpus_of(x3, ctx, d)
        assert ctx.corpus_events_dev(k, d["lv"], C_ROWS, C_BIN, event_rule(x3, C_EV_RULE), d["ev_ent"], d["ev_st"], d["ev_ln"],
                                     d["ev_lv"], C_CAP, d["cnt"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"events": tuple(ctx.events_result())}

    def events(self, which):
        return E.corpus_events(self.records(which), ENTRY_SAMPLES, C_BIN, C_EV_RULE)

    def expect(self, which):
        ev, elv = self.events(which)
        return {"out": slot_expect(ev, elv, C_CAP, True), "result": {"events": (0, len(ev))}}

    def counts(self):
        return len(self.events("A")[0]), len(self.events("B")[0]), C_CAP, 5

    def b_events(self):
        return self.events("B")[0], C_BIN, L.corpus_row_first(ENTRY_SAMPLES, C_BIN)


def corpus_adaptive_ref(lv, trule, rule):
    thr = Q.corpus_thresholds(lv, ENTRY_SAMPLES, C_BIN, trule)
    return Q.corpus_adaptive_events(lv, ENTRY_SAMPLES, C_BIN, thr, rule) + (thr,)


class CorpusAdaptiveFromRecords(CorpusRecordsCase):
    """x3_corpus_level_thresholds_dev, then x3_corpus_events_adaptive_dev on its records"""
    name = "corpus_adaptive_from_records"
    same_ok = {"empty": NONE_EMPTY}

    def outputs(self):
        return dict(slot_outputs(C_CAP, True), thr=16 * NE)

    def enqueue(self, x3, ctx, d, which, probe):
        k = self.corpus_of(x3, ctx, d)
        assert ctx.corpus_level_thresholds_dev(k, d["lv"], C_ROWS, C_BIN, threshold_rule(x3, TRULE_M), d["thr"]) == 0
        assert ctx.corpus_events_adaptive_dev(k, d["lv"], C_ROWS, C_BIN, event_rule(x3, C_AD_RULE), d["thr"], d["ev_ent"],
                                              d["ev_st"], d["ev_ln"], d["ev_lv"], C_CAP, d["cnt"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"empty": tuple(ctx.level_quantiles_result()), "events": tuple(ctx.events_result())}

    def events(self, which):
        return corpus_adaptive_ref(self.records(which), TRULE_M, C_AD_RULE)

    def expect(self, which):
        ev, elv, thr = self.events(which)
        return {"out": dict(slot_expect(ev, elv, C_CAP, True), thr=[(0, thr_records(thr), False)]),
                "result": {"empty": empty_summary([t[2] for t in thr]), "events": (0, len(ev))}}

    def counts(self):
        return len(self.events("A")[0]), len(self.events("B")[0]), C_CAP, 5

    def b_events(self):
        return self.events("B")[0], C_BIN, L.corpus_row_first(ENTRY_SAMPLES, C_BIN)


def corpus_table(which, n=64, max_len=5000):
    """(entries, starts, lens) inside the entries: random ones, and in entry e0 (A and B: another entry and frame) a zero
    length, a range inside one block, ranges on a frame's first position and one behind it, one over more than three
    frames, the entry's first and last positions, a range led by the frame that fails in the decoy"""
    rng = np.random.default_rng({"A": 73, "B": 84}[which])
    ent = rng.integers(0, NE, size=n).astype(np.uint32)
    lens = np.array([rng.integers(1, min(max_len, ENTRY_SAMPLES[e]) + 1) for e in ent], dtype=np.uint32)
    starts = np.array([rng.integers(0, ENTRY_SAMPLES[e] - int(k) + 1) for e, k in zip(ent, lens)], dtype=np.uint64)
    e0, f0, k = (2, 9, 2) if which == "A" else (0, 13, 4)
    bad = damaged_frame(e0)
    ne = ENTRY_SAMPLES[e0]
    special = [(e0, 777 + k, 0), (e0, ne, 0), (e0, f0 * C_SPF + 1 + 20 * k + 3, 9 + k), (e0, f0 * C_SPF, 1500 + k),
               (e0, f0 * C_SPF, 1), (e0, f0 * C_SPF + 1, 30 + k), (e0, f0 * C_SPF - 70 - k, 3500 + k), (e0, 0, 10 + k),
               (e0, ne - 300 - k, 300 + k), (e0, (bad + 1) * C_SPF, 200 + k), (e0, (bad + 1) * C_SPF + 1, 20 + k),
               (e0, (bad - 1) * C_SPF + 50, 2500 + k), (LOUD_ENTRY, 6_500 + k, 3000), (5, 16_999 - k, 1 + k)]
    at = rng.permutation(n)[:len(special)]
    for i, (e, s, ln) in zip(at, special):
        ent[i], starts[i], lens[i] = e, s, ln
    return ent, starts, lens


class CorpusTableCase(CorpusCase):
    W = 64
    MAX_LEN = 5000

    def tables(self, which):
        e, s, n = corpus_table(which, self.W, self.MAX_LEN)
        return {"ent": e, "starts": s, "lens": n}

    def own_valid(self, which):
        ent, starts, lens = corpus_table(which, self.W, self.MAX_LEN)
        assert int(ent.max()) < NE and all(int(s) + int(n) <= ENTRY_SAMPLES[e] for e, s, n in zip(ent, starts, lens))
        assert int(lens.max()) <= self.MAX_LEN and (lens == 0).any()
        assert any(n and (int(s) + int(n) - 1) // C_SPF - int(s) // C_SPF >= 3 for s, n in zip(starts, lens))


class CorpusRangeLevels(CorpusTableCase):
    """x3_corpus_range_levels_dev (samples) or x3_corpus_fir_range_levels_dev, packed and then padded"""
    STRIDE = 40

    def __init__(self, signal):
        self.name = "corpus_range_levels_" + signal
        self.signal = signal
        self.cap = self.W * self.STRIDE

    def outputs(self):
        return {"rows1": 32 * self.cap, "off1": 8 * (self.W + 1), "st1": 4 * self.W, "rows2": 32 * self.cap, "st2": 4 * self.W}

    def enqueue(self, x3, ctx, d, which, probe):
        k = self.corpus_of(x3, ctx, d)
        for stride, rows, off, st in ((0, "rows1", d["off1"], "st1"), (self.STRIDE, "rows2", None, "st2")):
            a = (k, d["ent"], d["starts"], d["lens"], self.W, C_BIN, stride, d[rows], self.cap, off, d[st])
            if self.signal == "samples":
                rc = ctx.corpus_range_levels_dev(*a)
            else:
                rc = ctx.corpus_fir_range_levels_dev(*a, fir=fir_of(x3, self.signal))
            assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"range_levels": tuple(ctx.range_levels_result())}

    def expect(self, which):
        ent, starts, lens = corpus_table(which, self.W, self.MAX_LEN)
        r1, off1, st1 = per_entry(lambda fr, so: range_levels_of(fr, so, starts, lens, C_BIN, 0, self.cap, self.signal),
                                  which, ent, lambda w: RL.rows_of(lens[w], C_BIN))
        r2, _, st2 = per_entry(lambda fr, so: range_levels_of(fr, so, starts, lens, C_BIN, self.STRIDE, self.cap, self.signal),
                               which, ent, lambda w: self.STRIDE)
        out = {"rows1": [(0, r1, False)], "off1": [(0, off1, False)], "st1": [(0, st1, False)], "rows2": [(0, r2, False)],
               "st2": [(0, st2, False)]}
        return {"out": out, "result": {"range_levels": summary(st2) + (int(off1[-1]),)}}

    def own_valid(self, which):
        CorpusTableCase.own_valid(self, which)
        rows = [RL.rows_of(n, C_BIN) for n in corpus_table(which, self.W, self.MAX_LEN)[2]]
        assert max(rows) <= self.STRIDE and sum(rows) <= self.cap


class CorpusRangesPair(CorpusTableCase):
    """x3_corpus_ranges_dev packed (int16), then padded (float32)"""
    name = "corpus_ranges_pair"
    STRIDE = 5000

    def __init__(self):
        self.cap = self.W * self.STRIDE

    def outputs(self):
        return {"rows1": 2 * self.cap, "off1": 8 * (self.W + 1), "st1": 4 * self.W, "rows2": 4 * self.cap, "st2": 4 * self.W}

    def enqueue(self, x3, ctx, d, which, probe):
        k = self.corpus_of(x3, ctx, d)
        a = (ctx._h, k._h, d["ent"], d["starts"], d["lens"], self.W)
        assert x3.lib().x3_corpus_ranges_dev(*a, 0, d["rows1"], self.cap, x3.WINDOW_I16, d["off1"], d["st1"]) == 0, ctx.last_error()
        assert x3.lib().x3_corpus_ranges_dev(*a, self.STRIDE, d["rows2"], self.cap, x3.WINDOW_F32, None, d["st2"]) == 0

    def results(self, x3, ctx, d, which):
        return {"ranges": tuple(ctx.decode_ranges_result())}

    def expect(self, which):
        ent, starts, lens = corpus_table(which, self.W, self.MAX_LEN)
        r1, off1, st1 = per_entry(lambda fr, so: RR.ranges(fr, so, starts, lens, 0, self.cap, CANARY16), which, ent,
                                  lambda w: int(lens[w]))
        r2, _, st2 = per_entry(lambda fr, so: RR.ranges(fr, so, starts, lens, self.STRIDE, self.cap, CANARY16), which, ent,
                               lambda w: self.STRIDE)
        out = {"rows1": [(0, r1, False)], "off1": [(0, off1, False)], "st1": [(0, st1, False)],
               "rows2": [(0, AC.f32_bits(r2), False)], "st2": [(0, st2, False)]}
        return {"out": out, "result": {"ranges": summary(st2) + (int(off1[-1]),)}}


# ---- the corpus chain; test_two_threads_two_contexts_one_corpus runs the same calls with other taps and rules

C_ROWS_FINE = C_CAP * RL.rows_of(C_AD_RULE.max_bins * C_BIN, C_FINE)
C_OUT = C_CAP * C_AD_RULE.max_bins * C_BIN
CHAIN_OUTPUTS = dict(slot_outputs(C_CAP, True), lv=32 * C_ROWS, thr=16 * NE, rl=32 * C_ROWS_FINE, rl_off=8 * (C_CAP + 1),
                     rl_st=4 * C_CAP, rg=2 * C_OUT, rg_off=8 * (C_CAP + 1), rg_st=4 * C_CAP)


@functools.lru_cache(maxsize=None)
def corpus_chain_ref(which, signal, trule):
    lv = corpus_levels(which, signal)[0]
    ev, elv, thr = corpus_adaptive_ref(lv, trule, C_AD_RULE)
    ent, starts, lens, _ = E.slots(ev, elv, C_CAP, True)
    rl = per_entry(lambda fr, so: range_levels_of(fr, so, starts, lens, C_FINE, 0, C_ROWS_FINE, signal), which, ent,
                   lambda w: RL.rows_of(lens[w], C_FINE))
    rg = per_entry(lambda fr, so: RR.ranges(fr, so, starts, lens, 0, C_OUT, CANARY16), which, ent, lambda w: int(lens[w]))
    return lv, thr, ev, elv, rl, rg


def corpus_chain_enqueue(x3, ctx, k, d, signal, trule, d_fst=None):
    """x3_corpus_fir_levels_dev, x3_corpus_level_thresholds_dev, x3_corpus_events_adaptive_dev, x3_corpus_fir_range_levels_dev
    and x3_corpus_ranges_dev on the events' arrays as they are, on context `ctx` (the corpus may be another context's)"""
    fir = fir_of(x3, signal)
    assert ctx.corpus_fir_levels_dev(k, C_BIN, d["lv"], C_ROWS, d_fst, fir) == 0, ctx.last_error()
    assert ctx.corpus_level_thresholds_dev(k, d["lv"], C_ROWS, C_BIN, threshold_rule(x3, trule), d["thr"]) == 0, ctx.last_error()
    assert ctx.corpus_events_adaptive_dev(k, d["lv"], C_ROWS, C_BIN, event_rule(x3, C_AD_RULE), d["thr"], d["ev_ent"], d["ev_st"],
                                          d["ev_ln"], d["ev_lv"], C_CAP, d["cnt"]) == 0, ctx.last_error()
    assert ctx.corpus_fir_range_levels_dev(k, d["ev_ent"], d["ev_st"], d["ev_ln"], C_CAP, C_FINE, 0, d["rl"], C_ROWS_FINE,
                                           d["rl_off"], d["rl_st"], fir=fir) == 0, ctx.last_error()
    assert x3.lib().x3_corpus_ranges_dev(ctx._h, k._h, d["ev_ent"], d["ev_st"], d["ev_ln"], C_CAP, 0, d["rg"], C_OUT,
                                         x3.WINDOW_I16, d["rg_off"], d["rg_st"]) == 0, ctx.last_error()


def corpus_chain_results(ctx):
    return {"ranges": tuple(ctx.decode_ranges_result()), "range_levels": tuple(ctx.range_levels_result()),
            "events": tuple(ctx.events_result()), "empty": tuple(ctx.level_quantiles_result()),
            "levels": tuple(ctx.levels_result())}


def corpus_chain_expect(which, signal, trule):
    """-> ({output: array}, {result key: value})"""
    lv, thr, ev, elv, (rl, rl_off, rl_st), (rg, rg_off, rg_st) = corpus_chain_ref(which, signal, trule)
    out = {k: v[0][1] for k, v in slot_expect(ev, elv, C_CAP, True).items()}
    out.update(lv=lv, thr=thr_records(thr), rl=rl, rl_off=rl_off, rl_st=rl_st, rg=rg, rg_off=rg_off, rg_st=rg_st)
    res = {"levels": summary(c_statuses(which)), "empty": empty_summary([t[2] for t in thr]), "events": (0, len(ev)),
           "range_levels": summary(rl_st) + (int(rl_off[-1]),), "ranges": summary(rg_st) + (int(rg_off[-1]),)}
    return out, res


class CorpusChain(CorpusCase):
    """the stream chain's steps 3-7 in their corpus forms, nothing waited for in between"""
    name = "corpus_chain"
    SIGNAL = "fir4"
    same_ok = {"empty": NONE_EMPTY, "rl_st": CLEAN_RANGES, "rg_st": CLEAN_RANGES}

    def outputs(self):
        return dict(CHAIN_OUTPUTS, fst=4 * c_statuses("B").size)

    def enqueue(self, x3, ctx, d, which, probe):
        corpus_chain_enqueue(x3, ctx, self.corpus_of(x3, ctx, d), d, self.SIGNAL, TRULE_M, d["fst"])

    def results(self, x3, ctx, d, which):
        return corpus_chain_results(ctx)

    def expect(self, which):
        out, res = corpus_chain_expect(which, self.SIGNAL, TRULE_M)
        out["fst"] = c_statuses(which)
        return {"out": {k: [(0, v, False)] for k, v in out.items()}, "result": res}

    def counts(self):
        return len(corpus_chain_ref("A", self.SIGNAL, TRULE_M)[2]), len(corpus_chain_ref("B", self.SIGNAL, TRULE_M)[2]), C_CAP, 3

    def b_events(self):
        return corpus_chain_ref("B", self.SIGNAL, TRULE_M)[2], C_BIN, L.corpus_row_first(ENTRY_SAMPLES, C_BIN)


CASES = ([LevelsCase(s, dmg) for s in ("samples", "diff", "fir3", "fir8") for dmg in (False, True)] +
         [RangeLevelsCase(s) for s in ("samples", "diff", "fir3")] + [RangeLevelsCase("fir3", damaged=True)] +
         [EventsFromRecords(), QuantilesFromRecords(), AdaptiveFromRecords(), StreamChain()] +
         [CorpusLevels(s) for s in ("samples", "diff", "fir3")] + [CorpusEventsFromRecords(), CorpusAdaptiveFromRecords()] +
         [CorpusRangeLevels(s) for s in ("samples", "fir3")] + [CorpusRangesPair(), CorpusChain()])

# what same_ok may name: statuses of clean content, totals that are equal by construction (NONE_EMPTY), the sample offsets
SAME_OK_ALLOWED = {"so", "empty", "rl_st", "rg_st"}
