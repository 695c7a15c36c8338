"""The exact-fit cases of the random-access and analysis calls under guard pages (not a test module).

tests/test_gpu_fence_analysis.py runs every case in a child under X3HIP_FENCE=16, X3HIP_FENCE_FILL=165 and
X3HIP_FENCE_TIGHT=1 (x3-rust_amd/csrc/x3_fence.h): every device buffer of a case comes from Context.alloc with EXACTLY the
bytes include/x3hip.h asks for, so it ends (rounded up to 16 bytes) where its mapping ends, and an access a few bytes or a
few records behind it is a memory fault at once.  Every output is compared with == as well; what no call may write keeps the
fill.  The tables and their expectations are made here from the CPU references of tests/ and the oracle alone (no GPU);
tests/test_fence_cases.py checks on the CPU that the cases are what they are meant to be.

Streams: block length 20, 7 and 100 blocks a frame, k = 1 .. 3 full frames and ONE sample, so the last frame is 22 bytes, a
header and one raw sample, and the stream's last byte is the buffer's.
    "m16"  the size is a multiple of 16: the last frame ends on a chunk boundary (the shape of the one fault a soak hit)
    "m2"   the size is 2 mod 16: the last chunk holds two bytes of the stream and 14 behind it, the widest over-read a stream
           can bring about -- the encoder pads every payload to whole 16-bit words, so no stream has an odd size and
           1 mod 16 does not exist
    "crc"  one payload byte of the last FULL frame flipped: a status other than 0 on the path, and the one-sample frame's
           lead frame (the history of the difference and the FIR signal) is the failed one
A corpus is the three streams of one geometry back to back in a buffer of exactly their summed length (entries m16, crc,
m2: the last entry's one-sample frame ends the buffer)."""
import functools
from collections import namedtuple

import numpy as np

import diff_levels_ref as DL
import events_ref as E
import fir_levels_ref as FL
import fir_range_levels_ref as FR
import levels_ref as L
import oracle_lib as O
import plane_events_ref as PE
import quantiles_ref as Q
import range_levels_ref as RL
import ranges_ref as RR
import seg_index_ref as SI
import signal_range_levels_ref as SR
import tone_bank_levels_ref as TB
import tone_bank_range_levels_ref as TBR
import tone_levels_ref as TL
import tone_range_levels_ref as TRL

FILL = 165                          # X3HIP_FENCE_FILL of the children: what a fresh buffer holds
ENV = {"X3HIP_FENCE": "16", "X3HIP_FENCE_FILL": str(FILL), "X3HIP_FENCE_TIGHT": "1"}
BL = 20
CRC = RR.ERR_PAYLOAD_CRC
BIN = 33                            # divides neither a frame (140, 2 000) nor a block (20), and 20 does not divide it
BINS = (BIN, 0, 1)
SEG_BLOCKS = {7: 4, 100: 32}        # two and four stretches a frame
# name -> (blocks a frame, full frames, kind)
STREAMS = {"m16_7": (7, 3, "m16"), "m2_7": (7, 1, "m2"), "crc_7": (7, 2, "crc"),
           "m16_100": (100, 1, "m16"), "m2_100": (100, 2, "m2"), "crc_100": (100, 3, "crc")}
RESIDUE = {"m16": 0, "m2": 2, "crc": None}   # size mod 16
CORPORA = {7: ("m16_7", "crc_7", "m2_7"), 100: ("m16_100", "crc_100", "m2_100")}

TAPS8, SHIFT8 = (-1000, 2900, -5000, 7400, -7400, 5000, -2900, 1000), 7
STEPS = (350_898_828, 992_137_445, 644_245_094, 1_760_936_591, 0, 1 << 31, (1 << 32) - 1, 1 << 30)
SIGNALS = ("samples", "diff", "fir8", "tone", "bank3", "bank8")   # bank3: three tones run the kernel instance of four
BANKS = {"tone": STEPS[:1], "bank3": STEPS[:3], "bank8": STEPS}
assert FL.check(TAPS8, SHIFT8)

Stream = namedtuple("Stream", "name bpf k kind bytes offs so frames total F seg_blocks n_index")


def oparams(bpf):
    return O.Params.make(BL, bpf)


def _wav(seed, n):
    """noise of a few hundred over a slow sine: frames of Rice and BFP blocks whose sizes move with the seed"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    w = 3000.0 * np.sin(t * 0.013 * (1 + seed % 5)) + rng.integers(-400, 401, n) * (1 + (t // 50) % 3)
    return np.clip(np.rint(w), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def stream(name):
    """the first seed whose stream has the size residue the name asks for"""
    bpf, k, kind = STREAMS[name]
    n = BL * bpf * k + 1
    want = RESIDUE[kind]
    for seed in range(2000):
        rc, s, _ = O.encode(_wav(1000 * bpf + 10 * seed + k, n), oparams(bpf))
        assert rc == 0
        if want is None or s.size % 16 == want:
            break
    else:
        raise AssertionError("no seed gives %s its size" % name)
    s = s.copy()
    offs = RR.frame_offsets(s)
    if kind == "crc":
        s[offs[k - 1] + 20 + 5] ^= 0x10          # (the last full frame's payload; its CRC is left as it was)
    frames = RR.frames_of(s, offs, oparams(bpf))
    so = RR.sample_offsets([(int(s[o + 4]) << 8) | int(s[o + 5]) for o in offs[:-1]])
    s.setflags(write=False)
    sb = SEG_BLOCKS[bpf]
    return Stream(name, bpf, k, kind, s, offs, so, frames, int(so[-1]), len(offs) - 1, sb, SI.n_words(len(offs) - 1, oparams(bpf), sb))


Corpus = namedtuple("Corpus", "bpf names bytes offsets lengths entries n_samples F total_rows_of seg_blocks")


@functools.lru_cache(maxsize=None)
def corpus(bpf, picks=(0, 1, 2)):
    """picks: the entries as indices into CORPORA[bpf], in the buffer's order or -- the tables of B4 -- with repeats, which
    the corpus calls allow; the buffer is the three streams either way"""
    three = [stream(n) for n in CORPORA[bpf]]
    ss = [three[i] for i in picks]
    at = [int(v) for v in np.concatenate([[0], np.cumsum([s.bytes.size for s in three])])]
    lengths = [s.bytes.size for s in ss]
    offsets = [at[i] for i in picks]
    buf = np.concatenate([s.bytes for s in three])
    buf.setflags(write=False)
    return Corpus(bpf, tuple(CORPORA[bpf][i] for i in picks), buf, offsets, lengths, ss, [s.total for s in ss], sum(s.F for s in ss),
                  lambda bin_len: int(L.corpus_row_first([s.total for s in ss], bin_len)[-1]), SEG_BLOCKS[bpf])


# ------------------------------------------------------------------------------------------------ references

def split(frames):
    """ranges_ref's frames -> (samples per frame, empty where it failed; statuses): the levels references' form"""
    return [w if st == 0 else np.zeros(0, dtype=np.int16) for st, w in frames], [int(st) for st, _ in frames]


def summary(st, extra=()):
    """what the result calls say about statuses: (rc, n_bad, first_bad, its status) + extra"""
    bad = np.flatnonzero(np.asarray(st))
    return (0, int(bad.size), int(bad[0]) if bad.size else len(st), int(st[bad[0]]) if bad.size else 0) + tuple(extra)


def planes_of(signal):
    return len(BANKS[signal]) if signal.startswith("bank") else 1


def levels_ref(signal, frames, so, bin_len, n_bins):
    """-> records [n_bins], or [planes, n_bins] of a bank"""
    fr, st = split(frames)
    so = [int(v) for v in so[:-1]]
    if signal == "samples":
        return L.levels(fr, st, so, bin_len, n_bins)
    if signal == "diff":
        return DL.signal_levels(fr, st, so, bin_len, n_bins, DL.DIFF)
    if signal == "fir8":
        return FL.fir_levels(fr, st, so, bin_len, n_bins, TAPS8, SHIFT8)
    if signal == "tone":
        return TL.tone_levels(fr, st, so, bin_len, n_bins, STEPS[0])
    return TB.tone_bank_levels(fr, st, so, bin_len, n_bins, BANKS[signal])


def corpus_levels_ref(signal, c, bin_len):
    """-> records [rows] or [planes, rows]: every entry a stream of its own, entry behind entry"""
    parts = [levels_ref(signal, s.frames, s.so, bin_len, L.n_bins_for(s.total, bin_len)) for s in c.entries]
    return np.concatenate(parts, axis=-1)


def power_ref(tone):
    """x3_tone_power_levels_dev over all planes at once"""
    flat = tone.reshape(-1)
    return TL.tone_power_levels(flat).reshape(tone.shape)


def range_levels_ref(signal, frames, so, starts, lens, bin_len, stride, cap):
    """-> (records uint8 [cap, 32] or [planes, cap, 32], row offsets, statuses); what no call writes keeps FILL"""
    a = (frames, so, starts, lens, bin_len, stride, cap)
    if signal == "samples":
        return RL.range_levels(*a, fill=FILL)
    if signal == "diff":
        return SR.range_levels(*a, SR.DIFF, fill=FILL)
    if signal == "fir8":
        return FR.range_levels(*a, TAPS8, SHIFT8, fill=FILL)
    if signal == "tone":
        return TRL.range_levels(*a, STEPS[0], None, fill=FILL)
    return TBR.range_levels(*a, BANKS[signal], None, fill=FILL)


def per_entry(fn, c, ent, span):
    """a corpus call's arrays from the stream reference on each entry alone: fn(frames, so) -> (out [..., cap(, 32)],
    offsets, statuses) over ALL ranges (the layout depends on the lengths alone); range w takes its span(w) rows at its
    offset, and its status, from the run on entry ent[w].  `out` is indexed along its axis -2 (records) or -1 (samples)."""
    out = off = st = None
    for e, s in enumerate(c.entries):
        o, f, t = fn(s.frames, s.so)
        rows = o.shape[-2] if o.dtype == np.uint8 else o.shape[-1]
        o2 = o.reshape(-1, rows, 32) if o.dtype == np.uint8 else o.reshape(1, rows)
        if out is None:
            out, off, st, shape = o2.copy(), f, t.copy(), o.shape
        for w in np.flatnonzero(np.asarray(ent) == e):
            a = int(f[w])
            out[:, a:a + span(w)] = o2[:, a:a + span(w)]
            st[w] = t[w]
    return out.reshape(shape), off, st


def samples_as(out16, fmt):
    """ranges_ref's int16 buffer (FILL where no call writes) in the call's format: int16, or float32 bits"""
    return out16 if fmt == 0 else RR.f32_bits(out16)


def ranges_ref(frames, so, starts, lens, stride, cap, fmt):
    """-> (out in the format, offsets, statuses); float32: the unwritten positions hold FILL in all four bytes"""
    o, off, st = RR.ranges(frames, so, starts, lens, stride, cap, FILL << 8 | FILL)
    if fmt == 0:
        return o, off, st
    z = RR.ranges(frames, so, starts, lens, stride, cap, 0)[0]
    f = RR.f32_bits(o)
    f[o != z] = np.uint32(FILL * 0x01010101)
    return f, off, st


# ------------------------------------------------------------------------------------------------ cases

class Case:
    """name; inputs: name -> array (a buffer of exactly its bytes, uploaded); outputs: name -> the expected array (a buffer
    of exactly its bytes, FILL before the call, compared byte for byte behind it); control: the outputs that are statuses,
    offsets or counts; exact: (what, the size the case gives, the reference's own need); result: what enqueue returns --
    the call's result call, every return code asserted 0 on the way"""

    def __init__(self, name, inputs, outputs, control, exact, result, enqueue):
        self.name, self.inputs, self.outputs, self.control = name, inputs, outputs, set(control)
        self.exact, self.result, self.enqueue = exact, result, enqueue


def u64(v):
    return np.asarray(v, dtype=np.uint64)


def u32(v):
    return np.asarray(v, dtype=np.uint32)


def ok(rc, ctx):
    assert rc == 0, (rc, ctx.last_error())


# ---- B1: windows and ranges

def b1_stream_cases(s):
    out = []
    spf = BL * s.bpf
    for idx in (False, True):
        for fmt in (0, 1):
            tag = "%s%s_%s" % (s.name, "_idx" if idx else "", "f32" if fmt else "i16")
            for what, f in (("last_frame", s.F - 1), ("last_full_frame", s.F - 2)):   # a window that is exactly frame f
                start, length = int(s.so[f]), spf if f == s.F - 2 else 1
                row, st = RR.one(s.frames, s.so, start, length)

                def enq(x3, ctx, src, d, length=length, fmt=fmt, idx=idx):
                    ok(ctx.decode_windows_dev(*src.args(), d["starts"], 1, length, d["out"], fmt, d["st"], **src.index(idx)), ctx)
                    return ctx.decode_windows_result()
                out.append(Case("window_%s_%s" % (what, tag), {"starts": u64([start])},
                                {"out": samples_as(row, fmt), "st": np.array([st], dtype=np.int32)}, {"st"},
                                [("window_len", length, int(s.so[f + 1] - s.so[f]))],
                                summary([st]), enq))
            starts, lens = [s.total - 1, s.total, 0], [1, 0, s.total]
            for stride in (0, max(lens)):
                cap = len(lens) * stride or sum(lens)
                o, off, st = ranges_ref(s.frames, s.so, starts, lens, stride, cap, fmt)

                def enq(x3, ctx, src, d, stride=stride, cap=cap, fmt=fmt, idx=idx, n=len(lens)):
                    ok(ctx.decode_ranges_dev(*src.args(), d["starts"], d["lens"], n, stride, d["out"], cap, fmt, d["off"], d["st"],
                                             **src.index(idx)), ctx)
                    return ctx.decode_ranges_result()
                out.append(Case("ranges_%s_%s" % ("padded" if stride else "packed", tag), {"starts": u64(starts), "lens": u32(lens)},
                                {"out": o, "off": off, "st": st}, {"off", "st"},
                                [("out_cap", cap, len(lens) * max(lens) if stride else sum(lens)), ("row_stride", stride, max(lens) if stride else 0)],
                                summary(st, (sum(lens),)), enq))
    return out


def corpus_table(c):
    """per entry: its last sample alone, the empty range at its end, all of it"""
    ent, starts, lens = [], [], []
    for e, s in enumerate(c.entries):
        ent += [e, e, e]
        starts += [s.total - 1, s.total, 0]
        lens += [1, 0, s.total]
    return ent, starts, lens


def b1_corpus_cases(c):
    out = []
    ent, starts, lens = corpus_table(c)
    n = len(ent)
    for fmt in (0, 1):
        for stride in (0, max(lens)):
            cap = n * stride or sum(lens)
            o, off, st = per_entry(lambda fr, so: ranges_ref(fr, so, starts, lens, stride, cap, fmt), c, ent,
                                   lambda w: stride or lens[w])

            def enq(x3, ctx, src, d, stride=stride, cap=cap, fmt=fmt):
                ok(src.corpus.ranges_into(d["ent"], d["starts"], d["lens"], n, stride, d["out"], cap, fmt, d["off"], d["st"]), ctx)
                return ctx.decode_ranges_result()
            out.append(Case("corpus%d_ranges_%s_%s" % (c.bpf, "padded" if stride else "packed", "f32" if fmt else "i16"),
                            {"ent": u32(ent), "starts": u64(starts), "lens": u32(lens)}, {"out": o, "off": off, "st": st},
                            {"off", "st"}, [("out_cap", cap, n * max(lens) if stride else sum(lens))], summary(st, (sum(lens),)), enq))
    return out


# ---- B2: levels

def signal_args(x3, ctx, src, signal):
    """-> (the prefix of the call's name in front of levels_dev / range_levels_dev, its keyword)"""
    if signal == "samples":
        return "", {}
    if signal == "diff":
        return "signal_", {"signal": x3.LEVEL_SIGNAL_DIFF}
    if signal == "fir8":
        return "fir_", {"fir": x3.Fir(TAPS8, SHIFT8)}
    if signal == "tone":
        return "tone_", {"tone": x3.LevelTone(STEPS[0], 0, src.d_table)}
    steps = list(BANKS[signal])
    return "tone_bank_", {"tones": x3.LevelToneBank(len(steps), 0, src.d_table,
                                                    (x3.C.c_uint32 * 8)(*(steps + [0xDEADBEEF] * (8 - len(steps)))))}


def levels_case(name, signal, want, statuses, n_rows, need_rows, call):
    """a levels call and, for the tone signals, x3_tone_power_levels_dev in place over all planes in one launch"""
    planes = planes_of(signal)
    tone = signal in BANKS

    def enq(x3, ctx, src, d):
        kind, kw = signal_args(x3, ctx, src, signal)
        ok(call(x3, ctx, src, d, kind, kw), ctx)
        res = ctx.levels_result()
        if tone:
            got = ctx.download(d["lv"], want.nbytes)
            assert np.array_equal(got, want.view(np.uint8).reshape(-1)), (name, "the tone records in front of the adapter")
            ok(ctx.tone_power_levels_dev(d["lv"], planes * n_rows, d["lv"]), ctx)
            ctx.sync()
        return res
    return Case(name, {}, {"lv": power_ref(want) if tone else want, "fst": np.array(statuses, dtype=np.int32)}, {"fst"},
                [("n_bins", n_rows, need_rows), ("levels bytes", want.nbytes, planes * need_rows * 32)], summary(statuses), enq)


def b2_stream_cases(s):
    out = []
    statuses = [st for st, _ in s.frames]
    for idx in (False, True):
        for signal in SIGNALS:
            for bin_len in BINS:
                nb = L.n_bins_for(s.total, bin_len)
                want = levels_ref(signal, s.frames, s.so, bin_len, nb)

                def call(x3, ctx, src, d, kind, kw, bin_len=bin_len, nb=nb, idx=idx):
                    return getattr(ctx, kind + "levels_dev")(*src.args(), bin_len, d["lv"], nb, d["fst"], **src.index(idx), **kw)
                out.append(levels_case("levels_%s%s_%s_bin%d" % (s.name, "_idx" if idx else "", signal, bin_len), signal, want,
                                       statuses, nb, -(-s.total // bin_len) if bin_len else 1, call))
    return out


def b2_corpus_cases(c):
    out = []
    statuses = [st for s in c.entries for st, _ in s.frames]
    for signal in SIGNALS:
        for bin_len in BINS:
            rows = c.total_rows_of(bin_len)
            want = corpus_levels_ref(signal, c, bin_len)

            def call(x3, ctx, src, d, kind, kw, bin_len=bin_len, rows=rows):
                return getattr(ctx, "corpus_" + kind + "levels_dev")(src.corpus, bin_len, d["lv"], rows, d["fst"], **kw)
            out.append(levels_case("corpus%d_levels_%s_bin%d" % (c.bpf, signal, bin_len), signal, want, statuses, rows,
                                   sum((-(-s.total // bin_len) if bin_len else 1) for s in c.entries), call))
    return out


# ---- B3: range levels

def stream_ranges(s):
    """one that ends on the last sample (from inside the last full frame); all; the empty one at the end; one inside the
    one-sample frame -- in a "crc" stream its lead frame, the history of DIFF and FIR, is the failed one; the first five
    positions of the last full frame (its lead frame is the frame in front, or none)"""
    spf = BL * s.bpf
    return [s.total - 3, 0, s.total, s.total - 1, (s.k - 1) * spf], [3, s.total, 0, 1, 5]


def range_levels_case(name, signal, inputs, want, n, bin_len, stride, cap, lens, call):
    rec, off, st = want
    rows = [RL.rows_of(v, bin_len) for v in lens]

    def enq(x3, ctx, src, d):
        kind, kw = signal_args(x3, ctx, src, signal)
        ok(call(x3, ctx, src, d, kind, kw), ctx)
        return ctx.range_levels_result()
    return Case(name, inputs, {"lv": rec, "off": off, "st": st}, {"off", "st"},
                [("rows_cap", cap, n * stride if stride else sum(rows)), ("row_stride", stride, max(rows) if stride else 0),
                 ("levels bytes", rec.nbytes, planes_of(signal) * cap * 32)], summary(st, (sum(rows),)), enq)


def b3_stream_cases(s):
    out = []
    starts, lens = stream_ranges(s)
    n = len(lens)
    for idx in (False, True):
        for signal in SIGNALS:
            for bin_len in (BIN, 0):
                rows = [RL.rows_of(v, bin_len) for v in lens]
                for stride in (0, max(rows)):
                    cap = n * stride or sum(rows)
                    want = range_levels_ref(signal, s.frames, s.so, starts, lens, bin_len, stride, cap)

                    def call(x3, ctx, src, d, kind, kw, bin_len=bin_len, stride=stride, cap=cap, idx=idx):
                        return getattr(ctx, kind + "range_levels_dev")(*src.args(), d["starts"], d["lens"], n, bin_len, stride, d["lv"],
                                                                        cap, d["off"], d["st"], **src.index(idx), **kw)
                    out.append(range_levels_case("range_levels_%s%s_%s_bin%d_%s" % (s.name, "_idx" if idx else "", signal, bin_len,
                                                                                  "padded" if stride else "packed"), signal,
                                                 {"starts": u64(starts), "lens": u32(lens)}, want, n, bin_len, stride, cap, lens, call))
    return out


def corpus_ranges(c):
    ent, starts, lens = [], [], []
    for e, s in enumerate(c.entries):
        a, b = stream_ranges(s)
        ent += [e] * len(a)
        starts += a
        lens += b
    return ent, starts, lens


def b3_corpus_cases(c):
    out = []
    ent, starts, lens = corpus_ranges(c)
    n = len(ent)
    for signal in SIGNALS:
        for bin_len in (BIN, 0):
            rows = [RL.rows_of(v, bin_len) for v in lens]
            for stride in (0, max(rows)):
                cap = n * stride or sum(rows)
                want = per_entry(lambda fr, so: range_levels_ref(signal, fr, so, starts, lens, bin_len, stride, cap), c, ent,
                                 lambda w: stride or rows[w])

                def call(x3, ctx, src, d, kind, kw, bin_len=bin_len, stride=stride, cap=cap):
                    return getattr(ctx, "corpus_" + kind + "range_levels_dev")(src.corpus, d["ent"], d["starts"], d["lens"], n, bin_len,
                                                                               stride, d["lv"], cap, d["off"], d["st"], **kw)
                out.append(range_levels_case("corpus%d_range_levels_%s_bin%d_%s" % (c.bpf, signal, bin_len, "padded" if stride else "packed"),
                                             signal, {"ent": u32(ent), "starts": u64(starts), "lens": u32(lens)}, want, n, bin_len,
                                             stride, cap, lens, call))
    return out


# ---- B4: from records (no decode): synthetic level records around the events kernels' tile of 256 rows

EVENTS_TILE = 256
N_ROWS = (255, 256, 257)
# A corpus form takes exactly the rows its entry table gives.  The entries of the corpus of 100 blocks a frame hold 2 001,
# 6 001 and 4 001 samples: n_rows -> (the entries of a table over that buffer, the bin length) with exactly n_rows rows
REC_TABLES = {255: ((0, 0, 1, 1, 2), 79), 256: ((0, 1, 1, 2), 71), 257: ((0, 1, 2), 47)}
Q_PPM = [100_000, 500_000, 990_000]
EV_RULE = E.Rule(mean_sq_min=1_000_000, peak_min=0, join_bins=2, min_bins=2, pad_bins=1, max_bins=3)
AD_RULE = E.Rule(join_bins=2, min_bins=2, pad_bins=1, max_bins=3)
TRULE = Q.TRule(peak=(900_000, 3, 2, 5), mean_sq=(500_000, 16, 1, 0))
PLANE_K = (8, 3)
# the rows of the loud runs of plane 0 (first, last), the last one from the rows' end backwards: it reaches the last row;
# which of them the other planes share: record_planes()
RUNS = ((3, 5), (40, 41), (100, 106), (130, 130), (200, 204), (-4, -1))


def quiet(n_rows, seed):
    """counting records of a floor whose keys differ from row to row"""
    REC_BIN = REC_TABLES[n_rows][1]
    rng = np.random.default_rng(seed)
    lv = L.empty(n_rows)
    lv["n"] = REC_BIN
    peak = rng.integers(5, 60, n_rows)
    lv["max"], lv["min"] = peak, -rng.integers(1, 60, n_rows)
    lv["sum"] = rng.integers(-200, 200, n_rows)
    lv["sum_sq"] = rng.integers(100, 5000, n_rows).astype(np.uint64) * np.uint64(REC_BIN)
    return lv


def loud(lv, a, b, amp):
    lv["max"][a:b + 1], lv["min"][a:b + 1] = amp, -amp + 7
    lv["sum_sq"][a:b + 1] = np.uint64(amp) * np.uint64(amp) * lv["n"][a:b + 1].astype(np.uint64) // np.uint64(2)


@functools.lru_cache(maxsize=None)
def record_planes(n_rows, K):
    """K planes [K, n_rows]: plane 0 holds every run, plane 1 all but run 1 (a row loud in exactly one plane), planes 2 and up
    runs 2, 4 and the last (rows loud in all K planes); run 3 is one row (min_bins drops it) and is loud in planes 0 and 1
    alone (a row loud in exactly two)"""
    planes = np.stack([quiet(n_rows, 7 * n_rows + t) for t in range(K)])
    for i, (a, b) in enumerate(RUNS):
        a, b = (a + n_rows, b + n_rows) if a < 0 else (a, b)
        for t in range(K):
            if t == 0 or (t == 1 and i != 1) or (t >= 2 and i in (2, 4, 5)):
                loud(planes[t], a, b, 9000 + 100 * t + i)
    planes.setflags(write=False)
    return planes


def loud_counts(planes, n_rows, rule):
    """per row the number of planes that are loud under the rule's values"""
    per = PE.plane_rules(rule, len(planes))
    return np.array([sum(E.is_hot(planes[t][b], per[t]) for t in range(len(planes))) for b in range(n_rows)])


def plane_rule(K, min_planes):
    return PE.PlaneRule([EV_RULE.mean_sq_min] * K, [0] * K, min_planes, EV_RULE.join_bins, EV_RULE.min_bins, EV_RULE.pad_bins,
                        EV_RULE.max_bins)


def slot_outputs(slots, with_entries, planes=False):
    """events_ref.slots / plane_events_ref.slots -> the outputs of a case"""
    if planes:
        ent, st, ln, mk, lv = slots
        o = {"ev_st": st, "ev_ln": ln, "ev_mk": mk, "ev_lv": lv}
    else:
        ent, st, ln, lv = slots
        o = {"ev_st": st, "ev_ln": ln, "ev_lv": lv}
    if with_entries:
        o["ev_ent"] = ent
    return o


def thr_records(thrs):
    a = np.zeros(len(thrs), dtype=np.dtype([("mean_sq_min", "<u8"), ("peak_min", "<u4"), ("counted", "<u4")]))
    for i, t in enumerate(thrs):
        a[i] = tuple(t)
    return a


def b4_cases(c, n_rows):
    """c: the corpus whose entry table the corpus forms run on, of exactly n_rows rows at its bin length; the stream forms
    take the same records as one stream of n_rows * REC_BIN - 3 samples"""
    out = []
    n_samples = c.n_samples
    REC_BIN = REC_TABLES[n_rows][1]
    assert c.total_rows_of(REC_BIN) == n_rows
    total = n_rows * REC_BIN - 3
    lv = record_planes(n_rows, 1)[0]
    for corpus_form in (False, True):
        tag = "%s%d" % ("corpus_" if corpus_form else "", n_rows)
        n_ent = len(n_samples) if corpus_form else 1
        inputs = {"lv": lv} if corpus_form else {"lv": lv, "total": u64([total])}
        ev, elv = E.corpus_events(lv, n_samples, REC_BIN, EV_RULE) if corpus_form else E.stream_events(lv, total, REC_BIN, EV_RULE)
        thrs = Q.corpus_thresholds(lv, n_samples, REC_BIN, TRULE) if corpus_form else Q.stream_thresholds(lv, total, REC_BIN, TRULE)
        aev, aelv = (Q.corpus_adaptive_events(lv, n_samples, REC_BIN, thrs, AD_RULE) if corpus_form else
                     Q.stream_adaptive_events(lv, total, REC_BIN, thrs[0], AD_RULE))
        for short in (0, 1):
            cap = len(ev) - short

            def enq(x3, ctx, src, d, cap=cap, n_rows=n_rows, corpus_form=corpus_form):
                r = x3.EventRule.make(*EV_RULE)
                if corpus_form:
                    ok(ctx.corpus_events_dev(src.corpus, d["lv"], n_rows, REC_BIN, r, d["ev_ent"], d["ev_st"], d["ev_ln"], d["ev_lv"],
                                             cap, d["cnt"]), ctx)
                else:
                    ok(ctx.events_dev(d["lv"], n_rows, REC_BIN, d["total"], r, d["ev_st"], d["ev_ln"], d["ev_lv"], cap, d["cnt"]), ctx)
                return ctx.events_result()
            out.append(Case("events_%s_cap%d" % (tag, cap), inputs,
                            dict(slot_outputs(E.slots(ev, elv, cap, corpus_form), corpus_form), cnt=u64([len(ev)])), {"cnt"},
                            [("cap", cap + short, len(ev))], (0, len(ev)), enq))
            acap = len(aev) - short

            def enq(x3, ctx, src, d, cap=acap, n_rows=n_rows, corpus_form=corpus_form):
                r, t = x3.EventRule.make(*AD_RULE), x3.ThresholdRule.make(TRULE.peak, TRULE.mean_sq)
                if corpus_form:
                    ok(ctx.corpus_level_thresholds_dev(src.corpus, d["lv"], n_rows, REC_BIN, t, d["thr"]), ctx)
                    ok(ctx.corpus_events_adaptive_dev(src.corpus, d["lv"], n_rows, REC_BIN, r, d["thr"], d["ev_ent"], d["ev_st"],
                                                      d["ev_ln"], d["ev_lv"], cap, d["cnt"]), ctx)
                else:
                    ok(ctx.level_thresholds_dev(d["lv"], n_rows, REC_BIN, d["total"], t, d["thr"]), ctx)
                    ok(ctx.events_adaptive_dev(d["lv"], n_rows, REC_BIN, d["total"], r, d["thr"], d["ev_st"], d["ev_ln"], d["ev_lv"],
                                               cap, d["cnt"]), ctx)
                return ctx.level_quantiles_result() + ctx.events_result()
            empty = [e for e, t in enumerate(thrs) if t[2] == 0]
            out.append(Case("adaptive_%s_cap%d" % (tag, acap), inputs,
                            dict(slot_outputs(E.slots(aev, aelv, acap, corpus_form), corpus_form), cnt=u64([len(aev)]),
                                 thr=thr_records(thrs)), {"cnt", "thr"},
                            [("cap", acap + short, len(aev)), ("thr bytes", thr_records(thrs).nbytes, 16 * n_ent)],
                            (0, len(empty), empty[0] if empty else n_ent, 0, len(aev)), enq))
        for key in (Q.PEAK, Q.MEAN_SQ):
            vals, counted = (Q.corpus_quantiles(lv, n_samples, REC_BIN, key, Q_PPM) if corpus_form else
                             Q.stream_quantiles(lv, total, REC_BIN, key, Q_PPM))

            def enq(x3, ctx, src, d, key=key, n_rows=n_rows, corpus_form=corpus_form):
                if corpus_form:
                    ok(ctx.corpus_level_quantiles_dev(src.corpus, d["lv"], n_rows, REC_BIN, key, Q_PPM, d["values"], d["counted"]), ctx)
                else:
                    ok(ctx.level_quantiles_dev(d["lv"], n_rows, REC_BIN, d["total"], key, Q_PPM, d["values"], d["counted"]), ctx)
                return ctx.level_quantiles_result()
            empty = [e for e, k in enumerate(counted) if k == 0]
            out.append(Case("quantiles_%s_key%d" % (tag, key), inputs, {"values": vals, "counted": counted}, {"values", "counted"},
                            [("values bytes", vals.nbytes, 4 * len(Q_PPM) * n_ent)], (0, len(empty), empty[0] if empty else n_ent), enq))
        for K in PLANE_K:
            planes = record_planes(n_rows, K)
            stride = n_rows + 5
            held = (K - 1) * stride + n_rows          # the header's minimum: no records behind the last plane's n_rows
            up = np.stack([L.empty(stride) for _ in range(K)])
            up["n"], up["max"], up["sum_sq"] = 1, 32767, 1 << 30     # (the slack: loud under every rule, never read)
            up[:, :n_rows] = planes
            pin = dict(inputs, lv=up.reshape(-1)[:held].copy())
            for mp in (1, 2, K):
                rule = plane_rule(K, mp)
                pev, pelv = (PE.corpus_plane_events(planes, n_samples, REC_BIN, rule) if corpus_form else
                             PE.stream_plane_events(planes, total, REC_BIN, rule))
                for short in (0, 1):
                    cap = len(pev) - short

                    def enq(x3, ctx, src, d, cap=cap, n_rows=n_rows, corpus_form=corpus_form, rule=rule, stride=stride):
                        r = x3.PlaneEventRule.make(list(rule.mean_sq_min), list(rule.peak_min), rule.min_planes, rule.join_bins,
                                                   rule.min_bins, rule.pad_bins, rule.max_bins)
                        if corpus_form:
                            ok(ctx.corpus_plane_events_dev(src.corpus, d["lv"], stride, n_rows, REC_BIN, r, None, d["ev_ent"],
                                                           d["ev_st"], d["ev_ln"], d["ev_mk"], d["ev_lv"], cap, d["cnt"]), ctx)
                        else:
                            ok(ctx.plane_events_dev(d["lv"], stride, n_rows, REC_BIN, d["total"], r, None, d["ev_st"], d["ev_ln"],
                                                    d["ev_mk"], d["ev_lv"], cap, d["cnt"]), ctx)
                        return ctx.events_result()
                    out.append(Case("plane_events_%s_K%d_min%d_cap%d" % (tag, K, mp, cap), pin,
                                    dict(slot_outputs(PE.slots(pev, pelv, cap, corpus_form), corpus_form, True), cnt=u64([len(pev)])),
                                    {"cnt"}, [("cap", cap + short, len(pev)), ("levels records", len(pin["lv"]), (K - 1) * (n_rows + 5) + n_rows)],
                                    (0, len(pev)), enq))
            # ... and with a threshold record per (plane, entry): exactly 16 * K * n_ent bytes
            rule = plane_rule(K, 2)
            thr = [[(rule.mean_sq_min[t], 0, 0xDEAD0000 + e) for e in range(n_ent)] for t in range(K)]
            pev, pelv = (PE.corpus_plane_events(planes, n_samples, REC_BIN, rule._replace(mean_sq_min=[0] * K), thr) if corpus_form else
                         PE.stream_plane_events(planes, total, REC_BIN, rule._replace(mean_sq_min=[0] * K), [t[0] for t in thr]))
            cap = len(pev)

            def enq(x3, ctx, src, d, cap=cap, n_rows=n_rows, corpus_form=corpus_form, rule=rule, stride=stride, K=K):
                r = x3.PlaneEventRule.make(None, None, rule.min_planes, rule.join_bins, rule.min_bins, rule.pad_bins, rule.max_bins,
                                           n_planes=K)
                if corpus_form:
                    ok(ctx.corpus_plane_events_dev(src.corpus, d["lv"], stride, n_rows, REC_BIN, r, d["pthr"], d["ev_ent"], d["ev_st"],
                                                   d["ev_ln"], d["ev_mk"], d["ev_lv"], cap, d["cnt"]), ctx)
                else:
                    ok(ctx.plane_events_dev(d["lv"], stride, n_rows, REC_BIN, d["total"], r, d["pthr"], d["ev_st"], d["ev_ln"],
                                            d["ev_mk"], d["ev_lv"], cap, d["cnt"]), ctx)
                return ctx.events_result()
            pthr = thr_records([v for t in thr for v in t])
            out.append(Case("plane_events_%s_K%d_thr" % (tag, K), dict(pin, pthr=pthr),
                            dict(slot_outputs(PE.slots(pev, pelv, cap, corpus_form), corpus_form, True), cnt=u64([len(pev)])),
                            {"cnt"}, [("cap", cap, len(pev)), ("thr bytes", pthr.nbytes, 16 * K * n_ent)], (0, len(pev)), enq))
    return out


# ------------------------------------------------------------------------------------------------ groups

@functools.lru_cache(maxsize=None)
def group(name):
    """-> [(source, cases)]: source a Stream or a Corpus, built once per group in the child"""
    ss, cs = [stream(n) for n in STREAMS], [corpus(b) for b in CORPORA]
    if name == "B1":
        return [(s, b1_stream_cases(s)) for s in ss] + [(c, b1_corpus_cases(c)) for c in cs]
    if name == "B2_stream":
        return [(s, b2_stream_cases(s)) for s in ss]
    if name == "B2_corpus":
        return [(c, b2_corpus_cases(c)) for c in cs]
    if name == "B3_stream":
        return [(s, b3_stream_cases(s)) for s in ss]
    if name == "B3_corpus":
        return [(c, b3_corpus_cases(c)) for c in cs]
    if name == "B4":
        return [(c, b4_cases(c, n)) for n in N_ROWS for c in [corpus(100, REC_TABLES[n][0])]]
    raise KeyError(name)


GROUPS = ("B1", "B2_stream", "B2_corpus", "B3_stream", "B3_corpus", "B4")
# cases per group: asserted on the CPU against the tables and on the GPU against what the child says it ran
COUNTS = {"B1": 6 * 2 * 2 * 4 + 2 * 4, "B2_stream": 6 * 2 * 6 * 3, "B2_corpus": 2 * 6 * 3, "B3_stream": 6 * 2 * 6 * 2 * 2,
          "B3_corpus": 2 * 6 * 2 * 2, "B4": 3 * 2 * (2 + 2 + 2 + 2 * (3 * 2 + 1))}


def n_cases(name):
    return sum(len(cases) for _, cases in group(name))


# ------------------------------------------------------------------------------------------------ the child's side

def bytes_of(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Source:
    """a stream or a corpus on the device, every buffer of exactly its bytes: the stream, F + 1 frame offsets, F + 1 sample
    offsets from x3_sample_offsets_dev, the index of exactly x3_seg_index_entries words from x3_seg_index_build_dev, a tone
    table of 4 096 bytes; a corpus: the buffer of the entries back to back, in the (ptr, size) form of x3hip.Corpus"""

    def __init__(self, x3, ctx, s):
        self.ctx, self.own, self.corpus = ctx, [], None
        self.params = x3.Params.make(BL, s.bpf)
        self.d_table = self.alloc(TL.table())
        if isinstance(s, Corpus):
            self.d_x3 = self.alloc(s.bytes)
            self.corpus = x3.Corpus(ctx, (self.d_x3, s.bytes.size), s.offsets, s.lengths, params=self.params, seg_blocks=s.seg_blocks,
                                    index="walk")
            assert self.corpus.entries["n_samples"].tolist() == s.n_samples and self.corpus.n_frames == s.F
            assert self.corpus.entries["n_frames"].tolist() == [e.F for e in s.entries]
            return
        self.d_x3, self.x3_len, self.F, self.sb = self.alloc(s.bytes), s.bytes.size, s.F, s.seg_blocks
        self.d_off = self.alloc(u64(s.offs))
        self.d_so = ctx.alloc(8 * (s.F + 1))
        self.own.append(self.d_so)
        ok(ctx.sample_offsets_dev(self.d_x3, self.x3_len, self.d_off, s.F, self.d_so), ctx)
        assert np.array_equal(ctx.download(self.d_so, 8 * (s.F + 1), np.uint64), s.so)
        ne = x3.lib().x3_seg_index_entries(s.F, x3.C.byref(self.params), s.seg_blocks)
        assert ne == s.n_index and ne > 0
        self.d_idx = ctx.alloc(8 * ne)
        self.own.append(self.d_idx)
        ok(ctx.seg_index_build_dev(self.d_x3, self.x3_len, self.d_off, s.F, self.params, self.d_idx, s.seg_blocks), ctx)

    def alloc(self, a):
        a = bytes_of(a)
        p = self.ctx.alloc(a.size)
        self.own.append(p)
        self.ctx.upload(p, a)
        return p

    def args(self):
        return (self.d_x3, self.x3_len, self.d_off, self.d_so, self.F, self.params)

    def index(self, on):
        return {"d_seg_index": self.d_idx, "seg_blocks": self.sb} if on else {}

    def close(self):
        if self.corpus is not None:
            self.corpus.close()
        for p in self.own:
            self.ctx.free(p)


def run_case(x3, ctx, src, case):
    d = {}
    try:
        for k, a in case.inputs.items():
            d[k] = ctx.alloc(bytes_of(a).size)
            ctx.upload(d[k], bytes_of(a))
        for k, a in case.outputs.items():
            d[k] = ctx.alloc(bytes_of(a).size)
            ctx.upload(d[k], np.full(bytes_of(a).size, FILL, dtype=np.uint8))
        res = tuple(case.enqueue(x3, ctx, src, d))
        assert res == tuple(case.result), (case.name, "result", res, case.result)
        for k, a in case.outputs.items():
            got, want = ctx.download(d[k], bytes_of(a).size), bytes_of(a)
            assert np.array_equal(got, want), (case.name, k, np.flatnonzero(got != want)[:8].tolist())
    finally:
        for p in d.values():
            ctx.free(p)


def run_group(x3, ctx, name):
    """every case of the group on `ctx` -> the number of cases run"""
    done = 0
    probe = ctx.alloc(48)                       # (the fence is on in this process: a fresh buffer holds the fill)
    assert (ctx.download(probe, 48) == FILL).all(), "X3HIP_FENCE and X3HIP_FENCE_FILL are not in force"
    ctx.free(probe)
    for s, cases in group(name):
        src = Source(x3, ctx, s)
        try:
            for case in cases:
                run_case(x3, ctx, src, case)
                done += 1
        finally:
            src.close()
    return done
