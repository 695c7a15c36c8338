"""The stalled-stream harness of test_gpu_async_contract.py and its cases (not a test module).

include/x3hip.h promises that the `*_dev` entry points enqueue on the context's stream and do not synchronise.  A test that
uploads, calls and waits never sees the GPU lag behind the host, so an ordering bug cannot show.  Here every case runs on a
caller-owned torch stream S behind a STALL (torch.cuda._sleep): the device buffers a call reads hold a DECOY (content A)
when the host enqueues the call, the real content B arrives by device-to-device copies enqueued on S behind the stall, and
every output is cloned on S behind the call.  A call that reads early, or a side stream that does not wait for its fork,
computes A's results: wrong, but never a wild access -- A is valid content of B's shape, in bounds everywhere.

A case is an object with
    options            {option: value} set on the context
    inputs(which)      {name: np array}: the device buffers the calls read, for content "A" or "B" (same shapes)
    outputs()          {name: bytes}: the device buffers the calls write (filled with CANARY first)
    enqueue(x3, ctx, d, which, probe)   the library calls; d[name] = device pointer; `which` tells a case whose calls take
                       host tables which content's tables to pass; probe() -> True while the stall is still running.  A
                       case whose LAST call waits by contract returns the probe's answer from just before that call
    results(x3, ctx, d, which)   after S.synchronize(): the x3_*_result calls -> {key: value}
    expect(which)      the oracle's answers: {"out": {name: [(byte offset, np array, final_only)]}, "result": {key: value}}
                       final_only segments are compared on the original after results() only, not on the clone
    same_ok            result keys / output names that are the same for A and B by construction (with the reason)
    valid(which)       asserts that the content is in bounds for the shapes the calls use
Everything expected comes from the CPU oracle (oracle_lib, seg_index_ref); nothing here needs a GPU until run_stalled."""
import functools
import time

import numpy as np

import oracle_lib as O
import seg_index_ref as R
from x3_cases import frame_offsets, refresh_crcs

CANARY = 0xC7
SPF = 10_000
F0 = 48
N0 = F0 * SPF
ERR_PAYLOAD_CRC = 14
LOG = []          # lines for the report (profiles/async/contract_tests.txt is one run's)


def log(line):
    LOG.append(line)
    print(line, flush=True)


# ------------------------------------------------------------------------------------------------ content

@functools.lru_cache(maxsize=None)
def wav(which, n=N0, spf=SPF):
    """quiet random walk with a few LOUD frames (white noise: payloads beyond the wave encoder's LDS image, so that the
    dense pass runs behind the encode kernel); A and B differ in every frame and in which frames are loud"""
    rng = np.random.default_rng({"A": 0xA11CE, "B": 0xB0B, "C": 0xC0C0A, "D": 0xD0D0}[which])
    amp = {"A": 3, "B": 6, "C": 2, "D": 9}[which]
    w = np.clip(np.cumsum(rng.integers(-amp, amp + 1, size=n)), -30000, 30000).astype(np.int16)
    for f in {"A": (7, 31), "B": (5, 6, 20), "C": (1,), "D": (2, 40)}[which]:
        if (f + 1) * spf <= n:
            w[f * spf:(f + 1) * spf] = rng.integers(-32768, 32768, size=spf).astype(np.int16)
    w.setflags(write=False)
    return w


def oparams(bl=20, bpf=500):
    return O.Params.make(bl, bpf, (0, 1, 3), (3, 8, 20))


@functools.lru_cache(maxsize=None)
def encoded(which, bl=20, bpf=500, n=N0):
    """the oracle's (stream bytes, frame offsets [F + 1], stats[6]) of wav(which)[:n]"""
    rc, s, st = O.encode(wav(which)[:n], oparams(bl, bpf))
    assert rc == 0
    offs = np.array(frame_offsets(s) + [s.size], dtype=np.uint64)
    return s, offs, [int(v) for v in st]


def padded(arrs):
    """the byte arrays zero-padded to one length (a multiple of 16, at least 64 bytes of slack)"""
    n = (max(a.size for a in arrs) + 64 + 15) // 16 * 16
    return [np.concatenate([a, np.zeros(n - a.size, dtype=np.uint8)]) for a in arrs]


@functools.lru_cache(maxsize=None)
def damaged_b():
    """stream B with a payload-CRC failure in frame 9 and a decode error under valid CRCs in frame 30
    -> (bytes, per-frame status)"""
    s, offs, _ = encoded("B")
    s = s.copy()
    s[int(offs[9]) + 20 + 100] ^= 0x10
    o = int(offs[30])
    plen = int(s[o + 6]) << 8 | int(s[o + 7])
    nsamp = int(s[o + 4]) << 8 | int(s[o + 5])
    clean = s[o + 20:o + 20 + plen].copy()
    rc30 = 0
    for at in range(40, plen - 16, 37):
        s[o + 20:o + 20 + plen] = clean
        s[o + 20 + at:o + 20 + at + 12] = 0
        rc30 = O.decode_frame(s[o + 20:o + 20 + plen], nsamp, oparams())[0]
        if rc30:
            break
    assert rc30, "no zero run made frame 30 fail to decode"
    refresh_crcs(s, o)
    st = np.zeros(F0, dtype=np.int32)
    st[9], st[30] = ERR_PAYLOAD_CRC, rc30
    return s, st


def f32_bits(a):
    return (np.asarray(a, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ cases

class Case:
    options = {}
    same_ok = {}
    waits_in_last_call = False

    def valid(self, which):
        pass

    def cleanup(self):
        pass

    def __repr__(self):
        return self.name


class EncodeCase(Case):
    """x3_encode_dev / x3_encode_dev_seg: bytes, frame offsets, statistics, index words"""

    def __init__(self, route):
        self.name = "encode_" + route
        self.route = route
        self.bl = 19 if route == "general" else 20
        self.n = N0 // (self.bl * 500) * (self.bl * 500) - 3000     # (a short last frame)
        self.options = {"enc_gen": 2 if route == "gen2" else 3}
        self.gen = {"wave": 3, "seg": 3, "gen2": 2, "general": 1}[route]
        self.op = oparams(self.bl)
        self.F = (self.n + self.bl * 500 - 1) // (self.bl * 500)
        self.cap = O.encode_bound(self.n, self.op)
        self.sb = 32

    def inputs(self, which):
        return {"wav": wav(which)[:self.n]}

    def outputs(self):
        o = {"out": self.cap + 16, "off": 8 * (self.F + 1)}
        if self.route == "seg":
            o["seg"] = 8 * R.n_words(self.F, self.op, self.sb)
        return o

    def enqueue(self, x3, ctx, d, which, probe):
        p = x3.Params.make(self.bl, 500)
        if self.route == "seg":
            rc = ctx.encode_dev_seg(d["wav"], self.n, p, d["out"], self.cap, d["seg"], self.sb, 0, d["off"])
        else:
            rc = ctx.encode_dev(d["wav"], self.n, p, d["out"], self.cap, 0, d["off"])
        assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        rc, pos, stats = ctx.encode_result()
        gen = ctx.get_option("enc_gen_in_use")
        assert gen in (self.gen, 0), gen        # (0: a launch that gave up its bounded wait and was redone in two passes)
        return {"rc": rc, "pos": pos, "stats": [int(v) for v in stats]}

    def expect(self, which):
        s, offs, st = encoded(which, self.bl, 500, self.n)
        out = {"out": [(0, s, False)], "off": [(0, offs, False)]}
        if self.route == "seg":
            out["seg"] = [(0, R.build(s, offs[:-1], self.op, self.sb)[0], False)]
        return {"out": out, "result": {"rc": 0, "pos": int(s.size), "stats": st}}


P_S = (20, 50)      # frames of 1 000 samples for the frame-table cases


@functools.lru_cache(maxsize=None)
def frame_table(k):
    """table k of x3_encode_frames_dev: 300 frames anywhere in the samples (even offsets), 1 .. 1 000 samples each"""
    rng = np.random.default_rng(7000 + k)
    n = rng.integers(1, 1001, size=300).astype(np.uint32)
    n[::5] = 1000
    off = (rng.integers(0, (N0 - 1000) // 2, size=300) * 2).astype(np.uint64)
    return off, n


@functools.lru_cache(maxsize=None)
def frames_encoded(which, k):
    off, n = frame_table(k)
    op = oparams(*P_S)
    parts, st = [], np.zeros(6, dtype=np.uint64)
    for o, m in zip(off, n):
        rc, s, t = O.encode(wav(which)[int(o):int(o) + int(m)], op)
        assert rc == 0
        parts.append(s)
        st += t
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts), offs, [int(v) for v in st]


class EncodeFramesPair(Case):
    """two x3_encode_frames_dev calls with different tables right behind each other: the second call's host copy must
    not reach the first call's pinned table.  The second call waits (on the host) for the first call's copy of the
    table, which stands behind the stall: the stall is proven in front of it"""
    name = "encode_frames_pair"
    waits_in_last_call = True

    def __init__(self):
        self.cap = 300 * (20 + 2 * 1000 + 64) + 64

    def inputs(self, which):
        return {"wav": wav(which)}

    def outputs(self):
        return {"out1": self.cap, "off1": 8 * 301, "out2": self.cap, "off2": 8 * 301}

    def enqueue(self, x3, ctx, d, which, probe):
        p = x3.Params.make(*P_S)
        o1, n1 = frame_table(1)
        o2, n2 = frame_table(2)
        assert ctx.encode_frames_dev(d["wav"], o1, n1, p, d["out1"], self.cap, 0, d["off1"]) == 0, ctx.last_error()
        still = probe()
        assert ctx.encode_frames_dev(d["wav"], o2, n2, p, d["out2"], self.cap, 0, d["off2"]) == 0, ctx.last_error()
        return still

    def results(self, x3, ctx, d, which):
        rc, pos, stats = ctx.encode_result()
        return {"rc": rc, "pos": pos, "stats": [int(v) for v in stats]}

    def expect(self, which):
        s1, f1, _ = frames_encoded(which, 1)
        s2, f2, st2 = frames_encoded(which, 2)
        return {"out": {"out1": [(0, s1, False)], "off1": [(0, f1, False)], "out2": [(0, s2, False)], "off2": [(0, f2, False)]},
                "result": {"rc": 0, "pos": int(s2.size), "stats": st2}}


class EncodeDecode(Case):
    """x3_encode_dev, then x3_decode_dev of its stream with no x3_encode_result in between"""
    name = "encode_then_decode"

    def __init__(self):
        self.cap = O.encode_bound(N0, oparams())

    def inputs(self, which):
        return {"wav": wav(which)}

    def outputs(self):
        return {"out": self.cap + 16, "off": 8 * (F0 + 1), "back": 2 * N0, "st": 4 * F0}

    def _decode(self, x3, ctx, d):
        p = x3.Params.default()
        assert ctx.decode_dev(d["out"], self.cap, d["off"], F0, p, d["back"], N0, n_per_clip=N0, d_status=d["st"]) == 0

    def enqueue(self, x3, ctx, d, which, probe):
        assert ctx.encode_dev(d["wav"], N0, x3.Params.default(), d["out"], self.cap, 0, d["off"]) == 0, ctx.last_error()
        self._decode(x3, ctx, d)

    def results(self, x3, ctx, d, which):
        fb = ctx.get_option("encode_fallbacks")
        rc, pos, stats = ctx.encode_result()
        dec = ctx.decode_result()
        if ctx.get_option("encode_fallbacks") != fb:    # the stream was rewritten under the decoder: decode it again
            self._decode(x3, ctx, d)
            dec = ctx.decode_result()
        return {"rc": rc, "pos": pos, "stats": [int(v) for v in stats], "decode": tuple(dec)}

    def expect(self, which):
        s, offs, st = encoded(which)
        out = {"out": [(0, s, False)], "off": [(0, offs, False)], "back": [(0, wav(which), False)],
               "st": [(0, np.zeros(F0, dtype=np.int32), False)]}
        return {"out": out, "result": {"rc": 0, "pos": int(s.size), "stats": st, "decode": (0, F0, 0, N0)}}

    same_ok = {"st": "both streams are intact: every status is 0", "decode": "both streams are intact"}


class DecodeCase(Case):
    """x3_decode_dev of a stream with one payload-CRC failure and one decode error under valid CRCs (A: intact): every
    decoder kernel, the check pass on either stream and in either launch order"""

    def __init__(self, kernel, check_main, check_first):
        self.name = "decode_%s_main%d_first%d" % (kernel, check_main, check_first)
        self.kernel = kernel
        self.options = {"check_main": check_main, "check_first": check_first,
                        "decode_blocks": int(kernel == "blocks"), "decode_single": int(kernel == "single")}
        self.kernel_in_use = {"default": (2,), "blocks": (3,), "single": (1, 0), "offsets": (1, 0)}[kernel]
        a, b = padded([encoded("A")[0], damaged_b()[0]])
        self.x3 = {"A": a, "B": b}
        self.len = a.size

    def wav_offsets(self, which):
        f = np.arange(F0, dtype=np.uint64)
        return (f if which == "A" else np.uint64(F0 - 1) - f) * np.uint64(SPF)

    def inputs(self, which):
        i = {"x3": self.x3[which], "off": encoded(which)[1]}
        if self.kernel == "offsets":
            i["wo"] = self.wav_offsets(which)
        return i

    def outputs(self):
        return {"back": 2 * N0, "st": 4 * F0}

    def enqueue(self, x3, ctx, d, which, probe):
        p = x3.Params.default()
        if self.kernel == "offsets":
            rc = ctx.decode_dev(d["x3"], self.len, d["off"], F0, p, d["back"], N0, d_wav_offsets=d["wo"], d_status=d["st"])
        else:
            rc = ctx.decode_dev(d["x3"], self.len, d["off"], F0, p, d["back"], N0, n_per_clip=N0, d_status=d["st"])
        assert rc == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        r = ctx.decode_result()
        assert ctx.get_option("decode_kernel_in_use") in self.kernel_in_use
        return {"decode": tuple(r)}

    def expect(self, which):
        st = np.zeros(F0, dtype=np.int32) if which == "A" else damaged_b()[1]
        pos = self.wav_offsets(which) if self.kernel == "offsets" else np.arange(F0, dtype=np.uint64) * np.uint64(SPF)
        w = wav(which)
        back = [(2 * int(pos[f]), w[f * SPF:(f + 1) * SPF], False) for f in range(F0) if st[f] == 0]
        bad = np.flatnonzero(st)
        res = (0, int(bad[0]), int(st[bad[0]]), int(bad[0]) * SPF) if bad.size else (0, F0, 0, N0)
        return {"out": {"back": back, "st": [(0, st, False)]}, "result": {"decode": res}}

    def valid(self, which):
        offs = encoded(which)[1]
        assert int(offs[-1]) <= self.len and np.all(np.diff(offs.astype(np.int64)) >= 22)
        assert int(self.wav_offsets(which).max()) + SPF <= N0


class SegCase(Case):
    """x3_seg_index_build_dev, x3_decode_dev_seg recording an index, x3_decode_dev_seg by that index, x3_sample_offsets_dev"""
    name = "seg_index_build_record_decode"
    SB = 32

    def __init__(self):
        a, b = padded([encoded("A")[0], encoded("B")[0]])
        self.x3 = {"A": a, "B": b}
        self.len = a.size
        self.nw = R.n_words(F0, oparams(), self.SB)

    def inputs(self, which):
        return {"x3": self.x3[which], "off": encoded(which)[1]}

    def outputs(self):
        return {"built": 8 * self.nw, "rec": 8 * self.nw, "back1": 2 * N0, "back2": 2 * N0, "st1": 4 * F0, "st2": 4 * F0,
                "so": 8 * (F0 + 1)}

    def enqueue(self, x3, ctx, d, which, probe):
        p = x3.Params.default()
        assert ctx.seg_index_build_dev(d["x3"], self.len, d["off"], F0, p, d["built"], self.SB) == 0, ctx.last_error()
        assert ctx.sample_offsets_dev(d["x3"], self.len, d["off"], F0, d["so"]) == 0
        assert ctx.decode_dev_seg(d["x3"], self.len, d["off"], F0, p, d["back1"], N0, d["rec"], self.SB, record=True,
                                  n_per_clip=N0, d_status=d["st1"]) == 0, ctx.last_error()
        assert ctx.decode_dev_seg(d["x3"], self.len, d["off"], F0, p, d["back2"], N0, d["rec"], self.SB, record=False,
                                  n_per_clip=N0, d_status=d["st2"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"decode": tuple(ctx.decode_result()), "irregular": ctx.get_option("last_seg_index_irregular")}

    def expect(self, which):
        s, offs, _ = encoded(which)
        words = R.build(s, offs[:-1], oparams(), self.SB)[0]
        z = np.zeros(F0, dtype=np.int32)
        so = np.arange(F0 + 1, dtype=np.uint64) * np.uint64(SPF)
        out = {"built": [(0, words, False)], "rec": [(0, words, False)], "back1": [(0, wav(which), False)],
               "back2": [(0, wav(which), False)], "st1": [(0, z, False)], "st2": [(0, z, False)], "so": [(0, so, False)]}
        return {"out": out, "result": {"decode": (0, F0, 0, N0), "irregular": 0}}

    same_ok = {"st1": "intact streams", "st2": "intact streams", "decode": "intact streams", "irregular": "intact streams",
               "so": "both contents are cut into the same full frames"}


class WindowsPair(Case):
    """x3_sample_offsets_dev, then two x3_decode_windows_dev calls with different starts (int16 rows, then float rows):
    the stream, its frame offsets and the starts are device data and arrive behind the stall"""
    name = "windows_pair"
    W, L = 64, 4000

    def __init__(self):
        a, b = padded([encoded("A")[0], encoded("B")[0]])
        self.x3 = {"A": a, "B": b}
        self.len = a.size

    def starts(self, which, k):
        rng = np.random.default_rng({"A": 10, "B": 20}[which] + k)
        s = rng.integers(0, N0 - self.L + 1, size=self.W).astype(np.uint64)
        s[0], s[1] = 0, N0 - self.L
        return s

    def inputs(self, which):
        return {"x3": self.x3[which], "off": encoded(which)[1], "starts1": self.starts(which, 1),
                "starts2": self.starts(which, 2)}

    def outputs(self):
        return {"so": 8 * (F0 + 1), "rows1": 2 * self.W * self.L, "st1": 4 * self.W, "rows2": 4 * self.W * self.L,
                "st2": 4 * self.W}

    def enqueue(self, x3, ctx, d, which, probe):
        p = x3.Params.default()
        assert ctx.sample_offsets_dev(d["x3"], self.len, d["off"], F0, d["so"]) == 0
        assert ctx.decode_windows_dev(d["x3"], self.len, d["off"], d["so"], F0, p, d["starts1"], self.W, self.L, d["rows1"],
                                      x3.WINDOW_I16, d["st1"]) == 0, ctx.last_error()
        assert ctx.decode_windows_dev(d["x3"], self.len, d["off"], d["so"], F0, p, d["starts2"], self.W, self.L, d["rows2"],
                                      x3.WINDOW_F32, d["st2"]) == 0, ctx.last_error()

    def results(self, x3, ctx, d, which):
        return {"windows": tuple(ctx.decode_windows_result())}

    def expect(self, which):
        w = wav(which)
        r1 = np.stack([w[int(s):int(s) + self.L] for s in self.starts(which, 1)])
        r2 = np.stack([f32_bits(w[int(s):int(s) + self.L]) for s in self.starts(which, 2)])
        z = np.zeros(self.W, dtype=np.int32)
        so = np.arange(F0 + 1, dtype=np.uint64) * np.uint64(SPF)
        out = {"so": [(0, so, False)], "rows1": [(0, r1, False)], "st1": [(0, z, False)], "rows2": [(0, r2, False)],
               "st2": [(0, z, False)]}
        return {"out": out, "result": {"windows": (0, 0, self.W, 0)}}

    same_ok = {"so": "both contents are cut into the same full frames", "st1": "intact streams", "st2": "intact streams",
               "windows": "intact streams"}

    def valid(self, which):
        for k in (1, 2):
            assert int(self.starts(which, k).max()) + self.L <= N0
        assert int(encoded(which)[1][-1]) <= self.len


# ---- batches of streams: the entry table is a HOST array of the call, so A's entries must have B's lengths.  Frames are
# independent, so the frames of a clean entry in reverse order are a clean entry of the same length with other samples.

ENTRY_SAMPLES = (25_000, 12_000, 30_000, 14_000, 21_000, 17_000)
ROW_LEN = 30_000


@functools.lru_cache(maxsize=None)
def entries(which, damaged, codes=(0, 1, 3), thr=(3, 8, 20)):
    """-> (buffer with 16 bytes of slack, offsets, lengths, [entry bytes])"""
    op = O.Params.make(20, 500, codes, thr)
    ents = []
    for e, n in enumerate(ENTRY_SAMPLES):
        w = wav("B")[e * 70_000:e * 70_000 + n]
        if e == 4:
            w = np.random.default_rng(44).integers(-32768, 32768, size=n).astype(np.int16)   # a loud entry
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        offs = frame_offsets(s) + [s.size]
        if which == "A":
            s = np.concatenate([s[offs[f]:offs[f + 1]] for f in reversed(range(len(offs) - 1))])
        elif damaged and e == 2:
            s = s.copy()
            s[offs[1] + 20 + 50] ^= 0x04          # the second frame's payload CRC fails
        ents.append(s)
    lens = [int(s.size) for s in ents]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    buf = np.concatenate(ents + [np.zeros(16, dtype=np.uint8)])
    return buf, offs, lens, ents


class StreamsCase(Case):
    """x3_decode_streams_dev, default codes and a row_len that is a multiple of 4 (no host trip): a clean batch, or one
    with a damaged entry between clean ones (that entry takes the general walk inside x3_decode_streams_result: its row
    and result are final only then).  pair: the batch as two calls right behind each other, the later one replacing the
    pending one; the second waits for the first one's table copy, so the stall is proven in front of it"""

    def __init__(self, fmt, damaged=False, pair=False):
        self.name = "streams_%s%s%s" % ("f32" if fmt else "i16", "_damaged" if damaged else "", "_pair" if pair else "")
        self.fmt, self.damaged, self.pair = fmt, damaged, pair
        self.waits_in_last_call = pair
        self.esz = 4 if fmt else 2
        self.E = len(ENTRY_SAMPLES)

    def inputs(self, which):
        return {"x3": entries(which, self.damaged)[0]}

    def outputs(self):
        return {"rows": self.esz * self.E * ROW_LEN, "res": 24 * self.E}

    def enqueue(self, x3, ctx, d, which, probe):
        buf, offs, lens, _ = entries(which, self.damaged)
        p = x3.Params.default()
        if not self.pair:
            assert ctx.decode_streams_dev(d["x3"], buf.size - 16, offs, lens, p, d["rows"], ROW_LEN, self.fmt, d["res"]) == 0
            return None
        h = self.E // 2
        assert ctx.decode_streams_dev(d["x3"], buf.size - 16, offs[:h], lens[:h], p, d["rows"], ROW_LEN, self.fmt,
                                      d["res"]) == 0, ctx.last_error()
        still = probe()
        assert ctx.decode_streams_dev(d["x3"], buf.size - 16, offs[h:], lens[h:], p, d["rows"] + self.esz * h * ROW_LEN,
                                      ROW_LEN, self.fmt, d["res"] + 24 * h) == 0, ctx.last_error()
        return still

    def results(self, x3, ctx, d, which):
        return {"streams": tuple(ctx.decode_streams_result())}

    def expect(self, which):
        _, _, _, ents = entries(which, self.damaged)
        rows, res, bad = [], [], []
        dt = np.dtype([("n_out", "<u8"), ("frames_ok", "<u8"), ("status", "<i4"), ("frame_errors", "<u4")])
        first = self.E // 2 if self.pair else 0     # (the summary is the last call's)
        for e, s in enumerate(ents):
            rc, w, fok, ferr = O.decode_stream(s, oparams(), wav_cap=ROW_LEN)
            full = np.zeros(ROW_LEN, dtype=np.int16)
            full[:w.size] = w
            late = bool(rc or ferr)                 # not one clean chain of good frames: the general walk, at result time
            rows.append((self.esz * e * ROW_LEN, f32_bits(full) if self.fmt else full, late))
            res.append((24 * e, np.array([(w.size, fok, rc, ferr)], dtype=dt), late))
            if rc and e >= first:
                bad.append((e - first, rc))
        n = self.E - first
        summary = (0, len(bad), bad[0][0] if bad else n, bad[0][1] if bad else 0)
        return {"out": {"rows": rows, "res": res}, "result": {"streams": summary}}

    def valid(self, which):
        buf, offs, lens, ents = entries(which, self.damaged)
        assert lens == entries("B", self.damaged)[2] and offs[-1] + lens[-1] == buf.size - 16
        if which == "A":
            for s in ents:
                rc, w, fok, ferr = O.decode_stream(s, oparams(), wav_cap=ROW_LEN)
                assert (rc, ferr) == (0, 0) and fok >= 2

    @property
    def same_ok(self):
        return {} if self.damaged else {"streams": "clean batches",
                                           "res": "A's entries are B's frames in another order: the same counts"}


class TunerCase(Case):
    """x3_tuner_add_dev twice under one stall, then x3_tuner_result: candidates' totals against the oracle's encoded sizes"""
    name = "tuner_add_twice"
    CANDS = (0, 500, 1188, 1500, 2183)
    HALF = N0 // 2
    tuner = None

    def inputs(self, which):
        return {"wav": wav(which)}

    def outputs(self):
        return {}

    def cleanup(self):
        if self.tuner is not None:
            self.tuner.close()
            self.tuner = None

    def enqueue(self, x3, ctx, d, which, probe):
        if self.tuner is None:
            self.tuner = x3.Tuner(ctx, SPF)       # (allocates: made in the warm-up pass)
        assert self.tuner.add_dev(d["wav"], self.HALF) == 0
        assert self.tuner.add_dev(d["wav"] + 2 * self.HALF, N0 - self.HALF) == 0

    def results(self, x3, ctx, d, which):
        rc, best, best_bytes, sizes = self.tuner.result()
        assert self.tuner.reset() == 0
        assert rc == 0 and best_bytes == int(sizes.min())
        return {"sizes": [int(sizes[i]) for i in self.CANDS]}

    @staticmethod
    def candidate(index, spf=SPF):
        """include/x3hip.h, "CANDIDATES": index = g * 728 + the rank of (t0, t1, t2) in lexicographic order"""
        g, r = divmod(index, 728)
        trip = [(a, b, c) for a in range(7) for b in range(a, 11) for c in range(15, 28)]
        assert len(trip) == 728
        bl = (10, 20, 40)[g]
        return O.Params.make(bl, spf // bl, (0, 1, 3), trip[r])

    def expect(self, which):
        w = wav(which)
        sizes = []
        for i in self.CANDS:
            op = self.candidate(i)
            sizes.append(sum(int(O.encode(part, op)[1].size) for part in (w[:self.HALF], w[self.HALF:])))
        return {"out": {}, "result": {"sizes": sizes}}


class SynthCase(Case):
    """x3_synth_dev: no input buffer; the warm-up pass and the pass under test ask for different signals.  The oracle has
    no generator: the expected samples are the library's host version, which the header declares bit-identical"""
    name = "synth"
    N = 300_001
    ARGS = {"A": (2, 5, 0), "B": (2, 77, 1234)}

    def inputs(self, which):
        return {}

    def outputs(self):
        return {"out": 2 * self.N}

    def enqueue(self, x3, ctx, d, which, probe):
        kind, seed, start = self.ARGS[which]
        ctx.synth_dev(kind, seed, start, self.N, d["out"])

    def results(self, x3, ctx, d, which):
        return {}

    def expect(self, which):
        import x3hip
        kind, seed, start = self.ARGS[which]
        return {"out": {"out": [(0, x3hip.synth(kind, seed, start, self.N), False)]}, "result": {}}


class CorpusWindows(Case):
    """x3_corpus_windows_dev in both formats over a corpus built in the warm-up pass (x3_corpus_build waits: it is no part
    of the pass under test): the entries and starts are device data and arrive behind the stall"""
    name = "corpus_windows"
    W, L = 48, 1500
    corpus = None

    def table(self, which):
        rng = np.random.default_rng({"A": 12, "B": 21}[which])
        e = rng.integers(0, len(ENTRY_SAMPLES), size=self.W).astype(np.uint32)
        return e, np.array([rng.integers(0, ENTRY_SAMPLES[k] - self.L + 1) for k in e], dtype=np.uint64)

    def inputs(self, which):
        e, s = self.table(which)
        return {"ent": e, "starts": s}

    def outputs(self):
        return {"rows1": 2 * self.W * self.L, "st1": 4 * self.W, "rows2": 4 * self.W * self.L, "st2": 4 * self.W}

    def enqueue(self, x3, ctx, d, which, probe):
        if self.corpus is None:
            buf, offs, lens, _ = entries("B", False)
            self.ctx, self.d_x3 = ctx, ctx.alloc(buf.size)
            ctx.upload(self.d_x3, buf)
            self.corpus = x3.Corpus(ctx, (self.d_x3, buf.size - 16), offs, lens, x3.Params.default(), seg_blocks=32)
        for fmt, rows, st in ((x3.WINDOW_I16, "rows1", "st1"), (x3.WINDOW_F32, "rows2", "st2")):
            assert self.corpus.decode_into(d["ent"], d["starts"], self.W, self.L, d[rows], fmt, d[st]) == 0, ctx.last_error()

    def cleanup(self):
        if self.corpus is not None:
            self.corpus.close()
            self.ctx.free(self.d_x3)
            self.corpus = None

    def results(self, x3, ctx, d, which):
        return {"windows": tuple(ctx.decode_windows_result())}

    def expect(self, which):
        ents = entries("B", False)[3]
        e, s = self.table(which)
        wavs = [O.decode_stream(b, oparams(), wav_cap=ROW_LEN)[1] for b in ents]
        rows = np.stack([wavs[k][int(s0):int(s0) + self.L] for k, s0 in zip(e, s)])
        z = np.zeros(self.W, dtype=np.int32)
        out = {"rows1": [(0, rows, False)], "st1": [(0, z, False)], "rows2": [(0, f32_bits(rows), False)], "st2": [(0, z, False)]}
        return {"out": out, "result": {"windows": (0, 0, self.W, 0)}}

    same_ok = {"st1": "every window lies inside its clean entry", "st2": "every window lies inside its clean entry",
               "windows": "every window lies inside its clean entry"}

    def valid(self, which):
        e, s = self.table(which)
        assert all(int(s0) + self.L <= ENTRY_SAMPLES[k] for k, s0 in zip(e, s)) and int(e.max()) < len(ENTRY_SAMPLES)


CASES = ([EncodeCase(r) for r in ("wave", "gen2", "general", "seg")] + [EncodeFramesPair(), EncodeDecode()] +
         [DecodeCase(k, m, f) for k in ("default", "blocks", "single", "offsets") for m in (0, 1) for f in (0, 1)] +
         [SegCase(), WindowsPair(), StreamsCase(0), StreamsCase(1), StreamsCase(0, damaged=True),
          StreamsCase(1, damaged=True), StreamsCase(0, pair=True), TunerCase(), SynthCase(), CorpusWindows()])


def flat(segs):
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for _, a, _ in segs]) if segs else \
        np.zeros(0, dtype=np.uint8)


def check_pair_differs(case):
    """the precondition of a case: every compared output of the oracle differs between A and B, A is valid for B's shapes"""
    a, b = case.expect("A"), case.expect("B")
    ia, ib = case.inputs("A"), case.inputs("B")
    assert ia.keys() == ib.keys()
    for k in ia:
        assert ia[k].shape == ib[k].shape and ia[k].dtype == ib[k].dtype, (case, k)
        assert not np.array_equal(ia[k], ib[k]), (case, k, "the decoy is the content")
    assert a["out"].keys() == b["out"].keys() == case.outputs().keys()
    for name in a["out"]:
        for segs in (a["out"][name], b["out"][name]):
            for off, arr, _ in segs:
                assert off + np.ascontiguousarray(arr).nbytes <= case.outputs()[name], (case, name)
        if name not in case.same_ok:
            assert not np.array_equal(flat(a["out"][name]), flat(b["out"][name])), (case, name)
    for key in a["result"]:
        if key not in case.same_ok and key != "rc":      # (the call's own status: X3_OK for both)
            assert a["result"][key] != b["result"][key], (case, key)
    for key in case.same_ok:
        assert key in a["out"] or key in a["result"], (case, key)
    case.valid("A")
    case.valid("B")


# ------------------------------------------------------------------------------------------------ the harness

def calibrate_sleep(torch):
    """cycles of torch.cuda._sleep per millisecond on this device, by two events"""
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    cycles = 20_000_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(cycles)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.05, "torch.cuda._sleep(%d) took %.3f ms: it does not stall this device" % (cycles, ms)
    log("calibration: torch.cuda._sleep(%d) = %.3f ms -> %.0f cycles per ms" % (cycles, ms, cycles / ms))
    return cycles / ms


def _compare(case, which, exp, clones, outs, res, clones_final):
    for name, segs in exp["out"].items():
        final = outs[name].cpu().numpy()
        early = clones[name].cpu().numpy()
        any_late = False
        for off, arr, late in segs:
            want = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            got = final[off:off + want.size]
            assert np.array_equal(got, want), "%s %s: %s differs from the oracle at byte %d (+%d)" % (
                case, which, name, off, int(np.flatnonzero(got != want)[0]))
            any_late = any_late or late
            if clones_final and not late:
                got = early[off:off + want.size]
                assert np.array_equal(got, want), "%s %s: the clone of %s, taken in stream order, differs from the oracle " \
                    "at byte %d (+%d)" % (case, which, name, off, int(np.flatnonzero(got != want)[0]))
        if clones_final and not any_late:
            assert np.array_equal(final, early), "%s %s: %s changed after its clone was taken" % (case, which, name)
    for key, want in exp["result"].items():
        assert res[key] == want, "%s %s: %s is %r, the oracle says %r" % (case, which, key, res[key], want)


def run_stalled(x3, torch, case, cycles_per_ms):
    """the warm-up pass with content A (synced), then the pass under test: stall, copies of B, the calls, clones -- and
    only then a wait.  The stall is proven by an event recorded right behind it that has not completed when the last
    enqueue has returned; an unproven pass is run again with the stall doubled, three times at most, then fails."""
    S = torch.cuda.Stream()
    ctx = x3.Context(0, stream=S.cuda_stream)
    try:
        with torch.cuda.stream(S):
            for k, v in case.options.items():
                ctx.set_option(k, v)

            def dev(a):
                return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
            src = {w: {k: dev(v) for k, v in case.inputs(w).items()} for w in ("A", "B")}
            work = {k: torch.empty_like(v) for k, v in src["A"].items()}
            outs = {k: torch.empty(max(n, 8), dtype=torch.uint8, device="cuda") for k, n in case.outputs().items()}
            d = {k: t.data_ptr() for k, t in list(work.items()) + list(outs.items())}

            def reset():
                for k, t in work.items():
                    t.copy_(src["A"][k])
                for t in outs.values():
                    t.fill_(CANARY)
                S.synchronize()

            reset()
            fb0 = ctx.get_option("encode_fallbacks")
            t0 = time.perf_counter()
            case.enqueue(x3, ctx, d, "A", lambda: True)
            clones = {k: t.clone() for k, t in outs.items()}
            enqueue_ms = (time.perf_counter() - t0) * 1e3
            S.synchronize()
            res = case.results(x3, ctx, d, "A")
            fell = ctx.get_option("encode_fallbacks") - fb0
            assert fell in (0, 1)
            _compare(case, "warm-up A", case.expect("A"), clones, outs, res, not fell)

            stall_ms = max(5.0, 4.0 * enqueue_ms)
            for attempt in range(4):
                reset()
                fb0 = ctx.get_option("encode_fallbacks")
                torch.cuda._sleep(int(stall_ms * cycles_per_ms))
                behind = torch.cuda.Event()
                behind.record(S)
                for k, t in work.items():
                    t.copy_(src["B"][k], non_blocking=True)
                early = case.enqueue(x3, ctx, d, "B", lambda: not behind.query())
                clones = {k: t.clone() for k, t in outs.items()}
                running = not behind.query()
                proven = bool(early) if case.waits_in_last_call else running
                S.synchronize()
                res = case.results(x3, ctx, d, "B")
                fell = ctx.get_option("encode_fallbacks") - fb0
                log("case %-34s enqueue %.3f ms  stall %.1f ms  query() == False %s: %s%s" % (
                    case.name, enqueue_ms, stall_ms,
                    "in front of the last call (it waits for the table copy)" if case.waits_in_last_call
                    else "after the last enqueue", "proven" if proven else "NOT proven",
                    "  [encode fallback]" if fell else ""))
                if proven:
                    break
                stall_ms *= 2
            else:
                raise AssertionError("%s: the stall was never proven: the event behind a stall of %.1f ms had completed when "
                                     "the enqueue returned (enqueue of the warm-up pass: %.3f ms)" % (case, stall_ms / 2, enqueue_ms))
            assert fell in (0, 1)
            _compare(case, "B", case.expect("B"), clones, outs, res, not fell)
    finally:
        case.cleanup()
        ctx.close()
