"""The multi-channel extension where tests/test_gpu_multichannel.py does not reach: x3_decode_mc_lanes_kernel's hand-over
decisions, x3_decode_stream_mc's capacities and limits, x3_encode_mc on other code sets, at the 24 KB payload edge and out of
memory.  Everything is `==` against the oracle (oracle_lib: encode_mc, decode_stream_mc, frame_plain(n_ch=)).

DECODER.  x3_decode_stream_mc stops at the first frame that fails, so every crafted frame of the pools (x3_cases.mc_pool;
tests/test_mc_cases.py counts their classes on the CPU) that fails stands in a stream of its own: k clean frames, the frame,
two clean frames, k in {0, 1, 63, 64, 65} -- first lane, last lane, next workgroup.  The frames that decode are chained
between clean frames.  The C ABI is called directly on rows filled with 0x5A5A: status, counts and samples are the oracle's,
the rows are untouched behind n_samples, and option last_decode_replays is exact:
  * on the lanes path the frames that are not plain (frame_plain == 0), those behind the failing frame included -- the
    kernel's five hand-over conditions (index bound, BFP width, zero run of 32 bits, read behind the payload; a frame the
    geometry refuses is BAD_ARG without a replay) each show as a frame the oracle calls not plain.  A frame wrongly kept
    gives other samples or another status; a frame wrongly handed over a count above the oracle's;
  * on the thread paths (option mc_decode_threads, block lengths above 60) every frame the walk takes.
Two geometries of clean frames: sample counts that are multiples of eight (rows 16-byte aligned: the 16-byte stores, every
crafted frame of a chain realigned by the clean frame behind its predecessor) and odd counts (sample-by-sample stores, lanes
of both kinds in one wave)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import x3hip
from test_gpu_code_sets import PIDS, PSETS, content
from x3_cases import (MC_CHANNELS, MC_PIDS, MC_PSETS, PAYLOAD_EDGE, edge_channels, frame_offsets, mc_clean_frames, mc_frame,
                      mc_params, mc_pool, mc_verdict, refresh_crcs)

pytestmark = pytest.mark.gpu

FILL = 0x5A5A
REPLAYS = {}   # parameter set -> [frames walked, frames handed over, crafted plain frames kept] on the lanes path


@pytest.fixture(scope="module")
def ctx():
    c = x3hip.Context(0)
    yield c
    c.close()


def xparams(op):
    return x3hip.Params.make(op.block_len, op.blocks_per_frame, tuple(op.codes), tuple(op.thresholds))


def decode_raw(ctx, stream, n_ch, p, cap, room=0):
    """x3_decode_stream_mc itself on rows of cap + room samples filled with 0x5A5A
    -> (rc, rows, n_samples, frames_ok, frame_errors, last_decode_replays)"""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    rows = [np.full(cap + room, FILL, dtype=np.int16) for _ in range(n_ch)]
    ptrs = (C.c_void_p * n_ch)(*[r.ctypes.data for r in rows])
    n, fok, ferr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = x3hip.lib()
    L.x3_decode_stream_mc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.x3_decode_stream_mc(ctx._h, stream.ctypes.data, stream.size, n_ch, C.byref(p), ptrs, cap, C.byref(n),
                               C.byref(fok), C.byref(ferr))
    return rc, rows, n.value, fok.value, ferr.value, ctx.get_option("last_decode_replays")


def both_paths(ctx, stream, n_ch, op, cap, want, lanes, nonplain, walked, tag, room=0):
    """the default path and mc_decode_threads = 1 against `want` = (rc, [samples], frames_ok, frame_errors); replays:
    `nonplain` on the lanes path, `walked` on the thread paths (None: not counted); both paths agree"""
    p = xparams(op)
    got = []
    for threads in ((0, 1) if lanes else (0,)):
        ctx.set_option("mc_decode_threads", threads)
        try:
            rc, rows, n, fok, ferr, rep = decode_raw(ctx, stream, n_ch, p, cap, room)
        finally:
            ctx.set_option("mc_decode_threads", 0)
        assert (rc, fok, ferr, n) == (want[0], want[2], want[3], want[1][0].size), \
            (tag, threads, (rc, fok, ferr, n), (want[0], want[2], want[3], want[1][0].size), ctx.last_error())
        for c in range(n_ch):
            assert np.array_equal(rows[c][:n], want[1][c]), (tag, threads, c)
            assert (rows[c][n:] == FILL).all(), (tag, threads, c)
        exp = nonplain if lanes and not threads else walked
        if exp is not None:
            assert rep == exp, (tag, threads, rep, exp)
        got.append((rc, n, fok, ferr, rows))
    if len(got) == 2:
        assert got[0][:4] == got[1][:4] and all(np.array_equal(a, b) for a, b in zip(got[0][4], got[1][4])), tag
    return got[0]


# ------------------------------------------------------------------ B. crafted frames in streams

@pytest.mark.parametrize("n_ch", MC_CHANNELS)
@pytest.mark.parametrize("pi", range(len(MC_PSETS)), ids=MC_PIDS)
def test_crafted_frames_in_streams(ctx, n_ch, pi):
    op = mc_params(MC_PSETS[pi], bpf=100)
    lanes = op.block_len <= 60
    pool = mc_pool(n_ch, pi)
    verdicts = [mc_verdict(pay, n, n_ch, op) for pay, n in pool]
    rng = np.random.default_rng([77, n_ch, pi])
    banks = [mc_clean_frames(rng, op, n_ch, [8 * int(v) for v in rng.integers(4, 76, size=67)]),
             mc_clean_frames(rng, op, n_ch, [2 * int(v) + 1 for v in rng.integers(15, 300, size=67)])]
    fillers = mc_clean_frames(rng, op, n_ch, [48 + r for r in range(8)])   # fillers[r]: r samples past a multiple of eight
    tally = REPLAYS.setdefault(MC_PIDS[pi], [0, 0, 0]) if lanes else [0, 0, 0]

    def run(frames, nonplain, walked, tag):
        """frames: [(frame bytes, samples)]"""
        stream = np.concatenate([f for f, _ in frames])
        cap = sum(m for _, m in frames) + 64
        want = O.decode_stream_mc(stream, n_ch, op, wav_cap=cap)
        both_paths(ctx, stream, n_ch, op, cap, want, lanes, nonplain, walked, tag)
        if lanes:
            tally[0] += walked
            tally[1] += nonplain
        return want

    # every frame that fails, where it stands
    decodes = []
    for j, ((pay, n), (st, _, plain)) in enumerate(zip(pool, verdicts)):
        if st[1] == 1:
            decodes.append(j)
            continue
        bank = banks[j & 1]
        k = (0, 1, 63, 64, 65)[int(rng.integers(0, 5))]
        frames = [(f, w[0].size) for f, w in bank[:k]] + [(mc_frame(pay, n, n_ch), n)] + [(f, w[0].size) for f, w in bank[k:k + 2]]
        refused = n == 0 or pay.size < 2 * n_ch          # the walk ends at a frame no decoder takes (BAD_ARG, no replay)
        want = run(frames, int(plain == 0), k + 1 if refused else k + 3, (n_ch, pi, j, k, pay.size, n))
        assert want[2] == k and (want[0] != 0 or want[3] == 1), (j, k, want[0], want[2:])
        for c in range(n_ch):   # (the clean frames in front are delivered)
            assert np.array_equal(want[1][c], np.concatenate([w[c] for _, w in bank[:k]] + [np.zeros(0, dtype=np.int16)]))
    # the frames that decode, plain or not, chained between clean frames
    assert decodes
    for geom in (0, 1):
        bank = banks[geom]
        step = 30 if geom == 0 else 60
        for at in range(0, len(decodes), step):
            frames = [(f, w[0].size) for f, w in bank[:2]]
            for j in decodes[at:at + step]:
                pay, n = pool[j]
                frames.append((mc_frame(pay, n, n_ch), n))
                if geom == 0:   # the next frame's rows start on a 16-byte boundary again
                    f, w = fillers[-n % 8]
                    frames.append((f, w[0].size))
            frames += [(f, w[0].size) for f, w in bank[2:4]]
            nonplain = sum(verdicts[j][2] == 0 for j in decodes[at:at + step])
            want = run(frames, nonplain, len(frames), (n_ch, pi, "chain", geom, at))
            assert (want[0], want[2], want[3]) == (0, len(frames), 0)
            if lanes:
                tally[2] += len(decodes[at:at + step]) - nonplain


def test_lanes_kernel_keeps_and_hands_over():
    """per parameter set of the lanes path: frames it decoded itself and frames it handed to the reference's reader"""
    print("lanes path, parameter set: [frames walked, handed over, crafted plain frames kept]", REPLAYS)
    if len(REPLAYS) < 6:
        pytest.skip("test_crafted_frames_in_streams did not run in full (-k?)")
    for pid, (walked, handed, kept) in REPLAYS.items():
        assert 0 < handed < walked and kept > 0, (pid, walked, handed, kept)


# ------------------------------------------------------------------ C. streams

@pytest.mark.parametrize("j", [0, 1, 64])
def test_channel_count_changes(ctx, j):
    """j frames of two channels, then one of three: MoreThanOneChannel behind j good frames"""
    op = O.Params.make(20, 100)
    rng = np.random.default_rng(j)
    two = mc_clean_frames(rng, op, 2, [8 * int(v) for v in rng.integers(4, 40, size=j + 1)])
    three = mc_clean_frames(rng, op, 3, [40])
    stream = np.concatenate([f for f, _ in two[:j]] + [three[0][0], two[j][0]])
    cap = sum(w[0].size for _, w in two) + 104
    want = O.decode_stream_mc(stream, 2, op, wav_cap=cap)
    assert (want[0], want[2], want[3]) == (6, j, 0)
    for c in range(2):
        assert np.array_equal(want[1][c], np.concatenate([w[c] for _, w in two[:j]] + [np.zeros(0, dtype=np.int16)]))
    # (no frame in front of the bad header: nothing is launched, and the counter keeps what an earlier call left)
    both_paths(ctx, stream, 2, op, cap, want, True, 0 if j else None, j if j else None, ("channels", j))


def test_wav_cap_edge(ctx):
    """four full frames and a ragged one, three channels: a frame that does not fit behind the samples so far ends the walk
    with BAD_ARG (24), the whole frames in front of it delivered -- x3_decode_stream's rule (include/x3hip.h), which holds
    "also when an early block of that very frame would not have decoded".  There the oracle, which like the reference
    slices the rows block by block (decoder.rs:49), reports the block's error where the first block row still fits; the
    header's rule decides, and the oracle's answer is held to be one of the two."""
    op = O.Params.make(20, 10)
    rng = np.random.default_rng(11)
    n = 4 * 200 + 77
    wavs = [np.cumsum(rng.integers(-9, 10, size=n)).astype(np.int16) for _ in range(3)]
    rc, stream, _ = O.encode_mc(wavs, op)
    assert rc == 0
    offs = frame_offsets(stream)
    ends = [200, 400, 600, 800, n]
    assert len(offs) == 5
    for cap in [n, n - 1, 1] + ends[:4] + [e - 1 for e in ends[:4]]:
        f = sum(e <= cap for e in ends)                     # whole frames that fit
        before = ends[f - 1] if f else 0
        exp = (0, 5, 0) if f == 5 else (24, f, 0)
        want = O.decode_stream_mc(stream, 3, op, wav_cap=cap)
        assert (want[0], want[2], want[3]) == exp and want[1][0].size == before, (cap, want[0], want[2:])
        both_paths(ctx, stream, 3, op, cap, want, True, 0, min(f + 1, 5), ("cap", cap), room=32)
        # the same with the first block row of the frame that does not fit (of the last frame, when all fit) made undecodable
        bad = stream.copy()
        g = min(f, 4)
        bad[offs[g] + 20 + 6:offs[g] + 20 + 18] = 0          # a BFP header of width 1 behind the first samples
        refresh_crcs(bad, offs[g])
        want = O.decode_stream_mc(bad, 3, op, wav_cap=cap)
        assert want[2] == g and want[1][0].size == (ends[g - 1] if g else 0)
        if f == 5:
            assert (want[0], want[3]) == (0, 1)
        else:
            assert (want[0], want[3]) in ((24, 0), (0, 1)), (cap, want[0], want[3])
            assert ((want[0], want[3]) == (24, 0)) == (cap - before < 21), cap   # (the oracle: no room for the block row)
            want = (24, want[1], g, 0)
        both_paths(ctx, bad, 3, op, cap, want, True, None, None, ("cap, bad block", cap), room=32)


@pytest.mark.parametrize("plen", [24576, 24578, 0x7FDF, 0x7FE0])
def test_headers_at_the_limits(ctx, plen):
    """a header that announces 24 576 bytes (taken), 24 578 and 0x7fdf (FrameHeaderInvalidPayloadLen) or 0x7fe0
    (FrameLength), valid header CRC, the data present, one clean frame in front and one behind"""
    bpf, n_ch = PAYLOAD_EDGE[0][:2]
    op = O.Params.make(10, bpf)
    rng = np.random.default_rng(plen)
    clean = mc_clean_frames(rng, op, n_ch, [64, 33])
    if plen == 24576:
        rc, big, _ = O.encode_mc(edge_channels(*PAYLOAD_EDGE[0][:3]), op)
        assert rc == 0 and big.size == 20 + plen
        m = 10 * bpf
    else:
        m = 100
        big = mc_frame(rng.integers(0, 256, size=plen, dtype=np.uint8), m, n_ch)
    stream = np.concatenate([clean[0][0], big, clean[1][0]])
    cap = 64 + m + 33 + 8
    want = O.decode_stream_mc(stream, n_ch, op, wav_cap=cap)
    assert (want[0], want[2], want[3]) == {24576: (0, 3, 0), 24578: (12, 1, 0), 0x7FDF: (12, 1, 0), 0x7FE0: (10, 1, 0)}[plen]
    both_paths(ctx, stream, n_ch, op, cap, want, True, 0, want[2], ("limit", plen))


# ------------------------------------------------------------------ D. encoder

def encode_raw(ctx, wavs, p, cap, start, guard=64):
    """x3_encode_mc itself into cap bytes with `guard` more behind them, all 0xAA -> (rc, buffer, out_pos)"""
    wavs = [np.ascontiguousarray(w, dtype=np.int16) for w in wavs]
    out = np.full(max(cap, 1) + guard, 0xAA, dtype=np.uint8)
    pos = C.c_uint64(0)
    ptrs = (C.c_void_p * len(wavs))(*[w.ctypes.data for w in wavs])
    L = x3hip.lib()
    L.x3_encode_mc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                               C.c_uint64, C.c_void_p, C.c_void_p]
    rc = L.x3_encode_mc(ctx._h, ptrs, len(wavs), wavs[0].size, C.byref(p), out.ctypes.data, cap, start, C.byref(pos), None)
    return rc, out, pos.value


MODES = [("one pass", {}, 1), ("two passes", {"two_pass": 1}, 0), ("look-back gives up", {"lb_drop": 1}, 0)]


def with_mode(ctx, kv, fn):
    for k, v in kv.items():
        ctx.set_option(k, v)
    try:
        return fn()
    finally:
        for k in kv:
            ctx.set_option(k, -1 if k == "lb_drop" else 0)


@pytest.mark.parametrize("codes,thr", PSETS, ids=PIDS)
def test_encode_code_sets(ctx, codes, thr):
    """x3_encode_mc == the oracle's encode_mc on every parameter set of the code-set tests: bytes, statistics, status and
    the generation in use; four whole frames and a ragged one"""
    for bl in (10, 20, 40, 13):
        bpf = 12
        spf = bl * bpf
        n = 4 * spf + spf // 3 + 1
        p, po = x3hip.Params.make(bl, bpf, codes, thr), O.Params.make(bl, bpf, codes, thr)
        for n_ch in MC_CHANNELS:
            wavs = [content(codes, thr, bl, bpf, 100 * bl + 10 * n_ch + c, n) for c in range(n_ch)]
            for sp in (0, 7):
                rc_o, x_o, st_o = O.encode_mc(wavs, po, start_pos=sp)
                assert rc_o == 0
                for name, kv, gen in MODES:
                    before = ctx.get_option("encode_fallbacks")
                    rc, x, st = with_mode(ctx, kv, lambda: ctx.encode_mc(wavs, p, start_pos=sp))
                    what = (bl, n_ch, sp, name)
                    assert rc == 0, (what, rc, ctx.last_error())
                    assert x.size == x_o.size and np.array_equal(x[sp:], x_o[sp:]), what
                    assert st.tolist() == st_o.tolist(), what
                    assert ctx.get_option("enc_gen_in_use") == gen, what
                    assert ctx.get_option("encode_fallbacks") == before + ("lb_drop" in kv), what


@pytest.mark.parametrize("bpf,n_ch,n_lit,plen,status", PAYLOAD_EDGE)
def test_encode_payload_edge(ctx, bpf, n_ch, n_lit, plen, status):
    """payloads of 24 576 and 24 574 bytes are written, 24 578 (fits the frame image in LDS), 24 640 (its last byte) and
    24 642 bytes (past it) are FrameLength; tests/test_mc_cases.py holds the lengths"""
    p, po = x3hip.Params.make(10, bpf), O.Params.make(10, bpf)
    wavs = edge_channels(bpf, n_ch, n_lit)
    rc_o, x_o, st_o = O.encode_mc(wavs, po)
    assert rc_o == status and (status or x_o.size == 20 + plen)
    for name, kv, gen in MODES[:2]:
        rc, x, st = with_mode(ctx, kv, lambda: ctx.encode_mc(wavs, p))
        assert rc == status, (name, rc, ctx.last_error())
        if status == 0:
            assert np.array_equal(x, x_o) and st.tolist() == st_o.tolist(), name


def test_encode_only_the_middle_frame_is_too_long(ctx):
    """three frames of 24 576 bytes, the middle one with one more literal block: FrameLength on both sides"""
    bpf, n_ch, n_lit = PAYLOAD_EDGE[0][:3]
    wavs = edge_channels(bpf, n_ch, n_lit, frames=3)
    at = 10 * bpf + 1 + 10 * 5
    wavs[1][at:at + 10] = wavs[0][at:at + 10]
    p, po = x3hip.Params.make(10, bpf), O.Params.make(10, bpf)
    assert O.encode_mc([w[:10 * bpf] for w in wavs], po)[0] == 0 and O.encode_mc([w[20 * bpf:] for w in wavs], po)[0] == 0
    assert O.encode_mc([w[10 * bpf:20 * bpf] for w in wavs], po)[0] == 10
    rc_o = O.encode_mc(wavs, po)[0]
    assert rc_o == 10
    for name, kv, gen in MODES[:2]:
        assert with_mode(ctx, kv, lambda: ctx.encode_mc(wavs, p))[0] == rc_o, name


def test_encode_insufficient_memory(ctx):
    """x3_encode's prefix guarantee (include/x3hip.h) holds for x3_encode_mc: every frame that fits is complete and in place,
    *out_pos is the end of the last of them, nothing behind it or in front of start_pos is touched"""
    p, po = x3hip.Params.make(20, 10), O.Params.make(20, 10)
    rng = np.random.default_rng(5)
    n = 4 * 200 + 77
    wavs = [np.cumsum(rng.integers(-30, 31, size=n)).astype(np.int16) for _ in range(3)]
    for start in (0, 7):
        rc, full, _ = O.encode_mc(wavs, po, start_pos=start)
        assert rc == 0
        ends = [start + (start & 1)] + [start + (start & 1) + o for o in frame_offsets(full[start + (start & 1):])[1:]] + [full.size]
        assert len(ends) == 6
        caps = [start, start + 1, start + 19, start + 21] + ends[1:5] + [e + 1 for e in ends[1:5]] + \
               [ends[2] - 1, ends[3] + 20, full.size - 2, full.size - 1]
        for cap in caps:
            rc_o, got_o, _ = O.encode_mc(wavs, po, start_pos=start, cap=cap)
            assert rc_o == 22, (start, cap, rc_o)
            want_end = max([e for e in ends if e <= cap] + [start])
            for name, kv, gen in MODES[:2]:
                rc, out, pos = with_mode(ctx, kv, lambda: encode_raw(ctx, wavs, p, cap, start))
                what = (start, cap, name)
                assert rc == 22, (what, rc, ctx.last_error())
                assert pos == want_end, (what, pos, want_end)
                assert np.array_equal(out[start:want_end], full[start:want_end]), what
                assert np.all(out[:start] == 0xAA) and np.all(out[want_end:] == 0xAA), what
                assert ctx.get_option("encode_needed_pos") == full.size, what
        # with room for all of it: the same bytes, nothing behind them
        rc, out, pos = encode_raw(ctx, wavs, p, full.size, start)
        assert rc == 0 and pos == full.size and np.array_equal(out[start:pos], full[start:]) and np.all(out[pos:] == 0xAA)
        assert np.all(out[:start] == 0xAA)


# ------------------------------------------------------------------ E. the fuzz tool's family m

def test_fuzz_family_m(ctx):
    """tools/fuzz_parity.py, family m (not in the soak slice of test_gpu_parity.py): 60 trials, code sets and thresholds drawn"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
    spec = importlib.util.spec_from_file_location("fuzz_parity_m", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    counts = mod.run(seed=7, trials=60, families="m", context=ctx)
    assert counts["m"] == 60 and sum(counts.values()) == 60, counts
