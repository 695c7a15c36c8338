"""What the four decoders do once per frame, in front of their hot loops (x3-rust_amd/csrc/x3_decode_frame.h: header check,
sample count and payload length, the frame's place in the output, the origin of its input ring), must come out the same on
all of them: the block-per-lane kernel (3), the three-wave kernel (2), the single-wave fast kernel (1) and the general
single-wave kernel (0, reached by a code set whose Rice codewords can pass 32 bits).

One stream of 70 short frames -- more than a group of 64, so that a wave holds present and absent lanes --, one sample count
per frame around 40, one frame of a single sample, a ragged last frame, one frame whose payload lost a byte of trailing
zero bits (the decoder hands it to the reference's reader: x3_decode_merge_kernel must find the same row).  Seven variants
of it, each decoded in the batch layout (two clips, a stride larger than the clip) and through caller-supplied sample
offsets, by every kernel; per-frame statuses against the oracle's verdicts, the output buffer byte for byte against the
oracle's samples in the good frames' rows and the pre-filled pattern everywhere else.  The same list once more in a child
process under guard pages (test_gpu_fence.py), on a stream whose last frame is one sample ending on a 16-byte boundary
at the very end of its buffer."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_lib as O
from x3_cases import refresh_crcs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

F = 70
FPC = 35                       # frames per clip of the batch layout: two clips
SPF = 20 * 500                 # the default parameters' frame
CLIP_STRIDE = FPC * SPF + 12   # larger than the clip; rows stay on 8-byte boundaries
PATTERN = 0x5A5A
TAIL = 64                      # samples of the buffer behind the last row
ONE = 20                       # the frame of exactly one sample
ENDS_IN_FRAME = -1             # the walk's quiet stop (decodefile.rs:107-116): no oracle error code, the decoders say -1

# (kernel, codes, thresholds, options)
KERNELS = [(3, (0, 1, 3), (3, 8, 20), {"decode_blocks": 1, "decode_single": 0}),
           (2, (0, 1, 3), (3, 8, 20), {"decode_blocks": 0, "decode_single": 0}),
           (1, (0, 1, 3), (3, 8, 20), {"decode_blocks": 0, "decode_single": 1}),
           (0, (2, 1, 3), (3, 8, 20), {"decode_blocks": 0, "decode_single": 0})]   # (test_gpu_code_sets.py: codes[0] = 2 -> kernel 0)

VARIANTS = ["intact", "samples_0", "payload_len_1", "header_crc", "offset_near_end", "cap_exact", "cap_one_short"]
V_FRAME = {"samples_0": 5, "payload_len_1": 9, "header_crc": 66, "offset_near_end": F - 1, "cap_exact": 40, "cap_one_short": 40}


def sample_counts(last_one):
    rng = np.random.default_rng(11)
    n = [int(x) for x in rng.integers(33, 48, size=F)]
    n[ONE] = 1
    n[F - 1] = 1 if last_one else 17
    return n


def content(n):
    """per frame a walk of another amplitude: Rice, BFP and literal blocks across the stream.  The same samples go into
    every kernel's stream, so a frame is kept only if the reference decodes what it encoded under every code set here: with
    codes[0] = 2 it does not where a block is quiet enough for the first code (decoder.rs:147-170 reads that code as unary
    whatever the parameters say), and a frame that fails inside its payload is no case of the frame setup."""
    rng = np.random.default_rng(12)
    ops = [O.Params.make(20, 500, codes, thr) for _, codes, thr, _ in KERNELS]
    out = []
    for k in n:
        for _ in range(200):
            amp = (3, 8, 20, 300, 9000)[int(rng.integers(0, 5))]
            w = np.clip(np.cumsum(rng.integers(-amp, amp + 1, size=k)), -32768, 32767).astype(np.int16)
            if all(np.array_equal(O.decode_frame(O.encode(w, op)[1][20:], k, op)[1], w) for op in ops):
                break
        else:
            raise AssertionError("no content for a frame of %d samples" % k)
        out.append(w)
    return out


def build_stream(codes, thr, last_one):
    """-> (stream, frame offsets, samples per frame, the frames' samples); the oracle encodes every frame on its own.
    last_one: the last frame is one sample and its two payload bytes end the stream on a 16-byte boundary."""
    op = O.Params.make(20, 500, codes, thr)
    n = sample_counts(last_one)
    wavs = content(n)
    frames = []
    for w in wavs:
        rc, s, _ = O.encode(w, op)
        assert rc == 0 and s.size == 20 + (int(s[6]) << 8 | int(s[7]))   # one frame
        frames.append(s)
    # one frame loses the last byte of its payload where that byte holds nothing but zero bits of its last codeword: the
    # same samples, read behind the payload's end -- not plain (oracle_lib.frame_plain), the reference's reader decodes it
    cut = None
    for f, s in enumerate(frames):
        pay = s[20:-1]
        if f in V_FRAME.values() or n[f] < 2 or pay.size < 3:
            continue
        rc, w = O.decode_frame(pay, n[f], op)
        if rc == 0 and np.array_equal(w, wavs[f]) and O.frame_plain(pay, n[f], op)[0] == 0:
            cut = f
            hdr = s[:20].copy()
            hdr[6], hdr[7] = pay.size >> 8, pay.size & 0xFF
            frames[f] = np.concatenate([hdr, pay])
            refresh_crcs(frames[f], 0)
            break
    assert cut is not None, "no frame of this content ends in a byte of zero bits"
    offs, chunks, pos = [], [], 0
    for f, s in enumerate(frames):
        pad = pos & 1                                    # frames begin at even offsets
        if last_one and f == F - 1:
            pad = (-(pos + s.size)) % 16                 # ... and the last one ends the stream on a 16-byte boundary
        chunks.append(np.zeros(pad, dtype=np.uint8))
        pos += pad
        offs.append(pos)
        chunks.append(s)
        pos += s.size
    stream = np.concatenate(chunks)
    assert not last_one or (stream.size % 16 == 0 and stream.size - offs[-1] == 22)
    return stream, offs, n, wavs


def sample_offsets(mode):
    if mode == "layout":
        return [(f // FPC) * CLIP_STRIDE + (f % FPC) * SPF for f in range(F)]
    return [48 * f + 16 * (f // 7) for f in range(F)]   # multiples of four, gaps between some rows


def variant(name, stream, offs, n, wo):
    """-> (stream, frame offsets, wav_cap) of the variant; CRCs are made good again (x3_cases.refresh_crcs), so that the
    check pass finds nothing and the decoder's own verdict stands"""
    s, offs = stream.copy(), list(offs)
    cap = max(wo[f] + n[f] for f in range(F)) + TAIL // 2
    k = V_FRAME.get(name)
    if name == "samples_0":
        s[offs[k] + 4], s[offs[k] + 5] = 0, 0
        refresh_crcs(s, offs[k])
    elif name == "payload_len_1":
        s[offs[k] + 6], s[offs[k] + 7] = 0, 1
        refresh_crcs(s, offs[k])
    elif name == "header_crc":
        s[offs[k] + 16] ^= 0x40
    elif name == "offset_near_end":
        offs[k] = s.size - 10
    elif name == "cap_exact":
        cap = wo[k] + n[k]
    elif name == "cap_one_short":
        cap = wo[k] + n[k] - 1
    return s, offs, cap


def oracle_verdicts(s, offs, wo, cap, op):
    """per frame what the reference makes of it: read_frame_header, the walk's length checks (decodefile.rs:107-121), the
    payload CRC, decode_frame into the room the output has left -> ([status], [samples or None], frames that are not plain)"""
    st, rows, not_plain = [], [], 0
    for f in range(F):
        off = offs[f]
        if off + 20 > s.size:
            st.append(ENDS_IN_FRAME); rows.append(None); continue
        h = O.FrameHeader()
        hb = np.ascontiguousarray(s[off:off + 20])
        rc = O.lib().x3o_read_frame_header(hb.ctypes.data, 20, C.byref(h))
        if rc == 0 and off + 20 + h.payload_len > s.size:
            rc = ENDS_IN_FRAME
        if rc == 0 and h.payload_len > 24576:
            rc = 12
        if rc == 0 and O.crc16(s[off + 20:off + 20 + h.payload_len]) != h.payload_crc:
            rc = 14
        w = None
        if rc == 0:
            pay = s[off + 20:off + 20 + h.payload_len]
            rc, w = O.decode_frame(pay, h.samples, op, wav_cap=max(0, cap - wo[f]))
            if rc == 0:
                not_plain += O.frame_plain(pay, h.samples, op)[0] == 0
        st.append(rc); rows.append(w if rc == 0 else None)
    return st, rows, not_plain


def run_all(x3, ctx, last_one):
    """every variant x {layout, offsets} x every kernel; -> launches checked"""
    checked = 0
    built = {}
    for mode in ("layout", "offsets"):
        wo = sample_offsets(mode)
        for name in VARIANTS:
            statuses = {}
            for kernel, codes, thr, opts in KERNELS:
                if codes not in built:
                    built[codes] = build_stream(codes, thr, last_one)
                stream, offs, n, wavs = built[codes]
                p, op = x3.Params.make(20, 500, codes, thr), O.Params.make(20, 500, codes, thr)
                s, o, cap = variant(name, stream, offs, n, wo)
                exp_st, exp_rows, exp_replays = oracle_verdicts(s, o, wo, cap, op)
                total = max(wo[f] + n[f] for f in range(F)) + TAIL
                exp = np.full(total, PATTERN, dtype=np.int16)
                for f in range(F):
                    if exp_rows[f] is not None:
                        assert np.array_equal(exp_rows[f], wavs[f])
                        exp[wo[f]:wo[f] + n[f]] = exp_rows[f]
                d_x3, d_off, d_wav, d_st = ctx.alloc(s.size), ctx.alloc(8 * (F + 1)), ctx.alloc(2 * total), ctx.alloc(4 * F)
                d_wo = ctx.alloc(8 * F)
                ctx.upload(d_x3, s)
                ctx.upload(d_off, np.array(o + [s.size], dtype=np.uint64))
                ctx.upload(d_wo, np.array(wo, dtype=np.uint64))
                ctx.upload(d_wav, np.full(total, PATTERN, dtype=np.int16))
                old = {k: ctx.get_option(k) for k in list(opts) + ["wav_offsets_x4"]}
                try:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    ctx.set_option("wav_offsets_x4", 1)
                    if mode == "layout":
                        rc = ctx.decode_dev(d_x3, s.size, d_off, F, p, d_wav, cap, n_per_clip=FPC * SPF, n_clips=2,
                                            clip_stride=CLIP_STRIDE, d_status=d_st)
                    else:
                        rc = ctx.decode_dev(d_x3, s.size, d_off, F, p, d_wav, cap, d_wav_offsets=d_wo, d_status=d_st)
                    assert rc == 0, ctx.last_error()
                    assert ctx.get_option("decode_kernel_in_use") == kernel, (mode, name, kernel)
                    rc, first_bad, _, _ = ctx.decode_result()
                    assert rc == 0
                finally:
                    for k, v in old.items():
                        ctx.set_option(k, v)
                what = (mode, name, kernel)
                got_st = ctx.download(d_st, 4 * F, np.int32).tolist()
                got = ctx.download(d_wav, 2 * total, np.int16)
                for d in (d_x3, d_off, d_wav, d_st, d_wo):
                    ctx.free(d)
                assert got_st == exp_st, (what, [(f, a, b) for f, (a, b) in enumerate(zip(got_st, exp_st)) if a != b])
                assert first_bad == next((f for f in range(F) if exp_st[f]), F), what
                assert ctx.get_option("last_decode_replays") == exp_replays, what
                bad = np.flatnonzero(got != exp)
                assert bad.size == 0, (what, "first difference at sample %d, wav_cap %d" % (bad[0], cap))
                statuses[kernel] = got_st
                checked += 1
            assert all(v == statuses[3] for v in statuses.values()), (mode, name)
            assert name == "intact" or any(statuses[3]), (mode, name)   # (the variant is one: some frame fails)
    return checked


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def test_frame_setup_is_the_same_on_the_four_decoders(x3, ctx):
    assert run_all(x3, ctx, last_one=False) == 2 * len(VARIANTS) * len(KERNELS)


def test_frame_setup_under_guard_pages():
    """the round-5 finding: the last frame is one sample whose payload ends on a 16-byte boundary at the end of the stream,
    and the stream's buffer ends at its mapping (X3HIP_FENCE: a fresh child process, as test_gpu_fence.py's)"""
    env = dict(os.environ, X3HIP_FENCE="16", X3HIP_FENCE_FILL="165")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x3-rust_amd"), HERE, env.get("PYTHONPATH", "")])
    code = """
        import x3hip
        import test_gpu_frame_setup as T
        ctx = x3hip.Context(0)
        print("checked", T.run_all(x3hip, ctx, last_one=True))
        ctx.close()
        """
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-15:])
    assert r.returncode == 0, "child under the fence ended with %d:\n%s" % (r.returncode, tail)
    assert int(r.stdout.split("checked")[1]) == 2 * len(VARIANTS) * len(KERNELS)
