"""Case generators shared by the GPU tests (not a test module): content that puts every block type side by side, frame
offsets of a stream, CRCs made good again after tampering, and crafted frames -- short, cut, overlong and garbage payloads
-- with the batch decode that checks each of them against the oracle's decode_frame."""
import numpy as np

import oracle_lib as O

STRIDE = 65544  # samples between the crafted frames' output ranges (a header can ask for up to 65535 samples)

AMPS = (0, 1, 2, 3, 4, 7, 8, 9, 19, 20, 21, 31, 32, 100, 1000, 8191, 8192, 16383, 16384, 30000, 65535)


def oparams(p):
    """the oracle's Params for an x3hip.Params"""
    return O.Params.make(p.block_len, p.blocks_per_frame, tuple(p.codes), tuple(p.thresholds))


def patchwork(seed, n, amps=AMPS):
    """runs of 3..70 samples whose differences stay inside one of the encoder's classes: silence, each Rice code's range and
    its edges, BFP widths, literals, saturating jumps -- so that blocks of every type and lanes of every mix sit side by side"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=np.int64)
    pos, level = 0, 0
    while pos < n:
        ln = int(rng.integers(3, 71))
        a = amps[int(rng.integers(0, len(amps)))]
        d = rng.integers(-a, a + 1, size=ln)
        if a and rng.integers(0, 4) == 0:
            d[int(rng.integers(0, ln))] = a if rng.integers(0, 2) else -a   # the class's edge itself
        seg = level + np.cumsum(d)
        seg = np.clip(seg, -32768, 32767)
        m = min(ln, n - pos)
        out[pos:pos + m] = seg[:m]
        level = int(seg[m - 1])
        pos += m
    return out.astype(np.int16)


def frame_offsets(stream):
    """byte offsets of the frames of an intact stream (by the headers' payload lengths)"""
    offs, pos = [], 0
    while pos + 20 <= len(stream):
        offs.append(pos)
        pos += 20 + (int(stream[pos + 6]) << 8 | int(stream[pos + 7]))
    return offs


def refresh_crcs(s, off):
    """payload and header CRC of the frame at `off`, after its payload or header was tampered with"""
    plen = int(s[off + 6]) << 8 | int(s[off + 7])
    pc = O.crc16(s[off + 20:off + 20 + plen])
    s[off + 18], s[off + 19] = pc >> 8, pc & 0xFF
    hc = O.crc16(s[off:off + 16])
    s[off + 16], s[off + 17] = hc >> 8, hc & 0xFF


def signals(x3, rng):
    """short clips whose blocks are mostly Rice0, Rice1, Rice3, BFP and literal"""
    out = []
    for amp in (1, 3, 8, 20, 300, 9000, 32000):
        n = int(rng.integers(30, 260))
        d = rng.integers(-amp, amp + 1, size=n)
        w = np.clip(np.cumsum(d), -32768, 32767).astype(np.int16) if amp < 9000 else \
            rng.integers(-amp, amp + 1, size=n).astype(np.int16)
        out.append(w)
    out.append(np.zeros(61, dtype=np.int16))
    out.append(x3.synth(2, 4242, 0, 241))
    return out


def crafted_frames(x3, rng, params, count):
    """-> list of (payload bytes, samples)"""
    base = []
    for w in signals(x3, rng):
        p1 = O.Params.make(params.block_len, 4000, tuple(params.codes), tuple(params.thresholds))  # one frame
        rc, s, _ = O.encode(w, p1)
        assert rc == 0
        base.append((s[20:].copy(), w.size))
    frames = []
    while len(frames) < count:
        pay, n = base[int(rng.integers(0, len(base)))]
        kind = int(rng.integers(0, 7))
        pay = pay.copy()
        if kind == 0:      # payload cut anywhere (odd lengths too), header samples unchanged
            pay = pay[: int(rng.integers(2, pay.size + 1))]
        elif kind == 1:    # more samples than the payload encodes
            n = n + int(rng.choice([1, 2, 3, 7, 19, 20, 21, 40, 41, 64, 333]))
        elif kind == 2:    # both
            pay = pay[: int(rng.integers(2, pay.size + 1))]
            n = n + int(rng.integers(0, 100))
        elif kind == 3:    # a long zero run somewhere (4..12 zero bytes), sometimes at the very end
            k = int(rng.integers(4, 13))
            at = int(rng.integers(2, max(3, pay.size - k + 1)))
            pay[at:at + k] = 0
            if rng.random() < 0.3:
                n += int(rng.integers(0, 50))
        elif kind == 4:    # garbage
            pay = rng.integers(0, 256, size=int(rng.integers(2, 120)), dtype=np.uint8)
            n = int(rng.integers(1, 400))
        elif kind == 5:    # sparse garbage: long zero runs with a few ones (phantom counts, one-word peeks)
            pay = np.zeros(int(rng.integers(3, 90)), dtype=np.uint8)
            for _ in range(int(rng.integers(0, 6))):
                pay[int(rng.integers(0, pay.size))] = 1 << int(rng.integers(0, 8))
            pay[2] |= int(rng.choice([0x40, 0x80, 0xC0]))   # a Rice block header up front
            n = int(rng.integers(1, 300))
        else:              # the untouched frame
            pass
        frames.append((pay, n))
    return frames


def run_batch(x3, ctx, params, frames, mode):
    """decode all frames in one launch; -> (status[F], list of sample arrays)"""
    F = len(frames)
    offs, chunks, pos = [], [], 0
    for pay, n in frames:
        hdr = x3.write_frame_header(n, 1, pay.size, O.crc16(pay))
        offs.append(pos)
        chunks += [hdr, pay]
        pos += 20 + pay.size
        if pos & 1:
            chunks.append(np.zeros(1, dtype=np.uint8))
            pos += 1
    stream = np.concatenate(chunks + [np.zeros(64, dtype=np.uint8)])
    d_x3 = ctx.alloc(stream.size)
    ctx.upload(d_x3, stream)
    d_off = ctx.alloc(8 * (F + 1))
    ctx.upload(d_off, np.array(offs + [pos], dtype=np.uint64))
    d_wav = ctx.alloc(2 * STRIDE * F)
    ctx.upload(d_wav, np.full(STRIDE * F, 0x5A5A, dtype=np.int16))
    d_st = ctx.alloc(4 * F)
    spf = params.block_len * params.blocks_per_frame
    if mode in ("offsets", "offsets_x4"):
        # caller-supplied sample offsets: the single-wave kernels -- or, with the caller's promise that they are multiples
        # of four samples (option wav_offsets_x4), the three-wave decoder and its list of rows (every row its own length)
        d_wo = ctx.alloc(8 * F)
        ctx.upload(d_wo, (np.arange(F, dtype=np.uint64) * STRIDE))
        ctx.set_option("wav_offsets_x4", 1 if mode == "offsets_x4" else 0)
        try:
            rc = ctx.decode_dev(d_x3, pos, d_off, F, params, d_wav, STRIDE * F, d_wav_offsets=d_wo, d_status=d_st)
        finally:
            ctx.set_option("wav_offsets_x4", 0)
    else:                     # a batch of F one-frame clips: the two-wave kernel for block_len 20
        d_wo = None
        rc = ctx.decode_dev(d_x3, pos, d_off, F, params, d_wav, STRIDE * F, n_per_clip=spf, n_clips=F,
                            clip_stride=STRIDE, d_status=d_st)
    assert rc == 0, ctx.last_error()
    rc, first_bad, st0, before = ctx.decode_result()
    assert rc == 0
    run_batch.replays = ctx.get_option("last_decode_replays")
    status = ctx.download(d_st, 4 * F, np.int32)
    wav = ctx.download(d_wav, 2 * STRIDE * F, np.int16).reshape(F, STRIDE)
    for d in (d_x3, d_off, d_wav, d_st) + ((d_wo,) if d_wo else ()):
        ctx.free(d)
    return status, wav, first_bad


def not_plain(frames, op):
    """how many of the (payload, samples) frames are not plain (oracle_lib.frame_plain): the frames a decode launch hands to
    the reference's reader (x3_decode_replay.h), option last_decode_replays.  Frames decode_frame refuses do not count."""
    return sum(O.frame_plain(pay, n, op)[0] == 0 for pay, n in frames)


def walked_frames(stream, cap):
    """the frames x3_decode_stream / x3_decode_stream_dev hand to the decoder in one launch: the reference's walk of the
    headers (decodefile.rs:105-121) -- up to a bad header, a cut or overlong payload, or a frame that is a panic there --
    less those whose payload CRC fails (the check pass decides them).  -> [(payload, samples)]"""
    out, pos, nsamp = [], 0, 0
    while len(stream) - pos > 20:
        h = stream[pos:pos + 20]
        if O.crc16(h[:16]) != (int(h[16]) << 8 | int(h[17])) or (int(h[0]) << 8 | int(h[1])) != 30771 or h[3] > 1:
            break
        n, plen = int(h[4]) << 8 | int(h[5]), int(h[6]) << 8 | int(h[7])
        if plen >= 0x7FE0 or plen > 24576 or len(stream) - pos - 20 < plen:   # (X3_READ_BUFFER_SIZE)
            break
        pay = stream[pos + 20:pos + 20 + plen]
        if n == 0 or plen < 2 or nsamp + n > cap:
            break
        if O.crc16(pay) == (int(h[18]) << 8 | int(h[19])):
            out.append((pay, n))
        nsamp += n
        pos += 20 + plen
    return out


def compare(x3, ctx, params, frames, mode):
    """crafted frames through run_batch against the oracle's decode_frame: status and samples of every frame, the 0x5A guard
    behind every good row, the first failing frame, and the frames the decoder handed to the reference's reader: exactly
    those that are not plain; -> {oracle status: frames}"""
    status, wav, first_bad = run_batch(x3, ctx, params, frames, mode)
    op = oparams(params)
    assert run_batch.replays == not_plain(frames, op), (mode, run_batch.replays, not_plain(frames, op))
    seen = {}
    exp_first_bad = len(frames)
    for i, (pay, n) in enumerate(frames):
        rc_o, w_o = O.decode_frame(pay, n, op)
        assert status[i] == rc_o, (mode, i, int(status[i]), rc_o, pay.size, n)
        if rc_o == 0:
            assert np.array_equal(wav[i, :n], w_o), (mode, i, pay.size, n)
            assert (wav[i, n:n + 8] == 0x5A5A).all()
        elif exp_first_bad == len(frames):
            exp_first_bad = i
        seen[rc_o] = seen.get(rc_o, 0) + 1
    assert first_bad == exp_first_bad
    return seen


_fuzz_tool = None


def damage(rng, stream, offs):
    """tools/fuzz_parity.py's damage(): a copy of `stream` with one to three of its frames tampered with (bits, zero runs,
    random bytes, sample counts, headers, cleared tails; CRCs refreshed or not), perhaps truncated.  The tool is loaded on
    first use, under a name of its own."""
    global _fuzz_tool
    if _fuzz_tool is None:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
        spec = importlib.util.spec_from_file_location("x3_cases_fuzz_parity", path)
        _fuzz_tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_fuzz_tool)
    return _fuzz_tool.damage(rng, stream, offs)
