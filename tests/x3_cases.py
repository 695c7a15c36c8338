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


def fuzz_tool():
    """tools/fuzz_parity.py, loaded on first use under a name of its own"""
    global _fuzz_tool
    if _fuzz_tool is None:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
        spec = importlib.util.spec_from_file_location("x3_cases_fuzz_parity", path)
        _fuzz_tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_fuzz_tool)
    return _fuzz_tool


def damage(rng, stream, offs):
    """tools/fuzz_parity.py's damage(): a copy of `stream` with one to three of its frames tampered with (bits, zero runs,
    random bytes, sample counts, headers, cleared tails; CRCs refreshed or not), perhaps truncated."""
    return fuzz_tool().damage(rng, stream, offs)


def draw_codes(rng):
    """tools/fuzz_parity.py's draw_codes(): (codes, thresholds) as its decode families draw them"""
    return fuzz_tool().draw_codes(rng)


# ------------------------------------------------------------------ multi-channel cases (x3_mc.h, x3_decode_mc_kernel.h)

MC_CHANNELS = (2, 3, 8)
# (codes, thresholds, block_len): x3_decode_mc_lanes_kernel takes the first six; block lengths above 60 send every frame
# down the thread-per-frame path
MC_PSETS = [((0, 1, 3), (3, 8, 20), 20), ((1, 1, 3), (3, 8, 20), 10), ((0, 1, 2), (3, 8, 18), 40),
            ((3, 3, 3), (2, 9, 27), 13), ((2, 1, 3), (3, 8, 20), 20), ((0, 1, 3), (3, 8, 20), 60),
            ((0, 1, 3), (3, 8, 20), 61), ((0, 1, 3), (3, 8, 20), 100)]
MC_PIDS = ["c%d%d%d-t%d_%d_%d-bl%d" % (c + t + (bl,)) for c, t, bl in MC_PSETS]
MC_POOL = 150   # crafted frames per (channel count, parameter set), the degenerate frames not counted
# code sets the extra base payloads are written under: valid frames of bit patterns the decoding code set never writes
MC_FOREIGN = [((0, 1, 3), (3, 8, 20)), ((1, 1, 3), (3, 8, 20)), ((3, 3, 3), (2, 9, 27)), ((0, 0, 0), (2, 4, 6))]


class _Seeded:
    """signals()' use of x3hip (synth kind 2, white noise) as a seeded draw: the pools need no GPU"""
    @staticmethod
    def synth(kind, seed, start, n):
        return np.random.default_rng(seed + start).integers(-32768, 32768, size=n).astype(np.int16)


def mc_params(pset, bpf=4000):
    """the oracle's Params of an MC_PSETS entry; 4 000 blocks: whatever the clip, one frame"""
    codes, thr, bl = pset
    return O.Params.make(bl, bpf, codes, thr)


def mc_frame(payload, samples, n_ch):
    """header (byte 3 = n_ch, both CRCs valid) + payload: one frame as it stands in a stream.  x3_decode_stream_mc finds
    the next header right behind the payload (the walk of decodefile.rs:105-121 has no alignment rule), so frames follow
    each other without padding: behind an encoder's payload -- always even -- they sit at even positions, as run_batch's
    do; behind a crafted payload of odd length every later frame sits at an odd one, which a decoder has to take too."""
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    hdr = np.zeros(20, dtype=np.uint8)
    O.lib().x3o_write_frame_header(samples, 1, payload.size, O.crc16(payload), hdr.ctypes.data)
    hdr[3] = n_ch
    hc = O.crc16(hdr[:16])
    hdr[16], hdr[17] = hc >> 8, hc & 0xFF
    return np.concatenate([hdr, payload])


def mc_encode_frame(wavs, bl, codes, thr):
    """one multi-channel frame of wavs (equally long channels) -> (status, frame bytes): the oracle's encoder up to the
    reference's block length limit of 60 (encoder.rs:296-299), beyond it the layout restated here -- first samples, the
    blocks in (block index, channel) order each coded as a mono block (encoder.rs:289-315), word_align --, which
    tests/test_mc_cases.py holds against the oracle's bytes at the block lengths both take"""
    if bl <= 60:
        rc, s, _ = O.encode_mc(wavs, O.Params.make(bl, 4000, codes, thr))
        return rc, s
    return 0, mc_encode_frame_py(wavs, bl, codes, thr)


def mc_encode_frame_py(wavs, bl, codes, thr):
    n = len(wavs[0])
    bits = [format(int(w[0]) & 0xFFFF, "016b") for w in wavs]
    for s in range(1, n, bl):
        for w in wavs:
            d = np.diff(w[s - 1:s + bl].astype(np.int64))
            m = int(np.abs(d).max())
            if m <= thr[2]:
                ft = int(m > thr[0]) + int(m > thr[1])
                k = codes[ft]
                bits.append(format(ft + 1, "02b"))
                for x in d.tolist():
                    u = 2 * x if x >= 0 else -2 * x - 1
                    bits.append("0" * (u >> k) + "1" + (format(u & ((1 << k) - 1), "0%db" % k) if k else ""))
            elif m.bit_length() >= 15:
                bits.append("001111")
                bits += [format(int(x) & 0xFFFF, "016b") for x in w[s:s + bl]]
            else:
                e = m.bit_length() + 1
                bits.append(format(e - 1, "06b"))
                bits += [format(x & ((1 << e) - 1), "0%db" % e) for x in d.tolist()]
    s = "".join(bits)
    s += "0" * (-len(s) % 16)
    payload = np.array([int(s[i:i + 8], 2) for i in range(0, len(s), 8)], dtype=np.uint8)
    return mc_frame(payload, n, len(wavs))


def _mc_bases(rng, bl, codes, thr, n_ch, take=None):
    """(payload, samples) of signals()' clips, one long frame each: channel c of clip i is clip i + c, cut or repeated to
    clip i's length -- blocks of every type side by side in one block row"""
    sigs = signals(_Seeded, rng)
    out = []
    for i, w in enumerate(sigs[:take]):
        wavs = [np.resize(sigs[(i + c) % len(sigs)], w.size) for c in range(n_ch)]
        rc, s = mc_encode_frame(wavs, bl, codes, thr)
        if rc == 0:   # (a difference outside a code's table is a panic in the reference: no frame)
            out.append((s[20:].copy(), w.size))
    return out


def crafted_frames_mc(rng, params, n_ch, count):
    """crafted_frames for n_ch channels -> list of (payload bytes, samples): `count` frames of the seven kinds of
    tampering, on payloads written under the decoding code set and under others, then the degenerate frames (no samples;
    payloads of 0, 2, 2 n_ch - 2 and 2 n_ch bytes)"""
    bl, codes, thr = params.block_len, tuple(params.codes), tuple(params.thresholds)
    base = _mc_bases(rng, bl, codes, thr, n_ch)
    assert len(base) >= 6, (codes, thr, len(base))
    for fc, ft in MC_FOREIGN:
        if fc != codes:
            base += _mc_bases(rng, bl, fc, ft, n_ch, take=4)
    first = 2 * n_ch   # the bit stream begins behind the channels' first samples
    frames = []
    while len(frames) < count:
        pay, n = base[int(rng.integers(0, len(base)))]
        kind = (0, 0, 1, 1, 2, 3, 4, 5, 6)[int(rng.integers(0, 9))]   # (cuts and long counts twice as often: the frames that
        pay = pay.copy()                                              # decode without being plain come from them)
        if kind == 0:      # payload cut anywhere at or behind the first samples (odd lengths too)
            pay = pay[: int(rng.integers(first, pay.size + 1))]
        elif kind == 1:    # more samples than the payload encodes
            n = n + int(rng.choice([1, 2, 3, 7, 19, 20, 21, 40, 41, 64, 333]))
        elif kind == 2:    # both
            pay = pay[: int(rng.integers(first, pay.size + 1))]
            n = n + int(rng.integers(0, 100))
        elif kind == 3:    # a long zero run somewhere (4..12 zero bytes), sometimes at the very end
            k = int(rng.integers(4, 13))
            at = int(rng.integers(first, max(first + 1, pay.size - k + 1)))
            pay[at:at + k] = 0
            if rng.random() < 0.3:
                n += int(rng.integers(0, 50))
        elif kind == 4:    # garbage
            pay = rng.integers(0, 256, size=int(rng.integers(first, first + 120)), dtype=np.uint8)
            n = int(rng.integers(1, 400))
        elif kind == 5:    # sparse garbage: long zero runs with a few ones, a Rice block header up front
            pay = np.zeros(int(rng.integers(first + 1, first + 90)), dtype=np.uint8)
            for _ in range(int(rng.integers(0, 6))):
                pay[int(rng.integers(0, pay.size))] = 1 << int(rng.integers(0, 8))
            pay[first] |= int(rng.choice([0x40, 0x80, 0xC0]))
            n = int(rng.integers(1, 300))
        frames.append((pay, n))
    pay, n = base[0]
    frames.append((pay.copy(), 0))
    for ln in (0, 2, first - 2, first):
        for m in (1, bl + 1):
            frames.append((pay[:ln].copy(), m))
    return frames


def mc_pool(n_ch, pi):
    """the seeded pool of (channel count, MC_PSETS[pi]): what tests/test_mc_cases.py classifies on the CPU and
    tests/test_gpu_multichannel_edges.py decodes, every frame of it"""
    rng = np.random.default_rng([2027, n_ch, pi])
    return crafted_frames_mc(rng, mc_params(MC_PSETS[pi]), n_ch, MC_POOL)


def mc_verdict(payload, samples, n_ch, op):
    """the oracle on the stream that holds this frame alone -> ((status, frames_ok, frame_errors), samples per channel,
    frame_plain's verdict: 1 plain, 0 not, -1 refused).  frames_ok == 1: the frame decodes."""
    rc, wavs, fok, ferr = O.decode_stream_mc(mc_frame(payload, samples, n_ch), n_ch, op, wav_cap=samples + 8)
    return (rc, fok, ferr), wavs, O.frame_plain(payload, samples, op, n_ch=n_ch)[0]


def mc_clean_frames(rng, op, n_ch, counts):
    """oracle-encoded frames of counts[i] samples a channel whose content round-trips under op's code set -- the
    reference's decoder hard-wires the Rice widths of (0, 1, 3) and refuses narrow BFP blocks, so under other sets only
    some block types come back: the first draw that does is taken -- and that are plain.  -> [(frame bytes, [channel])]"""
    def draw(kind, n):
        if kind < 3:
            a = (1, 3, 8)[kind]
            return np.cumsum(rng.integers(-a, a + 1, size=n)).astype(np.int16)
        a = (300, 9000, 32767)[kind - 3]
        return rng.integers(-a, a + 1, size=n).astype(np.int16)
    out = []
    for i, n in enumerate(counts):
        for attempt in range(12):
            kinds = [(i + c + attempt) % 6 if attempt < 6 else 3 + (i + c + attempt) % 3 for c in range(n_ch)]
            wavs = [draw(k, n) for k in kinds]
            rc, s = mc_encode_frame(wavs, op.block_len, tuple(op.codes), tuple(op.thresholds))
            if rc:
                continue
            rc, back, fok, ferr = O.decode_stream_mc(s, n_ch, op, wav_cap=n + 8)
            if (rc, fok, ferr) == (0, 1, 0) and all(np.array_equal(b, w) for b, w in zip(back, wavs)) and \
                    O.frame_plain(s[20:], n, op, n_ch=n_ch)[0] == 1:
                out.append((s, wavs))
                break
        else:
            raise AssertionError("no content that round-trips for %s" % (tuple(op.codes),))
    return out


# the encoder's payload edge at block_len 10: (blocks_per_frame, channels, channels of literal blocks, payload bytes,
# status).  A literal block of 10 samples is 166 bits, a silent one 12; the last block holds 9 samples.
PAYLOAD_EDGE = [(786, 8, 1, 24576, 0), (973, 4, 1, 24574, 0), (360, 7, 3, 24578, 10), (788, 8, 1, 24640, 10),
                (573, 3, 2, 24642, 10)]


def edge_channels(bpf, n_ch, n_lit, seed=5, frames=1):
    """n_lit channels of full-scale noise of alternating sign (every block a literal), the others silent"""
    rng = np.random.default_rng(seed)
    n = 10 * bpf * frames
    sign = np.where(np.arange(n) & 1, -1, 1)
    return [(sign * rng.integers(20000, 32768, size=n)).astype(np.int16) if c < n_lit else np.zeros(n, dtype=np.int16)
            for c in range(n_ch)]
