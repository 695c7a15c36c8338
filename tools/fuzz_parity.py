#!/usr/bin/env python3
"""Parity soak: the HIP path (through the C ABI) against the CPU oracle on randomly drawn inputs, for a time budget.
Not part of the test suite (it runs as long as it is told to); a failure prints the seed and the drawn case, and
`--seed S --only T` replays trial T of seed S.
   python tools/fuzz_parity.py --minutes 10 [--seed 1]
Families: (e) the single-pass encoders on block_len 20 with mixed content, many frames and ragged tails;
          (g) arbitrary geometry / codes / thresholds, every stream decoded back; (d) decode of tampered streams with
          refreshed CRCs, truncations and header damage, other code sets now and then (so in (k)); (b) batches of clips
          through the device API, of equal and of different lengths (x3_encode_frames_dev); (a) .x3a archives in memory and
          the incremental reader; (f) decode_frame frame by frame, with and without x3_decode_prefetch; (w) WAV and .x3a FILES through the
          chunked pipeline (not in the default family set: file I/O); (s) the segment index: the encoder's against the one a
          decode records, decode by it with the stream and the index intact or damaged; (c) random access: batches of
          windows (x3_decode_windows_dev) of random streams, geometries and lengths, with damaged frames, damaged indexes
          and wild starts, against the oracle's frame verdicts (not in the default family set); (x) the same with the
          index built by x3_seg_index_build_dev on the stream as it is -- any block length and code set, damage included
          (not in the default family set); (r) range levels (x3_range_levels_dev): random ranges x bin lengths x layouts x
          damage, with and without an index, GPU == tests/range_levels_ref.py (not in the default family set); (h) levels of the
          first difference (x3_signal_levels_dev / x3_corpus_signal_levels_dev, X3_LEVEL_SIGNAL_DIFF): random content x
          geometry x bin lengths x damage, with, without and with a damaged index, a stream and the same stream cut into
          corpus entries, GPU == tests/diff_levels_ref.py on the oracle's frame verdicts (not in the default family set);
          (l) family (r) on the first difference (x3_signal_range_levels_dev, X3_LEVEL_SIGNAL_DIFF), with starts drawn to
          frame and stretch boundaries as well (lead frames, seeds from the index), GPU == tests/signal_range_levels_ref.py
          (not in the default family set); (i) family (h) behind an integer FIR filter (x3_fir_levels_dev /
          x3_corpus_fir_levels_dev): random taps (1 .. 8, sum |c| <= 32768) and shifts as well, frames and stretches shorter
          than the taps among them, GPU == tests/fir_levels_ref.py; {1} against x3_levels_dev byte for byte (not in the
          default family set); (t) family (r) behind a random valid Fir (x3_fir_range_levels_dev; the letter (l) is the
          difference's), with starts drawn to frame and stretch boundaries +- T - 1 (lead frames, stretch fronts), GPU ==
          tests/fir_range_levels_ref.py (not in the default family set); (o) family (h) against one oscillator
          (x3_tone_levels_dev / x3_corpus_tone_levels_dev): a random step -- 0, 2^30, 2^31 and 2^32 - 1 among them -- and the
          usual table or a random one, GPU == tests/tone_levels_ref.py; the adapter (x3_tone_power_levels_dev, by
          levels(signal=Tone)) against the reference on the same records; a table of all (1, 0) against x3_levels_dev's sums
          (not in the default family set); (p) family (r) against a random Tone (x3_tone_range_levels_dev): a random step
          and the usual table or a random one, with starts drawn to frame and stretch boundaries +- 1 (the phase seeds of
          lanes and fix-up), as a stream and as a corpus of random entries (x3_corpus_tone_range_levels_dev: the phase is 0
          at every entry), GPU == tests/tone_range_levels_ref.py (not in the default family set); (q) family (h) against a
          random tone bank (x3_tone_bank_levels_dev / x3_corpus_tone_bank_levels_dev): 1 .. 8 drawn steps, equal ones among
          them, the usual table or a random one, garbage in the struct's spare steps; every plane GPU ==
          tests/tone_bank_levels_ref.py and == the single call's bytes, the adapter over all planes at once, then the same
          frames as a corpus (not in the default family set); (u) family (p) with a random tone bank on top
          (x3_tone_bank_range_levels_dev / x3_corpus_tone_bank_range_levels_dev): 1 .. 8 steps -- 0, 2^30, 2^31, 2^32 - 1 and
          equal ones among them, the family's own step in one slot -- against the same table, garbage in the spare steps;
          every plane GPU == tests/tone_range_levels_ref.py at its step and == the single call's bytes, what no call writes
          keeps its fill in every plane, then the same ranges on the corpus, plane by plane the single corpus call's bytes
          (not in the default family set); (v) plane events (x3_plane_events_dev / x3_corpus_plane_events_dev) on the band
          planes of a drawn tone bank over a random, possibly damaged stream: random K, min_planes, per-plane values (keys of
          the planes' own records, planes switched off), plane stride with loud records in the slack, rule, cap, NULL
          outputs, d_thr per (plane, entry) or none -- values off and above their limits among them -- GPU ==
          tests/plane_events_ref.py in every slot; bank_events (no host trip) on the same rule; then the same frames as a
          corpus of random entries (not in the default family set); (y) spectra (x3_spectra_rows_dev): int16 rows in HBM at
          drawn offsets x n_fft x hop x format x layout x capacities x table x in-statuses, lengths round n_fft and round
          whole frames, GPU == tests/spectra_ref.py in every word (not in the default family set; (w) is the files'); (z) band
          levels (x3_spectra_levels_dev): (y)'s rows, lengths round whole time bins as well, x frames_per_bin x n_bands x band
          maps with wild words and empty bands x plane strides, GPU == tests/spectra_levels_ref.py in every record of every
          plane (not in the default family set)."""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "x3-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import x3hip
if os.environ.get("X3HIP_LIB"):
    x3hip.LIB_PATH = os.environ["X3HIP_LIB"]
import oracle_lib as O

ctx = None   # the x3hip.Context under test (set by run())
START_TRIAL = 0   # --start: the sequence of trials begins here (a fresh context; for getting near a failing trial quickly)


def oparams(p):
    return O.Params.make(p.block_len, p.blocks_per_frame, tuple(p.codes), tuple(p.thresholds))


def content(rng, n):
    """a signal stitched from segments of different character, so that frames mix block types"""
    out = np.zeros(n, dtype=np.int64)
    i = 0
    while i < n:
        seg = int(rng.choice([1, 7, 19, 20, 21, 40, 100, 400, 1000, 5000, 20000]))
        seg = min(seg, n - i)
        kind = int(rng.integers(0, 9))
        if kind == 0:
            v = np.zeros(seg)
        elif kind == 1:
            v = np.full(seg, int(rng.choice([-32768, 32767, 1, -1, 12345])))
        elif kind == 2:
            v = rng.integers(-32768, 32768, size=seg)
        elif kind == 3:
            amp = int(rng.choice([1, 2, 3, 4, 5, 8, 9, 10, 20, 21, 30, 64, 500, 8000, 16383, 16384]))
            v = np.cumsum(rng.integers(-amp, amp + 1, size=seg))
        elif kind == 4:
            v = np.round(float(rng.choice([50, 1000, 20000, 32767])) * np.sin(np.arange(seg) * float(rng.uniform(0.001, 1.5))))
        elif kind == 5:
            v = np.tile(np.array([32767, -32768]), seg // 2 + 1)[:seg]
        elif kind == 6:
            amp = int(rng.choice([3, 4, 8, 9, 20, 21]))  # exactly at the Rice thresholds
            v = np.cumsum(rng.choice([-amp, 0, amp], size=seg))
        elif kind == 7:
            v = rng.integers(-3, 4, size=seg) + (rng.random(seg) < 0.02) * rng.integers(-30000, 30000, size=seg)
        else:
            v = x3hip.synth(int(rng.choice([0, 1, 2, 3, 4])), int(rng.integers(0, 1 << 30)), 0, seg).astype(np.int64)
        v = np.asarray(v, dtype=np.int64)
        # fold back into the i16 range (cumulative sums wander)
        v = ((v + 32768) % 65536) - 32768 if kind in (3, 6) and rng.random() < 0.3 else np.clip(v, -32768, 32767)
        out[i:i + seg] = v
        i += seg
    return out.astype(np.int16)


def frame_offsets(stream):
    offs, pos = [], 0
    while pos + 20 <= stream.size:
        plen = int(stream[pos + 6]) << 8 | int(stream[pos + 7])
        if pos + 20 + plen > stream.size:
            break
        offs.append(pos)
        pos += 20 + plen
    return offs


def refresh_crcs(s, off):
    plen = min(int(s[off + 6]) << 8 | int(s[off + 7]), s.size - off - 20)
    hc = O.crc16(s[off:off + 16])
    s[off + 16], s[off + 17] = hc >> 8, hc & 0xFF
    pc = O.crc16(s[off + 20:off + 20 + plen])
    s[off + 18], s[off + 19] = pc >> 8, pc & 0xFF


def cmp_encode(wav, p, sp, tag, cap_cut=None):
    spf = p.block_len * p.blocks_per_frame
    cap = sp + 64 + ((wav.size + spf - 1) // spf) * 84 + 3 * wav.size   # the same, generous, capacity for both
    if cap_cut is not None:
        cap = int(cap_cut * cap)                                       # ... or one both run out of
    rc_o, out_o, st_o = O.encode(wav, oparams(p), start_pos=sp, cap=cap)
    # (one input in three: the host front end takes it in chunks of eight frames, if it has sixteen)
    ctx.set_option("host_chunk_frames", 8 if wav.size % 3 == 0 else -1)
    try:
        rc_g, out_g, st_g = ctx.encode(wav, p, start_pos=sp, cap=cap)
    finally:
        ctx.set_option("host_chunk_frames", 0)
    assert rc_g == rc_o, (tag, "status", rc_g, rc_o, ctx.last_error())
    if rc_o == 0:
        assert out_g.size == out_o.size, (tag, "size", out_g.size, out_o.size)
        if not np.array_equal(out_g[sp:], out_o[sp:]):
            bad = np.nonzero(out_g[sp:] != out_o[sp:])[0]
            raise AssertionError((tag, "bytes differ", int(bad[0]) + sp, int(bad.size)))
        assert st_g.tolist() == st_o.tolist(), (tag, "stats")
    return rc_o, out_o


def cmp_decode(stream, p, cap, tag):
    r_o = O.decode_stream(stream, oparams(p), wav_cap=cap)
    # the walk on the host, on the GPU, and the stream taken in chunks of 1 + (its length mod 5) frames
    # (the GPU walk twice: its fast path for clean chains with the general walk behind it, and the general walk alone)
    for host_walk, chunk, no_fast in ((1, -1, 0), (0, -1, 0), (0, -1, 1), (-1, 1 + len(stream) % 5, 0)):
        ctx.set_option("host_walk", host_walk)
        ctx.set_option("host_chunk_frames", chunk)
        ctx.set_option("index_no_fast", no_fast)
        try:
            r_g = ctx.decode_stream(stream, p, wav_cap=cap)
        finally:
            ctx.set_option("host_walk", -1)
            ctx.set_option("host_chunk_frames", 0)
            ctx.set_option("index_no_fast", 0)
        ok = (r_g[0], r_g[2], r_g[3]) == (r_o[0], r_o[2], r_o[3]) and np.array_equal(r_g[1], r_o[1])
        if not ok and os.environ.get("X3_FUZZ_DUMP"):   # what went in and what came out, for a post-mortem on the CPU
            os.makedirs(os.environ["X3_FUZZ_DUMP"], exist_ok=True)
            np.savez(os.path.join(os.environ["X3_FUZZ_DUMP"], "fail_%s.npz" % "_".join(str(x) for x in tag[0])), stream=stream,
                     got=r_g[1], want=r_o[1], got_rc=np.array([r_g[0], r_g[2], r_g[3]]), want_rc=np.array([r_o[0], r_o[2], r_o[3]]),
                     params=np.array([p.block_len, p.blocks_per_frame]), mode=np.array([host_walk, chunk, no_fast]))
            # the same call again, twice, and on the other decoder kernels: is it the data or the moment?
            for name, opts in (("again", {}), ("again2", {}), ("three_wave", {"decode_blocks": 0}), ("single", {"decode_blocks": 0, "decode_single": 1})):
                old = {k: ctx.get_option(k) for k in opts}
                for k, v in opts.items():
                    ctx.set_option(k, v)
                ctx.set_option("host_walk", host_walk); ctx.set_option("host_chunk_frames", chunk); ctx.set_option("index_no_fast", no_fast)
                r2 = ctx.decode_stream(stream, p, wav_cap=cap)
                ctx.set_option("host_walk", -1); ctx.set_option("host_chunk_frames", 0); ctx.set_option("index_no_fast", 0)
                for k, v in old.items():
                    ctx.set_option(k, v)
                d = np.nonzero(r2[1][:min(r2[1].size, r_o[1].size)] != r_o[1][:min(r2[1].size, r_o[1].size)])[0]
                print("   %-10s rc %s sizes %d/%d first diffs %s" % (name, (r2[0], r2[2], r2[3]), r2[1].size, r_o[1].size, d[:8].tolist()), flush=True)
        assert (r_g[0], r_g[2], r_g[3]) == (r_o[0], r_o[2], r_o[3]), (tag, host_walk, chunk, r_g[0], r_g[2:], r_o[0], r_o[2:])
        assert np.array_equal(r_g[1], r_o[1]), (tag, host_walk, chunk, "samples")
    return r_o


def fam_e(rng, tag):
    bpf = int(rng.choice([1, 2, 3, 4, 6, 8, 16, 50, 100, 250, 500, 502, 504, 510, 511, 512])) if rng.random() < 0.7 else int(rng.integers(1, 513))
    p = x3hip.Params.make(20, bpf)
    spf = 20 * bpf
    frames = int(rng.choice([1, 2, 3, 5, 40, 300, 1500, 4000])) if bpf <= 16 else int(rng.choice([1, 2, 3, 7, 30, 90]))
    n = max(1, spf * frames - int(rng.integers(0, spf)) + int(rng.integers(0, 3)))
    wav = content(rng, n)
    sp = int(rng.choice([0, 0, 1, 2, 3, 18]))
    g2 = rng.random() < 0.25   # (a quarter of the trials on the second-generation kernel: it also serves the dense pass)
    ctx.set_option("enc_gen", 2 if g2 else 3)
    try:
        cut = float(rng.uniform(0.0, 0.3)) if rng.random() < 0.1 else None
        rc, out = cmp_encode(wav, p, sp, (tag, "e", bpf, n, sp, g2, cut), cut)
    finally:
        ctx.set_option("enc_gen", 3)
    if rc == 0:
        r = cmp_decode(out[(sp + 1) & ~1:], p, n, (tag, "e-dec", bpf, n))
        assert r[0] == 0 and np.array_equal(r[1], wav), (tag, "round trip")


def fam_n(rng, tag):
    """round 6: block lengths 10 and 40 on the single-pass encoders (wave encoder and second generation: a lane's run of 20
    samples is two blocks of 10 or half a block of 40), whole and ragged frames, other codes and thresholds now and then"""
    bl = int(rng.choice([10, 40]))
    per = 20 // bl if bl < 20 else 1
    bpf = int(rng.choice([1, 2, 3, 4, 6, 8, 16, 50, 100, 125, 250, 255, 256])) * (2 if bl == 10 else 1) if rng.random() < 0.7 else int(rng.integers(1, 257 * max(per, 1)))
    codes, thr = (0, 1, 3), (3, 8, 20)
    if rng.random() < 0.2:
        offsets = [6, 11, 20, 28]
        codes = tuple(int(c) for c in rng.integers(0, 4, size=3))
        thr = tuple(int(rng.integers(0, offsets[c] + 1)) for c in codes)
    p = x3hip.Params.make(bl, bpf, codes, thr)
    if x3hip.lib().x3_params_validate(C.byref(p)) != 0:
        return
    spf = bl * bpf
    frames = int(rng.choice([1, 2, 3, 5, 40, 300, 1500])) if spf <= 400 else int(rng.choice([1, 2, 3, 7, 30, 90]))
    n = max(1, spf * frames - int(rng.integers(0, spf)) + int(rng.integers(0, 3)))
    wav = content(rng, n)
    sp = int(rng.choice([0, 0, 1, 2, 3, 18]))
    g2 = rng.random() < 0.4
    ctx.set_option("enc_gen", 2 if g2 else 3)
    try:
        cut = float(rng.uniform(0.0, 0.3)) if rng.random() < 0.1 else None
        if thr != (3, 8, 20):
            cut = None   # (a parameter set the reference can panic on AND no room: which of the two it meets first is not modelled -- INTEGRATION.md, "Limits")
        rc, out = cmp_encode(wav, p, sp, (tag, "n", bl, bpf, codes, thr, n, sp, g2, cut), cut)
    finally:
        ctx.set_option("enc_gen", 3)
    if rc == 0:
        # (every code set: the reference's decoder hard-wires the sub-code widths of the default codes, so other streams
        # decode to errors or to other samples -- bit patterns the default encoder never writes, the oracle's answer exact)
        r = cmp_decode(out[(sp + 1) & ~1:], p, n, (tag, "n-dec", bl, bpf, codes, thr, n))
        # (with other thresholds the reference's own round trip is not always the identity -- BFP blocks of very few bits)
        assert codes != (0, 1, 3) or thr != (3, 8, 20) or (r[0] == 0 and np.array_equal(r[1], wav)), (tag, "round trip")


def fam_g(rng, tag):
    offsets = [6, 11, 20, 28]
    bl = int(rng.integers(1, 61))
    bpf = int(rng.integers(1, 60)) if rng.random() < 0.7 else int(rng.choice([100, 333, 500, 1000]))
    codes = (0, 1, 3) if rng.random() < 0.5 else tuple(int(c) for c in rng.integers(0, 4, size=3))
    thr = tuple(int(rng.integers(0, offsets[c] + 1)) for c in codes)
    if bl * bpf > 38000:   # the library's frames are LDS-resident: <= ~40 000 samples ("Limits")
        bpf = 38000 // bl
    p = x3hip.Params.make(bl, bpf, codes, thr)
    if x3hip.lib().x3_params_validate(C.byref(p)) != 0:
        return
    n = int(rng.integers(1, 5 * bl * bpf + 40))
    wav = content(rng, n)
    sp = int(rng.integers(0, 4))
    rc, out = cmp_encode(wav, p, sp, (tag, "g", bl, bpf, codes, thr, n, sp))
    if rc == 0:
        cmp_decode(out[(sp + 1) & ~1:], p, n, (tag, "g-dec", bl, bpf, codes, thr, n))


def draw_codes(rng):
    """(codes, thresholds) for the decode families: the defaults 70 % of the time; otherwise (1, 1, 3) -- the other code set
    the three-wave and block-per-lane kernels take -- half of the time, any valid set the other half"""
    if rng.random() < 0.7:
        return (0, 1, 3), (3, 8, 20)
    offsets = [6, 11, 20, 28]
    codes = (1, 1, 3) if rng.random() < 0.5 else tuple(int(c) for c in rng.integers(0, 4, size=3))
    thr = tuple(int(rng.integers(0, offsets[c] + 1)) for c in codes[:2]) + (int(rng.integers(0, 28)),)
    return codes, thr


def fam_k(rng, tag):
    """round 6's block-per-lane decoder: block lengths 10 and 40 (its units of 10 / 20 samples, two units per block of 40;
    the default decoder there) and 20 (option decode_blocks), frames of few and many blocks, damaged streams"""
    bl = int(rng.choice([10, 40, 20]))
    bpf = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 17, 31, 32, 33, 50, 64, 100, 250, 500])) if rng.random() < 0.8 else int(rng.integers(1, 600))
    if bl * bpf > 20000:
        bpf = 20000 // bl
    codes, thr = draw_codes(rng)
    p = x3hip.Params.make(bl, bpf, codes, thr)
    spf = bl * bpf
    n = spf * int(rng.integers(1, 9 if spf > 2000 else 200)) + int(rng.integers(0, spf))
    wav = content(rng, n)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc:
        return   # (a difference outside the code's table: the reference's encoder panics)
    s = damage(rng, stream, frame_offsets(stream)) if rng.random() < 0.6 else stream
    ctx.set_option("decode_blocks", 1)
    try:
        cmp_decode(s, p, n + 70000, (tag, "k", bl, bpf, codes, thr, n))
    finally:
        ctx.set_option("decode_blocks", 0)


def damage(rng, stream, offs):
    """a copy of `stream` with one to three of its frames (byte offsets `offs`) tampered with, perhaps truncated"""
    s = stream.copy()
    for _ in range(int(rng.integers(1, 4))):
        fi = int(rng.integers(0, len(offs)))
        off = offs[fi]
        plen = int(stream[off + 6]) << 8 | int(stream[off + 7])    # (of the intact stream: headers get damaged too)
        kind = int(rng.integers(0, 8))
        if kind == 0 and plen > 2:       # one bit, CRCs refreshed
            s[off + 20 + int(rng.integers(0, plen))] ^= 1 << int(rng.integers(0, 8)); refresh_crcs(s, off)
        elif kind == 1 and plen > 12:    # zero run
            q = off + 20 + int(rng.integers(0, plen - 10)); s[q:q + int(rng.integers(1, 10))] = 0; refresh_crcs(s, off)
        elif kind == 2 and plen > 12:    # random bytes
            q = off + 20 + int(rng.integers(0, plen - 10)); k = int(rng.integers(1, 10))
            s[q:q + k] = rng.integers(0, 256, size=k, dtype=np.uint8); refresh_crcs(s, off)
        elif kind == 3:                  # sample count in the header raised or lowered
            ns = int(s[off + 4]) << 8 | int(s[off + 5])
            ns2 = max(0, min(65535, ns + int(rng.choice([-200, -20, -1, 1, 19, 20, 21, 300, 5000]))))
            s[off + 4], s[off + 5] = ns2 >> 8, ns2 & 0xFF; refresh_crcs(s, off)
        elif kind == 4:                  # payload bit without CRC refresh
            s[off + 20 + int(rng.integers(0, max(1, plen)))] ^= 0x40
        elif kind == 5:                  # header byte, header CRC refreshed or not
            s[off + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
            if rng.random() < 0.5:
                hc = O.crc16(s[off:off + 16]); s[off + 16], s[off + 17] = hc >> 8, hc & 0xFF
        elif kind == 6 and plen > 40:    # all ones
            q = off + 20 + int(rng.integers(0, plen - 10)); s[q:q + int(rng.integers(1, 10))] = 0xFF; refresh_crcs(s, off)
        else:                            # the tail of the payload cleared (codes running off the end)
            k = int(rng.integers(1, min(40, max(2, plen)))); s[off + 20 + plen - k:off + 20 + plen] = 0; refresh_crcs(s, off)
    if rng.random() < 0.3:
        s = s[:int(rng.integers(0, s.size + 1))].copy()
    return s


def fam_d(rng, tag):
    bpf = int(rng.choice([3, 10, 50, 500]))
    codes, thr = draw_codes(rng)
    p = x3hip.Params.make(20, bpf, codes, thr)
    n = 20 * bpf * int(rng.integers(2, 9)) + int(rng.integers(0, 20 * bpf))
    wav = content(rng, n)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc:
        return   # (a difference outside the code's table: the reference's encoder panics)
    s = damage(rng, stream, frame_offsets(stream))
    cmp_decode(s, p, n + 70000, (tag, "d", bpf, codes, thr, n))


def fam_a(rng, tag):
    """.x3a archives in memory: encode == oracle; decode of intact and damaged archives through x3_x3a_decode and
    through the incremental reader (random window) == the oracle's x3a_to_wav"""
    rate = int(rng.choice([8000, 44100, 48000, 96000, 192000, 384000, 1, 999999, 1000000]))
    n = int(rng.integers(1, 60000))
    wav = content(rng, n)
    rc_o, x_o, st_o = O.x3a_encode(wav, rate)
    rc_g, x_g, st_g = ctx.x3a_encode(wav, rate)
    assert rc_g == rc_o and np.array_equal(x_g, x_o) and st_g.tolist() == st_o.tolist(), (tag, "a-enc", rate, n)
    arch = x_o
    if rng.random() < 0.7:
        hdr = 28 + (int(arch[8 + 6]) << 8 | int(arch[8 + 7]))
        offs = [hdr + o for o in frame_offsets(arch[hdr:])]
        if offs:
            arch = damage(rng, arch, offs)
        if rng.random() < 0.15 and arch.size > 40:   # the archive header itself
            arch = arch.copy(); arch[int(rng.integers(0, min(arch.size, hdr)))] ^= 1 << int(rng.integers(0, 8))
    cap = n + 70000
    r_o = O.x3a_decode(arch, wav_cap=cap)
    r_g = ctx.x3a_decode(arch, wav_cap=cap)
    assert (r_g[0],) + tuple(r_g[2:]) == (r_o[0],) + tuple(r_o[2:]), (tag, "a-dec", rate, n, r_g[0], r_g[2:], r_o[0], r_o[2:])
    assert np.array_equal(r_g[1], r_o[1]), (tag, "a-dec samples")
    # the incremental reader, as x3a_to_wav drives it
    ctx.set_option("reader_window_frames", int(rng.choice([1, 2, 3, 7, 64, 4096])))
    r = x3hip.Reader(ctx, arch)
    try:
        if r.rc:
            assert r.rc == r_o[0], (tag, "a-reader open", r.rc, r_o[0])
        else:
            out, rc = [], 0
            while True:
                rc, smp = r.next_frame()
                if rc or smp is None:
                    break
                out.append(smp)
            got = np.concatenate(out) if out else np.zeros(0, dtype=np.int16)
            assert (rc, r.frame_errors()) == (r_o[0], r_o[4]), (tag, "a-reader rc", rc, r.frame_errors(), r_o[0], r_o[4])
            assert np.array_equal(got, r_o[1]) and r.spec()[0] == r_o[2], (tag, "a-reader samples")
    finally:
        r.close()


def fam_f(rng, tag):
    """decoder::decode_frame frame by frame (with and without x3_decode_prefetch) on intact and damaged streams"""
    bpf = int(rng.choice([1, 3, 10, 50, 500]))
    p = x3hip.Params.make(20, bpf)
    n = 20 * bpf * int(rng.integers(1, 7)) + int(rng.integers(0, 20 * bpf))
    wav = content(rng, n)
    stream = O.encode(wav, oparams(p))[1]
    offs = frame_offsets(stream)
    s = damage(rng, stream, offs) if rng.random() < 0.6 else stream
    s = np.ascontiguousarray(s)
    pre = rng.random() < 0.5
    if pre:
        assert ctx.decode_prefetch(s, p) == 0
    try:
        for off in frame_offsets(s):
            plen = int(s[off + 6]) << 8 | int(s[off + 7])
            ns = int(s[off + 4]) << 8 | int(s[off + 5])
            if ns == 0:
                continue
            payload = s[off + 20:off + 20 + plen]
            cap = int(rng.choice([ns, ns, ns + 5, max(0, ns - 1)]))
            r_o = O.decode_frame(payload, ns, oparams(p), wav_cap=cap)
            r_g = ctx.decode_frame(payload, ns, p, wav_cap=cap)
            assert r_g[0] == r_o[0], (tag, "f rc", bpf, off, ns, plen, cap, r_g[0], r_o[0])
            if r_o[0] == 0:
                assert np.array_equal(r_g[1], r_o[1]), (tag, "f samples", bpf, off)
    finally:
        if pre:
            ctx.decode_prefetch(None)


def fam_b_ragged(rng, tag):
    """clips of DIFFERENT lengths: x3_encode_batch on host buffers (one launch set through x3_encode_frames_dev) and the
    device entry itself with clips at arbitrary sample offsets, against per-clip oracle streams; decoded back by frame
    index and per-frame sample offsets (with and without the promise that they are multiples of four)"""
    bpf = int(rng.choice([1, 2, 7, 8, 100, 500, 501, 512]))
    bl = 20 if rng.random() < 0.6 else int(rng.choice([7, 19, 33, 10, 40, 10, 40]))   # (10 and 40: the single-pass encoders' table forms since round 6)
    p = x3hip.Params.make(bl, bpf)
    spf = bl * bpf
    n_clips = int(rng.integers(1, 12))
    clips = [content(rng, int(rng.integers(1, 3 * spf + 40)) if rng.random() < 0.9 else 1) for _ in range(n_clips)]
    exp = [O.encode(c, oparams(p)) for c in clips]
    if any(e[0] != 0 for e in exp):
        return
    rc, out, offs, stats = ctx.encode_batch(clips, p)
    assert rc == 0, (tag, "b-ragged host", rc)
    for i, e in enumerate(exp):
        assert np.array_equal(out[offs[i]:offs[i + 1]], e[1]), (tag, "b-ragged host", i, bl, bpf, clips[i].size)
    assert stats.tolist() == np.sum([e[2] for e in exp], axis=0).tolist(), (tag, "b-ragged stats")
    # the device entry: clips anywhere (even / multiple-of-four / arbitrary offsets)
    mode = int(rng.integers(0, 3))
    step = [1, 2, 4][mode]
    starts, pos = [], 0
    for c in clips:
        pos += step * int(rng.integers(0, 9))
        starts.append(pos)
        pos += c.size
        pos += (-pos) % step
    total = pos + 16
    buf = np.zeros(total, dtype=np.int16)
    so, sn = [], []
    for s0, c in zip(starts, clips):
        buf[s0:s0 + c.size] = c
        for k in range(0, c.size, spf):
            so.append(s0 + k); sn.append(min(spf, c.size - k))
    F = len(so)
    L = x3hip.lib()
    cap = sum(L.x3_encode_bound(int(c.size), C.byref(p)) for c in clips) + 64
    d_wav = ctx.alloc(2 * total); d_out = ctx.alloc(cap + 16); d_off = ctx.alloc(8 * (F + 1)); d_wo = ctx.alloc(8 * F); d_back = ctx.alloc(2 * total)
    try:
        ctx.upload(d_wav, buf)
        sp = int(rng.choice([0, 0, 1, 6]))
        assert ctx.encode_frames_dev(d_wav, so, sn, p, d_out, cap, sp, d_off) == 0
        rc, end, st = ctx.encode_result()
        assert rc == 0, (tag, "b-ragged dev", rc)
        body0 = (sp + 1) & ~1
        expect = np.concatenate([e[1] for e in exp])
        got = ctx.download(d_out, end)
        assert end == body0 + expect.size and np.array_equal(got[body0:], expect), (tag, "b-ragged dev", bl, bpf, mode, sp)
        # (frames of 20 x 512 samples at most: a payload beyond the walk's 24 KB buffer is the reference's FrameLength)
        if tuple(p.codes) == (0, 1, 3) and step >= 2 and bl == 20:
            ctx.upload(d_wo, np.array(so, dtype=np.uint64)); ctx.upload(d_back, np.zeros(total, dtype=np.int16))
            ctx.set_option("wav_offsets_x4", 1 if (step == 4 and spf % 4 == 0) else 0)
            try:
                assert ctx.decode_dev(d_out, end, d_off, F, p, d_back, total, d_wav_offsets=d_wo) == 0
                r = ctx.decode_result()
            finally:
                ctx.set_option("wav_offsets_x4", 0)
            assert r[:3] == (0, F, 0), (tag, "b-ragged decode", r)
            assert np.array_equal(ctx.download(d_back, 2 * total).view(np.int16), buf), (tag, "b-ragged round trip", bl, bpf, mode)
    finally:
        for d in (d_wav, d_out, d_off, d_wo, d_back):
            ctx.free(d)


def fam_b(rng, tag):
    """clips of equal length through the device batch API against per-clip oracle streams"""
    if rng.random() < 0.5:
        return fam_b_ragged(rng, tag)
    bpf = int(rng.choice([2, 8, 100, 500]))
    p = x3hip.Params.make(20, bpf)
    spf = 20 * bpf
    n_clips = int(rng.integers(1, 9))
    npc = 8 * int(rng.integers(1, max(2, spf * 5 // 8)))
    wav = content(rng, npc * n_clips)
    L = x3hip.lib()
    fpc = L.x3_num_frames(npc, C.byref(p))
    F = fpc * n_clips
    cap = L.x3_encode_bound(npc, C.byref(p)) * n_clips
    d_wav = ctx.alloc(2 * wav.size); d_out = ctx.alloc(cap + 16); d_off = ctx.alloc(8 * (F + 1)); d_back = ctx.alloc(2 * wav.size)
    try:
        ctx.upload(d_wav, wav)
        assert ctx.encode_dev(d_wav, npc, p, d_out, cap, 0, d_off, n_clips=n_clips, clip_stride=npc) == 0
        rc, pos, st = ctx.encode_result()
        assert rc == 0, (tag, rc)
        expect = np.concatenate([O.encode(wav[c * npc:(c + 1) * npc], oparams(p))[1] for c in range(n_clips)])
        got = ctx.download(d_out, pos)
        assert pos == expect.size and np.array_equal(got, expect), (tag, "b", bpf, n_clips, npc)
        assert ctx.decode_dev(d_out, cap, d_off, F, p, d_back, wav.size, n_per_clip=npc, n_clips=n_clips, clip_stride=npc) == 0
        r = ctx.decode_result()
        assert r[:3] == (0, F, 0), (tag, r)
        assert np.array_equal(ctx.download(d_back, 2 * wav.size).view(np.int16), wav), (tag, "b round trip")
    finally:
        for d in (d_wav, d_out, d_off, d_back):
            ctx.free(d)


def _write_wav(path, wav, rate, extra=()):
    import struct
    data = np.ascontiguousarray(wav, dtype="<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, rate, rate * 2, 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, payload in extra:
        body += cid + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    body += b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def fam_w(rng, tag):
    """files: x3_wav_to_x3a / x3_x3a_to_wav (chunked pipeline, random chunk sizes and worker counts) == the oracle's
    wav_to_x3a / x3a_to_wav, byte for byte; damaged archives too"""
    import tempfile
    d = tempfile.mkdtemp(prefix="x3fz", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        rate = int(rng.choice([8000, 44100, 96000, 192000]))
        n = int(rng.integers(0, 400000)) if rng.random() < 0.8 else int(rng.integers(0, 30))
        wav = content(rng, n) if n else np.zeros(0, dtype=np.int16)
        a, b_o, b_g, c_o, c_g = (os.path.join(d, x) for x in ("in.wav", "o.x3a", "g.x3a", "o.wav", "g.wav"))
        extra = [(b"LIST", bytes(int(rng.integers(0, 9))))] if rng.random() < 0.3 else []
        _write_wav(a, wav, rate, extra)
        ctx.set_option("file_chunk_frames", int(rng.choice([1, 2, 3, 5, 16, 64])))
        ctx.set_option("file_workers", int(rng.choice([1, 2, 3, 4])))
        rc_o, st_o = O.wav_to_x3a(a, b_o)
        rc_g, st_g = ctx.wav_to_x3a(a, b_g)
        assert rc_g == rc_o, (tag, "w enc rc", rc_g, rc_o)
        if rc_o == 0:
            x_o, x_g = open(b_o, "rb").read(), open(b_g, "rb").read()
            assert x_o == x_g and st_g.tolist() == st_o.tolist(), (tag, "w enc bytes", n, rate)
            if rng.random() < 0.5 and len(x_o) > 400:
                arch = np.frombuffer(x_o, dtype=np.uint8)
                hdr = 28 + (int(arch[14]) << 8 | int(arch[15]))
                offs = [hdr + o for o in frame_offsets(arch[hdr:])]
                if offs:
                    arch = damage(rng, arch, offs)
                    open(b_o, "wb").write(bytes(arch))
            r_o = O.x3a_to_wav(b_o, c_o)
            r_g = ctx.x3a_to_wav(b_o, c_g)
            assert tuple(r_g) == tuple(r_o), (tag, "w dec", r_g, r_o)
            if os.path.exists(c_o) or os.path.exists(c_g):
                assert open(c_o, "rb").read() == open(c_g, "rb").read(), (tag, "w dec bytes")
    finally:
        ctx.set_option("file_chunk_frames", 800)
        ctx.set_option("file_workers", 4)
        import shutil
        shutil.rmtree(d, ignore_errors=True)


def fam_m(rng, tag):
    """multi-channel extension: x3_encode_mc / x3_decode_stream_mc == the oracle's x3o_encode_mc / x3o_decode_stream_mc over
    channels x geometry x codes / thresholds x content x start position, intact, damaged (CRCs refreshed or not) and
    truncated streams, wrong channel counts"""
    n_ch = int(rng.integers(1, 9))
    bl = int(rng.choice([20, 20, 20, 7, 33, 60, 1]))
    bpf = int(rng.integers(1, 200))
    n = int(rng.integers(1, 5 * bl * bpf + 50)) if rng.random() < 0.9 else int(rng.integers(1, 4))
    codes, thr = draw_codes(rng)
    p, po = x3hip.Params.make(bl, bpf, codes, thr), O.Params.make(bl, bpf, codes, thr)
    wavs = [content(rng, n) for _ in range(n_ch)]
    start = int(rng.integers(0, 5))
    cap = n_ch * O.encode_bound(n, po) + start + 64   # (the same capacity on both sides: running out of it is part of the result)
    rc_o, x_o, st_o = O.encode_mc(wavs, po, start_pos=start, cap=cap)
    rc_g, x_g, st_g = ctx.encode_mc(wavs, p, start_pos=start, cap=cap)
    assert rc_g == rc_o, (tag, "m enc rc", rc_g, rc_o, n_ch, bl, bpf, n)
    if rc_o:
        return
    assert np.array_equal(x_g[start:], x_o[start:]) and st_g.tolist() == st_o.tolist(), (tag, "m enc bytes", n_ch, bl, bpf, n)
    s = x_o[start + (start & 1):].copy()
    what = int(rng.integers(0, 4))
    if what == 1 and s.size > 40:
        at = int(rng.integers(0, s.size))
        s[at] ^= 1 << int(rng.integers(0, 8))
        if rng.random() < 0.5:       # CRCs made good again: the decoder, not the check pass, meets the damage
            refresh_crcs(s, max(o for o in frame_offsets(x_o[start + (start & 1):]) if o <= at))
    elif what == 2 and s.size > 40:
        s = s[: int(rng.integers(1, s.size))]
    ask = n_ch if what != 3 else int(rng.integers(1, 9))
    got = ctx.decode_stream_mc(s, ask, p, wav_cap=n + 8)
    want = O.decode_stream_mc(s, ask, po, wav_cap=n + 8)
    assert (got[0], got[2], got[3]) == (want[0], want[2], want[3]), (tag, "m dec", got[0], got[2:], want[0], want[2:])
    for k in range(ask):
        assert np.array_equal(got[1][k], want[1][k]), (tag, "m samples", k)


fams = {"w": fam_w, "e": fam_e, "g": fam_g, "d": fam_d, "b": fam_b, "a": fam_a, "f": fam_f, "m": fam_m, "k": fam_k, "n": fam_n}


def fam_s(rng, tag):
    """the segment index (x3_encode_dev_seg / x3_decode_dev_seg): mixed content in frames of up to 512 blocks, one clip or a
    batch; the encoder's index = the one a frame-by-frame decode records; decoding by it -- every entry, every second one, as
    the library picks -- gives the oracle's samples, with the stream intact or damaged (CRCs refreshed or not) and with the
    index intact, partly overwritten or random"""
    L = x3hip.lib()
    bpf = int(rng.choice([8, 16, 33, 64, 100, 128, 250, 256, 500, 501, 512]))
    p = x3hip.Params.make(20, bpf)
    spf = 20 * bpf
    n_clips = int(rng.choice([1, 1, 1, 2, 5]))
    n_per = spf * int(rng.integers(1, 6)) + int(rng.choice([0, 0, 1, 19, 20, 21, spf // 2, spf - 1]))
    if n_clips > 1:
        n_per = (n_per + 3) & ~3
    sb = int(rng.choice([4, 8, 16, 32, 64, 128]))
    wavs = [content(rng, n_per) for _ in range(n_clips)]
    wav = np.concatenate(wavs)
    n = wav.size
    F = L.x3_num_frames(n_per, C.byref(p)) * n_clips
    cap = L.x3_encode_bound(n_per, C.byref(p)) * n_clips
    ne = max(1, L.x3_seg_index_entries(F, C.byref(p), sb))
    d = [ctx.alloc(2 * n + 64), ctx.alloc(cap + 64), ctx.alloc(8 * (F + 1)), ctx.alloc(2 * n + 64), ctx.alloc(8 * ne + 8), ctx.alloc(8 * ne + 8)]
    d_wav, d_out, d_off, d_back, d_seg, d_seg2 = d
    try:
        ctx.upload(d_wav, wav)
        ctx.upload(d_seg, rng.integers(0, 1 << 62, ne, dtype=np.uint64))
        assert ctx.encode_dev_seg(d_wav, n_per, p, d_out, cap, d_seg, sb, 0, d_off, n_clips=n_clips) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0, (tag, rc)
        stream = ctx.download(d_out, pos)
        ref = np.concatenate([O.encode(w, oparams(p))[1] for w in wavs])
        assert np.array_equal(stream, ref), (tag, "stream")
        nseg = (bpf + sb - 1) // sb
        have_index = nseg >= 2 and ctx.get_option("enc_gen_in_use") == 3
        if nseg >= 2:
            assert ctx.decode_dev_seg(d_out, pos, d_off, F, p, d_back, n, d_seg2, sb, record=True, n_per_clip=n_per, n_clips=n_clips) == 0
            assert ctx.decode_result() == (0, F, 0, n), (tag, "record")
            if have_index:
                a, b = ctx.download(d_seg, 8 * ne, np.uint64), ctx.download(d_seg2, 8 * ne, np.uint64)
                assert np.array_equal(a, b), (tag, "index", np.flatnonzero(a != b)[:8].tolist())
        # damage: the stream, the index, both, neither
        offs = frame_offsets(stream)
        bad = stream
        if rng.random() < 0.6:
            # payload damage only (the device API places frames by the layout, the oracle's walk by the headers it reads:
            # the two agree as long as the headers do), CRCs refreshed or not
            bad = stream.copy()
            for _ in range(int(rng.integers(1, 4))):
                off = offs[int(rng.integers(0, len(offs)))]
                plen = int(stream[off + 6]) << 8 | int(stream[off + 7])
                if plen <= 2:
                    continue
                q = off + 20 + int(rng.integers(2, plen))
                k = min(int(rng.integers(1, 10)), off + 20 + plen - q)
                kind = int(rng.integers(0, 4))
                if kind == 0: bad[q] ^= np.uint8(1 << int(rng.integers(0, 8)))
                elif kind == 1: bad[q:q + k] = 0
                elif kind == 2: bad[q:q + k] = rng.integers(0, 256, size=k, dtype=np.uint8)
                else: bad[q:q + k] = 0xFF
                if rng.random() < 0.7:
                    refresh_crcs(bad, off)
        idx = ctx.download(d_seg2 if nseg >= 2 else d_seg, 8 * ne, np.uint64)
        r = rng.random()
        if r < 0.25 and ne > 1:
            k = int(rng.integers(1, ne)); idx[k] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 49)))
        elif r < 0.4 and ne > 1:
            sel = rng.random(ne) < 0.2; sel[0] = False
            idx[sel] = rng.integers(0, 1 << 49, int(sel.sum()), dtype=np.uint64)
        elif r < 0.45:
            idx[0] = 0
        ctx.upload(d_out, bad); ctx.upload(d_seg, idx)
        # the oracle's walk over the same frames (frame f's bytes at offs[f]; a bad frame stops it)
        want = O.decode_stream(bad, oparams(p), wav_cap=n + 70000)
        for want_st in (0, nseg, 2):
            ctx.set_option("seg_stretches", want_st)
            ctx.upload(d_back, np.zeros(n, dtype=np.int16))
            assert ctx.decode_dev_seg(d_out, pos, d_off, F, p, d_back, n, d_seg, sb, n_per_clip=n_per, n_clips=n_clips) == 0
            rc_d, first_bad, st, before = ctx.decode_result()
            if n_clips == 1:
                assert rc_d == 0 and first_bad == want[2] and before == want[1].size, (tag, want_st, first_bad, st, before, want[2], want[1].size)
                assert np.array_equal(ctx.download(d_back, 2 * before, np.int16), want[1]), (tag, want_st, "samples")
            else:   # (a batch: the oracle's walk knows nothing about clips; intact streams only)
                if bad is stream:
                    assert (rc_d, first_bad, st, before) == (0, F, 0, n), (tag, want_st)
                    assert np.array_equal(ctx.download(d_back, 2 * n, np.int16), wav), (tag, want_st, "samples")
    finally:
        ctx.set_option("seg_stretches", 0)
        for q in d:
            ctx.free(q)


fams["s"] = fam_s


def _frame_verdicts(stream, offs, p):
    """per frame (oracle): (status, samples) -- header CRC, key, channels, the walk's length checks, payload CRC, then
    decoder::decode_frame: the statuses x3_decode_dev gives"""
    out = []
    for f, off in enumerate(offs):
        h = stream[off:off + 20]
        samples, plen = int(h[4]) << 8 | int(h[5]), int(h[6]) << 8 | int(h[7])
        payload = stream[off + 20:off + 20 + plen]
        if O.crc16(h[:16]) != (int(h[16]) << 8 | int(h[17])):
            out.append((13, None))
        elif (int(h[0]) << 8 | int(h[1])) != 0x7833:
            out.append((11, None))
        elif int(h[3]) > 1:
            out.append((6, None))
        elif plen >= 0x7fe0:
            out.append((10, None))
        elif off + 20 + plen > stream.size:   # (a payload past the stream's end: the offsets are not this stream's)
            out.append((24, None))
        elif plen > 24576:             # (the reader's buffer, decodefile.rs:118-121: x3_decode_dev checks it too)
            out.append((12, None))
        elif O.crc16(payload) != (int(h[18]) << 8 | int(h[19])):
            out.append((14, None))
        elif samples == 0 or plen < 2:
            out.append((24, None))
        else:
            rc, w = O.decode_frame(payload, samples, oparams(p))
            out.append((rc, w if rc == 0 else None))
    return out


def _fam_windows(rng, tag, index):
    """random access: windows of a random stream against the oracle's verdict of every frame that covers them; the segment
    index recorded by a decode (index = "decode") or built by x3_seg_index_build_dev on the stream as it is, damage
    included (index = "walk": there always with an index)"""
    r = rng.random()
    if r < 0.6:
        p = x3hip.Params.default()
    elif r < 0.8:
        p = x3hip.Params.make(int(rng.choice([10, 40])), int(rng.choice([100, 256, 500])))
    else:
        bl = int(rng.integers(2, 61))
        codes = (0, 1, 3) if rng.random() < 0.5 else tuple(int(c) for c in rng.integers(0, 4, size=3))
        p = x3hip.Params.make(bl, int(rng.integers(1, max(2, 30000 // bl))), codes)
        if x3hip.lib().x3_params_validate(C.byref(p)) != 0:
            return
    spf = p.block_len * p.blocks_per_frame
    n = int(rng.integers(1, 12 * spf + 100))
    wav = content(rng, n)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc != 0:
        return
    offs = frame_offsets(stream)
    so = [0]
    for off in offs:
        so.append(so[-1] + (int(stream[off + 4]) << 8 | int(stream[off + 5])))
    if so[-1] != n:   # (frames whose payload outgrows the header's length field: not a stream the reader can walk)
        return
    bad = stream.copy()
    if rng.random() < 0.4:
        for _ in range(int(rng.integers(1, 4))):
            off = offs[int(rng.integers(0, len(offs)))]
            plen = int(stream[off + 6]) << 8 | int(stream[off + 7])
            kind = int(rng.integers(0, 4))
            if kind == 0 and plen > 2:      # payload bits, CRC refreshed (a decode error or other samples) or not
                q = off + 20 + int(rng.integers(2, plen))
                k = min(int(rng.integers(1, 12)), off + 20 + plen - q)
                bad[q:q + k] = 0 if rng.random() < 0.5 else rng.integers(0, 256, size=k, dtype=np.uint8)
                if rng.random() < 0.7:
                    refresh_crcs(bad, off)
            elif kind == 1:                 # a header byte other than the sample count
                q = off + int(rng.choice([0, 1, 2, 3, 6, 7, 8, 12, 16, 17, 18, 19]))
                bad[q] ^= np.uint8(1 << int(rng.integers(0, 8)))
            elif kind == 2 and plen > 2:    # one payload bit
                bad[off + 20 + int(rng.integers(0, plen))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    verdicts = _frame_verdicts(bad, offs, p)
    d = []
    try:
        d_off = ctx.alloc(8 * (len(offs) + 1)); d.append(d_off)
        ctx.upload(d_off, np.array(offs + [stream.size], dtype=np.uint64))
        sb = int(rng.choice([0, 4, 32, 64]))
        if index == "walk" and sb == 0:
            sb = 8
        src = x3hip.WindowSource(ctx, bad, p, seg_blocks=sb, frame_offsets=d_off, n_frames=len(offs), index=index)
        d.extend(src._own); src._own = []
        assert src.total == n, (tag, "total", src.total, n)
        if src.d_seg_index is not None and rng.random() < 0.3:   # a damaged index: a hint, never trusted
            ne = x3hip.lib().x3_seg_index_entries(len(offs), C.byref(p), src.seg_blocks)
            idx = ctx.download(src.d_seg_index, 8 * ne, np.uint64)
            if ne > 1:
                sel = rng.random(ne) < 0.2; sel[0] = False
                idx[sel] = rng.integers(0, 1 << 49, int(sel.sum()), dtype=np.uint64)
                if rng.random() < 0.3:
                    idx[1:] = np.roll(idx[1:], int(rng.integers(1, 5)))
            ctx.upload(src.d_seg_index, idx)
        L = int(rng.choice([1, 2, 19, 20, 21, 333, spf, int(rng.integers(1, n + 1))]))
        L = max(1, min(L, n))
        nw = int(rng.integers(1, 40))
        starts = [int(v) for v in rng.integers(0, n - L + 1, nw)]
        wild = [n - L + 1, n, 2 ** 63, 2 ** 64 - 1, 2 ** 64 - L, int(rng.integers(n - L + 1, 2 ** 62))]
        for _ in range(int(rng.integers(0, 3))):
            starts.insert(int(rng.integers(0, len(starts) + 1)), wild[int(rng.integers(0, len(wild)))])
        fmt = int(rng.integers(0, 2))
        rows, st = src.decode(starts, L, fmt)
        for w, s0 in enumerate(starts):
            want = np.zeros(L, dtype=np.int16)
            wst = 0
            if s0 > n - L:
                wst = 24
            else:
                f = int(np.searchsorted(so, s0, side="right")) - 1
                while f < len(offs) and so[f] < s0 + L:
                    v, samples = verdicts[f]
                    if v:
                        wst = v
                        break
                    lo, hi = max(so[f], s0), min(so[f + 1], s0 + L)
                    want[lo - s0:hi - s0] = samples[lo - so[f]:hi - so[f]]
                    f += 1
            assert st[w] == wst, (tag, "status", w, s0, L, int(st[w]), wst)
            got = rows[w].view(np.uint32) if fmt else rows[w]
            exp = (want.astype(np.float32) / np.float32(32768.0)).view(np.uint32) if fmt else want
            assert np.array_equal(got, exp), (tag, "samples", w, s0, L, fmt, np.flatnonzero(got != exp)[:8].tolist())
    finally:
        for q in d:
            ctx.free(q)


def fam_c(rng, tag):
    _fam_windows(rng, tag, "decode")


def fam_x(rng, tag):
    """(c) by a walk-built index: content x geometry x damage, any block length and code set"""
    _fam_windows(rng, tag, "walk")


fams["c"] = fam_c
fams["x"] = fam_x


def fam_r(rng, tag, diff=False, fir=None, tone=False, bank=False):
    """range levels (diff: of the first difference, against signal_range_levels_ref -- family (l); fir: behind that filter,
    against fir_range_levels_ref -- family (t); tone: against a drawn oscillator, tone_range_levels_ref, then the same
    frames as a corpus of random entries -- family (p)): the records, row offsets and statuses of random ranges of a random stream -- any geometry, damaged
    frames, a damaged or walk-built index, packed (exact, cut or roomy capacity) and padded -- against range_levels_ref on
    the oracle's frame verdicts; the output arrays are filled with 0x5A and what no call may write must keep it"""
    import range_levels_ref as RL
    r = rng.random()
    if r < 0.5:
        p = x3hip.Params.make(20, int(rng.choice([20, 100, 500])))
    elif r < 0.8:
        p = x3hip.Params.make(int(rng.choice([10, 40])), int(rng.choice([25, 100, 256])))
    else:
        bl = int(rng.integers(2, 61))
        codes = (0, 1, 3) if rng.random() < 0.5 else tuple(int(c) for c in rng.integers(0, 4, size=3))
        p = x3hip.Params.make(bl, int(rng.integers(1, max(2, 8000 // bl))), codes)
        if x3hip.lib().x3_params_validate(C.byref(p)) != 0:
            return
    spf = p.block_len * p.blocks_per_frame
    n = int(rng.integers(1, 10 * spf + 100))
    wav = content(rng, n)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc != 0:
        return
    offs = frame_offsets(stream)
    so = [0]
    for off in offs:
        so.append(so[-1] + (int(stream[off + 4]) << 8 | int(stream[off + 5])))
    if so[-1] != n:
        return
    bad = stream.copy()
    if rng.random() < 0.5:
        for _ in range(int(rng.integers(1, 4))):
            off = offs[int(rng.integers(0, len(offs)))]
            plen = int(stream[off + 6]) << 8 | int(stream[off + 7])
            kind = int(rng.integers(0, 3))
            if kind == 0 and plen > 2:      # payload bits, CRC refreshed (a decode error or other samples) or not
                q = off + 20 + int(rng.integers(2, plen))
                k = min(int(rng.integers(1, 12)), off + 20 + plen - q)
                bad[q:q + k] = 0 if rng.random() < 0.5 else rng.integers(0, 256, size=k, dtype=np.uint8)
                if rng.random() < 0.7:
                    refresh_crcs(bad, off)
            elif kind == 1:                 # a header byte other than the sample count
                q = off + int(rng.choice([0, 1, 2, 3, 6, 7, 8, 12, 16, 17, 18, 19]))
                bad[q] ^= np.uint8(1 << int(rng.integers(0, 8)))
            elif plen > 2:                  # one payload bit
                bad[off + 20 + int(rng.integers(0, plen))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    verdicts = _frame_verdicts(bad, offs, p)
    so_a = np.array(so, dtype=np.uint64)
    nr = int(rng.integers(1, 60))
    kind = int(rng.integers(0, 4))
    if kind == 0:      # anything
        lens = [int(rng.choice([0, 1, 19, 20, 21, spf - 1, spf, spf + 1, int(rng.integers(0, n + 1))])) for _ in range(nr)]
    elif kind == 1:    # short
        lens = [int(v) for v in rng.integers(0, 64, nr)]
    elif kind == 2:    # all long: many ranges over the same frames (pairs beyond the workspace's)
        lens = [int(rng.integers(max(1, n - 7), n + 1)) for _ in range(nr)]
    else:              # sliding
        L0, hop = int(rng.integers(1, n + 1)), int(rng.integers(1, spf + 1))
        lens = [L0] * nr
    lens = [min(v, n) for v in lens]
    starts = [int(rng.integers(0, n - v + 1)) for v in lens]
    if kind == 3:
        starts = [min(w * hop, n - L0) for w in range(nr)]
    if diff:           # starts at a frame's or a stretch's first sample, and one behind it
        for w in range(nr):
            if rng.random() < 0.4:
                at = int(rng.integers(0, len(offs))) * spf + int(rng.choice([0, 1, 1 + 4 * p.block_len, 1 + 32 * p.block_len]))
                starts[w] = min(at, n - lens[w])
    if fir is not None:   # ... T - 1 either side of a frame's or a stretch's first sample
        T = len(fir.taps)
        for w in range(nr):
            if rng.random() < 0.5:
                at = int(rng.integers(0, len(offs))) * spf + int(rng.choice([0, 1, 1 + 4 * p.block_len, 1 + 32 * p.block_len]))
                at += int(rng.choice([-(T - 1), -1, 0, 1, T - 2, T - 1, T]))
                starts[w] = max(0, min(at, n - lens[w]))
    if tone:   # ... one either side of a frame's or a stretch's first sample; the oscillator
        for w in range(nr):
            if rng.random() < 0.5:
                at = int(rng.integers(0, len(offs))) * spf + int(rng.choice([0, 1, 1 + 4 * p.block_len, 1 + 32 * p.block_len]))
                at += int(rng.choice([-1, 0, 1]))
                starts[w] = max(0, min(at, n - lens[w]))
        step = int(rng.choice([0, 1 << 22, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) | 1]))
        tab = None if rng.random() < 0.5 else rng.integers(-32768, 32768, (1024, 2)).astype(np.int16)
    if bank:   # family (u): a bank around the family's step
        n_tones = int(rng.integers(1, 9))
        steps = [int(rng.choice([0, 1 << 30, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) | 1]))
                 for _ in range(n_tones)]
        steps[int(rng.integers(0, n_tones))] = step
        if n_tones > 1 and rng.random() < 0.3:
            steps[-1] = steps[0]   # equal steps, equal planes
    wild = [n, n + 1, 2 ** 63, 2 ** 64 - 1, int(rng.integers(n + 1, 2 ** 62))]
    for _ in range(int(rng.integers(0, 3))):
        w = int(rng.integers(0, nr))
        starts[w] = wild[int(rng.integers(0, len(wild)))]
    for _ in range(int(rng.integers(0, 2))):
        lens[int(rng.integers(0, nr))] = int(rng.choice([n + 1, 2 ** 32 - 1]))
    bin_len = int(rng.choice([0, 1, 2, 7, 20, 100, spf - 1, spf, spf + 1, 2 ** 32, int(rng.integers(1, n + 2))]))
    rows = [RL.rows_of(v, bin_len) for v in lens]
    if sum(rows) > 1 << 21:               # (a 2^32 - 1 length at a fine bin: bound the buffers of a trial)
        bin_len = 1 << 20
        rows = [RL.rows_of(v, bin_len) for v in lens]
    layout = int(rng.integers(0, 4))
    if layout == 0:
        stride, cap = 0, sum(rows)
    elif layout == 1:
        stride, cap = 0, max(1, int(rng.integers(1, sum(rows) + 1)))
    elif layout == 2:
        stride, cap = 0, sum(rows) + int(rng.integers(1, 5000))
    else:
        stride = int(rng.choice([1, max(rows), max(1, max(rows) // 2), max(rows) + 3]))
        cap = nr * stride + int(rng.integers(0, 3))
    if tone:
        import tone_range_levels_ref as TRL
        want = TRL.range_levels(verdicts, so_a, starts, lens, bin_len, stride, cap, step, tab)
    elif fir is not None:
        import fir_range_levels_ref as FRL
        want = FRL.range_levels(verdicts, so_a, starts, lens, bin_len, stride, cap, fir.taps, fir.shift)
    elif diff:
        import signal_range_levels_ref as SRL
        want = SRL.range_levels(verdicts, so_a, starts, lens, bin_len, stride, cap, SRL.DIFF)
    else:
        want = RL.range_levels(verdicts, so_a, starts, lens, bin_len, stride, cap)
    d = []
    try:
        d_off = ctx.alloc(8 * (len(offs) + 1)); d.append(d_off)
        ctx.upload(d_off, np.array(offs + [stream.size], dtype=np.uint64))
        index = "walk" if rng.random() < 0.6 or p.block_len != 20 or tuple(p.codes) != (0, 1, 3) else "decode"
        sb = int(rng.choice([0, 4, 8, 32]))
        src = x3hip.WindowSource(ctx, bad, p, seg_blocks=sb, frame_offsets=d_off, n_frames=len(offs), index=index)
        d.extend(src._own); src._own = []
        assert src.total == n, (tag, "total", src.total, n)
        if src.d_seg_index is not None and rng.random() < 0.3:   # a damaged index: a hint, never trusted
            ne = x3hip.lib().x3_seg_index_entries(len(offs), C.byref(p), src.seg_blocks)
            idx = ctx.download(src.d_seg_index, 8 * ne, np.uint64)
            if ne > 1:
                sel = rng.random(ne) < 0.2; sel[0] = False
                idx[sel] = rng.integers(0, 1 << 49, int(sel.sum()), dtype=np.uint64)
            ctx.upload(src.d_seg_index, idx)
        sizes = (32 * cap, 8 * (nr + 1), 4 * nr)
        guard = 64
        bufs = [ctx.alloc(v + guard) for v in sizes] + [ctx.alloc(8 * nr), ctx.alloc(4 * nr)]
        d.extend(bufs)
        for q, v in zip(bufs[:3], sizes):
            ctx.upload(q, np.full(v + guard, 0x5A, dtype=np.uint8))
        ctx.upload(bufs[3], np.array(starts, dtype=np.uint64))
        ctx.upload(bufs[4], np.array(lens, dtype=np.uint32))
        if tone:
            d_tab = ctx.tone_table_dev()
            if tab is not None:
                d_tab = ctx.alloc(4096); d.append(d_tab)
                ctx.upload(d_tab, tab)
            level_tone = x3hip.LevelTone(step, 0, d_tab)
            if bank:   # (spare steps: garbage)
                level_bank = x3hip.LevelToneBank(n_tones, 0, d_tab, (C.c_uint32 * 8)(*(steps + [0xDEADBEEF] * (8 - n_tones))))
            rc = src.tone_range_levels_into(bufs[3], bufs[4], nr, bin_len, stride, bufs[0], cap, bufs[1], bufs[2], level_tone)
        elif fir is not None:
            rc = src.fir_range_levels_into(bufs[3], bufs[4], nr, bin_len, stride, bufs[0], cap, bufs[1], bufs[2], fir)
        else:
            rc = src.range_levels_into(bufs[3], bufs[4], nr, bin_len, stride, bufs[0], cap, bufs[1], bufs[2],
                                       signal=x3hip.LEVEL_SIGNAL_DIFF if diff else x3hip.LEVEL_SIGNAL_SAMPLES)
        assert rc == 0, (tag, "rc", rc, ctx.last_error())
        res = ctx.range_levels_result()
        raw = [ctx.download(q, v + guard) for q, v in zip(bufs[:3], sizes)]
        for name, a, v in zip(("levels", "offsets", "status"), raw, sizes):
            assert (a[v:] == 0x5A).all(), (tag, "canary", name)
        st = raw[2][:sizes[2]].view(np.int32)
        assert np.array_equal(st, want[2]), (tag, "status", np.flatnonzero(st != want[2])[:8].tolist(), bin_len, stride, cap)
        assert np.array_equal(raw[1][:sizes[1]].view(np.uint64), want[1]), (tag, "offsets")
        got = raw[0][:sizes[0]].reshape(cap, 32)
        assert np.array_equal(got, want[0]), (tag, "records", np.flatnonzero((got != want[0]).any(axis=1))[:8].tolist(), bin_len, stride, cap)
        nbad = np.flatnonzero(st)
        assert res == (0, nbad.size, int(nbad[0]) if nbad.size else nr, int(st[nbad[0]]) if nbad.size else 0, sum(rows)), (tag, res)
        if bank and n_tones * cap <= 1 << 22:   # (128 MB of records at most) the bank: every plane against the definition at its step and the single call's bytes, shared results once
            counters = (ctx.get_option("last_range_levels_replays"), ctx.get_option("last_range_levels_overflow"))
            bsize = 32 * n_tones * cap
            bb = [ctx.alloc(bsize + guard), ctx.alloc(sizes[1] + guard), ctx.alloc(sizes[2] + guard)]
            d.extend(bb)
            for q, v in zip(bb, (bsize, sizes[1], sizes[2])):
                ctx.upload(q, np.full(v + guard, 0x5A, dtype=np.uint8))
            rc = src.tone_bank_range_levels_into(bufs[3], bufs[4], nr, bin_len, stride, bb[0], cap, bb[1], bb[2], level_bank)
            assert rc == 0, (tag, "bank rc", rc, ctx.last_error())
            assert ctx.range_levels_result() == res, (tag, "bank result")
            assert (ctx.get_option("last_range_levels_replays"), ctx.get_option("last_range_levels_overflow")) == counters, (tag, "bank counters")
            braw = [ctx.download(q, v + guard) for q, v in zip(bb, (bsize, sizes[1], sizes[2]))]
            for name, a, v in zip(("levels", "offsets", "status"), braw, (bsize, sizes[1], sizes[2])):
                assert (a[v:] == 0x5A).all(), (tag, "bank canary", name)
            assert np.array_equal(braw[1], raw[1]) and np.array_equal(braw[2], raw[2]), (tag, "bank offsets or status")
            planes = braw[0][:bsize].reshape(n_tones, cap, 32)
            for t, v in enumerate(steps):
                w_t = want[0] if v == step else TRL.range_levels(verdicts, so_a, starts, lens, bin_len, stride, cap, v, tab)[0]
                assert np.array_equal(planes[t], w_t), (tag, "bank plane", t, v, np.flatnonzero((planes[t] != w_t).any(axis=1))[:8].tolist(),
                                                        bin_len, stride, cap, steps)
                if v != step:   # (the family's own step: `got` above)
                    ctx.upload(bufs[0], np.full(sizes[0] + guard, 0x5A, dtype=np.uint8))
                    rc = src.tone_range_levels_into(bufs[3], bufs[4], nr, bin_len, stride, bufs[0], cap, bufs[1], bufs[2],
                                                    x3hip.LevelTone(v, 0, d_tab))
                    assert rc == 0 and ctx.range_levels_result() == res, (tag, "single", v)
                    assert np.array_equal(planes[t], ctx.download(bufs[0], sizes[0]).reshape(cap, 32)), (tag, "plane is not the single call", t)
        if tone and bin_len <= 0xFFFFFFFF:
            # the same bytes as a corpus: the frames cut into entries at random frame boundaries, ranges of random entries
            # with starts counted from the entry -- each against the reference on that entry alone (phase 0 at its start)
            F = len(offs)
            cuts = sorted(set([0, F] + [int(v) for v in rng.integers(0, F + 1, int(rng.integers(0, 5)))]))
            ends = offs + [stream.size]
            e_off = [ends[a] for a in cuts[:-1]]
            e_len = [ends[b] - ends[a] for a, b in zip(cuts[:-1], cuts[1:])]
            try:
                corpus = x3hip.Corpus(ctx, bad, e_off, e_len, params=p, seg_blocks=src.seg_blocks or 8, index="walk")
            except x3hip.X3Error:   # (a geometry the corpus build refuses an index for)
                return
            try:
                if corpus.entries["n_frames"].tolist() != [b - a for a, b in zip(cuts[:-1], cuts[1:])]:
                    return
                ne = len(cuts) - 1
                ent = [int(rng.integers(0, ne)) if rng.random() < 0.95 else int(rng.choice([ne, 2 ** 32 - 1])) for _ in range(nr)]
                c_starts, c_lens = [], []
                for w in range(nr):   # the stream's range moved into the entry that holds its start, or as it is
                    e = ent[w]
                    base = so[cuts[e]] if e < ne else 0
                    size = so[cuts[e + 1]] - base if e < ne else 0
                    if starts[w] >= base and starts[w] - base <= size and rng.random() < 0.7:
                        c_starts.append(starts[w] - base)
                    else:
                        c_starts.append(int(rng.integers(0, size + 1)) if rng.random() < 0.9 else starts[w])
                    c_lens.append(lens[w] if rng.random() < 0.5 else min(lens[w], max(0, size - min(c_starts[-1], size))))
                c_rows = [RL.rows_of(v, bin_len) for v in c_lens]
                if sum(c_rows) > 1 << 21:
                    return
                c_stride = 0 if rng.random() < 0.5 else max(1, max(c_rows) - int(rng.integers(0, 2)))
                c_cap = nr * c_stride or sum(c_rows)
                sizes = (32 * c_cap, 8 * (nr + 1), 4 * nr)
                cb = [ctx.alloc(v + guard) for v in sizes] + [ctx.alloc(8 * nr), ctx.alloc(4 * nr), ctx.alloc(4 * nr)]
                d.extend(cb)
                for q, v in zip(cb[:3], sizes):
                    ctx.upload(q, np.full(v + guard, 0x5A, dtype=np.uint8))
                ctx.upload(cb[3], np.array(c_starts, dtype=np.uint64))
                ctx.upload(cb[4], np.array(c_lens, dtype=np.uint32))
                ctx.upload(cb[5], np.array(ent, dtype=np.uint32))
                rc = corpus.tone_range_levels_into(cb[5], cb[3], cb[4], nr, bin_len, c_stride, cb[0], c_cap, cb[1], cb[2], level_tone)
                assert rc == 0, (tag, "corpus rc", rc, ctx.last_error())
                res = ctx.range_levels_result()
                raw = [ctx.download(q, v + guard) for q, v in zip(cb[:3], sizes)]
                for name, a, v in zip(("levels", "offsets", "status"), raw, sizes):
                    assert (a[v:] == 0x5A).all(), (tag, "corpus canary", name)
                assert res[0] == 0 and res[4] == sum(c_rows), (tag, "corpus result", res)
                st = raw[2][:sizes[2]].view(np.int32)
                got = raw[0][:sizes[0]].reshape(c_cap, 32)
                at = 0
                for w in range(nr):
                    rows_w = c_stride or c_rows[w]
                    mine = got[w * c_stride:(w + 1) * c_stride] if c_stride else got[at:at + rows_w]
                    at += c_rows[w]
                    e = ent[w]
                    if e >= ne or cuts[e + 1] == cuts[e]:
                        assert st[w] == RL.ERR_BAD_ARG, (tag, "corpus entry", w, e, int(st[w]))
                        continue
                    a, b = cuts[e], cuts[e + 1]
                    e_so = np.array([so[f] - so[a] for f in range(a, b + 1)], dtype=np.uint64)
                    w_rec, _, w_st = TRL.range_levels(verdicts[a:b], e_so, [c_starts[w]], [c_lens[w]], bin_len, c_stride, rows_w, step, tab)
                    assert st[w] == w_st[0], (tag, "corpus status", w, e, c_starts[w], c_lens[w], int(st[w]), int(w_st[0]))
                    assert np.array_equal(mine, w_rec), (tag, "corpus records", w, e, c_starts[w], c_lens[w], bin_len, c_stride, cuts)
                if bank and n_tones * c_cap <= 1 << 22:   # the corpus form of the bank: plane by plane the single corpus call's bytes
                    cres = res
                    csize = 32 * n_tones * c_cap
                    d_cb = ctx.alloc(csize + guard); d.append(d_cb)
                    ctx.upload(d_cb, np.full(csize + guard, 0x5A, dtype=np.uint8))
                    rc = corpus.tone_bank_range_levels_into(cb[5], cb[3], cb[4], nr, bin_len, c_stride, d_cb, c_cap, cb[1], cb[2], level_bank)
                    assert rc == 0 and ctx.range_levels_result() == cres, (tag, "corpus bank rc", rc, ctx.last_error())
                    craw = ctx.download(d_cb, csize + guard)
                    assert (craw[csize:] == 0x5A).all(), (tag, "corpus bank canary")
                    assert np.array_equal(ctx.download(cb[2], sizes[2]).view(np.int32), st), (tag, "corpus bank status")
                    cplanes = craw[:csize].reshape(n_tones, c_cap, 32)
                    for t, v in enumerate(steps):
                        one = got
                        if v != step:
                            ctx.upload(cb[0], np.full(sizes[0] + guard, 0x5A, dtype=np.uint8))
                            rc = corpus.tone_range_levels_into(cb[5], cb[3], cb[4], nr, bin_len, c_stride, cb[0], c_cap, cb[1], cb[2],
                                                               x3hip.LevelTone(v, 0, d_tab))
                            assert rc == 0 and ctx.range_levels_result() == cres, (tag, "corpus single", v)
                            one = ctx.download(cb[0], sizes[0]).reshape(c_cap, 32)
                        assert np.array_equal(cplanes[t], one), (tag, "corpus plane is not the single call", t, v)
            finally:
                corpus.close()
    finally:
        for q in d:
            ctx.free(q)


fams["r"] = fam_r
fams["l"] = lambda rng, tag: fam_r(rng, tag, diff=True)


def draw_fir(rng):
    """random taps and shift of an x3hip.Fir: 1 .. 8 taps, small or as large as sum |c| <= 32768 lets them be"""
    T = int(rng.integers(1, 9))
    if rng.random() < 0.5:
        taps = rng.integers(-4, 5, T)
    else:
        taps = rng.integers(-32768, 32768, T)
        taps[rng.random(T) < 0.3] = 0
        while int(np.abs(taps).sum()) > 32768:
            taps = taps // 2
    return x3hip.Fir([int(c) for c in taps], int(rng.choice([0, 0, 1, 7, 15, int(rng.integers(0, 16))])))


def fam_h(rng, tag, fir=False, tone=False, bank=False):
    """signal levels: the DIFF records and frame statuses of a random stream -- any geometry, damaged frames, a damaged or
    walk-built index or none -- against diff_levels_ref on the oracle's frame verdicts; then the same frames as a corpus of
    random entries, where no difference may cross from one entry into the next; SAMPLES against x3_levels_dev byte for byte"""
    import diff_levels_ref as DL
    import levels_ref as LR
    if fir:   # family (i): the same behind a drawn filter, against fir_levels_ref
        import fir_levels_ref as FR
        signal = draw_fir(rng)
        ref_stream = lambda fr, st, so_, bl, nb: FR.fir_levels(fr, st, so_, bl, nb, signal.taps, signal.shift)
        ref_corpus = lambda ref, bl: FR.corpus_fir_levels(ref, bl, signal.taps, signal.shift)
        same_as = x3hip.Fir([1])
    else:
        signal, same_as = "diff", "samples"
        ref_stream = lambda fr, st, so_, bl, nb: DL.signal_levels(fr, st, so_, bl, nb, DL.DIFF)
        ref_corpus = lambda ref, bl: DL.corpus_signal_levels(ref, bl, DL.DIFF)
    stream_levels = lambda src, bl, nb: src.levels(bl, nb, signal=signal)
    corpus_levels = lambda corpus, bl: corpus.levels(bl, signal=signal)
    tone_tabs = []
    if tone:   # family (o): the tone records of a drawn step and table, against tone_levels_ref
        import tone_levels_ref as TR
        step = int(rng.choice([0, 1 << 30, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) | 1]))
        tab = None if rng.random() < 0.5 else rng.integers(-32768, 32768, (1024, 2)).astype(np.int16)
        ones = np.tile(np.array([[1, 0]], dtype=np.int16), (1024, 1))

        def level_tone(t):   # an x3_level_tone of a table in device memory (freed behind the trial)
            if t is None:
                return x3hip.LevelTone(step, 0, ctx.tone_table_dev())
            tone_tabs.append(ctx.alloc(4096))
            ctx.upload(tone_tabs[-1], t)
            return x3hip.LevelTone(step, 0, tone_tabs[-1])
        ref_stream = lambda fr, st, so_, bl, nb: TR.tone_levels(fr, st, so_, bl, nb, step, tab)
        ref_corpus = lambda ref, bl: TR.corpus_tone_levels(ref, bl, step, tab)
        stream_levels = lambda src, bl, nb: x3hip._levels_np(src, "x3_tone_levels_dev", bl, nb, x3hip.TONE_DTYPE,
                                                           lambda d_lv, n_, d_st: src.tone_levels_into(bl, level_tone(tab), d_lv, n_, d_st))
        corpus_levels = lambda corpus, bl: x3hip._levels_np(corpus, "x3_corpus_tone_levels_dev", bl, None, x3hip.TONE_DTYPE,
                                                             lambda d_lv, n_, d_st: corpus.tone_levels_into(bl, level_tone(tab), d_lv, n_, d_st))
    if bank:   # family (q): the planes of a drawn tone bank and table, against tone_bank_levels_ref
        import tone_bank_levels_ref as TB
        import tone_levels_ref as TR
        n_tones = int(rng.integers(1, 9))
        steps = [int(rng.choice([0, 1 << 30, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) | 1]))
                 for _ in range(n_tones)]
        if n_tones > 1 and rng.random() < 0.3:
            steps[-1] = steps[0]   # equal steps, equal planes
        tab = None if rng.random() < 0.5 else rng.integers(-32768, 32768, (1024, 2)).astype(np.int16)

        def level_bank():   # an x3_level_tone_bank of a table in device memory (freed behind the trial); spare steps: garbage
            d_tab = ctx.tone_table_dev()
            if tab is not None:
                tone_tabs.append(ctx.alloc(4096))
                ctx.upload(tone_tabs[-1], tab)
                d_tab = tone_tabs[-1]
            return x3hip.LevelToneBank(n_tones, 0, d_tab, (C.c_uint32 * 8)(*(steps + [0xDEADBEEF] * (8 - n_tones))))
        ref_stream = lambda fr, st, so_, bl, nb: TB.tone_bank_levels(fr, st, so_, bl, nb, steps, tab)
        ref_corpus = lambda ref, bl: TB.corpus_tone_bank_levels(ref, bl, steps, tab)
        stream_levels = lambda src, bl, nb: x3hip._levels_np(
            src, "x3_tone_bank_levels_dev", bl, nb, x3hip.TONE_DTYPE,
            lambda d_lv, n_, d_st: src.tone_bank_levels_into(bl, level_bank(), d_lv, n_, d_st), planes=n_tones)
        corpus_levels = lambda corpus, bl: x3hip._levels_np(
            corpus, "x3_corpus_tone_bank_levels_dev", bl, None, x3hip.TONE_DTYPE,
            lambda d_lv, n_, d_st: corpus.tone_bank_levels_into(bl, level_bank(), d_lv, n_, d_st), planes=n_tones)
    r = rng.random()
    if r < 0.5:
        p = x3hip.Params.default()
    elif r < 0.75:
        p = x3hip.Params.make(int(rng.choice([10, 40])), int(rng.choice([100, 256, 500])))
    else:
        bl = int(rng.integers(2, 61))
        codes = (0, 1, 3) if rng.random() < 0.5 else tuple(int(c) for c in rng.integers(0, 4, size=3))
        p = x3hip.Params.make(bl, int(rng.integers(1, max(2, 30000 // bl))), codes)
        if x3hip.lib().x3_params_validate(C.byref(p)) != 0:
            return
    spf = p.block_len * p.blocks_per_frame
    n = int(rng.integers(1, (12 if rng.random() < 0.8 else 80) * min(spf, 4000) + 100))
    wav = content(rng, n)
    if rng.random() < 0.2:   # full-scale steps: differences that clamp
        k = int(rng.integers(1, 200))
        at = rng.integers(0, n, k)
        wav[at] = np.where(rng.random(k) < 0.5, -32768, 32767).astype(np.int16)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc != 0:
        return
    offs = frame_offsets(stream)
    so = [0]
    for off in offs:
        so.append(so[-1] + (int(stream[off + 4]) << 8 | int(stream[off + 5])))
    if so[-1] != n:
        return
    F = len(offs)
    bad = stream.copy()
    if rng.random() < 0.5:
        for _ in range(int(rng.integers(1, 4))):
            off = offs[int(rng.integers(0, F))]
            plen = int(stream[off + 6]) << 8 | int(stream[off + 7])
            kind = int(rng.integers(0, 3))
            if kind == 0 and plen > 2:      # payload bits, CRC refreshed (a decode error or other samples) or not
                q = off + 20 + int(rng.integers(2, plen))
                k = min(int(rng.integers(1, 12)), off + 20 + plen - q)
                bad[q:q + k] = 0 if rng.random() < 0.5 else rng.integers(0, 256, size=k, dtype=np.uint8)
                if rng.random() < 0.7:
                    refresh_crcs(bad, off)
            elif kind == 1:                 # a header byte other than the sample count and the payload length
                q = off + int(rng.choice([0, 1, 2, 3, 8, 12, 16, 17, 18, 19]))
                bad[q] ^= np.uint8(1 << int(rng.integers(0, 8)))
            else:                           # one payload bit -- the first sample's among them: the seam's head
                bad[off + 20 + int(rng.integers(0, min(plen, 4) if rng.random() < 0.5 else plen))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    verdicts = _frame_verdicts(bad, offs, p)
    statuses = [v for v, _ in verdicts]
    frames = [w if v == 0 else np.zeros(0, dtype=np.int16) for v, w in verdicts]
    bin_len = int(rng.choice([0, 1, 2, 7, p.block_len, spf, spf + 1, max(1, spf - 1), int(rng.integers(1, n + 2)), 1 << 20]))
    if bin_len == 1 and n > 200_000:
        bin_len = 3
    exact = LR.n_bins_for(n, bin_len)
    n_bins = max(1, exact + int(rng.choice([0, 0, -1, 3])))
    d = []
    try:
        d_off = ctx.alloc(8 * (F + 1)); d.append(d_off)
        ctx.upload(d_off, np.array(offs + [stream.size], dtype=np.uint64))
        sb = int(rng.choice([0, 2, 4, 32, 64]))
        index = "walk" if rng.random() < 0.5 else "decode"
        if index == "walk" and sb == 0:
            sb = 8
        if sb == 2:   # (2 blocks per entry is no multiple of four: every index call refuses it, under either family;
            sb = 8    #  the draw stays so that the trials of a seed keep their numbers)
        src = x3hip.WindowSource(ctx, bad, p, seg_blocks=sb, frame_offsets=d_off, n_frames=F, index=index)
        d.extend(src._own); src._own = []
        assert src.total == n, (tag, "total", src.total, n)
        if src.d_seg_index is not None and rng.random() < 0.3:   # a damaged index: a hint, never trusted -- seeds included
            ne = x3hip.lib().x3_seg_index_entries(F, C.byref(p), src.seg_blocks)
            idx = ctx.download(src.d_seg_index, 8 * ne, np.uint64)
            if ne > 1:
                sel = rng.random(ne) < 0.2; sel[0] = False
                how = rng.random()
                if how < 0.4:      # the sample alone
                    idx[sel] ^= (rng.integers(1, 1 << 16, int(sel.sum()), dtype=np.uint64) << np.uint64(32))
                elif how < 0.7:    # the bit offset alone
                    idx[sel] += rng.integers(1, 9, int(sel.sum()), dtype=np.uint64)
                else:
                    idx[sel] = rng.integers(0, 1 << 49, int(sel.sum()), dtype=np.uint64)
            ctx.upload(src.d_seg_index, idx)
        got, st = stream_levels(src, bin_len, n_bins)
        assert st.tolist() == statuses, (tag, "statuses", st.tolist(), statuses)
        want = ref_stream(frames, statuses, so[:-1], bin_len, n_bins)
        for k in want.dtype.names:
            assert np.array_equal(got[k], want[k]), (tag, "stream", k, bin_len, n_bins, np.flatnonzero(got[k] != want[k])[:8].tolist())
        old, _ = src.levels(bin_len, n_bins)
        if bank:   # every plane is the single call's bytes; the adapter over all planes at once on the usual table's records
            for t, step in enumerate(steps):
                one, _ = x3hip._levels_np(src, "x3_tone_levels_dev", bin_len, n_bins, x3hip.TONE_DTYPE,
                                        lambda d_lv, n_, d_st: src.tone_levels_into(
                                            bin_len, x3hip.LevelTone(step, 0, tone_tabs[-1] if tab is not None else ctx.tone_table_dev()),
                                            d_lv, n_, d_st))
                assert one.tobytes() == got[t].tobytes(), (tag, "plane is not the single call", t)
            if tab is None:
                band, _ = src.tone_bank_levels(bin_len, [x3hip.Tone(v) for v in steps], n_bins, band=True)
                assert all(band[t].tobytes() == TR.tone_power_levels(want[t]).tobytes() for t in range(n_tones)), (tag, "adapter")
        elif tone:   # a table of all (1, 0): the sums of the levels call; the adapter on the usual table's records
            same, _ = x3hip._levels_np(src, "x3_tone_levels_dev", bin_len, n_bins, x3hip.TONE_DTYPE,
                                     lambda d_lv, n_, d_st: src.tone_levels_into(bin_len, level_tone(ones), d_lv, n_, d_st))
            assert np.array_equal(same["re"], old["sum"]) and not same["im"].any(), (tag, "ones")
            assert all(np.array_equal(same[k], old[k]) for k in ("min", "max", "n")), (tag, "ones: min, max, n")
            band, _ = src.levels(bin_len, n_bins, signal=x3hip.Tone(step))
            usual = TR.tone_levels(frames, statuses, so[:-1], bin_len, n_bins, step)
            assert band.tobytes() == TR.tone_power_levels(usual).tobytes(), (tag, "adapter")
        else:
            same, _ = src.levels(bin_len, n_bins, signal=same_as)
            assert same.tobytes() == old.tobytes(), (tag, "samples")
        # the same bytes as a corpus: the frames cut into entries at random frame boundaries
        if F >= 1 and bin_len <= 0xFFFFFFFF:
            cuts = sorted(set([0, F] + [int(v) for v in rng.integers(0, F + 1, int(rng.integers(0, 5)))]))
            ends = offs + [stream.size]
            e_off = [ends[a] for a in cuts[:-1]]
            e_len = [ends[b] - ends[a] for a, b in zip(cuts[:-1], cuts[1:])]
            try:
                corpus = x3hip.Corpus(ctx, bad, e_off, e_len, params=p, seg_blocks=src.seg_blocks or 8, index="walk")
            except x3hip.X3Error:   # (a geometry the corpus build refuses an index for)
                return
            try:
                if corpus.entries["n_frames"].tolist() == [b - a for a, b in zip(cuts[:-1], cuts[1:])]:
                    rows, rf, cst = corpus_levels(corpus, bin_len)
                    ref = []
                    for a, b in zip(cuts[:-1], cuts[1:]):
                        ref.append((frames[a:b], statuses[a:b], [so[f] - so[a] for f in range(a, b)], so[b] - so[a]))
                    wrows, wrf = ref_corpus(ref, bin_len)
                    assert np.array_equal(rf, wrf) and cst.tolist() == statuses, (tag, "corpus layout")
                    for k in wrows.dtype.names:
                        assert np.array_equal(rows[k], wrows[k]), (tag, "corpus", k, bin_len, cuts, np.flatnonzero(rows[k] != wrows[k])[:8].tolist())
            finally:
                corpus.close()
    finally:
        for q in d + tone_tabs:
            ctx.free(q)


fams["h"] = fam_h
fams["o"] = lambda rng, tag: fam_h(rng, tag, tone=True)
fams["i"] = lambda rng, tag: fam_h(rng, tag, fir=True)
fams["t"] = lambda rng, tag: fam_r(rng, tag, fir=draw_fir(rng))
fams["p"] = lambda rng, tag: fam_r(rng, tag, tone=True)
fams["q"] = lambda rng, tag: fam_h(rng, tag, bank=True)
fams["u"] = lambda rng, tag: fam_r(rng, tag, tone=True, bank=True)


def _plane_events_check(rng, tag, what, planes, bin_len, corpus, d_total, n_samples, total):
    """one drawn plane events call on the K planes `planes` (np, LEVEL_DTYPE [K, rows]) against plane_events_ref: a drawn
    rule whose values are keys of the planes' own records, min_planes, a plane stride with loud records in the slack, d_thr
    per (plane, entry) or none, a drawn cap, outputs left out now and then; every slot of every output with =="""
    import levels_ref as LR
    import plane_events_ref as PE
    K, n_rows = planes.shape
    n_ent = len(n_samples) if corpus is not None else 1
    join = int(rng.choice([0, 1, 2, 5, 40]))
    mb = int(rng.choice([0, 0, 1, 3, 64, 200]))
    if mb * bin_len > 0xFFFFFFFF:
        mb = 0
    use_thr = rng.random() < 0.4

    def values(t):   # the two values of plane t: keys of its own counting records, so that some rows are loud; or off
        rec = planes[t][planes[t]["n"] != 0]
        if rec.size == 0 or rng.random() < 0.1:
            return 0, 0
        r = rec[int(rng.integers(0, rec.size))]
        m = min(max(int(r["sum_sq"]) // int(r["n"]), 1), 1 << 30)
        p = min(max(int(r["max"]), -int(r["min"]), 1), 32768)
        c = int(rng.integers(0, 3))
        return (m if c != 0 else 0), (p if c != 1 else 0)
    vals = [values(t) for t in range(K)]
    on = sum(1 for m, p in vals if m or p)
    if on == 0:
        vals[0], on = (1, 0), 1
    mp = int(rng.integers(1, K + 1))
    thr = None
    if use_thr:   # per (plane, entry): the plane's values, or off, or above a limit; counted is garbage
        def one(t):
            m, p = vals[t]
            how = rng.random()
            return ((m, p) if how < 0.7 else (0, 0) if how < 0.8 else ((1 << 30) + 1, p) if how < 0.9 else (m, 32769)) + \
                (int(rng.integers(0, 1 << 32)),)
        thr = [[one(t) for _ in range(n_ent)] for t in range(K)]
        vals = [(0, 0)] * K
    else:
        mp = min(mp, on)
    rule = PE.PlaneRule([m for m, _ in vals], [p for _, p in vals], mp, join, int(rng.choice([0, 1, 2, 9])),
                        int(rng.integers(0, join // 2 + 1)), mb)
    if corpus is None:
        ev, elv = PE.stream_plane_events(planes, total, bin_len, rule, None if thr is None else [t[0] for t in thr])
    else:
        ev, elv = PE.corpus_plane_events(planes, n_samples, bin_len, rule, thr)
    cap = int(rng.choice([1, 3, max(len(ev), 1), len(ev) + 2]))
    went, wst, wln, wmk, wlv = PE.slots(ev, elv, cap, corpus is not None)
    stride = n_rows + int(rng.choice([0, 0, 5]))
    up = np.stack([LR.empty(stride) for _ in range(K)])
    up["n"], up["max"], up["sum_sq"] = 1, 32767, 1 << 30                # (the slack: loud under every rule, never read)
    up[:, :n_rows] = planes
    r = x3hip.PlaneEventRule.make(list(rule.mean_sq_min), list(rule.peak_min), mp, join, rule.min_bins, rule.pad_bins, mb)
    for t in range(K, 8):                                               # garbage behind n_planes
        r.mean_sq_min[t], r.peak_min[t] = int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 32))
    with_mask, with_levels = rng.random() < 0.85, rng.random() < 0.85
    sizes = [4 * cap, 8 * cap, 4 * cap, 4 * cap, 32 * K * cap, 8]
    held = (K - 1) * stride + n_rows   # (the header's minimum: plane t is the n_rows records at t * stride, no slack behind the last)
    d = [ctx.alloc(32 * held)] + [ctx.alloc(s) for s in sizes] + [ctx.alloc(16 * K * n_ent)]
    try:
        d_lv, d_ent, d_st, d_ln, d_mk, d_el, d_cnt, d_thr = d
        ctx.upload(d_lv, up.reshape(-1)[:held])
        for q, s in zip(d[1:7], sizes):
            ctx.upload(q, np.full(s, 0xA5, dtype=np.uint8))
        if thr is not None:
            a = np.zeros(K * n_ent, dtype=x3hip.EVENT_THRESHOLD_DTYPE)
            a[:] = [v for t in thr for v in t]
            ctx.upload(d_thr, a)
        args = (r, d_thr if thr is not None else None)
        outs = (d_st, d_ln, d_mk if with_mask else None, d_el if with_levels else None, cap, d_cnt)
        if corpus is None:
            rc = ctx.plane_events_dev(d_lv, stride, n_rows, bin_len, d_total, *args, *outs)
        else:
            rc = corpus.plane_events_into(d_lv, stride, n_rows, bin_len, *args, d_ent, *outs)
        assert rc == 0, (tag, what, "rc", rc, ctx.last_error())
        assert ctx.events_result() == (0, len(ev)), (tag, what, "count", len(ev))
        got = [ctx.download(q, s) for q, s in zip(d[1:7], sizes)]
        assert int(got[5].view(np.uint64)[0]) == len(ev), (tag, what, "d_count")
        if corpus is not None:
            assert np.array_equal(got[0].view(np.uint32), went), (tag, what, "entries")
        else:
            assert (got[0] == 0xA5).all(), (tag, what, "a stream call wrote entries")
        assert np.array_equal(got[1].view(np.uint64), wst), (tag, what, "starts", rule, got[1].view(np.uint64)[:6], wst[:6])
        assert np.array_equal(got[2].view(np.uint32), wln), (tag, what, "lens", rule)
        if with_mask:
            assert np.array_equal(got[3].view(np.uint32), wmk), (tag, what, "masks", rule, got[3].view(np.uint32)[:6], wmk[:6])
        else:
            assert (got[3] == 0xA5).all(), (tag, what, "a NULL mask array was written")
        if with_levels:
            assert got[4].tobytes() == wlv.tobytes(), (tag, what, "event levels", rule)
        else:
            assert (got[4] == 0xA5).all(), (tag, what, "a NULL event levels array was written")
    finally:
        for q in d:
            ctx.free(q)
    return rule, thr, ev, elv


def fam_v(rng, tag):
    """plane events: the band planes of a drawn tone bank over a random stream -- any geometry, damaged frames, whose bins
    count nothing and are never loud -- held against tone_bank_levels_ref, then x3_plane_events_dev on them with a drawn K,
    min_planes, per-plane values, plane stride, rule and d_thr or none, GPU == tests/plane_events_ref.py in every slot; the
    chain bank levels -> plane events with no host trip (bank_events) on the same rule; then the same frames as a corpus of
    random entries (x3_corpus_plane_events_dev, thresholds per plane and entry)"""
    import levels_ref as LR
    import plane_events_ref as PE
    import tone_bank_levels_ref as TB
    import tone_levels_ref as TR
    p = x3hip.Params.default() if rng.random() < 0.6 else x3hip.Params.make(int(rng.choice([10, 20, 40])), int(rng.choice([25, 100, 256])))
    spf = p.block_len * p.blocks_per_frame
    n = int(rng.integers(1, 12 * min(spf, 4000) + 100))
    wav = content(rng, n)
    rc, stream, _ = O.encode(wav, oparams(p))
    if rc != 0:
        return
    offs = frame_offsets(stream)
    so = [0]
    for off in offs:
        so.append(so[-1] + (int(stream[off + 4]) << 8 | int(stream[off + 5])))
    if so[-1] != n:
        return
    F = len(offs)
    bad = stream.copy()
    if rng.random() < 0.6:
        for _ in range(int(rng.integers(1, 4))):
            off = offs[int(rng.integers(0, F))]
            plen = int(stream[off + 6]) << 8 | int(stream[off + 7])
            if rng.random() < 0.5 and plen > 2:   # payload bits, CRC refreshed (a decode error or other samples) or not
                q = off + 20 + int(rng.integers(2, plen))
                k = min(int(rng.integers(1, 12)), off + 20 + plen - q)
                bad[q:q + k] = rng.integers(0, 256, size=k, dtype=np.uint8)
                if rng.random() < 0.7:
                    refresh_crcs(bad, off)
            else:                                 # a header byte other than the sample count and the payload length
                bad[off + int(rng.choice([0, 1, 2, 3, 8, 12, 16, 17, 18, 19]))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    verdicts = _frame_verdicts(bad, offs, p)
    statuses = [v for v, _ in verdicts]
    frames = [w if v == 0 else np.zeros(0, dtype=np.int16) for v, w in verdicts]
    bin_len = int(rng.choice([7, p.block_len, spf, spf + 1, max(1, n // int(rng.integers(1, 400)))]))
    bin_len = max(bin_len, -(-n // 4000))          # (the reference walks every row of every plane in Python)
    n_bins = max(1, LR.n_bins_for(n, bin_len) + int(rng.choice([0, 0, -1, 3])))
    K = int(rng.integers(1, 9))
    steps = [int(rng.choice([0, 1 << 30, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)) | 1])) for _ in range(K)]
    if K > 1 and rng.random() < 0.3:
        steps[-1] = steps[0]                       # equal steps, equal planes
    tones = [x3hip.Tone(s) for s in steps]
    d = []
    try:
        d_off = ctx.alloc(8 * (F + 1)); d.append(d_off)
        ctx.upload(d_off, np.array(offs + [stream.size], dtype=np.uint64))
        src = x3hip.WindowSource(ctx, bad, p, seg_blocks=int(rng.choice([0, 8, 32])), frame_offsets=d_off, n_frames=F)
        d.extend(src._own); src._own = []
        planes, st = src.tone_bank_levels(bin_len, tones, n_bins, band=True)
        assert st.tolist() == statuses, (tag, "statuses")
        want = TB.tone_bank_levels(frames, statuses, so[:-1], bin_len, n_bins, steps)
        assert all(planes[t].tobytes() == TR.tone_power_levels(want[t]).tobytes() for t in range(K)), (tag, "band planes")
        rule, thr, ev, elv = _plane_events_check(rng, tag, "stream", planes, bin_len, None, src.d_sample_offsets + 8 * F, None, n)
        if thr is None and n_bins == LR.n_bins_for(n, bin_len):   # the chain with no host trip, on the source's own bins
            cap = len(ev) + 1
            r = x3hip.PlaneEventRule.make(list(rule.mean_sq_min), list(rule.peak_min), rule.min_planes, rule.join_bins,
                                          rule.min_bins, rule.pad_bins, rule.max_bins)
            t_st, t_ln, t_cnt, t_mk, t_el = src.bank_events(bin_len, tones, r, cap)
            _, wst, wln, wmk, wlv = PE.slots(ev, elv, cap, False)
            assert int(t_cnt) == len(ev) and np.array_equal(t_st.cpu().numpy().view(np.uint64), wst), (tag, "bank_events starts")
            assert np.array_equal(t_ln.cpu().numpy().view(np.uint32), wln) and np.array_equal(t_mk.cpu().numpy().view(np.uint32), wmk), \
                (tag, "bank_events lens, masks")
            assert t_el.cpu().numpy().tobytes() == wlv.tobytes(), (tag, "bank_events levels")
        # the same bytes as a corpus: the frames cut into entries at random frame boundaries
        cuts = sorted(set([0, F] + [int(v) for v in rng.integers(0, F + 1, int(rng.integers(0, 5)))]))
        ends = offs + [stream.size]
        try:
            corpus = x3hip.Corpus(ctx, bad, [ends[a] for a in cuts[:-1]], [ends[b] - ends[a] for a, b in zip(cuts[:-1], cuts[1:])],
                                  params=p, seg_blocks=8, index="walk")
        except x3hip.X3Error:   # (a geometry the corpus build refuses an index for)
            return
        try:
            if corpus.entries["n_frames"].tolist() == [b - a for a, b in zip(cuts[:-1], cuts[1:])]:
                rows, rf, cst = corpus.tone_bank_levels(bin_len, tones, band=True)
                ref = [(frames[a:b], statuses[a:b], [so[f] - so[a] for f in range(a, b)], so[b] - so[a])
                       for a, b in zip(cuts[:-1], cuts[1:])]
                wrows, wrf = TB.corpus_tone_bank_levels(ref, bin_len, steps)
                assert np.array_equal(rf, wrf) and cst.tolist() == statuses, (tag, "corpus layout")
                assert all(rows[t].tobytes() == TR.tone_power_levels(wrows[t]).tobytes() for t in range(K)), (tag, "corpus band planes")
                _plane_events_check(rng, tag, "corpus", rows, bin_len, corpus, None, [e[3] for e in ref], None)
        finally:
            corpus.close()
    finally:
        for q in d:
            ctx.free(q)


fams["v"] = fam_v


def fam_y(rng, tag):
    """spectra (x3_spectra_rows_dev): rows of drawn samples in HBM at drawn (odd and even) offsets -- lengths round n_fft and
    round whole frames, zero lengths, wild offsets -- x n_fft x hop x format x layout x row and sample capacities x the usual
    table, ones or a random one x in-statuses (none, separate, in place); every word the call may write GPU ==
    tests/spectra_ref.py, what it may not write keeps its fill; the result call.  (The letter (w) is the WAV files'.)"""
    import spectra_ref as SP
    n_fft = int(rng.choice(SP.NFFTS))
    hop = int(rng.choice([1, 3, 48, n_fft // 2, n_fft, n_fft + 5, int(rng.integers(1, 3 * n_fft))]))
    fmt = int(rng.integers(0, 2))
    n = int(rng.integers(1, 12))
    max_rows = int(rng.choice([1, 3, 20]))
    lens, offsets, at = [], [], int(rng.integers(0, 4))
    for _ in range(n):
        r = int(rng.integers(0, max_rows + 1))
        ln = int(rng.choice([0, n_fft - 1, int(rng.integers(0, n_fft))])) if r == 0 else n_fft + (r - 1) * hop + int(rng.choice([0, hop - 1, int(rng.integers(0, hop))]))
        ln = min(ln, 60_000)
        offsets.append(at)
        lens.append(ln)
        at += int(rng.choice([ln, ln + 1, ln // 2]))     # (rows may overlap: they are only read)
    cap_s = max(o + l for o, l in zip(offsets, lens)) + int(rng.integers(0, 3))
    x = rng.integers(-32768, 32768, max(cap_s, 1)).astype(np.int16)
    if rng.random() < 0.3:
        x[:] = rng.choice(np.array([-32768, 32767, -129, -128, -1, 0, 127, 128, 255, 256], dtype=np.int16), x.size)
    if rng.random() < 0.3:
        cap_s = max(cap_s - int(rng.integers(1, n_fft)), 0)            # the last rows end behind samples_cap
    if rng.random() < 0.2:
        offsets[int(rng.integers(0, n))] = [1 << 63, (1 << 64) - 1, cap_s + 1][int(rng.integers(0, 3))]
    rows = [SP.n_rows(v, n_fft, hop) for v in lens]
    if rng.random() < 0.5:
        stride = max(1, max(rows) + int(rng.choice([0, 0, 1, -1])))
        rows_cap = n * stride + int(rng.integers(0, 3))
    else:
        stride = 0
        rows_cap = max(1, sum(rows) + int(rng.choice([0, 0, 2, -1, -sum(rows) // 2])))
    kind = int(rng.integers(0, 3))
    tab = None if kind == 0 else rng.integers(-32768, 32768, (SP.PAIRS, 2)).astype(np.int16)
    if kind == 2:
        tab[:] = (1, 0)
    mode = int(rng.integers(0, 3))                                       # no in-status, a separate array, in place
    ins = None if mode == 0 else [int(rng.choice([0, 0, 0, 14, 21, 24])) for _ in range(n)]
    null_off = bool(stride) and rng.random() < 0.3
    row_bytes = SP.n_bins(n_fft) * (16 if fmt == SP.SUMS else 4)
    sizes = (row_bytes * rows_cap, 8 * (n + 1), 4 * n)
    d = [ctx.alloc(v) for v in sizes] + [ctx.alloc(max(2 * x.size, 2)), ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(4 * SP.PAIRS)]
    d_out, d_ro, d_st, d_x, d_off, d_len, d_in, d_tab = d
    try:
        for q, v in zip(d[:3], sizes):
            ctx.upload(q, np.full(v, 0x5A, dtype=np.uint8))
        ctx.upload(d_x, x)
        ctx.upload(d_off, np.array(offsets, dtype=np.uint64))
        ctx.upload(d_len, np.array(lens, dtype=np.uint32))
        ctx.upload(d_tab, SP.table() if tab is None else tab)
        if ins is not None:
            ctx.upload(d_st if mode == 2 else d_in, np.array(ins, dtype=np.int32))
        rule = x3hip.SpectraRule(n_fft, hop, fmt, 0, d_tab)
        rc = ctx.spectra_rows_dev(d_x, cap_s, d_off, d_len, None if ins is None else (d_st if mode == 2 else d_in), n, rule, stride,
                                  d_out, rows_cap, None if null_off else d_ro, d_st)
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        assert rc == 0, (tag, rc, ctx.last_error())
        res = ctx.spectra_result()
        want = SP.spectra_rows(x[:cap_s], offsets, lens, ins, n_fft, hop, fmt, stride, rows_cap, tab)
        got = ctx.download(d_out, sizes[0])
        assert got.tobytes() == want[0].tobytes(), (tag, "rows", n_fft, hop, fmt, stride, rows_cap)
        off = ctx.download(d_ro, sizes[1], np.uint64)
        assert (off.view(np.uint8) == 0x5A).all() if null_off else np.array_equal(off, want[1]), (tag, "row offsets")
        st = ctx.download(d_st, sizes[2], np.int32)
        assert np.array_equal(st, want[2]), (tag, "statuses", st, want[2])
        bad = np.flatnonzero(st)
        assert res == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0, want[3]), (tag, res)
    finally:
        for q in d:
            ctx.free(q)


fams["y"] = fam_y


def fam_z(rng, tag):
    """band levels (x3_spectra_levels_dev): fam_y's rows -- lengths round n_fft, round whole frames and round whole time bins
    -- x n_fft x hop x frames_per_bin x n_bands x band maps with wild words and empty bands x layout x row capacities x plane
    strides x tables x in-statuses (none, separate, in place); every record of every plane GPU == tests/spectra_levels_ref.py,
    what the call may not write -- the records between rows_cap and plane_stride among them -- keeps its fill; the result call"""
    import spectra_levels_ref as SL
    import spectra_ref as SP
    n_fft = int(rng.choice(SP.NFFTS))
    nb = SP.n_bins(n_fft)
    hop = int(rng.choice([1, 3, 48, n_fft // 2, n_fft, n_fft + 5, int(rng.integers(1, 3 * n_fft))]))
    per_bin = int(rng.choice([1, 2, 3, 7, 16, 33, int(rng.integers(1, 50)), 0x7FFFFFFF]))
    n = int(rng.integers(1, 12))
    max_rows = int(rng.choice([1, 3, 20, 70]))
    lens, offsets, at = [], [], int(rng.integers(0, 4))
    for _ in range(n):
        r = int(rng.integers(0, max_rows + 1))
        if r and per_bin < 100 and rng.random() < 0.5:                      # a frame round a whole number of time bins
            r = max(1, (r // per_bin) * per_bin + int(rng.integers(-1, 2)))
        ln = int(rng.choice([0, n_fft - 1, int(rng.integers(0, n_fft))])) if r == 0 else n_fft + (r - 1) * hop + int(rng.choice([0, hop - 1, int(rng.integers(0, hop))]))
        ln = min(ln, 60_000)
        offsets.append(at)
        lens.append(ln)
        at += int(rng.choice([ln, ln + 1, ln // 2]))     # (rows may overlap: they are only read)
    cap_s = max(o + l for o, l in zip(offsets, lens)) + int(rng.integers(0, 3))
    x = rng.integers(-32768, 32768, max(cap_s, 1)).astype(np.int16)
    if rng.random() < 0.3:
        x[:] = rng.choice(np.array([-32768, 32767, -129, -128, -1, 0, 127, 128, 255, 256], dtype=np.int16), x.size)
    if rng.random() < 0.3:
        cap_s = max(cap_s - int(rng.integers(1, n_fft)), 0)            # the last rows end behind samples_cap
    if rng.random() < 0.2:
        offsets[int(rng.integers(0, n))] = [1 << 63, (1 << 64) - 1, cap_s + 1][int(rng.integers(0, 3))]
    bins = [SL.n_bins_of(SP.n_rows(v, n_fft, hop), per_bin) for v in lens]
    if rng.random() < 0.5:
        stride = max(1, max(bins) + int(rng.choice([0, 0, 1, -1])))
        rows_cap = n * stride + int(rng.integers(0, 3))
    else:
        stride = 0
        rows_cap = max(1, sum(bins) + int(rng.choice([0, 0, 2, -1, -sum(bins) // 2])))
    n_bands = int(rng.choice([1, 2, 8, nb, int(rng.integers(1, nb + 1))]))
    bin_band = rng.integers(0, n_bands + int(rng.integers(0, 3)), nb).astype(np.uint32)     # (words of K, K + 1: no band)
    wild = rng.random(nb) < 0.1
    bin_band[wild] = rng.choice(np.array([n_bands, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], dtype=np.uint32), int(wild.sum()))
    if rng.random() < 0.2:
        bin_band[:] = int(rng.integers(0, n_bands))                        # every bin in one band, the others empty
    plane_stride = int(rng.choice([0, rows_cap, rows_cap + 1, rows_cap + int(rng.integers(0, 40))]))
    ps = plane_stride or rows_cap
    kind = int(rng.integers(0, 3))
    tab = None if kind == 0 else rng.integers(-32768, 32768, (SP.PAIRS, 2)).astype(np.int16)
    if kind == 2:
        tab[:] = (32767, 0)                                                # every bin of a loud frame at its clamp
    mode = int(rng.integers(0, 3))                                       # no in-status, a separate array, in place
    ins = None if mode == 0 else [int(rng.choice([0, 0, 0, 14, 21, 24])) for _ in range(n)]
    null_off = bool(stride) and rng.random() < 0.3
    sizes = (32 * ((n_bands - 1) * ps + rows_cap), 8 * (n + 1), 4 * n)    # (the last plane ends at its rows_cap)
    d = [ctx.alloc(v) for v in sizes] + [ctx.alloc(max(2 * x.size, 2)), ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n),
                                         ctx.alloc(4 * SP.PAIRS), ctx.alloc(4 * nb)]
    d_out, d_ro, d_st, d_x, d_off, d_len, d_in, d_tab, d_map = d
    try:
        for q, v in zip(d[:3], sizes):
            ctx.upload(q, np.full(v, 0x5A, dtype=np.uint8))
        ctx.upload(d_x, x)
        ctx.upload(d_off, np.array(offsets, dtype=np.uint64))
        ctx.upload(d_len, np.array(lens, dtype=np.uint32))
        ctx.upload(d_tab, SP.table() if tab is None else tab)
        ctx.upload(d_map, bin_band)
        if ins is not None:
            ctx.upload(d_st if mode == 2 else d_in, np.array(ins, dtype=np.int32))
        rule = x3hip.SpectraRule(n_fft, hop, SP.POWER, 0, d_tab)
        fold = x3hip.SpectraFold(per_bin, n_bands, plane_stride, d_map, 0)
        rc = ctx.spectra_levels_dev(d_x, cap_s, d_off, d_len, None if ins is None else (d_st if mode == 2 else d_in), n, rule, fold,
                                    stride, d_out, rows_cap, None if null_off else d_ro, d_st)
        C.memset(C.byref(rule), 0xEE, C.sizeof(rule))
        C.memset(C.byref(fold), 0xEE, C.sizeof(fold))
        assert rc == 0, (tag, rc, ctx.last_error())
        res = ctx.spectra_result()
        want = SL.spectra_levels(x[:cap_s], offsets, lens, ins, n_fft, hop, per_bin, bin_band, n_bands, stride, rows_cap, plane_stride, tab)
        got = ctx.download(d_out, sizes[0])
        assert got.tobytes() == want[0].tobytes()[:sizes[0]], (tag, "records", n_fft, hop, per_bin, n_bands, stride, rows_cap, plane_stride)
        off = ctx.download(d_ro, sizes[1], np.uint64)
        assert (off.view(np.uint8) == 0x5A).all() if null_off else np.array_equal(off, want[1]), (tag, "row offsets")
        st = ctx.download(d_st, sizes[2], np.int32)
        assert np.array_equal(st, want[2]), (tag, "statuses", st, want[2])
        bad = np.flatnonzero(st)
        assert res == (0, bad.size, int(bad[0]) if bad.size else n, int(st[bad[0]]) if bad.size else 0, want[3]), (tag, res)
    finally:
        for q in d:
            ctx.free(q)


fams["z"] = fam_z


def run(seed=1, minutes=None, trials=None, families="egdbaf", only=-1, context=None):
    """draw and check cases until the time or the trial budget is used up -> {family: trials}"""
    global ctx
    own = context is None
    ctx = context if context is not None else x3hip.Context(0)
    t_end = time.time() + 60 * minutes if minutes is not None else None
    trace = open(os.environ["X3_FUZZ_TRACE"], "w") if os.environ.get("X3_FUZZ_TRACE") else None
    if os.environ.get("X3_FUZZ_TRACE_CALLS"):   # every Context call of the trial(s), appended before it is made
        calls = open(os.environ["X3_FUZZ_TRACE_CALLS"], "a")

        def brief(v):
            if isinstance(v, np.ndarray):
                return "ndarray(%s,%d)" % (v.dtype, v.size)
            if isinstance(v, (list, tuple)) and len(v) > 8:
                return "%s[%d]" % (type(v).__name__, len(v))
            if isinstance(v, int) and v > 1 << 32:
                return hex(v)
            return repr(v)[:80]

        def wrap(name, fn):
            def g(*a, **k):
                calls.write("%s(%s)\n" % (name, ", ".join([brief(v) for v in a] + ["%s=%s" % (q, brief(v)) for q, v in k.items()])))
                calls.flush()
                r = fn(*a, **k)
                if name == "alloc":
                    calls.write("  -> %s\n" % brief(r)); calls.flush()
                return r
            return g
        for name in dir(ctx):
            if not name.startswith("_") and callable(getattr(ctx, name)):
                setattr(ctx, name, wrap(name, getattr(ctx, name)))
    trial = START_TRIAL
    counts = {k: 0 for k in fams}
    try:
        while (t_end is None or time.time() < t_end) and (trials is None or trial < trials):
            if only >= 0:
                trial = only
            rng = np.random.default_rng([seed, trial])
            k = families[int(rng.integers(0, len(families)))]
            if trace is not None:     # (a trial that kills the process -- a GPU memory fault -- leaves its number here)
                trace.seek(0); trace.write("%d %d %s\n" % (seed, trial, k)); trace.flush()
            try:
                fams[k](rng, (seed, trial))
            except Exception:
                print("FAILED: seed %d trial %d family %s" % (seed, trial, k), flush=True)
                raise
            counts[k] += 1
            trial += 1
            if only >= 0:
                break
    finally:
        if own:
            ctx.close()
        else:  # a borrowed context goes back with the options the families touch at their defaults
            for name, value in (("reader_window_frames", 4096), ("enc_gen", 3), ("host_walk", -1), ("host_chunk_frames", 0), ("index_no_fast", 0),
                                ("file_chunk_frames", 800), ("file_workers", 4), ("seg_stretches", 0)):
                ctx.set_option(name, value)
        ctx = None
    return counts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--families", default="egdbaf")
    ap.add_argument("--start", type=int, default=0, help="begin the sequence of trials at this trial number (a fresh context)")
    ap.add_argument("--out", default=None, help="also write the trial counts here (JSON)")
    a = ap.parse_args()
    START_TRIAL = a.start
    c = run(a.seed, a.minutes, None, a.families, a.only)
    print("fuzz_parity: seed %d, %d trials OK in %.1f min %s" % (a.seed, sum(c.values()), a.minutes, c), flush=True)
    if a.out:
        import json
        with open(a.out, "w") as fh:
            json.dump({"seed": a.seed, "minutes": a.minutes, "families": a.families, "trials": c}, fh)
