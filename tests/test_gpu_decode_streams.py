"""Batches of streams (include/x3hip.h, "BATCHES OF STREAMS"): x3_decode_streams_dev / x3_decode_streams_result,
x3hip.decode_archives and the C++ mirror.  Every row and every x3_stream_result is held against the oracle's decode_stream
(or x3a_decode for archive entries) of that entry alone with wav_cap = row_len, and against the library's own single-entry
call as a second witness; the bytes around d_out and d_results are canaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 24
PAD = 256          # canary bytes on either side of d_out and d_results
CANARY = 0xA5
RES_BYTES = 24


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _f32(a):
    return (np.asarray(a, dtype=np.int16).astype(np.float32) / np.float32(32768.0)).view(np.uint32)


def _frames(stream):
    offs = [0]
    while offs[-1] + 8 <= stream.size:
        nxt = offs[-1] + 20 + ((int(stream[offs[-1] + 6]) << 8) | int(stream[offs[-1] + 7]))
        if nxt > stream.size:
            break
        offs.append(nxt)
    return offs


def _encode(ctx, wav, p=None):
    rc, s, _ = ctx.encode(wav, p)
    assert rc == 0
    return s


def _place(entries, mode, rng):
    """one buffer holding every entry: back to back at even offsets, at odd ones, with gaps, overlapping, repeated"""
    blob, offs = bytearray(), []
    for i, e in enumerate(entries):
        if mode == "even" and len(blob) & 1:
            blob += b"\0"
        elif mode == "odd" and not len(blob) & 1:
            blob += b"\x78"            # (half a key in front of the entry)
        elif mode == "gaps":
            blob += bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
        offs.append(len(blob))
        blob += bytes(e)
    lens = [len(e) for e in entries]
    if mode == "overlap":   # every entry again, and each one's second half as an entry of its own
        offs2, lens2 = list(offs), list(lens)
        for o, n in zip(offs, lens):
            offs2 += [o, o + n // 2]
            lens2 += [n, n - n // 2]
        offs, lens = offs2, lens2
    return np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), offs, lens


def _expect(buf, offs, lens, row_len, p, archive=False, headers=None):
    out = []
    for i, (o, n) in enumerate(zip(offs, lens)):
        entry = buf[o:o + n]
        if archive:
            rc, w, _rate, fok, ferr = O.x3a_decode(np.concatenate([headers[i], entry]), wav_cap=row_len)
        else:
            rc, w, fok, ferr = O.decode_stream(entry, p, wav_cap=row_len)
        out.append((rc, w, fok, ferr))
    return out


class Batch:
    """x3_decode_streams_dev on one host buffer, with canaries around the outputs"""

    def __init__(self, ctx, buf):
        self.ctx = ctx
        self.x3_len = buf.size - 16
        self.d_x3 = ctx.alloc(buf.size)
        ctx.upload(self.d_x3, buf)

    def run(self, offs, lens, row_len, fmt=0, p=None, flags=0, expect_rc=0):
        import x3hip
        n = len(offs)
        esz = 4 if fmt else 2
        nbytes = esz * n * row_len
        d_out = self.ctx.alloc(nbytes + 2 * PAD)
        d_res = self.ctx.alloc(RES_BYTES * n + 2 * PAD)
        try:
            self.ctx.upload(d_out, np.full(nbytes + 2 * PAD, CANARY, dtype=np.uint8))
            self.ctx.upload(d_res, np.full(RES_BYTES * n + 2 * PAD, CANARY, dtype=np.uint8))
            rc = self.ctx.decode_streams_dev(self.d_x3, self.x3_len, offs, lens, p or x3hip.Params.default(), d_out + PAD,
                                             row_len, fmt, d_res + PAD, flags)
            assert rc == expect_rc, (rc, self.ctx.last_error())
            if rc:
                summary = None
            else:
                summary = self.ctx.decode_streams_result()
                assert summary[0] == 0, self.ctx.last_error()
            raw = self.ctx.download(d_out, nbytes + 2 * PAD)
            rres = self.ctx.download(d_res, RES_BYTES * n + 2 * PAD)
            assert (raw[:PAD] == CANARY).all() and (raw[PAD + nbytes:] == CANARY).all(), "d_out written outside its rows"
            assert (rres[:PAD] == CANARY).all() and (rres[PAD + RES_BYTES * n:] == CANARY).all(), "d_results overrun"
            if rc:
                assert (raw == CANARY).all() and (rres == CANARY).all(), "a refused call wrote something"
                return None
            rows = raw[PAD:PAD + nbytes].view(np.float32 if fmt else np.int16).reshape(n, row_len)
            res = rres[PAD:PAD + RES_BYTES * n].view(x3hip.STREAM_RESULT_DTYPE)
            return rows, res, summary
        finally:
            self.ctx.free(d_out)
            self.ctx.free(d_res)

    def close(self):
        self.ctx.free(self.d_x3)


def _check(got, want, row_len, fmt):
    rows, res, (rc, n_bad, first_bad, first_status) = got
    bad = [i for i, w in enumerate(want) if w[0] != 0]
    assert (n_bad, first_bad) == (len(bad), bad[0] if bad else len(want))
    if bad:
        assert first_status == want[bad[0]][0]
    for i, (wrc, w, fok, ferr) in enumerate(want):
        r = res[i]
        assert (int(r["status"]), int(r["n_out"]), int(r["frames_ok"]), int(r["frame_errors"])) == (wrc, w.size, fok, ferr), i
        full = np.zeros(row_len, dtype=np.int16)
        full[:w.size] = w
        if fmt:
            assert np.array_equal(rows[i].view(np.uint32), _f32(full)), i
        else:
            assert np.array_equal(rows[i], full), i


def _clips(x3, lengths, seed=1):
    return [x3.synth(2 + (i % 3), seed * 1000 + i, 0, n) for i, n in enumerate(lengths)]


RAGGED = [0, 1, 9_999, 10_000, 10_001, 20_000, 33_333, 250_000]


@pytest.mark.parametrize("mode", ["even", "odd", "gaps", "overlap"])
def test_ragged_batches_both_formats(ctx, x3, mode):
    rng = np.random.default_rng({"even": 1, "odd": 2, "gaps": 3, "overlap": 4}[mode])
    entries = [_encode(ctx, w) if w.size else np.zeros(0, dtype=np.uint8) for w in _clips(x3, RAGGED)]
    buf, offs, lens = _place(entries, mode, rng)
    b = Batch(ctx, buf)
    try:
        for row_len in (250_000, 250_004):
            want = _expect(buf, offs, lens, row_len, None)
            for fmt in (0, 1):
                _check(b.run(offs, lens, row_len, fmt), want, row_len, fmt)
        assert ctx.get_option("last_streams_general_walks") == 0 or mode in ("odd", "gaps", "overlap")
    finally:
        b.close()


def test_clean_batch_takes_the_fast_walk_and_matches_the_single_call(ctx, x3):
    """an encoder's clips back to back: no entry needs the general walk, and every row equals x3_decode_stream_dev's"""
    clips = _clips(x3, [10_000 * k + 40 * k for k in range(1, 12)], seed=3)
    entries = [_encode(ctx, w) for w in clips]
    buf, offs, lens = _place(entries, "even", None)
    b = Batch(ctx, buf)
    row_len = 120_000
    try:
        rows, res, summary = b.run(offs, lens, row_len)
        assert summary[1] == 0
        assert ctx.get_option("last_streams_general_walks") == 0
        for i, w in enumerate(clips):
            assert np.array_equal(rows[i, :w.size], w) and not rows[i, w.size:].any()
            d_x3, d_wav = ctx.alloc(lens[i] + 16), ctx.alloc(2 * row_len)
            ctx.upload(d_x3, buf[offs[i]:offs[i] + lens[i]])
            rc, n_out, fok, ferr = ctx.decode_stream_dev(d_x3, lens[i], x3.Params.default(), d_wav, row_len)
            assert (int(res[i]["status"]), int(res[i]["n_out"]), int(res[i]["frames_ok"]), int(res[i]["frame_errors"])) == \
                (rc, n_out, fok, ferr)
            assert np.array_equal(ctx.download(d_wav, 2 * n_out, np.int16), rows[i, :n_out])
            ctx.free(d_x3)
            ctx.free(d_wav)
    finally:
        b.close()


def _damage(ctx, x3):
    """clean and damaged entries, each damaged one between clean ones"""
    clean = [_encode(ctx, w) for w in _clips(x3, [35_000, 42_000, 51_234, 38_000, 30_001, 44_444, 25_000, 60_000, 31_000], seed=5)]
    out = [clean[0]]
    s = clean[1].copy()                       # a flipped header-CRC bit in the second frame
    f = _frames(s)
    s[f[1] + 16] ^= 0x04
    out += [s, clean[2]]
    s = clean[3].copy()                       # a payload CRC error in the third frame
    f = _frames(s)
    s[f[2] + 40] ^= 0x10
    out += [s, clean[4]]
    s = clean[5].copy()                       # a truncated last payload
    out += [s[:-7], clean[6]]
    s = clean[7]                              # junk between frames
    f = _frames(s)
    out += [np.concatenate([s[:f[2]], np.array([1, 2, 3, 4, 0x78, 0x33], dtype=np.uint8), s[f[2]:]]), clean[8]]
    rng = np.random.default_rng(77)
    out += [rng.integers(0, 256, 5000, dtype=np.uint8), clean[0]]     # garbage bytes
    return out, clean


def _decode_error_entry(ctx, x3):
    """a stream whose second frame fails to DECODE (valid CRCs): frame_errors == 1, a quiet stop"""
    wav = x3.synth(2, 99, 0, 30_000)
    s = _encode(ctx, wav).copy()
    f = _frames(s)
    a, b = f[1] + 20, f[2]
    payload = s[a:b].copy()
    payload[10:18] = 0                        # a zero run of 64 bits: OutOfBoundsInverse
    s[a:b] = payload
    crc = O.crc16(payload.tobytes())
    s[f[1] + 18], s[f[1] + 19] = crc >> 8, crc & 0xFF
    hc = O.crc16(s[f[1]:f[1] + 16].tobytes())
    s[f[1] + 16], s[f[1] + 17] = hc >> 8, hc & 0xFF
    return s


def test_damaged_entries(ctx, x3):
    entries, clean = _damage(ctx, x3)
    entries = entries + [_decode_error_entry(ctx, x3), clean[1]]
    buf, offs, lens = _place(entries, "even", None)
    b = Batch(ctx, buf)
    try:
        for row_len in (60_000, 40_000):      # 40 000: several entries longer than their row
            want = _expect(buf, offs, lens, row_len, None)
            assert any(w[3] == 1 for w in want), "the decode-error entry must count a frame error"
            assert sum(w[0] != 0 for w in want) >= 3
            for fmt in (0, 1):
                _check(b.run(offs, lens, row_len, fmt), want, row_len, fmt)
                assert ctx.get_option("last_streams_general_walks") > 0      # junk between frames takes the general walk
        # the library's own single-entry call agrees with the oracle on every one of them
        for i, (o, n) in enumerate(zip(offs, lens)):
            d_x3, d_wav = ctx.alloc(n + 16), ctx.alloc(2 * 60_000)
            ctx.upload(d_x3, buf[o:o + n])
            rc, n_out, fok, ferr = ctx.decode_stream_dev(d_x3, n, x3.Params.default(), d_wav, 60_000)
            wrc, w, wfok, wferr = O.decode_stream(buf[o:o + n], wav_cap=60_000)
            assert (rc, n_out, fok, ferr) == (wrc, w.size, wfok, wferr), i
            ctx.free(d_x3)
            ctx.free(d_wav)
    finally:
        b.close()


def test_archive_entries(ctx, x3):
    """the frame parts of .x3a archives (default and tuned parameters) with X3_STREAMS_ARCHIVE_FRAMES == x3_x3a_decode"""
    clips = _clips(x3, [44_100, 12_345, 90_000, 1, 0], seed=9)
    archives = [ctx.x3a_encode(w, 44_100)[1] for w in clips]
    by_p = {}
    for a in archives:
        rc, rate, p, ch, hs = x3.archive_header_read(a)
        assert rc == 0
        by_p.setdefault(bytes(p), (p, []))[1].append((a[:8 + hs], a[8 + hs:]))
    # one truncated, one with 3 bytes fewer than the phantom bytes would cover
    p, lst = by_p[bytes(x3.Params.default())]
    h, body = lst[0]
    lst += [(h, body[:-3]), (h, body[:-100])]
    p, lst = next(iter(by_p.values()))
    headers = [h for h, _ in lst]
    buf, offs, lens = _place([b for _, b in lst], "odd", None)
    bt = Batch(ctx, buf)
    try:
        for fmt in (0, 1):
            want = _expect(buf, offs, lens, 92_000, None, archive=True, headers=headers)
            _check(bt.run(offs, lens, 92_000, fmt, p, flags=x3.STREAMS_ARCHIVE_FRAMES), want, 92_000, fmt)
    finally:
        bt.close()


def test_decode_archives_mixed_parameter_sets(ctx, x3, tmp_path):
    """x3hip.decode_archives on default and tuned archives (block lengths 10 / 20 / 40), bytes and paths: input order"""
    clips = _clips(x3, [30_000, 20_001, 50_000, 7, 41_000, 25_000], seed=11)
    kinds = [x3.SYNTH_WHITE, x3.SYNTH_SINE, x3.SYNTH_WALK, x3.SYNTH_HYDROPHONE]
    clips += [x3.synth(k, 40 + k, 0, 36_000) for k in kinds]
    archives, bls = [], set()
    for i, w in enumerate(clips):
        if i % 2:
            rc, a, _, p = ctx.x3a_encode_tuned(w, 16_000 + i)
            bls.add(p.block_len)
        else:
            rc, a, _ = ctx.x3a_encode(w, 16_000 + i)
            bls.add(20)
        assert rc == 0
        archives.append(a)
    path = tmp_path / "clip.x3a"
    path.write_bytes(archives[2].tobytes())
    inputs = list(archives)
    inputs[2] = str(path)
    for fmt in (0, 1):
        rows, res, rates = x3.decode_archives(ctx, inputs, fmt=fmt)
        assert rows.shape == (len(clips), 50_000)
        for i, (a, w) in enumerate(zip(archives, clips)):
            rc, ref, rate, fok, ferr = O.x3a_decode(a, wav_cap=50_000)
            assert rc == 0 and np.array_equal(ref, w)
            assert (int(res[i]["status"]), int(res[i]["n_out"]), int(res[i]["frames_ok"])) == (0, w.size, fok)
            assert rates[i] == 16_000 + i
            full = np.zeros(50_000, dtype=np.int16)
            full[:w.size] = w
            assert np.array_equal(rows[i].view(np.uint32) if fmt else rows[i], _f32(full) if fmt else full), i
    assert len(bls) >= 2, bls


@pytest.mark.parametrize("bl,bpf,codes,row_len", [(10, 1000, (0, 1, 3), 40_000), (40, 250, (0, 1, 3), 40_000),
                                                  (20, 500, (0, 1, 3), 40_001), (20, 500, (1, 2, 3), 40_000),
                                                  (20, 100, (0, 1, 3), 40_000)])
def test_parameter_sets(ctx, x3, bl, bpf, codes, row_len):
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    op = O.Params.make(bl, bpf, codes)
    clips = _clips(x3, [0, 1, 10_000, 19_999, 20_000, 39_000, 40_000], seed=13)
    entries = []
    for w in clips:
        if w.size == 0:
            entries.append(np.zeros(0, dtype=np.uint8))
            continue
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        entries.append(s)
    entries.insert(3, _damage(ctx, x3)[0][1][:3000])
    buf, offs, lens = _place(entries, "gaps", np.random.default_rng(bl))
    want = _expect(buf, offs, lens, row_len, op)
    b = Batch(ctx, buf)
    try:
        for fmt in (0, 1):
            _check(b.run(offs, lens, row_len, fmt, p), want, row_len, fmt)
    finally:
        b.close()


def test_argument_errors_enqueue_nothing(ctx, x3):
    s = _encode(ctx, x3.synth(2, 5, 0, 20_000))
    buf = np.concatenate([s, np.zeros(16, dtype=np.uint8)])
    b = Batch(ctx, buf)
    n = s.size
    try:
        L = x3.lib()
        p = x3.Params.default()
        d_out = ctx.alloc(4 * 3 * 30_000 + 64)
        d_res = ctx.alloc(RES_BYTES * 3 + 64)
        off = np.array([0, 0], dtype=np.uint64)
        ln = np.array([n, n], dtype=np.uint64)

        def call(d_x3=b.d_x3, x3_len=n, offs=off, lens=ln, k=2, flags=0, params=p, out=d_out, row_len=30_000, fmt=0, res=d_res):
            return L.x3_decode_streams_dev(ctx._h, d_x3, x3_len, offs.ctypes.data, lens.ctypes.data, k, flags, C.byref(params),
                                           out, row_len, fmt, res)
        assert call(k=0) == BAD
        assert call(row_len=0) == BAD
        assert call(fmt=2) == BAD
        assert call(flags=2) == BAD
        assert call(d_x3=b.d_x3 + 1) == BAD
        assert call(out=d_out + 1) == BAD
        assert call(out=d_out + 2, fmt=1) == BAD
        assert call(offs=np.array([0, 1], dtype=np.uint64)) == BAD
        assert call(lens=np.array([n, n + 1], dtype=np.uint64)) == BAD
        assert call(offs=np.array([0, n + 1], dtype=np.uint64), lens=np.array([n, 0], dtype=np.uint64)) == BAD
        assert call(params=x3.Params.make(codes=(0, 1, 4))) == BAD
        # nothing pending behind a refused call
        assert ctx.decode_streams_result()[0] == BAD
        ctx.free(d_out)
        ctx.free(d_res)
        # and the canaries stay whole for a refused call through the helper
        b.run([0], [n + 1], 100, expect_rc=BAD)
        # an entry of length 0 at x3_len itself is in range
        rows, res, summary = b.run([n], [0], 4)
        assert summary[1] == 0 and not rows.any() and int(res[0]["n_out"]) == 0
    finally:
        b.close()


def test_a_streams_call_replaces_the_pending_decode(ctx, x3):
    s = _encode(ctx, x3.synth(2, 6, 0, 20_000))
    buf = np.concatenate([s, np.zeros(16, dtype=np.uint8)])
    b = Batch(ctx, buf)
    try:
        b.run([0], [s.size], 20_000)
        assert ctx.decode_result()[0] == BAD
        assert ctx.decode_streams_result()[0] == BAD    # (the result was taken)
    finally:
        b.close()


def test_large_batch_1000_one_minute_clips_at_96k(ctx, x3):
    """config 5's shape: 1 000 clips of 60 s at 96 kHz (x3_synth_dev), encoded by x3_encode_frames_dev back to back, decoded in
    one x3_decode_streams_dev call; every row equals its clip"""
    n_clips, n = 1000, 60 * 96_000
    p = x3.Params.default()
    spf = 10_000
    total = n_clips * n
    d_wav = ctx.alloc(2 * total)
    ctx.synth_dev(x3.SYNTH_HYDROPHONE, 0x96, 0, total, d_wav)
    so, sn = [], []
    for c in range(n_clips):
        for a in range(0, n, spf):
            so.append(c * n + a)
            sn.append(min(spf, n - a))
    F = len(so)
    cap = n_clips * x3.lib().x3_encode_bound(n, C.byref(p)) + 64
    d_x3, d_off = ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    d_out = ctx.alloc(2 * total)
    d_res = ctx.alloc(RES_BYTES * n_clips)
    try:
        assert ctx.encode_frames_dev(d_wav, so, sn, p, d_x3, cap, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        fo = ctx.download(d_off, 8 * (F + 1), np.uint64)
        fpc = n // spf + (1 if n % spf else 0)
        offs = [int(fo[c * fpc]) for c in range(n_clips)]
        lens = [int(fo[(c + 1) * fpc]) - offs[c] for c in range(n_clips)]
        assert ctx.decode_streams_dev(d_x3, pos, offs, lens, p, d_out, n, 0, d_res) == 0
        rc, n_bad, first_bad, _ = ctx.decode_streams_result()
        assert (rc, n_bad, first_bad) == (0, 0, n_clips)
        assert ctx.get_option("last_streams_general_walks") == 0
        res = ctx.download(d_res, RES_BYTES * n_clips, np.uint8).view(x3.STREAM_RESULT_DTYPE)
        assert (res["n_out"] == n).all() and (res["status"] == 0).all() and (res["frames_ok"] == fpc).all()
        step = 50
        for c in range(0, n_clips, step):
            got = ctx.download(d_out + 2 * c * n, 2 * step * n, np.int16)
            ref = ctx.download(d_wav + 2 * c * n, 2 * step * n, np.int16)
            assert np.array_equal(got, ref), c
    finally:
        for q in (d_wav, d_x3, d_off, d_out, d_res):
            ctx.free(q)


def test_x3_hpp_decode_streams(tmp_path):
    """tests/host_cpp/test_streams_hpp.cpp: device::decode_streams of the C++ mirror"""
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_streams_hpp.cpp")
    exe = str(tmp_path / "test_streams_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
