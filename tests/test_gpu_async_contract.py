"""The asynchronous contract of include/x3hip.h: `*_dev` entry points enqueue on the context's stream and do not
synchronise; a context works on a stream its caller owns; several contexts on one GPU, from several host threads, are
supported use; whatever is enqueued behind an encode finds the whole stream.

A-B  every asynchronous entry point behind a stalled stream, its inputs arriving behind the stall (async_cases.py)
C    more than 4 096 calls on one context: the 12-bit epochs that replace clearing wrap
D    several contexts on one GPU: one thread, four threads, the file pipeline beside another context
No test asserts a time, none asserts that a fallback happens; the figures go to the report (X3_ASYNC_REPORT=<file>)."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import async_cases as AC
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch     # (bench.py's order: torch first, its HIP runtime serves the library too)
    return torch


@pytest.fixture(scope="module")
def x3(torch):
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def report():
    t0 = time.perf_counter()
    yield AC.log
    AC.log("run time of tests/test_gpu_async_contract.py: %.1f s" % (time.perf_counter() - t0))
    path = os.environ.get("X3_ASYNC_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(AC.LOG) + "\n")


@pytest.fixture(scope="module")
def cycles_per_ms(torch, report):
    return AC.calibrate_sleep(torch)


# ------------------------------------------------------------------------------------------------ A, B

@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.name)
def test_behind_a_stalled_stream(x3, torch, cycles_per_ms, case):
    """the call's inputs hold a decoy when it is enqueued; the content arrives behind a stall that is proven to be still
    running when the enqueue returns; clones taken in stream order and the originals equal the oracle's results"""
    AC.run_stalled(x3, torch, case, cycles_per_ms)


def test_calls_that_wait_return_the_content_behind_the_stall(x3, torch, cycles_per_ms):
    """x3_decode_stream_dev, x3_index_dev, x3_crc16_dev, x3_corpus_build and the single-wave shapes of x3_decode_streams_dev
    go to the host by design: called behind a stall and an on-stream copy of B over the decoy, they return B's results.
    (x3_index_dev is here and not among the stalled cases because the header marks it "Synchronous": the stall would only
    be waited out.)"""
    S = torch.cuda.Stream()
    ctx = x3.Context(0, stream=S.cuda_stream)
    p = x3.Params.default()
    a, b = AC.padded([AC.encoded("A")[0], AC.damaged_b()[0]])
    blen = AC.encoded("B")[0].size
    try:
        with torch.cuda.stream(S):
            src = {w: torch.from_numpy(v.copy()).to("cuda") for w, v in (("A", a), ("B", b))}
            work = torch.empty_like(src["A"])
            back = torch.zeros(AC.N0, dtype=torch.int16, device="cuda")
            offs = torch.zeros(AC.F0 + 8, dtype=torch.int64, device="cuda")
            woffs = torch.zeros(AC.F0 + 8, dtype=torch.int64, device="cuda")

            def stalled():
                work.copy_(src["A"])
                S.synchronize()
                torch.cuda._sleep(int(5 * cycles_per_ms))
                work.copy_(src["B"], non_blocking=True)

            stalled()
            got = ctx.decode_stream_dev(work.data_ptr(), blen, p, back.data_ptr(), AC.N0)
            want = O.decode_stream(b[:blen], AC.oparams(), wav_cap=AC.N0)
            assert got == (want[0], want[1].size, want[2], want[3]), (got, want[0], want[1].size)
            assert np.array_equal(back.cpu().numpy()[:want[1].size], want[1])

            stalled()
            rc, nf, ns, term = ctx.index_dev(work.data_ptr(), blen, AC.F0 + 8, offs.data_ptr(), woffs.data_ptr())
            assert (rc, nf, ns, term) == (0, AC.F0, AC.N0, 0)      # (the walk checks headers only: every frame of B)
            assert np.array_equal(offs.cpu().numpy()[:AC.F0].astype(np.uint64), AC.encoded("B")[1][:-1])

            stalled()
            crc = C.c_uint16(0)
            assert x3.lib().x3_crc16_dev(ctx._h, work.data_ptr(), blen, C.byref(crc)) == 0
            assert crc.value == O.crc16(b[:blen]) != O.crc16(a[:blen])

            bufs = {w: AC.entries(w, False) for w in ("A", "B")}
            src = {w: torch.from_numpy(bufs[w][0].copy()).to("cuda") for w in ("A", "B")}
            work = torch.empty_like(src["A"])
            stalled()
            buf, eoffs, elens, ents = bufs["B"]
            corpus = x3.Corpus(ctx, (work.data_ptr(), buf.size - 16), eoffs, elens, p, seg_blocks=32)
            try:
                assert corpus.entries["n_samples"].tolist() == list(AC.ENTRY_SAMPLES)
                rng = np.random.default_rng(3)
                e = rng.integers(0, len(ents), size=40).astype(np.uint32)
                st = np.array([rng.integers(0, AC.ENTRY_SAMPLES[k] - 999) for k in e], dtype=np.uint64)
                rows, status = corpus.decode(e, st, 1000)
                assert not status.any()
                for r, k, s0 in zip(rows, e, st):
                    w = O.decode_stream(ents[k], AC.oparams(), wav_cap=AC.ROW_LEN)[1]
                    assert np.array_equal(r, w[int(s0):int(s0) + 1000])
            finally:
                corpus.close()

            # x3_decode_streams_dev where the decoder cannot read its frame count from the device and the call waits once
            # for it: a row_len that is no multiple of 4, and codes other than the defaults -- both formats each
            for codes, thr, row_len in (((0, 1, 3), (3, 8, 20), AC.ROW_LEN + 2), ((0, 1, 2), (3, 8, 18), AC.ROW_LEN)):
                bufs = {w: AC.entries(w, False, codes, thr) for w in ("A", "B")}
                assert bufs["A"][2] == bufs["B"][2] and not np.array_equal(bufs["A"][0], bufs["B"][0])
                src = {w: torch.from_numpy(bufs[w][0].copy()).to("cuda") for w in ("A", "B")}
                work = torch.empty_like(src["A"])
                buf, eoffs, elens, ents = bufs["B"]
                pp, op = x3.Params.make(20, 500, codes, thr), O.Params.make(20, 500, codes, thr)
                want = [O.decode_stream(s, op, wav_cap=row_len) for s in ents]
                bad = [(e, w[0]) for e, w in enumerate(want) if w[0]]
                E = len(ents)
                for fmt in (0, 1):
                    rows = torch.full((E * row_len,), -7, dtype=torch.float32 if fmt else torch.int16, device="cuda")
                    res = torch.zeros(24 * E, dtype=torch.uint8, device="cuda")
                    stalled()
                    assert ctx.decode_streams_dev(work.data_ptr(), buf.size - 16, eoffs, elens, pp, rows.data_ptr(), row_len,
                                                  fmt, res.data_ptr()) == 0, ctx.last_error()
                    assert ctx.decode_streams_result() == (0, len(bad), bad[0][0] if bad else E, bad[0][1] if bad else 0)
                    got = rows.cpu().numpy().reshape(E, row_len)
                    r = res.cpu().numpy().view(x3.STREAM_RESULT_DTYPE)
                    for e, (rc, w, fok, ferr) in enumerate(want):
                        assert (int(r[e]["status"]), int(r[e]["n_out"]), int(r[e]["frames_ok"]), int(r[e]["frame_errors"])) == \
                            (rc, w.size, fok, ferr), (codes, row_len, fmt, e)
                        full = np.zeros(row_len, dtype=np.int16)
                        full[:w.size] = w
                        assert np.array_equal(got[e].view(np.uint32), AC.f32_bits(full)) if fmt else np.array_equal(got[e], full), \
                            (codes, row_len, fmt, e)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ C

class RoundTrip:
    """one input on the device with the oracle's stream beside it: encode + decode enqueued with nothing waited for in
    between, then both results and a comparison of every output on the device"""

    def __init__(self, x3, torch, which, bl, bpf, n):
        self.x3, self.torch, self.n = x3, torch, n
        self.p = x3.Params.make(bl, bpf)
        op = AC.oparams(bl, bpf)
        self.F = (n + bl * bpf - 1) // (bl * bpf)
        self.cap = O.encode_bound(n, op)
        s, offs, self.stats = AC.encoded(which, bl, bpf, n)
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.want = {"out": cuda(s), "off": cuda(offs), "back": cuda(AC.wav(which)[:n])}
        self.pos = int(s.size)
        self.wav = self.want["back"].clone()
        self.out = torch.empty(self.cap + 16, dtype=torch.uint8, device="cuda")
        self.off = torch.empty(8 * (self.F + 1), dtype=torch.uint8, device="cuda")
        self.back = torch.empty(2 * n, dtype=torch.uint8, device="cuda")

    def _decode(self, ctx):
        assert ctx.decode_dev(self.out.data_ptr(), self.cap, self.off.data_ptr(), self.F, self.p, self.back.data_ptr(),
                              self.n, n_per_clip=self.n) == 0, ctx.last_error()

    def enqueue(self, ctx, decode=True):
        for t in (self.out, self.off, self.back):
            t.fill_(AC.CANARY)
        assert ctx.encode_dev(self.wav.data_ptr(), self.n, self.p, self.out.data_ptr(), self.cap, 0,
                              self.off.data_ptr()) == 0, ctx.last_error()
        if decode:
            self._decode(ctx)

    def check(self, ctx, what, decode=True):
        """-> 1 if the encode launch fell back to two passes"""
        fb = ctx.get_option("encode_fallbacks")
        rc, pos, stats = ctx.encode_result()
        fell = ctx.get_option("encode_fallbacks") - fb
        assert fell in (0, 1), (what, fell)
        if fell:
            assert ctx.get_option("enc_gen_in_use") == 0, what
        assert (rc, pos, [int(v) for v in stats]) == (0, self.pos, self.stats), (what, rc, pos)
        if decode:
            r = ctx.decode_result()
            if fell:      # (the stream was rewritten under the decoder: the header's rule)
                self._decode(ctx)
                r = ctx.decode_result()
            assert r == (0, self.F, 0, self.n), (what, r)
            assert self.torch.equal(self.back, self.want["back"]), (what, "samples")
        assert self.torch.equal(self.out[:self.pos], self.want["out"]), (what, "stream bytes")
        assert self.torch.equal(self.off, self.want["off"]), (what, "frame offsets")
        return fell


LONG_RUNS = {
    # name: (block length, options, kernels expected: encoder generation, decoder kernel)
    "wave_and_three_wave_decoder": (20, {}, 3, 2),
    "second_generation": (20, {"enc_gen": 2}, 2, 2),
    "general_one_pass": (19, {}, 1, 1),
    "block_per_lane_decoder": (20, {"decode_blocks": 1}, 3, 3),
}


@pytest.mark.parametrize("name", list(LONG_RUNS))
def test_4200_round_trips_on_one_context(x3, torch, report, name):
    """the 12-bit epochs (desc_epoch, lb_epoch, enc_log_epoch, the decoder's pace word) wrap at 4 096 calls.  Call 0 is a
    large one (400 frames, content C): its descriptors carry epoch 1.  Calls 1 .. 4 094 alternate between two small inputs
    of different frame sizes and counts, which rewrite the first few descriptors only.  Call 4 095 is the one whose epoch
    wraps to 1 again, and it is a large call with OTHER content (D): descriptors that were not cleared would read "ready"
    with C's frame sizes.  Call 4 150 is larger than any before: the buffer grows (the `fresh` branch).  Every call is
    held against the oracle's bytes, nothing is waited for between an encode and its decode"""
    bl, options, gen, dec = LONG_RUNS[name]
    S = torch.cuda.Stream()
    ctx = x3.Context(0, stream=S.cuda_stream)
    try:
        with torch.cuda.stream(S):
            for k, v in options.items():
                ctx.set_option(k, v)
            small = [RoundTrip(x3, torch, "A", bl, 50, bl * 50 * 5 - 200), RoundTrip(x3, torch, "B", bl, 100, bl * 100 * 3)]
            special = {0: RoundTrip(x3, torch, "C", bl, 50, bl * 50 * 400), 4095: RoundTrip(x3, torch, "D", bl, 50, bl * 50 * 400),
                       4150: RoundTrip(x3, torch, "B", bl, 50, bl * 50 * 480)}
            fell = 0
            for i in range(4200):
                rt = special.get(i, small[i & 1])
                rt.enqueue(ctx)
                fell += rt.check(ctx, (name, i))
                if i in (0, 1, 4095, 4199) and not fell:
                    assert (ctx.get_option("enc_gen_in_use"), ctx.get_option("decode_kernel_in_use")) == (gen, dec), (name, i)
            report("long run %-30s 4200 round trips, %d encode fallbacks" % (name, fell))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ D

def test_two_contexts_one_thread(x3, torch, report):
    """two persistent encoder grids enqueued before either is waited for, then an encode beside a decode: the streams and
    statistics are the oracle's whether or not a launch gave up its bounded wait; per call encode_fallbacks grows by 0 or
    1 and a call that fell back was served in two passes"""
    S = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [x3.Context(0, stream=s.cuda_stream) for s in S]
    try:
        rts = []
        for s, which in zip(S, ("A", "B")):
            with torch.cuda.stream(s):
                rts.append(RoundTrip(x3, torch, which, 20, 500, AC.N0))
                s.synchronize()
        fell = [0, 0]
        for rnd in range(50):
            for k in (0, 1):
                with torch.cuda.stream(S[k]):
                    rts[k].enqueue(ctxs[k], decode=False)
            for k in (0, 1):
                with torch.cuda.stream(S[k]):
                    fell[k] += rts[k].check(ctxs[k], ("encode beside encode", rnd, k), decode=False)
            # context 1 encodes while context 0 decodes the stream it has just checked
            with torch.cuda.stream(S[0]):
                rts[0].back.fill_(AC.CANARY)
                rts[0]._decode(ctxs[0])
            with torch.cuda.stream(S[1]):
                rts[1].enqueue(ctxs[1], decode=False)
            with torch.cuda.stream(S[0]):
                assert ctxs[0].decode_result() == (0, AC.F0, 0, AC.N0), rnd
                assert torch.equal(rts[0].back, rts[0].want["back"]), rnd
            with torch.cuda.stream(S[1]):
                fell[1] += rts[1].check(ctxs[1], ("encode beside decode", rnd), decode=False)
        report("two contexts, one thread: 50 rounds, 150 encode calls, encode fallbacks %d + %d" % tuple(fell))
    finally:
        for c in ctxs:
            c.close()


def _thread_content(k):
    n = 12 * AC.SPF
    w = AC.wav("ABCD"[k])[k * 1000:k * 1000 + n]
    rc, s, st = O.encode(w, AC.oparams())
    assert rc == 0
    ents = []
    for e in range(3):
        m = (23_000, 11_000, 16_000)[e]
        ents.append(O.encode(w[e * 30_000:e * 30_000 + m], AC.oparams())[1])
    return w, s, [int(v) for v in st], ents


def test_four_threads_four_contexts(x3, report):
    """a context per host thread, started behind a barrier: 25 rounds of encode, decode, windows and a batch of streams
    each, everything held against oracle results computed before the threads start"""
    T, ROUNDS, L = 4, 25, 3000
    content = [_thread_content(k) for k in range(T)]
    barrier = threading.Barrier(T)
    errors, fell = [], [0] * T

    def work(k):
        ctx = ws = None
        try:
            w, s, st, ents = content[k]
            n, F, p = w.size, 12, x3.Params.default()
            ctx = x3.Context(0)
            cap = O.encode_bound(n, AC.oparams())
            d_wav, d_out, d_off, d_back = ctx.alloc(2 * n), ctx.alloc(cap + 16), ctx.alloc(8 * (F + 1)), ctx.alloc(2 * n)
            ctx.upload(d_wav, w)
            ws = x3.WindowSource(ctx, s, p, seg_blocks=32)
            blob = np.concatenate(ents + [np.zeros(16, dtype=np.uint8)])
            lens = [int(e.size) for e in ents]
            offs = [0, lens[0], lens[0] + lens[1]]
            d_blob, d_rows, d_res = ctx.alloc(blob.size), ctx.alloc(2 * 3 * 24_000), ctx.alloc(24 * 3)
            ctx.upload(d_blob, blob)
            want_rows = np.zeros((3, 24_000), dtype=np.int16)
            for e in range(3):
                m = (23_000, 11_000, 16_000)[e]
                want_rows[e, :m] = w[e * 30_000:e * 30_000 + m]
            rng = np.random.default_rng(k)
            barrier.wait()
            for rnd in range(ROUNDS):
                fb = ctx.get_option("encode_fallbacks")
                assert ctx.encode_dev(d_wav, n, p, d_out, cap, 0, d_off) == 0
                assert ctx.decode_dev(d_out, cap, d_off, F, p, d_back, n, n_per_clip=n) == 0
                rc, pos, stats = ctx.encode_result()
                d = ctx.get_option("encode_fallbacks") - fb
                assert d in (0, 1) and (d == 0 or ctx.get_option("enc_gen_in_use") == 0)
                fell[k] += d
                assert (rc, pos, [int(v) for v in stats]) == (0, s.size, st), (k, rnd)
                r = ctx.decode_result()
                if d:
                    assert ctx.decode_dev(d_out, cap, d_off, F, p, d_back, n, n_per_clip=n) == 0
                    r = ctx.decode_result()
                assert r == (0, F, 0, n), (k, rnd, r)
                assert np.array_equal(ctx.download(d_out, (pos + 3) & ~3)[:pos], s), (k, rnd)
                assert np.array_equal(ctx.download(d_back, 2 * n, np.int16), w), (k, rnd)
                starts = rng.integers(0, n - L + 1, size=16)
                rows, status = ws.decode(starts, L, rnd & 1)
                assert not status.any()
                for row, s0 in zip(rows, starts):
                    want = w[s0:s0 + L]
                    assert np.array_equal(row.view(np.uint32), AC.f32_bits(want)) if rnd & 1 else np.array_equal(row, want), (k, rnd)
                assert ctx.decode_streams_dev(d_blob, blob.size - 16, offs, lens, p, d_rows, 24_000, 0, d_res) == 0
                assert ctx.decode_streams_result() == (0, 0, 3, 0), (k, rnd)
                assert np.array_equal(ctx.download(d_rows, 2 * 3 * 24_000, np.int16).reshape(3, 24_000), want_rows), (k, rnd)
                res = ctx.download(d_res, 72, x3.STREAM_RESULT_DTYPE)
                assert res["n_out"].tolist() == [23_000, 11_000, 16_000] and not res["status"].any()
        except BaseException as e:   # noqa: BLE001 -- re-raised in the main thread
            errors.append((k, e))
            barrier.abort()
        finally:
            if ws is not None:
                ws.close()
            if ctx is not None:
                ctx.close()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(T)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    report("four threads, four contexts: %d rounds each, encode fallbacks %s" % (ROUNDS, fell))
    if errors:
        raise errors[0][1]


def test_file_pipeline_beside_another_context(x3, report, tmp_path):
    """x3_wav_to_x3a with four workers on one context while a second thread encodes on another: the pipeline's gate does
    not know about the second context"""
    n = 64 * AC.SPF
    w = np.concatenate([AC.wav("A"), AC.wav("B")[:n - AC.N0]])
    wav_path, got_path, want_path = (str(tmp_path / f) for f in ("in.wav", "gpu.x3a", "oracle.x3a"))
    with open(wav_path, "wb") as f:
        f.write(O.wav_header(48_000, n).tobytes())
        f.write(w.tobytes())
    rc, st_o = O.wav_to_x3a(wav_path, want_path)
    assert rc == 0
    s, _, st = AC.encoded("B")
    errors, fell, stop = [], [0, 0], threading.Event()

    def encoder():
        ctx = None
        try:
            ctx = x3.Context(0)
            cap = O.encode_bound(AC.N0, AC.oparams())
            d_wav, d_out = ctx.alloc(2 * AC.N0), ctx.alloc(cap + 16)
            ctx.upload(d_wav, AC.wav("B"))
            rounds = 0
            while rounds < 20 or (not stop.is_set() and rounds < 400):
                fb = ctx.get_option("encode_fallbacks")
                assert ctx.encode_dev(d_wav, AC.N0, x3.Params.default(), d_out, cap, 0, None) == 0
                rc, pos, stats = ctx.encode_result()
                d = ctx.get_option("encode_fallbacks") - fb
                assert d in (0, 1) and (d == 0 or ctx.get_option("enc_gen_in_use") == 0)
                fell[1] += d
                assert (rc, pos, [int(v) for v in stats]) == (0, s.size, st), rounds
                assert np.array_equal(ctx.download(d_out, (pos + 3) & ~3)[:pos], s), rounds
                rounds += 1
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
        finally:
            if ctx is not None:
                ctx.close()

    t = threading.Thread(target=encoder)
    ctx = x3.Context(0)
    try:
        ctx.set_option("file_workers", 4)
        ctx.set_option("file_chunk_frames", 4)
        t.start()
        for k in range(3):
            rc, stats = ctx.wav_to_x3a(wav_path, got_path)
            assert rc == 0, ctx.last_error()
            assert [int(v) for v in stats] == [int(v) for v in st_o]
            with open(got_path, "rb") as f, open(want_path, "rb") as g:
                assert f.read() == g.read(), k
        fell[0] = ctx.get_option("encode_fallbacks")
    finally:
        stop.set()
        t.join()
        ctx.close()
    report("file pipeline (4 workers, 3 files of 16 chunks) beside an encoding context: encode fallbacks %d (the pipeline's "
           "own context) + %d (the other context)" % tuple(fell))
    if errors:
        raise errors[0]


def test_32_contexts_one_after_the_other(x3):
    w = AC.wav("A")[:25_000]
    rc, s, st = O.encode(w, AC.oparams())
    for k in range(32):
        ctx = x3.Context(0)
        try:
            rc, got, stats = ctx.encode(w)
            assert rc == 0 and np.array_equal(got, s) and [int(v) for v in stats] == [int(v) for v in st], k
            rc, back, fok, ferr = ctx.decode_stream(got, wav_cap=w.size)
            assert (rc, fok, ferr) == (0, 3, 0) and np.array_equal(back, w), k
        finally:
            ctx.close()
