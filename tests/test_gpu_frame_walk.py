"""The GPU frame walk on long, dense and adversarial streams (x3_index_kernels.h, index_dev_impl and
decode_stream_dev_impl in x3_decode.hip), held to the plain walk of frame_walk_ref and to the CPU oracle.

Every call says which branch it reached: the read-only counters index_fast_walks / index_general_walks (path),
last_index_candidates (what the candidate scan found = frame_walk_ref.scan), index_rescans (the second scan of a stream
with more candidates than the first buffer holds) and stream_one_trip (x3_decode_stream_dev's speculative decode kept).
Outputs go to device buffers with 1 MiB of 0x5A behind wav_cap that must come back untouched.

Wall time of this file on one MI355X, measured once: 6 s for the pytest process (87 tests; the largest stream is the
27 MB chain of 2^20 + 1 frames, the slowest step building the 5 MB dense stream on the CPU)."""
import numpy as np
import pytest

import frame_walk_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

SLACK = 1 << 20


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def xparams(x3, case):
    return x3.Params.make(case.params.block_len, case.params.blocks_per_frame)


class Dev:
    """device copies of a stream and output buffers, freed on exit"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, n):
        p = self.ctx.alloc(max(n, 16))
        self.ptrs.append(p)
        return p

    def stream(self, s):
        d = self.alloc(s.size + 16)
        self.ctx.upload(d, np.concatenate([s, np.zeros(16, dtype=np.uint8)]))
        return d

    def wav(self, cap):
        """cap samples and SLACK bytes behind them, all 0x5A"""
        d = self.alloc(2 * cap + SLACK)
        self.ctx.upload(d, np.full(2 * cap + SLACK, 0x5A, dtype=np.uint8))
        return d

    def slack_intact(self, d, cap):
        return bool(np.all(self.ctx.download(d + 2 * cap, SLACK) == 0x5A))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.ctx.free(p)


def counters(ctx):
    return {k: ctx.get_option(k) for k in ("index_fast_walks", "index_general_walks", "index_rescans", "stream_one_trip")}


def delta(ctx, before):
    now = counters(ctx)
    return {k: now[k] - before[k] for k in now}


def is_clean(case, w):
    """one clean chain from offset 0: every candidate is a frame the walk steps over (the fast path's case)"""
    return (w.terminal == R.OK and np.array_equal(R.scan(case.stream), w.frame_off.astype(np.int64))
            and w.n_frames > 0)


def check_index(ctx, case, no_fast, max_frames=None):
    """x3_index_dev == the plain walk; the counters show the path.  -> the counters' change"""
    s = case.stream
    w = R.walk(s)
    ctx.set_option("index_no_fast", no_fast)
    mf = max_frames if max_frames is not None else s.size // 20 + 2
    with Dev(ctx) as d:
        d_x3 = d.stream(s)
        room = max(mf, 1) + 8
        d_fo, d_wo = d.alloc(8 * room + SLACK), d.alloc(8 * room + SLACK)
        for p in (d_fo, d_wo):
            ctx.upload(p + 8 * room, np.full(SLACK, 0x5A, dtype=np.uint8))
        before = counters(ctx)
        rc, nf, ns, term = ctx.index_dev(d_x3, s.size, mf, d_fo, d_wo)
        dl = delta(ctx, before)
        for p in (d_fo, d_wo):
            assert np.all(ctx.download(p + 8 * room, SLACK) == 0x5A)
        if w.n_frames > mf:
            assert rc == R.BAD_ARG, (case, rc)
            return dl
        assert rc == 0, (case, ctx.last_error())
        assert (nf, ns, term) == (w.n_frames, w.n_samples, w.terminal), (case, no_fast, w)
        if nf:
            assert np.array_equal(ctx.download(d_fo, 8 * nf, np.uint64), w.frame_off), case
            assert np.array_equal(ctx.download(d_wo, 8 * nf, np.uint64), w.wav_off), case
    if no_fast or not is_clean(case, w):
        assert (dl["index_general_walks"], dl["index_fast_walks"]) == (1, 0), (case, dl)
        assert ctx.get_option("last_index_candidates") == R.scan(s).size, case
    else:
        assert (dl["index_general_walks"], dl["index_fast_walks"]) == (0, 1), (case, dl)
    return dl


def check_decode(ctx, x3, case, two_trips, wav_cap=None, decode_blocks=0):
    """x3_decode_stream_dev == the oracle's decode_stream, nothing written behind wav_cap.  -> the counters' change"""
    s = case.stream
    cap = wav_cap if wav_cap is not None else int(R.walk(s).n_samples) + 65536
    rc_o, wav_o, fok_o, ferr_o = O.decode_stream(s, case.params, wav_cap=cap)
    ctx.set_option("index_no_fast", 0)
    ctx.set_option("two_trips", two_trips)
    ctx.set_option("decode_blocks", decode_blocks)
    try:
        with Dev(ctx) as d:
            d_x3, d_wav = d.stream(s), d.wav(cap)
            before = counters(ctx)
            rc, n, fok, ferr = ctx.decode_stream_dev(d_x3, s.size, xparams(x3, case), d_wav, cap)
            dl = delta(ctx, before)
            assert (rc, n, fok, ferr) == (rc_o, wav_o.size, fok_o, ferr_o), (case, two_trips, decode_blocks)
            if n:
                assert np.array_equal(ctx.download(d_wav, 2 * n, np.int16), wav_o), case
            assert d.slack_intact(d_wav, cap), ("written behind wav_cap", case)
    finally:
        ctx.set_option("two_trips", 0)
        ctx.set_option("decode_blocks", 0)
    return dl


def zero_lengths():
    return [n for m in (9, 10, 11, 12) for n in (2 ** m - 1, 2 ** m, 2 ** m + 1)] + [2 ** 17 + 1]


def damaged():
    from test_frame_walk_ref import dense_lead_in
    return [("padded+junk", lambda: R.junk_front(R.padded())), ("dense+broken", lambda: R.broken_header(R.dense(), 100)),
            ("dense+lead", dense_lead_in), ("odd_tails-cut", lambda: R.truncated(R.odd_tails(), 100)),
            ("zeros+broken", lambda: R.broken_header(R.zero_chain(2 ** 12 + 1), 3000)),
            ("sparse+junk", lambda: R.junk_front(R.sparse(), 3)), ("sparse-cut", lambda: R.truncated(R.sparse(), 7))]


GENERATED = [("padded", R.padded), ("odd_tails", R.odd_tails), ("sparse", R.sparse), ("dense", R.dense)]
STREAMS = GENERATED + damaged()


# ------------------------------------------------------------------ x3_index_dev

@pytest.mark.parametrize("no_fast", [0, 1])
@pytest.mark.parametrize("n", zero_lengths())
def test_index_long_clean_chains(ctx, n, no_fast):
    """pointer doubling over 2^m - 1 .. 2^m + 1 candidates: (levels - 1) mod 4 = 0..3, several double4 launches"""
    check_index(ctx, R.zero_chain(n), no_fast)


@pytest.mark.parametrize("no_fast", [0, 1])
@pytest.mark.parametrize("name,make", STREAMS, ids=[n for n, _ in STREAMS])
def test_index_generated_and_damaged_streams(ctx, name, make, no_fast):
    check_index(ctx, make(), no_fast)


@pytest.mark.parametrize("no_fast", [0, 1])
def test_index_dense_stream_overflows_the_workgroups_and_rescans(x3, no_fast):
    """more than 384 key places and 256 candidates per workgroup span, more candidates than the first buffer: a new
    context (its buffer starts small) scans the stream twice, once"""
    c = x3.Context(0)
    try:
        case = R.dense()
        dl = check_index(c, case, no_fast)
        assert dl["index_rescans"] == 1
        assert c.get_option("last_index_candidates") > case.stream.size // 256 + 1024
        assert check_index(c, R.broken_header(case, 100), no_fast)["index_rescans"] == 0   # (the buffer has grown)
    finally:
        c.close()


@pytest.mark.parametrize("no_fast", [0, 1])
def test_index_max_frames_edge_on_a_long_chain(ctx, no_fast):
    n = 2 ** 17 + 1
    case = R.zero_chain(n)
    check_index(ctx, case, no_fast, max_frames=n)
    check_index(ctx, case, no_fast, max_frames=n - 1)


# ------------------------------------------------------------------ x3_decode_stream_dev

@pytest.mark.parametrize("two_trips", [0, 1])
@pytest.mark.parametrize("name,make", STREAMS + [("zeros4097", lambda: R.zero_chain(2 ** 12 + 1))],
                         ids=[n for n, _ in STREAMS] + ["zeros4097"])
def test_decode_stream_dev_generated_and_damaged(ctx, x3, name, make, two_trips):
    case = make()
    dl = check_decode(ctx, x3, case, two_trips)
    w = R.walk(case.stream)
    spf = case.params.block_len * case.params.blocks_per_frame
    one = (not two_trips and spf >= 2048 and is_clean(case, w)
           and w.n_frames <= R.one_trip_bound(1, case.stream.size) and not np.any(w.wav_off % 4))
    assert dl["stream_one_trip"] == (1 if one else 0), (case, dl)


@pytest.mark.parametrize("two_trips", [0, 1])
def test_decode_stream_dev_one_trip_bound(ctx, x3, two_trips):
    """306-byte frames at 2 060 samples: the one-trip decode is kept at and below the bound, thrown away above it"""
    from test_frame_walk_ref import quiet_counts
    lo, at, hi = quiet_counts()
    for n, kept in ((lo, True), (at, True), (hi, False)):
        dl = check_decode(ctx, x3, R.zero_chain(n, 103), two_trips)
        assert dl["stream_one_trip"] == (1 if kept and not two_trips else 0), (n, two_trips, dl)


@pytest.mark.parametrize("two_trips", [0, 1])
def test_decode_stream_dev_speculative_decode_over_false_headers(ctx, x3, two_trips):
    """the sparse stream's false headers (odd places, ~65 535 samples) are candidates the fast path writes into the frame
    table before it sees that the chain is not clean: the speculative decode runs over them, is thrown away, and writes
    nothing behind wav_cap -- with room for all their samples, and with wav_cap exactly the stream's samples"""
    case = R.sparse()
    for cap in (None, case.wav.size, case.wav.size + 3):
        assert check_decode(ctx, x3, case, two_trips, wav_cap=cap)["stream_one_trip"] == 0


@pytest.mark.parametrize("two_trips", [0, 1])
def test_decode_stream_dev_output_cut_at_frame_40000(ctx, x3, two_trips):
    check_decode(ctx, x3, R.zero_chain(100_000), two_trips, wav_cap=40_000 * 20 + 7)


@pytest.mark.parametrize("decode_blocks", [0, 1])
def test_decode_stream_dev_more_than_2_20_frames_takes_the_retry(ctx, x3, decode_blocks):
    n = 2 ** 20 + 1
    check_decode(ctx, x3, R.zero_chain(n), 0, wav_cap=20 * n, decode_blocks=decode_blocks)


# ------------------------------------------------------------------ host entry points

@pytest.mark.parametrize("make", [R.dense, R.sparse_long])
def test_host_decode_stream_of_4_to_16_mib(ctx, x3, make):
    """no options: the library walks a stream of this size on the GPU (the general path here); then the host walk and
    chunks of three frames"""
    case = make()
    assert 4 << 20 <= case.stream.size <= 16 << 20
    cap = case.wav.size + 65536
    want = O.decode_stream(case.stream, case.params, wav_cap=cap)
    ctx.set_option("index_no_fast", 0)
    for opt, val in ((None, None), ("host_walk", 1), ("host_chunk_frames", 3)):
        old = ctx.get_option(opt) if opt else None
        if opt:
            ctx.set_option(opt, val)
        try:
            before = counters(ctx)
            rc, wav, fok, ferr = ctx.decode_stream(case.stream, xparams(x3, case), wav_cap=cap)
            dl = delta(ctx, before)
        finally:
            if opt:
                ctx.set_option(opt, old)
        assert (rc, fok, ferr) == (want[0], want[2], want[3]), (case, opt)
        assert np.array_equal(wav, want[1]), (case, opt)
        if opt is None:
            assert dl["index_general_walks"] == 1, dl
            assert ctx.get_option("last_index_candidates") == R.scan(case.stream).size


def test_x3a_archive_cut_inside_the_phantom_bytes(ctx):
    """a 4-16 MiB archive whose last frame is a few bytes short: the reader believes in 8 bytes more than there are, so
    the GPU walk ends with Io"""
    case = R.dense()
    rc, head = O.archive_header_write(16000)
    assert rc == 0
    for cut in (1, 8):
        x3a = np.concatenate([head, case.stream[:case.stream.size - cut]])
        want = O.x3a_decode(x3a, wav_cap=case.wav.size + 65536)
        assert want[0] == R.IO
        got = ctx.x3a_decode(x3a, wav_cap=case.wav.size + 65536)
        assert got[0] == want[0] and got[2:] == want[2:], cut
        assert np.array_equal(got[1], want[1]), cut
