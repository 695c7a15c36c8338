"""The frame walk restated in plain Python, a scanner of every valid header, and seeded generators of long, dense and
adversarial streams (tests/test_frame_walk_ref.py pins them on the CPU, tests/test_gpu_frame_walk.py holds the GPU walk to
them).

The walk is X3aReader::decode_next_frame (decodefile.rs:105-136) over decoder::read_frame_header (decoder.rs:69-118), with
the rules the library states in x3i_kind and x3_index_finalize_kernel: at most 20 bytes left -> done; a header that does
not validate -> its error; a payload past the bytes the reader believes in -> quiet stop; past the real end but inside the
believed end -> Io; payload_len > 24 576 -> FrameHeaderInvalidPayloadLen; samples == 0, payload_len < 2, a frame past
wav_cap or (block length 0) more than one sample -> pushed, then BAD_ARG.  The header CRC is the oracle's crc16
(crc16_rows is a vectorised copy of it, pinned against it)."""
import functools

import numpy as np

import oracle_lib as O

OK, IO, FRAME_LENGTH, INVALID_KEY, INVALID_PAYLOAD_LEN, INVALID_HEADER_CRC, MORE_THAN_ONE_CHANNEL, BAD_ARG = \
    0, 1, 10, 11, 12, 13, 6, 24
CONT, LAST_BAD, QUIET, PLEN, KIND_IO = 0, 1, 2, 3, 4      # what the walk does with a valid header (x3i_kind)
KIND_NAMES = {"cont": CONT, "merge": CONT, "last_bad": LAST_BAD, "quiet": QUIET, "plen": PLEN}
READ_BUFFER = 24576
MAX_LENGTH = 0x7FE0
KEY = (0x78, 0x33)


# ------------------------------------------------------------------ CRC (CRC-16/CCITT, init 0xFFFF, as the oracle's)

def _crc_table():
    t = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) if c & 0x8000 else (c << 1)
        t[i] = c & 0xFFFF
    return t


_T = _crc_table()


def crc16_rows(rows):
    """CRC of every row of a (n, m) uint8 array -> (n,) uint32"""
    rows = np.asarray(rows, dtype=np.uint8)
    crc = np.full(rows.shape[0], 0xFFFF, dtype=np.uint32)
    for j in range(rows.shape[1]):
        crc = ((crc << 8) & 0xFFFF) ^ _T[((crc >> 8) ^ rows[:, j]) & 0xFF]
    return crc


def _crc16_py(data):
    c = 0xFFFF
    for x in data:
        c = ((c << 8) & 0xFFFF) ^ int(_T[((c >> 8) ^ x) & 0xFF])
    return c


@functools.lru_cache(maxsize=None)
def _solver(pos):
    """inv[v] = the value d of bytes pos, pos+1 (big-endian) that adds v to the CRC of a 16-byte header (CRC-16 is affine:
    crc(x ^ d) = crc(x) ^ crc(d) ^ crc(0), and 16 contiguous bits reach every value)"""
    rows = np.zeros((65536, 16), dtype=np.uint8)
    d = np.arange(65536, dtype=np.uint32)
    rows[:, pos], rows[:, pos + 1] = d >> 8, d & 0xFF
    delta = crc16_rows(rows) ^ _crc16_py(bytes(16))
    inv = np.zeros(65536, dtype=np.uint32)
    inv[delta] = d
    assert np.unique(delta).size == 65536
    return inv


def _solve(h16, pos, target):
    """set bytes pos, pos+1 of the 16-byte bytearray h16 so that its CRC is `target`"""
    h16[pos] = h16[pos + 1] = 0
    d = int(_solver(pos)[_crc16_py(h16) ^ target])
    h16[pos], h16[pos + 1] = d >> 8, d & 0xFF


# ------------------------------------------------------------------ headers, scanner, walk

def header_status(stream, off):
    """decoder::read_frame_header at `off` (20 bytes there): -> (status, samples, payload_len), checks in its order"""
    h = stream[off:off + 20]
    samples, plen = int(h[4]) << 8 | int(h[5]), int(h[6]) << 8 | int(h[7])
    if O.crc16(h[:16]) != (int(h[16]) << 8 | int(h[17])):
        return INVALID_HEADER_CRC, samples, plen
    if (int(h[0]), int(h[1])) != KEY:
        return INVALID_KEY, samples, plen
    if h[3] > 1:
        return MORE_THAN_ONE_CHANNEL, samples, plen
    if plen >= MAX_LENGTH:
        return FRAME_LENGTH, samples, plen
    return OK, samples, plen


def kind_of(length, believed, off, plen, samples, bl0=False):
    """x3i_kind: what the walk does with a VALID header at `off`"""
    if believed - off - 20 < plen:
        return QUIET
    if plen > READ_BUFFER:
        return PLEN
    if length - off - 20 < plen:
        return KIND_IO
    if samples == 0 or plen < 2 or (bl0 and samples > 1):
        return LAST_BAD
    return CONT


def _valid_rows(b, offs):
    rows = b[offs[:, None] + np.arange(20)]
    plen = rows[:, 6].astype(np.uint32) << 8 | rows[:, 7]
    ok = crc16_rows(rows[:, :16]) == (rows[:, 16].astype(np.uint32) << 8 | rows[:, 17])
    ok &= (rows[:, 0] == KEY[0]) & (rows[:, 1] == KEY[1]) & (rows[:, 3] <= 1) & (plen < MAX_LENGTH)
    return ok


def scan(stream):
    """byte offsets of every valid header (20 bytes inside the stream) -- what the candidate kernel must find"""
    b = np.ascontiguousarray(stream, dtype=np.uint8)
    if b.size < 20:
        return np.zeros(0, dtype=np.int64)
    offs = np.nonzero((b[:-1] == KEY[0]) & (b[1:] == KEY[1]))[0].astype(np.int64)
    offs = offs[offs + 20 <= b.size]
    return offs[_valid_rows(b, offs)] if offs.size else offs


class Walk:
    def __init__(self, frame_off, wav_off, n_samples, terminal):
        self.frame_off = np.asarray(frame_off, dtype=np.uint64)
        self.wav_off = np.asarray(wav_off, dtype=np.uint64)
        self.n_frames = len(self.frame_off)
        self.n_samples = n_samples
        self.terminal = terminal

    def __repr__(self):
        return "Walk(n_frames=%d, n_samples=%d, terminal=%d)" % (self.n_frames, self.n_samples, self.terminal)


def walk(stream, phantom=0, wav_cap=None, bl0=False):
    """the reference's walk from offset 0.  -> Walk: the pushed frames' byte offsets and exclusive sample offsets, their
    number, the samples of the frames the walk steps over, and how it ends.  (Headers are read without their CRC on the
    way and validated in one batch behind it; the walk is cut at the first that fails -- the same walk.)"""
    b = np.ascontiguousarray(stream, dtype=np.uint8)
    raw = b.tobytes()
    length, believed = len(raw), len(raw) + phantom
    cap = (1 << 64) - 1 if wav_cap is None else wav_cap
    offs, woffs = [], []
    pos = nsamp = 0
    terminal = OK
    while True:
        if believed - pos <= 20:
            break
        if length - pos < 20:
            terminal = IO
            break
        samples, plen = raw[pos + 4] << 8 | raw[pos + 5], raw[pos + 6] << 8 | raw[pos + 7]
        if plen >= MAX_LENGTH or raw[pos + 3] > 1 or raw[pos] != KEY[0] or raw[pos + 1] != KEY[1]:
            offs.append(pos)   # (invalid for sure: the batch below finds it and reports its error)
            woffs.append(nsamp)
            break
        k = kind_of(length, believed, pos, plen, samples, bl0)
        if k == QUIET:
            offs.append(pos)
            woffs.append(nsamp)
            terminal = -QUIET
            break
        if k in (PLEN, KIND_IO):
            offs.append(pos)
            woffs.append(nsamp)
            terminal = -k
            break
        offs.append(pos)
        woffs.append(nsamp)
        if k == LAST_BAD or nsamp + samples > cap:
            terminal = -LAST_BAD
            break
        nsamp += samples
        pos += 20 + plen
    # validate every header the walk read, in one batch; the walk ends at the first invalid one
    offs_a = np.asarray(offs, dtype=np.int64)
    ok = _valid_rows(b, offs_a) if offs_a.size else np.zeros(0, dtype=bool)
    bad = np.nonzero(~ok)[0]
    if bad.size:
        j = int(bad[0])
        st = header_status(b, offs[j])[0]
        assert st != OK
        return Walk(offs[:j], woffs[:j], woffs[j], st)
    if terminal == OK:
        return Walk(offs, woffs, nsamp, OK)
    if terminal == -LAST_BAD:
        return Walk(offs, woffs, nsamp, BAD_ARG)
    # the last header read is valid and not a frame: QUIET -> OK, PLEN, IO
    st = {-QUIET: OK, -PLEN: INVALID_PAYLOAD_LEN, -KIND_IO: IO}[terminal]
    return Walk(offs[:-1], woffs[:-1], nsamp, st)


# ------------------------------------------------------------------ streams

class Case:
    """a generated stream: bytes, parameters, expected samples (None: not known), planted false headers [(off, kind)]"""

    def __init__(self, name, stream, params, wav=None, planted=(), phantom=0):
        self.name, self.stream, self.params, self.wav = name, stream, params, wav
        self.planted, self.phantom = list(planted), phantom

    def __repr__(self):
        return "Case(%s, %d bytes)" % (self.name, self.stream.size)


def frame_offsets(stream):
    offs, pos = [], 0
    while pos + 20 <= len(stream):
        offs.append(pos)
        pos += 20 + (int(stream[pos + 6]) << 8 | int(stream[pos + 7]))
    return offs


def noise(n, seed, sd=20):
    return np.round(np.random.default_rng(seed).normal(0, sd, n)).astype(np.int16)


def encode(wav, params=None):
    rc, s, _ = O.encode(wav, params)
    assert rc == 0
    return s


def _refresh(s, off):
    plen = int(s[off + 6]) << 8 | int(s[off + 7])
    pc = O.crc16(s[off + 20:off + 20 + plen])
    s[off + 18], s[off + 19] = pc >> 8, pc & 0xFF
    hc = O.crc16(s[off:off + 16])
    s[off + 16], s[off + 17] = hc >> 8, hc & 0xFF


def with_tails(stream, tail_lens, fill, rng):
    """every frame's payload gains tail_lens[f] bytes behind its last block (random, then fill(buf, t0, t1, next_off,
    is_last, rng) -> [(off, kind)] plants what it likes in [t0, t1)); payload_len and both CRCs follow.  -> (stream,
    planted)"""
    offs = frame_offsets(stream)
    ends = offs[1:] + [len(stream)]
    size = len(stream) + int(sum(tail_lens))
    out = np.frombuffer(rng.bytes(size), dtype=np.uint8).copy()
    spans, pos = [], 0
    for f, (a, e) in enumerate(zip(offs, ends)):
        n = e - a
        out[pos:pos + n] = stream[a:e]
        plen = n - 20 + int(tail_lens[f])
        assert plen <= READ_BUFFER
        out[pos + 6], out[pos + 7] = plen >> 8, plen & 0xFF
        spans.append((pos, pos + n, pos + n + int(tail_lens[f])))
        pos += n + int(tail_lens[f])
    planted = []
    for f, (h, t0, t1) in enumerate(spans):
        if fill is not None and t1 > t0:
            planted += fill(out, t0, t1, t1, f == len(spans) - 1, rng)
    for h, _, _ in spans:
        _refresh(out, h)
    return out, planted


def _put_fields(buf, o, ident, ch, samples, plen):
    buf[o], buf[o + 1] = KEY
    buf[o + 2], buf[o + 3] = ident, ch
    buf[o + 4], buf[o + 5] = samples >> 8, samples & 0xFF
    buf[o + 6], buf[o + 7] = plen >> 8, plen & 0xFF


def dense_fill(kinds):
    """a run of valid headers eight bytes apart over the whole tail: header B at A + 8 has A's time field as its key, id,
    channels, samples and length and A's header CRC as its time bytes 0-1, so every header CRC is "x3" -- the key of
    the header two places on.  Built front to back: B's samples are solved so that A's CRC comes out right.  `kinds`
    cycles over "cont" (to a later header of the run), "merge" (to the next real frame), "last_bad", "plen" and "quiet"
    (where the stream's end allows; "last_bad" where not)."""
    def fill(buf, t0, t1, next_off, is_last, rng):
        n = (t1 - t0 - 20) // 8 + 1
        if n < 2:
            return []
        end = len(buf)
        fields = []        # (ident, ch, plen, kind) of header i
        for i in range(n + 1):
            o = t0 + 8 * i
            want = kinds[i % len(kinds)] if i < n else None
            plen, kind = int(rng.integers(0, 0x7FE0)), None
            if want == "cont" and n - 1 - i >= 3:
                m = int(rng.integers(3, min(n - 1 - i, 40) + 1))
                plen, kind = 8 * m - 20, "cont"
            elif want == "merge" and next_off - o - 20 >= 2:
                plen, kind = next_off - o - 20, "merge"
            elif want == "plen" and end - o - 20 >= MAX_LENGTH:
                plen, kind = int(rng.integers(READ_BUFFER + 1, MAX_LENGTH)), "plen"
            elif want == "quiet" and end - o - 20 < MAX_LENGTH - 1:
                plen, kind = int(rng.integers(end - o - 20 + 1, MAX_LENGTH)), "quiet"
            elif want is not None:
                plen, kind = int(rng.integers(0, 2)), "last_bad"
            fields.append((int(rng.integers(0, 256)), int(rng.integers(0, 2)), plen, kind))
        i0, c0, p0, _ = fields[0]
        _put_fields(buf, t0, i0, c0, int(rng.integers(1, 65536)), p0)
        planted = []
        for i in range(n):
            o = t0 + 8 * i
            ident, ch, plen, kind = fields[i + 1]
            while True:
                _put_fields(buf, o + 8, ident, ch, 0, plen)
                h = bytearray(buf[o:o + 16].tobytes())
                _solve(h, 12, 0x7833)          # bytes 12-13 of A = B's samples
                s = h[12] << 8 | h[13]
                if s or kind in (None, "last_bad"):
                    break
                ident = (ident + 1) & 0xFF
            buf[o + 12], buf[o + 13] = h[12], h[13]
            buf[o + 16], buf[o + 17] = KEY      # A's header CRC (= the key of the header at A + 16)
            planted.append((o, fields[i][3]))
        buf[t0 + 8 * (n + 1)], buf[t0 + 8 * (n + 1) + 1] = KEY
        return planted
    return fill


def sparse_fill(buf, t0, t1, next_off, is_last, rng):
    """one false header per tail, at an odd or even place, samples near 65 535, continuing to the next real frame"""
    o = int(rng.integers(t0, t1 - 22 + 1))
    plen = next_off - o - 20
    if plen < 2:
        return []
    _put_fields(buf, o, int(rng.integers(0, 256)), 1, 65535 - int(rng.integers(0, 16)), plen)
    h = bytearray(buf[o:o + 16].tobytes())
    _solve(h, 8, int(buf[o + 16]) << 8 | int(buf[o + 17]))     # time bytes 0-1 carry the CRC
    buf[o + 8], buf[o + 9] = h[8], h[9]
    return [(o, "merge")]


@functools.lru_cache(maxsize=None)
def padded(seed=1, n_samples=50_000, pad=4000):
    """real frames whose payloads end in `pad` random bytes: decodes to the unpadded samples"""
    wav = noise(n_samples, seed)
    s0 = encode(wav)
    s, _ = with_tails(s0, [pad] * len(frame_offsets(s0)), None, np.random.default_rng(seed))
    return Case("padded", s, O.Params.default(), wav)


@functools.lru_cache(maxsize=None)
def odd_tails(seed=2, n_samples=200_000):
    """tails of odd and even lengths: real frames start at odd offsets"""
    wav = noise(n_samples, seed, 60)
    s0 = encode(wav)
    rng = np.random.default_rng(seed)
    tails = [int(2 * rng.integers(0, 300) + (f & 1)) for f in range(len(frame_offsets(s0)))]
    s, _ = with_tails(s0, tails, None, rng)
    return Case("odd_tails", s, O.Params.default(), wav)


DENSE_KINDS = ("cont", "merge", "cont", "last_bad", "cont", "plen", "merge", "quiet")


@functools.lru_cache(maxsize=None)
def dense(seed=3, n_samples=2_600_000, tail_min=6000, tail_max=14000):
    """dense false headers (512 per 4 KiB) in every frame's tail; ~6 MiB: the GPU walk's general path and, from the host,
    x3_decode_stream's GPU walk"""
    wav = noise(n_samples, seed)
    s0 = encode(wav)
    rng = np.random.default_rng(seed)
    tails = [int(rng.integers(tail_min, tail_max + 1)) for _ in frame_offsets(s0)]
    s, planted = with_tails(s0, tails, dense_fill(DENSE_KINDS), rng)
    return Case("dense", s, O.Params.default(), wav, planted)


@functools.lru_cache(maxsize=None)
def sparse(seed=4, n_samples=300_000):
    """one false header per frame tail (odd places, ~65 535 samples): few enough that the one-trip decode runs over them"""
    wav = noise(n_samples, seed)
    s0 = encode(wav)
    rng = np.random.default_rng(seed)
    tails = [int(rng.integers(40, 400)) for _ in frame_offsets(s0)]
    s, planted = with_tails(s0, tails, sparse_fill, rng)
    return Case("sparse", s, O.Params.default(), wav, planted)


@functools.lru_cache(maxsize=None)
def sparse_long(seed=5, n_samples=5_000_000):
    """the sparse kind at 4-16 MiB (host x3_decode_stream picks the GPU walk there)"""
    c = sparse(seed, n_samples)
    return Case("sparse_long", c.stream, c.params, c.wav, c.planted)


@functools.lru_cache(maxsize=None)
def _zero_frame(bpf):
    p = O.Params.make(blocks_per_frame=bpf)
    s = encode(np.zeros(20 * bpf, dtype=np.int16), p)
    assert len(frame_offsets(s)) == 1
    return s, p


def zero_chain(n, bpf=1):
    """n frames of zeros at block length 20, bpf blocks a frame (26 bytes a frame at 1, 306 at 103)"""
    f, p = _zero_frame(bpf)
    return Case("zeros%dx%d" % (bpf, n), np.tile(f, n), p, np.zeros(20 * bpf * n, dtype=np.int16))


def one_trip_bound(frame_bytes, n):
    """x3_decode_stream_dev's one-trip bound for n frames of frame_bytes each: len / 1024 + 64"""
    return n * frame_bytes // 1024 + 64


# ------------------------------------------------------------------ damage

def junk_front(case, n=37, seed=9):
    """random bytes in front: the walk ends at offset 0 with that header's error"""
    j = np.frombuffer(np.random.default_rng(seed).bytes(n), dtype=np.uint8)
    return Case(case.name + "+junk", np.concatenate([j, case.stream]), case.params, None,
                [(o + n, k) for o, k in case.planted])


def broken_header(case, frame):
    """one bit of frame `frame`'s header flipped (its CRC fails): the walk ends there"""
    s = case.stream.copy()
    s[frame_offsets(s)[frame] + 5] ^= 0x10
    return Case(case.name + "+broken%d" % frame, s, case.params, None, case.planted)


def lead_in(case, target):
    """a valid header at offset 0 whose payload is the stream's first `target` bytes: the walk steps from it onto the
    (false) header at `target` and follows whatever chain that one starts -- through false headers into the real ones"""
    s = np.concatenate([np.zeros(20, dtype=np.uint8), case.stream])
    _put_fields(s, 0, 7, 1, 1000, target)
    _refresh(s, 0)
    return Case(case.name + "+lead%d" % target, s, case.params, None, [(o + 20, k) for o, k in case.planted])


def truncated(case, cut):
    """the last `cut` bytes gone: the last frame's payload runs past the end"""
    return Case(case.name + "-%d" % cut, case.stream[:len(case.stream) - cut].copy(), case.params, None, case.planted)
