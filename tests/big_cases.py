"""A stream of more than 2^32 bytes and more than 2^32 samples, tiled from a few tiles that the CPU oracle encodes, with an
exact reference for every sample, offset and level record of it (not a test module: tests/test_big_cases.py proves it on the
CPU at four places, tests/test_gpu_beyond_4gib.py holds the device calls to it at the full size).

A TILE is 64 frames of 10 000 samples at the default parameters: quiet frames, ordinary ones and dense ones (full-scale
noise, a payload of about 20 KB: more than the 9 728-byte image, less than the reader's 24 576).  A frame's bytes depend on
its own samples only -- the header carries no counter and a frame is an even number of bytes -- so tiles laid back to back in
any order are one valid chain of frames.  PLACE m of the stream holds tile kind[m].  The table alternates tiles 0 and 1;
tile 2 stands at the place that holds byte 2^32 and at the place that holds sample position 2^32, tile 3 (with frames louder
than any other tile has) at the last place: an access that wraps modulo 2^32 lands on other content.

Everything a test needs is closed-form in kind[] and the tiles: the bytes of any span, the samples of any span, the frame
and sample offset tables, and the level records of every bin at any bin length that divides a tile, for the samples, for
their first difference and for a FIR-filtered signal (fir(): seams between places included, the history taken from the
last frame of the tile in front), at any phase of the bins against the tiles.  Damage is one flipped bit in chosen frames;
the reference then follows the contract (include/x3hip.h): a failed frame adds nothing to levels, takes both of its seams
with it in the first difference and the T - 1 positions behind it in a FIR signal of T taps, and leaves zeros from its
first sample on in a window.  Tone records are NOT periodic in the places -- the phase of position i is (i * step) mod
2^32 -- so tone_records walks the samples of a slice; the whole stream is compared on the device."""
import numpy as np

import diff_levels_ref as DR
import fir_levels_ref as FL
import levels_ref as LR
import oracle_lib as O
import ranges_ref as RR
import tone_levels_ref as TL

SPF, FPT = 10000, 64                  # samples a frame, frames a tile
TS = SPF * FPT                        # samples a tile
EDGE, MARGIN = 1 << 32, 1 << 27       # both totals exceed EDGE + MARGIN
MAX_BYTES = 6_000_000_000
IMAGE, READER = 9728, 24576           # the wave encoder's image, the reader's limit (payload bytes)
SAMPLES, DIFF = DR.SAMPLES, DR.DIFF
BAD_ARG = RR.ERR_BAD_ARG
LOUD_MEAN_SQ = 600_000_000            # only tile 3 has bins of 10 000 samples above this mean square
QUIET, ORDINARY, DENSE, LOUD = range(4)
FIR_HIST = 7                          # X3L_FIR_HIST: a FIR value reaches at most so many samples back


def fir(taps, shift=0):
    """the `signal` of a FIR-filtered signal (fir_levels_ref's contract): hashable, so that it keys the records' cache"""
    assert FL.check(taps, shift)
    return ("fir", tuple(int(c) for c in taps), int(shift))


# eight taps of mixed signs and a shift: a gain of 323 / 256, so full-scale noise clamps at some positions and not at most
FIR8 = fir((-12, 50, -90, 70, 30, -40, 25, -6), 8)
FIR_DIFF = fir((1, -1))               # x[i] - x[i - 1]: DIFF's records wherever both count a position


def is_fir(signal):
    return isinstance(signal, tuple) and signal[0] == "fir"


def _signal_levels(frames, st, so, bin_len, n_bins, signal):
    """the records of the three kinds of signal over frames at sample offsets so"""
    if is_fir(signal):
        return FL.fir_levels(frames, st, so, bin_len, n_bins, signal[1], signal[2])
    return DR.signal_levels(frames, st, so, bin_len, n_bins, signal)


def tone_records_of(x, counted, pos0, bin_len, step, tab=None):
    """the x3_tone_level records of samples x at the absolute positions pos0 .. pos0 + len(x) - 1 (those with counted False add
    nothing), bins of bin_len counted from pos0, a last one of fewer positions included.  The phase is by absolute position:
    pair ((i mod 2^32) * step mod 2^32) >> 22, in uint64 whose product stays below 2^64 -- never a wrapped int64 product"""
    assert 0 <= step <= 0xFFFFFFFF and pos0 >= 0 and bin_len > 0
    tab = (TL.table() if tab is None else np.asarray(tab, dtype=np.int16).reshape(TL.PAIRS, 2)).astype(np.int64)
    n = len(x)
    pos = (np.arange(n, dtype=np.uint64) + np.uint64(pos0 % EDGE)) & np.uint64(EDGE - 1)      # i mod 2^32, exact
    k = (((pos * np.uint64(step)) & np.uint64(EDGE - 1)) >> np.uint64(22)).astype(np.int64)
    x = np.asarray(x, dtype=np.int64)
    out = TL.empty(max(1, -(-n // bin_len)) if n else 0)
    for j in range(out.size):
        s = slice(j * bin_len, min((j + 1) * bin_len, n))
        ok = np.asarray(counted[s], dtype=bool)
        v, kk = x[s][ok], k[s][ok]
        if v.size:
            out[j] = (int(np.sum(v * tab[kk, 0])), int(np.sum(v * tab[kk, 1])), v.min(), v.max(), v.size, 0)
    return out


class Tile:
    """64 frames: .wav int16 [TS], .frame_kind [64], .stream (the oracle's bytes), .fo (65 byte offsets), .nbytes"""

    def __init__(self, seed, loud=False, block_len=20):
        rng = np.random.default_rng(seed)
        fk = np.array([DENSE] * 24 + [ORDINARY] * 28 + [QUIET] * 12)
        rng.shuffle(fk)
        if loud:
            fk[rng.choice(FPT, size=8, replace=False)] = LOUD
        wav = np.zeros(TS, dtype=np.int16)
        for f, k in enumerate(fk):
            w = wav[f * SPF:(f + 1) * SPF]
            if k == DENSE:
                w[:] = rng.integers(-32768, 32768, size=SPF)
            elif k == ORDINARY:
                w[:] = np.round(rng.normal(0, (3, 6, 10)[f % 3], SPF) + 300 * np.sin(np.arange(SPF) * 0.01 * (1 + f % 5)))
            elif k == QUIET:
                w[:] = rng.integers(-2, 3, size=SPF) if f % 2 else 0
            else:   # a full-scale square wave of random period: mean square near 1e9, three times white noise's
                w[:] = np.where((np.arange(SPF) // int(rng.integers(3, 40))) % 2, 32000, -32000) + rng.integers(-700, 700, size=SPF)
        self.wav, self.frame_kind = wav, fk
        rc, self.stream, _ = O.encode(wav, O.Params.make(block_len, SPF // block_len))
        assert rc == 0
        self.fo = np.array(RR.frame_offsets(self.stream), dtype=np.int64)
        assert self.fo.size == FPT + 1 and self.fo[-1] == self.stream.size and not np.any(self.fo % 2)
        self.nbytes = int(self.stream.size)
        plen = np.diff(self.fo) - 20
        assert np.all(plen[fk >= DENSE] > IMAGE) and np.all(plen[fk < DENSE] <= IMAGE) and plen.max() < READER
        self.frames = [wav[f * SPF:(f + 1) * SPF] for f in range(FPT)]


SEEDS = (0x4B1, 0x4B2, 0x4B3, 0x4B4)
_TILES, _RECORDS = {}, {}


def tiles(block_len=20):
    """the four tiles, encoded with blocks of block_len samples (cached: they are never written to)"""
    if block_len not in _TILES:
        _TILES[block_len] = [Tile(s, loud=(i == 3), block_len=block_len) for i, s in enumerate(SEEDS)]
        for t in _TILES[block_len]:
            t.wav.setflags(write=False)
            t.stream.setflags(write=False)
    return _TILES[block_len]


def _kinds(M, tb):
    """kind[] of M places for tiles of tb bytes: 0, 1 alternating, tile 3 last, tile 2 at the two places that hold 2^32"""
    kind = np.arange(M) % 2
    if M >= 2:
        kind[-1] = 3
    ms = EDGE // TS
    if ms < M - 1:
        kind[ms] = 2
    elif M >= 3:
        kind[1] = 2            # (a short stream: tile 2 still occurs, between two other tiles)
    mb = None
    for _ in range(8):         # (tile 2's own length may move byte 2^32 out of the place: repeat to the fixed point)
        off = np.concatenate([[0], np.cumsum(tb[kind])])
        if off[-1] <= EDGE:
            break
        m = int(np.searchsorted(off, EDGE, side="right")) - 1
        if kind[m] == 2 or m == M - 1:
            break
        if mb is not None and mb != ms:
            kind[mb] = mb % 2
        mb = m
        kind[m] = 2
    return kind


def place_count(tb):
    """the smallest number of places at which bytes and samples both exceed EDGE + MARGIN"""
    M = (EDGE + MARGIN) // TS + 1
    while int(tb[_kinds(M, tb)].sum()) <= EDGE + MARGIN:
        M += max(1, (EDGE + MARGIN - int(tb[_kinds(M, tb)].sum())) // int(tb.max()))
    return M


def merge(recs):
    """the merge of level records (x3_events_dev's): sums added (n modulo 2^32), min and max taken"""
    out = LR.empty(1)
    if len(recs):
        out["sum_sq"] = np.sum(recs["sum_sq"], dtype=np.uint64)
        out["sum"] = np.sum(recs["sum"], dtype=np.int64)
        out["n"] = np.uint32(int(np.sum(recs["n"], dtype=np.uint64)) & 0xFFFFFFFF)
        out["min"], out["max"] = recs["min"].min(), recs["max"].max()
    return out


class Case:
    """the tiled stream of n_places places (None: the full size), its tiles encoded at block_len"""

    def __init__(self, n_places=None, block_len=20):
        self.tiles, self.block_len = tiles(block_len), block_len
        self.tb = np.array([t.nbytes for t in self.tiles], dtype=np.int64)
        self.tfo = np.stack([t.fo for t in self.tiles])
        self.full = n_places is None
        self.M = place_count(self.tb) if self.full else int(n_places)
        self.kind = _kinds(self.M, self.tb)
        self.place_off = np.concatenate([[0], np.cumsum(self.tb[self.kind])]).astype(np.int64)
        self.total_bytes, self.total = int(self.place_off[-1]), self.M * TS
        self.F = self.M * FPT
        self.bad = {}          # global frame -> the oracle's status
        self.flips = []        # (byte offset in the stream, xor mask)
        self._cache = _RECORDS             # (the records depend on the samples alone, and a key names all it depends on)
        if self.full:
            assert self.total_bytes > EDGE + MARGIN and self.total > EDGE + MARGIN and self.total_bytes <= MAX_BYTES
            assert all(modulo_conditions(self).values()), modulo_conditions(self)
            mb, ms = self.place_of_byte(EDGE), EDGE // TS
            for m in (mb, ms, self.M - 1):
                assert self.kind[m] >= 2 and self.kind[m - 1] != self.kind[m] and (m == self.M - 1 or self.kind[m + 1] != self.kind[m])
            assert np.all(self.kind[:ms + 1] != 3)       # (the loud tile lies above sample 2^32 only)

    # ---- where things are
    def place_of_byte(self, b):
        return int(np.searchsorted(self.place_off, b, side="right")) - 1

    def frame_of_byte(self, b):
        m = self.place_of_byte(b)
        return m * FPT + int(np.searchsorted(self.tfo[self.kind[m]], b - int(self.place_off[m]), side="right")) - 1

    def frame_offsets(self):
        """uint64 [F + 1]: byte offset of every frame, the total last"""
        fo = (self.place_off[:-1, None] + self.tfo[self.kind][:, :FPT]).ravel()
        return np.concatenate([fo, [self.total_bytes]]).astype(np.uint64)

    def sample_offsets(self):
        return np.arange(self.F + 1, dtype=np.uint64) * np.uint64(SPF)

    def frame_span(self, f):
        """byte range [a, b) of global frame f"""
        m, i = divmod(f, FPT)
        t = self.tfo[self.kind[m]]
        return int(self.place_off[m] + t[i]), int(self.place_off[m] + t[i + 1])

    # ---- bytes and samples of a span
    def stream_bytes(self, b0, b1):
        """bytes [b0, b1) of the stream, damage included"""
        out = np.empty(b1 - b0, dtype=np.uint8)
        for m in range(self.place_of_byte(b0), self.place_of_byte(max(b1 - 1, b0)) + 1):
            o = int(self.place_off[m])
            a, b = max(b0, o), min(b1, int(self.place_off[m + 1]))
            out[a - b0:b - b0] = self.tiles[self.kind[m]].stream[a - o:b - o]
        for pos, mask in self.flips:
            if b0 <= pos < b1:
                out[pos - b0] ^= mask
        return out

    def samples(self, g0, g1):
        """the samples at positions [g0, g1) of the undamaged signal"""
        out = np.empty(g1 - g0, dtype=np.int16)
        for m in range(g0 // TS, (max(g1 - 1, g0)) // TS + 1):
            a, b = max(g0, m * TS), min(g1, (m + 1) * TS)
            out[a - g0:b - g0] = self.tiles[self.kind[m]].wav[a - m * TS:b - m * TS]
        return out

    def first_bad(self, f0, f1):
        """the first damaged frame in [f0, f1) and its status, or (None, 0)"""
        hit = [f for f in self.bad if f0 <= f < f1]
        return (min(hit), self.bad[min(hit)]) if hit else (None, 0)

    def window(self, start, length):
        """x3_decode_windows_dev's row and status for the window (start, length)"""
        if start > self.total or length > self.total - start:
            return np.zeros(length, dtype=np.int16), BAD_ARG
        if length == 0:
            return np.zeros(0, dtype=np.int16), 0
        row = self.samples(start, start + length)
        f, st = self.first_bad(start // SPF, (start + length - 1) // SPF + 1)
        if f is not None:
            row[max(0, f * SPF - start):] = 0
        return row, st

    def signal_values(self, g0, g1, signal):
        """what positions [g0, g1) add to level records: (values int64, counted bool)"""
        pos = np.arange(g0, g1, dtype=np.int64)
        good = np.ones(self.F, dtype=bool)
        good[np.array(sorted(self.bad), dtype=np.int64)] = False
        fr = pos // SPF
        if signal == SAMPLES:
            return self.samples(g0, g1).astype(np.int64), good[fr]
        if is_fir(signal):     # (the T positions i - T + 1 .. i lie in at most two frames: T - 1 < SPF)
            _, taps, shift = signal
            T = len(taps)
            x = np.concatenate([np.zeros(T - 1, dtype=np.int64), self.samples(max(g0 - (T - 1), 0), g1).astype(np.int64)])
            x = x[x.size - (g1 - g0) - (T - 1):]                 # x[j + T - 1 - t] is the sample at position g0 + j - t
            acc = sum(int(c) * x[T - 1 - t:x.size - t] for t, c in enumerate(taps))
            ok = (pos >= T - 1) & good[fr] & good[np.maximum(pos - (T - 1), 0) // SPF]
            return np.clip(acc >> shift, -32768, 32767), ok
        x = self.samples(max(g0 - 1, 0), g1).astype(np.int64)
        if g0 == 0:
            x = np.concatenate([[0], x])
        seam = pos % SPF == 0
        ok = good[fr] & (~seam | ((pos > 0) & good[np.maximum(fr - 1, 0)]))
        return np.clip(x[1:] - x[:-1], -32768, 32767), ok

    def record_of(self, g0, g1, signal):
        """the one level record of positions [g0, g1), straight from the samples"""
        v, ok = self.signal_values(g0, g1, signal)
        v = v[ok]
        out = LR.empty(1)
        if v.size:
            out["n"], out["sum"], out["sum_sq"] = v.size, v.sum(), np.sum((v * v).astype(np.uint64), dtype=np.uint64)
            out["min"], out["max"] = v.min(), v.max()
        return out

    def tone_records(self, g0, g1, bin_len, step, tab=None):
        """the x3_tone_level records of positions [g0, g1): bins of bin_len counted from g0 (a last one of fewer positions
        included), a failed frame adds nothing, the phase by absolute position.  For slices: it walks the samples"""
        good = np.ones(self.F, dtype=bool)
        good[np.array(sorted(self.bad), dtype=np.int64)] = False
        return tone_records_of(self.samples(g0, g1), good[np.arange(g0, g1, dtype=np.int64) // SPF], g0, bin_len, step, tab)

    # ---- damage
    def damage(self, frames, where="payload", bit=3):
        """flip one bit in each (place, frame in tile): of the payload's middle byte, or of the header's sample count.
        -> the statuses the oracle gives those frames"""
        out = []
        for m, i in frames:
            f = m * FPT + i
            a, b = self.frame_span(f)
            pos = a + (20 + (b - a - 20) // 2 if where == "payload" else 5)
            self.flips.append((pos, 1 << bit))
            fb = self.stream_bytes(a, b)
            st = RR.frames_of(fb, [0, fb.size])[0][0]
            assert st != 0
            self.bad[f] = st
            out.append(st)
        return out

    # ---- level records
    def _bad_of(self, m):
        return tuple(sorted((f - m * FPT, st) for f, st in self.bad.items() if f // FPT == m))

    def _place_records(self, key):
        """the nb records whose bins begin in a place: bins of bin_len from `phase` samples into it.  key = (bin_len, phase,
        signal, tile in front or None, its damage, the place's tile, its damage, the next tile or None, its damage)"""
        if key in self._cache:
            return self._cache[key]
        bin_len, phase, signal, p, bad_p, c, bad_c, n, bad_n = key
        frames, st = [], []
        if p is None:
            frames.append(np.zeros(0, dtype=np.int16))     # (no sample in front of the stream: no seam)
            st.append(0)
        else:
            frames.append(self.tiles[p].frames[-1])
            st.append(dict(bad_p).get(FPT - 1, 0))
        lead = len(frames[0])
        frames += self.tiles[c].frames
        st += [dict(bad_c).get(i, 0) for i in range(FPT)]
        if n is not None:
            k = -(-phase // SPF)
            frames += self.tiles[n].frames[:k]
            st += [dict(bad_n).get(i, 0) for i in range(k)]
        shift = (-(lead + phase)) % bin_len                 # the place's sample `phase` falls on a bin boundary
        so = np.concatenate([[0], np.cumsum([len(w) for w in frames])])[:-1] + shift
        b0, nb = (lead + phase + shift) // bin_len, TS // bin_len
        # (a FIR value reaches FIR_HIST < SPF samples back: the one frame in front carries all the history a place needs)
        rec = _signal_levels(frames, st, so, bin_len, b0 + nb, signal)[b0:]
        self._cache[key] = rec
        return rec

    def records(self, bin_len, signal=SAMPLES, phase=0, places=None):
        """the records of the bins [m * TS + phase + j * bin_len, ... + bin_len) that begin in places [m0, m1) (all of them
        by default), TS // bin_len a place; bin_len divides TS, 0 <= phase < bin_len"""
        assert bin_len > 0 and TS % bin_len == 0 and 0 <= phase < bin_len
        m0, m1 = places or (0, self.M)
        keys, idx = {}, np.empty(m1 - m0, dtype=np.int64)
        for m in range(m0, m1):
            p, n = (self.kind[m - 1] if m else None), (self.kind[m + 1] if m + 1 < self.M else None)
            key = (bin_len, phase, signal, p, self._bad_of(m - 1) if m else (), int(self.kind[m]), self._bad_of(m),
                   n, self._bad_of(m + 1) if n is not None else ())
            key = tuple(int(v) if isinstance(v, np.integer) else v for v in key)
            idx[m - m0] = keys.setdefault(key, len(keys))
        table = np.stack([self._place_records(k) for k in keys])
        return table[idx].reshape(-1)

    def levels(self, bin_len, n_bins=None, signal=SAMPLES):
        """x3_signal_levels_dev's records: n_bins of them (default: as many as cover the stream); bin_len 0: one bin"""
        if bin_len == 0:
            return merge(self.records(TS, signal))
        rec = self.records(bin_len, signal)
        if n_bins is None or n_bins == rec.size:
            return rec
        return rec[:n_bins] if n_bins < rec.size else np.concatenate([rec, LR.empty(n_bins - rec.size)])

    def range_status(self, start, length):
        if start > self.total or length > self.total - start:
            return BAD_ARG
        return self.first_bad(start // SPF, (start + length - 1) // SPF + 1)[1] if length else 0

    def range_levels(self, start, length, bin_len, signal=SAMPLES):
        """x3_signal_range_levels_dev's records of the range (start, length): bins counted from `start`; bin_len divides TS"""
        rows = max(1, -(-length // bin_len))
        if self.range_status(start, length) == BAD_ARG or length == 0:
            return LR.empty(rows)
        phase, full = start % bin_len, length // bin_len
        m0 = (start - phase) // TS
        m1 = min(self.M, (start + full * bin_len - 1) // TS + 1) if full else m0
        parts = []
        if full:
            i0 = (start - phase - m0 * TS) // bin_len
            parts.append(self.records(bin_len, signal, phase, (m0, m1))[i0:i0 + full])
            assert parts[0].size == full
        if length % bin_len:
            parts.append(self.record_of(start + full * bin_len, start + length, signal))
        return np.concatenate(parts)


def modulo_conditions(case):
    """what keeps a wrap modulo 2^32 from passing by accident: 2^32 modulo each tile's byte length is no frame boundary of
    that tile, and 2^32 modulo the tile's sample count is not 0"""
    out = {"samples": EDGE % TS != 0}
    for k, t in enumerate(case.tiles):
        out["tile %d" % k] = int(EDGE % t.nbytes) not in set(t.fo.tolist())
    return out
