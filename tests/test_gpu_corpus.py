"""Corpus windows (include/x3hip.h, "CORPUS: windows of many streams"): x3_corpus_build / x3_corpus_windows_dev,
x3hip.Corpus and the C++ mirror.  Every row and status is held against the per-entry contract -- x3_decode_windows_dev on
a copy of the entry alone, its frames from x3_index_dev (archive entries: frame_walk_ref.walk with 8 phantom bytes) and its
sample offsets from x3_sample_offsets_dev -- and clean entries also against the oracle's decode of the entry, sliced.  The
bytes around d_out and d_status are canaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_walk_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 24
PAD = 256
CANARY = 0xA5


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _encode(ctx, wav):
    rc, s, _ = ctx.encode(wav)
    assert rc == 0
    return s


def _clips(x3, lengths, seed=1):
    return [x3.synth(2 + (i % 3), seed * 1000 + i, 0, n) for i, n in enumerate(lengths)]


def _frames(stream):
    offs = [0]
    while offs[-1] + 8 <= stream.size:
        nxt = offs[-1] + 20 + ((int(stream[offs[-1] + 6]) << 8) | int(stream[offs[-1] + 7]))
        if nxt > stream.size:
            break
        offs.append(nxt)
    return offs


def _place(entries, mode, rng):
    """one buffer holding every entry: back to back at even offsets, at odd ones, with gaps, overlapping, repeated"""
    blob, offs = bytearray(), []
    for e in entries:
        if mode == "even" and len(blob) & 1:
            blob += b"\0"
        elif mode == "odd" and not len(blob) & 1:
            blob += b"\x78"
        elif mode == "gaps":
            blob += bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
        offs.append(len(blob))
        blob += bytes(e)
    lens = [len(e) for e in entries]
    if mode == "overlap":
        offs2, lens2 = list(offs), list(lens)
        for o, n in zip(offs, lens):
            offs2 += [o, o + n // 2]
            lens2 += [n, n - n // 2]
        offs, lens = offs2, lens2
    return np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), offs, lens


def _contract(ctx, x3, entry, starts, L, fmt, p, archive=False):
    """x3_decode_windows_dev on a copy of the entry alone -> (rows, statuses, n_frames, n_samples)"""
    n = len(starts)
    zero = (np.zeros((n, L), dtype=np.float32 if fmt else np.int16), np.full(n, BAD, dtype=np.int32))
    entry = np.ascontiguousarray(entry, dtype=np.uint8)
    if archive:
        fo = R.walk(entry, phantom=8).frame_off
        if fo.size == 0:
            return zero + (0, 0)
        d_x3, d_fo = ctx.alloc(entry.size + 16), ctx.alloc(8 * (fo.size + 1))
        ctx.upload(d_x3, np.concatenate([entry, np.zeros(16, dtype=np.uint8)]))
        ctx.upload(d_fo, fo)
        try:
            ws = x3.WindowSource(ctx, (d_x3, entry.size), params=p, seg_blocks=0, frame_offsets=d_fo, n_frames=fo.size)
        except BaseException:
            ctx.free(d_x3)
            ctx.free(d_fo)
            raise
        ws._own += [d_x3, d_fo]
    else:
        # the entry's frames by x3_index_dev on a copy of it; only an entry without a frame has no stream to ask
        cap = entry.size // 20 + 2
        d_x3, d_fo, d_wo = ctx.alloc(entry.size + 16), ctx.alloc(8 * (cap + 1)), ctx.alloc(8 * cap)
        try:
            ctx.upload(d_x3, np.concatenate([entry, np.zeros(16, dtype=np.uint8)]))
            rc, nf, _, _ = ctx.index_dev(d_x3, entry.size, cap, d_fo, d_wo)
            assert rc == 0, ctx.last_error()
            if nf == 0:
                raise LookupError
            ws = x3.WindowSource(ctx, (d_x3, entry.size), params=p, seg_blocks=0, frame_offsets=d_fo, n_frames=nf)
        except BaseException as ex:
            for q in (d_x3, d_fo, d_wo):
                ctx.free(q)
            if isinstance(ex, LookupError):
                return zero + (0, 0)
            raise
        ws._own += [d_x3, d_fo, d_wo]
    try:
        rows, st = ws.decode(np.asarray(starts, dtype=np.uint64), L, fmt)
        return rows, st, ws.n_frames, ws.total
    finally:
        ws.close()


def _windows(corpus, entries, starts, L, fmt):
    """x3_corpus_windows_dev with canaries around d_out and d_status -> (rows, statuses, summary)"""
    ctx = corpus.ctx
    n = len(entries)
    esz = 4 if fmt else 2
    nbytes = esz * n * L
    d_e, d_s = ctx.alloc(4 * n), ctx.alloc(8 * n)
    d_out, d_st = ctx.alloc(nbytes + 2 * PAD), ctx.alloc(4 * n + 2 * PAD)
    try:
        ctx.upload(d_e, np.asarray(entries, dtype=np.uint32))
        ctx.upload(d_s, np.asarray(starts, dtype=np.uint64))
        ctx.upload(d_out, np.full(nbytes + 2 * PAD, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * n + 2 * PAD, CANARY, dtype=np.uint8))
        rc = corpus.decode_into(d_e, d_s, n, L, d_out + PAD, fmt, d_st + PAD)
        assert rc == 0, ctx.last_error()
        summary = ctx.decode_windows_result()
        assert summary[0] == 0
        raw = ctx.download(d_out, nbytes + 2 * PAD)
        rst = ctx.download(d_st, 4 * n + 2 * PAD)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + nbytes:] == CANARY).all(), "d_out written outside its rows"
        assert (rst[:PAD] == CANARY).all() and (rst[PAD + 4 * n:] == CANARY).all(), "d_status overrun"
        rows = raw[PAD:PAD + nbytes].view(np.float32 if fmt else np.int16).reshape(n, L)
        return rows, rst[PAD:PAD + 4 * n].view(np.int32), summary
    finally:
        for q in (d_e, d_s, d_out, d_st):
            ctx.free(q)


def _check_contract(ctx, x3, corpus, buf, offs, lens, wents, wstarts, L, fmt, p=None, archive=False, clips=None):
    """every window against the per-entry contract (grouped by entry), clean entries also against their clip"""
    rows, st, summary = _windows(corpus, wents, wstarts, L, fmt)
    wents, wstarts = np.asarray(wents), np.asarray(wstarts, dtype=np.uint64)
    bad = np.nonzero(st != 0)[0]
    assert summary[1:3] == (bad.size, int(bad[0]) if bad.size else len(wents))
    for e in np.unique(wents):
        sel = np.nonzero(wents == e)[0]
        if e >= len(offs):
            assert (st[sel] == BAD).all() and not rows[sel].any()
            continue
        entry = buf[offs[e]:offs[e] + lens[e]]
        want_rows, want_st, _, _ = _contract(ctx, x3, entry, wstarts[sel], L, fmt, p, archive)
        assert np.array_equal(st[sel], want_st), (e, st[sel], want_st)
        assert np.array_equal(rows[sel].view(np.uint16 if not fmt else np.uint32),
                              want_rows.view(np.uint16 if not fmt else np.uint32)), e
        if clips is not None and clips[e] is not None:
            for i in sel:
                s = int(wstarts[i])
                if st[i] == 0:
                    want = clips[e][s:s + L]
                    got = rows[i] if not fmt else np.round(rows[i] * 32768.0).astype(np.int16)
                    assert np.array_equal(got, want), (e, s)
    return rows, st


def _check_entries(corpus, buf, offs, lens, archive=False):
    for e, (o, n) in enumerate(zip(offs, lens)):
        w = R.walk(buf[o:o + n], phantom=8 if archive else 0)
        en = corpus.entries[e]
        assert (int(en["n_frames"]), int(en["walk_status"])) == (w.n_frames, w.terminal), (e, en, w)
        if e:
            prev = corpus.entries[e - 1]
            assert int(en["first_frame"]) == int(prev["first_frame"]) + int(prev["n_frames"])


def _draw(rng, corpus, k, L, extra_bad=True):
    ents, starts = [], []
    ns = corpus.entries["n_samples"].astype(np.int64)
    for _ in range(k):
        e = int(rng.integers(0, corpus.n_entries))
        top = int(ns[e]) - L
        s = int(rng.integers(0, top + 1)) if top >= 0 else int(rng.integers(0, 3))
        ents.append(e)
        starts.append(s)
    if extra_bad:
        ents += [corpus.n_entries, 0xFFFFFFFF, 0]
        starts += [0, 0, (1 << 64) - 5]
    return ents, starts


RAGGED = [0, 1, 9_999, 10_000, 10_001, 20_000, 33_333, 120_000]


@pytest.mark.parametrize("mode", ["even", "odd", "gaps", "overlap"])
def test_ragged_clean_corpora(ctx, x3, mode):
    clips = _clips(x3, RAGGED, seed=3)
    entries = [_encode(ctx, w) if w.size else np.zeros(0, dtype=np.uint8) for w in clips]
    buf, offs, lens = _place(entries, mode, np.random.default_rng(1))
    eclips = clips + ([None] * (len(offs) - len(clips)))
    for seg in (32, 0):
        corpus = x3.Corpus(ctx, buf[:-16], offs, lens, seg_blocks=seg)
        try:
            assert corpus.seg_blocks == seg
            _check_entries(corpus, buf, offs, lens)
            for e, w in enumerate(clips):
                assert int(corpus.entries[e]["n_samples"]) == w.size
            rng = np.random.default_rng(seg + len(mode))
            for fmt, L in ((0, 4_410), (1, 1_000)):
                ents, starts = _draw(rng, corpus, 48, L)
                _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, L, fmt, clips=eclips)
        finally:
            corpus.close()


def test_clips_written_back_to_back_by_encode_frames_dev(ctx, x3):
    """clips of one x3_encode_frames_dev call, one entry each: the fast walk vouches for every one"""
    lens_s = [12_345, 40_000, 1, 29_999, 70_001]
    clips = _clips(x3, lens_s, seed=4)
    wav = np.concatenate(clips)
    p = x3.Params.default()
    so, sn, first = [], [], []
    base = 0
    for w in clips:
        first.append(len(so))
        for a in range(0, w.size, 10_000):
            so.append(base + a)
            sn.append(min(10_000, w.size - a))
        base += w.size
    F = len(so)
    d_wav = ctx.alloc(2 * wav.size)
    cap = x3.lib().x3_encode_bound(wav.size, C.byref(p)) + 64 * F
    d_x3, d_off = ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    try:
        ctx.upload(d_wav, wav)
        assert ctx.encode_frames_dev(d_wav, so, sn, p, d_x3, cap, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        fo = ctx.download(d_off, 8 * (F + 1), np.uint64)
        offs = [int(fo[f]) for f in first]
        lens = [int(fo[f1]) - o for f1, o in zip(first[1:] + [F], offs)]
        buf = np.concatenate([ctx.download(d_x3, pos), np.zeros(16, dtype=np.uint8)])
        corpus = x3.Corpus(ctx, (d_x3, pos), offs, lens)
        try:
            assert corpus.n_frames == F and corpus.total_samples == wav.size
            assert not corpus.entries["general_walk"].any()
            _check_entries(corpus, buf, offs, lens)
            rng = np.random.default_rng(5)
            ents, starts = _draw(rng, corpus, 64, 2_000)
            _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, 2_000, 0, clips=clips)
        finally:
            corpus.close()
    finally:
        for q in (d_wav, d_x3, d_off):
            ctx.free(q)


def test_entry_edges(ctx, x3):
    clips = _clips(x3, [25_000, 1, 0, 18_000], seed=6)
    entries = [_encode(ctx, w) if w.size else np.zeros(0, dtype=np.uint8) for w in clips]
    entries.append(np.arange(300, dtype=np.uint8))      # bytes, no frame
    buf, offs, lens = _place(entries, "even", None)
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens)
    try:
        ns = corpus.entries["n_samples"]
        assert list(ns) == [25_000, 1, 0, 18_000, 0]
        L = 1_000
        ents = [0, 0, 0, 3, 1, 1, 2, 4, 5, 3, 0]
        starts = [25_000 - L, 25_000 - L + 1, 0, 18_000 - L, 0, 1, 0, 0, 0, (1 << 63), 24_999]
        rows, st = _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, L, 0, clips=clips + [None])
        assert st[0] == 0 and np.array_equal(rows[0], clips[0][-L:])        # ends exactly at n_samples
        assert st[1] == BAD and not rows[1].any()                           # one sample further: not the next entry's
        assert st[2] == 0 and st[3] == 0
        assert (st[4:] == BAD).all() and not rows[4:].any()
        rows, st = _check_contract(ctx, x3, corpus, buf, offs, lens, [1, 1], [0, 1], 1, 1, clips=clips + [None])
        assert list(st) == [0, BAD]                                          # the one-sample entry
    finally:
        corpus.close()


def _damaged(ctx, x3):
    clean = [_encode(ctx, w) for w in _clips(x3, [35_000, 42_000, 51_234, 38_000, 30_001, 44_444], seed=5)]
    out, clips = [clean[0]], [True]
    s = clean[1].copy()                       # a broken header mid-stream
    f = _frames(s)
    s[f[1] + 16] ^= 0x04
    out.append(s)
    s = clean[2].copy()                       # a payload CRC error
    f = _frames(s)
    s[f[2] + 40] ^= 0x10
    out.append(s)
    out.append(clean[3][:-7])                 # a truncated last frame
    s = clean[4]                              # junk in front
    out.append(np.concatenate([np.array([1, 2, 3, 0x78, 0x33, 9], dtype=np.uint8), s]))
    out.append(clean[5])
    return out, clean


def test_damaged_entries_and_damage_after_the_build(ctx, x3):
    entries, clean = _damaged(ctx, x3)
    buf, offs, lens = _place(entries, "even", None)
    d_x3 = ctx.alloc(buf.size)
    ctx.upload(d_x3, buf)
    corpus = x3.Corpus(ctx, (d_x3, buf.size - 16), offs, lens)
    try:
        _check_entries(corpus, buf, offs, lens)
        assert corpus.entries["general_walk"].any()
        rng = np.random.default_rng(8)
        L = 3_000
        ents = [e for e in range(len(offs)) for _ in range(6)]
        starts = [int(rng.integers(0, max(int(corpus.entries[e]["n_samples"]) - L, 0) + 1)) for e in ents]
        for fmt in (0, 1):
            _, st = _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, L, fmt)
        assert (st != 0).any()
        # damage after the build: a payload CRC error in clean entry 0, a broken header in entry 5; the windows give the
        # statuses of the damaged bytes, against the frame table of the build
        dam = buf.copy()
        f0 = _frames(entries[0])
        dam[offs[0] + f0[1] + 60] ^= 0x01
        f5 = _frames(entries[5])
        dam[offs[5] + f5[2] + 16] ^= 0x04
        ctx.upload(d_x3, dam)
        ents2 = [0] * 8 + [5] * 8
        starts2 = [int(s) for s in np.linspace(0, int(corpus.entries[0]["n_samples"]) - L, 8)] + \
                  [int(s) for s in np.linspace(0, int(corpus.entries[5]["n_samples"]) - L, 8)]
        rows, st, _ = _windows(corpus, ents2, starts2, L, 0)
        for e, sel in ((0, slice(0, 8)), (5, slice(8, 16))):
            want_rows, want_st, _, _ = _contract_with_frames(ctx, x3, dam[offs[e]:offs[e] + lens[e]],
                                                             buf[offs[e]:offs[e] + lens[e]], starts2[sel], L)
            assert np.array_equal(st[sel], want_st), (e, st[sel], want_st)
            assert np.array_equal(rows[sel], want_rows), e
        assert (st == 14).any() and (st == 13).any()
    finally:
        corpus.close()
        ctx.free(d_x3)


def _contract_with_frames(ctx, x3, entry, frames_of, starts, L):
    """the contract of bytes damaged after the build: the frames and sample offsets of the undamaged entry"""
    fo = R.walk(frames_of).frame_off
    d_x3, d_fo = ctx.alloc(entry.size + 16), ctx.alloc(8 * (fo.size + 1))
    ctx.upload(d_fo, fo)
    ctx.upload(d_x3, np.ascontiguousarray(frames_of))
    ws = x3.WindowSource(ctx, (d_x3, entry.size), seg_blocks=0, frame_offsets=d_fo, n_frames=fo.size)
    ws._own += [d_x3, d_fo]
    try:
        ctx.upload(d_x3, np.ascontiguousarray(entry))
        rows, st = ws.decode(np.asarray(starts, dtype=np.uint64), L, 0)
        return rows, st, ws.n_frames, ws.total
    finally:
        ws.close()


def test_archive_frames_and_from_archives(ctx, x3, tmp_path):
    clips = _clips(x3, [44_100, 12_345, 90_000, 1, 30_000], seed=9)
    archives = [ctx.x3a_encode(w, 44_100)[1] for w in clips]
    hs = [x3.archive_header_read(a)[4] for a in archives]
    parts = [a[8 + h:] for a, h in zip(archives, hs)]
    # one truncated into its phantom bytes, in front of another entry
    parts = [parts[0], parts[2][:-3], parts[1], parts[2][:-100], parts[3], parts[4]]
    buf, offs, lens = _place(parts, "odd", None)
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens, flags=x3.STREAMS_ARCHIVE_FRAMES)
    try:
        _check_entries(corpus, buf, offs, lens, archive=True)
        rng = np.random.default_rng(10)
        ents, starts = _draw(rng, corpus, 40, 2_000)
        ents += [1, 1]
        starts += [int(corpus.entries[1]["n_samples"]) - 2_000, int(corpus.entries[1]["n_samples"]) - 1_999]
        for fmt in (0, 1):
            _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, 2_000, fmt, archive=True)
    finally:
        corpus.close()
    # from_archives: bytes and paths, the input order, the oracle's x3a_decode sliced
    path = tmp_path / "a.x3a"
    path.write_bytes(bytes(archives[2]))
    corpus = x3.Corpus.from_archives(ctx, [archives[0], str(path), archives[1]])
    try:
        assert list(corpus.entries["n_samples"]) == [44_100, 90_000, 12_345]
        assert list(corpus.rates) == [44_100] * 3
        rows, st = corpus.decode([0, 1, 2, 1], [100, 86_000, 0, 0], 5_000)
        assert list(st) == [0, BAD, 0, 0]
        assert np.array_equal(rows[0], clips[0][100:5_100]) and np.array_equal(rows[2], clips[1][:5_000])
        assert np.array_equal(rows[3], clips[2][:5_000]) and not rows[1].any()
    finally:
        corpus.close()
    # an archive of another parameter set (block length 10): a corpus takes one
    rc, hdr = x3.archive_header_write(16_000, x3.Params.make(block_len=10))
    assert rc == 0
    rc, _, p_read, _, _ = x3.archive_header_read(np.concatenate([hdr, np.zeros(32, dtype=np.uint8)]))
    assert rc == 0 and p_read.block_len == 10 and bytes(p_read) != bytes(x3.Params.default())
    rc, frames, _ = O.encode(x3.synth(x3.SYNTH_WHITE, 3, 0, 36_000), O.Params.make(10, p_read.blocks_per_frame, (0, 1, 3)))
    assert rc == 0
    other = np.concatenate([hdr, frames])
    with pytest.raises(ValueError):
        x3.Corpus.from_archives(ctx, [archives[0], other])
    c10 = x3.Corpus.from_archives(ctx, [other, other])     # (by itself it is a corpus of its own)
    try:
        assert list(c10.entries["n_samples"]) == [36_000, 36_000] and c10.seg_blocks == 0
    finally:
        c10.close()


@pytest.mark.parametrize("bl,bpf,codes", [(10, 1000, (0, 1, 3)), (40, 250, (0, 1, 3)), (20, 100, (0, 1, 3)),
                                          (20, 500, (1, 1, 3))])
def test_parameter_sets(ctx, x3, bl, bpf, codes):
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    op = O.Params.make(bl, bpf, codes)
    clips = _clips(x3, [0, 1, 10_000, 19_999, 39_000, 40_000], seed=13)
    entries = []
    for w in clips:
        if w.size == 0:
            entries.append(np.zeros(0, dtype=np.uint8))
            continue
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        entries.append(s)
    buf, offs, lens = _place(entries, "gaps", np.random.default_rng(bl))
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens, params=p)
    try:
        records = bl == 20 and tuple(codes[1:]) == (1, 3)     # (the three-wave decoder: block length 20, codes 1 and 3 behind)
        assert corpus.seg_blocks == (32 if records else 0)
        _check_entries(corpus, buf, offs, lens)
        rng = np.random.default_rng(bl + bpf)
        for fmt in (0, 1):
            ents, starts = _draw(rng, corpus, 32, 3_000)
            _check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, 3_000, fmt, p=p, clips=clips)
    finally:
        corpus.close()


def test_scale_2000_clips_1024_windows(ctx, x3):
    """2 000 clips of 5-15 s at 44.1 kHz written by x3_encode_frames_dev, 1 024 random one-second windows, bit-exact; the
    recording decode takes several slices of its 256 MiB scratch"""
    rng = np.random.default_rng(2000)
    n_clips, spf = 2000, 10_000
    lens_s = rng.integers(5 * 44_100, 15 * 44_100 + 1, n_clips)
    base = np.concatenate([[0], np.cumsum(lens_s)]).astype(np.int64)
    total = int(base[-1])
    p = x3.Params.default()
    so, sn, first = [], [], []
    for c in range(n_clips):
        first.append(len(so))
        for a in range(0, int(lens_s[c]), spf):
            so.append(int(base[c]) + a)
            sn.append(min(spf, int(lens_s[c]) - a))
    F = len(so)
    d_wav = ctx.alloc(2 * total)
    cap = x3.lib().x3_encode_bound(total, C.byref(p)) + 64 * F
    d_x3, d_off = ctx.alloc(cap), ctx.alloc(8 * (F + 1))
    corpus = None
    try:
        ctx.synth_dev(x3.SYNTH_HYDROPHONE, 0x2000, 0, total, d_wav)
        assert ctx.encode_frames_dev(d_wav, so, sn, p, d_x3, cap, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        fo = ctx.download(d_off, 8 * (F + 1), np.uint64)
        offs = [int(fo[f]) for f in first]
        lens = [int(fo[f1]) - o for f1, o in zip(first[1:] + [F], offs)]
        corpus = x3.Corpus(ctx, (d_x3, pos), offs, lens)
        assert corpus.n_frames == F and corpus.total_samples == total and corpus.seg_blocks == 32
        assert ctx.get_option("last_corpus_record_slices") > 1
        # the sliced recording leaves what ONE recording call over the same table leaves (frames on the four-sample grid)
        ne = x3.lib().x3_seg_index_entries(F, C.byref(p), 32)
        assert corpus.seg_index_words == ne
        d_idx, d_back, d_woff = ctx.alloc(8 * ne), ctx.alloc(2 * F * spf), ctx.alloc(8 * F)
        try:
            ctx.upload(d_woff, np.arange(F, dtype=np.uint64) * np.uint64(spf))
            x4 = ctx.get_option("wav_offsets_x4")
            ctx.set_option("wav_offsets_x4", 1)
            try:
                assert ctx.decode_dev_seg(d_x3, pos, d_off, F, p, d_back, F * spf, d_idx, 32, record=True,
                                          d_wav_offsets=d_woff) == 0
                assert ctx.decode_result()[0] == 0
            finally:
                ctx.set_option("wav_offsets_x4", x4)
            assert ctx.get_option("last_seg_stretches") == -1          # (the call recorded)
            one = ctx.download(d_idx, 8 * ne, np.uint64)
            mine = ctx.download(corpus.d_seg_index, 8 * ne, np.uint64)
            assert (one[1:] != 0).any()
            assert np.array_equal(mine, one)
        finally:
            for q in (d_idx, d_back, d_woff):
                ctx.free(q)
        assert (corpus.entries["n_samples"] == lens_s).all() and not corpus.entries["general_walk"].any()
        L = 44_100
        ents = rng.integers(0, n_clips, 1024)
        starts = np.array([int(rng.integers(0, int(lens_s[e]) - L + 1)) for e in ents], dtype=np.uint64)
        for fmt in (0, 1):
            rows, st, summary = _windows(corpus, ents, starts, L, fmt)
            assert summary[1] == 0 and not st.any()
            assert ctx.get_option("last_window_replays") == 0         # (every stretch ended where the index said)
            for i in range(0, 1024, 1):
                want = ctx.download(d_wav + 2 * (int(base[ents[i]]) + int(starts[i])), 2 * L, np.int16)
                got = rows[i] if not fmt else np.round(rows[i] * 32768.0).astype(np.int16)
                assert np.array_equal(got, want), i
    finally:
        if corpus is not None:
            corpus.close()
        for q in (d_wav, d_x3, d_off):
            ctx.free(q)


def test_more_windows_than_the_plan_grid_has_threads(ctx, x3):
    """2^20 + 4 099 windows of one sample: the plan grid is capped at 4 096 groups of 256 threads, and every window past
    them gets its plan too -- corpus and single-stream calls alike; statuses, rows and canaries"""
    clips = _clips(x3, [30_000, 25_001], seed=21)
    entries = [_encode(ctx, w) for w in clips]
    buf, offs, lens = _place(entries, "odd", None)
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens)
    n = (1 << 20) + 4099
    rng = np.random.default_rng(21)
    ents = rng.integers(0, 3, n).astype(np.uint32)                  # entry 2 is past the corpus
    starts = rng.integers(0, 30_001, n).astype(np.uint64)            # past some entries' ends too
    try:
        rows, st, summary = _windows(corpus, ents, starts, 1, 0)
        ns = np.array([30_000, 25_001, 0], dtype=np.uint64)
        ok = (ents < 2) & (starts < ns[np.minimum(ents, 2)])
        assert np.array_equal(st == 0, ok) and (st[~ok] == BAD).all()
        assert summary[1] == int((~ok).sum())
        want = np.zeros(n, dtype=np.int16)
        for e in (0, 1):
            sel = ok & (ents == e)
            want[sel] = clips[e][starts[sel].astype(np.int64)]
        assert np.array_equal(rows[:, 0], want)
        assert ok[1 << 20:].any() and (~ok[1 << 20:]).any()
    finally:
        corpus.close()
    # x3_decode_windows_dev through the same launcher: the stream of clip 0
    ws = x3.WindowSource(ctx, entries[0], seg_blocks=32)
    d_s, d_out, d_st = ctx.alloc(8 * n), ctx.alloc(2 * n + 2 * PAD), ctx.alloc(4 * n + 2 * PAD)
    try:
        ctx.upload(d_s, starts)
        ctx.upload(d_out, np.full(2 * n + 2 * PAD, CANARY, dtype=np.uint8))
        ctx.upload(d_st, np.full(4 * n + 2 * PAD, CANARY, dtype=np.uint8))
        assert ws.decode_into(d_s, n, 1, d_out + PAD, 0, d_st + PAD) == 0
        assert ctx.decode_windows_result()[0] == 0
        raw, rst = ctx.download(d_out, 2 * n + 2 * PAD), ctx.download(d_st, 4 * n + 2 * PAD)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + 2 * n:] == CANARY).all()
        assert (rst[:PAD] == CANARY).all() and (rst[PAD + 4 * n:] == CANARY).all()
        ok = starts < 30_000
        assert np.array_equal(rst[PAD:PAD + 4 * n].view(np.int32) == 0, ok)
        want = np.where(ok, clips[0][np.minimum(starts, 29_999).astype(np.int64)], 0).astype(np.int16)
        assert np.array_equal(raw[PAD:PAD + 2 * n].view(np.int16), want)
    finally:
        for q in (d_s, d_out, d_st):
            ctx.free(q)
        ws.close()


def test_state_argument_errors_and_a_pending_decode(ctx, x3):
    wav = x3.synth(2, 5, 0, 30_000)
    s = _encode(ctx, wav)
    buf = np.concatenate([s, np.zeros(16, dtype=np.uint8)])
    corpus = x3.Corpus(ctx, buf[:-16], [0, 0], [s.size, s.size])
    L = x3.lib()
    d_e, d_s = ctx.alloc(64), ctx.alloc(64)
    d_out, d_st = ctx.alloc(4 * 4 * 1000 + 64), ctx.alloc(64)
    d_fo, d_wav = ctx.alloc(8 * 8), ctx.alloc(2 * 30_000)
    try:
        ctx.upload(d_e, np.array([0, 1, 2, 0], dtype=np.uint32))
        ctx.upload(d_s, np.array([0, 100, 0, 29_000], dtype=np.uint64))

        def call(k=corpus._h, ents=d_e, starts=d_s, n=4, wl=1000, out=d_out, fmt=0, st=d_st):
            return L.x3_corpus_windows_dev(ctx._h, k, ents, starts, n, wl, out, fmt, st)
        # an earlier windows call's result survives every refused call
        assert call() == 0
        for bad in (dict(k=None), dict(ents=None), dict(ents=d_e + 2), dict(starts=d_s + 4), dict(n=0), dict(wl=0),
                    dict(fmt=2), dict(out=d_out + 1), dict(out=d_out + 2, fmt=1), dict(st=d_st + 2), dict(st=None)):
            assert call(**bad) == BAD, bad
        rc, n_bad, first_bad, first_status = ctx.decode_windows_result()
        assert (rc, n_bad, first_bad, first_status) == (0, 1, 2, BAD)
        assert ctx.decode_windows_result()[0] == BAD       # (taken)
        # a pending x3_decode_dev is left alone by a corpus windows call
        fo = np.array(_frames(s)[:-1], dtype=np.uint64)
        ctx.upload(d_fo, fo)
        assert ctx.decode_dev(corpus.d_x3, s.size, d_fo, fo.size, x3.Params.default(), d_wav, 30_000, n_per_clip=30_000) == 0
        assert call() == 0
        assert ctx.decode_ranges_result()[0] == BAD        # (the pending call is a windows call, and stays pending)
        assert ctx.decode_windows_result()[0] == 0
        rc, first_bad, _, _ = ctx.decode_result()
        assert (rc, first_bad) == (0, fo.size)
        assert np.array_equal(ctx.download(d_wav, 60_000, np.int16), wav)
        assert call(n=2) == 0 and ctx.decode_windows_result() == (0, 0, 2, 0)      # none bad: the count, status 0
        # build refusals
        p = x3.Params.default()
        offs = np.array([0], dtype=np.uint64)
        lens = np.array([s.size], dtype=np.uint64)
        h = C.c_void_p(0)

        def build(d_x3=corpus.d_x3, x3_len=s.size, o=offs, ln=lens, n=1, flags=0, params=p, seg=32):
            return L.x3_corpus_build(ctx._h, d_x3, x3_len, o.ctypes.data, ln.ctypes.data, n, flags, C.byref(params), seg,
                                     C.byref(h))
        for bad in (dict(n=0), dict(flags=2), dict(d_x3=corpus.d_x3 + 2), dict(params=x3.Params.make(codes=(0, 1, 4))),
                    dict(seg=30), dict(seg=3204), dict(ln=np.array([s.size + 1], dtype=np.uint64)),
                    dict(o=np.array([s.size + 1], dtype=np.uint64), ln=np.array([0], dtype=np.uint64))):
            assert build(**bad) == BAD, bad
            assert not h.value
        assert build() == 0 and h.value
        L.x3_corpus_destroy(h)
    finally:
        corpus.close()
        for q in (d_e, d_s, d_out, d_st, d_fo, d_wav):
            ctx.free(q)


def test_x3_hpp_corpus(tmp_path):
    """tests/host_cpp/test_corpus_hpp.cpp: device::Corpus of the C++ mirror"""
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_corpus_hpp.cpp")
    exe = str(tmp_path / "test_corpus_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
