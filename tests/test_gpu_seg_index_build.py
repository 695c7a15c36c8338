"""x3_seg_index_build_dev (include/x3hip.h): the segment index of any stream by a walk that stores no sample, and
x3_corpus_build's X3_CORPUS_INDEX_WALK.  Bit-exact, no tolerances:

  1. on block length 20 it equals, word for word, what x3_encode_dev_seg fills and what a recording decode leaves;
  2. for other block lengths it equals seg_index_ref's index from the CPU oracle, with every entry a frame has valid;
  3. the consumers believe it: windows by it give the oracle's samples with last_window_replays == 0 (a wrong entry is
     contradicted by a stretch and shows up there);
  4. a corpus built with the flag has an index for every parameter set;
  5. hostile bytes, offsets and headers under guard pages: no fault, same windows as without an index;
  6. 200 trials of tools/fuzz_parity.py's family x."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import oracle_lib as O
import seg_index_ref as S
import test_gpu_corpus as TC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD = 24
POISON = 0xDEADBEEFDEADBEEF
ORACLE_SETS = [(10, 1000), (40, 250), (13, 300), (20, 100), (60, 50)]


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture()
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def _mixed(x3, n, seed, spf):
    """hydrophone noise with every third frame loud (BFP and literal blocks)"""
    wav = x3.synth(x3.SYNTH_HYDROPHONE, seed, 0, n)
    for f in range(1, n // spf, 3):
        wav[spf * f:spf * (f + 1)] = x3.synth(x3.SYNTH_WHITE, seed + f, 0, spf)
    return wav


def _build(ctx, x3, d_x3, x3_len, d_off, F, p, sb):
    """-> (the index's words, last_seg_index_irregular), the buffer poisoned first: every word must be written"""
    ne = x3.lib().x3_seg_index_entries(F, C.byref(p), sb)
    assert ne > 0
    d_idx = ctx.alloc(8 * ne + 64)
    try:
        ctx.upload(d_idx, np.full(ne + 8, POISON, dtype=np.uint64))
        assert ctx.seg_index_build_dev(d_x3, x3_len, d_off, F, p, d_idx, sb) == 0, ctx.last_error()
        irregular = ctx.get_option("last_seg_index_irregular")
        raw = ctx.download(d_idx, 8 * ne + 64, np.uint64)
        assert (raw[ne:] == np.uint64(POISON)).all(), "written behind the index"
        return raw[:ne].copy(), irregular
    finally:
        ctx.free(d_idx)


def _on_device(ctx, stream, offs):
    d_x3, d_off = ctx.alloc(stream.size + 16), ctx.alloc(8 * (len(offs) + 1))
    ctx.upload(d_x3, np.concatenate([stream, np.zeros(16, dtype=np.uint8)]))
    ctx.upload(d_off, np.array(list(offs) + [stream.size], dtype=np.uint64))
    return d_x3, d_off


# ---- 1. equals what exists
@pytest.mark.parametrize("sb", [32, 64, 128])
def test_equals_the_encoders_index_and_the_recorded_one(ctx, x3, sb):
    """the stream of test_the_encoders_index_is_the_one_a_serial_decode_records: quiet, every seventh frame loud, a short
    last frame; all three indexes are the same words, word 0 included"""
    p = x3.Params.default()
    n = 1_234_567
    wav = x3.synth(2, 77 + sb, 0, n)
    for f in range(3, n // 10000, 7):
        wav[10000 * f:10000 * (f + 1)] = x3.synth(1, 500 + f, 0, 10000)
    L = x3.lib()
    F = L.x3_num_frames(n, C.byref(p)); cap = L.x3_encode_bound(n, C.byref(p))
    ne = L.x3_seg_index_entries(F, C.byref(p), sb)
    d_wav = ctx.alloc(2 * n + 64); d_out = ctx.alloc(cap + 16); d_off = ctx.alloc(8 * (F + 1)); d_back = ctx.alloc(2 * n)
    d_enc = ctx.alloc(8 * ne); d_rec = ctx.alloc(8 * ne)
    try:
        ctx.upload(d_wav, wav)
        ctx.upload(d_enc, np.full(ne, POISON, dtype=np.uint64))
        ctx.upload(d_rec, np.zeros(ne, dtype=np.uint64))
        assert ctx.encode_dev_seg(d_wav, n, p, d_out, cap, d_enc, sb, 0, d_off) == 0
        rc, pos, _ = ctx.encode_result()
        assert rc == 0
        assert ctx.decode_dev_seg(d_out, pos, d_off, F, p, d_back, n, d_rec, sb, record=True, n_per_clip=n) == 0
        assert ctx.decode_result() == (0, F, 0, n)
        enc, rec = ctx.download(d_enc, 8 * ne, np.uint64), ctx.download(d_rec, 8 * ne, np.uint64)
        mine, irregular = _build(ctx, x3, d_out, pos, d_off, F, p, sb)
        assert irregular == 0
        assert int(mine[0]) == S.SEG_MAGIC | (sb << 32)
        assert np.array_equal(mine, rec), np.flatnonzero(mine != rec)[:10]
        assert np.array_equal(mine, enc), np.flatnonzero(mine != enc)[:10]
        assert (mine[1:] != 0).sum() > F                     # (and it is an index, not two empty ones)
    finally:
        for q in (d_wav, d_out, d_off, d_back, d_enc, d_rec):
            ctx.free(q)


@pytest.mark.parametrize("sb", [32, 64, 128])
def test_equals_the_recorded_index_on_codes_1_1_3(ctx, x3, sb):
    """(the decoders read blocks of type 1 with code 0 whatever the parameters say, as the reference does: threshold 0
    keeps the encoder from writing any on this content, so that the stream decodes)"""
    p = x3.Params.make(20, 500, (1, 1, 3), (0, 8, 20))
    n = 20 * 500 * 9 + 4_568
    wav = _mixed(x3, n, 31 + sb, 10_000)
    rc, stream, _ = O.encode(wav, O.Params.make(20, 500, (1, 1, 3), (0, 8, 20)))
    assert rc == 0
    offs = S.frames(stream)[:-1]
    F = len(offs)
    ne = x3.lib().x3_seg_index_entries(F, C.byref(p), sb)
    d_x3, d_off = _on_device(ctx, stream, offs)
    d_back, d_rec = ctx.alloc(2 * n), ctx.alloc(8 * ne)
    try:
        ctx.upload(d_rec, np.zeros(ne, dtype=np.uint64))
        assert ctx.decode_dev_seg(d_x3, stream.size, d_off, F, p, d_back, n, d_rec, sb, record=True, n_per_clip=n) == 0
        assert ctx.decode_result() == (0, F, 0, n) and ctx.get_option("last_seg_stretches") == -1
        rec = ctx.download(d_rec, 8 * ne, np.uint64)
        mine, irregular = _build(ctx, x3, d_x3, stream.size, d_off, F, p, sb)
        assert irregular == 0 and np.array_equal(mine, rec), np.flatnonzero(mine != rec)[:10]
        assert (mine[1:] != 0).any()
    finally:
        for q in (d_x3, d_off, d_back, d_rec):
            ctx.free(q)


# ---- 2. equals the oracle
@pytest.mark.parametrize("bl,bpf", ORACLE_SETS)
@pytest.mark.parametrize("sb", [4, 32])
def test_equals_the_oracles_index(ctx, x3, bl, bpf, sb):
    """word for word; every entry in front of a block the frame has is valid, none was given up"""
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf), O.Params.make(bl, bpf, (0, 1, 3))
    n = spf * 7 + spf // 3 + 1
    wav = _mixed(x3, n, 1000 * bl + sb, spf)
    rc, stream, _ = O.encode(wav, op)
    assert rc == 0
    offs = S.frames(stream)[:-1]
    want, expect = S.build(stream, offs, op, sb)
    d_x3, d_off = _on_device(ctx, stream, offs)
    try:
        mine, irregular = _build(ctx, x3, d_x3, stream.size, d_off, len(offs), p, sb)
    finally:
        ctx.free(d_x3); ctx.free(d_off)
    assert irregular == 0
    assert np.array_equal(mine, want), np.flatnonzero(mine != want)[:10]
    ns = S.n_seg(op, sb)
    valid = ((mine[1:] >> np.uint64(48)) & np.uint64(1)).reshape(len(offs), ns - 1)
    for f, off in enumerate(offs):
        samples, _ = S.header(stream, off)
        nbf = (samples - 1 + bl - 1) // bl
        assert [j for j in range(1, ns) if valid[f, j - 1]] == [j for j in range(1, ns) if sb * j < nbf], f
    assert sum(expect) == int(valid.sum()) > 0


# ---- 3. the consumer believes it
def _windows_by_the_walk(ctx, x3, p, stream, wav, sb=32):
    """x3_decode_windows_dev by a walk-built index over the stream alone: the input's samples, no status, no replay"""
    ws = x3.WindowSource(ctx, stream, p, seg_blocks=sb, index="walk")
    try:
        assert ws.seg_blocks == sb and ws.d_seg_index is not None and ws.total == wav.size
        assert ctx.get_option("last_seg_index_irregular") == 0
        rng = np.random.default_rng(wav.size)
        for fmt in (0, 1):
            L = 3_000
            starts = np.concatenate([[0, wav.size - L], rng.integers(0, wav.size - L + 1, 30)]).astype(np.uint64)
            rows, st = ws.decode(starts, L, fmt)
            assert not st.any()
            assert ctx.get_option("last_window_replays") == 0
            for i, s in enumerate(starts):
                got = rows[i] if not fmt else np.round(rows[i] * 32768.0).astype(np.int16)
                assert np.array_equal(got, wav[int(s):int(s) + L]), (fmt, i)
    finally:
        ws.close()


def _corpus_windows_by_the_walk(ctx, x3, p, entries, clips, archive=False, sb=32):
    buf, offs, lens = TC._place(entries, "gaps", np.random.default_rng(7))
    flags = x3.STREAMS_ARCHIVE_FRAMES if archive else 0
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens, params=p, flags=flags, seg_blocks=sb, index="walk")
    try:
        assert corpus.seg_blocks == sb and ctx.get_option("last_seg_index_irregular") == 0
        rng = np.random.default_rng(len(entries))
        for fmt in (0, 1):
            L = 3_000
            ents, starts = TC._draw(rng, corpus, 32, L, extra_bad=False)
            rows, st, summary = TC._windows(corpus, ents, starts, L, fmt)
            assert not st.any() and summary[1] == 0
            assert ctx.get_option("last_window_replays") == 0
            for i, (e, s) in enumerate(zip(ents, starts)):
                got = rows[i] if not fmt else np.round(rows[i] * 32768.0).astype(np.int16)
                assert np.array_equal(got, clips[e][s:s + L]), (fmt, i)
    finally:
        corpus.close()


@pytest.mark.parametrize("bl,bpf", ORACLE_SETS)
def test_windows_by_the_built_index_need_no_replay(ctx, x3, bl, bpf):
    spf = bl * bpf
    p, op = x3.Params.make(bl, bpf), O.Params.make(bl, bpf, (0, 1, 3))
    clips = [_mixed(x3, spf * 5 + 17 * k + 1, 50 * bl + k, spf) for k in range(3)]
    entries = []
    for w in clips:
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        entries.append(s)
    _windows_by_the_walk(ctx, x3, p, entries[0], clips[0])
    _corpus_windows_by_the_walk(ctx, x3, p, entries, clips)


def test_windows_of_a_tuned_archive(ctx, x3):
    """what the project's own tuner writes: an archive at a block length other than 20 gets an index"""
    for seed in range(40, 60):
        wav = x3.synth(x3.SYNTH_HYDROPHONE, seed, 0, 150_000)
        rc, arc, _, p = ctx.x3a_encode_tuned(wav, 16_000)
        assert rc == 0
        if p.block_len != 20:
            break
    assert p.block_len != 20, "the tuner chose block length 20 for every seed"
    rc, _, p_read, _, hs = x3.archive_header_read(arc)
    assert rc == 0 and p_read.block_len == p.block_len
    _windows_by_the_walk(ctx, x3, p_read, arc[8 + hs:], wav)      # (the parameters a reader of the archive has)
    corpus = x3.Corpus.from_archives(ctx, [arc, arc], index="walk")
    try:
        assert corpus.seg_blocks == 32 and ctx.get_option("last_corpus_record_slices") == 0
        rng = np.random.default_rng(3)
        for fmt in (0, 1):
            ents, starts = TC._draw(rng, corpus, 32, 16_000, extra_bad=False)
            rows, st, summary = TC._windows(corpus, ents, starts, 16_000, fmt)
            assert not st.any() and ctx.get_option("last_window_replays") == 0
            for i, s in enumerate(starts):
                got = rows[i] if not fmt else np.round(rows[i] * 32768.0).astype(np.int16)
                assert np.array_equal(got, wav[s:s + 16_000]), (fmt, i)
    finally:
        corpus.close()
    # the same archives without the option: today's behaviour, no index off block length 20
    plain = x3.Corpus.from_archives(ctx, [arc, arc])
    try:
        assert plain.seg_blocks == 0 and plain.d_seg_index is None
    finally:
        plain.close()


# ---- 4. corpus
@pytest.mark.parametrize("bl,bpf,codes", [(10, 1000, (0, 1, 3)), (40, 250, (0, 1, 3)), (20, 100, (0, 1, 3)),
                                          (20, 500, (1, 1, 3))])
def test_corpus_parameter_sets_with_the_walk(ctx, x3, bl, bpf, codes):
    """test_gpu_corpus.py::test_parameter_sets' corpora, built with X3_CORPUS_INDEX_WALK"""
    p = x3.Params.make(block_len=bl, blocks_per_frame=bpf, codes=codes)
    op = O.Params.make(bl, bpf, codes)
    clips = TC._clips(x3, [0, 1, 10_000, 19_999, 39_000, 40_000], seed=13)
    entries = []
    for w in clips:
        if w.size == 0:
            entries.append(np.zeros(0, dtype=np.uint8))
            continue
        rc, s, _ = O.encode(w, op)
        assert rc == 0
        entries.append(s)
    buf, offs, lens = TC._place(entries, "gaps", np.random.default_rng(bl))
    records = bl == 20 and tuple(codes[1:]) == (1, 3)
    plain = x3.Corpus(ctx, buf[:-16], offs, lens, params=p)
    try:
        assert plain.seg_blocks == (32 if records else 0)            # (without the flag: as before)
        plain_idx = ctx.download(plain.d_seg_index, 8 * plain.seg_index_words, np.uint64) if records else None
    finally:
        plain.close()
    corpus = x3.Corpus(ctx, buf[:-16], offs, lens, params=p, index="walk")
    try:
        assert corpus.seg_blocks == 32
        assert ctx.get_option("last_corpus_record_slices") == 0
        # (codes (1, 1, 3) at the default thresholds: the encoder writes blocks of type 1 with code 1 and every decoder reads
        # them with code 0, as the reference does -- frames of these clips fail to decode, and their walks stop there)
        clean = tuple(codes) == (0, 1, 3)
        assert clean == (ctx.get_option("last_seg_index_irregular") == 0)
        assert corpus.seg_index_words == x3.lib().x3_seg_index_entries(corpus.n_frames, C.byref(p), 32)
        mine = ctx.download(corpus.d_seg_index, 8 * corpus.seg_index_words, np.uint64)
        assert (mine[1:] != 0).any()
        if records:
            # The recorded index, frame by frame.  A frame that decodes: the same words.  A frame that does not (codes
            # (1, 1, 3), above): the recording decoder goes on recording behind the error, the walk gives no entry from
            # there on -- what it did give is what was recorded.
            pitch = S.n_seg(op, 32) - 1
            a, b = mine[1:].reshape(-1, pitch), plain_idx[1:].reshape(-1, pitch)
            assert mine[0] == plain_idx[0] and a.shape == b.shape
            decoding = 0
            for e, s in enumerate(entries):
                fo = S.frames(s)[:-1]
                first = int(corpus.entries[e]["first_frame"])
                assert len(fo) == int(corpus.entries[e]["n_frames"])
                for k, off in enumerate(fo):
                    samples, plen = S.header(s, off)
                    rc, _ = O.decode_frame(s[off + 20:off + 20 + plen], samples, op)
                    if rc == 0:
                        assert np.array_equal(a[first + k], b[first + k]), (e, k)
                        decoding += 1
                    else:
                        given = a[first + k] != 0
                        assert np.array_equal(a[first + k][given], b[first + k][given]), (e, k)
            assert decoding > 0 and (clean == (decoding == a.shape[0]))
        TC._check_entries(corpus, buf, offs, lens)
        rng = np.random.default_rng(bl + bpf)
        for fmt in (0, 1):
            ents, starts = TC._draw(rng, corpus, 32, 3_000)
            TC._check_contract(ctx, x3, corpus, buf, offs, lens, ents, starts, 3_000, fmt, p=p, clips=clips)
            # (_check_contract ends with a windows call of its own, on one entry alone)
        ents, starts = TC._draw(rng, corpus, 32, 3_000)
        TC._windows(corpus, ents, starts, 3_000, 0)
        assert clean == (ctx.get_option("last_window_replays") == 0)
    finally:
        corpus.close()


def test_flags_and_arguments(ctx, x3):
    L = x3.lib()
    p = x3.Params.make(40, 250)
    wav = x3.synth(2, 9, 0, 30_000)
    rc, s, _ = O.encode(wav, O.Params.make(40, 250, (0, 1, 3)))
    assert rc == 0
    offs = S.frames(s)[:-1]
    F = len(offs)
    d_x3, d_off = _on_device(ctx, s, offs)
    ne = L.x3_seg_index_entries(F, C.byref(p), 32)
    d_idx, d_back, d_res = ctx.alloc(8 * ne), ctx.alloc(2 * 30_000), ctx.alloc(64)
    try:
        def call(x=d_x3, n=s.size, fo=d_off, nf=F, params=p, idx=d_idx, sb=32):
            return L.x3_seg_index_build_dev(ctx._h, x, n, fo, nf, C.byref(params), idx, sb)
        for bad in (dict(x=None), dict(fo=None), dict(idx=None), dict(x=d_x3 + 2), dict(fo=d_off + 4), dict(idx=d_idx + 4),
                    dict(nf=0), dict(nf=1 << 31), dict(sb=0), dict(sb=30), dict(sb=3204),
                    dict(params=x3.Params.make(codes=(0, 1, 4))), dict(params=x3.Params.make(0, 10))):
            assert call(**bad) == BAD, bad
        # a pending x3_decode_dev and a pending windows call are left alone
        assert ctx.decode_dev(d_x3, s.size, d_off, F, p, d_back, 30_000, n_per_clip=30_000) == 0
        assert call() == 0
        assert ctx.get_option("last_seg_index_irregular") == 0
        rc, first_bad, _, _ = ctx.decode_result()
        assert (rc, first_bad) == (0, F) and np.array_equal(ctx.download(d_back, 60_000, np.int16), wav)
        # frames of one stretch: nothing to write
        assert L.x3_seg_index_entries(F, C.byref(p), 252) == 0
        ctx.upload(d_idx, np.full(ne, POISON, dtype=np.uint64))
        assert call(sb=252) == 0
        assert (ctx.download(d_idx, 8 * ne, np.uint64) == np.uint64(POISON)).all()
        # the new flag is x3_corpus_build's alone
        offs1, lens1 = np.array([0], dtype=np.uint64), np.array([s.size], dtype=np.uint64)
        assert L.x3_decode_streams_dev(ctx._h, d_x3, s.size, offs1.ctypes.data, lens1.ctypes.data, 1, x3.CORPUS_INDEX_WALK,
                                       C.byref(p), d_back, 30_000, 0, d_res) == BAD
        h = C.c_void_p(0)
        for flags in (2, 0x200, 0x101 | 4):
            assert L.x3_corpus_build(ctx._h, d_x3, s.size, offs1.ctypes.data, lens1.ctypes.data, 1, flags, C.byref(p), 32,
                                     C.byref(h)) == BAD and not h.value
        with pytest.raises(ValueError):
            x3.Corpus(ctx, (d_x3, s.size), [0], [s.size], params=p, index="other")
        with pytest.raises(ValueError):
            x3.WindowSource(ctx, (d_x3, s.size), p, index="other")
    finally:
        for q in (d_x3, d_off, d_idx, d_back, d_res):
            ctx.free(q)


# ---- 5. hostile input, under guard pages
def _child(code, timeout=900):
    env = dict(os.environ, X3HIP_FENCE="16", X3HIP_FENCE_FILL="165")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "x3-rust_amd"), HERE, os.path.join(ROOT, "tools"),
                                         env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-15:])
    assert r.returncode == 0, "child under the fence ended with %d:\n%s" % (r.returncode, tail)
    return r.stdout


def test_hostile_streams_under_the_fence():
    """damaged streams (x3_cases.damage: flipped and cleared payload bits, sample counts and header bytes that lie,
    truncation) in buffers that end at an unmapped page, frame tables that also point at junk, at the last bytes and at
    x3_len: the build runs clean, stays inside its index, and windows by what it built are the windows without an index --
    rows and statuses (which the window tests hold against the oracle).  Then family x of tools/fuzz_parity.py under the
    same fence: windows by the built index against the oracle's frame verdicts."""
    out = _child("""
        import ctypes as C
        import numpy as np
        import x3hip, oracle_lib as O, x3_cases as XC, seg_index_ref as S
        ctx = x3hip.Context(0)
        L = x3hip.lib()
        POISON = 0xDEADBEEFDEADBEEF
        builds = stopped = 0
        for trial in range(60):
            rng = np.random.default_rng([5, trial])
            bl, bpf = [(20, 500), (20, 100), (10, 200), (40, 250), (13, 77), (60, 50)][trial % 6]
            sb = int(rng.choice([4, 8, 32]))
            p, op = x3hip.Params.make(bl, bpf), O.Params.make(bl, bpf, (0, 1, 3))
            n = bl * bpf * int(rng.integers(2, 6)) + int(rng.integers(1, bl * bpf))
            wav = x3hip.synth(int(rng.choice([1, 2, 4])), 100 + trial, 0, n)
            rc, stream, _ = O.encode(wav, op)
            assert rc == 0
            offs = S.frames(stream)[:-1]
            bad = XC.damage(rng, stream, offs)
            if bad.size < 4:
                continue
            table = [o for o in offs if o < bad.size]
            if trial % 2:       # offsets that are no frame's: junk, the last bytes, x3_len itself, far behind it
                table += [int(rng.integers(0, bad.size)), max(bad.size - 21, 0), bad.size - 1, bad.size, bad.size + 5, 2 ** 63]
            if not table:
                continue
            F = len(table)
            ne = L.x3_seg_index_entries(F, C.byref(p), sb)
            if ne == 0:
                continue
            d_x3, d_off, d_idx = ctx.alloc(bad.size), ctx.alloc(8 * (F + 1)), ctx.alloc(8 * ne)   # (exact sizes: the fence is behind them)
            ctx.upload(d_x3, bad); ctx.upload(d_off, np.array(table + [bad.size], dtype=np.uint64))
            ctx.upload(d_idx, np.full(ne, POISON, dtype=np.uint64))
            assert ctx.seg_index_build_dev(d_x3, bad.size, d_off, F, p, d_idx, sb) == 0
            stopped += ctx.get_option("last_seg_index_irregular")
            idx = ctx.download(d_idx, 8 * ne, np.uint64)
            assert int(idx[0]) == S.SEG_MAGIC | (sb << 32) and not (idx == np.uint64(POISON)).any()
            with_idx = x3hip.WindowSource(ctx, (d_x3, bad.size), p, seg_blocks=sb, frame_offsets=d_off, n_frames=F, seg_index=d_idx)
            without = x3hip.WindowSource(ctx, (d_x3, bad.size), p, seg_blocks=0, frame_offsets=d_off, n_frames=F)
            total = with_idx.total
            assert total == without.total
            if total:
                for fmt in (0, 1):
                    Lw = int(rng.choice([1, 20, 333, min(total, bl * bpf)]))
                    Lw = max(1, min(Lw, total))
                    starts = [int(v) for v in rng.integers(0, total - Lw + 1, 24)] + [total, 2 ** 64 - 1]
                    a, sa = with_idx.decode(starts, Lw, fmt)
                    b, sb_ = without.decode(starts, Lw, fmt)
                    assert np.array_equal(sa, sb_), (trial, sa, sb_)
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), trial
            with_idx.close(); without.close()
            for q in (d_x3, d_off, d_idx):
                ctx.free(q)
            builds += 1
        ctx.close()
        import fuzz_parity as FZ
        c = FZ.run(seed=15, trials=150, families="x")
        print("builds", builds, "stopped", stopped, "trials", sum(c.values()))
        """)
    words = out.split()
    builds, stopped, trials = (int(words[words.index(k) + 1]) for k in ("builds", "stopped", "trials"))
    print(out)
    assert builds >= 40 and stopped > 0 and trials == 150


# ---- 6. the fuzz family
def test_200_trials_of_fuzz_family_x(ctx):
    spec = importlib.util.spec_from_file_location("seg_index_fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    FZ = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(FZ)
    counts = FZ.run(seed=14, trials=200, families="x", context=ctx)
    assert counts["x"] == 200


def test_x3_hpp_seg_index(tmp_path):
    """tests/host_cpp/test_seg_index_hpp.cpp: device::build_seg_index, index_by_walk and Corpus::build(index_walk) of the
    C++ mirror"""
    import x3hip
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_seg_index_hpp.cpp")
    exe = str(tmp_path / "test_seg_index_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
