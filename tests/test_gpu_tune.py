"""Parameter tuning on the GPU (include/x3hip.h, "parameter tuning"): every candidate's size against the oracle's encode
byte for byte, accumulation, the choice and its tie rule, the tuned archive through every reader, files and the CLI, the
C++ mirror, and the argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from x3_cases import frame_offsets, patchwork

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 24
N_CAND = 2184
DEFAULT = 1188


@pytest.fixture(scope="module")
def x3():
    import x3hip
    return x3hip


@pytest.fixture(scope="module")
def ctx(x3):
    c = x3.Context(0)
    yield c
    c.close()


def oparams(x3, i, spf):
    rc, p = x3.tune_candidate(i, spf)
    assert rc == 0
    return O.Params.make(block_len=p.block_len, blocks_per_frame=p.blocks_per_frame, codes=(0, 1, 3),
                         thresholds=tuple(p.thresholds))


def oracle_size(x3, w, i, spf):
    rc, b, _ = O.encode(w, oparams(x3, i, spf))
    assert rc == 0
    return len(b)


def oracle_table(x3, w, spf):
    return np.array([oracle_size(x3, w, i, spf) for i in range(N_CAND)], dtype=np.uint64)


def expected_choice(sizes):
    m = sizes.min()
    return DEFAULT if sizes[DEFAULT] == m else int(np.flatnonzero(sizes == m)[0])


def tune_dev(ctx, x3, w, spf, clip_stride=None, n_clips=1, n_per_clip=None):
    """one Tuner.add_dev of w (already laid out) -> (rc, best, best_bytes, sizes, max payloads)"""
    d = ctx.alloc(max(w.nbytes, 2))
    try:
        ctx.upload(d, w)
        t = x3.Tuner(ctx, spf)
        npc = w.size if n_per_clip is None else n_per_clip
        assert t.add_dev(d, npc, clip_stride, n_clips) == 0
        rc, best, bb, sizes = t.result()
        mp = t.max_payloads()
        t.close()
        return rc, best, bb, sizes, mp
    finally:
        ctx.free(d)


def kinds(x3, n):
    return {
        "patchwork": patchwork(11, n).astype(np.int16),
        "zeros": np.zeros(n, dtype=np.int16),
        "white": x3.synth(x3.SYNTH_WHITE, 0x58330001, 0, n),
        "hydrophone": x3.synth(x3.SYNTH_HYDROPHONE, 0x58330001, 0, n),
    }


@pytest.mark.parametrize("kind", ["patchwork", "zeros", "white", "hydrophone"])
def test_every_candidate_size_is_exact(ctx, x3, kind):
    w = kinds(x3, 60_000)[kind]
    rc, best, bb, sizes, mp = tune_dev(ctx, x3, w, 10000)
    assert rc == 0
    ref = oracle_table(x3, w, 10000)
    bad = np.flatnonzero(sizes != ref)
    assert bad.size == 0, (kind, bad[:8], sizes[bad[:8]], ref[bad[:8]])
    k = expected_choice(ref)
    rc, p = x3.tune_candidate(k, 10000)
    assert (best.block_len, list(best.thresholds)) == (p.block_len, list(p.thresholds)) and bb == ref[k]
    # the largest frame payload of a few candidates, from the oracle's frames
    for i in (0, DEFAULT, k, N_CAND - 1):
        s = O.encode(w, oparams(x3, i, 10000))[1]
        offs = list(frame_offsets(s)) + [s.size]
        assert mp[i] == max(offs[j + 1] - offs[j] - 20 for j in range(len(offs) - 1)), i


@pytest.mark.parametrize("n,spf", [(60_001, 10000), (1, 10000), (50_001, 10000), (33_333, 40), (61_441, 10240),
                                   (20_479, 10240), (41, 40)])
def test_ragged_and_edge_geometries(ctx, x3, n, spf):
    w = patchwork(n + spf, n).astype(np.int16)
    rc, best, bb, sizes, _ = tune_dev(ctx, x3, w, spf)
    assert rc == 0
    ref = oracle_table(x3, w, spf)
    bad = np.flatnonzero(sizes != ref)
    assert bad.size == 0, (n, spf, bad[:8], sizes[bad[:8]], ref[bad[:8]])


@pytest.mark.parametrize("stride_extra,odd_base", [(0, False), (13, False), (40, True)])
def test_batch_of_clips(ctx, x3, stride_extra, odd_base):
    """clips framed from their own starts; a stride larger than the clip; a base that is not on a dword boundary"""
    n, clips, spf = 14_007, 4, 10000
    stride = n + stride_extra
    src = [x3.synth(x3.SYNTH_HYDROPHONE, 77 + c, 0, n) if c % 2 else patchwork(90 + c, n).astype(np.int16)
           for c in range(clips)]
    lay = np.full(stride * clips + 1, 12345, dtype=np.int16)   # garbage between clips must not count
    off = 1 if odd_base else 0
    for c in range(clips):
        lay[off + c * stride: off + c * stride + n] = src[c]
    d = ctx.alloc(lay.nbytes)
    try:
        ctx.upload(d, lay)
        t = x3.Tuner(ctx, spf)
        assert t.add_dev(d + 2 * off, n, stride, clips) == 0
        rc, best, bb, sizes = t.result()
        t.close()
    finally:
        ctx.free(d)
    assert rc == 0
    ref = sum(oracle_table(x3, s, spf) for s in src)
    bad = np.flatnonzero(sizes != ref)
    assert bad.size == 0, (bad[:8], sizes[bad[:8]], ref[bad[:8]])


def test_large_inputs_on_a_sample_of_candidates(ctx, x3):
    rng = np.random.default_rng(5)
    pick = sorted(set(rng.choice(N_CAND, 64, replace=False).tolist()) | {DEFAULT})
    for kind, n in ((x3.SYNTH_HYDROPHONE, 4_000_000), (x3.SYNTH_WALK, 3_000_017)):
        w = x3.synth(kind, 0x58330001, 0, n)
        p, bb, sizes = ctx.tune(w)
        for i in pick:
            assert sizes[i] == oracle_size(x3, w, i, 10000), (kind, i)
        k = expected_choice(sizes)
        assert bb == sizes[k] == oracle_size(x3, w, k, 10000)


def test_accumulation_and_reset(ctx, x3):
    spf = 10000
    w = x3.synth(x3.SYNTH_HYDROPHONE, 3, 0, 95_123)
    whole = tune_dev(ctx, x3, w, spf)[3]
    d = ctx.alloc(w.nbytes)
    try:
        ctx.upload(d, w)
        t = x3.Tuner(ctx, spf)
        for a, b in ((0, 30000), (30000, 70000), (70000, w.size)):   # every chunk but the last is whole frames
            assert t.add_dev(d + 2 * a, b - a) == 0
        rc, _, _, chunked = t.result()
        assert rc == 0 and np.array_equal(chunked, whole)
        assert t.reset() == 0
        rc, best, bb, empty = t.result()
        assert rc == 0 and not empty.any() and bb == 0
        assert (best.block_len, list(best.thresholds)) == (20, [3, 8, 20])
        assert t.add_dev(d, w.size) == 0
        assert np.array_equal(t.result()[3], whole)
        t.close()
    finally:
        ctx.free(d)


def test_choice_and_encode_with_it(ctx, x3):
    for kind in (x3.SYNTH_HYDROPHONE, x3.SYNTH_WALK, x3.SYNTH_SINE, x3.SYNTH_WHITE, x3.SYNTH_ZEROS):
        w = x3.synth(kind, 0x58330001, 0, 400_000)
        p, bb, sizes = ctx.tune(w)
        k = expected_choice(sizes)
        assert bb == sizes[k] <= sizes[DEFAULT]
        if kind == x3.SYNTH_ZEROS:
            assert k == 2 * 728   # silence: every triple ties, blocks of 40 have the fewest headers -> the lowest index
        rc, q = x3.tune_candidate(k)
        assert (p.block_len, p.blocks_per_frame, list(p.thresholds)) == (q.block_len, q.blocks_per_frame, list(q.thresholds))
        # x3_encode_dev with the choice writes exactly best_bytes, on a single-pass encoder
        d = ctx.alloc(w.nbytes)
        cap = int(O.encode_bound(w.size, oparams(x3, k, 10000)))
        dout = ctx.alloc(cap)
        try:
            ctx.upload(d, w)
            assert ctx.encode_dev(d, w.size, p, dout, cap) == 0
            rc, pos, _ = ctx.encode_result()
            assert rc == 0 and pos == bb
            assert ctx.get_option("enc_gen_in_use") in (2, 3)
            assert np.array_equal(ctx.download(dout, pos), O.encode(w, oparams(x3, k, 10000))[1])
        finally:
            ctx.free(dout)
            ctx.free(d)


def _best_of_geometry(sizes, g):
    part = sizes[g * 728:(g + 1) * 728]
    return g * 728 + int(np.argmin(part))


@pytest.mark.parametrize("kind", ["hydrophone", "walk", "patchwork"])
def test_tuned_archives_round_trip_through_every_reader(ctx, x3, kind, tmp_path):
    n = 123_457
    w = {"hydrophone": x3.synth(x3.SYNTH_HYDROPHONE, 0x58330001, 0, n), "walk": x3.synth(x3.SYNTH_WALK, 0x58330001, 0, n),
         "patchwork": patchwork(21, n).astype(np.int16)}[kind]
    rc, arch, stats, chosen = ctx.x3a_encode_tuned(w, 96000)
    assert rc == 0
    p, bb, sizes = ctx.tune(w)
    assert (chosen.block_len, list(chosen.thresholds)) == (p.block_len, list(p.thresholds))
    h = np.zeros(1024, np.uint8)
    hl = C.c_uint64(0)
    assert x3.lib().x3_archive_header_write(96000, C.byref(chosen), h.ctypes.data, h.size, C.byref(hl)) == 0
    assert arch.size == hl.value + bb and np.array_equal(arch[:hl.value], h[:hl.value])
    archives = [arch]
    # and the best set of each block length, written as an archive: header with its BLKLEN / T, then its stream
    for g in range(3):
        rc, q = x3.tune_candidate(_best_of_geometry(sizes, g))
        h = np.zeros(1024, np.uint8)
        hl = C.c_uint64(0)
        assert x3.lib().x3_archive_header_write(96000, C.byref(q), h.ctypes.data, h.size, C.byref(hl)) == 0
        rc, s, _ = ctx.encode(w, q, start_pos=hl.value)
        assert rc == 0
        s = s.copy()
        s[:hl.value] = h[:hl.value]
        archives.append(s)
    for a in archives:
        r = O.x3a_decode(a, wav_cap=n + 100)
        assert r[0] == 0 and np.array_equal(r[1], w), "oracle"
        r = ctx.x3a_decode(a, wav_cap=n + 100)
        assert r[0] == 0 and np.array_equal(r[1], w) and r[4] == 0, ("x3_x3a_decode", r[0], r[4])
        rd = x3.Reader(ctx, a)
        assert rd.rc == 0
        got = []
        while True:
            rc, smp = rd.next_frame()
            assert rc == 0
            if smp is None or len(smp) == 0:
                break
            got.append(np.array(smp, copy=True))
        assert rd.frame_errors() == 0
        rd.close()
        assert np.array_equal(np.concatenate(got), w), "reader"
        f = tmp_path / "a.x3a"
        f.write_bytes(a.tobytes())
        rc, ns, ferr = ctx.x3a_to_wav(str(f), str(tmp_path / "b.wav"))
        assert rc == 0 and ns == n and ferr == 0
        assert np.array_equal(np.frombuffer((tmp_path / "b.wav").read_bytes()[44:], dtype=np.int16), w)


def test_argument_checks_leave_the_totals(ctx, x3):
    w = x3.synth(x3.SYNTH_HYDROPHONE, 9, 0, 30_000)
    d = ctx.alloc(w.nbytes + 4)
    try:
        ctx.upload(d, w)
        t = x3.Tuner(ctx, 10000)
        assert t.add_dev(d, w.size) == 0
        before = t.result()[3]
        L = x3.lib()
        assert t.add_dev(d + 1, 1000) == BAD                          # misaligned
        assert L.x3_tuner_add_dev(t._h, None, C.byref(x3.Batch(10, 10, 1))) == BAD   # NULL samples
        assert L.x3_tuner_add_dev(t._h, C.c_void_p(d), None) == BAD   # NULL batch
        assert t.add_dev(d, 0) == BAD                                 # empty clip
        assert t.add_dev(d, 100, 100, 0) == BAD                       # no clips
        assert t.add_dev(d, 1000, 999, 2) == BAD                      # stride smaller than the clip
        assert np.array_equal(t.result()[3], before)
        t.close()
        for spf in (0, 30, 10280, 10020):
            with pytest.raises(x3.X3Error):
                x3.Tuner(ctx, spf)
            with pytest.raises(x3.X3Error):
                ctx.tune(w, spf)
        with pytest.raises(x3.X3Error):
            ctx.tune(np.zeros(0, np.int16))
    finally:
        ctx.free(d)


def _write_wav(path, wav, rate):
    data = np.ascontiguousarray(wav, dtype="<i2").tobytes()
    hdr = (b"RIFF" + (36 + len(data)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little")
           + (1).to_bytes(2, "little") + (1).to_bytes(2, "little") + rate.to_bytes(4, "little")
           + (2 * rate).to_bytes(4, "little") + (2).to_bytes(2, "little") + (16).to_bytes(2, "little")
           + b"data" + len(data).to_bytes(4, "little"))
    with open(path, "wb") as f:
        f.write(hdr + data)


def test_files_with_and_without_the_option(ctx, x3, tmp_path):
    n = 1_234_567
    w = x3.synth(x3.SYNTH_WALK, 0x58330001, 0, n)
    a = str(tmp_path / "in.wav")
    _write_wav(a, w, 44100)
    plain, tuned = str(tmp_path / "plain.x3a"), str(tmp_path / "tuned.x3a")
    assert ctx.get_option("file_tune") == 0
    ctx.set_option("file_chunk_frames", 16)   # several chunks: the tuning pass and the pipeline both go in pieces
    try:
        assert ctx.wav_to_x3a(a, plain)[0] == 0
        assert open(plain, "rb").read() == bytes(O.x3a_encode(w, 44100)[1])   # option off: today's bytes
        ctx.set_option("file_tune", 1)
        assert ctx.wav_to_x3a(a, tuned)[0] == 0
    finally:
        ctx.set_option("file_tune", 0)
        ctx.set_option("file_chunk_frames", 800)
    rc, arch, _, chosen = ctx.x3a_encode_tuned(w, 44100)
    assert rc == 0 and open(tuned, "rb").read() == bytes(arch)
    assert (chosen.block_len, list(chosen.thresholds)) != (20, [3, 8, 20])   # the walk prefers other thresholds
    r = O.x3a_decode(np.frombuffer(open(tuned, "rb").read(), np.uint8), wav_cap=n + 10)
    assert r[0] == 0 and np.array_equal(r[1], w)


def test_cli_tune(x3, tmp_path):
    n = 300_001
    w = x3.synth(x3.SYNTH_HYDROPHONE, 0x58330001, 0, n)
    a, b, c = str(tmp_path / "in.wav"), str(tmp_path / "out.x3a"), str(tmp_path / "back.wav")
    _write_wav(a, w, 192000)
    cli = os.path.join(ROOT, "x3-rust_amd", "bin", "x3")
    r = subprocess.run([cli, "--tune", "-i", a, "-o", b], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [s for s in r.stdout.splitlines() if s.startswith("Tuned parameters:")]
    assert len(line) == 1, r.stdout
    ctx = x3.Context(0)
    try:
        rc, arch, _, chosen = ctx.x3a_encode_tuned(w, 192000)
    finally:
        ctx.close()
    assert line[0] == "Tuned parameters: block length %d, thresholds (%d, %d, %d)" % ((chosen.block_len,) + tuple(chosen.thresholds))
    assert open(b, "rb").read() == bytes(arch)
    r = subprocess.run([cli, "-i", b, "-o", c], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.frombuffer(open(c, "rb").read()[44:], dtype=np.int16), w)
    r = subprocess.run([cli, "--tune", "-i", b, "-o", c], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


def test_x3_hpp_tune():
    """tests/host_cpp/test_tune_hpp.cpp: x3::tune, x3::tune_candidate and device::Tuner of the C++ mirror"""
    import x3hip
    O.lib()
    x3hip.lib()
    src = os.path.join(ROOT, "tests", "host_cpp", "test_tune_hpp.cpp")
    exe = os.path.join(ROOT, "tests", "host_cpp", "test_tune_hpp")
    libdir = os.path.dirname(x3hip.LIB_PATH)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, src, "-L" + libdir, "-lx3hip", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    subprocess.run([exe], check=True, timeout=300)
