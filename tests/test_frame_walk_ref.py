"""The plain frame walk (frame_walk_ref.walk), the header scanner and the stream generators, pinned against the CPU oracle
before tests/test_gpu_frame_walk.py judges the GPU walk by them.  No GPU."""
import numpy as np
import pytest

import frame_walk_ref as R
import oracle_lib as O


def test_crc16_rows_is_the_oracles():
    rows = np.random.default_rng(0).integers(0, 256, (2000, 16), dtype=np.uint8)
    assert [int(c) for c in R.crc16_rows(rows)] == [O.crc16(r) for r in rows]
    assert R._crc16_py(rows[7].tobytes()) == O.crc16(rows[7])


def chains():
    """(name, case factory): every generator, plus damage at depth"""
    out = [("padded", R.padded), ("odd_tails", R.odd_tails), ("sparse", R.sparse), ("dense", R.dense)]
    for m in (9, 10, 11, 12):
        for n in (2 ** m - 1, 2 ** m, 2 ** m + 1):
            out.append(("zeros%d" % n, lambda n=n: R.zero_chain(n)))
    out.append(("zeros%d" % (2 ** 17 + 1), lambda: R.zero_chain(2 ** 17 + 1)))
    for n in quiet_counts():
        out.append(("quiet%d" % n, lambda n=n: R.zero_chain(n, 103)))
    out += [("padded+junk", lambda: R.junk_front(R.padded())),
            ("dense+broken", lambda: R.broken_header(R.dense(), 100)),
            ("dense+lead", lambda: dense_lead_in()),
            ("odd_tails-cut", lambda: R.truncated(R.odd_tails(), 100)),
            ("zeros+broken", lambda: R.broken_header(R.zero_chain(2 ** 12 + 1), 3000)),
            ("sparse+junk", lambda: R.junk_front(R.sparse(), 3))]
    return out


def quiet_counts():
    """frame counts of 306-byte frames at, one below and one above x3_decode_stream_dev's one-trip bound"""
    fb = len(R._zero_frame(103)[0])
    n = max(k for k in range(1, 1000) if k <= R.one_trip_bound(fb, k))
    return (n - 1, n, n + 1)


def dense_lead_in():
    """a header at offset 0 whose successor is a planted "cont" header of the dense stream's first tail: the walk runs
    through false headers and merges into the real chain"""
    d = R.dense()
    target = next(o for o, k in d.planted if k == "cont" and o <= R.READ_BUFFER)
    return R.lead_in(d, target)


@pytest.mark.parametrize("name,make", chains(), ids=[n for n, _ in chains()])
def test_walk_agrees_with_the_oracle(name, make):
    case = make()
    w = R.walk(case.stream)
    total = int(w.n_samples) + 65536
    rc, wav, fok, ferr = O.decode_stream(case.stream, case.params, wav_cap=total)
    if w.terminal == R.BAD_ARG:      # the last pushed frame is the one the walk stops at
        assert (rc, fok, wav.size) == (R.BAD_ARG, w.n_frames - 1, w.n_samples), (w, rc, fok, wav.size)
    elif ferr == 0 and fok == w.n_frames:
        assert (rc, wav.size) == (w.terminal, w.n_samples), (w, rc, wav.size)
    else:                            # a pushed frame that does not decode (the lead-in's payload)
        assert name.endswith("lead")
        assert fok < w.n_frames
    assert np.all(np.diff(w.frame_off.astype(np.int64)) > 0)
    if case.wav is not None:
        assert np.array_equal(wav, case.wav)
        assert w.n_frames == len(R.frame_offsets(case.stream))


def test_the_walk_stops_where_the_output_ends():
    case = R.zero_chain(100_000)
    cap = 40_000 * 20 + 7
    w = R.walk(case.stream, wav_cap=cap)
    assert (w.n_frames, w.n_samples, w.terminal) == (40_001, 800_000, R.BAD_ARG)
    rc, wav, fok, ferr = O.decode_stream(case.stream, case.params, wav_cap=cap)
    assert (rc, wav.size, fok, ferr) == (R.BAD_ARG, 800_000, 40_000, 0)


@pytest.mark.parametrize("make", [R.padded, R.odd_tails, R.sparse, R.dense])
def test_padded_streams_decode_to_the_unpadded_samples(make):
    case = make()
    plain = R.encode(case.wav)
    assert case.stream.size > plain.size
    rc, wav, fok, ferr = O.decode_stream(case.stream, case.params, wav_cap=case.wav.size)
    assert (rc, fok, ferr) == (0, len(R.frame_offsets(plain)), 0)
    assert np.array_equal(wav, case.wav)


def test_odd_tails_put_frames_on_odd_offsets():
    offs = R.frame_offsets(R.odd_tails().stream)
    assert sum(o & 1 for o in offs) >= len(offs) // 3


@pytest.mark.parametrize("make", [R.sparse, R.dense])
def test_planted_headers_are_valid_and_of_their_kind(make):
    case = make()
    s = case.stream
    found = set(R.scan(s).tolist())
    real = R.frame_offsets(s)
    for off, kind in case.planted:
        st, samples, plen = R.header_status(s, off)
        assert st == R.OK, (off, kind, st)
        assert R.kind_of(s.size, s.size, off, plen, samples) == R.KIND_NAMES[kind], (off, kind)
        if kind == "merge":
            assert off + 20 + plen in set(real) | {s.size}   # (the next real frame, or the end behind the last)
    assert found >= set(real) | {o for o, _ in case.planted}
    assert len(found) == len(real) + len(case.planted)


def test_dense_stream_overflows_every_limit_of_the_candidate_scan():
    """512 candidates in a 4 KiB span (> X3I_WG_RAW = 384 key places, > X3I_WG_CANDS = 256), more candidates than the
    general walk's first buffer (max(4096, len / 256 + 1024)), every planted kind, chains that merge"""
    case = R.dense()
    offs = R.scan(case.stream)
    per_span = np.bincount(offs // 4096)
    assert per_span.max() >= 512
    assert (per_span > 384).sum() >= 200
    assert offs.size > max(4096, case.stream.size // 256 + 1024)
    kinds = {k for _, k in case.planted}
    assert kinds == {"cont", "merge", "last_bad", "plen", "quiet"}
    assert 4 << 20 <= case.stream.size <= 16 << 20


def test_sparse_stream_has_false_headers_within_the_one_trip_bound():
    case = R.sparse()
    n = R.scan(case.stream).size
    assert n == 2 * len(R.frame_offsets(case.stream))
    assert n <= case.stream.size // 1024 + 64
    samples = [R.header_status(case.stream, o)[1] for o, _ in case.planted]
    assert min(samples) >= 65520
    assert any(o & 1 for o, _ in case.planted)
    assert 4 << 20 <= R.sparse_long().stream.size <= 16 << 20


def test_zero_chains_are_clean_and_choose_every_doubling_remainder():
    """levels = 1 + ceil(log2 n) candidates: (levels - 1) mod 4 takes all four values over the chain lengths used"""
    rems = set()
    for m in (9, 10, 11, 12):
        for n in (2 ** m - 1, 2 ** m, 2 ** m + 1):
            levels = 1
            while (1 << (levels - 1)) < n:
                levels += 1
            rems.add((levels - 1) % 4)
    assert rems == {0, 1, 2, 3}
    case = R.zero_chain(2 ** 12 + 1)
    assert np.array_equal(R.scan(case.stream), R.walk(case.stream).frame_off.astype(np.int64))
    fb = len(R._zero_frame(103)[0])
    lo, at, hi = quiet_counts()
    assert at <= R.one_trip_bound(fb, at) and hi > R.one_trip_bound(fb, hi)
