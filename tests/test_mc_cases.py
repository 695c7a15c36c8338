"""The multi-channel case builders of x3_cases.py, pinned on the CPU with the oracle alone: the pools of crafted frames
that tests/test_gpu_multichannel_edges.py decodes hold frames of all three classes -- frames that fail to decode, frames that
decode and are not plain (x3_decode_mc_lanes_kernel has to hand them to the reference's reader), and plain frames (it has to
decode them itself) -- the clean frames round-trip, and the encoder's payload-edge inputs have exactly the payload lengths the
GPU test names."""
import numpy as np
import pytest

import oracle_lib as O
from x3_cases import (MC_CHANNELS, MC_FOREIGN, PAYLOAD_EDGE, edge_channels, MC_PIDS, MC_POOL, MC_PSETS, _Seeded, frame_offsets, mc_clean_frames,
                      mc_encode_frame_py, mc_frame, mc_params, mc_pool, mc_verdict, signals)

def payload_bits(bpf, n_ch, n_lit):
    """the payload length the layout gives (x3_mc.h): first samples, blocks in (block index, channel) order, word_align"""
    bits = 16 * n_ch + (bpf - 1) * (n_lit * 166 + (n_ch - n_lit) * 12) + n_lit * (6 + 16 * 9) + (n_ch - n_lit) * (2 + 9)
    return (((bits + 7) >> 3) + 1) & ~1


def classify(n_ch, pi):
    """-> (fails, decodes and is not plain, plain) of the pool"""
    op = mc_params(MC_PSETS[pi])
    fails = odd = plain = 0
    for pay, n in mc_pool(n_ch, pi):
        (rc, fok, ferr), wavs, pl = mc_verdict(pay, n, n_ch, op)
        assert pl in ((-1,) if n == 0 or pay.size < 2 * n_ch else (0, 1)), (n_ch, pi, pay.size, n)
        if fok != 1:
            assert (rc, ferr) != (0, 0) or pay.size == 0, (n_ch, pi, pay.size, n)   # (an empty payload at the end: no frame)
            fails += 1
            continue
        assert (rc, ferr) == (0, 0) and all(w.size == n for w in wavs)
        if pl == 1:   # a plain frame decodes to the same samples read as a plain bit string
            assert np.array_equal(np.array(wavs), O.frame_plain(pay, n, op, n_ch=n_ch)[1])
            plain += 1
        else:
            assert pl == 0
            odd += 1
    return fails, odd, plain


def frame_status(pay, n, n_ch, op):
    """x3o_decode_frame_mc's own status (a stream only counts the frame as an error)"""
    import ctypes as C
    pay = np.ascontiguousarray(pay, dtype=np.uint8)
    rows = [np.zeros(n + 8, dtype=np.int16) for _ in range(n_ch)]
    ptrs = (C.c_void_p * n_ch)(*[r.ctypes.data for r in rows])
    L = O.lib()
    L.x3o_decode_frame_mc.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t,
                                      C.c_void_p]
    return L.x3o_decode_frame_mc(pay.ctypes.data, pay.size, ptrs, n + 8, n_ch, C.byref(op), n, None)


@pytest.mark.parametrize("pi", range(6), ids=MC_PIDS[:6])
def test_pools_reach_every_hand_over(pi):
    """what x3_decode_mc_lanes_kernel hands over or refuses, per parameter set it takes: frames that end in
    OutOfBoundsInverse (5: the index bound, and with it the zero runs of 32 bits and more, which it defers),
    FrameDecodeInvalidBPF (20: the BFP width), frames that decode by reading behind their payload or across a long zero
    run (not plain), and frames whose geometry is BAD_ARG (24)"""
    op = mc_params(MC_PSETS[pi])
    seen = {}
    for n_ch in MC_CHANNELS:
        for pay, n in mc_pool(n_ch, pi):
            st = frame_status(pay, n, n_ch, op)
            if st == 0 and O.frame_plain(pay, n, op, n_ch=n_ch)[0] == 0:
                st = "not plain"
            seen[st] = seen.get(st, 0) + 1
    print(MC_PIDS[pi], seen)
    assert seen.get(5, 0) >= 10 and seen.get(20, 0) >= 10 and seen.get(24, 0) >= 10 and seen.get(0, 0) >= 10, seen
    assert seen.get("not plain", 0) >= 1 and set(seen) <= {0, 5, 20, 24, "not plain"}, seen


def test_pools_hold_all_three_classes():
    total = np.zeros(3, dtype=np.int64)
    table = {}
    for n_ch in MC_CHANNELS:
        for pi in range(len(MC_PSETS)):
            pool = mc_pool(n_ch, pi)
            assert len(pool) >= MC_POOL >= 150
            table[(n_ch, MC_PIDS[pi])] = classify(n_ch, pi)
            total += table[(n_ch, MC_PIDS[pi])]
    print("pools: (fails, decodes and is not plain, plain)", table, total.tolist())
    assert total[0] >= 500 and total[1] >= 12 and total[2] >= 300, total.tolist()
    # every parameter set the lanes kernel takes sees both decisions: frames to keep and frames to hand over
    for pi in range(6):
        per = np.sum([table[(n_ch, MC_PIDS[pi])] for n_ch in MC_CHANNELS], axis=0)
        assert per[2] > 0 and per[0] + per[1] > 0, (MC_PIDS[pi], per.tolist())


def test_pools_are_seeded():
    a, b = mc_pool(3, 1), mc_pool(3, 1)
    assert len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(a, b))


def test_mc_frame_is_a_frame():
    """mc_frame's header is what the oracle's encoder writes around the same payload"""
    wavs = [np.arange(50, dtype=np.int16) * (c + 1) for c in range(3)]
    rc, s, _ = O.encode_mc(wavs, O.Params.make(20, 4000))
    assert rc == 0 and np.array_equal(mc_frame(s[20:], 50, 3), s)
    assert frame_offsets(np.concatenate([s, s])) == [0, s.size]


@pytest.mark.parametrize("bl", [13, 20, 60])
def test_the_restated_layout_is_the_oracles(bl):
    """mc_encode_frame_py, which writes the frames of block lengths 61 and 100, gives the oracle's bytes at the block
    lengths the oracle's encoder takes: every code set of the pools, blocks of every type, ragged last blocks"""
    rng = np.random.default_rng(bl)
    sigs = signals(_Seeded, rng)
    seen = 0
    for codes, thr in MC_FOREIGN + [(c, t) for c, t, _ in MC_PSETS]:
        for n_ch in MC_CHANNELS:
            for i, w in enumerate(sigs):
                wavs = [np.resize(sigs[(i + c) % len(sigs)], w.size) for c in range(n_ch)]
                rc, s, _ = O.encode_mc(wavs, O.Params.make(bl, 4000, codes, thr))
                if rc == 0:
                    assert np.array_equal(mc_encode_frame_py(wavs, bl, codes, thr), s), (codes, thr, n_ch, i)
                    seen += 1
    assert seen >= 200


@pytest.mark.parametrize("pi", range(len(MC_PSETS)), ids=MC_PIDS)
def test_clean_frames_round_trip(pi):
    """aligned (multiples of eight) and odd sample counts, every channel count: one stream of them decodes to its content"""
    op = mc_params(MC_PSETS[pi])
    for n_ch in MC_CHANNELS:
        rng = np.random.default_rng([9, n_ch, pi])
        counts = [32, 600, 40, 31, 599, 33, 101]
        frames = mc_clean_frames(rng, op, n_ch, counts)
        stream = np.concatenate([f for f, _ in frames])
        rc, back, fok, ferr = O.decode_stream_mc(stream, n_ch, op, wav_cap=sum(counts) + 8)
        assert (rc, fok, ferr) == (0, len(counts), 0)
        for c in range(n_ch):
            assert np.array_equal(back[c], np.concatenate([w[c] for _, w in frames]))


@pytest.mark.parametrize("bpf,n_ch,n_lit,plen,status", PAYLOAD_EDGE)
def test_payload_edge_lengths(bpf, n_ch, n_lit, plen, status):
    """the oracle's encoder at the 24 KB limit: 24 576 and 24 574 bytes are accepted and round-trip, 24 578, 24 640 and
    24 642 are FrameLength"""
    assert payload_bits(bpf, n_ch, n_lit) == plen
    po = O.Params.make(10, bpf)
    wavs = edge_channels(bpf, n_ch, n_lit)
    rc, s, st = O.encode_mc(wavs, po)
    assert rc == status
    if status:
        return
    assert s.size == 20 + plen and (int(s[6]) << 8 | int(s[7])) == plen and s[3] == n_ch
    assert st[5] == n_lit * (10 * bpf - 1) and st[0] == (n_ch - n_lit) * (10 * bpf - 1)   # literal and silent blocks only
    rc, back, fok, ferr = O.decode_stream_mc(s, n_ch, po, wav_cap=10 * bpf)
    assert (rc, fok, ferr) == (0, 1, 0) and all(np.array_equal(b, w) for b, w in zip(back, wavs))
    assert O.frame_plain(s[20:], 10 * bpf, po, n_ch=n_ch)[0] == 1
