"""seg_index_ref.py proved on the CPU: the oracle's reader restarted at an entry's bit, with the entry's previous sample in
front, reproduces the rest of the frame's samples -- for block lengths 10 / 13 / 20 / 40, ragged last frames and a frame
of one sample.  The GPU tests hold x3_seg_index_build_dev against this reference word for word."""
import numpy as np
import pytest

import oracle_lib as O
import seg_index_ref as S


def _wav(n, seed, loud_every=0):
    """quiet noise on a slow swell, with loud stretches (BFP and literal blocks) every `loud_every` samples"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    w = 300.0 * np.sin(t / 37.0) + rng.normal(0, 4.0, n)
    if loud_every:
        for a in range(loud_every // 2, n, loud_every):
            w[a:a + 170] += rng.normal(0, 9000.0, min(170, n - a))
    return np.clip(np.round(w), -32768, 32767).astype(np.int16)


CASES = [(10, 100, 32, 2_500), (13, 30, 4, 1_000), (20, 500, 32, 25_003), (20, 500, 64, 10_001), (40, 250, 32, 20_002),
         (40, 25, 8, 3_001), (20, 100, 32, 1), (13, 30, 8, 390 * 2 + 1)]


@pytest.mark.parametrize("bl,bpf,sb,n", CASES)
def test_restarting_at_an_entry_reproduces_the_rest_of_the_frame(bl, bpf, sb, n):
    p = O.Params.make(bl, bpf, (0, 1, 3))
    wav = _wav(n, bl * 1000 + n, loud_every=777)
    rc, stream, _ = O.encode(wav, p)
    assert rc == 0
    fo = S.frames(stream)[:-1]
    spf = bl * bpf
    assert len(fo) == (n + spf - 1) // spf
    words, expect = S.build(stream, fo, p, sb)
    ns = S.n_seg(p, sb)
    assert words.size == S.n_words(len(fo), p, sb) and words[0] == np.uint64(S.SEG_MAGIC | (sb << 32))
    seen = 0
    for f, off in enumerate(fo):
        samples, plen = S.header(stream, off)
        assert samples == min(spf, n - f * spf)
        payload = stream[off + 20:off + 20 + plen]
        frame = wav[f * spf:f * spf + samples]
        nbf = (samples - 1 + bl - 1) // bl
        assert expect[f] == min(ns - 1, (nbf - 1) // sb if nbf else 0)       # every block the frame has, and no other
        for q in range(1, ns):
            w = int(words[1 + f * (ns - 1) + q - 1])
            if q > expect[f]:
                assert w == 0                                                  # at or behind the frame's last block
                continue
            bit, prev, valid = w & 0xFFFFFFFF, (w >> 32) & 0xFFFF, (w >> 48) & 1
            assert valid and 16 <= bit <= 8 * plen
            b = sb * q
            assert prev == int(frame[b * bl]) & 0xFFFF                       # sample b * bl is the one in front of block b
            rc, rest, _ = S.decode_from(payload, samples, p, b, bit, prev)
            assert rc == 0 and np.array_equal(rest, frame[1 + b * bl:])
            seen += 1
    assert seen == sum(expect)
    if n > sb * bl + 1:
        assert seen > 0


def test_a_wrong_entry_does_not_reproduce_the_frame():
    """the check has teeth: one bit off, or another previous sample, and the rest of the frame differs"""
    p = O.Params.make(20, 100, (0, 1, 3))
    wav = _wav(2_000, 5)
    rc, stream, _ = O.encode(wav, p)
    assert rc == 0
    words, expect = S.build(stream, [0], p, 32)
    assert expect == [3]
    samples, plen = S.header(stream, 0)
    payload = stream[20:20 + plen]
    w = int(words[1])
    bit, prev = w & 0xFFFFFFFF, (w >> 32) & 0xFFFF
    want = wav[1 + 32 * 20:samples]
    rc, rest, _ = S.decode_from(payload, samples, p, 32, bit, prev)
    assert rc == 0 and np.array_equal(rest, want)
    rc, rest, _ = S.decode_from(payload, samples, p, 32, bit, (prev + 1) & 0xFFFF)
    assert rc != 0 or not np.array_equal(rest, want)
    rc, rest, _ = S.decode_from(payload, samples, p, 32, bit + 1, prev)
    assert rc != 0 or not np.array_equal(rest, want)
