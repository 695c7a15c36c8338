"""payload_cases.py builds what it says (no GPU): for every spec the GPU tests of the 9 728-byte edge use, the oracle's
encode of the constructed stream has exactly the demanded payload_len in every frame header, the blocks' measured bits
sum to the demanded bit count, and the oracle's decode_stream returns the samples.  No spec is skipped or approximated: a
target the construction cannot reach raises in frame() and fails here."""
import numpy as np
import pytest

import oracle_lib as O
import payload_cases as PC

SPECS = PC.all_specs()


def test_the_specs_are_the_ones_the_issue_asks_for(capsys):
    by_name = {s.name: s for s in SPECS}
    assert len(by_name) == len(SPECS)
    with capsys.disabled():
        print("\npayload_cases: %d specs, %d frames" % (len(SPECS), sum(len(s.frames) for s in SPECS)))
    # A: every bit count of L = 9 726, 9 728 and 9 730, shuffled, and two more arrangements where L changes
    a = by_name["A"].frames
    assert sorted(f.target_bits for f in a if f.arrangement == "shuffled") == list(range(77793, 77841))
    for arr in ("last_wide", "wide_first"):
        assert sorted(f.target_bits for f in a if f.arrangement == arr) == [77808, 77809, 77824, 77825]
    assert {PC.payload_len(f.target_bits) for f in a} == {9726, 9728, 9730} and all(f.n == 10000 for f in a)
    # B: every row boundary k = 6 .. 38 -- the largest bit count of each L and the smallest of 256 k -- and the short clips
    b = [f for part in range(3) for f in by_name["B%d" % part].frames]
    whole = sorted(f.target_bits for f in b if f.n == 10000)
    assert whole == sorted(bits for k in range(6, 39)
                           for bits in (8 * (256 * k - 2), 8 * 256 * k, 8 * (256 * k - 2) + 1, 8 * (256 * k + 2)))
    assert sorted(PC.payload_len(f.target_bits) for f in b if f.n != 10000) == [254, 256, 258]
    assert all(by_name["B%d" % part].frames[-1].n % 20 not in (0, 1) for part in range(3))   # (a ragged last block as well)
    # C: a full image in frames of 6 001 and 5 121 samples, BFP and literal
    c = [s.frames[-1] for s in SPECS if s.name.startswith("C")]
    assert sorted((f.n, f.target_bits, str(f.wide)) for f in c) == sorted(
        (n, bits, str(w)) for n, ws in ((6001, (13, "lit")), (5121, (14, "lit"))) for bits in (77824, 77825) for w in ws)
    # D: blocks of 10 and 40 at A's two-arrangement points
    for bl in (10, 40):
        d = by_name["D%d" % bl]
        assert (d.block_len, d.blocks_per_frame) == (bl, 10000 // bl)
        assert sorted({f.target_bits for f in d.frames}) == [77808, 77809, 77824, 77825] and len(d.frames) == 12
    # the groups: 64 + 64 frames at L = 9 728, wide_first then wide_last; frame 37 of each at L = 9 730 in the second spec
    for name, dense in (("G_full", []), ("G_one_dense", [37, 101])):
        g = by_name[name].frames
        assert [f.arrangement for f in g] == ["wide_first"] * 64 + ["wide_last"] * 64
        lens = [PC.payload_len(f.target_bits) for f in g]
        assert lens == [9730 if i in dense else 9728 for i in range(128)]
    assert all(sum(f.n for f in s.frames) <= 1_500_000 and len(s.frames) <= 150 for s in SPECS)


@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_the_oracle_sees_the_demanded_payloads(spec):
    b = PC.built(spec)
    po = spec.oparams
    assert len(b.plens) == len(spec.frames) and b.offsets[-1] == b.x3.size
    for i, (fs, w) in enumerate(zip(spec.frames, b.frames)):
        assert w.size == fs.n and w.dtype == np.int16
        assert PC.frame_bits(w, po) == fs.target_bits, (spec.name, i)
        assert b.plens[i] == PC.payload_len(fs.target_bits), (spec.name, i, b.plens[i], fs.target_bits)
        hdr = b.x3[b.offsets[i]:b.offsets[i] + 20]
        assert (int(hdr[4]) << 8 | int(hdr[5])) == fs.n
    rc, back, fok, ferr = O.decode_stream(b.x3, po, wav_cap=b.wav.size)
    assert (rc, fok, ferr) == (0, len(spec.frames), 0) and np.array_equal(back, b.wav)
    # every frame encodes on its own to the bytes it has in the stream (what a table of frames in any order is held against)
    for i in range(len(spec.frames)):
        rc, one, _ = O.encode(b.frames[i], po)
        assert rc == 0 and np.array_equal(one, b.x3[b.offsets[i]:b.offsets[i + 1]])


def test_frame_hits_every_target_round_the_edge_in_every_arrangement():
    """frame() on its own: every arrangement at every bit count from 77 793 to 77 840, and what it refuses"""
    for arr in PC.ARRANGEMENTS:
        for bits in range(77793, 77841, 5):
            w = PC.frame(bits, 10000, None, arr, seed=bits)
            assert PC.frame_bits(w, O.Params.default()) == bits
            rc, s, _ = O.encode(w)
            assert rc == 0 and (int(s[6]) << 8 | int(s[7])) == PC.payload_len(bits) == s.size - 20
    with pytest.raises(ValueError):
        PC.frame(11000, 10000)           # fewer bits than silence has
    with pytest.raises(ValueError):
        PC.frame(8 * 20400, 10000)       # more than literal blocks have
    with pytest.raises(ValueError):
        PC.frame(77824, 10000, None, "sideways")
    assert [PC.payload_len(b) for b in (77808, 77809, 77824, 77825)] == [9726, 9728, 9728, 9730]
