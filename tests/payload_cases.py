"""Frames with a chosen payload bit count (not a test module): content for the 9 728-byte edge that two encoders and two
decoders share (x3_encode_wave_kernel.h X3W_IMG_BYTES, x3_encode_stream2_kernel.h X3_DENSE_PAYLOAD_BYTES, `dense_grp` of
x3_decode_split_kernel.h and x3_decode_blocks_kernel.h).

A frame's payload is 16 bits for its first sample plus the bits of its blocks (encoder.rs:189-200), padded to an even
number of bytes (bitpacker.rs:124-132): L = (((bits + 7) >> 3) + 1) & ~1.  A block's bits depend on its first differences
and the parameters only, and are MEASURED here with the oracle's encode_block into a BitPacker over a scratch writer
(8 * byte_len + p_bit) -- no code table is restated.  frame() builds a frame from a palette of blocks:
  silence                              the cheapest block (Rice, all differences zero);
  alternating +d, -d                   a BFP block of width 6 .. 14 (d of that many bits);
  alternating +16 385, -16 385         a literal block;
and takes the last steps with single +1 and -1 differences in otherwise silent blocks.  The bit count of what it built is
measured again, block by block, before the frame is handed out: a target the palette cannot reach raises ValueError.

ARRANGEMENTS decide which lanes of a kernel carry the bits:
  wide_first   every wide block at the front of the frame (the short last block is a Rice block);
  wide_last    every wide block at the back (the short last block is wide as well);
  shuffled     the full blocks permuted by the seed; the short last block wide for an odd seed;
  last_wide    shuffled, the short last block wide  -- a wide field ends in the payload's last dword;
  last_rice    shuffled, the short last block Rice  -- a short codeword ends there.
"""
import ctypes as C
import functools
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np

import oracle_lib as O

ARRANGEMENTS = ("wide_first", "wide_last", "shuffled", "last_wide", "last_rice")
BFP_WIDTHS = tuple(range(6, 15))
LITERAL = "lit"
LITERAL_STEP = 16385
IMAGE_BYTES = 9728          # the wave encoder's image = the largest payload that is not dense


def payload_len(bits):
    """bytes of a payload of `bits` bits (bitpacker.rs:124-132: to a byte, then to an even number of bytes)"""
    return (((bits + 7) >> 3) + 1) & ~1


def bits_of_len(L):
    """(smallest, largest) bit count whose payload is L bytes (L even, > 0)"""
    return 8 * (L - 2) + 1, 8 * L


# ------------------------------------------------------------------ measuring with the oracle

_scratch = np.zeros(256, dtype=np.uint8)


def block_bits(block, prev, params):
    """bits the oracle's encode_block writes for `block` (int16 samples) behind the sample `prev`"""
    block = np.ascontiguousarray(block, dtype=np.int16)
    w, bp, ft = O.Writer(), O.BitPacker(), C.c_size_t(0)
    L = O.lib()
    L.x3o_writer_init(C.byref(w), _scratch.ctypes.data, _scratch.size)
    L.x3o_bp_new(C.byref(bp), C.byref(w))
    rc = L.x3o_encode_block(block.ctypes.data, block.size, int(prev), C.byref(bp), C.byref(params), C.byref(ft))
    if rc:
        raise ValueError("encode_block refused a block: %d" % rc)
    return 8 * bp.byte_len + bp.p_bit


def frame_bits(wav, params):
    """bits of the payload of the frame `wav`: 16 for the first sample + its blocks' (the last one shorter)"""
    wav = np.ascontiguousarray(wav, dtype=np.int16)
    bl = params.block_len
    return 16 + sum(block_bits(wav[s:s + bl], wav[s - 1], params) for s in range(1, wav.size, bl))


def _key(params):
    return (params.block_len, params.blocks_per_frame, tuple(params.codes), tuple(params.thresholds))


def _wide_step(kind):
    """the largest step of a wide block's alternating differences"""
    return LITERAL_STEP if kind == LITERAL else (1 << kind) - 1


@functools.lru_cache(maxsize=None)
def _cost(key, kind, length):
    """measured bits of a block of `length` samples: kind None = silence, "+1" / "-1" = silence with one such difference,
    6 .. 14 = BFP of that width, "lit" = literal"""
    params = O.Params.make(*key)
    d = np.zeros(length, dtype=np.int64)
    if kind in ("+1", "-1"):
        d[length // 2] = 1 if kind == "+1" else -1
    elif kind is not None:
        d[:] = _wide_step(kind) * np.where(np.arange(length) % 2 == 0, 1, -1)
    return block_bits(np.cumsum(d).astype(np.int16), 0, params)


# ------------------------------------------------------------------ one frame

def _plan(target_bits, n, key, final_wide, kind):
    """-> (wide full blocks, +1 steps, -1 steps) that reach target_bits with wide blocks of `kind`, or None"""
    bl = key[0]
    nbf, r = (n - 1) // bl, (n - 1) % bl      # full blocks, samples of the short last one
    if nbf == 0:
        return None
    cs, cw = _cost(key, None, bl), _cost(key, kind, bl)
    up, down = _cost(key, "+1", bl) - cs, _cost(key, "-1", bl) - cs     # what one +1 / one -1 adds to a silent block
    if r and (_cost(key, "+1", r) - _cost(key, None, r), _cost(key, "-1", r) - _cost(key, None, r)) != (up, down):
        return None
    need = target_bits - 16 - nbf * cs - (0 if not r else _cost(key, kind if final_wide else None, r))
    if need < 0 or up <= 0 or down <= 0 or cw <= cs:
        return None
    a = min(nbf, need // (cw - cs))
    need -= a * (cw - cs)
    p = need // up
    m, rest = divmod(need - p * up, down)
    room = (nbf - a) * bl + (r if r and not final_wide else 0)
    if rest or p + m > room:
        return None
    return a, p, m


def frame(target_bits, n, params=None, arrangement="shuffled", seed=0, wide=None):
    """-> int16[n]: a frame of n samples whose payload has exactly target_bits bits under `params` (an oracle_lib.Params;
    default: the default parameters).  wide: the kind of the wide blocks -- a BFP width 6 .. 14 or "lit"; None: one of the
    three narrowest kinds that reach the target, by the seed.  ValueError if the target cannot be reached."""
    params = params or O.Params.default()
    if arrangement not in ARRANGEMENTS:
        raise ValueError("arrangement: one of %s" % (ARRANGEMENTS,))
    key = _key(params)
    bl = key[0]
    if n < 1 or n > bl * key[1]:
        raise ValueError("a frame has 1 .. block_len * blocks_per_frame samples")
    rng = np.random.default_rng([seed, target_bits, n])
    nbf, r = (n - 1) // bl, (n - 1) % bl
    final_wide = bool(r) and (arrangement in ("wide_last", "last_wide") or (arrangement == "shuffled" and seed % 2 == 1))
    kinds = (wide,) if wide is not None else BFP_WIDTHS + (LITERAL,)
    plans = [(k, pl) for k in kinds for pl in (_plan(target_bits, n, key, final_wide, k),) if pl is not None]
    if not plans:
        raise ValueError("no frame of %d samples has %d bits (%s, wide %s)" % (n, target_bits, arrangement, wide))
    kind, (a, p, m) = plans[seed % min(len(plans), 3)]
    # the order of the full blocks
    is_wide = np.zeros(nbf, dtype=bool)
    if arrangement == "wide_first":
        is_wide[:a] = True
    elif arrangement == "wide_last":
        is_wide[nbf - a:] = True
    else:
        is_wide[rng.permutation(nbf)[:a]] = True
    lens = [bl] * nbf + ([r] if r else [])
    is_wide = list(is_wide) + ([final_wide] if r else [])
    # the +1 / -1 steps: anywhere in the silent samples
    silent_at = np.concatenate([np.arange(1 + bl * i, 1 + bl * i + ln) for i, (ln, w) in enumerate(zip(lens, is_wide)) if not w]
                               + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    diffs = np.zeros(n, dtype=np.int64)
    at = rng.choice(silent_at, size=p + m, replace=False) if p + m else np.zeros(0, dtype=np.int64)
    steps = np.array([1] * p + [-1] * m, dtype=np.int64)
    rng.shuffle(steps)
    diffs[at] = steps
    # the wide blocks: +d, -d, ... with d of the block's width, away from the nearer rail
    lo, hi = (LITERAL_STEP, LITERAL_STEP) if kind == LITERAL else (1 << (kind - 1), (1 << kind) - 1)
    diffs[0] = int(rng.integers(-1000, 1001))          # the first sample
    level = int(diffs[0])
    for i, (ln, w) in enumerate(zip(lens, is_wide)):
        s = 1 + bl * i
        if w:
            d = int(rng.integers(lo, hi + 1))
            diffs[s:s + ln] = (d if level <= 0 else -d) * np.where(np.arange(ln) % 2 == 0, 1, -1)
        level += int(diffs[s:s + ln].sum())
    walk = np.cumsum(diffs)
    if walk.min() < -32768 or walk.max() > 32767:
        raise ValueError("the walk leaves int16")
    wav = walk.astype(np.int16)
    got = frame_bits(wav, params)
    if got != target_bits:
        raise ValueError("built %d bits for a target of %d (%s, wide %s)" % (got, target_bits, arrangement, kind))
    wav.setflags(write=False)
    return wav


# ------------------------------------------------------------------ specs: streams of such frames

class FrameSpec(NamedTuple):
    target_bits: int
    n: int
    arrangement: str = "shuffled"
    seed: int = 0
    wide: Optional[Union[int, str]] = None


class StreamSpec(NamedTuple):
    name: str
    block_len: int
    blocks_per_frame: int
    frames: Tuple[FrameSpec, ...]

    @property
    def oparams(self):
        return O.Params.make(self.block_len, self.blocks_per_frame)

    @property
    def spf(self):
        return self.block_len * self.blocks_per_frame


def stream(frame_specs, params=None):
    """the frames of a list of FrameSpec, concatenated -> (int16 samples, [frame, ...]).  Frames are independent (each
    begins with its raw first sample); every frame but the last must be a whole frame of the parameters for an encoder
    to cut the samples into the same frames again."""
    params = params or O.Params.default()
    spf = params.block_len * params.blocks_per_frame
    frames = [frame(f.target_bits, f.n, params, f.arrangement, f.seed, f.wide) for f in frame_specs]
    if any(f.size != spf for f in frames[:-1]):
        raise ValueError("only the last frame of a stream may be short")
    wav = np.concatenate(frames)
    wav.setflags(write=False)
    return wav, frames


class Built(NamedTuple):
    spec: StreamSpec
    wav: np.ndarray          # the stream's samples
    frames: tuple            # ... frame by frame
    x3: np.ndarray           # the oracle's stream from start_pos 0
    stats: tuple             # ... and its statistics
    offsets: tuple           # byte offset of every frame in x3, and its end
    plens: tuple             # payload_len of every frame's header


@functools.lru_cache(maxsize=None)
def built(spec):
    """the samples of `spec` and the oracle's encoding of them (made once, shared, read-only)"""
    po = spec.oparams
    wav, frames = stream(spec.frames, po)
    rc, x3, stats = O.encode(wav, po)
    if rc:
        raise ValueError("the oracle refused %s: %d" % (spec.name, rc))
    offs, plens, pos = [], [], 0
    while pos < x3.size:
        offs.append(pos)
        plens.append(int(x3[pos + 6]) << 8 | int(x3[pos + 7]))
        pos += 20 + plens[-1]
    x3.setflags(write=False)
    return Built(spec, wav, tuple(frames), x3, tuple(int(v) for v in stats), tuple(offs + [pos]), tuple(plens))


EDGE_BITS = (77808, 77809, 77824, 77825)     # the last bit of L = 9 726, the first and last of 9 728, the first of 9 730


def spec_a():
    """every bit position round the edge: sixteen bit counts each for L = 9 726, 9 728 and 9 730, shuffled; two more
    arrangements at the four bit counts where L changes"""
    fs = [FrameSpec(b, 10000, "shuffled", 100 + b) for b in range(77793, 77841)]
    fs += [FrameSpec(b, 10000, arr, 200 + b) for arr in ("last_wide", "wide_first") for b in EDGE_BITS]
    return StreamSpec("A", 20, 500, tuple(fs))


def spec_b(part):
    """row boundaries of the image: L = 256 k - 2, 256 k and 256 k + 2 at their largest bit counts and L = 256 k at its
    smallest too, for every k = 6 .. 38 with k % 3 == part; the last frame a short one with L = 254, 256 or 258"""
    fs = []
    for k in range(6, 39):
        if k % 3 != part:
            continue
        arr = ARRANGEMENTS[k % len(ARRANGEMENTS)]
        for j, bits in enumerate((bits_of_len(256 * k - 2)[1], bits_of_len(256 * k)[1], bits_of_len(256 * k)[0],
                                  bits_of_len(256 * k + 2)[1])):
            fs.append(FrameSpec(bits, 10000, arr, 300 + 4 * k + j))
    fs.append(FrameSpec(bits_of_len(254 + 2 * part)[1], 1234, "last_wide" if part == 1 else "shuffled", 400 + part))
    return StreamSpec("B%d" % part, 20, 500, tuple(fs))


def specs_c():
    """a full image with half-empty lanes: a last frame of 6 001 samples, and of 5 121 (the second half's first block only),
    at 77 824 and 77 825 bits, in wide BFP and in literal blocks; a whole frame at the same bit count in front"""
    out = []
    for n, width in ((6001, 13), (5121, 14)):
        for bits in (77824, 77825):
            for wide in (width, LITERAL):
                out.append(StreamSpec("C%d_%d_%s" % (n, bits, wide), 20, 500,
                                      (FrameSpec(bits, 10000, "last_rice", 500 + n + bits),
                                       FrameSpec(bits, n, "shuffled", 600 + n + bits, wide))))
    return out


def spec_d(block_len):
    """block lengths 10 (x 1 000) and 40 (x 250): the bit counts where L changes, three arrangements"""
    fs = [FrameSpec(b, 10000, arr, 700 + block_len + b) for arr in ("shuffled", "last_wide", "wide_first") for b in EDGE_BITS]
    return StreamSpec("D%d" % block_len, block_len, 10000 // block_len, tuple(fs))


def spec_groups(one_dense):
    """two decoder groups of 64 frames, every frame at L = 9 728 (all sixteen bit counts): the first group wide_first, the
    second wide_last -- the most a group that is not dense can hold.  one_dense: frame 37 of each group at L = 9 730
    instead, which alone makes its whole group dense."""
    fs = []
    for g, arr in enumerate(("wide_first", "wide_last")):
        for i in range(64):
            bits = 77824 - (i * 7) % 16 if i % 4 else 77824
            if one_dense and i == 37:
                bits = 77825 + g * 15
            fs.append(FrameSpec(bits, 10000, arr, 800 + 64 * g + i))
    return StreamSpec("G_one_dense" if one_dense else "G_full", 20, 500, tuple(fs))


def stream_specs():
    """the streams that go through every encoder and decoder"""
    return [spec_a(), spec_b(0), spec_b(1), spec_b(2)] + specs_c() + [spec_d(10), spec_d(40)]


def group_specs():
    return [spec_groups(False), spec_groups(True)]


def all_specs():
    """every spec the GPU tests use"""
    return stream_specs() + group_specs()
