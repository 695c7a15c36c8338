// x3_decode_frame.h -- what a decoder does ONCE PER FRAME, in front of its hot loop, written once:
//
//  x3_frame_header_check   decoder::read_frame_header + the walk's length checks (also the check kernel's, on its own words)
//  x3_frame_wav_offset     where a frame's samples go: the caller's offset, or the batch layout
//  x3_frame_setup          header, sample count, payload length and output range of a lane's frame -> X3FrameSetup
//  x3_ring_origin          the 16-byte chunk a lane's input ring starts at -> X3RingOrigin
//  x3_ring_last_payload_chunk / x3_ring_last_stream_chunk   the two meanings of "the last chunk a lane may ask for"
//
// Who takes what: x3_decode_split_kernel, x3_decode_fast_kernel and the walker of x3_decode_blocks_kernel take all of it (the
// first two end their ring at the payload, the walker at the stream); x3_decode_lanes_kernel takes the setup and keeps its
// older ring of 64-bit virtual offsets; x3_decode_merge_kernel takes the offset rule, x3_seg_index_kernel (which trusts no
// header and has its own checks) the ring origin and the stream's last chunk.
#pragma once
#include "x3_device.h"

#define X3D_STREAM_ENDS_IN_FRAME (-1)  // quiet stop of the walk (decodefile.rs:107-116)

struct X3FrameMeta {
  uint32_t payload_len;
  uint32_t samples;
};

// 4 stream bytes at byte offset `o` of the 4-byte-aligned buffer xw, as a big-endian value;
// dwords at or beyond n_dw read as zero
__device__ __forceinline__ uint32_t x3_be32_at(const uint32_t* __restrict__ xw, uint64_t n_dw, uint64_t o) {
  const uint64_t j = o >> 2;
  const uint32_t sh = (uint32_t)(o & 3u) * 8u;
  const uint32_t a = j < n_dw ? x3_bswap32(xw[j]) : 0u;
  if (sh == 0) return a;
  const uint32_t b = (j + 1) < n_dw ? x3_bswap32(xw[j + 1]) : 0u;
  return (a << sh) | (b >> (32u - sh));
}

// decoder::read_frame_header (decoder.rs:69-118) + the walk's length checks (decodefile.rs:107-121) for
// the frame at byte offset `off`; same check order as the reference.
// ... on the five big-endian words of the header
// hc = CRC-16 of the first 16 header bytes, computed by the caller (table-free or from LDS tables)
__device__ __forceinline__ int32_t x3_frame_header_check_words(uint32_t h0, uint32_t h1, uint32_t h4, uint32_t hc,
                                                               uint64_t x3_len, uint64_t off, uint32_t& plen,
                                                               uint32_t& samples, uint32_t& pcrc, uint32_t n_ch = 1u) {
  samples = h1 >> 16;
  plen = h1 & 0xFFFFu;
  pcrc = h4 & 0xFFFFu;
  if ((h4 >> 16) != hc) return X3D_FRAME_HEADER_INVALID_HEADER_CRC;
  if ((h0 >> 16) != 0x7833u) return X3D_FRAME_HEADER_INVALID_KEY;
  // (n_ch > 1: the multi-channel extension -- the frame must say exactly n_ch; else the reference's test)
  if (n_ch == 1u ? (h0 & 0xFFu) > 1u : (h0 & 0xFFu) != n_ch) return X3D_MORE_THAN_ONE_CHANNEL;
  if (plen >= 0x7fe0u) return X3D_FRAME_LENGTH;
  if (off + 20 + plen > x3_len) return X3D_STREAM_ENDS_IN_FRAME;   // decodefile.rs:114-116
  if (plen > 24576u) return X3D_FRAME_HEADER_INVALID_PAYLOAD_LEN;  // decodefile.rs:118-121
  return X3D_OK;
}

__device__ __forceinline__ int32_t x3_frame_header_check(const uint32_t* __restrict__ xw, uint64_t n_dw,
                                                         uint64_t x3_len, uint64_t off, uint32_t& plen,
                                                         uint32_t& samples, uint32_t& pcrc) {
  plen = 0;
  samples = 0;
  pcrc = 0;
  if (off + 20 > x3_len) return X3D_STREAM_ENDS_IN_FRAME;
  const uint32_t h0 = x3_be32_at(xw, n_dw, off), h1 = x3_be32_at(xw, n_dw, off + 4);
  const uint32_t h2 = x3_be32_at(xw, n_dw, off + 8), h3 = x3_be32_at(xw, n_dw, off + 12);
  const uint32_t h4 = x3_be32_at(xw, n_dw, off + 16);
  uint32_t hc = 0xFFFFu;
  hc = x3_crc_be32(hc, h0);
  hc = x3_crc_be32(hc, h1);
  hc = x3_crc_be32(hc, h2);
  hc = x3_crc_be32(hc, h3);
  return x3_frame_header_check_words(h0, h1, h4, hc, x3_len, off, plen, samples, pcrc);
}

// The sample offset of frame f in the output: the caller's table, or the batch layout (frame f - clip * fpc of clip
// f / fpc, clips clip_stride samples apart).  x3_decode_merge_kernel replays a frame into the row this gives, which is the
// row the decoder validated: one rule for both.  (The encoders' src_off is another thing.)
__device__ __forceinline__ uint64_t x3_frame_wav_offset(uint64_t f, const X3Geom& g, const X3DevParams& p,
                                                        const uint64_t* __restrict__ wav_off) {
  if (wav_off) return wav_off[f];
  const uint64_t clip = f / g.fpc;
  return clip * g.clip_stride + (f - clip * g.fpc) * (uint64_t)p.spf;
}

// A lane's frame, as the lane-per-frame decoders and the blocks walker set it up.  active: the frame is there, its header
// holds, and it has samples, a payload and room in the output; st: why not, where it is not (X3D_OK for a lane without a
// frame).  samples and plen are the header's (zero where the stream ends in front of it) and p0 is the payload's first
// byte whether the frame is active or not: they are what the caller writes to meta[f].  A caller that goes on with an
// idle lane gives it harmless values of its own (p0 = 0, plen = 2, wo = 0).
struct X3FrameSetup {
  bool active;
  int32_t st;
  uint32_t samples, plen;
  uint64_t p0, wo;
};

// The header is validated here again (cheap, once per frame) so that a decoder does not depend on
// x3_frame_check_kernel: the payload-CRC pass runs CONCURRENTLY on a second stream and the two status arrays
// are merged afterwards (x3_decode_merge_kernel).
__device__ __forceinline__ X3FrameSetup x3_frame_setup(const uint8_t* __restrict__ x3, uint64_t x3_len,
                                                       const uint64_t* __restrict__ frame_off, uint64_t f, bool present,
                                                       const X3Geom& g, const uint64_t* __restrict__ wav_off,
                                                       const X3DevParams& p, uint64_t wav_cap) {
  X3FrameSetup s{present, X3D_OK, 0u, 2u, 0u, 0u};
  if (present) {
    // (the header is read in aligned dwords: from the 4-byte boundary at or below x3)
    const uint32_t a4 = (uint32_t)(reinterpret_cast<uintptr_t>(x3) & 3u);
    uint32_t pcrc_unused;
    s.st = x3_frame_header_check(reinterpret_cast<const uint32_t*>(x3 - a4), (x3_len + a4 + 3) >> 2, x3_len + a4,
                                 frame_off[f] + a4, s.plen, s.samples, pcrc_unused);
    s.p0 = frame_off[f] + 20;
    if (s.st != X3D_OK) {
      s.active = false;
    } else if (s.samples == 0 || s.plen < 2) {
      s.st = X3D_BAD_ARG;  // the reference panics (decoder.rs:42,47)
      s.active = false;
    } else {
      s.wo = x3_frame_wav_offset(f, g, p, wav_off);
      if (s.wo + s.samples > wav_cap) {
        s.st = X3D_BAD_ARG;  // slice index panic
        s.active = false;
      }
    }
  }
  return s;
}

// ---- the input ring's origin.  A lane streams its payload in aligned 16-byte chunks; positions are bytes from x3b, the
// lane's first chunk (a frame is < 64 KB): a 64-bit pointer per lane, 32-bit arithmetic on everything else, streams of any
// length.  abs_base is that chunk in bytes from the 16-byte boundary at or below x3 (the coordinates of
// x3_ring_last_stream_chunk), v_bits the byte of the first block header the lane parses (0..16).
//
// The first chunk is the one that holds that byte -- or the payload's LAST byte, where the bit stream starts at the very
// end of the payload (a frame of one sample; an index entry that points there) on a 16-byte boundary: the chunk behind
// the payload may be the first one behind the stream (found by the guard pages of x3_fence.h: until round 5 such a lane
// read its eight chunks from there, 128 bytes that nobody used and that nobody may have mapped).
// first_header_byte: payload byte of the lane's first block header -- 2, behind the raw first sample, or hb >> 3 of a
// segment-index entry; first_header_byte <= plen, plen >= 2.
struct X3RingOrigin {
  const uint8_t* x3b;
  uint32_t v_bits;
  uint64_t abs_base;
};

__device__ __forceinline__ X3RingOrigin x3_ring_origin(const uint8_t* __restrict__ x3, uint64_t p0, uint32_t plen,
                                                       uint32_t first_header_byte) {
  const uint32_t adj = (uint32_t)(reinterpret_cast<uintptr_t>(x3) & 15u);
  const uint64_t abs_bits = (uint64_t)adj + p0 + first_header_byte;
  const uint64_t abs_last = (uint64_t)adj + p0 + plen - 1u;   // the payload's last byte
  const uint64_t abs_base = (abs_bits < abs_last ? abs_bits : abs_last) & ~15ull;
  return {(x3 - adj) + abs_base, (uint32_t)(abs_bits - abs_base), abs_base};
}

// The last chunk a lane asks for (requests behind it repeat it), from x3b.  TWO meanings:
//
// the last chunk that holds PAYLOAD (v_end: the payload's end from x3b) -- the lane-per-frame kernels, where parser and
// valuer share one view of the ring and what lies behind the payload is never needed;
__device__ __forceinline__ uint32_t x3_ring_last_payload_chunk(uint32_t v_end) { return (v_end - 1u) & ~15u; }

// ... and the last chunk that holds STREAM -- the blocks walker and the walk-only kernel.
// The ring takes the STREAM as it comes -- behind the payload the next frame's bytes, up to the stream's last 16-byte
// chunk, which repeats from there on -- and the blocks kernel's decoders stage the very same bytes: a codeword is then
// parsed alike by walker and decoders wherever it stands.  (Until the soak of round 6 the walker stopped at the PAYLOAD's
// last chunk, as the lane-per-frame kernels do; there parser and valuer share one view.  Here a codeword whose zero run
// began in the payload's last bits was parsed on different bits by the two sides, and the frame was not flagged:
// tools/r6/repro_overread.py.)  What is read behind the payload still sends the frame to the reference's reader.
// (An idle lane's origin may lie behind a stream of a few bytes: chunk 0 then.)
__device__ __forceinline__ uint32_t x3_ring_last_stream_chunk(const uint8_t* __restrict__ x3, uint64_t x3_len,
                                                              uint64_t abs_base) {
  const uint64_t lastc_abs = ((reinterpret_cast<uintptr_t>(x3) & 15u) + x3_len - 1u) & ~15ull;   // (in the coordinates of abs_base)
  const uint64_t rel = lastc_abs > abs_base ? lastc_abs - abs_base : 0u;
  return rel > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)rel;
}
