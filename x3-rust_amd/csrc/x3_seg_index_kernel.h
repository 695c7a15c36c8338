// x3_seg_index_kernel.h -- the SEGMENT INDEX of a stream somebody else wrote, by a walk that stores no sample
// (x3_seg_index_build_dev; include/x3hip.h "The SEGMENT INDEX").
//
// An index entry is where a block begins and the sample in front of it.  Both come out of walking the frame's codewords
// and adding up their values (decoder.rs:36-58 wraps the running sample in 16 bits); neither needs a sample to be
// written anywhere.  So: a frame per lane, the blocks in order, one 8-byte store per `sb` blocks -- and no other store,
// which is what made the per-lane window decoder slow (its stores share vmcnt with its refills: DESIGN.md section 10).
//
// Any x3_params the window calls take: block length, blocks per frame, codes and thresholds are run-time values
// (X3DevParams).  The codeword step is ONE path for all four block types -- zero run (0 for BFP), then nb bits (1 / 2 / 4
// with the terminating one for the Rice codes, E for BFP), the value by selects -- so that the lanes of a wave, whose blocks
// are of different types, do not take turns.  The arithmetic is x3w_block's (x3_decode_window_kernel.h), which is
// x3_replay_block's on plain frames.
//
// INPUT.  A lane's refills must not wait for each other's: every wait for a load is a wait for the wave's LAST load.  So
// the stream goes through a ring in LDS, X3X_RING_DW dwords per lane (word j of the lane in slot j & 63, the lanes
// interleaved: ring[slot * 64 + lane], no bank is hit twice), and it is topped up by the wave as a whole: at the top of
// every block ALL lanes park the 16-byte chunks they asked for one block earlier and ask for the next ones (up to
// X3X_REQ) -- the loads of a service are a block's walk old when they are waited for.  A lane that runs dry in between
// (a block of more than X3X_REQ chunks: literal blocks of 40 samples and more) serves itself at once, alone; that costs
// time only.  The reader keeps the next ring word in a register, so an LDS read is a refill old too when it is used.
//
// NOTHING IS TRUSTED.  The frame's offset and its header's two lengths are checked against x3_len before anything is
// read through them; chunks are aligned 16-byte pieces between the one that holds the payload's first codeword and the
// last one that holds a byte of the stream (x3_fence.h), whatever the bits ask for; an entry is stored only inside the
// frame's own nseg - 1 words.  A frame that is irregular in any way the fast decoders flag -- a decode error, a BFP width
// <= 5, a zero run of 32 bits or more, a block that ends behind the payload's last byte -- gets no valid entry from
// that point on and is counted.  Why is not reported: the consumers' check and fix-up kernels give the frame its status.
// Every word of the index is written (invalid entries as zero).
#pragma once
#include "x3_device.h"
#include "x3_decode_split_kernel.h"    // X3S_SEG_MAGIC, X3S_SEG_VALID: the index's layout
#include "x3_decode_window_kernel.h"   // x3w_be32_at

#define X3X_RING_DW 64u      // ring dwords per lane (16 KiB of LDS per wave)
#define X3X_REQ 4u           // 16-byte chunks a lane asks for per service
#define X3X_WAVES_PER_CU 8u  // grid = this many single-wave groups per CU at most (the frames beyond: grid-stride)

__global__ void __launch_bounds__(64)
x3_seg_index_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off, uint64_t F,
                    X3DevParams p, uint2* __restrict__ idx, uint32_t sb, uint32_t nseg,
                    unsigned long long* __restrict__ irregular) {
  __shared__ uint32_t ring[X3X_RING_DW * 64u];
  const uint32_t lane = threadIdx.x;
  const uint32_t pitch = nseg - 1u;
  if (blockIdx.x == 0 && lane == 0) idx[0] = make_uint2(X3S_SEG_MAGIC, sb);
  const uint64_t n_groups = (F + 63u) >> 6;
  for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const uint64_t f = grp * 64u + lane;
    const bool present = f < F;
    // ---- the frame: offset and header lengths against x3_len
    bool bad = !present;
    uint32_t samples = 0, plen = 0;
    uint64_t p0 = 0;
    if (present) {
      const uint64_t off = frame_off[f];
      if (len < 20u || off > len - 20u) {
        bad = true;
      } else {
        const uint32_t h1 = x3w_be32_at(x3, len, off + 4u);
        samples = h1 >> 16;
        plen = h1 & 0xFFFFu;
        p0 = off + 20u;
        bad = samples == 0u || plen < 2u || plen > len - p0;
      }
    }
    // blocks of the frame, the last entry it has (entry q is in front of block sb * q < nbf), the blocks in front of that
    const uint32_t nbf = bad ? 0u : (samples - 1u + p.block_len - 1u) / p.block_len;
    const uint32_t q_max = nbf ? min(pitch, (nbf - 1u) / sb) : 0u;
    uint32_t target = sb * q_max;
    uint2* const ent = idx + 1 + f * (uint64_t)pitch;   // (dereferenced by present lanes only)
    uint32_t next_q = 1;

    // ---- the ring and the reader.  Positions count from x3b, the aligned chunk that holds the first block header.
    const uint8_t* x3b = x3;
    uint32_t v_last = 0, d8 = 0, end_pos = 0;
    uint32_t wr = 0, rd = 0, nv = 0, pos = 0, npend = 0, nx = 0, last = 0;
    uint64_t win = 0;
    uint4 ld[X3X_REQ];
#pragma unroll
    for (uint32_t k = 0; k < X3X_REQ; ++k) ld[k] = make_uint4(0, 0, 0, 0);
    auto request = [&](uint32_t chunk) -> uint4 {   // (never behind the last chunk that holds stream: it repeats)
      const uint32_t a = chunk > (v_last >> 4) ? v_last : chunk << 4;
      return *reinterpret_cast<const uint4*>(x3b + a);
    };
    auto park = [&](const uint4& c) {
      ring[((wr + 0u) & (X3X_RING_DW - 1u)) * 64u + lane] = x3_bswap32(c.x);
      ring[((wr + 1u) & (X3X_RING_DW - 1u)) * 64u + lane] = x3_bswap32(c.y);
      ring[((wr + 2u) & (X3X_RING_DW - 1u)) * 64u + lane] = x3_bswap32(c.z);
      ring[((wr + 3u) & (X3X_RING_DW - 1u)) * 64u + lane] = x3_bswap32(c.w);
      wr += 4u;
    };
    auto park_pending = [&]() {
#pragma unroll
      for (uint32_t k = 0; k < X3X_REQ; ++k)
        if (k < npend) park(ld[k]);
      npend = 0;
    };
    auto next_word = [&]() -> uint32_t {   // ring word rd; a lane that has run dry serves itself
      if (rd >= wr) {
        if (npend) park_pending();
        else park(request(wr >> 2));
      }
      const uint32_t w = ring[(rd & (X3X_RING_DW - 1u)) * 64u + lane];
      ++rd;
      return w;
    };
    auto service = [&]() {   // (all lanes of the wave together)
      park_pending();
      const uint32_t fit = (X3X_RING_DW - (wr - rd)) >> 2;
      npend = fit < X3X_REQ ? fit : X3X_REQ;
#pragma unroll
      for (uint32_t k = 0; k < X3X_REQ; ++k)
        if (k < npend) ld[k] = request((wr >> 2) + k);
    };
    auto fill = [&]() {   // at least 32 valid bits in the window
      if (nv < 32u) {
        win |= (uint64_t)nx << (32u - nv);
        nv += 32u;
        nx = next_word();
      }
    };
    auto take = [&](uint32_t n) {
      win <<= n;
      nv -= n;
      pos += n;
    };
    if (target) {
      const X3RingOrigin ro = x3_ring_origin(x3, p0, plen, 2u);   // (x3_decode_frame.h; the byte behind the first sample)
      x3b = ro.x3b;
      v_last = x3_ring_last_stream_chunk(x3, len, ro.abs_base);
      d8 = 8u * ro.v_bits;                         // position of the first block header (payload bit 16)
      end_pos = d8 + 8u * plen - 16u;              // position of the payload's end
      last = x3w_be32_at(x3, len, p0) >> 16;
#pragma unroll
      for (uint32_t k = 0; k < X3X_REQ; ++k) ld[k] = request(k);
      npend = X3X_REQ;
      park_pending();
      rd = d8 >> 5;
      const uint32_t sh = d8 & 31u;
      const uint32_t a = next_word(), b = next_word();
      win = (((uint64_t)a << 32) | b) << sh;
      nv = 64u - sh;
      nx = next_word();
      pos = d8;
    }

    // ---- the walk: the wave steps block by block, a lane is in it while it has blocks in front of its last entry
    const uint32_t maxb = (uint32_t)__builtin_amdgcn_readfirstlane((int)x3_wave_max_u32(target));
    const uint32_t bl = p.block_len;
    for (uint32_t b = 0; b < maxb; ++b) {
      bool act = b < target;
      if (act) service();
      // block header (decoder.rs:138-144): 2 bits ftype; BFP: 4 bits E - 1
      bool rice = false, lit = false;
      uint32_t nb = 1, bound = 0, half = 0, n = 0;
      int32_t level = 1;
      if (act) {
        n = min(bl, samples - 1u - b * bl);
        fill();
        const uint32_t ftype = (uint32_t)(win >> 62);
        take(2u);
        if (ftype == 0u) {
          nb = ((uint32_t)(win >> 60)) + 1u;   // E
          take(4u);
          lit = nb == 16u;
          half = 1u << (nb - 1u);
          if (nb <= 5u) act = false, bad = true;
        } else {
          rice = true;
          nb = (1u << ftype) >> 1;             // 1, 2, 4: the sub-bits WITH the terminating one
          level = ftype == 1u ? 1 : 1 << p.k[ftype - 1u];
          bound = p.inv_len[ftype - 1u];
        }
      }
      for (uint32_t i = 0; i < bl; ++i) {
        if (act && i < n) {
          fill();
          const uint32_t t = (uint32_t)(win >> 32);
          const uint32_t z = rice ? (uint32_t)__clz((int)t) : 0u;   // (32 for a window of zeros)
          if (z >= 32u) {
            act = false, bad = true;   // the reference's reader differs from here on (x3_decode_replay.h)
          } else {
            take(z);
            fill();
            const uint32_t v = (uint32_t)(win >> 32) >> (32u - nb);
            take(nb);
            if (rice) {
              const int32_t ix = (int32_t)(int16_t)((int32_t)v + level * ((int32_t)z - 1));
              if (ix < 0 || (uint32_t)ix >= bound) {
                act = false, bad = true;
              } else {
                const uint32_t u = (uint32_t)ix;
                last = (last + ((u & 1u) ? 0u - ((u + 1u) >> 1) : (u >> 1))) & 0xFFFFu;
              }
            } else if (lit) {
              last = v;
            } else {
              last = (last + (v > half ? v - (half << 1) : v)) & 0xFFFFu;
            }
          }
        }
      }
      if (act && pos > end_pos) act = false, bad = true;   // read behind the payload
      if (bad) target = 0;
      if ((b + 1u) % sb == 0u && act) {   // in front of block b + 1 = sb * q, q <= q_max
        const uint32_t q = (b + 1u) / sb;
        ent[q - 1u] = make_uint2(pos - d8 + 16u, last | X3S_SEG_VALID);
        next_q = q + 1u;
      }
    }
    // ---- the entries the walk did not reach: not valid
    if (present)
      for (uint32_t q = next_q; q <= pitch; ++q) ent[q - 1u] = make_uint2(0u, 0u);
    const unsigned long long stopped = __ballot(present && bad);
    if (lane == 0 && stopped) atomicAdd(irregular, (unsigned long long)__popcll(stopped));
  }
}
