// x3_tune_kernel.h -- the tuning pass: the exact encoded size of one input under every candidate parameter set, in one
// read of the samples (include/x3hip.h, "Parameter tuning").
//
// Candidates: codes (0, 1, 3), block length 10, 20 or 40 (g = 0, 1, 2), t0 in 0..6, t1 in t0..10, t2 in 15..27 -- 728
// triples per block length, index g * 728 + the triple's lexicographic rank.  All share one frame length spf (a multiple
// of 40), so a block of 40 is two of 20 and four of 10, each counted from frame sample 1.
//
// A block's bits (encoder.rs:289-315, the wave encoder's x3w_analyse): Rice when m = max|d| <= t2, 2 + cnt (k + 1) +
// sum(zigzag >> k) with k = code[[m > t0] + [m > t1]]; otherwise the escape E, BFP 6 + cnt (nb + 1) with nb = bits of m
// below 15, else literal 6 + 16 cnt.  With t0 <= t1 <= t2 that is, per block,
//     E + [m <= t2] (R3 - E) + [m <= t1] (R1 - R3) + [m <= t0] (R0 - R1),         Rk = 2 + cnt (k + 1) + sum(zigzag >> k)
// -- separable in the three thresholds.  So a frame's bits under candidate (g; t0, t1, t2) are
//     16 + SE[g] + G0[g][t0] + G1[g][t1] + G2[g][t2 - 15]
// with SE = the frame's sum of E and Gx[t] the sums of the differences over the blocks with m <= t: 32 numbers per block
// length, 96 per frame.  A lane keeps them in registers for the chunks of 40 samples it takes, no histogram and no atomic
// (silence and noise cost what any content costs), the wave adds them up by DPP at the frame's end, and each lane then
// prices 35 of the 2 184 candidates: 20 + 2 ceil(bits / 16) bytes into the workgroup's 64-bit totals in LDS, the payload
// into its maxima.  A workgroup flushes its totals to the tuner's once, at its end.
#pragma once
#include "x3_device.h"

// (the encoders' packed helpers of x3_encode_common.h, which comes with kernels of its own)
__device__ __forceinline__ uint32_t x3t_pk_sub_sat(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_sub_i16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t x3t_pk_min_i16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_min_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t x3t_pk_max_i16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <int SH>
__device__ __forceinline__ uint32_t x3t_pk_shr_u16(uint32_t a) {
  uint32_t r;
  asm("v_pk_lshrrev_b16 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "i"(SH), "v"(a));
  return r;
}

typedef uint32_t x3t_v4u32 __attribute__((ext_vector_type(4)));
typedef uint32_t x3t_v2u32 __attribute__((ext_vector_type(2)));

#define X3T_CANDIDATES 2184u
#define X3T_TRIPLES 728u
#define X3T_WAVES 8u
#define X3T_THREADS (64u * X3T_WAVES)
#define X3T_SUMS 32u   // per block length: SE, G0[0..6], G1[0..10], G2[15..27]

struct X3TuneArgs {
  const int16_t* wav;
  uint64_t n_per_clip, clip_stride, n_frames;
  uint32_t spf, fpc;
  unsigned long long* tot;  // X3T_CANDIDATES byte totals
  uint32_t* maxpay;         // X3T_CANDIDATES largest frame payloads
};

// sum over the wave's 64 lanes (every lane active); the total is in lane 63
__device__ __forceinline__ uint32_t x3t_wave_sum63(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8: lane 15 of a row = its sum
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 into rows 1, 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 into rows 2, 3
  return v;
}

// one block into a lane's sums S[0..31] of its block length: m = max|d| (>= 0x10000: no block), cnt samples, z0 / z1 / z3 =
// the sums of zigzag >> 0 / 1 / 3 (meaningful when m <= 27, the only case that reads them)
__device__ __forceinline__ void x3t_block(uint32_t (&S)[X3T_SUMS], uint32_t m, uint32_t cnt, uint32_t z0, uint32_t z1, uint32_t z3) {
  const uint32_t nb = 32u - (uint32_t)__clz((int)m);
  const uint32_t esc = cnt == 0u ? 0u : nb < 15u ? 6u + cnt * (nb + 1u) : 6u + 16u * cnt;
  const uint32_t r0 = 2u + cnt + z0, r1 = 2u + 2u * cnt + z1, r3 = 2u + 4u * cnt + z3;
  const uint32_t d0 = r0 - r1, d1 = r1 - r3, d2 = r3 - esc;   // (mod 2^32: the totals come out right)
  S[0] += esc;
#pragma unroll
  for (uint32_t t = 0; t < 7u; ++t) S[1 + t] += m <= t ? d0 : 0u;
#pragma unroll
  for (uint32_t t = 0; t < 11u; ++t) S[8 + t] += m <= t ? d1 : 0u;
#pragma unroll
  for (uint32_t t = 0; t < 13u; ++t) S[19 + t] += m <= 15u + t ? d2 : 0u;
}

__global__ void __launch_bounds__(X3T_THREADS) x3_tune_kernel(X3TuneArgs a) {
  __shared__ unsigned long long s_tot[X3T_CANDIDATES];
  __shared__ uint32_t s_max[X3T_CANDIDATES];
  __shared__ uint32_t s_trip[X3T_TRIPLES];                  // t0 | t1 << 8 | t2 << 16
  __shared__ uint32_t s_sum[X3T_WAVES][3 * X3T_SUMS];      // a wave's frame, summed over its lanes
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  for (uint32_t k = tid; k < X3T_CANDIDATES; k += X3T_THREADS) {
    s_tot[k] = 0;
    s_max[k] = 0;
  }
  for (uint32_t r = tid; r < X3T_TRIPLES; r += X3T_THREADS) {
    uint32_t t0 = 0, rem = r;
    while (rem >= (11u - t0) * 13u) rem -= (11u - t0++) * 13u;
    s_trip[r] = t0 | ((t0 + rem / 13u) << 8) | ((15u + rem % 13u) << 16);
  }
  __syncthreads();

  const uint64_t waves = (uint64_t)gridDim.x * X3T_WAVES;
  for (uint64_t f = (uint64_t)blockIdx.x * X3T_WAVES + w; f < a.n_frames; f += waves) {
    const uint64_t clip = f / a.fpc, idx = f % a.fpc;
    const uint64_t left = a.n_per_clip - idx * a.spf;
    const uint32_t n = left < a.spf ? (uint32_t)left : a.spf;
    // the frame's samples through a range-checked descriptor on the dword in front of them: dwords behind the frame read
    // as zero; sh = 1 when the frame starts in the middle of a dword
    const uintptr_t fa = (uintptr_t)(a.wav + clip * a.clip_stride + idx * a.spf);
    const uint32_t sh = (uint32_t)(fa >> 1) & 1u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(fa & ~(uintptr_t)3), 0,
                                                                        (int)((2u * (n + sh) + 3u) & ~3u), 0x00020000);
    uint32_t S[3][X3T_SUMS];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (uint32_t i = 0; i < X3T_SUMS; ++i) S[g][i] = 0;
    const uint32_t nchunks = (n - 1u + 39u) / 40u;   // chunk c = frame samples 40c + 1 .. 40c + 40, predicted from 40c
    for (uint32_t c = lane; c < nchunks; c += 64u) {
      uint32_t X[22];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const x3t_v4u32 q = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(80u * c + 16u * i), 0, 0);
        X[4 * i] = q.x; X[4 * i + 1] = q.y; X[4 * i + 2] = q.z; X[4 * i + 3] = q.w;
      }
      const x3t_v2u32 q = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(80u * c + 80u), 0, 0);
      X[20] = q.x; X[21] = q.y;
      // P[j] = (s[40c + 2j], s[40c + 2j + 1])
      if (sh) {
#pragma unroll
        for (int j = 0; j < 21; ++j) X[j] = __builtin_amdgcn_alignbit(X[j + 1], X[j], 16);
      }
      const uint32_t rem = min(n - 1u - 40u * c, 40u);   // samples of the chunk inside the frame
      uint32_t m[4], z0[4], z1[4], z3[4], cnt[4];
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        uint32_t mx = 0, mn = 0, a0 = 0, a1 = 0, a3 = 0;
#pragma unroll
        for (int jj = 0; jj < 5; ++jj) {
          const int j = 5 * q4 + jj;
          const uint32_t nx = __builtin_amdgcn_alignbit(X[j + 1], X[j], 16);   // (s[2j + 1], s[2j + 2])
          uint32_t d = x3t_pk_sub_sat(nx, X[j]);
          const uint32_t keep = (2u * j < rem ? 0x0000FFFFu : 0u) | (2u * j + 1u < rem ? 0xFFFF0000u : 0u);
          d &= keep;
          mx = x3t_pk_max_i16(mx, d);
          mn = x3t_pk_min_i16(mn, d);
          const uint32_t z = x3_pk_shl_b16_1(d) ^ x3_pk_ashr_i16_15(d);
          a0 = x3_pk_add_u16(a0, z);
          a1 = x3_pk_add_u16(a1, x3t_pk_shr_u16<1>(z));
          a3 = x3_pk_add_u16(a3, x3t_pk_shr_u16<3>(z));
        }
        const uint32_t ab = x3t_pk_max_i16(mx, x3t_pk_sub_sat(0u, mn));
        m[q4] = max(ab & 0xFFFFu, ab >> 16);
        z0[q4] = (a0 & 0xFFFFu) + (a0 >> 16);
        z1[q4] = (a1 & 0xFFFFu) + (a1 >> 16);
        z3[q4] = (a3 & 0xFFFFu) + (a3 >> 16);
        const int32_t r = (int32_t)rem - 10 * q4;
        cnt[q4] = r <= 0 ? 0u : r >= 10 ? 10u : (uint32_t)r;
      }
      const uint32_t NONE = 0x10000u;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) x3t_block(S[0], cnt[q4] ? m[q4] : NONE, cnt[q4], z0[q4], z1[q4], z3[q4]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t c2 = cnt[2 * h] + cnt[2 * h + 1];
        x3t_block(S[1], c2 ? max(m[2 * h], m[2 * h + 1]) : NONE, c2, z0[2 * h] + z0[2 * h + 1], z1[2 * h] + z1[2 * h + 1],
                  z3[2 * h] + z3[2 * h + 1]);
      }
      x3t_block(S[2], max(max(m[0], m[1]), max(m[2], m[3])), cnt[0] + cnt[1] + cnt[2] + cnt[3], z0[0] + z0[1] + z0[2] + z0[3],
                z1[0] + z1[1] + z1[2] + z1[3], z3[0] + z3[1] + z3[2] + z3[3]);
    }
    // the frame's 96 sums: lane 63 writes them, the wave's own DS instructions execute in order
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (uint32_t i = 0; i < X3T_SUMS; ++i) S[g][i] = x3t_wave_sum63(S[g][i]);
    if (lane == 63u) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (uint32_t i = 0; i < X3T_SUMS; ++i) s_sum[w][g * X3T_SUMS + i] = S[g][i];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t k = lane; k < X3T_CANDIDATES; k += 64u) {
      const uint32_t g = k / X3T_TRIPLES, tr = s_trip[k - g * X3T_TRIPLES];
      const uint32_t* s = &s_sum[w][g * X3T_SUMS];
      const uint32_t bits = 16u + s[0] + s[1 + (tr & 0xFFu)] + s[8 + ((tr >> 8) & 0xFFu)] + s[19 + (tr >> 16) - 15u];
      const uint32_t pay = 2u * ((bits + 15u) >> 4);
      atomicAdd(&s_tot[k], (unsigned long long)(20u + pay));
      atomicMax(&s_max[k], pay);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  for (uint32_t k = tid; k < X3T_CANDIDATES; k += X3T_THREADS) {
    if (s_tot[k]) {
      atomicAdd(&a.tot[k], s_tot[k]);
      atomicMax(&a.maxpay[k], s_max[k]);
    }
  }
}
