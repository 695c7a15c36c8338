// x3_spectra_kernel.h -- SPECTRA: the exact integer STFT of int16 rows in HBM, on the matrix cores (x3_spectra_rows_dev;
// DESIGN.md section 29).  Row w is lens[w] samples at samples + offsets[w], as the ranges calls write them; frame r of it
// is samples [r * H, r * H + N), r < R(w) = len < N ? 0 : (len - N) / H + 1, and bin k <= N / 2 of a frame is
//     re = sum x[n] * cos[((n * k) mod N) * (1024 / N)],   im = the same against sin,
// int64 and exact, from the tone calls' table of 1 024 (cos, sin) int16 pairs.
//
// THE SPLIT.  A 16-bit value v is 256 * vh + vl + 128 with vh = v >> 8 and vl = (v & 255) - 128, both int8.  With
// X = 256 * xh + xl and C = 256 * ch + cl, x * c = (X + 128) * (C + 128), so over a frame
//     sum x * c = 65536 * hh + 256 * (hl + lh) + ll + 128 * sX + 128 * sC + 16384 * N,
// hh .. ll the four int8 dot products (each below N * 2^14 <= 2^24: exact in the int32 accumulators of
// v_mfma_i32_16x16x64_i8), sX = sum X the frame's own, sC = sum C the column's.
//
// Three kernels, one launch set:
//  x3_spectra_plan_kernel      -- one workgroup: R(w), its exclusive scan, the statuses, the caller's row offsets, the summary
//  x3_spectra_basis_kernel     -- the B operand from the caller's table, which is device data: built in every call.  Columns
//                                 come in TILE PAIRS: tile 2t holds cos of bins 16t .. 16t + 15, tile 2t + 1 their sin, so a
//                                 lane's accumulator slots of the two tiles belong to the same (frame, bin).  Bins behind
//                                 N / 2 are columns of zeros.  A tile's operand of K step s is 64 lanes x 16 bytes, twice (the
//                                 ch plane, the cl plane), in the order the transform's lanes load it; sC behind them.
//  x3_spectra_transform_kernel -- a workgroup per 16 * MT flat rows: the rows look up their own range (a tile may span
//                                 several), their samples go to LDS split into the two int8 planes, and the four waves share
//                                 the tile pairs: four accumulator chains per tile, N / 64 steps, then the epilogue in int64.
//                                 sX comes from two more chains against an operand of ones.  Rows behind R(w) of a padded
//                                 layout and the rows of a range with a status are stored as zeros by the same epilogue,
//                                 and a tile without a live row skips the staging and the matrix work.
//
// x3_spectra_levels_kernel.h (band levels, x3_spectra_levels_dev) takes from here the basis kernel as it is, x3sp_plan -- the
// plan kernel's body, with what a range takes in the output as a parameter -- x3sp_power, and x3sp_transform_tiles, the
// transform's tile loop with the row lookup and the epilogue's store as parameters.
//
// OPERAND LAYOUT (v_mfma_i32_16x16x64_i8): lane l holds A[row l & 15][16 bytes of K, group l >> 4] and
// B[the same 16 of K][column l & 15]; D[row 4 * (l >> 4) + j][column l & 15] in slot j.  A and B take their K from the same
// positions n = 64 * s + 16 * (l >> 4) + byte, so the order of K inside a step cannot matter.
//
// No atomics: every output word, status and offset has one writer.  No scratch.  Nothing trusts offsets, lengths or
// statuses: a range is read only when offsets[w] + lens[w] <= samples_cap, a frame r < R(w) ends inside its length; an
// output row index is below rows_cap (packed: a range is written only when row_off[w] + R(w) <= rows_cap; padded:
// n * stride <= rows_cap on the host); a range index comes from x3w_owner (below n) or from f / stride with f < n * stride.
#pragma once
#include "x3_decode_window_kernel.h"

#define X3SP_TABLE 1024

typedef int x3sp_v4i __attribute__((ext_vector_type(4)));

struct X3SpGeo {
  uint32_t N;        // n_fft: 64 .. 1024, a power of two
  uint32_t lgN;      // its log2
  uint32_t H;        // hop >= 1
  uint32_t B;        // N / 2 + 1 bins
  uint32_t KT;       // tile pairs: ceil(B / 16)
  uint32_t format;   // X3_SPECTRA_SUMS / X3_SPECTRA_POWER
};

__device__ __forceinline__ uint32_t x3sp_rows(uint32_t len, uint32_t N, uint32_t H) {
  return len < N ? 0u : (len - N) / H + 1u;
}

// ---- plan: one workgroup.  live[w]: the rows of range w that are transformed (0 for a range with a status); wr[w]: the
// rows of a packed range that are this call's to write (0: no room).  in_status may be status (in place): a thread reads
// its range's word before it writes it.  x3sp_plan is the body of both plan kernels: items(R) is what the range's R frames
// take in the output -- R rows here, ceil(R / M) time bins in x3_spectra_levels_kernel.h -- and the scan, the fits rule, the
// statuses, the offsets and the summary run on that; live[w] stays the frames.  s: 1 024 words of LDS.
template <class Items>
__device__ __forceinline__ void x3sp_plan(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lens,
                                          const int32_t* in_status, uint64_t n, uint64_t samples_cap, const X3SpGeo& g,
                                          uint64_t stride, uint64_t rows_cap, unsigned long long* __restrict__ row_off,
                                          uint32_t* __restrict__ live, uint32_t* __restrict__ wr, uint64_t* __restrict__ out_off,
                                          int32_t* status, X3WinSummary* __restrict__ sum, unsigned long long* s, Items items) {
  unsigned long long bad = 0, first = ~0ull;
  unsigned long long F = 0, R = 0;   // the range's frames, and its rows in the output
  const unsigned long long total = x3w_scan_items(
      n, s, [&](uint64_t w) { return R = items(F = x3sp_rows(lens[w], g.N, g.H)); },
      [&](uint64_t w, unsigned long long run) {
        const bool fits = stride ? R <= stride : (run <= rows_cap && R <= rows_cap - run);
        const uint64_t off = offsets[w], len = lens[w];
        int32_t st = in_status ? in_status[w] : X3D_OK;
        if (st == X3D_OK && (off > samples_cap || len > samples_cap - off)) st = X3D_BAD_ARG;
        if (st == X3D_OK && !fits) st = X3D_BAD_ARG;
        status[w] = st;
        row_off[w] = run;
        if (out_off) out_off[w] = stride ? w * stride : run;
        live[w] = st == X3D_OK ? (uint32_t)F : 0u;
        wr[w] = fits ? (uint32_t)R : 0u;
        if (st != X3D_OK) {
          ++bad;
          first = min(first, (unsigned long long)(w << 8) | ((uint32_t)st & 0xFFu));
        }
      });
  if (threadIdx.x == 0) {
    row_off[n] = total;
    if (out_off) out_off[n] = stride ? n * stride : total;
  }
  unsigned long long n_bad;
  (void)x3w_block_excl_scan(bad, s, &n_bad);
  s[threadIdx.x] = first;
  __syncthreads();
  for (uint32_t d = blockDim.x >> 1; d; d >>= 1) {
    if (threadIdx.x < d) s[threadIdx.x] = min(s[threadIdx.x], s[threadIdx.x + d]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sum->n_bad = n_bad;
    sum->first = s[0];
    sum->replays = 0;
    sum->total = total;
  }
}

__global__ void __launch_bounds__(1024)
x3_spectra_plan_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lens, const int32_t* in_status,
                       uint64_t n, uint64_t samples_cap, X3SpGeo g, uint64_t stride, uint64_t rows_cap,
                       unsigned long long* __restrict__ row_off, uint32_t* __restrict__ live, uint32_t* __restrict__ wr,
                       uint64_t* __restrict__ out_off, int32_t* status, X3WinSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  x3sp_plan(offsets, lens, in_status, n, samples_cap, g, stride, rows_cap, row_off, live, wr, out_off, status, sum, s,
            [](unsigned long long R) { return R; });
}

// ---- basis: a lane per (tile T, step s, operand lane l): its 16 bytes of either plane; the first 32 * KT lanes also sum
// their column.  basis[((T * S + s) * 2 + plane) * 64 + l], S = N / 64; colsum[T * 16 + c] = sum over n of (256 * ch + cl).
__device__ __forceinline__ int32_t x3sp_basis_value(const int16_t* __restrict__ table, const X3SpGeo& g, uint32_t T, uint32_t c,
                                                    uint32_t n) {
  const uint32_t k = (T >> 1) * 16u + c;
  if (k >= g.B) return 0;
  const uint32_t idx = ((n * k) & (g.N - 1u)) * ((uint32_t)X3SP_TABLE >> g.lgN);   // (n < 1024, k <= 512: no wrap)
  return table[2u * idx + (T & 1u)];
}

__global__ void __launch_bounds__(256)
x3_spectra_basis_kernel(const int16_t* __restrict__ table, X3SpGeo g, uint4* __restrict__ basis, int32_t* __restrict__ colsum) {
  const uint32_t S = g.N >> 6, tiles = 2u * g.KT;
  const uint32_t items = tiles * S * 64u, cols = tiles * 16u;
  const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x, lanes = gridDim.x * blockDim.x;
  for (uint32_t i = i0; i < items; i += lanes) {
    const uint32_t l = i & 63u, s = (i >> 6) % S, T = (i >> 6) / S;
    const uint32_t n0 = 64u * s + 16u * (l >> 4);
    uint32_t h[4] = {0, 0, 0, 0}, lo[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
      const uint32_t v = (uint32_t)x3sp_basis_value(table, g, T, l & 15u, n0 + j);
      h[j >> 2] |= ((v >> 8) & 0xFFu) << (8u * (j & 3u));
      lo[j >> 2] |= ((v & 0xFFu) ^ 0x80u) << (8u * (j & 3u));
    }
    uint4* const at = basis + ((size_t)(T * S + s) * 2u) * 64u + l;
    at[0] = make_uint4(h[0], h[1], h[2], h[3]);
    at[64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
  for (uint32_t col = i0; col < cols; col += lanes) {
    int32_t sc = 0;
    for (uint32_t n = 0; n < g.N; ++n) sc += x3sp_basis_value(table, g, col >> 4, col & 15u, n) - 128;   // (256 * ch + cl = c - 128)
    colsum[col] = sc;
  }
}

// ---- transform
#define X3SP_ROW_WRITE 1u   // the row is this call's to write
#define X3SP_ROW_LIVE 2u    // ... and its frame is transformed (otherwise: zeros)

__device__ __forceinline__ x3sp_v4i x3sp_mfma(x3sp_v4i a, x3sp_v4i b, x3sp_v4i c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

// The adapter's ms at n = N, word for word (x3_tone_power_levels_dev): a = re >> 15, b = im >> 15, P = a * a + b * b,
// ms = min(2^30, floor(floor(2 * P / N) / N)); N is a power of two and P >= 0, so the divisions are shifts.
__device__ __forceinline__ uint32_t x3sp_power(int64_t re, int64_t im, uint32_t lgN) {
  const int64_t a = re >> 15, b = im >> 15;
  const uint64_t P = (uint64_t)(a * a) + (uint64_t)(b * b);   // (|re| <= N * 2^30: a * a <= 2^50)
  const uint64_t ms = ((2u * P) >> lgN) >> lgN;
  return (uint32_t)min(ms, (uint64_t)1u << 30);
}

// LDS: the rows' samples as two int8 planes, a row RS = N + 16 bytes apart (16 rows of one operand read then hit 16
// different 16-byte slots of the banks); dynamic, 2 * 16 * MT * RS bytes.
// THE TILE LOOP BELOW HAS A TWIN: x3sp_transform_tiles, behind this kernel, is the same loop with the row lookup and the
// store as parameters (the band levels' kernels run it).  A change to the staging, the sums or the K loop is made in both.
template <int MT>
__global__ void __launch_bounds__(256)
x3_spectra_transform_kernel(const int16_t* __restrict__ samples, const uint64_t* __restrict__ offsets, uint64_t n, X3SpGeo g,
                            uint64_t stride, uint64_t rows_cap, const unsigned long long* __restrict__ row_off,
                            const uint32_t* __restrict__ live, const uint32_t* __restrict__ wr, const uint4* __restrict__ basis,
                            const int32_t* __restrict__ colsum, void* __restrict__ out) {
  constexpr uint32_t ROWS = 16u * MT;
  extern __shared__ uint4 x3sp_lds[];
  __shared__ uint64_t s_src[ROWS];
  __shared__ uint32_t s_flags[ROWS];
  uint8_t* const planes = reinterpret_cast<uint8_t*>(x3sp_lds);
  const uint32_t RS = g.N + 16u, S = g.N >> 6;
  uint8_t* const plane_h = planes;
  uint8_t* const plane_l = planes + (size_t)ROWS * RS;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t lc = lane & 15u, lg = lane >> 4;
  const uint64_t n_flat = stride ? n * stride : min((uint64_t)row_off[n], rows_cap);
  const uint64_t n_tiles = (n_flat + ROWS - 1u) / ROWS;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();   // (the tile before is read out of LDS)
    uint32_t flags = 0;
    if (t < ROWS) {
      const uint64_t f = tile * ROWS + t;
      uint64_t src = 0;
      if (f < n_flat) {
        uint64_t w, r;
        if (stride) {
          w = f / stride, r = f - w * stride;
          flags = X3SP_ROW_WRITE;
        } else {
          w = x3w_owner(row_off, n, f), r = f - row_off[w];
          flags = r < wr[w] ? X3SP_ROW_WRITE : 0u;
        }
        if (flags && r < live[w]) {
          flags |= X3SP_ROW_LIVE;
          src = offsets[w] + r * g.H;   // (r < R(w): [src, src + N) lies inside the range, the range inside samples_cap)
        }
      }
      s_src[t] = src;
      s_flags[t] = flags;
    }
    const int any_live = __syncthreads_or((int)(flags & X3SP_ROW_LIVE));
    x3sp_v4i sx[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) sx[m] = x3sp_v4i{0, 0, 0, 0};
    if (any_live) {
      // staging: 16 threads a row, four samples a thread and step; a row without a frame holds zeros
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const uint32_t row = (uint32_t)m * 16u + (t >> 4);
        const bool lv = (s_flags[row] & X3SP_ROW_LIVE) != 0u;
        const int16_t* const x = samples + s_src[row];
        for (uint32_t q = t & 15u; q < (g.N >> 2); q += 16u) {
          uint32_t h = 0, lo = 0;
          if (lv) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
              const uint32_t v = (uint16_t)x[4u * q + j];
              h |= (v >> 8) << (8u * j);
              lo |= ((v & 0xFFu) ^ 0x80u) << (8u * j);
            }
          }
          *reinterpret_cast<uint32_t*>(plane_h + (size_t)row * RS + 4u * q) = h;
          *reinterpret_cast<uint32_t*>(plane_l + (size_t)row * RS + 4u * q) = lo;
        }
      }
      __syncthreads();
      // sX of the lane's four frames per row tile: the two planes against ones
      const x3sp_v4i ones = x3sp_v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        x3sp_v4i sh = x3sp_v4i{0, 0, 0, 0}, sl = x3sp_v4i{0, 0, 0, 0};
        const size_t at = (size_t)((uint32_t)m * 16u + lc) * RS + 16u * lg;
        for (uint32_t s = 0; s < S; ++s) {
          sh = x3sp_mfma(*reinterpret_cast<const x3sp_v4i*>(plane_h + at + 64u * s), ones, sh);
          sl = x3sp_mfma(*reinterpret_cast<const x3sp_v4i*>(plane_l + at + 64u * s), ones, sl);
        }
        sx[m] = sh * 256 + sl;
      }
    }
    for (uint32_t tp = wave; tp < g.KT; tp += 4u) {
      x3sp_v4i acc[MT][2][4];   // [row tile][cos, sin][hh, hl, lh, ll]
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[m][p][c] = x3sp_v4i{0, 0, 0, 0};
      if (any_live) {
        const uint4* const bt = basis + (size_t)(2u * tp) * S * 128u + lane;   // (tile 2 * tp; the sin tile S * 128 behind it)
        for (uint32_t s = 0; s < S; ++s) {
          x3sp_v4i b[2][2];   // [cos, sin][ch, cl]
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const uint4 v = bt[((size_t)p * S + s) * 128u + (size_t)q * 64u];
              b[p][q] = x3sp_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
            }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const size_t at = (size_t)((uint32_t)m * 16u + lc) * RS + 16u * lg + 64u * s;
            const x3sp_v4i ah = *reinterpret_cast<const x3sp_v4i*>(plane_h + at);
            const x3sp_v4i al = *reinterpret_cast<const x3sp_v4i*>(plane_l + at);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              acc[m][p][0] = x3sp_mfma(ah, b[p][0], acc[m][p][0]);
              acc[m][p][1] = x3sp_mfma(ah, b[p][1], acc[m][p][1]);
              acc[m][p][2] = x3sp_mfma(al, b[p][0], acc[m][p][2]);
              acc[m][p][3] = x3sp_mfma(al, b[p][1], acc[m][p][3]);
            }
          }
        }
      }
      // epilogue: slot j of the lane is (row 4 * lg + j of the row tile, bin 16 * tp + lc) in the cos and the sin tile
      const uint32_t k = tp * 16u + lc;
      if (k < g.B) {
        const int64_t fix_re = 128ll * colsum[(2u * tp) * 16u + lc] + 16384ll * g.N;
        const int64_t fix_im = 128ll * colsum[(2u * tp + 1u) * 16u + lc] + 16384ll * g.N;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t row = (uint32_t)m * 16u + 4u * lg + (uint32_t)j;
            const uint32_t fl = s_flags[row];
            if (!(fl & X3SP_ROW_WRITE)) continue;
            int64_t re = 0, im = 0;
            if (fl & X3SP_ROW_LIVE) {
              const int64_t fx = 128ll * sx[m][j];
              re = 65536ll * acc[m][0][0][j] + 256ll * ((int64_t)acc[m][0][1][j] + acc[m][0][2][j]) + acc[m][0][3][j] + fx + fix_re;
              im = 65536ll * acc[m][1][0][j] + 256ll * ((int64_t)acc[m][1][1][j] + acc[m][1][2][j]) + acc[m][1][3][j] + fx + fix_im;
            }
            const uint64_t f = tile * ROWS + row;   // (below n_flat <= rows_cap: the row has X3SP_ROW_WRITE)
            if (g.format == X3_SPECTRA_POWER) {
              reinterpret_cast<uint32_t*>(out)[f * g.B + k] = (fl & X3SP_ROW_LIVE) ? x3sp_power(re, im, g.lgN) : 0u;
            } else {
              int64_t* const pair = reinterpret_cast<int64_t*>(out) + 2u * (f * g.B + k);   // (8-byte aligned, no more)
              pair[0] = re;
              pair[1] = im;
            }
          }
        }
      }
    }
  }
}

// x3sp_transform_tiles: the tile loop above -- the tiles grid-stride, the staging, the frames' own sums, the K loop and the
// int64 sums of every (row, bin) -- with what a row is and what becomes of a bin as parameters, for the kernels that do not
// store a row per frame (x3_spectra_levels_kernel.h):
//   rows(f, &src) -> the flags of flat row f < n_flat and, for a live one, the sample position of its frame (called by
//                    thread f mod ROWS);
//   sink.word(tile, row, k, flags, re, im) takes bin k < B of a row that has X3SP_ROW_WRITE (re = im = 0 unless it is live);
//   sink.tile_done(tile) runs once behind a tile's last word, by every thread.
// s_src, s_flags: ROWS words of LDS each.  x3_spectra_transform_kernel keeps its own text: instantiated through this
// template the compiler orders its prologue differently (seven instructions more), and the rows call's kernels stay what
// they were, instruction for instruction.
template <int MT, class Rows, class Sink>
__device__ __forceinline__ void x3sp_transform_tiles(const int16_t* __restrict__ samples, const X3SpGeo g, uint64_t n_flat,
                                                     const uint4* __restrict__ basis, const int32_t* __restrict__ colsum,
                                                     uint8_t* planes, uint64_t* s_src, uint32_t* s_flags, Rows rows, Sink sink) {
  constexpr uint32_t ROWS = 16u * MT;
  const uint32_t RS = g.N + 16u, S = g.N >> 6;
  uint8_t* const plane_h = planes;
  uint8_t* const plane_l = planes + (size_t)ROWS * RS;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t lc = lane & 15u, lg = lane >> 4;
  const uint64_t n_tiles = (n_flat + ROWS - 1u) / ROWS;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();   // (the tile before is read out of LDS)
    uint32_t flags = 0;
    if (t < ROWS) {
      const uint64_t f = tile * ROWS + t;
      uint64_t src = 0;
      if (f < n_flat) flags = rows(f, src);
      s_src[t] = src;
      s_flags[t] = flags;
    }
    const int any_live = __syncthreads_or((int)(flags & X3SP_ROW_LIVE));
    x3sp_v4i sx[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) sx[m] = x3sp_v4i{0, 0, 0, 0};
    if (any_live) {
      // staging: 16 threads a row, four samples a thread and step; a row without a frame holds zeros
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const uint32_t row = (uint32_t)m * 16u + (t >> 4);
        const bool lv = (s_flags[row] & X3SP_ROW_LIVE) != 0u;
        const int16_t* const x = samples + s_src[row];
        for (uint32_t q = t & 15u; q < (g.N >> 2); q += 16u) {
          uint32_t h = 0, lo = 0;
          if (lv) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
              const uint32_t v = (uint16_t)x[4u * q + j];
              h |= (v >> 8) << (8u * j);
              lo |= ((v & 0xFFu) ^ 0x80u) << (8u * j);
            }
          }
          *reinterpret_cast<uint32_t*>(plane_h + (size_t)row * RS + 4u * q) = h;
          *reinterpret_cast<uint32_t*>(plane_l + (size_t)row * RS + 4u * q) = lo;
        }
      }
      __syncthreads();
      // sX of the lane's four frames per row tile: the two planes against ones
      const x3sp_v4i ones = x3sp_v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        x3sp_v4i sh = x3sp_v4i{0, 0, 0, 0}, sl = x3sp_v4i{0, 0, 0, 0};
        const size_t at = (size_t)((uint32_t)m * 16u + lc) * RS + 16u * lg;
        for (uint32_t s = 0; s < S; ++s) {
          sh = x3sp_mfma(*reinterpret_cast<const x3sp_v4i*>(plane_h + at + 64u * s), ones, sh);
          sl = x3sp_mfma(*reinterpret_cast<const x3sp_v4i*>(plane_l + at + 64u * s), ones, sl);
        }
        sx[m] = sh * 256 + sl;
      }
    }
    for (uint32_t tp = wave; tp < g.KT; tp += 4u) {
      x3sp_v4i acc[MT][2][4];   // [row tile][cos, sin][hh, hl, lh, ll]
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[m][p][c] = x3sp_v4i{0, 0, 0, 0};
      if (any_live) {
        const uint4* const bt = basis + (size_t)(2u * tp) * S * 128u + lane;   // (tile 2 * tp; the sin tile S * 128 behind it)
        for (uint32_t s = 0; s < S; ++s) {
          x3sp_v4i b[2][2];   // [cos, sin][ch, cl]
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const uint4 v = bt[((size_t)p * S + s) * 128u + (size_t)q * 64u];
              b[p][q] = x3sp_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
            }
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const size_t at = (size_t)((uint32_t)m * 16u + lc) * RS + 16u * lg + 64u * s;
            const x3sp_v4i ah = *reinterpret_cast<const x3sp_v4i*>(plane_h + at);
            const x3sp_v4i al = *reinterpret_cast<const x3sp_v4i*>(plane_l + at);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              acc[m][p][0] = x3sp_mfma(ah, b[p][0], acc[m][p][0]);
              acc[m][p][1] = x3sp_mfma(ah, b[p][1], acc[m][p][1]);
              acc[m][p][2] = x3sp_mfma(al, b[p][0], acc[m][p][2]);
              acc[m][p][3] = x3sp_mfma(al, b[p][1], acc[m][p][3]);
            }
          }
        }
      }
      // epilogue: slot j of the lane is (row 4 * lg + j of the row tile, bin 16 * tp + lc) in the cos and the sin tile
      const uint32_t k = tp * 16u + lc;
      if (k < g.B) {
        const int64_t fix_re = 128ll * colsum[(2u * tp) * 16u + lc] + 16384ll * g.N;
        const int64_t fix_im = 128ll * colsum[(2u * tp + 1u) * 16u + lc] + 16384ll * g.N;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t row = (uint32_t)m * 16u + 4u * lg + (uint32_t)j;
            const uint32_t fl = s_flags[row];
            if (!(fl & X3SP_ROW_WRITE)) continue;
            int64_t re = 0, im = 0;
            if (fl & X3SP_ROW_LIVE) {
              const int64_t fx = 128ll * sx[m][j];
              re = 65536ll * acc[m][0][0][j] + 256ll * ((int64_t)acc[m][0][1][j] + acc[m][0][2][j]) + acc[m][0][3][j] + fx + fix_re;
              im = 65536ll * acc[m][1][0][j] + 256ll * ((int64_t)acc[m][1][1][j] + acc[m][1][2][j]) + acc[m][1][3][j] + fx + fix_im;
            }
            sink.word(tile, row, k, fl, re, im);
          }
        }
      }
    }
    sink.tile_done(tile);
  }
}
