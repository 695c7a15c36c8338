// x3_spectra_levels_kernel.h -- SPECTRA, band levels: the POWER words of x3_spectra_kernel.h's transform folded into bands
// and summed over M = frames_per_bin consecutive frames, one x3_level per (time bin, band), and no row per frame anywhere
// (x3_spectra_levels_dev).  Range w has R(w) frames and T(w) = ceil(R(w) / M) time bins; time bin j
// holds frames [j * M, min((j + 1) * M, R(w))); band b of frame r is
//     bp = min(2^30, sum over the bins k with bin_band[k] == b of ms[r][k])           (64 bits, then the clamp)
// and the record is {sum_sq = sum of bp, sum = 0, min = -peak, max = peak = min(32767, isqrt(2 * max of bp)), n = frames}.
// Plane b of the output is levels + b * plane_stride; the rows of a plane are the time bins, laid as the rows call lays
// its rows (packed at the exclusive sum of T(w), or padded to a stride).
//
// Three kernels of its own behind x3_spectra_basis_kernel, one launch set:
//  x3_spectra_levels_plan_kernel      -- one workgroup: x3sp_plan with T(w) as a range's item, so the scan, the statuses, the
//                                        caller's offsets and the summary are the rows call's; then the same scan once more
//                                        over the frames of the ranges without a status: frame_off, n + 1 words.
//  x3_spectra_levels_init_kernel      -- the identity into every record the call owns, in every plane.
//  x3_spectra_levels_transform_kernel -- x3sp_transform_tiles over the FRAMES of frame_off: a flat row is a frame that is
//                                        transformed, so no tile is without one.  Its sink stores nothing per frame: a lane
//                                        adds its ms into acc[row of the tile][band] in LDS (64-bit adds: the four waves hold
//                                        different bins of the same rows, and a band's sum passes 2^32).  Behind a barrier
//                                        thread b walks band b down the tile's rows: it clamps each frame's sum, joins the
//                                        consecutive frames that share an output record, and issues one set of global atomics
//                                        per (tile, record, band): add on sum_sq and n, max on max, min on min.  It clears its
//                                        accumulators on the way, so the workgroup's next tile starts from zeros.
//
// Integer atomics commute: the records do not depend on the order of the tiles.  isqrt is monotone, so the max of the
// peaks is the peak of the max.  No scratch.  Nothing trusts bin_band (a word >= K is dropped), offsets, lengths or
// statuses: a flat frame f < frame_off[n] belongs to range w = x3w_owner(frame_off, n, f) < n with r = f - frame_off[w] <
// live[w] = R(w), which the plan set only for a range that lies inside samples_cap and whose T(w) rows have room below
// rows_cap (packed) or its stride (padded); its record's row is row_off[w] + r / M or w * stride + r / M, below rows_cap.
#pragma once
#include "x3_levels_kernel.h"
#include "x3_spectra_kernel.h"

struct X3SpFold {
  uint32_t M;              // frames per time bin, 1 .. 2^31 - 1
  uint32_t K;              // bands, 1 .. B
  uint64_t plane_stride;   // records between two planes, >= rows_cap
};

__global__ void __launch_bounds__(1024)
x3_spectra_levels_plan_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ lens, const int32_t* in_status,
                              uint64_t n, uint64_t samples_cap, X3SpGeo g, uint32_t M, uint64_t stride, uint64_t rows_cap,
                              unsigned long long* __restrict__ row_off, unsigned long long* __restrict__ frame_off,
                              uint32_t* __restrict__ live, uint32_t* __restrict__ wr, uint64_t* __restrict__ out_off,
                              int32_t* status, X3WinSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  x3sp_plan(offsets, lens, in_status, n, samples_cap, g, stride, rows_cap, row_off, live, wr, out_off, status, sum, s,
            [M](unsigned long long R) { return (R + M - 1u) / M; });
  __syncthreads();   // (thread 0 has read the summary's minimum out of s; live[w] is read by the thread that wrote it)
  const unsigned long long frames = x3w_scan_items(
      n, s, [&](uint64_t w) { return (unsigned long long)live[w]; }, [&](uint64_t w, unsigned long long run) { frame_off[w] = run; });
  if (threadIdx.x == 0) frame_off[n] = frames;
}

// the records the call owns: rows [0, min(total, rows_cap)) packed, [0, n * stride) padded, of every plane
__global__ void __launch_bounds__(256)
x3_spectra_levels_init_kernel(const unsigned long long* __restrict__ row_off, uint64_t n, uint64_t stride, uint64_t rows_cap,
                              X3SpFold fd, x3_level* __restrict__ levels) {
  const uint64_t rows = stride ? n * stride : min((uint64_t)row_off[n], rows_cap);
  const x3_level id = X3L_IDENTITY;
  for (uint32_t b = blockIdx.y; b < fd.K; b += gridDim.y)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (uint64_t)gridDim.x * blockDim.x)
      levels[b * fd.plane_stride + i] = id;
}

// the sink of the levels call: acc[row * K + band] in LDS, orow[row] the row's record in a plane (X3SPL_NO_ROW: no record yet)
#define X3SPL_NO_ROW 0xFFFFFFFFu

template <uint32_t ROWS>
struct X3SpLevelsSink {
  uint32_t lgN;
  X3SpFold fd;
  const uint32_t* __restrict__ bin_band;
  unsigned long long* acc;
  const uint32_t* orow;
  x3_level* levels;
  uint64_t n_flat;

  __device__ __forceinline__ void clear() const {
    for (uint32_t i = threadIdx.x; i < ROWS * fd.K; i += blockDim.x) acc[i] = 0ull;
  }
  __device__ __forceinline__ void word(uint64_t, uint32_t row, uint32_t k, uint32_t fl, int64_t re, int64_t im) const {
    if (!(fl & X3SP_ROW_LIVE)) return;
    const uint32_t band = bin_band[k];   // (k < B)
    if (band < fd.K) atomicAdd(acc + row * fd.K + band, (unsigned long long)x3sp_power(re, im, lgN));
  }
  // one record's share of this tile, band b: cnt frames, their clamped sum and the largest of them
  __device__ __forceinline__ void flush(uint32_t at, uint32_t b, uint32_t cnt, uint64_t sum, uint32_t top) const {
    x3_level* const rec = levels + (b * fd.plane_stride + at);
    const int32_t peak = (int32_t)min(x3l_isqrt(2ull * top), 32767u);
    atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sum_sq), (unsigned long long)sum);
    atomicAdd(&rec->n, cnt);
    atomicMax(&rec->max, peak);
    atomicMin(&rec->min, -peak);
  }
  __device__ __forceinline__ void tile_done(uint64_t tile) const {
    __syncthreads();   // (every wave's adds of this tile are in acc)
    const uint32_t rows = (uint32_t)min((uint64_t)ROWS, n_flat - tile * ROWS);   // (behind them: no frame, stale orow words)
    for (uint32_t b = threadIdx.x; b < fd.K; b += blockDim.x) {
      uint32_t at = X3SPL_NO_ROW, cnt = 0, top = 0;
      uint64_t sum = 0;
      for (uint32_t row = 0; row < rows; ++row) {
        const uint32_t o = orow[row];
        if (o != at) {
          if (cnt) flush(at, b, cnt, sum, top);
          at = o, cnt = 0, top = 0, sum = 0;
        }
        const uint32_t bp = (uint32_t)min(acc[row * fd.K + b], 1ull << 30);
        acc[row * fd.K + b] = 0ull;   // (the next tile's; the barrier at the tiles' top stands in between)
        sum += bp;
        top = max(top, bp);
        ++cnt;
      }
      if (cnt) flush(at, b, cnt, sum, top);
    }
  }
};

// dynamic LDS: the two planes of x3_spectra_transform_kernel, 2 * ROWS * (N + 16) bytes, then ROWS * K accumulators of 8
template <int MT>
__global__ void __launch_bounds__(256)
x3_spectra_levels_transform_kernel(const int16_t* __restrict__ samples, const uint64_t* __restrict__ offsets, uint64_t n,
                                   X3SpGeo g, X3SpFold fd, uint64_t stride, const unsigned long long* __restrict__ row_off,
                                   const unsigned long long* __restrict__ frame_off, const uint4* __restrict__ basis,
                                   const int32_t* __restrict__ colsum, const uint32_t* __restrict__ bin_band, x3_level* levels) {
  constexpr uint32_t ROWS = 16u * MT;
  extern __shared__ uint4 x3sp_lds[];
  __shared__ uint64_t s_src[ROWS];
  __shared__ uint32_t s_flags[ROWS];
  __shared__ uint32_t s_orow[ROWS];
  uint8_t* const planes = reinterpret_cast<uint8_t*>(x3sp_lds);
  const uint64_t n_flat = frame_off[n];
  const X3SpLevelsSink<ROWS> sink{g.lgN, fd, bin_band, reinterpret_cast<unsigned long long*>(planes + 2u * (size_t)ROWS * (g.N + 16u)),
                                  s_orow, levels, n_flat};
  sink.clear();   // (the barrier at the tiles' top stands behind it)
  x3sp_transform_tiles<MT>(
      samples, g, n_flat, basis, colsum, planes, s_src, s_flags,
      [&](uint64_t f, uint64_t& src) {
        const uint64_t w = x3w_owner(frame_off, n, f), r = f - frame_off[w];   // (w < n, r < live[w] = R(w): the header)
        src = offsets[w] + r * g.H;
        s_orow[threadIdx.x] = (uint32_t)((stride ? w * stride : (uint64_t)row_off[w]) + r / fd.M);   // (below rows_cap < 2^31)
        return X3SP_ROW_WRITE | X3SP_ROW_LIVE;
      },
      sink);
}
