// x3_quantiles_kernel.h -- QUANTILES of level records per entry and thresholds from them (x3_level_quantiles_dev,
// x3_level_thresholds_dev and their corpus forms).  The events calls that take the thresholds
// (d_thr) are x3_events_kernel.h's: this header includes it for rows and entries, and for the limits of the two values.
//
// Rows and entries are the events calls' (x3e_entry_of).  A row COUNTS for its entry when it lies in one and its n != 0;
// its KEY is max(max, -min) clamped to 0 .. 32 768 (X3_LEVEL_KEY_PEAK) or min(floor(sum_sq / n), 2^30)
// (X3_LEVEL_KEY_MEAN_SQ): the largest peak_min / mean_sq_min at which x3e_loud still calls the row hot.  Quantile j of entry
// e is the key of rank floor((K(e) - 1) * q_ppm[j] / 1 000 000) among the entry's K(e) counting keys in ascending order.
//
// A segmented radix select, most significant digit first, digits of X3Q_DIGIT_BITS bits: 2 passes for the peak (its top
// digit, key >> 8, runs to 128), 4 for the mean square (key >> 24 runs to 64).  No workgroup waits for another:
//
//  x3_quantiles_key_kernel     -- a lane per row: (key, entry) as 8 bytes into the workspace, entry X3E_NONE for a row
//                                 that does not count; the summary's start values
//  x3_quantiles_hist_kernel    -- per pass, a lane per row in tiles of X3E_TILE: a row adds to bin digit(key) of histogram
//                                 (entry, j) when the key's higher digits are the prefix selected so far for (entry, j).
//                                 A tile whose counting rows share one entry adds in LDS and issues one global atomic per
//                                 non-zero bin; another tile adds to global memory directly.  In pass 0 there is no prefix
//                                 yet: one histogram an entry, (entry, 0), serves every j.
//  x3_quantiles_select_kernel  -- per pass, a workgroup per entry and a wave per j: the scan of the 256 bins; pass 0 takes
//                                 K as their sum and forms the rank; the digit that holds the rank goes into the prefix,
//                                 the rank becomes the rank inside that bin, the bins are cleared for the next pass.  After
//                                 the last pass the prefix is the value.
//  x3_quantiles_map_kernel     -- a lane per entry: x3_event_threshold from the two values by x3_threshold_rule
//
// Workspace (q_ws), from host-known arguments: 8 * n_rows bytes of (key, entry) + 4 * n_ent * n_q * 256 bytes of
// histograms + 8 * n_ent * n_q bytes of (prefix, rank) + 3 * 4 * n_ent bytes (the two values and K of a thresholds call) +
// the summary + 8 * (n_ent + 1) bytes of row prefix; each piece rounded to 256 bytes.
//
// Bounds: an entry number comes from x3w_owner (below n_ent whatever the prefix holds) behind the test lo <= r, or is 0 in
// the stream form; every histogram index is (e * n_q + j) * 256 + digit with e < n_ent, j < n_q, digit < 256.  An entry
// table overwritten after the build moves or empties entries and changes values, never an index.  Values, K and
// thresholds are written below n_ent only.
#pragma once
#include "x3_events_kernel.h"

#define X3Q_DIGIT_BITS 8u
#define X3Q_BINS 256u                  // 1 << X3Q_DIGIT_BITS; = X3E_TILE, so a lane of a tile owns a bin at the flush
#define X3Q_MAX_Q 8u
#define X3Q_PEAK_MAX X3E_PEAK_MAX       // a key's largest value is its threshold's limit
#define X3Q_MEAN_SQ_MAX X3E_MEAN_SQ_MAX
#define X3Q_DEAD 0xFFFFFFFFu           // a slot's rank: the entry has no counting row (ranks are below 2^31)

struct X3QSlot {                       // per (entry, j)
  uint32_t prefix, rank;               // the digits selected so far; the rank among the rows that share them
};
struct X3QSummary {
  unsigned long long n_empty, first_empty;   // entries with K == 0, the first of them (~0: none)
};
struct X3QPpm {
  uint32_t v[X3Q_MAX_Q];
};

// the key of a record that counts (n != 0)
__device__ __forceinline__ uint32_t x3q_key(const x3_level& r, int key) {
  if (key == X3_LEVEL_KEY_PEAK) {
    const int64_t peak = max((int64_t)r.max, -(int64_t)r.min);
    return (uint32_t)min(max(peak, (int64_t)0), (int64_t)X3Q_PEAK_MAX);
  }
  return (uint32_t)min(r.sum_sq / (uint64_t)r.n, (uint64_t)X3Q_MEAN_SQ_MAX);
}

// ---- key: a lane per row
__global__ void __launch_bounds__(256)
x3_quantiles_key_kernel(X3EvRows q, int key, uint2* __restrict__ keys, X3QSummary* __restrict__ sum) {
  if (sum && blockIdx.x == 0 && threadIdx.x == 0) *sum = X3QSummary{0ull, ~0ull};
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < q.n_rows; r += (uint64_t)gridDim.x * blockDim.x) {
    const x3_level rec = q.levels[r];
    X3EvEntry en;
    const bool counts = rec.n != 0u && x3e_entry_of(q, r, &en);
    keys[r] = counts ? make_uint2(x3q_key(rec, key), (uint32_t)en.e) : make_uint2(0u, X3E_NONE);
  }
}

// ---- histogram of pass `pass` of `passes`: digit = (key >> shift) & 255, shift = 8 * (passes - 1 - pass)
__global__ void __launch_bounds__(256)
x3_quantiles_hist_kernel(const uint2* __restrict__ keys, uint64_t n_rows, uint64_t n_tiles, uint64_t n_ent, uint32_t n_q,
                         uint32_t pass, uint32_t passes, const X3QSlot* __restrict__ slots, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_hist[X3Q_MAX_Q * X3Q_BINS];
  __shared__ uint32_t s_lo[4], s_hi[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t shift = X3Q_DIGIT_BITS * (passes - 1u - pass);
  const uint32_t nj = pass ? n_q : 1u;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t r = t * X3E_TILE + threadIdx.x;
    const uint2 ke = r < n_rows ? keys[r] : make_uint2(0u, X3E_NONE);
    const bool counts = ke.y != X3E_NONE && ke.y < n_ent;
    // the smallest and the largest entry among the tile's counting rows
    uint32_t lo = counts ? ke.y : X3E_NONE, hi = counts ? ke.y : 0u;
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) {
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, X3_WAVE));
      hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, X3_WAVE));
    }
    if (lane == 0) {
      s_lo[wv] = lo;
      s_hi[wv] = hi;
    }
    for (uint32_t j = 0; j < nj; ++j) s_hist[j * X3Q_BINS + threadIdx.x] = 0u;
    __syncthreads();
    lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    const bool one = lo == hi;          // (lo == X3E_NONE: no row counts, nothing is added either way)
    if (counts) {
      const uint32_t digit = (ke.x >> shift) & (X3Q_BINS - 1u);
      for (uint32_t j = 0; j < nj; ++j) {
        bool in = true;
        if (pass) {
          const X3QSlot sl = slots[(uint64_t)ke.y * n_q + j];
          in = sl.rank != X3Q_DEAD && (ke.x >> (shift + X3Q_DIGIT_BITS)) == sl.prefix;
        }
        if (in) {
          if (one) atomicAdd(&s_hist[j * X3Q_BINS + digit], 1u);
          else atomicAdd(&hist[((uint64_t)ke.y * n_q + j) * X3Q_BINS + digit], 1u);
        }
      }
    }
    __syncthreads();
    if (one && lo != X3E_NONE) {        // (lo is a counting row's entry: below n_ent)
      for (uint32_t j = 0; j < nj; ++j) {
        const uint32_t v = s_hist[j * X3Q_BINS + threadIdx.x];
        if (v) atomicAdd(&hist[((uint64_t)lo * n_q + j) * X3Q_BINS + threadIdx.x], v);
      }
    }
    __syncthreads();
  }
}

// ---- select: a workgroup of n_q waves per entry, wave j for quantile j
__global__ void __launch_bounds__(64 * X3Q_MAX_Q)
x3_quantiles_select_kernel(uint64_t n_ent, uint32_t n_q, X3QPpm ppm, uint32_t pass, uint32_t passes, uint32_t* __restrict__ hist,
                           X3QSlot* __restrict__ slots, uint32_t* __restrict__ values, uint32_t* __restrict__ counted,
                           X3QSummary* __restrict__ sum) {
  const uint32_t lane = threadIdx.x & 63u, j = threadIdx.x >> 6;
  const bool last = pass + 1u == passes;
  for (uint64_t e = blockIdx.x; e < n_ent; e += gridDim.x) {
    const uint64_t slot = e * n_q + j;
    const uint4 c = reinterpret_cast<const uint4*>(hist + (e * n_q + (pass ? j : 0u)) * X3Q_BINS)[lane];
    const uint32_t s = c.x + c.y + c.z + c.w;
    uint32_t incl = s;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, X3_WAVE);
      if (lane >= d) incl += up;
    }
    X3QSlot sl;
    if (pass == 0u) {
      const uint32_t K = (uint32_t)__shfl((int)incl, 63, X3_WAVE);
      sl.prefix = 0u;
      sl.rank = K ? (uint32_t)((uint64_t)(K - 1u) * ppm.v[j] / 1000000ull) : X3Q_DEAD;
      if (lane == 0 && j == 0u) {
        counted[e] = K;
        if (!K && sum) {
          atomicAdd(&sum->n_empty, 1ull);
          atomicMin(&sum->first_empty, (unsigned long long)e);
        }
      }
    } else {
      sl = slots[slot];
    }
    const uint32_t excl = incl - s;
    const bool mine = sl.rank != X3Q_DEAD && excl <= sl.rank && sl.rank < incl;   // (one lane at most: the bins' scan is monotone)
    if (mine) {
      uint32_t rk = sl.rank - excl, d = 0u;
      if (rk >= c.x) {
        rk -= c.x, d = 1u;
        if (rk >= c.y) {
          rk -= c.y, d = 2u;
          if (rk >= c.z) rk -= c.z, d = 3u;
        }
      }
      const uint32_t prefix = (sl.prefix << X3Q_DIGIT_BITS) | (lane * 4u + d);
      slots[slot] = X3QSlot{prefix, rk};
      if (last) values[slot] = prefix;
    }
    if (!__ballot(mine) && lane == 0) {   // no counting row (or a rank no bin holds): the value is 0
      slots[slot] = X3QSlot{0u, X3Q_DEAD};
      if (last) values[slot] = 0u;
    }
    __syncthreads();                      // (pass 0: every wave has read histogram (e, 0))
    if (!last) reinterpret_cast<uint4*>(hist + slot * X3Q_BINS)[lane] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---- map: thr = clamp(floor(value * mul / div) + add, 1, limit) for a criterion that is on and K != 0, else 0
__device__ __forceinline__ uint64_t x3q_map(uint32_t value, uint32_t mul, uint32_t div, uint32_t add, uint64_t limit) {
  const uint64_t t = (uint64_t)value * mul / div + add;   // (value <= 2^30, mul and add < 2^32: below 2^63)
  return min(max(t, (uint64_t)1), limit);
}

__global__ void __launch_bounds__(256)
x3_quantiles_map_kernel(uint64_t n_ent, x3_threshold_rule rule, const uint32_t* __restrict__ val_peak,
                        const uint32_t* __restrict__ val_mean_sq, const uint32_t* __restrict__ counted,
                        x3_event_threshold* __restrict__ thr) {
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_ent; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t K = counted[e];
    x3_event_threshold t{0ull, 0u, K};
    if (K && rule.peak_div)
      t.peak_min = (uint32_t)x3q_map(val_peak[e], rule.peak_mul, rule.peak_div, rule.peak_add, X3Q_PEAK_MAX);
    if (K && rule.mean_sq_div)
      t.mean_sq_min = x3q_map(val_mean_sq[e], rule.mean_sq_mul, rule.mean_sq_div, rule.mean_sq_add, X3Q_MEAN_SQ_MAX);
    thr[e] = t;
  }
}
