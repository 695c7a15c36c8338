// x3_plane_events_kernel.h -- PLANE EVENTS: runs of rows that are loud in at least min_planes of K planes of level records
// (x3_plane_events_dev, x3_corpus_plane_events_dev).
//
// The events of x3_events_kernel.h on one synthetic row verdict.  Of section 17's seven kernels only the first and the last
// know what a record is; the five in between work on the hot bytes and the tile words and are launched as they are.
//
//  x3_plane_events_flag_kernel<false> -- a lane per row: the K records of the row, the rule's values per plane (kernel
//                                        arguments, uniform); the entry only of a row that reaches min_planes
//  x3_plane_events_flag_kernel<true>  -- the entry first: the values of plane t and entry e from thr[t * n_ent + e]
//  x3_plane_events_emit_kernel        -- a wave per piece: entry, start, len once; per plane the merged record and the
//                                        mask bit "loud in some row of the piece"; the fillers behind the last event
//
// LOUD is x3e_loud on the rule's values, which the host has held to their limits, and x3q_loud (x3_quantiles_kernel.h) on
// d_thr's, which nobody has: each value is tested against its limit first.  The emit kernel uses x3q_loud for both.
//
// Bounds.  A record is read at t * plane_stride + r in 64 bits with r < n_rows <= plane_stride < 2^31 and t < n_planes <= 8: plane
// t is the n_rows records at d_levels + t * plane_stride, so the (n_planes - 1) * plane_stride + n_rows records the header asks
// the caller for hold every read -- the records between n_rows and plane_stride are never read, behind the last plane they
// need not exist; thr at t * n_ent + e with e < n_ent by x3w_owner (n_ent 1 and
// e 0 in the stream form); an event level is written at t * cap + i with i < cap; the mask at i < cap.
#pragma once
#include "x3_quantiles_kernel.h"

// the planes of a call beside its rows (q.levels is plane 0); thr: nullptr, or the thresholds per (plane, entry)
struct X3EvPlanes {
  x3_plane_event_rule rule;                     // (max_bins: the host has put the default in, as in x3_event_rule)
  uint64_t stride;                              // records from one plane to the next, >= q.n_rows
  const x3_event_threshold* thr;
};

// the rule's two values of plane t: selects on a uniform t, so that the rule stays in scalar registers (no indexed copy)
__device__ __forceinline__ void x3p_values(const x3_plane_event_rule& k, uint32_t t, uint64_t* mean_sq_min, uint32_t* peak_min) {
  uint64_t m = 0;
  uint32_t p = 0;
#pragma unroll
  for (uint32_t j = 0; j < X3_EVENT_PLANES_MAX; ++j)
    if (j == t) {
      m = k.mean_sq_min[j];
      p = k.peak_min[j];
    }
  *mean_sq_min = m;
  *peak_min = p;
}

// ---- flag.  The loop over planes is unrolled over the compile-time maximum behind a uniform t < n_planes: rec[t] are
// registers, never an indexed array.  All K loads of a row are issued in front of the first test, so that their round trips
// overlap: K independent 32-byte loads a lane, a wave reading 2 KB contiguous per plane.
template <bool kThr>
__global__ void __launch_bounds__(256)
x3_plane_events_flag_kernel(X3EvRows q, X3EvPlanes pl, uint64_t n_tiles, uint8_t* __restrict__ hot,
                            uint32_t* __restrict__ tile_prev, uint32_t* __restrict__ tile_next) {
  const uint32_t K = pl.rule.n_planes;
  x3e_flag_tiles(q, [&](const X3EvRows& q, uint64_t r) {
    x3_level rec[X3_EVENT_PLANES_MAX];
    uint32_t loud = 0;
    if (kThr) {
      X3EvEntry en;
      if (!x3e_entry_of(q, r, &en)) return false;   // (en.e: below n_ent, 0 in the stream form)
      const uint64_t n_ent = q.ent ? q.n_ent : 1u;
      x3_event_threshold k[X3_EVENT_PLANES_MAX];
#pragma unroll
      for (uint32_t t = 0; t < X3_EVENT_PLANES_MAX; ++t)
        if (t < K) {
          rec[t] = q.levels[t * pl.stride + r];
          k[t] = pl.thr[t * n_ent + en.e];
        }
#pragma unroll
      for (uint32_t t = 0; t < X3_EVENT_PLANES_MAX; ++t)
        if (t < K) loud += x3q_loud(rec[t], k[t].mean_sq_min, k[t].peak_min) ? 1u : 0u;
      return loud >= pl.rule.min_planes;
    }
#pragma unroll
    for (uint32_t t = 0; t < X3_EVENT_PLANES_MAX; ++t)
      if (t < K) rec[t] = q.levels[t * pl.stride + r];
#pragma unroll
    for (uint32_t t = 0; t < X3_EVENT_PLANES_MAX; ++t)
      if (t < K)   // (the host has held the rule's values to their limits: x3e_loud, as in x3_events_flag_kernel)
        loud += x3e_loud(rec[t], x3_event_rule{pl.rule.mean_sq_min[t], pl.rule.peak_min[t], 0, 0, 0, 0, 0}) ? 1u : 0u;
    X3EvEntry en;
    return loud >= pl.rule.min_planes && x3e_entry_of(q, r, &en);
  }, n_tiles, hot, tile_prev, tile_next);
}

// ---- emit: x3_events_emit_kernel with a loop over planes inside the wave.  One kernel for both forms: a piece's values
// are uniform in its wave either way (the rule's, or thr's of the piece's entry), so the form is one uniform branch.
// A wave reads records only when the mask or the event levels are wanted.
__global__ void __launch_bounds__(256)
x3_plane_events_emit_kernel(X3EvRows q, X3EvPlanes pl, const uint32_t* __restrict__ run_first, const uint32_t* __restrict__ run_last,
                            const unsigned long long* __restrict__ piece_off, const X3EvSummary* __restrict__ sum, uint64_t cap,
                            uint32_t* __restrict__ entries, uint64_t* __restrict__ starts, uint32_t* __restrict__ lens,
                            uint32_t* __restrict__ ev_planes, x3_level* __restrict__ ev_levels) {
  const uint32_t lane = threadIdx.x & 63u, K = pl.rule.n_planes;
  const uint64_t n_runs = min((uint64_t)sum->n_runs, q.n_rows);
  const uint64_t n_emit = min((uint64_t)sum->count, cap), mb = pl.rule.max_bins;
  const uint64_t n_ent = q.ent ? q.n_ent : 1u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_emit; i += waves) {
    const uint64_t k = x3w_owner(piece_off, n_runs, i);   // (the run with piece_off[k] <= i < piece_off[k + 1])
    const uint64_t b1 = min((uint64_t)run_last[k], q.n_rows);
    const uint64_t p0 = min(run_first[k] + (i - piece_off[k]) * mb, b1), p1 = min(p0 + mb, b1);
    X3EvEntry en;
    (void)x3e_entry_of(q, min(p0, q.n_rows - 1u), &en);   // (en.e: below n_ent, 0 in the stream form)
    if (lane == 0) {
      const uint64_t lo = min(en.lo, p0), start = (p0 - lo) * q.bin_len, end = min((p1 - lo) * q.bin_len, en.n_samples);
      if (entries) entries[i] = (uint32_t)en.e;
      starts[i] = start;
      lens[i] = (uint32_t)min(end > start ? end - start : 0ull, 0xFFFFFFFFull);
    }
    if (!ev_planes && !ev_levels) continue;
    uint32_t mask = 0;
    for (uint32_t t = 0; t < K; ++t) {
      uint64_t mean_sq_min;
      uint32_t peak_min;
      if (pl.thr) {
        const x3_event_threshold v = pl.thr[t * n_ent + en.e];
        mean_sq_min = v.mean_sq_min;
        peak_min = v.peak_min;
      } else {
        x3p_values(pl.rule, t, &mean_sq_min, &peak_min);
      }
      const x3_level* __restrict__ plane = q.levels + t * pl.stride;
      X3LevAcc acc;
      acc.reset();
      bool loud = false;
      for (uint64_t r = p0 + lane; r < p1; r += 64u) {   // (p1 <= n_rows <= stride)
        const x3_level rec = plane[r];
        loud = loud || x3q_loud(rec, mean_sq_min, peak_min);
        X3LevAcc o;
        o.load(rec);
        acc.join(o);
      }
      if (__ballot(loud) != 0ull) mask |= 1u << t;
      if (ev_levels) {
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) {
          X3LevAcc o;
          o.sum_sq = (uint64_t)__shfl_xor((long long)acc.sum_sq, d, X3_WAVE);
          o.sum = (int64_t)__shfl_xor((long long)acc.sum, d, X3_WAVE);
          o.mn = __shfl_xor(acc.mn, d, X3_WAVE);
          o.mx = __shfl_xor(acc.mx, d, X3_WAVE);
          o.n = (uint32_t)__shfl_xor((int)acc.n, d, X3_WAVE);
          acc.join(o);
        }
        if (lane == 0) ev_levels[t * cap + i] = acc.record();
      }
    }
    if (lane == 0 && ev_planes) ev_planes[i] = mask;
  }
  const x3_level id = X3L_IDENTITY;
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = n_emit + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += lanes) {
    if (entries) entries[i] = 0u;
    starts[i] = 0ull;
    lens[i] = 0u;
    if (ev_planes) ev_planes[i] = 0u;
    if (ev_levels)
      for (uint32_t t = 0; t < K; ++t) ev_levels[t * cap + i] = id;
  }
}
