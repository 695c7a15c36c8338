// x3_events_kernel.h -- EVENTS: runs of loud bins of level records as ranges (entry, start, len), found on the device
// (x3_events_dev, x3_events_adaptive_dev, x3_plane_events_dev and their corpus forms; DESIGN.md sections 17, 19 and 28).
//
// The input is what the levels calls write: a record per bin (row), a corpus's rows entry after entry, in K PLANES of
// n_rows records each (X3EvPlanes; K == 1: the records of one levels call).  A plane is LOUD at a row when the record
// counted samples and meets the plane's two values (x3e_loud); a row is HOT when it belongs to an entry and is loud in at
// least min_planes planes.  The two values are the rule's, the same for every entry, or d_thr's per (plane, entry).  A RUN
// is a maximal set of hot rows of one entry whose gaps are at most join_bins cold rows; runs shorter than min_bins are
// dropped, the others padded by pad_bins rows, clipped to the entry, and cut into pieces of max_bins rows: the EVENTS, in
// order of (entry, start).  All integers.
//
// No workgroup waits for another: what a row needs from other tiles (the hot row in front of it and behind it, how many
// runs start and end in front of it) comes from tile totals that a one-workgroup kernel scans between two grid launches.
// Only the first and the last kernel know what a record is; the five in between work on the hot bytes and the tile words.
//
//  x3_events_flag_kernel<kThr, kPlanes> -- a lane per row: hot or not (a byte in the workspace); per tile its first and
//                             last hot row.  kThr: the values from d_thr (the entry first) or the rule's (the record
//                             first); kPlanes: the bound of the plane loop, 1 or X3_EVENT_PLANES_MAX
//  x3_events_near_kernel   -- one workgroup: per tile the last hot row in front of it and the first one behind it
//  x3_events_mark_kernel   -- a lane per hot row: does it start a run, does it end one (bits in its byte); counts per tile
//  x3_events_count_kernel  -- one workgroup: the exclusive scans of the tiles' counts; the number of runs
//  x3_events_table_kernel  -- a lane per row: the k-th start and the k-th end into the run tables
//  x3_events_runs_kernel   -- one workgroup: per run min_bins, padding, clipping; the exclusive scan of its pieces; the count
//  x3_events_emit_kernel   -- a wave per piece: entry, start, len and the merged record; the filler behind the last event
//  x3_plane_events_emit_kernel -- the same piece walk (x3e_emit_pieces); per plane the merged record and the mask bit
//                             "loud in some row of the piece"
//
// Bounds.  Nothing trusts the records, *d_total, the entry table or d_thr: a row's entry is looked up in the row prefix the
// device computed from the table (x3_corpus_levels_rows_kernel) and clipped to n_rows, every table index is below its
// table's size ("Bounds"), and only slots below cap are written.  A record is read at
// t * stride + r in 64 bits with r < n_rows <= stride < 2^31 and t < n_planes <= 8: plane t is the n_rows records at
// d_levels + t * stride, so the (n_planes - 1) * stride + n_rows records the header asks the caller for hold every read --
// the records between n_rows and stride are never read, behind the last plane they need not exist; thr at t * n_ent + e
// with e < n_ent by x3w_owner (n_ent 1 and e 0 in the stream form); an event level is written at t * cap + i with i < cap;
// the mask at i < cap.
#pragma once
#include "x3_levels_kernel.h"

#define X3E_TILE 256u           // rows of a tile = lanes of a workgroup (read-only option "events_tile_rows")
#define X3E_NONE 0xFFFFFFFFu    // "no hot row" (rows are numbered below 2^31)
#define X3E_HOT 1u              // a row's byte: hot, starts a run, ends a run
#define X3E_START 2u
#define X3E_END 4u
// the limits of a rule's or a threshold's two values (mean_sq_min * n stays below 2^62).  The kernels test d_thr's values
// against them, the host holds a rule's to them (EvVerdict, x3_decode.hip), and the quantiles' keys end there
// (X3Q_MEAN_SQ_MAX, X3Q_PEAK_MAX): this header is the one place all three include.
#define X3E_MEAN_SQ_MAX (1u << 30)
#define X3E_PEAK_MAX 32768u

struct X3EvSummary {
  unsigned long long count;     // events found (may exceed cap)
  unsigned long long n_runs;    // runs before min_bins
};

// the rows of a call: a stream's (ent == nullptr: one entry of min(n_rows, ceil(*d_total / bin_len)) rows) or a corpus's
struct X3EvRows {
  const x3_level* levels;
  uint64_t n_rows, bin_len;                     // (bin_len: 1 .. 2^32 - 1)
  const uint64_t* d_total;
  const x3_corpus_entry* ent;
  uint64_t n_ent;
  const unsigned long long* row_first;          // n_ent + 1 words, in the workspace
};

struct X3EvEntry {
  uint64_t e, lo, hi, n_samples;                // rows [lo, hi) of d_levels, hi <= n_rows
};

// the entry of row r < n_rows; false: the row belongs to none (then *en is the row alone, with no samples)
__device__ __forceinline__ bool x3e_entry_of(const X3EvRows& q, uint64_t r, X3EvEntry* en) {
  uint64_t e = 0, lo = 0, rows, ns;
  if (q.ent) {
    e = x3w_owner(q.row_first, q.n_ent, r);     // (below n_ent whatever the prefix holds; lo <= r is tested below)
    lo = q.row_first[e];
    ns = q.ent[e].n_samples;
    rows = x3l_entry_rows(ns, q.bin_len);
  } else {
    ns = *q.d_total;
    rows = ns / q.bin_len + (ns % q.bin_len ? 1u : 0u);
  }
  if (lo <= r && r - lo < rows) {
    *en = X3EvEntry{e, lo, lo + min(rows, q.n_rows - lo), ns};   // (lo <= r < n_rows)
    return true;
  }
  *en = X3EvEntry{0, r, r + 1u, 0};
  return false;
}

// the planes of a call beside its rows (q.levels is plane 0) and the verdict on a row: what the host has checked
// (EvVerdict, x3_decode.hip).  An events call is one plane with min_planes 1 and the stride n_rows.
struct X3EvPlanes {
  x3_plane_event_rule rule;                     // (max_bins: the host has put the default in)
  uint64_t stride;                              // records from one plane to the next, >= q.n_rows
  const x3_event_threshold* thr;                // nullptr: the rule's values; or the values per (plane, entry)
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

// LOUD: two values within their limits on one record (a value of 0: its criterion is off)
__device__ __forceinline__ bool x3e_loud(const x3_level& r, uint64_t mean_sq_min, uint32_t peak_min) {
  if (r.n == 0u) return false;
  const int64_t peak = max((int64_t)r.max, -(int64_t)r.min);
  return (mean_sq_min && r.sum_sq >= mean_sq_min * (uint64_t)r.n) || (peak_min && peak >= (int64_t)peak_min);
}
// ... values nobody has checked (d_thr's): one above its limit makes its criterion never hot, tested in front of the
// multiply; both 0 leaves the entry without hot rows
__device__ __forceinline__ bool x3e_loud_unchecked(const x3_level& r, uint64_t mean_sq_min, uint32_t peak_min) {
  return x3e_loud(r, mean_sq_min <= X3E_MEAN_SQ_MAX ? mean_sq_min : 0ull, peak_min <= X3E_PEAK_MAX ? peak_min : 0u);
}

// first and last set lane of a wave's ballot as rows from `base` on
__device__ __forceinline__ uint32_t x3e_first_of(unsigned long long m, uint32_t base) {
  return m ? base + (uint32_t)__ffsll((long long)m) - 1u : X3E_NONE;
}
__device__ __forceinline__ uint32_t x3e_last_of(unsigned long long m, uint32_t base) {
  return m ? base + 63u - (uint32_t)__clzll((long long)m) : X3E_NONE;
}

// ---- flag: a lane per row.  verdict(q, r): is row r < n_rows hot -- the rule on its record and its entry, each caller's own
template <class Verdict>
__device__ __forceinline__ void x3e_flag_tiles(const X3EvRows& q, Verdict verdict, uint64_t n_tiles, uint8_t* __restrict__ hot,
                                               uint32_t* __restrict__ tile_prev, uint32_t* __restrict__ tile_next) {
  __shared__ uint32_t s_first[4], s_last[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t r = t * X3E_TILE + threadIdx.x;
    bool h = false;
    if (r < q.n_rows) {
      h = verdict(q, r);
      hot[r] = h ? X3E_HOT : 0u;
    }
    const unsigned long long m = __ballot(h);
    if (lane == 0) {
      s_first[wv] = x3e_first_of(m, (uint32_t)(r - lane));
      s_last[wv] = x3e_last_of(m, (uint32_t)(r - lane));
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // (the tile's own first and last; the next kernel turns them into its neighbours')
      uint32_t first = X3E_NONE, last = X3E_NONE;
      for (uint32_t w = 0; w < 4u; ++w) {
        if (s_last[w] != X3E_NONE) last = s_last[w];
        if (s_first[3u - w] != X3E_NONE) first = s_first[3u - w];
      }
      tile_prev[t] = last;
      tile_next[t] = first;
    }
    __syncthreads();
  }
}

// The one flag kernel.  The loop over planes is unrolled over its compile-time bound behind a uniform t < K: rec[t] are
// registers, never an indexed array, and all K loads of a row are issued in front of the first test, so that their round
// trips overlap (K independent 32-byte loads a lane, a wave reading 2 KB contiguous per plane).  The rule's values
// (!kThr), which the host has held to their limits: the records first, the entry only of a row that reaches min_planes.
// d_thr's (kThr): the entry first, then the values of plane t and entry e from thr[t * n_ent + e].
template <bool kThr, uint32_t kPlanes>
__global__ void __launch_bounds__(256)
x3_events_flag_kernel(X3EvRows q, X3EvPlanes pl, uint64_t n_tiles, uint8_t* __restrict__ hot,
                      uint32_t* __restrict__ tile_prev, uint32_t* __restrict__ tile_next) {
  const uint32_t K = kPlanes == 1u ? 1u : pl.rule.n_planes, need = kPlanes == 1u ? 1u : pl.rule.min_planes;
  x3e_flag_tiles(q, [&](const X3EvRows& q, uint64_t r) {
    X3EvEntry en;
    if (kThr && !x3e_entry_of(q, r, &en)) return false;   // (en.e: below n_ent, 0 in the stream form)
    const uint64_t n_ent = q.ent ? q.n_ent : 1u;
    x3_level rec[kPlanes];
    x3_event_threshold k[kPlanes];
#pragma unroll
    for (uint32_t t = 0; t < kPlanes; ++t)
      if (t < K) {
        rec[t] = q.levels[t * pl.stride + r];
        if (kThr) k[t] = pl.thr[t * n_ent + en.e];
      }
    uint32_t loud = 0;
#pragma unroll
    for (uint32_t t = 0; t < kPlanes; ++t)
      if (t < K)
        loud += (kThr ? x3e_loud_unchecked(rec[t], k[t].mean_sq_min, k[t].peak_min)
                      : x3e_loud(rec[t], pl.rule.mean_sq_min[t], pl.rule.peak_min[t])) ? 1u : 0u;
    return loud >= need && (kThr || x3e_entry_of(q, r, &en));
  }, n_tiles, hot, tile_prev, tile_next);
}

// ---- near: tile_prev[t] = the last hot row in front of tile t, tile_next[t] = the first one behind it (exclusive scans
// of "the last one that is there" from the left and from the right); one workgroup, a run of tiles per thread
__global__ void __launch_bounds__(1024)
x3_events_near_kernel(uint64_t n_tiles, uint32_t* __restrict__ tile_prev, uint32_t* __restrict__ tile_next) {
  __shared__ uint32_t s_l[1024], s_f[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (n_tiles + blockDim.x - 1) / blockDim.x;
  const uint64_t a = min((uint64_t)t * per, n_tiles), b = min(a + per, n_tiles);
  uint32_t last = X3E_NONE, first = X3E_NONE;
  for (uint64_t i = a; i < b; ++i) {
    if (tile_prev[i] != X3E_NONE) last = tile_prev[i];
    if (first == X3E_NONE) first = tile_next[i];
  }
  s_l[t] = last;
  s_f[t] = first;
  __syncthreads();
  for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
    const uint32_t l = t >= d ? s_l[t - d] : X3E_NONE, f = t + d < blockDim.x ? s_f[t + d] : X3E_NONE;
    __syncthreads();
    if (s_l[t] == X3E_NONE) s_l[t] = l;
    if (s_f[t] == X3E_NONE) s_f[t] = f;
    __syncthreads();
  }
  uint32_t carry = t ? s_l[t - 1u] : X3E_NONE;
  for (uint64_t i = a; i < b; ++i) {
    const uint32_t own = tile_prev[i];
    tile_prev[i] = carry;
    if (own != X3E_NONE) carry = own;
  }
  carry = t + 1u < blockDim.x ? s_f[t + 1u] : X3E_NONE;
  for (uint64_t i = b; i > a; --i) {
    const uint32_t own = tile_next[i - 1u];
    tile_next[i - 1u] = carry;
    if (own != X3E_NONE) carry = own;
  }
}

// ---- mark: a hot row starts a run when no hot row of its entry lies within join_bins + 1 rows in front of it, and ends
// one symmetrically; tile_ns / tile_ne: how many of each the tile holds
__global__ void __launch_bounds__(256)
x3_events_mark_kernel(X3EvRows q, uint32_t join_bins, uint64_t n_tiles, uint8_t* __restrict__ hot,
                      const uint32_t* __restrict__ tile_prev, const uint32_t* __restrict__ tile_next,
                      uint32_t* __restrict__ tile_ns, uint32_t* __restrict__ tile_ne) {
  __shared__ uint32_t s_first[4], s_last[4], s_ns[4], s_ne[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t reach = (uint64_t)join_bins + 1u;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t r = t * X3E_TILE + threadIdx.x;
    const uint32_t base = (uint32_t)(r - lane);
    const bool h = r < q.n_rows && hot[r] != 0u;
    const unsigned long long m = __ballot(h);
    if (lane == 0) {
      s_first[wv] = x3e_first_of(m, base);
      s_last[wv] = x3e_last_of(m, base);
    }
    __syncthreads();
    bool start = false, end = false;
    if (h) {
      uint32_t prev = x3e_last_of(m & ((1ull << lane) - 1ull), base);
      for (uint32_t w = wv; prev == X3E_NONE && w > 0u; --w) prev = s_last[w - 1u];
      if (prev == X3E_NONE) prev = tile_prev[t];
      uint32_t next = x3e_first_of(m & ~((2ull << lane) - 1ull), base);
      for (uint32_t w = wv + 1u; next == X3E_NONE && w < 4u; ++w) next = s_first[w];
      if (next == X3E_NONE) next = tile_next[t];
      X3EvEntry en;
      (void)x3e_entry_of(q, r, &en);
      start = !(prev != X3E_NONE && prev >= en.lo && r - prev <= reach);
      end = !(next != X3E_NONE && next < en.hi && next - r <= reach);
      hot[r] = (uint8_t)(X3E_HOT | (start ? X3E_START : 0u) | (end ? X3E_END : 0u));
    }
    const uint32_t ns = (uint32_t)__popcll(__ballot(start)), ne = (uint32_t)__popcll(__ballot(end));
    if (lane == 0) {
      s_ns[wv] = ns;
      s_ne[wv] = ne;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      tile_ns[t] = s_ns[0] + s_ns[1] + s_ns[2] + s_ns[3];
      tile_ne[t] = s_ne[0] + s_ne[1] + s_ne[2] + s_ne[3];
    }
    __syncthreads();
  }
}

// ---- count: the tiles' counts become their exclusive scans (at most n_rows < 2^31 in all); the number of runs
__global__ void __launch_bounds__(1024)
x3_events_count_kernel(uint64_t n_tiles, uint32_t* __restrict__ tile_ns, uint32_t* __restrict__ tile_ne,
                       X3EvSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  unsigned long long total[2];
  uint32_t* const tabs[2] = {tile_ns, tile_ne};
#pragma unroll
  for (uint32_t k = 0; k < 2u; ++k) {
    uint32_t* const tab = tabs[k];
    total[k] = x3w_scan_items(
        n_tiles, s, [&](uint64_t i) { return (unsigned long long)tab[i]; },
        [&](uint64_t i, unsigned long long run) { tab[i] = (uint32_t)run; });
  }
  if (threadIdx.x == 0) sum->n_runs = min(total[0], total[1]);   // (equal: the k-th start and the k-th end are one run)
}

// ---- table: the k-th start to run_first[k], the k-th end to run_last[k] (k below the count of hot rows <= n_rows)
__global__ void __launch_bounds__(256)
x3_events_table_kernel(uint64_t n_rows, uint64_t n_tiles, const uint8_t* __restrict__ hot, const uint32_t* __restrict__ tile_ns,
                       const uint32_t* __restrict__ tile_ne, uint32_t* __restrict__ run_first, uint32_t* __restrict__ run_last) {
  __shared__ uint32_t s_ns[4], s_ne[4];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t r = t * X3E_TILE + threadIdx.x;
    const uint32_t f = r < n_rows ? hot[r] : 0u;
    const unsigned long long ms = __ballot((f & X3E_START) != 0u), me = __ballot((f & X3E_END) != 0u);
    if (lane == 0) {
      s_ns[wv] = (uint32_t)__popcll(ms);
      s_ne[wv] = (uint32_t)__popcll(me);
    }
    __syncthreads();
    uint32_t ks = tile_ns[t] + (uint32_t)__popcll(ms & below), ke = tile_ne[t] + (uint32_t)__popcll(me & below);
    for (uint32_t w = 0; w < wv; ++w) {
      ks += s_ns[w];
      ke += s_ne[w];
    }
    if ((f & X3E_START) && ks < n_rows) run_first[ks] = (uint32_t)r;
    if ((f & X3E_END) && ke < n_rows) run_last[ke] = (uint32_t)r;
    __syncthreads();
  }
}

// ---- runs: run k = hot rows first .. last becomes rows [b0, b1) in its tables (b0 == b1: dropped), piece_off[k] the
// events in front of it (n_runs + 1 words, 64-bit sums); the count to the caller and the summary.  One workgroup.
__global__ void __launch_bounds__(1024)
x3_events_runs_kernel(X3EvRows q, x3_event_rule rule, uint32_t* __restrict__ run_first, uint32_t* __restrict__ run_last,
                      unsigned long long* __restrict__ piece_off, X3EvSummary* __restrict__ sum, uint64_t* __restrict__ d_count) {
  __shared__ unsigned long long s[1024];
  const uint64_t n = min((uint64_t)sum->n_runs, q.n_rows);
  const uint64_t mb = rule.max_bins;   // (the host has put the default in: at least 1)
  auto pieces = [&](uint64_t k) { return (unsigned long long)(((uint64_t)run_last[k] - run_first[k] + mb - 1u) / mb); };
  unsigned long long mine = 0;
  x3w_own_items(n, [&](uint64_t k) {
    const uint64_t first = run_first[k], last = run_last[k];
    uint64_t b0 = 0, b1 = 0;
    if (first <= last && last < q.n_rows && last - first + 1u >= rule.min_bins) {
      X3EvEntry en;
      (void)x3e_entry_of(q, first, &en);
      b0 = first - min((uint64_t)rule.pad_bins, first - min(en.lo, first));
      b1 = min(last + 1u + rule.pad_bins, max(en.hi, last + 1u));
      b1 = min(b1, q.n_rows);
    }
    run_first[k] = (uint32_t)b0;
    run_last[k] = (uint32_t)b1;
    mine += (b1 - b0 + mb - 1u) / mb;
  });
  const unsigned long long total =
      x3w_scan_own_items(n, s, mine, pieces, [&](uint64_t k, unsigned long long run) { piece_off[k] = run; });
  if (threadIdx.x == 0) {
    piece_off[n] = total;
    sum->count = total;
    *d_count = total;
  }
}

// ---- emit: a wave per event below cap; then the filler into every slot behind them.  records(i, p0, p1, en): what the
// wave of event i does with the records of its rows [p0, p1), p1 <= n_rows, of entry en (every lane calls); fill(i): the
// caller's own outputs of a slot behind the last event.  Entry, start and len of either are written here.
template <class Records, class Fill>
__device__ __forceinline__ void x3e_emit_pieces(const X3EvRows& q, uint64_t mb, const uint32_t* __restrict__ run_first,
                                                const uint32_t* __restrict__ run_last, const unsigned long long* __restrict__ piece_off,
                                                const X3EvSummary* __restrict__ sum, uint64_t cap, uint32_t* __restrict__ entries,
                                                uint64_t* __restrict__ starts, uint32_t* __restrict__ lens, Records records, Fill fill) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_runs = min((uint64_t)sum->n_runs, q.n_rows);
  const uint64_t n_emit = min((uint64_t)sum->count, cap);
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
    records(i, p0, p1, en);
  }
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = n_emit + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += lanes) {
    if (entries) entries[i] = 0u;
    starts[i] = 0ull;
    lens[i] = 0u;
    fill(i);
  }
}

// (one plane and no mask: a record is merged, never tested; of the verdict it takes the runs' max_bins alone)
__global__ void __launch_bounds__(256)
x3_events_emit_kernel(X3EvRows q, x3_event_rule rule, const uint32_t* __restrict__ run_first, const uint32_t* __restrict__ run_last,
                      const unsigned long long* __restrict__ piece_off, const X3EvSummary* __restrict__ sum, uint64_t cap,
                      uint32_t* __restrict__ entries, uint64_t* __restrict__ starts, uint32_t* __restrict__ lens,
                      x3_level* __restrict__ ev_levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const x3_level id = X3L_IDENTITY;
  x3e_emit_pieces(q, rule.max_bins, run_first, run_last, piece_off, sum, cap, entries, starts, lens,
      [&](uint64_t i, uint64_t p0, uint64_t p1, const X3EvEntry&) {
        if (!ev_levels) return;
        X3LevAcc acc;
        acc.reset();
        for (uint64_t r = p0 + lane; r < p1; r += 64u) {
          X3LevAcc o;
          o.load(q.levels[r]);
          acc.join(o);
        }
        acc.join_wave();
        if (lane == 0) ev_levels[i] = acc.record();
      },
      [&](uint64_t i) {
        if (ev_levels) ev_levels[i] = id;
      });
}

// (K planes, or the mask of one.  One kernel for both forms of the values: a piece's are uniform in its wave either way
// -- the rule's, or thr's of the piece's entry -- so the form is one uniform branch, and x3e_loud_unchecked serves both.
// A wave reads records only when the mask or the event levels are wanted.)
__global__ void __launch_bounds__(256)
x3_plane_events_emit_kernel(X3EvRows q, X3EvPlanes pl, const uint32_t* __restrict__ run_first, const uint32_t* __restrict__ run_last,
                            const unsigned long long* __restrict__ piece_off, const X3EvSummary* __restrict__ sum, uint64_t cap,
                            uint32_t* __restrict__ entries, uint64_t* __restrict__ starts, uint32_t* __restrict__ lens,
                            uint32_t* __restrict__ ev_planes, x3_level* __restrict__ ev_levels) {
  const uint32_t lane = threadIdx.x & 63u, K = pl.rule.n_planes;
  const uint64_t n_ent = q.ent ? q.n_ent : 1u;
  const x3_level id = X3L_IDENTITY;
  x3e_emit_pieces(q, pl.rule.max_bins, run_first, run_last, piece_off, sum, cap, entries, starts, lens,
      [&](uint64_t i, uint64_t p0, uint64_t p1, const X3EvEntry& en) {
        if (!ev_planes && !ev_levels) return;
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
            loud = loud || x3e_loud_unchecked(rec, mean_sq_min, peak_min);
            X3LevAcc o;
            o.load(rec);
            acc.join(o);
          }
          if (__ballot(loud) != 0ull) mask |= 1u << t;
          if (ev_levels) {
            acc.join_wave();
            if (lane == 0) ev_levels[t * cap + i] = acc.record();
          }
        }
        if (lane == 0 && ev_planes) ev_planes[i] = mask;
      },
      [&](uint64_t i) {
        if (ev_planes) ev_planes[i] = 0u;
        if (ev_levels)
          for (uint32_t t = 0; t < K; ++t) ev_levels[t * cap + i] = id;
      });
}
