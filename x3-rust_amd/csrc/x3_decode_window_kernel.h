// x3_decode_window_kernel.h -- random access: batches of sample windows from a device-resident stream (x3_decode_windows_dev).
//
// A window is the samples at positions [start, start + L) of the stream, position = sample_offsets[f] + i for sample i of
// frame f.  The work of a call follows the windows, not the stream: per window, the frames that cover it, and per frame
// its stretches of the segment index.  Five launches, nothing comes back to the host in between (every count lives in the
// workspace and the later kernels walk it grid-stride):
//
//  x3_window_plan_kernel    -- a thread per window: the start is checked against the total (sample_offsets[F]), the
//      covering frames [fa, fb] are found by binary search.  A window off the end is X3_ERR_BAD_ARG and covers nothing.
//  x3_window_scan_kernel    -- one workgroup: exclusive scans of the covering frames and of the work items per window
//      (x3w_scan_items, the run-per-thread scan of every one-workgroup scan kernel here and in the levels family).
//  x3_window_check_kernel   -- a WAVE per (window, covering frame): header (x3_frame_header_check_words), payload CRC as a
//      segmented reduction over the wave, `samples` against sample_offsets[f + 1] - sample_offsets[f].  The verdict goes
//      to the frame's word of a per-frame array (every window that covers the frame writes the same word).
//  x3_window_decode_kernel  -- a LANE per (window, covering frame, stretch).  A stretch starts at block 0 or at a usable
//      index entry and runs to the next usable entry, where it compares its end -- bit position and last sample -- with
//      that entry (x3_decode_split_kernel.h, "STRETCHES"): by induction from block 0 the frame then decodes as the serial
//      walk does.  Every stretch of every covering frame runs, also those outside the window: they are the proof chain of
//      the stretches inside it, and a frame's verdict (decode errors behind the window included) is the whole frame's.
//      Only samples inside the window are stored.  Without an index a frame is one stretch: one lane, serially.
//  x3_window_fixup_kernel   -- a wave per window, in frame order: a frame that a stretch has flagged (contradicted entry,
//      decode error, zero run of 32 bits or more, a read behind the payload) goes through the reference's reader
//      (x3_replay_block, x3_decode_replay.h), which rewrites its in-window samples.  At the first frame that fails the
//      window's status is set and the rest of the row is zeroed.
//
// Nothing here trusts the caller's offsets, starts or index: every stream read is bounds-checked against x3_len (a
// partial last dword is read byte by byte), every store is at a row position in [0, L).
//
// RANGES (x3_decode_ranges_dev): the same launch set with a length per window.  x3_range_plan_kernel / x3_corpus_range_plan_kernel
// read lens[w], x3_range_scan_kernel scans the lengths in front of the covering frames (x3w_range_scan, the body it shares with
// x3_range_levels_scan_kernel), and the decode and fix-up kernels are
// the templates' other instance: their rows come from X3WinRangeGeo instead of w * L and L.
#pragma once
#include "x3_device.h"
#include "x3_decode_kernel.h"
#include "x3_decode_replay.h"
#include "x3_decode_split_kernel.h"   // X3S_SEG_MAGIC, X3S_SEG_VALID: the segment index

// (X3_WINDOW_I16 / X3_WINDOW_F32: include/x3hip.h)
#define X3W_FLAG 0x10000      // per-frame word: a stretch has flagged the frame for the reference's reader
#define X3W_GRID_LIMIT 4096u  // workgroups of the grid-stride kernels

struct X3WinPlan {
  uint64_t fa;     // first covering frame
  uint32_t ncov;   // covering frames (0: the window is off the end)
  int32_t status;  // X3D_OK or X3D_BAD_ARG from the plan
};

// the windows' summary: n_bad and min(w << 8 | status) over the bad windows; replays: the (window, covering frame) pairs
// x3_window_fixup_kernel re-decoded through the reference's reader (option "last_window_replays")
struct X3WinSummary {
  unsigned long long n_bad;
  unsigned long long first;
  unsigned long long replays;
  unsigned long long total;   // ranges only: the sum of all lengths (x3_range_scan_kernel)
};

// stream dword j (bytes 4j .. 4j+3) as a big-endian value, bytes at or beyond len read as zero
__device__ __forceinline__ uint32_t x3w_be_dword(const uint8_t* __restrict__ x3, uint64_t len, uint64_t j) {
  const uint64_t b = j << 2;
  if (b + 4u <= len) return x3_bswap32(reinterpret_cast<const uint32_t*>(x3)[j]);
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4u; ++k)
    if (b + k < len) v |= (uint32_t)x3[b + k] << (24u - 8u * k);
  return v;
}

// 4 stream bytes at byte offset o, big-endian (zero beyond len)
__device__ __forceinline__ uint32_t x3w_be32_at(const uint8_t* __restrict__ x3, uint64_t len, uint64_t o) {
  const uint32_t sh = (uint32_t)(o & 3u) * 8u;
  const uint32_t a = x3w_be_dword(x3, len, o >> 2);
  if (sh == 0) return a;
  return (a << sh) | (x3w_be_dword(x3, len, (o >> 2) + 1u) >> (32u - sh));
}

// MSB-first bit reader over the stream at an absolute bit position: a 64-bit window with at least 32 valid bits after every
// refill, fed from four stream dwords loaded together.  On gfx9 a wave's stores count in the same vmcnt as its loads, so a
// refill waits for every sample stored before it: one wait per 128 bits instead of per 32 (measured: the kernel of a single
// window: 0.82 ms with a refill per dword, profiles/windows/).  Reads behind the payload are not refused
// here (the bits are the stream's, or zero behind len); the caller compares the position with the payload's end, as the fast
// decoders do (x3_decode_replay.h).
struct X3WinBits {
  const uint8_t* x3;
  uint64_t len;
  uint64_t win;   // bits [pos, pos + nv) in the top nv bits
  uint64_t pos;   // absolute bit position of the next bit
  uint64_t nxt;   // next dword to load
  uint32_t nv;
  uint32_t q0, q1, q2, q3, nq;   // loaded dwords not yet in the window (big-endian values), nq of them
  __device__ __forceinline__ void open(const uint8_t* s, uint64_t n, uint64_t bitpos) {
    x3 = s;
    len = n;
    pos = bitpos;
    const uint64_t j = bitpos >> 5;
    const uint32_t sh = (uint32_t)(bitpos & 31u);
    win = (((uint64_t)x3w_be_dword(s, n, j) << 32) | x3w_be_dword(s, n, j + 1u)) << sh;
    nv = 64u - sh;
    nxt = j + 2u;
    nq = 0;
  }
  __device__ __forceinline__ void load4() {
    if ((nxt + 4u) * 4u <= len) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(x3) + nxt;
      q0 = x3_bswap32(w[0]); q1 = x3_bswap32(w[1]); q2 = x3_bswap32(w[2]); q3 = x3_bswap32(w[3]);
    } else {
      q0 = x3w_be_dword(x3, len, nxt); q1 = x3w_be_dword(x3, len, nxt + 1u);
      q2 = x3w_be_dword(x3, len, nxt + 2u); q3 = x3w_be_dword(x3, len, nxt + 3u);
    }
    nxt += 4u;
    nq = 4u;
  }
  __device__ __forceinline__ void fill() {
    if (nv < 32u) {
      if (nq == 0u) load4();
      win |= (uint64_t)q0 << (32u - nv);
      nv += 32u;
      q0 = q1; q1 = q2; q2 = q3;
      --nq;
    }
  }
  __device__ __forceinline__ uint32_t bits(uint32_t n) {  // 1 <= n <= 16
    fill();
    const uint32_t r = (uint32_t)(win >> (64u - n));
    win <<= n;
    nv -= n;
    pos += n;
    return r;
  }
  // the zero run in front of the next one bit; 32 or more -> `run32` (the reference's reader differs there)
  __device__ __forceinline__ uint32_t zeros(bool& run32) {
    fill();
    const uint32_t top = (uint32_t)(win >> 32);
    if (top == 0u) {
      run32 = true;
      return 0u;
    }
    const uint32_t z = (uint32_t)__clz(top);
    win <<= z;
    nv -= z;
    pos += z;
    return z;
  }
};

// decoder::decode_block over X3WinBits: x3_replay_block's arithmetic.  Returns false where the reference's reader may
// disagree or the block is an error -- the frame then goes to x3_replay_frame's loop.  Sample i of the block is handed
// to put(i, value).
template <class Put>
__device__ __forceinline__ bool x3w_block(X3WinBits& br, uint32_t n, const X3DevParams& p, uint32_t& last, Put put) {
  const uint32_t ftype = br.bits(2u);
  bool run32 = false;
  if (ftype == 0u) {
    const uint32_t E = br.bits(4u) + 1u;
    if (E <= 5u || n == 0u) return false;
    if (E == 16u) {
      for (uint32_t i = 0; i < n; ++i) {
        last = br.bits(16u) & 0xFFFFu;
        put(i, last);
      }
    } else {
      const uint32_t half = 1u << (E - 1u);
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t v = br.bits(E) & 0xFFFFu;
        if (v > half) v -= half << 1;
        last = (last + v) & 0xFFFFu;
        put(i, last);
      }
    }
  } else if (ftype == 1u) {
    const uint32_t bound = p.inv_len[0];
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t ix = br.zeros(run32);
      if (run32) return false;
      (void)br.bits(1u);
      if (ix >= bound) return false;
      const uint32_t d = (ix & 1u) ? 0u - ((ix + 1u) >> 1) : (ix >> 1);
      last = (last + d) & 0xFFFFu;
      put(i, last);
    }
  } else {
    const uint32_t nb = ftype == 2u ? 2u : 4u;
    const int32_t level = 1 << p.k[ftype - 1u];
    const uint32_t bound = p.inv_len[ftype - 1u];
    for (uint32_t i = 0; i < n; ++i) {
      const int32_t nz = (int32_t)br.zeros(run32);
      if (run32) return false;
      const int32_t r = (int32_t)(int16_t)br.bits(nb);
      const int32_t ix = (int32_t)(int16_t)(r + level * (nz - 1));
      if (ix < 0 || (uint32_t)ix >= bound) return false;
      const uint32_t u = (uint32_t)ix;
      const uint32_t d = (u & 1u) ? 0u - ((u + 1u) >> 1) : (u >> 1);
      last = (last + d) & 0xFFFFu;
      put(i, last);
    }
  }
  return true;
}

__device__ __forceinline__ void x3w_store(void* __restrict__ out, int fmt, uint64_t at, uint32_t v) {
  if (fmt == X3_WINDOW_F32) reinterpret_cast<float*>(out)[at] = (float)(int16_t)(uint16_t)v * (1.0f / 32768.0f);
  else reinterpret_cast<int16_t*>(out)[at] = (int16_t)(uint16_t)v;
}

// index header: {X3S_SEG_MAGIC, blocks per entry}; anything else (or no index) = decode frames whole
__device__ __forceinline__ bool x3w_index_ok(const uint2* __restrict__ idx, uint32_t sb) {
  if (!idx || sb == 0u) return false;
  const uint2 h = idx[0];
  return h.x == X3S_SEG_MAGIC && h.y == sb;
}

// largest f in [lo, hi) with so[f] <= x, given so[lo] <= x < so[hi]
__device__ __forceinline__ uint64_t x3w_search(const uint64_t* __restrict__ so, uint64_t lo, uint64_t hi, uint64_t x) {
  while (hi - lo > 1u) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (so[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// largest w with off[w] <= i (off[0] = 0, non-decreasing, n + 1 entries)
__device__ __forceinline__ uint64_t x3w_owner(const unsigned long long* __restrict__ off, uint64_t n, uint64_t i) {
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- sample offsets: so[f] = exclusive prefix of the headers' `samples` (0 for a header that is not inside the stream),
// so[F] = the total.  One workgroup of 1024: a contiguous run of frames per thread, a workgroup scan of the runs' sums.
__device__ __forceinline__ unsigned long long x3w_block_excl_scan(unsigned long long v, unsigned long long* s, unsigned long long* total) {
  const uint32_t t = threadIdx.x, n = blockDim.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < n; d <<= 1) {
    const unsigned long long a = t >= d ? s[t - d] : 0ull;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  const unsigned long long incl = s[t];
  *total = s[n - 1];
  __syncthreads();
  return incl - v;
}

// The scan of n items by one workgroup, a contiguous run of items per thread (x3w_own_items: each(i) for the thread's own).
// count(i) is item i's weight, put(i, sum) takes the sum of the weights in front of it (count(i) is read before put(i) runs,
// so put may overwrite what count reads); the total comes back to every thread.  s: blockDim.x words of LDS.
// x3w_scan_own_items: `mine` is the sum of the thread's own weights already -- a site that forms the weights in a first walk
// over its items, or while it writes an earlier scan, sums them there.
template <class Each>
__device__ __forceinline__ void x3w_own_items(uint64_t n, Each each) {
  const uint64_t per = (n + blockDim.x - 1) / blockDim.x;
  const uint64_t a = min((uint64_t)threadIdx.x * per, n), b = min(a + per, n);
  for (uint64_t i = a; i < b; ++i) each(i);
}

template <class Count, class Put>
__device__ __forceinline__ unsigned long long x3w_scan_own_items(uint64_t n, unsigned long long* s, unsigned long long mine,
                                                                 Count count, Put put) {
  unsigned long long total;
  unsigned long long run = x3w_block_excl_scan(mine, s, &total);
  x3w_own_items(n, [&](uint64_t i) {
    const unsigned long long own = count(i);
    put(i, run);
    run += own;
  });
  return total;
}

template <class Count, class Put>
__device__ __forceinline__ unsigned long long x3w_scan_items(uint64_t n, unsigned long long* s, Count count, Put put) {
  unsigned long long mine = 0;
  x3w_own_items(n, [&](uint64_t i) { mine += count(i); });
  return x3w_scan_own_items(n, s, mine, count, put);
}

__device__ __forceinline__ uint32_t x3w_header_samples(const uint8_t* __restrict__ x3, uint64_t len, uint64_t off) {
  if (len < 20u || off > len - 20u) return 0u;
  return ((uint32_t)x3[off + 4u] << 8) | x3[off + 5u];
}

__global__ void __launch_bounds__(1024)
x3_window_sample_offsets_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off,
                                uint64_t F, uint64_t* __restrict__ so) {
  __shared__ unsigned long long s[1024];
  const unsigned long long total = x3w_scan_items(
      F, s, [&](uint64_t f) { return (unsigned long long)x3w_header_samples(x3, len, frame_off[f]); },
      [&](uint64_t f, unsigned long long run) { so[f] = run; });
  if (threadIdx.x == 0) so[F] = total;
}

// The plan of positions [start, start + L) of a stream: BAD_ARG off the end, else the covering frames by binary search.
// ZeroLen (the range plans; the window calls refuse L == 0 on the host and their instances hold no test of it): L == 0 covers
// nothing and start + L - 1 is not formed.
template <bool ZeroLen>
__device__ __forceinline__ X3WinPlan x3w_plan_stream(const uint64_t* __restrict__ so, uint64_t F, uint64_t total, uint64_t start,
                                                     uint32_t L) {
  X3WinPlan pl{0, 0, X3D_BAD_ARG};
  // (so[0] <= start and so[F] > start + L - 1 are the search's invariants; offsets that break them are not this stream's)
  if (L <= total && start <= total - L && so[0] <= start) {
    if (ZeroLen && L == 0u) return X3WinPlan{0, 0, X3D_OK};
    const uint64_t e = start + (L - 1u);
    const uint64_t fa = x3w_search(so, 0, F, start);
    const uint64_t fb = x3w_search(so, fa, F, e);
    // more covering frames than samples: a frame of 0 samples or offsets out of order, no stream's frames
    if (fb - fa < (uint64_t)L) pl = X3WinPlan{fa, (uint32_t)(fb - fa + 1u), X3D_OK};
  }
  return pl;
}

// ---- plan: a thread per window, grid-stride (the grid is capped at X3W_GRID_LIMIT groups; every window gets its plan)
__device__ __forceinline__ void x3w_summary_init(X3WinSummary* __restrict__ sum) {
  sum->n_bad = 0;
  sum->first = ~0ull;
  sum->replays = 0;
}

__global__ void __launch_bounds__(256)
x3_window_plan_kernel(const uint64_t* __restrict__ so, uint64_t F, const uint64_t* __restrict__ starts, uint64_t n_windows,
                      uint32_t L, X3WinPlan* __restrict__ plan, X3WinSummary* __restrict__ sum) {
  const uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w0 == 0) x3w_summary_init(sum);
  const uint64_t total = so[F];
  for (uint64_t w = w0; w < n_windows; w += (uint64_t)gridDim.x * blockDim.x) plan[w] = x3w_plan_stream<false>(so, F, total, starts[w], L);
}

// the same with a length per range (x3_decode_ranges_dev)
__global__ void __launch_bounds__(256)
x3_range_plan_kernel(const uint64_t* __restrict__ so, uint64_t F, const uint64_t* __restrict__ starts,
                     const uint32_t* __restrict__ lens, uint64_t n_ranges, X3WinPlan* __restrict__ plan,
                     X3WinSummary* __restrict__ sum) {
  const uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w0 == 0) x3w_summary_init(sum);
  const uint64_t total = so[F];
  for (uint64_t w = w0; w < n_ranges; w += (uint64_t)gridDim.x * blockDim.x) plan[w] = x3w_plan_stream<true>(so, F, total, starts[w], lens[w]);
}

// ---- exclusive scans of the covering frames (cov) and the work items (cov * stretches) per window; n + 1 entries each
__global__ void __launch_bounds__(1024)
x3_window_scan_kernel(const X3WinPlan* __restrict__ plan, uint64_t n, const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg,
                      unsigned long long* __restrict__ cov_off, unsigned long long* __restrict__ item_off) {
  __shared__ unsigned long long s[1024];
  const uint32_t ns = x3w_index_ok(idx, sb) ? nseg : 1u;
  const unsigned long long total = x3w_scan_items(
      n, s, [&](uint64_t w) { return (unsigned long long)plan[w].ncov; },
      [&](uint64_t w, unsigned long long run) {
        cov_off[w] = run;
        item_off[w] = run * ns;
      });
  if (threadIdx.x == 0) {
    cov_off[n] = total;
    item_off[n] = total * ns;
  }
}

// ---- RANGES (x3_decode_ranges_dev / x3_corpus_ranges_dev): a length per range, rows packed at the
// exclusive scan of the lengths (stride 0) or padded to a common stride.
// The rows of a call: where row w begins and how many samples of it are the range's.  X3WinFixedGeo is the window calls'
// w * L and L; X3WinRangeGeo reads what x3_range_scan_kernel left in the workspace.  kTails: the fix-up zeroes
// [len, row_end) of every row.
struct X3WinFixedGeo {
  uint32_t L;
  static constexpr bool kTails = false;
  __device__ __forceinline__ uint64_t base(uint64_t w) const { return w * (uint64_t)L; }
  __device__ __forceinline__ uint32_t len(uint64_t) const { return L; }
  __device__ __forceinline__ uint64_t row_end(uint64_t) const { return (uint64_t)L; }
};
struct X3WinRangeGeo {
  const uint32_t* __restrict__ elen;            // the range's length, 0 for a range that has no room in its row
  const unsigned long long* __restrict__ off;   // packed: the exclusive scan of ALL lengths, n + 1 words
  uint64_t stride;                              // padded: the row stride; 0 = packed
  static constexpr bool kTails = true;
  __device__ __forceinline__ uint64_t base(uint64_t w) const { return stride ? w * stride : off[w]; }
  __device__ __forceinline__ uint32_t len(uint64_t w) const { return elen[w]; }
  __device__ __forceinline__ uint64_t row_end(uint64_t w) const { return stride ? stride : elen[w]; }
};

// x3_window_scan_kernel with the scan of the ranges' sizes in front of it -- size(w): the length of range w (the ranges calls)
// or its level records (the range-levels calls, x3_range_levels_kernel.h): off[w] (packed; n + 1 words, also to the caller's
// out_off, which gets w * stride when padded), the verdict on the row -- a range with off[w] + size > cap (packed) or
// size > stride (padded) is X3D_BAD_ARG, covers nothing and stores nothing: esize[w] = 0 -- and then the covering frames
// and, with Items, the work items of what is left.  Returns the sum of all sizes (64-bit sums of at most 2^31 32-bit sizes:
// no wrap).
template <bool Items, class Size>
__device__ __forceinline__ unsigned long long x3w_range_scan(X3WinPlan* __restrict__ plan, uint64_t n, Size size, uint64_t stride,
                                                             uint64_t cap, uint32_t ns, unsigned long long* __restrict__ cov_off,
                                                             unsigned long long* __restrict__ item_off,
                                                             unsigned long long* __restrict__ off, uint32_t* __restrict__ esize,
                                                             uint64_t* __restrict__ out_off, unsigned long long* s) {
  unsigned long long covers = 0;   // (the thread's own ranges: the covering frames of those that have room)
  unsigned long long sz = 0;       // (size(w), at most 2^32 - 1: the scan reads a range's size in front of its put)
  const unsigned long long total = x3w_scan_items(n, s, [&](uint64_t w) { return sz = size(w); }, [&](uint64_t w, unsigned long long run) {
    const bool fits = stride ? sz <= stride : (run <= cap && sz <= cap - run);
    if (!fits) plan[w] = X3WinPlan{0, 0, X3D_BAD_ARG};
    esize[w] = fits ? (uint32_t)sz : 0u;
    off[w] = run;
    if (out_off) out_off[w] = stride ? w * stride : run;
    covers += fits ? plan[w].ncov : 0u;
  });
  if (threadIdx.x == 0) {
    off[n] = total;
    if (out_off) out_off[n] = stride ? n * stride : total;
  }
  const unsigned long long n_cov = x3w_scan_own_items(
      n, s, covers, [&](uint64_t w) { return (unsigned long long)plan[w].ncov; },
      [&](uint64_t w, unsigned long long run) {
        cov_off[w] = run;
        if (Items) item_off[w] = run * ns;
      });
  if (threadIdx.x == 0) {
    cov_off[n] = n_cov;
    if (Items) item_off[n] = n_cov * ns;
  }
  return total;
}

__global__ void __launch_bounds__(1024)
x3_range_scan_kernel(X3WinPlan* __restrict__ plan, uint64_t n, const uint32_t* __restrict__ lens, uint64_t stride,
                     uint64_t out_cap, const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg,
                     unsigned long long* __restrict__ cov_off, unsigned long long* __restrict__ item_off,
                     unsigned long long* __restrict__ off, uint32_t* __restrict__ elen, uint64_t* __restrict__ out_off,
                     X3WinSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  const uint32_t ns = x3w_index_ok(idx, sb) ? nseg : 1u;
  const unsigned long long total = x3w_range_scan<true>(
      plan, n, [&](uint64_t w) { return (unsigned long long)lens[w]; }, stride, out_cap, ns, cov_off, item_off, off, elen, out_off, s);
  if (threadIdx.x == 0) sum->total = total;
}

// ---- check: a wave per (window, covering frame)
// The verdict of frame f by one wave (every lane returns it): header, payload CRC, what x3_decode_dev's decoders refuse behind
// the check, and the header's `samples` against the caller's sample offsets.
__device__ __forceinline__ int32_t x3w_check_frame(const uint8_t* __restrict__ x3, uint64_t len, uint64_t off,
                                                   const uint64_t* __restrict__ so, uint64_t f, uint32_t lane) {
  uint32_t plen = 0, samples = 0, pcrc = 0;
  int32_t st;
  if (len < 20u || off > len - 20u) {
    st = X3D_BAD_ARG;   // (the caller's offset is not inside this stream)
  } else {
    const uint32_t h0 = x3w_be32_at(x3, len, off), h1 = x3w_be32_at(x3, len, off + 4u);
    const uint32_t h2 = x3w_be32_at(x3, len, off + 8u), h3 = x3w_be32_at(x3, len, off + 12u);
    const uint32_t h4 = x3w_be32_at(x3, len, off + 16u);
    uint32_t hc = 0xFFFFu;
    hc = x3_crc_be32(hc, h0);
    hc = x3_crc_be32(hc, h1);
    hc = x3_crc_be32(hc, h2);
    hc = x3_crc_be32(hc, h3);
    st = x3_frame_header_check_words(h0, h1, h4, hc, len, off, plen, samples, pcrc);
    if (st == X3D_STREAM_ENDS_IN_FRAME) st = X3D_BAD_ARG;
  }
  if (st == X3D_OK) {
    // payload CRC: lane t CRCs a contiguous chunk with init 0, the chunks are joined by x^(8 * bytes behind them)
    const uint64_t p0 = off + 20u;
    const uint32_t chunk = (plen + 63u) >> 6;
    const uint32_t a = min(lane * chunk, plen), b = min(a + chunk, plen);
    uint32_t c = 0;
    for (uint32_t k = a; k < b; ++k) c = x3_crc_byte(c, x3[p0 + k]);
    // x^(8 * (plen - b)) by squaring; lane 0 also carries the init value 0xFFFF times x^(8 * plen)
    auto xpow8 = [](uint32_t nbytes) -> uint32_t {
      uint32_t r = 1u, base = 0x100u;
      while (nbytes) {
        if (nbytes & 1u) r = x3_gf_mul(r, base);
        base = x3_gf_mul(base, base);
        nbytes >>= 1;
      }
      return r;
    };
    uint32_t part = x3_gf_mul(c, xpow8(plen - b));
    if (lane == 0) part ^= x3_gf_mul(0xFFFFu, xpow8(plen));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part ^= (uint32_t)__shfl_xor((int)part, o, X3_WAVE);
    if ((part & 0xFFFFu) != pcrc) st = X3D_FRAME_HEADER_INVALID_PAYLOAD_CRC;
  }
  // what x3_decode_dev's decoders refuse behind the check, and the caller's offsets against the header
  if (st == X3D_OK && (samples == 0u || plen < 2u)) st = X3D_BAD_ARG;
  if (st == X3D_OK && (so[f + 1u] < so[f] || so[f + 1u] - so[f] != samples)) st = X3D_BAD_ARG;
  return st;
}

__global__ void __launch_bounds__(256)
x3_window_check_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off,
                       const uint64_t* __restrict__ so, const X3WinPlan* __restrict__ plan, uint64_t n_windows,
                       const unsigned long long* __restrict__ cov_off, int32_t* __restrict__ fst) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n_items = cov_off[n_windows];
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_items; i += waves) {
    const uint64_t w = x3w_owner(cov_off, n_windows, i);
    const uint64_t f = plan[w].fa + (i - cov_off[w]);
    const int32_t st = x3w_check_frame(x3, len, frame_off[f], so, f, lane);
    if (lane == 0) fst[f] = st;
  }
}

// ---- decode: a lane per (window, covering frame, stretch)
// Stretch j of checked frame f by one lane: from block 0 or from usable entry j to the next usable entry, whose bit position
// and last sample it must meet.  Sample s of the frame goes to put_at(s, value).  0: entry j starts no stretch (the
// stretch in front runs through its blocks), 1: decoded and proven, -1: the frame is one for the reference's reader.
// `watch` (optional) sees the two samples a consumer with one sample of history needs and put_at does not carry:
// watch.seed(v), the sample in front of a stretch that starts at an index entry -- the entry's, unproven like its bit
// position until the stretch in front has met it -- and watch.end(v), the frame's last sample, from the one stretch that
// runs to the frame's end.  This function stays the only reader of the entry format.
struct X3WNoWatch {
  __device__ __forceinline__ void seed(uint32_t) const {}
  __device__ __forceinline__ void end(uint32_t) const {}
};
template <class Put, class Watch = X3WNoWatch>
__device__ __forceinline__ int x3w_stretch(const uint8_t* __restrict__ x3, uint64_t len, uint64_t off, const X3DevParams& p,
                                           const uint2* __restrict__ idx, bool segd, uint32_t sb, uint32_t nseg, uint64_t f,
                                           uint32_t j, Put put_at, Watch watch = Watch{}) {
  const uint32_t pitch = nseg - 1u;
  const uint64_t p0 = off + 20u;
  const uint32_t h1 = x3w_be32_at(x3, len, off + 4u);
  const uint32_t samples = h1 >> 16, plen = h1 & 0xFFFFu;
  const uint32_t nbf = (samples - 1u + p.block_len - 1u) / p.block_len;   // blocks of the frame
  const uint2* const e = segd ? idx + 1 + f * (uint64_t)pitch : nullptr;
  auto usable = [&](uint32_t q) -> bool {   // entry q (1 .. nseg-1) is one to start from / end at
    if (sb * q >= nbf) return false;
    const uint2 h = e[q - 1u];
    return (h.y & X3S_SEG_VALID) && h.x >= 16u && h.x <= 8u * plen;
  };
  if (j && !usable(j)) return 0;   // (the stretch in front runs through these blocks)
  uint32_t q = j + 1u;             // the next usable entry, nseg if none
  if (segd)
    while (q < nseg && !usable(q)) ++q;
  else
    q = 1u;
  const uint32_t b0 = sb * j;
  const uint32_t b1 = (segd && q < nseg) ? sb * q : nbf;
  uint32_t last;
  X3WinBits br;
  if (j == 0u) {
    last = x3w_be32_at(x3, len, p0) >> 16;
    put_at(0u, last);
    br.open(x3, len, p0 * 8u + 16u);
  } else {
    const uint2 h = e[j - 1u];
    last = h.y & 0xFFFFu;
    watch.seed(last);
    br.open(x3, len, p0 * 8u + h.x);
  }
  const uint64_t end_bit = (p0 + plen) * 8u;
  bool ok = true;
  for (uint32_t b = b0; b < b1 && ok; ++b) {
    const uint32_t s0 = 1u + b * p.block_len;
    const uint32_t n = min(p.block_len, samples - s0);
    ok = x3w_block(br, n, p, last, [&](uint32_t t, uint32_t v) { put_at(s0 + t, v); });
    ok = ok && br.pos <= end_bit;
  }
  if (ok && segd && q < nseg) {
    const uint2 h = e[q - 1u];
    ok = br.pos - p0 * 8u == h.x && last == (h.y & 0xFFFFu);
  }
  if (ok && b1 == nbf) watch.end(last);
  return ok ? 1 : -1;
}

// (Geo: the rows -- X3WinFixedGeo for the window calls, X3WinRangeGeo for the ranges)
template <class Geo>
__global__ void __launch_bounds__(256)
x3_window_decode_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off,
                        const uint64_t* __restrict__ so, const uint64_t* __restrict__ starts, const X3WinPlan* __restrict__ plan,
                        uint64_t n_windows, Geo geo, const unsigned long long* __restrict__ item_off, X3DevParams p,
                        const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg, void* __restrict__ out, int fmt,
                        int32_t* __restrict__ fst) {
  const bool segd = x3w_index_ok(idx, sb);
  const uint32_t ns = segd ? nseg : 1u;
  const uint64_t n_items = item_off[n_windows];
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += lanes) {
    const uint64_t w = x3w_owner(item_off, n_windows, i);
    const uint64_t k = i - item_off[w];
    const uint64_t f = plan[w].fa + k / ns;
    const uint32_t j = (uint32_t)(k % ns);
    if (fst[f] != X3D_OK) continue;   // (checked: header, CRC, sample count; a frame that failed is not decoded)
    const uint64_t rbase = geo.base(w), start = starts[w], fpos = so[f];
    const auto L = geo.len(w);
    auto put_at = [&](uint32_t s, uint32_t v) {   // sample s of the frame
      const uint64_t g = fpos + s;
      if (g >= start && g - start < (uint64_t)L) x3w_store(out, fmt, rbase + (g - start), v);
    };
    if (x3w_stretch(x3, len, frame_off[f], p, idx, segd, sb, nseg, f, j, put_at) < 0) atomicOr(&fst[f], X3W_FLAG);
  }
}

// decoder::decode_frame of a checked frame through the reference's reader (x3_replay_frame's loop), block by block into
// `blk` (a block's samples); sample s of the frame goes to put_at(s, value), a failing block hands over nothing.
template <class Put>
__device__ __forceinline__ int32_t x3w_replay_frame(const uint8_t* __restrict__ payload, const X3DevParams& p,
                                                    int16_t* __restrict__ blk, Put put_at) {
  const uint32_t samples = ((uint32_t)payload[-16] << 8) | payload[-15];
  const uint32_t plen = ((uint32_t)payload[-14] << 8) | payload[-13];
  uint32_t last = ((uint32_t)payload[0] << 8) | payload[1];
  put_at(0u, last);
  X3RefReader br;
  br.open(payload + 2, plen - 2u);
  uint32_t at = 1u, remaining = samples - 1u;
  int32_t fs = X3D_OK;
  while (remaining && fs == X3D_OK) {
    const uint32_t n = remaining < p.block_len ? remaining : p.block_len;
    fs = x3_replay_block(br, n, p, last, blk);
    if (fs == X3D_OK)
      for (uint32_t t = 0; t < n; ++t) put_at(at + t, (uint16_t)blk[t]);
    remaining -= n;
    at += n;
  }
  return fs;
}

// ---- fix-up: a wave per window, frames in order; scratch: a block's samples per window (x3_replay_block's output)
// (Geo: the rows, as in x3_window_decode_kernel)
template <class Geo>
__global__ void __launch_bounds__(256)
x3_window_fixup_kernel(const uint8_t* __restrict__ x3, const uint64_t* __restrict__ frame_off, const uint64_t* __restrict__ so,
                       const uint64_t* __restrict__ starts, const X3WinPlan* __restrict__ plan, uint64_t n_windows, Geo geo,
                       X3DevParams p, const int32_t* __restrict__ fst, void* __restrict__ out, int fmt,
                       int32_t* __restrict__ status, int16_t* __restrict__ scratch, uint32_t scratch_per,
                       X3WinSummary* __restrict__ sum) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_windows; w += waves) {
    const X3WinPlan pl = plan[w];
    const uint64_t start = starts[w], rbase = geo.base(w);
    const auto L = geo.len(w);
    int32_t st = pl.status;
    uint64_t zero_from = 0;   // (st != 0) the row from here on is zero
    uint32_t replayed = 0;
    if (lane == 0 && st == X3D_OK) {
      int16_t* const blk = scratch + w * (uint64_t)scratch_per;
      for (uint64_t f = pl.fa; f < pl.fa + pl.ncov; ++f) {
        int32_t fs = fst[f];
        if (fs == X3W_FLAG) {
          const uint64_t fpos = so[f];
          auto put_at = [&](uint32_t s, uint32_t v) {
            const uint64_t g = fpos + s;
            if (g >= start && g - start < (uint64_t)L) x3w_store(out, fmt, rbase + (g - start), v);
          };
          fs = x3w_replay_frame(x3 + frame_off[f] + 20u, p, blk, put_at);
          ++replayed;
        }
        if (fs != X3D_OK) {
          st = fs;
          zero_from = so[f] > start ? min(so[f] - start, (uint64_t)L) : 0u;
          break;
        }
      }
    }
    st = __shfl(st, 0, X3_WAVE);
    zero_from = (uint64_t)__shfl((long long)zero_from, 0, X3_WAVE);
    if constexpr (Geo::kTails) {   // a bad range's zeros and the tail behind every length, in one run
      const uint64_t row_end = geo.row_end(w);
      for (uint64_t t = (st != X3D_OK ? zero_from : (uint64_t)L) + lane; t < row_end; t += 64u) x3w_store(out, fmt, rbase + t, 0u);
    } else {
      if (st != X3D_OK)
        for (uint64_t t = zero_from + lane; t < L; t += 64u) x3w_store(out, fmt, rbase + t, 0u);
    }
    if (lane == 0) {
      if (replayed) atomicAdd(&sum->replays, (unsigned long long)replayed);
      status[w] = st;
      if (st != X3D_OK) {
        atomicAdd(&sum->n_bad, 1ull);
        atomicMin(&sum->first, (unsigned long long)(w << 8) | (uint32_t)st);
      }
    }
  }
}

// ---- CORPUS (x3_corpus_windows_dev)
// an entry's positions: so[first_frame + n_frames] - so[first_frame] (the build, one thread per entry)
__global__ void __launch_bounds__(256)
x3_corpus_samples_kernel(const uint64_t* __restrict__ so, uint64_t F, x3_corpus_entry* __restrict__ ent, uint64_t n) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint64_t a = ent[e].first_frame, b = a + ent[e].n_frames;
  ent[e].n_samples = b <= F && so[b] >= so[a] ? so[b] - so[a] : 0ull;
}

// plan: a thread per window (entry, start), grid-stride as x3_window_plan_kernel.  The entry's positions are consecutive in
// the corpus's sample offsets, so its start s is the global position so[first_frame] + s; the covering frames are searched
// inside the entry's frames as x3_window_plan_kernel searches a stream's.  gstart[w]: the position the later kernels read
// where they read d_starts.  ZeroLen: L == 0 (a range) covers nothing, as in x3w_plan_stream.
template <bool ZeroLen>
__device__ __forceinline__ X3WinPlan x3w_plan_entry(const x3_corpus_entry* __restrict__ ent, uint64_t n_ent,
                                                    const uint64_t* __restrict__ so, uint64_t F, uint32_t e, uint64_t start,
                                                    uint32_t L, uint64_t& g) {
  X3WinPlan pl{0, 0, X3D_BAD_ARG};
  g = 0;
  if (e < n_ent) {
    const x3_corpus_entry en = ent[e];
    const uint64_t fa0 = en.first_frame, fb0 = en.first_frame + en.n_frames;
    // (the table's words are checked, not trusted: the entry's frames inside the table, its positions inside so's range)
    if (en.n_frames && fa0 < F && en.n_frames <= F - fa0 && L <= en.n_samples && start <= en.n_samples - L) {
      const uint64_t base = so[fa0], total = so[fb0];
      if (total >= base && total - base == en.n_samples) {
        g = base + start;
        if (ZeroLen && L == 0u) return X3WinPlan{0, 0, X3D_OK};
        const uint64_t fa = x3w_search(so, fa0, fb0, g);
        const uint64_t fb = x3w_search(so, fa, fb0, g + (L - 1u));
        if (fb - fa < (uint64_t)L) pl = X3WinPlan{fa, (uint32_t)(fb - fa + 1u), X3D_OK};
      }
    }
  }
  return pl;
}

__global__ void __launch_bounds__(256)
x3_corpus_plan_kernel(const x3_corpus_entry* __restrict__ ent, uint64_t n_ent, const uint64_t* __restrict__ so, uint64_t F,
                      const uint32_t* __restrict__ entries, const uint64_t* __restrict__ starts, uint64_t n_windows, uint32_t L,
                      X3WinPlan* __restrict__ plan, uint64_t* __restrict__ gstart, X3WinSummary* __restrict__ sum) {
  const uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w0 == 0) x3w_summary_init(sum);
  for (uint64_t w = w0; w < n_windows; w += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t g;
    plan[w] = x3w_plan_entry<false>(ent, n_ent, so, F, entries[w], starts[w], L, g);
    gstart[w] = g;
  }
}

// the same with a length per range (x3_corpus_ranges_dev)
__global__ void __launch_bounds__(256)
x3_corpus_range_plan_kernel(const x3_corpus_entry* __restrict__ ent, uint64_t n_ent, const uint64_t* __restrict__ so, uint64_t F,
                            const uint32_t* __restrict__ entries, const uint64_t* __restrict__ starts,
                            const uint32_t* __restrict__ lens, uint64_t n_ranges, X3WinPlan* __restrict__ plan,
                            uint64_t* __restrict__ gstart, X3WinSummary* __restrict__ sum) {
  const uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w0 == 0) x3w_summary_init(sum);
  for (uint64_t w = w0; w < n_ranges; w += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t g;
    plan[w] = x3w_plan_entry<true>(ent, n_ent, so, F, entries[w], starts[w], lens[w], g);
    gstart[w] = g;
  }
}
