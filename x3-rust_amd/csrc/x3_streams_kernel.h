// x3_streams_kernel.h -- the frame walk of MANY independent streams in one launch set (x3_decode_streams_dev,
// include/x3hip.h "BATCHES OF STREAMS").
//
// The fast path of x3_index_kernels.h over entries (streams at any byte offset of one device buffer): these kernels call its
// helpers for every walk rule (x3i_load_chunk, x3i_scan_chunk, x3i_consider, x3i_store_span, x3i_link, x3i_walk_end) and
// keep what is per entry.  Each entry is cut into spans of X3T_SPAN_BYTES, a workgroup's each, whose candidates carry
// offsets RELATIVE to the entry and the walk's kind against the entry's own length and phantom bytes.  One exclusive scan
// over all spans (x3_index_chain_kernel) numbers every candidate; an entry's spans are consecutive, so its first candidate
// and sample base are the scans at its first span.  The link kernel checks each entry's chain and writes the decoder's frame
// table (buffer offsets, sample offsets entry * row_len + position).  A candidate the decoder must not see -- not a frame
// the walk steps over, past its row, off the four-sample grid of the multi-wave decoders -- gets the offset x3_len, which
// every decoder and the check pass give a status without reading or writing; its entry, like one whose chain breaks, is
// left to the general walk at result time.
#pragma once
#include "x3_index_kernels.h"

#define X3T_SPAN_BYTES 65536ull   // bytes of an entry one scanning workgroup covers (4 096 chunks of 16 bytes)
#define X3T_DIRTY 1u              // ent_flags: not one clean chain (or a frame the fast path leaves alone)

struct X3StreamsSum {
  unsigned long long bad_first;   // min over entries with status != 0 of (entry << 8 | status)
  unsigned int n_bad;             // entries with status != 0 (clean entries only)
  unsigned int n_dirty;           // entries left to the general walk (their numbers: dirty[0 .. n_dirty))
  unsigned int over;              // the candidates outnumber the frames the decode launch covered
  unsigned int pad[3];
};

// the entry span b belongs to: the last e with span_first[e] <= b (entries without bytes have no span)
__device__ __forceinline__ uint32_t x3t_entry_of(const uint32_t* __restrict__ span_first, uint32_t n, uint32_t b) {
  uint32_t lo = 0, hi = n;   // span_first[lo] <= b < span_first[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (span_first[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 1. candidates of one span (x3_index_candidates_kernel<true>'s scan, over the span's chunks): count[b], samp[b] and the
// span's candidates in offset order at cand[b * X3I_WG_CANDS ...], offsets relative to the entry
__global__ void __launch_bounds__(256)
x3_streams_candidates_kernel(const uint32_t* __restrict__ xw, uint64_t x3_len, const uint64_t* __restrict__ eoff,
                             const uint64_t* __restrict__ elen, const uint32_t* __restrict__ span_first, uint32_t n,
                             uint64_t phantom, X3Cand* __restrict__ cand, unsigned int* __restrict__ count,
                             unsigned long long* __restrict__ samp, uint32_t* __restrict__ ent_flags) {
  __shared__ X3ScanLds s;
  if (threadIdx.x == 0) { s.n = 0; s.nraw = 0; }
  __syncthreads();
  const uint32_t b = blockIdx.x;
  const uint32_t e = x3t_entry_of(span_first, n, b);
  const uint64_t a = eoff[e], L = elen[e];
  const uint64_t lo = a + (uint64_t)(b - span_first[e]) * X3T_SPAN_BYTES;
  const uint64_t hi = lo + X3T_SPAN_BYTES < a + L ? lo + X3T_SPAN_BYTES : a + L;   // header offsets [lo, hi) of this span
  const uint64_t end = hi + 19 < a + L ? hi + 19 : a + L;                          // ... whose 20 bytes lie in the entry
  const uint64_t n_dw = (x3_len + 3) >> 2;
  auto consider = [&](uint64_t off) {
    X3Cand cd;
    x3i_consider(s, xw, n_dw, off, a, L, L + phantom, 0u, cd);
  };
  for (uint64_t t = (lo >> 4) + threadIdx.x; 16 * t < hi; t += blockDim.x) {
    uint32_t w[5];
    x3i_load_chunk(xw, n_dw, t, w);
    x3i_scan_chunk(w, t, lo, end, s, consider);
  }
  x3i_check_raw(s, consider);
  x3i_store_span(s, b, cand, count, samp, &ent_flags[e], X3T_DIRTY);
}

// 2. (x3_index_chain_kernel: exclusive scans of count and samp over all spans)

// 3. candidate i of span b is candidate k = base[b] + i of the batch.  Checks the entry's chain, writes the decoder's
// frame table (frame_off, wav_off), the candidate's entry (fent) and, for the entry's last candidate, where it ends and
// the entry's sample count behind it.  x4: the decode launch needs row offsets that are multiples of four samples.
__global__ void __launch_bounds__(64)
x3_streams_link_kernel(const X3Cand* __restrict__ cand_wg, const unsigned int* __restrict__ count,
                       const uint32_t* __restrict__ base, const unsigned long long* __restrict__ sbase,
                       const uint64_t* __restrict__ eoff, const uint32_t* __restrict__ span_first, uint32_t n,
                       uint64_t x3_len, uint64_t row_len, uint32_t x4, unsigned long long* __restrict__ frame_off,
                       unsigned long long* __restrict__ wav_off, uint32_t* __restrict__ fent,
                       uint32_t* __restrict__ ent_flags, unsigned long long* __restrict__ ent_end,
                       unsigned long long* __restrict__ ent_nsamp) {
  const uint32_t b = blockIdx.x;
  const uint32_t cnt = count[b];
  if (cnt == 0) return;
  const uint32_t e = x3t_entry_of(span_first, n, b);
  const uint32_t fs = span_first[e], fe = span_first[e + 1];
  const unsigned long long k0 = base[fs], s0 = sbase[fs];   // the entry's first candidate and sample base
  bool dirty = false;
  for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
    const X3Link l = x3i_link(cand_wg, count, base, sbase, b, cnt, i, fe, k0, s0);
    if (l.next == ~0ull) {   // the entry's last candidate
      ent_end[e] = l.end;
      ent_nsamp[e] = l.acc + l.cd.samples;
    }
    // what the decoder may see: a frame the walk steps over, inside its row, on the grid the launch needs
    const bool live = (l.cd.plen_kind >> 16) == X3I_CONT && l.acc + l.cd.samples <= row_len &&
                      (!x4 || (l.acc & 3ull) == 0ull);
    dirty = dirty || !l.ok || !live;
    frame_off[l.k] = live ? eoff[e] + l.cd.off : x3_len;
    wav_off[l.k] = live ? (unsigned long long)e * row_len + l.acc : 0ull;
    fent[l.k] = e;
  }
  if (dirty) atomicOr(&ent_flags[e], X3T_DIRTY);
}

// 4. per frame of a clean entry that failed (merged status: check pass first, then the decoder): the entry's first one
__global__ void __launch_bounds__(256)
x3_streams_firstbad_kernel(const int32_t* __restrict__ status, const uint32_t* __restrict__ fent, uint64_t F,
                           const unsigned long long* __restrict__ d_nf, unsigned long long* __restrict__ ent_bad) {
  const uint64_t nf = *d_nf < F ? *d_nf : F;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nf; k += (uint64_t)gridDim.x * blockDim.x)
    if (status[k] != 0) atomicMin(&ent_bad[fent[k]], (unsigned long long)k);
}

// 5. one thread per entry: x3_decode_stream_dev's verdict on a clean entry (x3_stream_result), its sample count in
// nout[e] (~0: left to the general walk, listed in dirty[])
__global__ void __launch_bounds__(256)
x3_streams_resolve_kernel(const uint32_t* __restrict__ xw, uint64_t x3_len, const uint64_t* __restrict__ eoff,
                          const uint64_t* __restrict__ elen, const uint32_t* __restrict__ span_first, uint32_t n,
                          uint64_t phantom, const uint32_t* __restrict__ base, uint32_t G,
                          const unsigned long long* __restrict__ d_nf, uint64_t F, const int32_t* __restrict__ status,
                          const unsigned long long* __restrict__ wav_off, const uint32_t* __restrict__ ent_flags,
                          const unsigned long long* __restrict__ ent_bad, const unsigned long long* __restrict__ ent_end,
                          const unsigned long long* __restrict__ ent_nsamp, uint64_t row_len,
                          x3_stream_result* __restrict__ results, unsigned long long* __restrict__ nout,
                          uint32_t* __restrict__ dirty, X3StreamsSum* __restrict__ sum) {
  const unsigned long long total = *d_nf;
  if (total > F) {   // the decode launch did not cover every candidate: the host launches it again with the count
    if (blockIdx.x == 0 && threadIdx.x == 0) sum->over = 1u;
    return;
  }
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (ent_flags[e] & X3T_DIRTY) {
    nout[e] = ~0ull;
    dirty[atomicAdd(&sum->n_dirty, 1u)] = e;
    return;
  }
  const uint32_t fs = span_first[e], fe = span_first[e + 1];
  const unsigned long long k0 = fs < G ? base[fs] : total, k1 = fe < G ? base[fe] : total;
  const unsigned long long m = k1 - k0;
  const unsigned long long kb = ent_bad[e];
  x3_stream_result r;
  r.frame_errors = 0u;
  if (kb < k1) {
    const int32_t st = status[kb];
    r.frames_ok = kb - k0;
    r.n_out = wav_off[kb] - (unsigned long long)e * row_len;
    if (st == X3D_OUT_OF_BOUNDS_INVERSE || st == X3D_FRAME_DECODE_INVALID_BPF) {
      r.status = 0;
      r.frame_errors = 1u;   // counted, the walk ends quietly (decodefile.rs:129-135)
    } else {
      r.status = st;
    }
  } else {
    // every frame good: how the walk ends behind the last one
    const uint64_t L = elen[e];
    r.frames_ok = m;
    r.n_out = m ? ent_nsamp[e] : 0ull;
    r.status = x3i_walk_end(xw, (x3_len + 3) >> 2, eoff[e], L, L + phantom, m ? ent_end[e] : 0ull, 0u);
  }
  results[e] = r;
  nout[e] = r.n_out;
  if (r.status != 0) {
    atomicAdd(&sum->n_bad, 1u);
    atomicMin(&sum->bad_first, ((unsigned long long)e << 8) | (uint32_t)(r.status & 0xFF));
  }
}

// 6. the rows: zeros from n_out on (int16, in place), or every sample as float32 from the int16 workspace.  Rows
// blockIdx.y, blockIdx.y + gridDim.y, ...; entries left to the general walk (nout = ~0) are its business.  nout == nullptr:
// one row of no_value samples (the general walk's rows).
template <bool F32>
__global__ void __launch_bounds__(256)
x3_streams_rows_kernel(const int16_t* __restrict__ ws, void* __restrict__ out, uint64_t n, uint64_t row_len,
                       const unsigned long long* __restrict__ nout, unsigned long long no_value,
                       const X3StreamsSum* __restrict__ sum) {
  if (sum && sum->over) return;
  for (uint64_t r = blockIdx.y; r < n; r += gridDim.y) {
    const unsigned long long no = nout ? nout[r] : no_value;
    if (no == ~0ull) continue;
    const uint64_t from = F32 ? 0ull : no;
    for (uint64_t i = from + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < row_len; i += (uint64_t)gridDim.x * blockDim.x) {
      if (F32) {
        reinterpret_cast<float*>(out)[r * row_len + i] = i < no ? (float)ws[r * row_len + i] * (1.0f / 32768.0f) : 0.0f;
      } else {
        reinterpret_cast<int16_t*>(out)[r * row_len + i] = 0;
      }
    }
  }
}

// ---- CORPUS (x3_corpus_build): the same walk as an index.  Its link step is x3_streams_link_kernel
// with row_len = ~0 and x4 = 0: every frame the walk steps over is live, at its buffer offset, whatever its position.

// C1. one thread per entry: a clean entry's candidates [k0, k0 + m) are its frames, its walk ends as x3i_walk_end says
// behind them; m = ~0 marks an entry left to the general walk
__global__ void __launch_bounds__(256)
x3_corpus_walk_kernel(const uint32_t* __restrict__ xw, uint64_t x3_len, const uint64_t* __restrict__ eoff,
                      const uint64_t* __restrict__ elen, const uint32_t* __restrict__ span_first, uint32_t n, uint64_t phantom,
                      const uint32_t* __restrict__ base, uint32_t G, const unsigned long long* __restrict__ d_total,
                      const uint32_t* __restrict__ ent_flags, const unsigned long long* __restrict__ ent_end,
                      unsigned long long* __restrict__ ent_k0, unsigned long long* __restrict__ ent_m,
                      int32_t* __restrict__ ent_st) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (ent_flags[e] & X3T_DIRTY) {
    ent_k0[e] = 0ull;
    ent_m[e] = ~0ull;
    ent_st[e] = 0;
    return;
  }
  const unsigned long long total = *d_total;
  const uint32_t fs = span_first[e], fe = span_first[e + 1];
  const unsigned long long k0 = fs < G ? base[fs] : total, k1 = fe < G ? base[fe] : total;
  const uint64_t L = elen[e];
  ent_k0[e] = k0;
  ent_m[e] = k1 - k0;
  ent_st[e] = x3i_walk_end(xw, (x3_len + 3) >> 2, eoff[e], L, L + phantom, k1 > k0 ? ent_end[e] : 0ull, 0u);
}

// C2. one thread per candidate: a clean entry's frame goes to its place in the corpus's frame table (entries in order);
// the general walk's entries are filled from the host
__global__ void __launch_bounds__(256)
x3_corpus_compact_kernel(const unsigned long long* __restrict__ frame_off, const uint32_t* __restrict__ fent, uint64_t cap,
                         const unsigned long long* __restrict__ d_total, const unsigned long long* __restrict__ ent_k0,
                         const x3_corpus_entry* __restrict__ ent, uint64_t F, uint64_t* __restrict__ out) {
  const unsigned long long total = *d_total < cap ? *d_total : cap;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
    const x3_corpus_entry& en = ent[fent[k]];
    if (en.general_walk) continue;
    const uint64_t i = k - ent_k0[fent[k]];
    if (i < en.n_frames && en.first_frame + i < F) out[en.first_frame + i] = frame_off[k];
  }
}
