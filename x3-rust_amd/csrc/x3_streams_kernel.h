// x3_streams_kernel.h -- the frame walk of MANY independent streams in one launch set (x3_decode_streams_dev,
// include/x3hip.h "BATCHES OF STREAMS").
//
// The fast path of x3_index_kernels.h made segmented.  Every entry (a stream at any byte offset of one device buffer) is
// cut into spans of X3T_SPAN_BYTES; a span belongs to exactly one entry, so its workgroup tests only that entry's byte
// offsets and states its candidates RELATIVE to the entry's start, with the walk's length rules taken against the entry's
// own length and phantom bytes.  One exclusive scan of the spans' counts and sample sums (x3_index_chain_kernel) numbers
// every candidate of the batch; an entry's spans are consecutive, so its first candidate and its sample base are the
// scans' values at its first span, and a difference gives everything relative to the entry.  The link kernel then checks,
// per entry, that the candidates are one clean chain from offset 0, and writes the decoder's frame table: byte offsets
// into the buffer and sample offsets entry * row_len + position.  A candidate the decoder must not see -- not a frame the
// walk steps over, a frame that does not fit its row, a row offset off the four-sample grid the multi-wave decoders need
// -- gets the offset x3_len: every decoder and the check pass give such a frame a status without reading or writing
// anything.  Its entry is then not clean, and so is every entry whose chain breaks: the host walks those again with the
// general walk when the result is asked for.
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

// 1. candidates of one span (x3_index_candidates_kernel<true>, segmented): count[b], samp[b] and the span's candidates in
// offset order at cand[b * X3I_WG_CANDS ...], offsets relative to the entry
__global__ void __launch_bounds__(256)
x3_streams_candidates_kernel(const uint32_t* __restrict__ xw, uint64_t x3_len, const uint64_t* __restrict__ eoff,
                             const uint64_t* __restrict__ elen, const uint32_t* __restrict__ span_first, uint32_t n,
                             uint64_t phantom, X3Cand* __restrict__ cand, unsigned int* __restrict__ count,
                             unsigned long long* __restrict__ samp, uint32_t* __restrict__ ent_flags) {
  __shared__ X3Cand s_c[X3I_WG_CANDS];
  __shared__ uint32_t s_n, s_nraw;
  __shared__ unsigned long long s_raw[X3I_WG_RAW];
  if (threadIdx.x == 0) { s_n = 0; s_nraw = 0; }
  __syncthreads();
  const uint32_t b = blockIdx.x;
  const uint32_t e = x3t_entry_of(span_first, n, b);
  const uint64_t a = eoff[e], L = elen[e];
  const uint64_t lo = a + (uint64_t)(b - span_first[e]) * X3T_SPAN_BYTES;
  const uint64_t hi = lo + X3T_SPAN_BYTES < a + L ? lo + X3T_SPAN_BYTES : a + L;   // header offsets [lo, hi) of this span
  const uint64_t n_dw = (x3_len + 3) >> 2;
  auto consider = [&](uint64_t off) {
    uint32_t plen, samples;
    if (x3i_read_header(xw, n_dw, off, plen, samples) != X3D_OK) return;
    X3Cand cd;
    cd.off = off - a;
    cd.plen_kind = plen | (x3i_kind(L, L + phantom, off - a, plen, samples, 0u) << 16);
    cd.samples = samples;
    const uint32_t li = atomicAdd(&s_n, 1u);
    if (li < X3I_WG_CANDS) s_c[li] = cd;
  };
  for (uint64_t t = (lo >> 4) + threadIdx.x; 16 * t < hi; t += blockDim.x) {
    uint32_t w[5];
    if (4 * t + 4 < n_dw) {
      const uint4 v = reinterpret_cast<const uint4*>(xw)[t];
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      w[4] = xw[4 * t + 4];
    } else {
#pragma unroll
      for (int d = 0; d < 5; ++d) w[d] = 4 * t + d < n_dw ? xw[4 * t + d] : 0u;
    }
    // the key 0x78 0x33 at any of the sixteen byte offsets? (x3_index_candidates_kernel's filter)
    uint32_t hit = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t ev = w[d] ^ 0x33783378u;
      const uint32_t o = __builtin_amdgcn_alignbit(w[d + 1], w[d], 8) ^ 0x33783378u;
      hit |= ((ev - 0x00010001u) & ~ev) | ((o - 0x00010001u) & ~o);
    }
    if ((hit & 0x80008000u) == 0) continue;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t lw = w[k >> 2] >> (8 * (k & 3));
      const uint32_t hw = ((k & 3) == 3 ? (lw & 0xFFu) | ((w[(k >> 2) + 1] & 0xFFu) << 8) : lw) & 0xFFFFu;
      if (hw != 0x3378u) continue;
      const uint64_t off = 16 * t + k;
      if (off < lo || off >= hi || off + 20 > a + L) continue;   // (the entry's bytes only)
      const uint32_t ri = atomicAdd(&s_nraw, 1u);
      if (ri < X3I_WG_RAW) { s_raw[ri] = off; continue; }
      consider(off);
    }
  }
  __syncthreads();
  {
    const uint32_t nraw = s_nraw < X3I_WG_RAW ? s_nraw : X3I_WG_RAW;
    for (uint32_t i = threadIdx.x; i < nraw; i += blockDim.x) consider(s_raw[i]);
  }
  __syncthreads();
  const uint32_t mine = s_n < X3I_WG_CANDS ? s_n : X3I_WG_CANDS;
  if (threadIdx.x == 0) {
    if (s_n > X3I_WG_CANDS) atomicOr(&ent_flags[e], X3T_DIRTY);
    count[b] = mine;
  }
  X3Cand* const dst = cand + (size_t)b * X3I_WG_CANDS;
  for (uint32_t i = threadIdx.x; i < mine; i += blockDim.x) {
    const X3Cand me = s_c[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < mine; ++j) rank += s_c[j].off < me.off ? 1u : 0u;
    dst[rank] = me;
  }
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
    for (uint32_t j = 0; j < mine; ++j) tot += s_c[j].samples;
    samp[b] = tot;
  }
}

// 2. (x3_index_chain_kernel: exclusive scans of count and samp over all spans)

// 3. candidate i of span b is candidate k = base[b] + i of the batch.  Checks the entry's chain, writes the decoder's
// frame table (frame_off, wav_off), the candidate's entry (fent) and, for the entry's last candidate, where it ends and
// the entry's sample count behind it.  x4: the decode launch needs row offsets that are multiples of four samples.
__global__ void __launch_bounds__(64)
x3_streams_link_kernel(const X3Cand* __restrict__ cand_wg, const unsigned int* __restrict__ count,
                       const uint32_t* __restrict__ base, const unsigned long long* __restrict__ sbase, uint32_t G,
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
  const unsigned long long k0 = base[fs];
  const X3Cand* const mine = cand_wg + (size_t)b * X3I_WG_CANDS;
  bool dirty = false;
  for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
    const X3Cand cd = mine[i];
    const unsigned long long k = (unsigned long long)base[b] + i;
    unsigned long long acc = sbase[b] - sbase[fs];
    for (uint32_t j = 0; j < i; ++j) acc += mine[j].samples;
    const unsigned long long end = cd.off + 20ull + (cd.plen_kind & 0xFFFFu);
    bool ok = (cd.plen_kind >> 16) == X3I_CONT;
    if (k == k0) ok = ok && cd.off == 0ull;
    unsigned long long next_off = ~0ull;
    if (i + 1u < cnt) {
      next_off = mine[i + 1u].off;
    } else {
      for (uint32_t b2 = b + 1u; b2 < fe && b2 < G; ++b2)
        if (count[b2]) { next_off = cand_wg[(size_t)b2 * X3I_WG_CANDS].off; break; }
    }
    if (next_off != ~0ull) {
      ok = ok && end == next_off;
    } else {
      ent_end[e] = end;
      ent_nsamp[e] = acc + cd.samples;
    }
    // what the decoder may see: a frame the walk steps over, inside its row, on the grid the launch needs
    const bool live = (cd.plen_kind >> 16) == X3I_CONT && acc + cd.samples <= row_len && (!x4 || (acc & 3ull) == 0ull);
    dirty = dirty || !ok || !live;
    frame_off[k] = live ? eoff[e] + cd.off : x3_len;
    wav_off[k] = live ? (unsigned long long)e * row_len + acc : 0ull;
    fent[k] = e;
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
    // every frame good: how the walk ends behind the last one (x3_index_finalize_kernel's ending_at, per entry)
    const uint64_t L = elen[e], believed = L + phantom, pos = m ? ent_end[e] : 0ull;
    int st = X3D_OK;
    if (believed - pos <= 20) {
      st = X3D_OK;
    } else if (L - pos < 20) {
      st = X3D_IO;
    } else {
      uint32_t plen, samples;
      st = x3i_read_header(xw, (x3_len + 3) >> 2, eoff[e] + pos, plen, samples);
      if (st == X3D_OK) {   // (a valid header would be a candidate of the chain; the kinds that end the walk)
        const uint32_t kind = x3i_kind(L, believed, pos, plen, samples, 0u);
        st = kind == X3I_QUIET ? X3D_OK : kind == X3I_IO ? X3D_IO
             : kind == X3I_PLEN ? X3D_FRAME_HEADER_INVALID_PAYLOAD_LEN : X3D_BAD_ARG;
      }
    }
    r.frames_ok = m;
    r.n_out = m ? ent_nsamp[e] : 0ull;
    r.status = st;
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
