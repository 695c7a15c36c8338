// x3_range_levels_kernel.h -- RANGE LEVELS: the level records (x3_levels_kernel.h) of (entry, start, len) ranges of a stream
// (x3_range_levels_dev) or a corpus (x3_corpus_range_levels_dev), bins counted from each range's own start (DESIGN.md
// section 18).
//
// The work follows the ranges, as the window and ranges calls' does: the plan is theirs (x3_range_plan_kernel /
// x3_corpus_range_plan_kernel), the check is theirs (x3_window_check_kernel), the decode is x3w_stretch with the levels'
// consumer (X3LevBinner: a bin in registers, atomics at a bin boundary and at the stretch's end, no store per sample).
//
// ROLLBACK PER PAIR.  A pair is (range, covering frame).  A frame whose status is not 0 adds nothing, so a stretch never adds
// to the caller's records: it adds to the PAIR'S OWN partial rows in the workspace -- per pair, not per frame, because bins are
// counted from the range's start and a frame under two ranges has two sets of bins.  The frame's word is shared by every
// range that covers it: a stretch that fails flags it for all of them.  The merge kernel adds a pair's rows to the caller's
// records only when the word is still X3D_OK behind the accumulate kernel; a flagged frame goes through the reference's
// reader in the fix-up, per pair, once for its status and, if that is 0, once more straight into the caller's records.
//
//  x3_range_plan_kernel / x3_corpus_range_plan_kernel -- as they are
//  x3_range_levels_scan_kernel   -- one workgroup: rows per range R(w), their exclusive scan (row_off, also to the caller),
//      the verdict on ranges without room ({0 frames, X3D_BAD_ARG}, erows[w] = 0), then the scan of the covering frames
//  x3_window_check_kernel        -- as it is
//  x3_range_levels_prep_kernel   -- a lane per pair q = cov_off[w] + k: the frame's samples cut to the range, its first bin
//      and its bin count; and a lane per caller's record: the identities (here the layout is known)
//  x3_range_levels_pair_scan_kernel -- one workgroup: the exclusive scan of the bin counts; pairs that do not fit are counted
//  x3_range_levels_init_kernel   -- identities into the partial rows in use
//  x3_range_levels_accum_kernel  -- a lane per (pair, stretch)
//  x3_range_levels_fixup_kernel  -- a wave per range, frames in order: flagged frames and pairs without rows through the
//      reference's reader; the range's status; the summary
//  x3_range_levels_merge_kernel  -- a lane per partial row, rows of one record side by side in a wave joined first
// The accumulate and fix-up kernels are templates over the SIGNAL and call it by THE SIGNAL PROTOCOL of x3_levels_kernel.h,
// around one x3l_bin_samples each: X3LevSamples (the range-levels calls), X3LevDiff (x3_signal_range_levels_dev /
// x3_corpus_signal_range_levels_dev), X3LevFir (x3_fir_range_levels_dev / x3_corpus_fir_range_levels_dev;
// section 23; the accumulate kernel only), X3LevTone (x3_tone_range_levels_dev / x3_corpus_tone_range_levels_dev; section 25)
// and X3LevToneBank<NT> (x3_tone_bank_range_levels_dev / x3_corpus_tone_bank_range_levels_dev; section 27), whose flushes go to
// n_tones PLANES of the partial rows and of the caller's records.  What this file adds for a signal is only what is a
// property of the ranges' walk, not of a sample:
//  x3_range_levels_lead_kernel   -- X3LevDiff (need 1) and X3LevFir (need T - 1), behind the plan: the frames in front of a
//      range that starts early in its first frame
//  x3_range_levels_seam_kernel   -- X3LevDiff, behind the accumulate kernel: a lane per pair, the difference across the
//      frame's front seam; the fix-up's share of the seams is behind its one flag, kSeam
//  x3_range_levels_fir_fixup_kernel -- X3LevFir: x3_range_levels_fixup_kernel with the last seven samples carried from frame
//      to frame (X3LevFirCarry), a different walk
//  x3_range_levels_fir_seam_kernel  -- X3LevFir, behind the merge: a lane per (pair, stretch), the stretch's first T - 1 positions
//  x3_range_levels_planes_kernel -- X3LevToneBank, behind the prep: the identities of the caller's records in planes 1 and up;
//      the init and merge kernels run once per plane on offset pointers
//
// CAPACITY.  The workspace holds P pairs and cap = rows_cap + P partial rows, both sized on the host.  A pair with q >= P or
// whose rows end behind cap has no rows: accumulate and merge skip it (x3rl_no_rows, recomputed from q and the scan) and the
// fix-up decodes it through the reader.  The bounds cost time, never memory or a result.
//
// Nothing trusts starts, lengths, offsets, sample offsets, index, entry table or bytes: stream reads are the window
// kernels', a pair index is below P, a partial row index below cap, a caller's record index below rows_cap (the range scan
// gives range w records [base, base + erows[w]) inside rows_cap, and every add checks its bin against erows[w]).
#pragma once
#include "x3_levels_kernel.h"

struct X3RLevSummary {
  X3WinSummary w;                // n_bad, first (range << 8 | status), replays (pairs the fix-up decoded), total (rows)
  unsigned long long overflow;   // pairs without partial rows (option "last_range_levels_overflow")
};

struct X3RLevPair {
  uint64_t f;      // the covering frame
  uint32_t w;      // the range
  uint32_t lo, hi; // samples [lo, hi) of the frame lie in the range
  uint32_t r0;     // position of sample lo, counted from the range's start
  uint32_t b0;     // its bin: the pair's first
  uint32_t cnt;    // bins the pair touches (0: the frame failed its check, or nothing of it lies in the range)
};

// samples [lo, hi) of checked frame f (so[f + 1] - so[f] = its samples, 1 .. 65535) in positions [start, start + L), and
// the position of sample lo behind `start`; false: none.  start + L does not wrap (the plan: L <= total, start <= total - L).
__device__ __forceinline__ bool x3rl_cut(const uint64_t* __restrict__ so, uint64_t f, uint64_t start, uint32_t L, uint32_t& lo,
                                         uint32_t& hi, uint32_t& r0) {
  const uint64_t fpos = so[f], end = start + L;
  const uint64_t samples = min(so[f + 1u] - fpos, (uint64_t)0xFFFFu);
  const uint64_t a = start > fpos ? start - fpos : 0u;
  const uint64_t b = end > fpos ? min(end - fpos, samples) : 0u;
  lo = hi = r0 = 0;
  if (a >= b) return false;
  lo = (uint32_t)a;
  hi = (uint32_t)b;
  r0 = (uint32_t)(fpos + a - start);   // (below L: fpos + a < end)
  return true;
}

// the caller's records of range w: where they begin
__device__ __forceinline__ uint64_t x3rl_base(const unsigned long long* __restrict__ row_off, uint64_t stride, uint64_t w) {
  return stride ? w * stride : row_off[w];
}

// pair q has no partial rows of its own: it lies beyond the P pairs the workspace holds, or it touches bins and they end
// behind the capacity (a pair that touches none needs no rows)
__device__ __forceinline__ bool x3rl_no_rows(const unsigned long long* __restrict__ prow, uint64_t q, uint64_t P, uint64_t cap) {
  return q >= P || (prow[q + 1u] > cap && prow[q + 1u] > prow[q]);
}

// ---- range scan: x3w_range_scan with rows where x3_range_scan_kernel has lengths, and no work items
__global__ void __launch_bounds__(1024)
x3_range_levels_scan_kernel(X3WinPlan* __restrict__ plan, uint64_t n, const uint32_t* __restrict__ lens, uint64_t bin_len,
                            uint64_t stride, uint64_t rows_cap, unsigned long long* __restrict__ cov_off,
                            unsigned long long* __restrict__ row_off, uint32_t* __restrict__ erows,
                            uint64_t* __restrict__ out_off, X3RLevSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  const unsigned long long total = x3w_range_scan<false>(
      plan, n, [&](uint64_t w) { return x3l_entry_rows(lens[w], bin_len); }, stride, rows_cap, 1u, cov_off, nullptr, row_off, erows,
      out_off, s);
  if (threadIdx.x == 0) sum->w.total = total;
}

// ---- prep: a lane per pair (below P), and a lane per caller's record: the identities.  Packed: the records of ranges that
// have room (the others stay untouched); padded: all n * stride.
__global__ void __launch_bounds__(256)
x3_range_levels_prep_kernel(const uint64_t* __restrict__ so, const uint64_t* __restrict__ starts, const uint32_t* __restrict__ lens,
                            const X3WinPlan* __restrict__ plan, uint64_t n, const unsigned long long* __restrict__ cov_off,
                            const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows, uint64_t bin_len,
                            uint64_t stride, uint64_t rows_cap, uint64_t P, const int32_t* __restrict__ fst,
                            X3RLevPair* __restrict__ pairs, x3_level* __restrict__ levels) {
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t np = min((uint64_t)cov_off[n], P);
  for (uint64_t q = i0; q < np; q += lanes) {
    const uint64_t w = x3w_owner(cov_off, n, q);
    X3RLevPair pr{plan[w].fa + (q - cov_off[w]), (uint32_t)w, 0, 0, 0, 0, 0};
    if (fst[pr.f] == X3D_OK && x3rl_cut(so, pr.f, starts[w], lens[w], pr.lo, pr.hi, pr.r0)) {
      pr.b0 = (uint32_t)(pr.r0 / bl);
      pr.cnt = (uint32_t)((pr.r0 + (uint64_t)(pr.hi - pr.lo - 1u)) / bl) - pr.b0 + 1u;   // (at most hi - lo <= 65535)
    }
    pairs[q] = pr;
  }
  const x3_level id = X3L_IDENTITY;
  const uint64_t n_rec = stride ? n * stride : min((uint64_t)row_off[n], rows_cap);   // (n * stride <= rows_cap: the host)
  for (uint64_t i = i0; i < n_rec; i += lanes) {
    if (!stride) {
      const uint64_t w = x3w_owner(row_off, n, i);
      if (i - row_off[w] >= erows[w]) continue;   // (no room: [row_off[w], ..) is not this call's to write)
    }
    levels[i] = id;
  }
}

// ---- pair scan: the exclusive scan of the pairs' bin counts (np + 1 words); pairs without rows (x3rl_no_rows: those beyond P,
// whatever their frames hold, and those below it whose bins end behind cap) are counted
__global__ void __launch_bounds__(1024)
x3_range_levels_pair_scan_kernel(const X3RLevPair* __restrict__ pairs, const unsigned long long* __restrict__ cov_off, uint64_t n,
                                 uint64_t P, uint64_t cap, unsigned long long* __restrict__ prow, X3RLevSummary* __restrict__ sum) {
  __shared__ unsigned long long s[1024];
  const uint64_t n_cov = cov_off[n], np = min(n_cov, P);
  unsigned long long over = 0;
  unsigned long long total = x3w_scan_items(
      np, s, [&](uint64_t q) { return (unsigned long long)pairs[q].cnt; },
      [&](uint64_t q, unsigned long long run) {
        prow[q] = run;
        over += pairs[q].cnt && run + pairs[q].cnt > cap ? 1u : 0u;   // (x3rl_no_rows)
      });
  if (threadIdx.x == 0) prow[np] = total;
  (void)x3w_block_excl_scan(over, s, &total);
  if (threadIdx.x == 0) sum->overflow = total + (n_cov - np);
}

// ---- identities into the partial rows in use
__global__ void __launch_bounds__(256)
x3_range_levels_init_kernel(const unsigned long long* __restrict__ cov_off, uint64_t n, uint64_t P, uint64_t cap,
                            const unsigned long long* __restrict__ prow, x3_level* __restrict__ rows) {
  const uint64_t used = min((uint64_t)prow[min((uint64_t)cov_off[n], P)], cap);
  const x3_level id = X3L_IDENTITY;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < used; i += (uint64_t)gridDim.x * blockDim.x) rows[i] = id;
}

// ---- planes: the identities of the caller's records in planes 1 .. planes - 1, where x3_range_levels_prep_kernel wrote plane
// 0's -- the same records by the same tests (packed: those of ranges that have room; padded: all n * stride), one owner
// search per record for all planes.  Bounds: i < rows_cap (n * stride <= rows_cap: the host), t < planes: below planes * rows_cap.
__global__ void __launch_bounds__(256)
x3_range_levels_planes_kernel(uint64_t n, const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows,
                              uint64_t stride, uint64_t rows_cap, uint32_t planes, x3_level* __restrict__ levels) {
  const x3_level id = X3L_IDENTITY;
  const uint64_t n_rec = stride ? n * stride : min((uint64_t)row_off[n], rows_cap);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!stride) {
      const uint64_t w = x3w_owner(row_off, n, i);
      if (i - row_off[w] >= erows[w]) continue;   // (no room: not this call's to write, in any plane)
    }
    for (uint32_t t = 1; t < planes; ++t) levels[t * rows_cap + i] = id;
  }
}

// ---- accumulate: a lane per (pair, stretch) into the pair's own rows -- a bank's planes of them -- by the signal protocol
// (x3_levels_kernel.h).  The lane sees every sample of its stretch and keeps those of the pair's cut [lo, hi): the others go
// to the signal's skip(), so the sample in front of lo is sample lo's history and the phase steps over it; its first position
// is origin() + r0 - lo + s0 for a signal that counts from the stream or entry (pr.w < n: the prep kernel's owner of q).  What
// end() and the watch leave per frame (the edge record, the frame's last sample) several pairs of one frame write with the
// same values.  A pair with an empty cut (a lead frame) runs its stretches for the proof and those, and touches no row: cnt is 0.
template <class Signal>
__global__ void __launch_bounds__(256)
x3_range_levels_accum_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off, X3DevParams p,
                             const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg, uint64_t bin_len,
                             const unsigned long long* __restrict__ cov_off, uint64_t n, uint64_t P, uint64_t cap,
                             const X3RLevPair* __restrict__ pairs, const unsigned long long* __restrict__ prow,
                             x3_level* __restrict__ rows, int32_t* __restrict__ fst, typename Signal::Tail tail) {
  const bool segd = x3w_index_ok(idx, sb);
  const uint32_t ns = segd ? nseg : 1u;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t n_items = min((uint64_t)cov_off[n], P) * ns;
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t* const tab = Signal::lds_table(tail);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += lanes) {
    const uint64_t q = i / ns;
    const uint32_t j = (uint32_t)(i - q * ns);
    const X3RLevPair pr = pairs[q];
    if (fst[pr.f] != X3D_OK) continue;            // (failed its check, or flagged already: nothing to prove here)
    if (x3rl_no_rows(prow, q, P, cap)) continue;   // (the fix-up's)
    x3_level* const mine = rows + prow[q];
    const uint32_t b0 = pr.b0, cnt = pr.cnt, lo = pr.lo, span = pr.hi - pr.lo;
    // a stretch's samples come in order, from sample 0 or from the first sample of block sb * j; the first of them inside
    // the range, if any, is sample max(s0, lo)
    const uint64_t s0 = j ? 1u + (uint64_t)sb * j * p.block_len : 0u;
    Signal sig;
    sig.begin(tail, X3LevAt{pr.f, j, Signal::origin(tail, pr.w) + pr.r0 - lo + s0, tab, true});
    auto flush = [&](uint64_t bin, const X3LevAcc& a) {
      if (bin - b0 < (uint64_t)cnt) sig.flush(mine + (bin - b0), a);
      else sig.drop();
    };
    const int r = x3l_bin_samples(
        (uint64_t)pr.r0 + (s0 > lo ? s0 - lo : 0u), bl,
        [&](auto put_at) { return x3w_stretch(x3, len, frame_off[pr.f], p, idx, segd, sb, nseg, pr.f, j, put_at, sig.watch()); },
        [&](uint32_t s) { return s - lo < span; }, flush, sig);
    sig.end(false);
    if (r < 0) atomicOr(&fst[pr.f], X3W_FLAG);
  }
}

// ---- fix-up: a wave per range (lane 0 works), frames in order; scratch: a block's samples per wave of the grid.  The
// frame words are read, never written: a frame may lie under other ranges, whose waves read it too -- and for the same
// reason the signal's end() is not called: what a frame leaves behind its last sample belongs to the pairs that went the
// fast way (x3rl_fast).  The replay into the records begins the signal at the frame's sample 0 and reads the caller's table.
// kSeam (X3LevDiff): the wave carries the frame in front -- its final status, its last sample, whether its pair went the fast
// way -- adds the seams x3_range_levels_seam_kernel leaves, stores tail[f] of every frame it replays to status 0, and a lead
// frame (k < lead[w]: the plan's first frames lie in front of the range) never gives the range its status.  This is the one
// place where a kernel asks for a signal by a flag, and it stays a flag, not a member of the protocol: what it guards is state
// of THIS walk -- the loop's k, the previous frame's verdict, the plan's lead -- and no property of a sample; a hook would take
// all of that as arguments and be the same lines at a distance.
__device__ __forceinline__ bool x3rl_fast(int32_t word, const unsigned long long* __restrict__ prow, uint64_t q, uint64_t P, uint64_t cap) {
  return word == X3D_OK && !x3rl_no_rows(prow, q, P, cap);
}

template <class Signal>
__global__ void __launch_bounds__(256)
x3_range_levels_fixup_kernel(const uint8_t* __restrict__ x3, const uint64_t* __restrict__ frame_off, const uint64_t* __restrict__ so,
                             const uint64_t* __restrict__ starts, const uint32_t* __restrict__ lens,
                             const X3WinPlan* __restrict__ plan, uint64_t n, X3DevParams p, uint64_t bin_len,
                             const unsigned long long* __restrict__ cov_off, const unsigned long long* __restrict__ row_off,
                             const uint32_t* __restrict__ erows, uint64_t stride, uint64_t P, uint64_t cap,
                             const unsigned long long* __restrict__ prow, const int32_t* __restrict__ fst,
                             x3_level* __restrict__ levels, int32_t* __restrict__ status, int16_t* __restrict__ scratch,
                             uint32_t scratch_per, X3RLevSummary* __restrict__ sum, typename Signal::Tail tail,
                             const uint32_t* __restrict__ lead) {
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (threadIdx.x & 63u) return;
  int16_t* const blk = scratch + wave * (uint64_t)scratch_per;
  const uint64_t bl = x3l_bin_len(bin_len);
  for (uint64_t w = wave; w < n; w += waves) {
    const X3WinPlan pl = plan[w];
    int32_t st = pl.status;
    uint32_t replayed = 0;
    if (st == X3D_OK) {
      const uint64_t start = starts[w], q0 = cov_off[w];
      const uint32_t L = lens[w], R = erows[w];
      uint32_t ld = 0;   // the plan's lead frames (only a signal with a seam has a lead kernel)
      if constexpr (Signal::kSeam) ld = lead[w];
      x3_level* const mine = levels + x3rl_base(row_off, stride, w);
      // kSeam: the frame in front -- its final status (none yet: not X3D_OK), its last sample, the way its pair went
      [[maybe_unused]] int32_t pfs = X3D_BAD_ARG, ptail = 0;
      [[maybe_unused]] bool pfast = false;
      for (uint32_t k = 0; k < pl.ncov; ++k) {
        const uint64_t f = pl.fa + k;
        int32_t fs = fst[f];
        [[maybe_unused]] int32_t ftail = 0;
        [[maybe_unused]] const bool fast = x3rl_fast(fs, prow, q0 + k, P, cap);
        if (fs == X3W_FLAG || (fs == X3D_OK && x3rl_no_rows(prow, q0 + k, P, cap))) {
          const uint8_t* const payload = x3 + frame_off[f] + 20u;
          if constexpr (Signal::kSeam) {
            fs = x3w_replay_frame(payload, p, blk, [&](uint32_t, uint32_t v) { ftail = (int32_t)(int16_t)(uint16_t)v; });
            if (fs == X3D_OK) tail[f] = ftail;
          } else {
            fs = x3w_replay_frame(payload, p, blk, [](uint32_t, uint32_t) {});
          }
          uint32_t lo, hi, r0;
          if (fs == X3D_OK && x3rl_cut(so, f, start, L, lo, hi, r0)) {   // every block decodes: once more, into the records
            Signal sig;
            sig.begin(tail, X3LevAt{f, 0u, Signal::origin(tail, w) + r0 - lo, Signal::table(tail), false});
            auto flush = [&](uint64_t bin, const X3LevAcc& a) {
              if (bin < (uint64_t)R) sig.flush(mine + bin, a);
              else sig.drop();
            };
            const uint32_t span = hi - lo;
            (void)x3l_bin_samples(
                r0, bl, [&](auto put_at) { return x3w_replay_frame(payload, p, blk, put_at); },
                [&](uint32_t s) { return s - lo < span; }, flush, sig);
          }
          ++replayed;
        } else if constexpr (Signal::kSeam) {
          if (fast) ftail = tail[f];   // (the accumulate kernel's: every stretch of the frame is proven, the last one stored it)
        }
        if constexpr (Signal::kSeam) {
          // the seam in front of frame f: both frames end with status 0, sample 0 of f lies in the range; the seam kernel has
          // it iff both pairs went the fast way (the same tests there)
          uint32_t lo, hi, r0;
          if (k >= 1u && fs == X3D_OK && pfs == X3D_OK && !(fast && pfast) && x3rl_cut(so, f, start, L, lo, hi, r0) && lo == 0u &&
              r0 / bl < (uint64_t)R) {
            // (a checked frame: its payload's first two bytes lie inside the stream)
            const uint8_t* const payload = x3 + frame_off[f] + 20u;
            X3LevAcc a;
            a.reset();
            a.add_value(x3l_diff((int32_t)(int16_t)(uint16_t)(((uint32_t)payload[0] << 8) | payload[1]), ptail));
            x3l_merge(mine + r0 / bl, a);
          }
          pfs = fs;
          ptail = ftail;
          pfast = fast;
        }
        // THE STATUS RULE (this kernel's and x3_range_levels_fir_fixup_kernel's): the first COVERING frame in frame order
        // that ends with a status gives it to the range; the frames behind it still count
        if (fs != X3D_OK && st == X3D_OK && k >= ld) st = fs;
      }
    }
    if (replayed) atomicAdd(&sum->w.replays, (unsigned long long)replayed);
    status[w] = st;
    if (st != X3D_OK) {
      atomicAdd(&sum->w.n_bad, 1ull);
      atomicMin(&sum->w.first, (unsigned long long)(w << 8) | (uint32_t)st);
    }
  }
}

// ---- merge: a lane per partial row.  A row counts when its frame's word is X3D_OK: checked, every stretch proven.  Rows of
// the same record that lie side by side in a wave (the boundary bin of a range's neighbouring frames; with one bin, all of
// them) are joined in registers as in x3_levels_merge_kernel, and the first lane of each run adds the sum.
__global__ void __launch_bounds__(256)
x3_range_levels_merge_kernel(const X3RLevPair* __restrict__ pairs, const unsigned long long* __restrict__ cov_off, uint64_t n,
                             uint64_t P, uint64_t cap, const unsigned long long* __restrict__ prow,
                             const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows, uint64_t stride,
                             const x3_level* __restrict__ rows, const int32_t* __restrict__ fst, x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t np = min((uint64_t)cov_off[n], P);
  const uint64_t n_rows = min((uint64_t)prow[np], cap);
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_rows; i0 += lanes) {   // (whole waves)
    const uint64_t i = i0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    if (i < n_rows && np) {
      const uint64_t q = x3w_owner(prow, np, i);
      const X3RLevPair pr = pairs[q];
      const uint64_t bin = (uint64_t)pr.b0 + (i - prow[q]);
      if (fst[pr.f] == X3D_OK && !x3rl_no_rows(prow, q, P, cap) && bin < (uint64_t)erows[pr.w]) {
        const x3_level r = rows[i];
        key = x3rl_base(row_off, stride, pr.w) + bin;   // (below the range's base + erows: inside rows_cap, the range scan)
        a.load(r);
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}

// ---- THE LEAD FRAMES (the signals with history: X3LevDiff, need = 1; X3LevFir, need = T - 1, section 23)
// The first positions of a range need the `need` samples in front of them.  Inside a frame a lane has them: it decodes the
// frame from its start or from a stretch in front.  A range with len > 0 that starts less than `need` samples behind the first
// sample of its first covering frame fa needs the frames in front: checked, proven by all their stretches, their last samples
// known.  This kernel, behind the plan kernel and in front of the range scan, widens such a plan by ld frames (fa - ld,
// ncov + ld), ld the smallest count with start - so[fa - ld] >= need, not past the first frame of its stream or entry, and
// notes it in lead[w]; the frames are then ordinary pairs whose cut is empty (x3rl_cut false, cnt 0).  At most
// min(need, 7) steps whatever so[] says (a checked frame has a sample; one that fails its check ends the history anyway).
// ent: the corpus's entry table (first: the entry's first frame), NULL for a stream (0).
// Bounds: fa - ld >= first >= 0, frames of the table the plan searched; ncov + ld <= F.
// ONE KERNEL FOR BOTH.  The difference had a kernel of its own, whose rule was: one frame, iff fa > first and
// so[fa] == start.  With need = 1 the loop below runs at most once, iff fa > first, and takes the frame unless
// so[fa] <= start and start - so[fa] >= 1, that is iff so[fa] >= start.  The two differ only where so[fa] > start, and no plan
// has that: fa is x3w_search's result (x3w_plan_stream, x3w_plan_entry), whose lower bound moves only to an f with
// so[f] <= start and begins at one the plan has tested (a stream: so[0] <= start; a corpus: `starts` here is the plan's
// gstart, g = so[first_frame] + the caller's entry-relative start, which does not wrap, so so[first_frame] <= g), so
// so[fa] <= start holds for every so[], one that lies included -- the search may then name a wrong frame, never one that
// begins behind the start.  A plan without status 0 or without covering frames passes both rules untouched.  So lead[w] and
// the widened plan are the same word for word, and lead[w] is 0 or 1 when need is 1.
__global__ void __launch_bounds__(256)
x3_range_levels_lead_kernel(const uint64_t* __restrict__ so, const x3_corpus_entry* __restrict__ ent, uint64_t n_ent,
                            const uint32_t* __restrict__ entries, const uint64_t* __restrict__ starts,
                            const uint32_t* __restrict__ lens, uint64_t n, uint32_t need, X3WinPlan* __restrict__ plan,
                            uint32_t* __restrict__ lead) {
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += (uint64_t)gridDim.x * blockDim.x) {
    X3WinPlan pl = plan[w];
    uint32_t ld = 0;
    if (pl.status == X3D_OK && pl.ncov && lens[w] && need) {
      uint64_t first = 0;
      bool known = true;
      if (ent) {
        const uint32_t e = entries[w];
        known = e < n_ent;   // (the plan has refused the others)
        if (known) first = ent[e].first_frame;
      }
      const uint64_t start = starts[w];
      if (known && pl.fa >= first) {
        const uint32_t most = (uint32_t)min((uint64_t)min(need, (uint32_t)X3L_FIR_HIST), pl.fa - first);
        while (ld < most) {
          const uint64_t pos = so[pl.fa - ld];
          if (pos <= start && start - pos >= (uint64_t)need) break;
          ++ld;
        }
        if (ld) {
          pl.fa -= ld;
          pl.ncov += ld;
          plan[w] = pl;
        }
      }
    }
    lead[w] = ld;
  }
}

// ---- seam: a lane per pair q (below P), behind the accumulate kernel.  The difference at the position of frame f's sample
// 0 is the frame's first sample (the 16-bit literal at the start of its payload) minus frame f - 1's last (tail[f - 1]).  It
// is the range's when sample 0 of f lies in the range (the pair's cut has lo == 0) and f - 1 is a frame of the same stream or
// entry: pair q - 1 of the same range -- a covering frame, or the lead frame, which the plan holds only inside the entry.
// This kernel takes the seam iff both pairs went the fast way: both words X3D_OK behind the accumulate kernel (checked, every
// stretch proven, tail[f - 1] stored by the stretch that reached the frame's end) and both with rows (x3rl_fast; a pair with
// cnt 0 needs none).  Every other seam is the fix-up wave's, which tests the same and takes the complement: a seam is counted
// once.  Lanes are joined by record as in x3_range_levels_merge_kernel: with one bin every seam of a range is one record's.
// Bounds: q < min(cov_off[n], P), so pairs[q], pairs[q - 1] and prow[q + 1] lie in the workspace; pr.f and pr.f - 1 are
// frames of the plan; frame f is checked, so its payload's first bytes lie inside the stream; the record is below the
// range's base + erows[w], inside rows_cap (the range scan).
__global__ void __launch_bounds__(256)
x3_range_levels_seam_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off, uint64_t bin_len,
                            const X3RLevPair* __restrict__ pairs, const unsigned long long* __restrict__ cov_off, uint64_t n,
                            uint64_t P, uint64_t cap, const unsigned long long* __restrict__ prow,
                            const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows, uint64_t stride,
                            const int32_t* __restrict__ fst, const int32_t* __restrict__ tail, x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t np = min((uint64_t)cov_off[n], P);
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); q0 < np; q0 += lanes) {   // (whole waves)
    const uint64_t q = q0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    if (q >= 1u && q < np) {
      const X3RLevPair pr = pairs[q], pp = pairs[q - 1u];
      if (pp.w == pr.w && pp.f + 1u == pr.f && pr.cnt && pr.lo == 0u && x3rl_fast(fst[pr.f], prow, q, P, cap) &&
          x3rl_fast(fst[pp.f], prow, q - 1u, P, cap)) {
        const uint64_t bin = (uint64_t)pr.r0 / bl;
        if (bin < (uint64_t)erows[pr.w]) {
          const int32_t head = (int32_t)(int16_t)(uint16_t)(x3w_be32_at(x3, len, frame_off[pr.f] + 20u) >> 16);
          a.add_value(x3l_diff(head, tail[pp.f]));
          key = x3rl_base(row_off, stride, pr.w) + bin;
        }
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}

// ---- FIR RANGE LEVELS (x3_fir_range_levels_dev / x3_corpus_fir_range_levels_dev)
// The call cuts the stream's or entry's FIR signal (x3_levels_kernel.h, X3LevFir): position start + r adds y[start + r] when
// all T samples under the taps exist in the stream or entry and lie in frames that end with status 0.
//
// WHO ADDS A POSITION.  Sample s of covering frame f of range w (pair q), inside the cut [lo, hi), one owner by two tests
// that every side makes the same way:
//   pair q is not fast (x3rl_fast)              -- the fix-up wave, which replays the frame and forms every position from the
//                                                  history it carries;
//   fast, s < T - 1                             -- the fix-up wave again: the taps reach in front of the frame, and what lies
//                                                  there (a fast frame, a replayed one, a failed one, nothing) only the wave
//                                                  that walks the range's frames in order knows.  It reads the frame's first
//                                                  samples from its edge records' heads;
//   fast, s >= T - 1, s - s0 >= T - 1           -- the accumulate lane of the stretch (s0: its first sample), which decoded all
//                                                  T samples itself; into the pair's rows, merged because the pair is fast;
//   fast, s >= T - 1, s - s0 < T - 1            -- x3_range_levels_fir_seam_kernel, from the heads of the stretch and the tails
//                                                  of the stretches in front of it in the SAME frame: s >= T - 1, so they hold
//                                                  all the history.
// The fix-up writes no edge record: a frame it replays for one range (a pair without rows) may be another range's fast frame.
// Edge records are read only for a fast pair's frame: q < P, the frame's word X3D_OK behind the accumulate kernel, so that
// pair's own lanes ran every stretch to its proof and stored all ns records; index f * stride + j with f a frame of the
// plan (< F) and j < ns <= stride.

// The signal, its multiply and x3l_fir_set are x3_levels_kernel.h's.  The loops that collect samples from edge records and
// x3rl_fir_front below are written out in these kernels as they were before the signal protocol: a shared gather and a
// shared front helper were measured in their place, and x3_range_levels_fir_fixup_kernel came out 8 % and the seam kernel
// 5 % slower with no cause visible in the source, so these two kernels are reverted to that form (profiles/levels_protocol/).

// y at the consecutive samples s_first + c, c < m <= 7, of a frame: hd[c] the samples, hist[h] the sample h + 1 in front of
// s_first (h < H).  A position counts when its history is complete (c + H >= T - 1), s_from <= s < s_to and s lies in the
// pair's cut (s - lo < span; its position behind the range's start is r0 + s - lo).  Bins that fill go to the range's records
// `mine` (bin < R) at once; the open one stays in (a, cur) for the caller (cur ~0: none).
__device__ __forceinline__ void x3rl_fir_front(const X3FirTaps& k, const int32_t (&hd)[X3L_FIR_HIST], uint32_t m,
                                               const int32_t (&hist)[X3L_FIR_HIST], uint32_t H, uint32_t s_first, uint32_t s_from,
                                               uint32_t s_to, uint32_t lo, uint32_t span, uint32_t r0, uint64_t bl, uint32_t R,
                                               x3_level* __restrict__ mine, X3LevAcc& a, uint64_t& cur) {
  const uint32_t need = k.T - 1u;
#pragma unroll
  for (int c = 0; c < X3L_FIR_HIST; ++c) {
    const uint32_t s = s_first + (uint32_t)c;
    if ((uint32_t)c < m && (uint32_t)c + H >= need && s >= s_from && s < s_to && s - lo < span) {
      int32_t d[X3L_FIR_HIST];
#pragma unroll
      for (int t = 1; t < X3L_FIR_TAPS; ++t) d[t - 1] = c >= t ? hd[c - t] : hist[t - c - 1];
      const uint64_t bin = ((uint64_t)r0 + (s - lo)) / bl;
      if (bin < (uint64_t)R) {
        if (bin != cur) {
          if (cur != ~0ull) x3l_merge(mine + cur, a);
          a.reset();
          cur = bin;
        }
        a.add_value(x3l_fir_value(k, hd[c], d));
      }
    }
  }
}

// ---- fix-up: a wave per range (lane 0 works), frames in order, as x3_range_levels_fixup_kernel.  The wave carries the last
// seven samples in front of the current frame and how many of them are valid (X3LevFirCarry): none at the plan's first frame
// and behind a frame that ends with a status, all that a frame with status 0 leaves.  A frame it replays (flagged, or a pair
// without rows) is one stretch whose every position it forms from that history, into the caller's records.  Of a fast frame
// it forms the positions s < T - 1 from the heads of the frame's edge records, and refills the history from their tails.  A
// lead frame (k < lead[w]) never gives the range its status.  A lead-frame pair it decodes counts as a replay.
__global__ void __launch_bounds__(256)
x3_range_levels_fir_fixup_kernel(const uint8_t* __restrict__ x3, const uint64_t* __restrict__ frame_off, const uint64_t* __restrict__ so,
                                 const uint64_t* __restrict__ starts, const uint32_t* __restrict__ lens,
                                 const X3WinPlan* __restrict__ plan, uint64_t n, X3DevParams p, const uint2* __restrict__ idx,
                                 uint32_t sb, uint32_t nseg, uint64_t bin_len, const unsigned long long* __restrict__ cov_off,
                                 const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows, uint64_t stride,
                                 uint64_t P, uint64_t cap, const unsigned long long* __restrict__ prow,
                                 const int32_t* __restrict__ fst, x3_level* __restrict__ levels, int32_t* __restrict__ status,
                                 int16_t* __restrict__ scratch, uint32_t scratch_per, X3RLevSummary* __restrict__ sum,
                                 X3LevFirTail ft, const uint32_t* __restrict__ lead) {
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (threadIdx.x & 63u) return;
  int16_t* const blk = scratch + wave * (uint64_t)scratch_per;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint32_t ns = x3w_index_ok(idx, sb) ? nseg : 1u;
  const uint32_t need = ft.k.T - 1u;
  for (uint64_t w = wave; w < n; w += waves) {
    const X3WinPlan pl = plan[w];
    int32_t st = pl.status;
    uint32_t replayed = 0;
    if (st == X3D_OK) {
      const uint64_t start = starts[w], q0 = cov_off[w];
      const uint32_t L = lens[w], R = erows[w], ld = lead[w];
      x3_level* const mine = levels + x3rl_base(row_off, stride, w);
      X3LevFirCarry hs;
      hs.k = ft.k;
      for (uint32_t k = 0; k < pl.ncov; ++k) {
        const uint64_t f = pl.fa + k;
        int32_t fs = fst[f];
        const bool fast = x3rl_fast(fs, prow, q0 + k, P, cap);
        uint32_t lo, hi, r0;
        (void)x3rl_cut(so, f, start, L, lo, hi, r0);   // (none: lo = hi = r0 = 0, no sample is kept)
        const uint32_t span = hi - lo;
        if (fs == X3W_FLAG || (fs == X3D_OK && !fast)) {
          const uint8_t* const payload = x3 + frame_off[f] + 20u;
          fs = x3w_replay_frame(payload, p, blk, [](uint32_t, uint32_t) {});
          if (fs == X3D_OK) {   // every block decodes: once more, into the records and the history
            auto flush = [&](uint64_t bin, const X3LevAcc& a) {
              if (bin < (uint64_t)R) x3l_merge(mine + bin, a);
            };
            (void)x3l_bin_samples(
                r0, bl, [&](auto put_at) { return x3w_replay_frame(payload, p, blk, put_at); },
                [&](uint32_t s) { return s - lo < span; }, flush, hs);
          }
          ++replayed;
        } else if (fs == X3D_OK) {   // fast: every stretch proven, its edge records stored by this pair's own lanes
          const X3FirEdge* const fe = ft.edges + f * ft.stride;
          if (need && span) {        // the positions s < T - 1: the frame's first samples are its first stretches' heads
            int32_t hd[X3L_FIR_HIST] = {0, 0, 0, 0, 0, 0, 0};
            uint32_t m = 0;
            for (uint32_t j = 0; j < ns && m < need; ++j) {
              const X3FirEdge e = fe[j];
              const uint32_t c = min(e.n, (uint32_t)X3L_FIR_HIST);   // (n <= 7: all of the stretch; else m reaches 7)
#pragma unroll
              for (int t = 0; t < X3L_FIR_HIST; ++t) {
                if ((uint32_t)t < c && m < need) {
                  x3l_fir_set(hd, m, (int32_t)e.head[t]);
                  ++m;
                }
              }
            }
            X3LevAcc a;
            a.reset();
            uint64_t cur = ~0ull;
            x3rl_fir_front(ft.k, hd, m, hs.d, hs.cnt, 0u, 0u, need, lo, span, r0, bl, R, mine, a, cur);
            if (cur != ~0ull) x3l_merge(mine + cur, a);
          }
          // the frame's last samples, newest first, are its last stretches' tails
          int32_t tl[X3L_FIR_HIST] = {0, 0, 0, 0, 0, 0, 0};
          uint32_t tc = 0;
          for (uint32_t j = ns; j-- > 0u && tc < (uint32_t)X3L_FIR_HIST;) {
            const X3FirEdge e = fe[j];
            const uint32_t c = min(e.n, (uint32_t)X3L_FIR_HIST);
#pragma unroll
            for (int t = 0; t < X3L_FIR_HIST; ++t) {
              if ((uint32_t)t < c && tc < (uint32_t)X3L_FIR_HIST) {
                x3l_fir_set(tl, tc, (int32_t)e.tail[t]);
                ++tc;
              }
            }
          }
#pragma unroll
          for (int t = X3L_FIR_HIST - 1; t >= 0; --t) {
            if ((uint32_t)t < tc) hs.push(tl[t]);
          }
        }
        hs.cnt = fs == X3D_OK ? min(hs.cnt, (uint32_t)X3L_FIR_HIST) : 0u;
        if (fs != X3D_OK && st == X3D_OK && k >= ld) st = fs;   // (the first COVERING frame in frame order)
      }
    }
    if (replayed) atomicAdd(&sum->w.replays, (unsigned long long)replayed);
    status[w] = st;
    if (st != X3D_OK) {
      atomicAdd(&sum->w.n_bad, 1ull);
      atomicMin(&sum->w.first, (unsigned long long)(w << 8) | (uint32_t)st);
    }
  }
}

// ---- seam: a lane per (pair q below P, stretch j >= 1), behind the merge.  Of a fast pair's stretch it adds the positions
// s0 + c, c < min(n, T - 1), with s0 + c >= T - 1 (the others are the fix-up's): the samples are the stretch's heads, the
// history the tails of the stretches in front of it in the same frame, which hold s0 >= T - 1 - c samples.  The pair is
// fast, so the frame's word is final and the records are the caller's; lanes are joined by record as in
// x3_range_levels_merge_kernel.  The stream is not read.  Bounds: q < min(cov_off[n], P); edge index pr.f * estride + j with
// j < ns <= estride; a record at the range's base + bin with bin < erows[w], inside rows_cap (the range scan).
__global__ void __launch_bounds__(256)
x3_range_levels_fir_seam_kernel(uint32_t block_len, const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg, uint64_t bin_len,
                                const X3RLevPair* __restrict__ pairs, const unsigned long long* __restrict__ cov_off, uint64_t n,
                                uint64_t P, uint64_t cap, const unsigned long long* __restrict__ prow,
                                const unsigned long long* __restrict__ row_off, const uint32_t* __restrict__ erows, uint64_t stride,
                                const int32_t* __restrict__ fst, const X3FirEdge* __restrict__ edges, uint32_t estride, X3FirTaps k,
                                x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ns = x3w_index_ok(idx, sb) ? nseg : 1u;
  const uint32_t need = k.T - 1u;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t n_items = min((uint64_t)cov_off[n], P) * ns;
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_items; i0 += lanes) {   // (whole waves)
    const uint64_t i = i0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    const uint64_t q = i / ns;
    const uint32_t j = (uint32_t)(i - q * ns);
    const uint64_t s0 = 1u + (uint64_t)sb * j * block_len;   // the stretch's first sample
    if (i < n_items && j >= 1u && s0 < 0x10000u) {
      const X3RLevPair pr = pairs[q];
      if (pr.cnt && x3rl_fast(fst[pr.f], prow, q, P, cap)) {
        const X3FirEdge* const fe = edges + pr.f * estride;
        const X3FirEdge e = fe[j];
        if (e.n) {
          int32_t hist[X3L_FIR_HIST] = {0, 0, 0, 0, 0, 0, 0}, hd[X3L_FIR_HIST];
          uint32_t H = 0;
          for (uint32_t wj = j; wj-- > 0u && H < need;) {
            const X3FirEdge h = fe[wj];
            const uint32_t c = min(h.n, (uint32_t)X3L_FIR_HIST);
#pragma unroll
            for (int t = 0; t < X3L_FIR_HIST; ++t) {
              if ((uint32_t)t < c && H < need) {
                x3l_fir_set(hist, H, (int32_t)h.tail[t]);
                ++H;
              }
            }
          }
#pragma unroll
          for (int t = 0; t < X3L_FIR_HIST; ++t) hd[t] = (int32_t)e.head[t];
          x3_level* const mine = levels + x3rl_base(row_off, stride, pr.w);
          uint64_t cur = ~0ull;
          x3rl_fir_front(k, hd, min(e.n, need), hist, H, (uint32_t)s0, need, 0x10000u, pr.lo, pr.hi - pr.lo, pr.r0, bl, erows[pr.w],
                         mine, a, cur);
          if (cur != ~0ull) key = x3rl_base(row_off, stride, pr.w) + cur;
        }
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}
