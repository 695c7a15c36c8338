// x3_levels_kernel.h -- LEVELS: min, max, count, sum and sum of squares per bin of sample positions, for a stream
// (x3_levels_dev) or every entry of a corpus (x3_corpus_levels_dev), without a sample buffer.
//
// The decode is x3_decode_window_kernel.h's: x3w_check_frame per frame, x3w_stretch per (frame, stretch) with its proof
// against the next usable index entry, x3w_replay_frame for the frames a stretch flags.  What differs is the consumer: put()
// adds the sample to five registers and stores nothing; a lane touches memory (beyond the bit window's refills) only where
// its position crosses a bin boundary and at its end.  All five quantities are integers: the result does not depend on the
// order in which lanes arrive.
//
// ROLLBACK.  A frame whose status is not 0 must add nothing, also when its first stretches decoded cleanly, and a stretch
// cannot know how the frame's other stretches end.  So a stretch never adds to the caller's bins.  It adds to the FRAME'S
// OWN partial rows in the workspace: frame f touches bins b0 .. b1 (clipped to its stream's bins), an exclusive scan of
// b1 - b0 + 1 gives it rows [row[f], row[f + 1]) -- with the positions of consecutive frames back to back that is at most
// n_bins + n_frames rows in all, which is what the workspace holds.  Only when every stretch of the frame has been proven
// (its word is still X3D_OK behind the accumulate kernel) does the merge kernel add the frame's rows to the caller's bins.  A
// flagged frame's rows are never read again: the fix-up kernel decodes it through the reference's reader, once for its
// status and, if that is 0, a second time straight into the caller's bins.  Frames whose rows would not fit (offsets out
// of order: not this stream's) are flagged by the scan and take that path too.
//
//  x3_levels_init_kernel     -- identities into every caller's record and every partial row; the summary
//  x3_levels_check_kernel    -- a wave per frame of the table: x3w_check_frame
//  x3_corpus_levels_rows_kernel / x3_levels_prep_kernel / x3_corpus_levels_prep_kernel
//                            -- per frame: its position, its stream's rows in d_levels, its first bin, its row count
//  x3_levels_scan_kernel     -- one workgroup: the exclusive scan of the row counts; frames that do not fit are flagged
//  x3_levels_accum_kernel    -- a lane per (frame, stretch)
//  x3_levels_fixup_kernel    -- a wave per frame: flagged frames through the reference's reader; d_frame_status, summary
//  x3_levels_merge_kernel    -- a lane per partial row; rows of one bin that lie side by side in a wave are joined first
//  x3_levels_seam_kernel     -- X3_LEVEL_SIGNAL_DIFF only: a lane per frame, the one difference across the frame's front seam
//  x3_levels_fir_seam_kernel -- x3_fir_levels_dev only: a lane per (frame, stretch), the stretch's first T - 1 positions
//  x3_tone_power_kernel      -- x3_tone_power_levels_dev: a lane per tone record, the record of the band's level
// The accumulate and fix-up kernels are templates over the SIGNAL, what a position adds to its bin, and call it by THE SIGNAL
// PROTOCOL (below, in front of the signals): X3LevSamples (the levels calls), X3LevDiff (x3_signal_levels_dev; DESIGN.md
// section 20), X3LevFir (x3_fir_levels_dev; section 22), X3LevTone (x3_tone_levels_dev; section 24) or X3LevToneBank<NT>
// (x3_tone_bank_levels_dev; section 26), NT of the last in one pass, whose records go to NT planes of the partial rows and of
// the caller's records.  x3_range_levels_kernel.h runs the same signals over ranges.
//
// What the range levels, events and quantiles kernels (x3_range_levels_kernel.h, x3_events_kernel.h, x3_quantiles_kernel.h)
// share with these: X3L_IDENTITY, the record of an empty bin; X3LevAcc, a record in registers (load, record, join);
// x3l_bin_samples, the sequence "open a binner, decode into it, flush the open bin"; x3l_merge_runs, the keyed wave join.
//
// Nothing trusts offsets, sample offsets, index, entry table or bytes: stream reads are those of the window kernels, every
// partial row index is below the workspace's row count, every caller's record index below n_rows.
#pragma once
#include "x3_decode_window_kernel.h"

#define X3L_DONE 0x20000      // per-frame word: the fix-up has given the frame its status (low 16 bits) by the reader
#define X3L_FAR 0x20000u      // "the bin does not end inside this frame": more than a frame's 65 535 samples

struct X3LevSummary {
  unsigned long long n_bad;     // frames with status != 0
  unsigned long long first;     // min(f << 8 | status) over them
  unsigned long long replays;   // frames the fix-up decoded through the reference's reader (option "last_levels_replays")
};

struct X3LevFrame {
  uint64_t pos;     // position of the frame's sample 0 in its stream / entry
  uint64_t obase;   // d_levels record of that stream's / entry's bin 0
  uint64_t nlim;    // its bins (0: the frame belongs to no entry, nothing is counted)
  uint64_t b0;      // the frame's first bin
};

__device__ __forceinline__ uint64_t x3l_bin_len(uint64_t bin_len) { return bin_len ? bin_len : ~0ull; }   // 0: one bin

// the record of a bin without samples: what every join leaves as it is
constexpr x3_level X3L_IDENTITY{0, 0, 32767, -32768, 0, 0};

// the registers of a bin
struct X3LevAcc {
  uint64_t sum_sq;
  int64_t sum;
  int32_t mn, mx;
  uint32_t n;
  __device__ __forceinline__ void load(const x3_level& r) {
    sum_sq = r.sum_sq;
    sum = r.sum;
    mn = r.min;
    mx = r.max;
    n = r.n;
  }
  __device__ __forceinline__ x3_level record() const { return x3_level{sum_sq, sum, mn, mx, n, 0}; }
  __device__ __forceinline__ void reset() { load(X3L_IDENTITY); }
  __device__ __forceinline__ void add(uint32_t v) { add_value((int32_t)(int16_t)(uint16_t)v); }
  __device__ __forceinline__ void add_value(int32_t s) {   // -32768 <= s <= 32767
    sum_sq += (uint32_t)(s * s);
    sum += s;
    mn = min(mn, s);
    mx = max(mx, s);
    ++n;
  }
  __device__ __forceinline__ void join(const X3LevAcc& o) {
    sum_sq += o.sum_sq;
    sum += o.sum;
    mn = min(mn, o.mn);
    mx = max(mx, o.mx);
    n += o.n;
  }
  // ... of the 64 lanes of a wave: every lane calls and holds the sum
  __device__ __forceinline__ void join_wave() {
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) {
      X3LevAcc o;
      o.sum_sq = (uint64_t)__shfl_xor((long long)sum_sq, d, X3_WAVE);
      o.sum = (int64_t)__shfl_xor((long long)sum, d, X3_WAVE);
      o.mn = __shfl_xor(mn, d, X3_WAVE);
      o.mx = __shfl_xor(mx, d, X3_WAVE);
      o.n = (uint32_t)__shfl_xor((int)n, d, X3_WAVE);
      join(o);
    }
  }
};

// ... into a record that other lanes add to as well
__device__ __forceinline__ void x3l_merge(x3_level* __restrict__ r, const X3LevAcc& a) {
  if (a.n == 0u) return;
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_sq), (unsigned long long)a.sum_sq);
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum), (unsigned long long)a.sum);
  atomicMin(&r->min, a.mn);
  atomicMax(&r->max, a.mx);
  atomicAdd(&r->n, a.n);
}

// The keyed join of a wave: lane `lane` holds the registers `a` of record levels[key] (~0: none).  Lanes with the same key
// that lie side by side form a run -- a lane starts one where its key differs from its left neighbour's (or it has none) --
// whose registers are joined, and the first lane of each run adds the sum to the record.  Every lane of the wave calls.
__device__ __forceinline__ void x3l_merge_runs(x3_level* __restrict__ levels, uint64_t key, X3LevAcc a, uint32_t lane) {
  const uint64_t left = (uint64_t)__shfl_up((long long)key, 1, X3_WAVE);
  const bool head = lane == 0u || key == ~0ull || left != key;
  const unsigned long long heads = __ballot(head);
  const uint32_t run = (uint32_t)__popcll(heads & (~0ull >> (63u - lane)));
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    X3LevAcc o;
    o.sum_sq = (uint64_t)__shfl_down((long long)a.sum_sq, d, X3_WAVE);
    o.sum = (int64_t)__shfl_down((long long)a.sum, d, X3_WAVE);
    o.mn = __shfl_down(a.mn, d, X3_WAVE);
    o.mx = __shfl_down(a.mx, d, X3_WAVE);
    o.n = (uint32_t)__shfl_down((int)a.n, d, X3_WAVE);
    const uint32_t orun = (uint32_t)__shfl_down((int)run, d, X3_WAVE);
    if (lane + d < 64u && orun == run) a.join(o);
  }
  if (head && key != ~0ull) x3l_merge(levels + key, a);
}

// Consecutive positions from g on: `left` samples are still missing in bin `bin` (X3L_FAR: more than any frame has, so
// a count that reaches 0 is always a real boundary).  flush(bin, acc) takes a finished or abandoned bin.
struct X3LevBinner {
  X3LevAcc a;
  uint64_t bin;
  uint32_t left, step;
  __device__ __forceinline__ void open(uint64_t g, uint64_t bl) {
    a.reset();
    bin = g / bl;
    const uint64_t rem = bl - (g - bin * bl);
    left = rem < X3L_FAR ? (uint32_t)rem : X3L_FAR;
    step = bl < X3L_FAR ? (uint32_t)bl : X3L_FAR;
  }
  // one position: the signal decides what it adds to the open bin, if anything; the position counts either way
  template <class Signal, class Flush>
  __device__ __forceinline__ void put(Signal&& sig, uint32_t v, Flush flush) {
    sig.add(a, v);
    if (--left == 0u) {
      flush(bin, a);
      a.reset();
      ++bin;
      left = step;
    }
  }
};

// THE SIGNAL PROTOCOL.  A signal is what a position adds to its bin.  The accumulate and fix-up kernels of this file and of
// x3_range_levels_kernel.h are templates over it; they call the members below and never ask which signal they hold, so a new
// signal is a struct here and a case in the host's two switches.
//   Tail                -- the kernels' last argument: what the signal takes from the call
//   lds_table(tail)     -- the accumulate kernels, every lane in front of the item loop: the workgroup's LDS copy of the
//                          signal's table (NULL: it has none); table(tail): the caller's array, which the fix-ups read
//   origin(tail, w)     -- the range kernels only: the position in the stream or entry that range w's positions count from
//                          (0: the signal counts from the range's start)
//   begin(tail, at)     -- the set-up of a lane's (accumulate) or a wave's (fix-up) signal at X3LevAt
//   watch()             -- what x3w_stretch takes as its watch
//   add(a, v) / skip(v) -- a position of the open bin `a`, and one the lane sees that its bins do not hold (in front of or
//                          behind a range's cut of the frame): history and phase move all the same
//   flush(r, a)         -- the open bin to record r, which other lanes add to as well; drop(): the bin is no record's
//   end(frame)          -- behind the last sample of the stretch, or (frame) of the whole frame a fix-up replayed
//   kSeam               -- the one flag: the difference across a frame's front seam, which x3_range_levels_fixup_kernel books
//                          frame by frame (there is why it is a flag)
// X3LevPlain has the members of a signal without table, watch, state or end; the signals below replace what differs.
struct X3LevAt {
  uint64_t f;            // the frame
  uint32_t j;            // the stretch (a replayed frame is one stretch: 0)
  uint64_t g;            // position of the first sample the signal sees (the levels calls: in the stream or entry; the range
                         // calls: origin() plus its position behind the range's start)
  const uint32_t* tab;   // lds_table() or table()
  bool rows;             // flushes go to partial rows (accumulate), not to the caller's records (fix-up)
};
struct X3LevNoTail {};
struct X3LevPlain {
  static constexpr bool kSeam = false;
  template <class T> static __device__ __forceinline__ const uint32_t* lds_table(const T&) { return nullptr; }
  template <class T> static __device__ __forceinline__ const uint32_t* table(const T&) { return nullptr; }
  template <class T> static __device__ __forceinline__ uint64_t origin(const T&, uint64_t) { return 0; }
  template <class T> __device__ __forceinline__ void begin(const T&, const X3LevAt&) {}
  __device__ __forceinline__ X3WNoWatch watch() { return X3WNoWatch{}; }
  __device__ __forceinline__ void skip(uint32_t) {}
  __device__ __forceinline__ void flush(x3_level* __restrict__ r, const X3LevAcc& a) { x3l_merge(r, a); }
  __device__ __forceinline__ void drop() {}
  __device__ __forceinline__ void end(bool) {}
};

// X3LevSamples (the levels calls): the sample
struct X3LevSamples : X3LevPlain {
  using Tail = X3LevNoTail;
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t v) { a.add(v); }
};

// X3LevDiff (x3_signal_levels_dev): the sample minus the one in front of it, clamped to 16 bits -- `prev`
// in a register; the first sample a lane sees without a seed (sample 0 of a frame) adds nothing: that difference crosses the
// frame's seam and is x3_levels_seam_kernel's.  The watch hands over the stretch's seed, the sample in front of it, and stores
// the frame's last sample to its word of the tails, the per-frame array that is this signal's Tail; a replayed frame's is end()'s.
__device__ __forceinline__ int32_t x3l_diff(int32_t s, int32_t prev) { return min(max(s - prev, -32768), 32767); }
struct X3LevDiff;
struct X3LevDiffWatch {
  X3LevDiff& sig;
  int32_t* at;
  __device__ __forceinline__ void seed(uint32_t v) const;
  __device__ __forceinline__ void end(uint32_t v) const { *at = (int32_t)(int16_t)(uint16_t)v; }
};
struct X3LevDiff : X3LevPlain {
  static constexpr bool kSeam = true;
  using Tail = int32_t*;   // per frame: its last sample
  int32_t* last = nullptr;
  int32_t prev = 0;
  bool have = false;
  __device__ __forceinline__ void begin(Tail tail, const X3LevAt& at) { last = tail + at.f; }
  __device__ __forceinline__ X3LevDiffWatch watch() { return X3LevDiffWatch{*this, last}; }
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t v) {
    const int32_t s = (int32_t)(int16_t)(uint16_t)v;
    if (have) a.add_value(x3l_diff(s, prev));
    skip(v);
  }
  __device__ __forceinline__ void skip(uint32_t v) {   // (the next position's `prev`; a seed is the same)
    prev = (int32_t)(int16_t)(uint16_t)v;
    have = true;
  }
  __device__ __forceinline__ void end(bool frame) {
    if (frame) *last = prev;
  }
};
__device__ __forceinline__ void X3LevDiffWatch::seed(uint32_t v) const { sig.skip(v); }

// X3LevFir (x3_fir_levels_dev): y = clamp((sum over t < T of c[t] * x[i - t]) >> shift, 16 bits).  The
// taps come uniform from a kernel argument, those at and behind T zero, so that one instance serves every T; sum |c| <= 32768
// (the host's check) keeps the sum inside 2^30, and taps and samples inside the 24 bits of the multiply.  The lane holds the
// seven samples in front of the current one in registers and counts the samples it has seen: a position adds y once the lane
// has decoded T samples of its own.  It takes no seed: nothing rests on the index's sample field.  The positions a lane cannot
// form -- the first T - 1 of its stretch -- are the FIR seam kernels', from the EDGE RECORD the lane leaves: the stretch's
// first and last min(n, 7) samples and n.  The heads are stored as they pass, the rest by end().
#define X3L_FIR_TAPS 8
#define X3L_FIR_HIST (X3L_FIR_TAPS - 1)
struct X3FirTaps {
  int32_t c[X3L_FIR_TAPS];   // c[t] = 0 for t >= T
  uint32_t T, shift;
};
struct X3FirEdge {   // per (frame, stretch); a replayed frame is one stretch, at its stretch 0
  int16_t head[X3L_FIR_HIST];   // sample k of the stretch, k < min(n, 7)
  int16_t tail[X3L_FIR_HIST];   // sample n - 1 - k of the stretch, k < min(n, 7)
  uint32_t n;                   // the stretch's samples (0: the stretch in front runs through its blocks)
};
static_assert(sizeof(X3FirEdge) == 32, "an edge record is 32 bytes");
struct X3LevFirTail {   // the kernels' last argument
  X3FirTaps k;
  X3FirEdge* edges;   // F * stride records
  uint32_t stride;    // records per frame: the stretches of a frame at most
};
// THE MULTIPLY.  Taps (16 bits by the host's check) and samples are sign-extended from 24 bits in the open and multiplied
// plainly: the compiler picks the full-rate v_mul_i32_i24 by itself, in every FIR kernel of both files (the listing record in
// profiles/levels_protocol/ counts them).  The other form the family had, HIP's __mul24, is a static inline wrapper of the HIP
// headers that is not force-inlined: how the compiler treats it in one kernel depended on how many others called it (one
// multiply came out in another encoding when the range kernels were added; profiles/fir_range_levels/isa_compare.txt), so a
// kernel's instructions could change with a kernel added elsewhere.  The taps' extension is scalar and loop-invariant.
__device__ __forceinline__ int32_t x3l_mul24(int32_t c, int32_t v) {
  return ((int32_t)((uint32_t)c << 8) >> 8) * ((int32_t)((uint32_t)v << 8) >> 8);
}
__device__ __forceinline__ int32_t x3l_fir_value(const X3FirTaps& k, int32_t s, const int32_t (&d)[X3L_FIR_HIST]) {
  int32_t acc = x3l_mul24(k.c[0], s);
#pragma unroll
  for (int t = 1; t < X3L_FIR_TAPS; ++t) acc += x3l_mul24(k.c[t], d[t - 1]);
  return min(max(acc >> k.shift, -32768), 32767);
}
// The delay line, in ONE copy.  kEdge (X3LevFir: the accumulate kernels of both files and the levels fix-up): the lane leaves
// the edge record of its (frame, stretch).  Without (X3LevFirCarry: x3_range_levels_fir_fixup_kernel): no record is touched,
// the history is the caller's to keep from frame to frame, and cnt is how many of the samples in d[] are valid.
template <bool kEdge>
struct X3LevFirT : X3LevPlain {
  using Tail = X3LevFirTail;
  X3FirTaps k;   // (uniform: the kernel's argument)
  X3FirEdge* edge = nullptr;
  int32_t d[X3L_FIR_HIST] = {0, 0, 0, 0, 0, 0, 0};   // d[t]: the sample t + 1 positions in front of the current one
  uint32_t cnt = 0;                                  // samples seen (what counts is cnt >= T - 1)
  __device__ __forceinline__ void begin(const Tail& tail, const X3LevAt& at) {
    k = tail.k;
    if constexpr (kEdge) edge = tail.edges + (at.f * tail.stride + at.j);   // (f < F, j < ns <= stride: below F * stride)
  }
  __device__ __forceinline__ void push(int32_t s) {
    if constexpr (kEdge) {
      if (cnt < (uint32_t)X3L_FIR_HIST) edge->head[cnt] = (int16_t)s;
    }
    ++cnt;
#pragma unroll
    for (int t = X3L_FIR_HIST - 1; t >= 1; --t) d[t] = d[t - 1];
    d[0] = s;
  }
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t v) {
    const int32_t s = (int32_t)(int16_t)(uint16_t)v;
    if (cnt + 1u >= k.T) a.add_value(x3l_fir_value(k, s, d));   // THE HISTORY RULE: T samples of the lane's own
    push(s);
  }
  __device__ __forceinline__ void skip(uint32_t v) { push((int32_t)(int16_t)(uint16_t)v); }
  // behind the stretch's or the replayed frame's last sample: the rest of the edge record
  __device__ __forceinline__ void end(bool) const {
    static_assert(kEdge, "only a signal with an edge record has an end");
#pragma unroll
    for (int t = 0; t < X3L_FIR_HIST; ++t) edge->tail[t] = (int16_t)d[t];
    edge->n = cnt;
  }
};
using X3LevFir = X3LevFirT<true>;
using X3LevFirCarry = X3LevFirT<false>;

// out[at] = v without a dynamic register index (the FIR seam kernels and the range FIR fix-up, collecting samples from
// edge records, here and in x3_range_levels_kernel.h)
__device__ __forceinline__ void x3l_fir_set(int32_t (&out)[X3L_FIR_HIST], uint32_t at, int32_t v) {
#pragma unroll
  for (int q = 0; q < X3L_FIR_HIST; ++q) out[q] = (uint32_t)q == at ? v : out[q];
}

// X3LevTone (x3_tone_levels_dev): a position adds x * cos[k] to the record's first slot (re, where
// x3_level has sum_sq) and x * sin[k] to its second (im, where sum is), k = ph >> 22 of the 32-bit phase ph = position * step
// mod 2^32; min, max and n are the samples'.  |x * w| <= 2^30 is formed in 32 bits and added in 64: exact, in any order, and
// the atomic add of two's-complement re on the unsigned slot is exact too, so X3LevAcc, x3l_merge and x3l_merge_runs serve as
// they are.  THE PHASE is seeded by begin() with the position of the first sample the signal sees -- the product in 64 bits,
// then truncated -- and steps once per position, counted or not: no history, no seam, no edge record.  In the range calls
//  the position is in the STREAM OR ENTRY, not in the range: `starts` is the CALLER'S d_starts,
// entry-relative in the corpus form too, where the kernels otherwise see the plan's stream positions; arithmetic mod 2^64,
// then mod 2^32, on untrusted words: a wrong start changes sums, never an address (ph >> 22 < 1 024).  The table is 1 024
// words of (cos: low half, sin: high half): the workgroup's LDS copy in the accumulate kernels, the caller's array in the fix-ups.
#define X3L_TONE_TABLE 1024
struct X3LevToneTail {   // the kernels' last argument
  const uint32_t* table;   // the caller's d_table: X3L_TONE_TABLE words
  uint32_t step;
  const uint64_t* starts = nullptr;   // the range calls: the caller's d_starts, n words
};
// the accumulate kernels' copy of the table: 4 KB of LDS per workgroup, filled by all its lanes in front of the item loop
__device__ __forceinline__ const uint32_t* x3l_tone_table(const uint32_t* __restrict__ table) {
  __shared__ uint32_t s_tab[X3L_TONE_TABLE];
  for (uint32_t t = threadIdx.x; t < (uint32_t)X3L_TONE_TABLE; t += blockDim.x) s_tab[t] = table[t];
  __syncthreads();
  return s_tab;
}
struct X3LevTone : X3LevPlain {
  using Tail = X3LevToneTail;
  const uint32_t* tab = nullptr;
  uint32_t step = 0, ph = 0;
  static __device__ __forceinline__ const uint32_t* lds_table(const Tail& tail) { return x3l_tone_table(tail.table); }
  static __device__ __forceinline__ const uint32_t* table(const Tail& tail) { return tail.table; }
  static __device__ __forceinline__ uint64_t origin(const Tail& tail, uint64_t w) { return tail.starts[w]; }
  __device__ __forceinline__ void begin(const Tail& tail, const X3LevAt& at) {
    tab = at.tab;
    step = tail.step;
    ph = (uint32_t)(at.g * (uint64_t)step);
  }
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t v) {
    const int32_t s = (int32_t)(int16_t)(uint16_t)v;
    const uint32_t w = tab[ph >> 22];
    ph += step;
    a.sum_sq += (uint64_t)(int64_t)(s * (int32_t)(int16_t)(uint16_t)w);
    a.sum += (int64_t)(s * ((int32_t)w >> 16));
    a.mn = min(a.mn, s);
    a.mx = max(a.mx, s);
    ++a.n;
  }
  __device__ __forceinline__ void skip(uint32_t) { ph += step; }
};

// X3LevToneBank<NT> (x3_tone_bank_levels_dev): NT oscillators against the one table in one pass over
// the stretch.  Slot t has a phase and a pair of int64 sums of its own, formed as X3LevTone forms its one pair and seeded with
// the same position; min, max and n are the samples' and live once, in the binner's X3LevAcc, whose two sums stay 0.  NT is a
// compile-time count and every loop over it is unrolled, so every slot index is a constant: registers, no scratch.  The steps
// are the tail's (uniform); a call with fewer than NT tones has step 0 in its spare slots, which flush() never writes.
// THE PLANE STORE: flush() adds slot t < n_tones of the open bin to the same record of PLANE t -- `r` is plane 0's record, the
// planes lie `stride` records apart (partial rows or the caller's records: X3LevAt::rows) -- through x3l_merge, and the sums
// start anew either way: one plane is X3LevTone's record byte for byte, and the bounds of one plane hold in each.
#define X3L_TONE_BANK 8
struct X3LevToneBankTail {   // the kernels' last argument
  const uint32_t* table;   // the caller's d_table: X3L_TONE_TABLE words
  uint32_t n_tones;        // 2 .. X3L_TONE_BANK planes are stored
  uint32_t steps[X3L_TONE_BANK];
  uint64_t rows_stride;    // plane stride of the partial rows (the accumulate kernels)
  uint64_t levels_stride;  // plane stride of the caller's records (the fix-up kernels)
  const uint64_t* starts = nullptr;   // the range calls: the caller's d_starts, n words
};
template <uint32_t NT>
struct X3LevToneBank : X3LevPlain {
  static_assert(NT >= 2 && NT <= X3L_TONE_BANK, "2 .. X3L_TONE_BANK slots");
  using Tail = X3LevToneBankTail;
  const uint32_t* tab = nullptr;
  uint64_t stride = 0;
  uint32_t n_tones = 0;
  uint32_t step[NT], ph[NT];
  uint64_t re[NT];
  int64_t im[NT];
  static __device__ __forceinline__ const uint32_t* lds_table(const Tail& tail) { return x3l_tone_table(tail.table); }
  static __device__ __forceinline__ const uint32_t* table(const Tail& tail) { return tail.table; }
  static __device__ __forceinline__ uint64_t origin(const Tail& tail, uint64_t w) { return tail.starts[w]; }
  __device__ __forceinline__ void begin(const Tail& tail, const X3LevAt& at) {
    tab = at.tab;
    stride = at.rows ? tail.rows_stride : tail.levels_stride;
    n_tones = tail.n_tones;
#pragma unroll
    for (uint32_t t = 0; t < NT; ++t) {
      step[t] = tail.steps[t];
      ph[t] = (uint32_t)(at.g * (uint64_t)step[t]);
    }
    drop();
  }
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t v) {
    const int32_t s = (int32_t)(int16_t)(uint16_t)v;
#pragma unroll
    for (uint32_t t = 0; t < NT; ++t) {
      const uint32_t w = tab[ph[t] >> 22];
      ph[t] += step[t];
      re[t] += (uint64_t)(int64_t)(s * (int32_t)(int16_t)(uint16_t)w);
      im[t] += (int64_t)(s * ((int32_t)w >> 16));
    }
    a.mn = min(a.mn, s);
    a.mx = max(a.mx, s);
    ++a.n;
  }
  __device__ __forceinline__ void skip(uint32_t) {
#pragma unroll
    for (uint32_t t = 0; t < NT; ++t) ph[t] += step[t];
  }
  // (a: the open bin's min, max, n; t * stride < n_tones * stride: inside the planes)
  __device__ __forceinline__ void flush(x3_level* __restrict__ r, const X3LevAcc& a) {
#pragma unroll
    for (uint32_t t = 0; t < NT; ++t) {
      if (t < n_tones) {
        X3LevAcc b = a;
        b.sum_sq = re[t];
        b.sum = im[t];
        x3l_merge(r + t * stride, b);
      }
    }
    drop();
  }
  __device__ __forceinline__ void drop() {
#pragma unroll
    for (uint32_t t = 0; t < NT; ++t) {
      re[t] = 0;
      im[t] = 0;
    }
  }
};

// The bins of consecutive positions from g on: decode(put_at) hands sample s of a frame to put_at(s, value), in order;
// the positions with keep(s) go to the signal's add(), the others to its skip() and count in no bin; bins that fill go to
// flush(bin, acc), and so does the open one at the end.  Returns decode's.
template <class Signal, class Decode, class Keep, class Flush>
__device__ __forceinline__ int32_t x3l_bin_samples(uint64_t g, uint64_t bl, Decode decode, Keep keep, Flush flush, Signal& sig) {
  X3LevBinner bn;
  bn.open(g, bl);
  const int32_t r = decode([&](uint32_t s, uint32_t v) {
    if (keep(s)) bn.put(sig, v, flush);
    else sig.skip(v);
  });
  flush(bn.bin, bn.a);
  return r;
}
// (the levels calls: every sample of the frame)
struct X3LevKeepAll {
  __device__ __forceinline__ bool operator()(uint32_t) const { return true; }
};

// ---- identities; the summary
__global__ void __launch_bounds__(256)
x3_levels_init_kernel(x3_level* __restrict__ levels, uint64_t n_rows, x3_level* __restrict__ rows, uint64_t cap,
                      X3LevSummary* __restrict__ sum) {
  const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
  if (i0 == 0) {
    sum->n_bad = 0;
    sum->first = ~0ull;
    sum->replays = 0;
  }
  const x3_level id = X3L_IDENTITY;
  for (uint64_t i = i0; i < n_rows + cap; i += stride) {
    if (i < n_rows) levels[i] = id;
    else rows[i - n_rows] = id;
  }
}

// ---- check: a wave per frame
__global__ void __launch_bounds__(256)
x3_levels_check_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off,
                       const uint64_t* __restrict__ so, uint64_t F, int32_t* __restrict__ fst) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t f = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); f < F; f += waves) {
    const int32_t st = x3w_check_frame(x3, len, frame_off[f], so, f, lane);
    if (lane == 0) fst[f] = st;
  }
}

// the rows of a checked frame (so[f + 1] - so[f] = its samples >= 1): bins b0 .. b1 below nlim
__device__ __forceinline__ void x3l_frame_rows(X3LevFrame& fr, uint64_t samples, uint64_t bl, bool ok, uint32_t* cnt) {
  if (fr.pos > ~0ull - 0x10000u) fr.nlim = 0;   // (no checked frame's positions wrap: its samples end at so[f + 1])
  fr.b0 = fr.pos / bl;
  uint32_t c = 0;
  if (ok && samples && fr.b0 < fr.nlim) {
    const uint64_t b1 = min((fr.pos + (samples - 1u)) / bl, fr.nlim - 1u);
    c = (uint32_t)(b1 - fr.b0 + 1u);   // (at most `samples`, which the check holds to 16 bits)
  }
  *cnt = c;
}

// ---- prep, stream: positions are the sample offsets, one stream of n_bins bins
__global__ void __launch_bounds__(256)
x3_levels_prep_kernel(const uint64_t* __restrict__ so, uint64_t F, uint64_t bin_len, uint64_t n_bins,
                      const int32_t* __restrict__ fst, X3LevFrame* __restrict__ frames, uint32_t* __restrict__ cnt) {
  const uint64_t bl = x3l_bin_len(bin_len);
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (uint64_t)gridDim.x * blockDim.x) {
    X3LevFrame fr{so[f], 0, n_bins, 0};
    const bool ok = fst[f] == X3D_OK;
    x3l_frame_rows(fr, ok ? so[f + 1u] - so[f] : 0u, bl, ok, &cnt[f]);
    frames[f] = fr;
  }
}

// ---- corpus: rows per entry, max(1, ceil(n_samples / bin_len)), and their exclusive scan (n + 1 words); one workgroup
__device__ __forceinline__ unsigned long long x3l_entry_rows(uint64_t n_samples, uint64_t bin_len) {
  if (bin_len == 0 || n_samples == 0) return 1ull;
  return n_samples / bin_len + (n_samples % bin_len ? 1u : 0u);
}

__global__ void __launch_bounds__(1024)
x3_corpus_levels_rows_kernel(const x3_corpus_entry* __restrict__ ent, uint64_t n, uint64_t bin_len,
                             unsigned long long* __restrict__ row_first) {
  __shared__ unsigned long long s[1024];
  const unsigned long long total = x3w_scan_items(
      n, s, [&](uint64_t e) { return x3l_entry_rows(ent[e].n_samples, bin_len); },
      [&](uint64_t e, unsigned long long run) { row_first[e] = run; });
  if (threadIdx.x == 0) row_first[n] = total;
}

// ---- prep, corpus: the frame's entry by a search of the entry table (checked, not trusted: its frames inside the table,
// its positions as the sample offsets give them, its rows inside d_levels); positions are relative to the entry
__global__ void __launch_bounds__(256)
x3_corpus_levels_prep_kernel(const x3_corpus_entry* __restrict__ ent, uint64_t n_ent, const unsigned long long* __restrict__ row_first,
                             const uint64_t* __restrict__ so, uint64_t F, uint64_t bin_len, uint64_t n_rows,
                             const int32_t* __restrict__ fst, X3LevFrame* __restrict__ frames, uint32_t* __restrict__ cnt) {
  const uint64_t bl = x3l_bin_len(bin_len);
  for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t lo = 0, hi = n_ent;   // the last entry whose first frame is at or in front of f
    while (hi - lo > 1u) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (ent[mid].first_frame <= f) lo = mid;
      else hi = mid;
    }
    const x3_corpus_entry en = ent[lo];
    X3LevFrame fr{0, 0, 0, 0};
    const unsigned long long r0 = row_first[lo];
    if (en.first_frame <= f && f - en.first_frame < en.n_frames && en.n_frames <= F - en.first_frame &&
        so[f] >= so[en.first_frame] && r0 <= n_rows) {
      fr.pos = so[f] - so[en.first_frame];
      fr.obase = r0;
      fr.nlim = min((uint64_t)x3l_entry_rows(en.n_samples, bin_len), n_rows - r0);
    }
    const bool ok = fst[f] == X3D_OK;
    x3l_frame_rows(fr, ok ? so[f + 1u] - so[f] : 0u, bl, ok, &cnt[f]);
    frames[f] = fr;
  }
}

// ---- exclusive scan of the row counts (F + 1 words); a frame whose rows end behind `cap` is flagged for the fix-up
__global__ void __launch_bounds__(1024)
x3_levels_scan_kernel(const uint32_t* __restrict__ cnt, uint64_t F, uint64_t cap, unsigned long long* __restrict__ row,
                      int32_t* __restrict__ fst) {
  __shared__ unsigned long long s[1024];
  const unsigned long long total = x3w_scan_items(
      F, s, [&](uint64_t f) { return (unsigned long long)cnt[f]; },
      [&](uint64_t f, unsigned long long run) {
        row[f] = run;
        if (cnt[f] && run + cnt[f] > cap) fst[f] = X3W_FLAG;
      });
  if (threadIdx.x == 0) row[F] = total;
}

// ---- accumulate: a lane per (frame, stretch) into the frame's own rows -- a bank's planes of them -- by the signal protocol
template <class Signal>
__global__ void __launch_bounds__(256)
x3_levels_accum_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off, uint64_t F,
                       X3DevParams p, const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg, uint64_t bin_len,
                       const X3LevFrame* __restrict__ frames, const unsigned long long* __restrict__ row,
                       x3_level* __restrict__ rows, int32_t* __restrict__ fst, typename Signal::Tail tail) {
  const bool segd = x3w_index_ok(idx, sb);
  const uint32_t ns = segd ? nseg : 1u;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t n_items = F * ns;
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t* const tab = Signal::lds_table(tail);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += lanes) {
    const uint64_t f = i / ns;
    const uint32_t j = (uint32_t)(i - f * ns);
    if (fst[f] != X3D_OK) continue;   // (failed its check, or its rows do not fit: nothing to prove here)
    const X3LevFrame fr = frames[f];
    x3_level* const mine = rows + row[f];
    const uint64_t nlim = fr.nlim, b0 = fr.b0;
    // a stretch's samples come in order, from sample 0 or from the first sample of block sb * j
    const uint64_t g = fr.pos + (j ? 1u + (uint64_t)sb * j * p.block_len : 0u);
    Signal sig;
    sig.begin(tail, X3LevAt{f, j, g, tab, true});
    auto flush = [&](uint64_t bin, const X3LevAcc& a) {
      if (bin < nlim) sig.flush(mine + (bin - b0), a);
      else sig.drop();
    };
    const int r = x3l_bin_samples(
        g, bl, [&](auto put_at) { return x3w_stretch(x3, len, frame_off[f], p, idx, segd, sb, nseg, f, j, put_at, sig.watch()); },
        X3LevKeepAll{}, flush, sig);
    sig.end(false);
    if (r < 0) atomicOr(&fst[f], X3W_FLAG);
  }
}

// ---- fix-up: a wave per frame (lane 0 works); scratch: a block's samples per wave of the grid.  A frame it replays to
// status 0 is ONE stretch, at its stretch 0 (X3L_DONE says so), straight into the caller's records
template <class Signal>
__global__ void __launch_bounds__(256)
x3_levels_fixup_kernel(const uint8_t* __restrict__ x3, const uint64_t* __restrict__ frame_off, uint64_t F, X3DevParams p,
                       uint64_t bin_len, const X3LevFrame* __restrict__ frames, int32_t* __restrict__ fst,
                       x3_level* __restrict__ levels, int32_t* __restrict__ status, int16_t* __restrict__ scratch,
                       uint32_t scratch_per, X3LevSummary* __restrict__ sum, typename Signal::Tail tail) {
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (threadIdx.x & 63u) return;
  int16_t* const blk = scratch + wave * (uint64_t)scratch_per;
  const uint64_t bl = x3l_bin_len(bin_len);
  for (uint64_t f = wave; f < F; f += waves) {
    int32_t fs = fst[f];
    if (fs == X3W_FLAG) {
      const uint8_t* const payload = x3 + frame_off[f] + 20u;
      fs = x3w_replay_frame(payload, p, blk, [](uint32_t, uint32_t) {});
      if (fs == X3D_OK) {   // every block decodes: once more, now into the caller's bins
        const X3LevFrame fr = frames[f];
        Signal sig;
        sig.begin(tail, X3LevAt{f, 0u, fr.pos, Signal::table(tail), false});
        auto flush = [&](uint64_t bin, const X3LevAcc& a) {
          if (bin < fr.nlim) sig.flush(levels + fr.obase + bin, a);
          else sig.drop();
        };
        (void)x3l_bin_samples(fr.pos, bl, [&](auto put_at) { return x3w_replay_frame(payload, p, blk, put_at); }, X3LevKeepAll{},
                              flush, sig);
        sig.end(true);
      }
      fst[f] = fs | X3L_DONE;
      atomicAdd(&sum->replays, 1ull);
    }
    if (status) status[f] = fs;
    if (fs != X3D_OK) {
      atomicAdd(&sum->n_bad, 1ull);
      atomicMin(&sum->first, (unsigned long long)(f << 8) | (uint32_t)fs);
    }
  }
}

// ---- merge: a lane per partial row.  A row counts when its frame's word is X3D_OK: checked, every stretch proven.  Rows
// of the same record that lie side by side in a wave (the boundary bin of neighbouring frames; with one bin, all of them)
// are joined in registers, and the first lane of each run adds the sum.
__global__ void __launch_bounds__(256)
x3_levels_merge_kernel(const X3LevFrame* __restrict__ frames, const unsigned long long* __restrict__ row, uint64_t F,
                       uint64_t cap, const x3_level* __restrict__ rows, const int32_t* __restrict__ fst,
                       x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t n = min((uint64_t)row[F], cap);
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += lanes) {   // (whole waves)
    const uint64_t i = i0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    if (i < n) {
      const uint64_t f = x3w_owner(row, F, i);
      if (fst[f] == X3D_OK) {
        const X3LevFrame fr = frames[f];
        const x3_level r = rows[i];
        key = fr.obase + fr.b0 + (i - row[f]);   // (below obase + nlim <= the caller's rows: x3l_frame_rows)
        a.load(r);
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}

// ---- seam (X3LevDiff only): a lane per frame f >= 1, behind the fix-up, when every frame's word is final -- X3D_OK, or
// X3L_DONE | status.  The difference at the position of frame f's sample 0 is the frame's first sample (the 16-bit literal
// at the start of its payload) minus frame f - 1's last (tail[f - 1]); it counts when both frames have status 0 and belong
// to the same stream or entry: the same records (obase) with nlim != 0 -- positions of two good neighbours are then back to
// back, since a checked frame's samples are so[f + 1] - so[f].  Lanes are joined by record as in x3_levels_merge_kernel: with
// one bin every seam of a stream is the same record's.
__device__ __forceinline__ bool x3l_frame_good(int32_t w) { return w == X3D_OK || w == X3L_DONE; }

__global__ void __launch_bounds__(256)
x3_levels_seam_kernel(const uint8_t* __restrict__ x3, uint64_t len, const uint64_t* __restrict__ frame_off, uint64_t F,
                      uint64_t bin_len, const X3LevFrame* __restrict__ frames, const int32_t* __restrict__ fst,
                      const int32_t* __restrict__ tail, x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t f0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); f0 < F; f0 += lanes) {   // (whole waves)
    const uint64_t f = f0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    if (f >= 1u && f < F && x3l_frame_good(fst[f]) && x3l_frame_good(fst[f - 1u])) {
      const X3LevFrame fr = frames[f];
      const X3LevFrame fp = frames[f - 1u];
      const uint64_t bin = fr.pos / bl;
      if (fr.nlim && fp.nlim && fr.obase == fp.obase && bin < fr.nlim) {
        // (a checked frame: its header and payload lie inside the stream)
        const int32_t head = (int32_t)(int16_t)(uint16_t)(x3w_be32_at(x3, len, frame_off[f] + 20u) >> 16);
        a.add_value(x3l_diff(head, tail[f - 1u]));
        key = fr.obase + bin;   // (below obase + nlim <= the caller's rows: x3l_frame_rows)
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}

// ---- seam (X3LevFir only): a lane per (frame, stretch), behind the fix-up, when every frame's word is final.  The first
// T - 1 positions of a stretch are the ones its lane could not form.  A frame whose word is X3D_OK has the records of its
// stretches, every one written by a lane that ran to its proof; a frame whose word is X3L_DONE has ONE record, the fix-up's,
// at its stretch 0.  The lane collects up to T - 1 samples of history by walking back over the records' tails -- earlier
// stretches of the frame, then the frame in front while that one is good and belongs to the same stream or entry (the same
// records, obase, with nlim != 0: as in x3_levels_seam_kernel, good neighbours are back to back in position) -- and stops at
// a failed frame or the entry's first sample.  Every good frame has a sample, so a frame's step finds one: the walk ends after
// at most (T - 1) * ns records.  Then y at the first min(n, T - 1) positions from history plus heads; a position whose history
// is not complete adds nothing.  A bin edge can fall between those positions: a bin that fills goes to its record at once,
// the open one is joined by record across the wave as in x3_levels_merge_kernel.  The stream is not read.
// Every edge record read lies below F * stride (j < ns <= stride), every caller's record at obase + bin with bin < nlim.
struct X3FirSeamValue {
  int32_t y;
  bool counts;
  __device__ __forceinline__ void add(X3LevAcc& a, uint32_t) const {
    if (counts) a.add_value(y);
  }
};

__global__ void __launch_bounds__(256)
x3_levels_fir_seam_kernel(uint64_t F, uint32_t block_len, const uint2* __restrict__ idx, uint32_t sb, uint32_t nseg, uint64_t bin_len,
                          const X3LevFrame* __restrict__ frames, const int32_t* __restrict__ fst,
                          const X3FirEdge* __restrict__ edges, uint32_t stride, X3FirTaps k, x3_level* __restrict__ levels) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t ns = x3w_index_ok(idx, sb) ? nseg : 1u;
  const uint32_t need = k.T - 1u;   // samples of history a position takes
  const uint64_t bl = x3l_bin_len(bin_len);
  const uint64_t n_items = F * ns;
  const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_items; i0 += lanes) {   // (whole waves)
    const uint64_t i = i0 + lane;
    X3LevAcc a;
    a.reset();
    uint64_t key = ~0ull;
    const uint64_t f = i / ns;
    const uint32_t j = (uint32_t)(i - f * ns);
    const int32_t w = i < n_items ? fst[f] : -1;
    if (w == X3D_OK || (w == X3L_DONE && j == 0u)) {
      const X3LevFrame fr = frames[f];
      const X3FirEdge e = edges[f * stride + j];
      if (fr.nlim && e.n) {
        // history: hist[h] = the sample h + 1 positions in front of the stretch, h < H
        int32_t hist[X3L_FIR_HIST] = {0, 0, 0, 0, 0, 0, 0};
        uint32_t H = 0;
        uint64_t wf = f;
        uint32_t wj = j;
        while (H < need) {
          if (wj) {
            --wj;
          } else {
            if (wf == 0u) break;
            const int32_t pw = fst[wf - 1u];
            if (!x3l_frame_good(pw)) break;
            const X3LevFrame fp = frames[wf - 1u];
            if (!fp.nlim || fp.obase != fr.obase) break;
            --wf;
            wj = pw == X3D_OK ? ns - 1u : 0u;
          }
          const X3FirEdge h = edges[wf * stride + wj];
          const uint32_t m = min(h.n, (uint32_t)X3L_FIR_HIST);
#pragma unroll
          for (int t = 0; t < X3L_FIR_HIST; ++t) {
            if ((uint32_t)t < m && H < need) {
              x3l_fir_set(hist, H, (int32_t)h.tail[t]);
              ++H;
            }
          }
        }
        // y at sample c of the stretch, c < min(n, T - 1), from x[c - t]: a head (c >= t) or history (hist[t - c - 1])
        const uint32_t m = min(e.n, need);
        auto flush = [&](uint64_t bin, const X3LevAcc& acc) {
          if (bin < fr.nlim) x3l_merge(levels + fr.obase + bin, acc);
        };
        X3LevBinner bn;
        bn.open(fr.pos + (j ? 1u + (uint64_t)sb * j * block_len : 0u), bl);
#pragma unroll
        for (int c = 0; c < X3L_FIR_HIST; ++c) {
          if ((uint32_t)c < m) {
            int32_t d[X3L_FIR_HIST];
#pragma unroll
            for (int t = 1; t < X3L_FIR_TAPS; ++t) d[t - 1] = c >= t ? (int32_t)e.head[c - t] : hist[t - c - 1];
            bn.put(X3FirSeamValue{x3l_fir_value(k, (int32_t)e.head[c], d), (uint32_t)c + H >= need}, 0u, flush);
          }
        }
        if (bn.bin < fr.nlim) {
          a = bn.a;
          key = fr.obase + bn.bin;   // (below obase + nlim <= the caller's rows: x3l_frame_rows)
        }
      }
    }
    x3l_merge_runs(levels, key, a, lane);
  }
}

// ---- the adapter (x3_tone_power_levels_dev): a lane per record, x3_tone_level (re, im in x3_level's
// first two slots) -> the x3_level of the band's level, in place or into rows that do not overlap.  Integers only:
//   e = max(0, bitlen(n) - 15); a = re >> (15 + e), b = im >> (15 + e) (arithmetic); P = a * a + b * b, below 2^62 for a
//   record the tone call wrote (|re|, |im| <= n * 2^30); m = n >> e (1 .. 2^15 - 1, or n itself);
//   ms = min(2^30, (2 * P / m) / m); peak = min(32767, isqrt(2 * ms)); -> {ms * n, 0, -peak, peak, n, 0}; n == 0: X3L_IDENTITY.
// Records that no tone call wrote cannot fault anything: the products wrap in 64 unsigned bits and ms is clamped.
__device__ __forceinline__ uint32_t x3l_isqrt(uint64_t x) {   // floor square root, x < 2^32
  uint32_t r = 0;
#pragma unroll
  for (int b = 15; b >= 0; --b) {
    const uint32_t t = r | (1u << b);
    if ((uint64_t)t * t <= x) r = t;
  }
  return r;
}

__global__ void __launch_bounds__(256)
x3_tone_power_kernel(const x3_level* tone, uint64_t n_rows, x3_level* levels) {   // (in place: no __restrict__)
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * blockDim.x) {
    const x3_level r = tone[i];
    x3_level o = X3L_IDENTITY;
    if (r.n) {
      const uint32_t bits = 32u - (uint32_t)__clz((int)r.n);
      const uint32_t e = bits > 15u ? bits - 15u : 0u;
      const uint64_t a = (uint64_t)((int64_t)r.sum_sq >> (15u + e)), b = (uint64_t)(r.sum >> (15u + e));
      const uint64_t P = a * a + b * b;
      const uint64_t m = r.n >> e;
      const uint64_t ms = min((2u * P / m) / m, (uint64_t)1 << 30);
      const int32_t peak = (int32_t)min(x3l_isqrt(2u * ms), 32767u);
      o = x3_level{ms * r.n, 0, -peak, peak, r.n, 0};
    }
    levels[i] = o;
  }
}
