// x3_decode.hip -- decoder, frame-check and index kernels and the x3_decode* / x3_index_dev entry points, the stream walks,
// the BitReader / BitPacker handles (C ABI: include/x3hip.h; units: x3_internal.h).
#include <chrono>
#include "x3_internal.h"
#include "x3_decode_kernel.h"
#include "x3_decode_split_kernel.h"
#include "x3_decode_blocks_kernel.h"
#include "x3_index_kernels.h"
#include "x3_decode_mc_kernel.h"
#include "x3_decode_window_kernel.h"
#include "x3_seg_index_kernel.h"
#include "x3_levels_kernel.h"
#include "x3_events_kernel.h"
#include "x3_quantiles_kernel.h"
#include "x3_range_levels_kernel.h"
#include "x3_spectra_kernel.h"
#include "x3_spectra_levels_kernel.h"

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
// The kernels' view of the caller's parameters.  (Samples per frame beyond 32 bits: 0 -- the entry points that need a
// frame length refuse that, the others never use it.)
static int derive_params(const x3_params* p, X3DevParams* d) {
  const uint64_t spf = spf_of(p);
  return derive(p, spf > 0xFFFFFFFFull ? 0 : spf, d);
}

// The SEGMENT INDEX (include/x3hip.h): the stretches of `seg_blocks` blocks that the index tells apart in a frame.  Its
// pitch follows the PARAMETERS -- the blocks of a full frame -- not the call: x3_seg_index_entries, the encoder and every
// launch that reads or writes an index go by this whatever the clips' lengths are.
static uint64_t seg_stretches(uint64_t blocks_per_frame, uint32_t seg_blocks) {
  return (blocks_per_frame + seg_blocks - 1) / seg_blocks;
}
// ... as a launch takes them: 1 where the index has no entries (x3_seg_index_entries() == 0: frames of one stretch, or
// seg_blocks 0, no index) -- whole frames
static uint32_t seg_index_nseg(uint64_t blocks_per_frame, uint32_t seg_blocks) {
  const uint64_t nidx = seg_blocks ? seg_stretches(blocks_per_frame, seg_blocks) : 1;
  return nidx >= 2 ? (uint32_t)nidx : 1u;
}

// The parameters as the decoders take them: block length 0 travels as 1 (frames that need it are BAD_ARG frames of the walk)
static x3_params decoder_params(const x3_params* p) {
  x3_params pp = *p;
  if (pp.block_len == 0) pp.block_len = 1;
  return pp;
}

// ... for the entry points that address blocks inside a frame (windows, the segment index): both lengths are needed
static int derive_block_params(const x3_params* p, X3DevParams* d) {
  const int rc = derive_params(p, d);
  return rc ? rc : d->block_len == 0 || d->blocks_per_frame == 0 ? X3_ERR_BAD_ARG : X3_OK;
}

// what the entry points take for a frame table: the stream on a 4-byte boundary, offsets on an 8-byte one, a count in 31 bits
static bool frame_table_args_ok(const uint8_t* d_x3, const uint64_t* d_frame_offsets, uint64_t n_frames) {
  return (reinterpret_cast<uintptr_t>(d_x3) & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_frame_offsets) & 7u) == 0 &&
         n_frames != 0 && n_frames <= 0x7FFFFFFFull;
}

// ... and for a segment index: stretches of whole groups of four blocks, an 8-byte aligned table
static bool seg_index_args_ok(const uint64_t* d_seg_index, uint32_t seg_blocks) {
  return seg_blocks != 0 && (seg_blocks & 3u) == 0 && seg_blocks <= 3200u && (reinterpret_cast<uintptr_t>(d_seg_index) & 7u) == 0;
}

// The decoder of a call (the inputs: x3_internal.h).
DecodeRoute decode_route(const X3DevParams& dp, const X3Geom& g, const int16_t* d_wav, bool offsets, bool x4, int seg_mode,
                         const X3Opts& o) {
  // the branch-free kernels need every valid Rice codeword (zeros + terminator + sub-code) to fit 32 bits
  bool fast = true;
  const uint32_t widths[3] = {1, 2, 4};
  for (int k = 0; k < 3; ++k) {
    const uint32_t level = k == 0 ? 1u : (1u << dp.k[k]);
    fast = fast && (dp.inv_len[k] / level + 1 + widths[k] <= 32);
  }
  if (!fast) return {X3_DEC_SINGLE, 0, 0, false};
  // The three-wave kernel's parser hands over i = (z << k) + r with r the k bits behind the terminating one, which equals
  // the reference's r' + level * (n - 1) (decoder.rs:186, r' = the hard-wired 2 / 4 bits INCLUDING the one) only when the
  // code of ftype 2 has one sub-bit and that of ftype 3 three -- the default codes; the block-per-lane kernel likewise.  The
  // single-wave kernels follow the reference's formula literally and take every other code set.  Both multi-wave kernels
  // need rows on 8-byte boundaries (x3_decode_split_kernel.h flush_rows): a frame's samples begin where the layout says --
  // multiples of spf samples or of the clip stride, or the caller's offsets, which only the caller can vouch for (x4).
  const bool rows8 = (reinterpret_cast<uintptr_t>(d_wav) & 7u) == 0 &&
                     (offsets ? x4 : (dp.spf % 4u) == 0 && (g.fpc >= g.n_frames || (g.clip_stride % 4u) == 0));
  if (dp.k[1] != 1u || dp.k[2] != 3u || !rows8 || o.decode_single) return {X3_DEC_SINGLE_FAST, 0, 0, false};
  // Block length 20: the three-wave kernel, which also decodes by the segment index and records it.  Option "decode_blocks"
  // moves the calls without an index to the block-per-lane kernel (x3_decode_blocks_kernel.h): bit-exact, but it walks
  // every frame twice and is slower on config 3 (profiles/r6/decoder_blocks_kernel.txt).  Block lengths 10 and 40: the
  // block-per-lane kernel is the default -- the three-wave kernel is written for blocks of 20, and the single-wave kernels
  // are one serial chain per frame with nothing beside it (1.8 / 1.1 ms at config 3's size).
  if (dp.block_len == X3S_BL)
    return o.decode_blocks && !seg_mode ? DecodeRoute{X3_DEC_BLOCKS, 20u, 1u, true} : DecodeRoute{X3_DEC_SPLIT, 0, 0, true};
  if (dp.block_len == 40u && !o.decode_blocks_off) return {X3_DEC_BLOCKS, 20u, 2u, false};
  if (dp.block_len == 10u && !o.decode_blocks_off) return {X3_DEC_BLOCKS, 10u, 1u, false};
  return {X3_DEC_SINGLE_FAST, 0, 0, false};
}

// wav_off_aligned: the caller knows that every d_wav_offsets[f] is a multiple of FOUR samples (the three-wave decoder
// moves rows in 8- or 16-byte pieces); without that knowledge caller-supplied offsets go to the single-wave kernels
int decode_dev_impl(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                           uint64_t F, const x3_batch* batch, const uint64_t* d_wav_offsets, const x3_params* p,
                           int16_t* d_wav, uint64_t wav_cap, int32_t* d_status, bool wav_off_aligned,
                           bool bl0,    // bl0: the caller's block_len is 0 and p carries 1 (x3_decode_merge_kernel)
                           const X3SegSpec* seg, const unsigned long long* d_nf) {
  if (reinterpret_cast<uintptr_t>(d_x3) & 3u) return X3_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(d_wav) & 1u) return X3_ERR_BAD_ARG;
  if (F == 0 || F > 0x7FFFFFFFull) return X3_ERR_BAD_ARG;
  const uint64_t spf = spf_of(p);
  X3DevParams dp;
  int rc = derive_params(p, &dp);
  if (rc) return rc;
  X3Geom g{0, 0, 1, F};
  if (!d_wav_offsets) {
    if (!batch || spf == 0) return X3_ERR_BAD_ARG;
    const uint64_t fpc = (batch->n_per_clip + spf - 1) / spf;
    if (fpc == 0 || fpc > 0xFFFFFFFFull) return X3_ERR_BAD_ARG;
    g.n_per_clip = batch->n_per_clip;
    g.clip_stride = batch->clip_stride;
    g.fpc = (uint32_t)fpc;
  }
  const bool by_seg = seg && seg->mode && seg->d_index && seg->seg_blocks;
  const DecodeRoute rt = decode_route(dp, g, d_wav, d_wav_offsets != nullptr, wav_off_aligned, by_seg ? seg->mode : 0, c->opt);
  if (d_nf && !rt.device_count) return X3_ERR_BAD_ARG;
  c->last_seg_stretches = 0;
  if ((rc = ensure(c, c->dec_meta, F * sizeof(X3FrameMeta)))) return rc;
  if (!d_status) {
    if ((rc = ensure(c, c->dec_status, F * sizeof(int32_t)))) return rc;
    d_status = (int32_t*)c->dec_status.p;
  }
  if ((rc = ensure(c, c->dec_cstatus, F * sizeof(int32_t)))) return rc;
  // fork: header + payload-CRC pass on the side stream, decoder on the main stream (independent;
  // the decoder's one-wave-per-SIMD dependency chains leave the CUs mostly idle)
#ifdef X3_PROFILING
  hipStream_t check_stream = c->opt.check_serial ? c->stream : c->stream2;
  const bool no_check = c->opt.no_check != 0;
#else
  // (option check_main: the two passes swap streams -- the one on the side stream starts a cross-queue event later)
  hipStream_t check_stream = c->opt.check_main ? c->stream : c->stream2;
  const bool no_check = false;
#endif
  hipStream_t dec_stream = check_stream == c->stream2 ? c->stream : c->stream2;
  const uint64_t check_wgs_per_cu = (uint64_t)c->opt.check_wgs;
  HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  // The check pass and the decoder are independent and run side by side; the decoder is enqueued first.  (Neither the
  // order nor the side stream's queue priority selects between the decoder's timing modes -- 0.81 / 0.87 / 0.94 ms
  // per process on one box, 0.98 on another with no check kernel at all: measured, tools/dbg_modes.sh, DESIGN.md.)
  auto launch_check = [&]() -> int {
    if (no_check) {
      // profiling builds only: time the decoder without the check pass beside it (payload CRCs are NOT verified)
      HIPCHK(c, hipMemsetAsync(c->dec_cstatus.p, 0, F * sizeof(int32_t), c->stream2));

    } else {
      TimerScope ts(c, 4, check_stream, true);
      const uint64_t check_grid = std::min<uint64_t>((F + 3) / 4, (uint64_t)c->n_cus * check_wgs_per_cu);
      X3_LAUNCH_TIMED(ts, x3_frame_check_kernel, dim3((unsigned)check_grid), dim3(256), 0, check_stream,
                         reinterpret_cast<const uint32_t*>(d_x3), x3_len, d_frame_offsets, F,
                         (const uint16_t*)c->d_xinv8, (const uint16_t*)c->d_chktab, (const uint32_t*)c->d_kx64,
                         (int32_t*)c->dec_cstatus.p, reinterpret_cast<unsigned long long*>(c->d_summary), 1u, d_nf);
    }
    if (check_stream == c->stream2) HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    return X3_OK;
  };
  if (c->opt.check_first && (rc = launch_check())) return rc;
  {
    // (X3HIP_DECODE_DYN_LDS: extra LDS per decoder group = fewer groups per CU; an occupancy experiment)
    const size_t dyn_lds = (size_t)c->opt.dyn_lds;
    const bool paced = rt.kernel == X3_DEC_SPLIT || rt.kernel == X3_DEC_BLOCKS;   // (the kernels with a pace word)
    c->last_decode_kernel = rt.kernel;
    TimerScope ts(c, 1, dec_stream, paced);   // (events on the dispatch packet of the kernels launched with X3_LAUNCH_TIMED; the rarer single-wave kernels below: bracketed)
    // the pace word's 12-bit epoch: launches 1, 2, ... 4095, then the word starts over
    if (paced && (c->dec_epoch & 0xFFFu) == 0u) {
      HIPCHK(c, hipMemsetAsync(c->d_pace, 0, 16, dec_stream));  // (achieved and aimed-at, one word per launch parity)
      HIPCHK(c, hipMemsetAsync(c->d_pace + 8, 0, 8, dec_stream));   // (the launch shapes)
      HIPCHK(c, hipMemsetAsync(c->d_pace + X3_LOG_BASE, 0, X3_LOG_ENTRIES * X3_LOG_WORDS * sizeof(uint32_t), dec_stream));  // (its atomicMax entries carry the epoch too)
      ++c->dec_epoch;
    }
    if (rt.kernel == X3_DEC_BLOCKS) {
      // as many groups as give every CU the same number (five are resident per CU: the walkers of ALL groups must run
      // side by side, a frame's walk is the kernel's critical path): config 3 is 1 280 groups of 54 frames
      const uint64_t slots = (uint64_t)c->n_cus * 5;
      uint64_t fpg = 1;
      if (F >= slots) {
        const uint64_t rounds = (F + 64 * slots - 1) / (64 * slots);
        fpg = (F + rounds * slots - 1) / (rounds * slots);
      }
      const uint64_t groups = (F + fpg - 1) / fpg;
#define X3B_LAUNCH(UNIT, UPB)                                                                                             \
      X3_LAUNCH_TIMED(ts, (x3_decode_blocks_kernel<UNIT, UPB>), dim3((unsigned)groups), dim3(64 * X3B_WAVES), dyn_lds, dec_stream, \
                      d_x3, x3_len, d_frame_offsets, F, (uint32_t)fpg, g, d_wav_offsets, dp, d_wav, wav_cap, d_status,     \
                      (X3FrameMeta*)c->dec_meta.p, c->d_pace, c->dec_epoch & 0xFFFu, d_nf)
      if (rt.upb == 2u) X3B_LAUNCH(20u, 2u);
      else if (rt.unit == 10u) X3B_LAUNCH(10u, 1u);
      else X3B_LAUNCH(20u, 1u);
#undef X3B_LAUNCH
      ++c->dec_epoch;
    }
    else if (rt.kernel == X3_DEC_SPLIT) {
      // The segment index (x3_decode_split_kernel.h, "STRETCHES"): decode by it -- a lane per stretch of `seg_blocks` blocks,
      // nseg times the groups -- or record it while decoding frame by frame.  Frames of at most one stretch need none.
      X3SegArgs sg{nullptr, nullptr, 0u, 1u, 0u, 1u};
      uint64_t groups = (F + 63) / 64;
      if (by_seg) {
        const uint64_t nidx = seg_index_nseg((dp.spf + X3S_BL - 1) / X3S_BL, seg->seg_blocks);
        if (nidx >= 2) {
          sg.pitch = (uint32_t)(nidx - 1);
          if (seg->mode == 1) {
            // As many stretches as fill the chip and no more: a launch whose groups fill it anyway is faster frame by frame
            // (a stretch pays a group's start: header, ring fill, the flusher's tables; 1 080 groups: 0.70 against 0.78 ms,
            // profiles/r5/segments_split_kernel.txt), a stream of 42 groups five times faster by stretches.
            const uint64_t want = c->opt.seg_stretches > 0 ? (uint64_t)c->opt.seg_stretches
                                  : (groups * 2 >= (uint64_t)c->n_cus * 5 ? 1 : ((uint64_t)c->n_cus * 4 + groups - 1) / groups);
            const uint64_t mul = (nidx + std::min<uint64_t>(want, nidx) - 1) / std::min<uint64_t>(want, nidx);
            const uint64_t nseg = (nidx + mul - 1) / mul;
            if (nseg >= 2 && groups * nseg <= 0x7FFFFFFFull) {
              sg.in = reinterpret_cast<const uint2*>(seg->d_index);
              sg.mul = (uint32_t)mul;
              sg.sb = (uint32_t)(seg->seg_blocks * mul);
              sg.nseg = (uint32_t)nseg;
              groups *= nseg;
              HIPCHK(c, hipMemsetAsync(d_status, 0, F * sizeof(int32_t), dec_stream));  // (the stretches of a frame add to its status)
            }
          } else {
            sg.out = reinterpret_cast<uint2*>(seg->d_index);
            sg.sb = seg->seg_blocks;
            sg.nseg = (uint32_t)nidx;
            HIPCHK(c, hipMemsetAsync(seg->d_index, 0, (1 + F * (nidx - 1)) * sizeof(uint2), dec_stream));   // (no entry: not valid)
          }
        }
      }
      c->last_seg_stretches = sg.in ? (int)sg.nseg : (sg.out ? -1 : 0);
      X3_LAUNCH_TIMED(ts, x3_decode_split_kernel, dim3((unsigned)groups), dim3(64 * X3S_WAVES),
                         dyn_lds, dec_stream, d_x3, x3_len,
                         d_frame_offsets, F, g, d_wav_offsets, dp, d_wav, wav_cap, d_status, (X3FrameMeta*)c->dec_meta.p,
                         c->d_pace, c->dec_epoch & 0xFFFu, sg, d_nf);
      ++c->dec_epoch;
    }
    else if (rt.kernel == X3_DEC_SINGLE_FAST) {
      hipLaunchKernelGGL(x3_decode_fast_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, dec_stream, d_x3, x3_len,
                         d_frame_offsets, F, g, d_wav_offsets, dp, d_wav, wav_cap, d_status,
                         (X3FrameMeta*)c->dec_meta.p);
    } else {
      hipLaunchKernelGGL(x3_decode_lanes_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, dec_stream,
                         d_x3, x3_len, d_frame_offsets, F, g, d_wav_offsets, dp, d_wav, wav_cap, d_status,
                         (X3FrameMeta*)c->dec_meta.p);
    }
  }
  if (dec_stream == c->stream2) HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
  if (!c->opt.check_first && (rc = launch_check())) return rc;
  // join, then merge the two status arrays and summarise
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  if (no_check) {  // otherwise the check kernel's first thread does this
    X3DecodeSummary init;
    init.first_bad = F;
    init.samples_before = 0;
    init.first_bad_status = 0;
    init.replays = 0;
    *c->h_summary_init = init;
    HIPCHK(c, hipMemcpyAsync(c->d_summary, c->h_summary_init, sizeof init, hipMemcpyHostToDevice, c->stream));
  }
  hipLaunchKernelGGL(x3_decode_merge_kernel, dim3((unsigned)std::min<uint64_t>((F + 255) / 256, 64)), dim3(256), 0, c->stream,
                     (const int32_t*)c->dec_cstatus.p, d_status, (const X3FrameMeta*)c->dec_meta.p, F, c->d_summary,
                     d_x3, d_frame_offsets, g, d_wav_offsets, dp, d_wav, bl0 ? 1u : 0u, d_nf);
  c->dec_status_ptr = d_status;
  HIPCHK(c, hipGetLastError());
  c->decode_pending = true;
  c->dec_frames = F;
  return X3_OK;
}

extern "C" int x3_decode_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                             uint64_t n_frames, const x3_batch* batch, const uint64_t* d_wav_offsets,
                             const x3_params* p, int16_t* d_wav, uint64_t wav_cap, int32_t* d_status) {
  if (!c || !d_x3 || !d_frame_offsets || !p || !d_wav) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  // (caller-supplied sample offsets: the three-wave decoder needs rows on 8-byte boundaries, and only the caller can know
  // that without a pass over the offsets -- option "wav_offsets_x4")
  return decode_dev_impl(c, d_x3, x3_len, d_frame_offsets, n_frames, batch, d_wav_offsets, p, d_wav, wav_cap, d_status,
                         d_wav_offsets != nullptr && c->opt.wav_offsets_x4 != 0);
}

// x3_decode_dev with the SEGMENT INDEX (include/x3hip.h): record = 0 decodes by it, record = 1 decodes frame by frame and
// leaves it in d_seg_index for the next decode of the same stream
extern "C" uint64_t x3_seg_index_entries(uint64_t n_frames, const x3_params* p, uint32_t seg_blocks) {
  if (!p || seg_blocks == 0 || p->blocks_per_frame == 0) return 0;
  const uint64_t nseg = seg_stretches(p->blocks_per_frame, seg_blocks);
  return nseg >= 2 ? 1 + n_frames * (nseg - 1) : 0;   // (a header word, then nseg - 1 entries per frame)
}

extern "C" int x3_decode_dev_seg(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                 uint64_t n_frames, const x3_batch* batch, const uint64_t* d_wav_offsets,
                                 const x3_params* p, int16_t* d_wav, uint64_t wav_cap, int32_t* d_status,
                                 uint64_t* d_seg_index, uint32_t seg_blocks, int record) {
  if (!c || !d_x3 || !d_frame_offsets || !p || !d_wav) return X3_ERR_BAD_ARG;
  if (d_seg_index && !seg_index_args_ok(d_seg_index, seg_blocks)) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const X3SegSpec seg{d_seg_index, seg_blocks, d_seg_index ? (record ? 2 : 1) : 0};
  return decode_dev_impl(c, d_x3, x3_len, d_frame_offsets, n_frames, batch, d_wav_offsets, p, d_wav, wav_cap, d_status,
                         d_wav_offsets != nullptr && c->opt.wav_offsets_x4 != 0, false, &seg);
}

extern "C" int x3_decode_result(x3_ctx* c, uint64_t* first_bad, int* first_bad_status, uint64_t* samples_before) {
  if (!c || !c->decode_pending) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(X3DecodeSummary), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->decode_pending = false;
  c->last_decode_replays = c->h_summary->replays;
  c->decode_replays += c->h_summary->replays;
  if (c->h_summary->first_bad < c->dec_frames) {
    // rare: a frame is bad -- its status and the samples of the good frames before it
    hipLaunchKernelGGL(x3_decode_prefix_kernel, dim3(1), dim3(1024), 0, c->stream, (const int32_t*)c->dec_status_ptr,
                       (const X3FrameMeta*)c->dec_meta.p, c->dec_frames, c->d_summary);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(X3DecodeSummary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (first_bad) *first_bad = c->h_summary->first_bad;
  if (first_bad_status) *first_bad_status = c->h_summary->first_bad_status;
  if (samples_before) *samples_before = c->h_summary->samples_before;
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// GPU-side frame index of a device-resident stream (x3_index_kernels.h)
// ------------------------------------------------------------------------------------------------
// the scanning grid of a stream of len bytes: a workgroup per 4 KiB, at most 16 per CU (0: an empty stream)
static unsigned index_grid(const x3_ctx* c, uint64_t len) {
  const uint64_t chunks = (len + 15) >> 4;
  return (unsigned)std::min<uint64_t>((chunks + 255) / 256, (uint64_t)c->n_cus * 16);
}

// the walk's summary back to the host (one wait); a chain longer than max_frames is BAD_ARG
static int index_summary(x3_ctx* c, const X3IndexSummary* d_sum, X3IndexSummary* result) {
  HIPCHK(c, hipMemcpyAsync(c->h_summary_init, d_sum, sizeof *result, hipMemcpyDeviceToHost, c->stream));  // (pinned)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(result, c->h_summary_init, sizeof *result);
  if (result->pad) {
    c->last_error = "x3_index_dev: more frames in the stream than max_frames";
    return X3_ERR_BAD_ARG;
  }
  return X3_OK;
}

// what a walk of a stream of len bytes starts from: summary and candidate counter on the device (idx_sum), its grid
struct IndexWords { X3IndexSummary* d_sum; unsigned int* d_count; unsigned grid; };
static int index_words(x3_ctx* c, uint64_t len, IndexWords* w) {
  const int rc = ensure(c, c->idx_sum, 256);
  if (rc == X3_OK) *w = {(X3IndexSummary*)c->idx_sum.p, (unsigned int*)((char*)c->idx_sum.p + 128), index_grid(c, len)};
  return rc;
}

// The fast path's five launches (x3_index_kernels.h), nothing waited for: the summary -- frame and sample count, how the
// walk ends, pad2 = "not one clean chain: take the general walk" -- stays in *w.d_sum on the device.
static int index_fast_launch(x3_ctx* c, const uint8_t* d_x3, uint64_t len, uint64_t phantom, uint32_t bl0, uint64_t wav_cap,
                             uint64_t max_frames, uint64_t* d_frame_offsets, uint64_t* d_wav_offsets, const IndexWords& w) {
  const uint32_t* xw = reinterpret_cast<const uint32_t*>(d_x3);
  int rc;
  if (!w.grid) return X3_ERR_BAD_ARG;
  const size_t G = w.grid;
  if ((rc = ensure(c, c->idx_wg, G * X3I_WG_CANDS * sizeof(X3Cand)))) return rc;
  if ((rc = ensure(c, c->idx_sorted, G * X3I_WG_CANDS * sizeof(X3Cand)))) return rc;
  if ((rc = ensure(c, c->idx_scan, G * 32))) return rc;   // count u32 | base u32 | samp u64 | sbase u64 per span
  unsigned int* cnt = reinterpret_cast<unsigned int*>(c->idx_scan.p);
  uint32_t* base = reinterpret_cast<uint32_t*>(cnt + G);
  unsigned long long* samp = reinterpret_cast<unsigned long long*>(base + G);
  unsigned long long* sbase = samp + G;
  hipLaunchKernelGGL(x3_index_init_kernel, dim3(1), dim3(64), 0, c->stream, w.d_sum, w.d_count);
  hipLaunchKernelGGL(x3_index_candidates_kernel<true>, dim3(w.grid), dim3(256), 0, c->stream, xw, len, len + phantom, bl0,
                     (X3Cand*)c->idx_wg.p, 0u, cnt, samp, &w.d_sum->pad2);
  hipLaunchKernelGGL(x3_index_chain_kernel, dim3(1), dim3(1024), 0, c->stream, (const unsigned int*)cnt,
                     (const unsigned long long*)samp, (uint32_t)G, base, sbase, w.d_sum);
  hipLaunchKernelGGL(x3_index_link_kernel, dim3(w.grid), dim3(64), 0, c->stream, (const X3Cand*)c->idx_wg.p,
                     (const unsigned int*)cnt, (uint32_t)G, (const uint32_t*)base, (const unsigned long long*)sbase,
                     (X3Cand*)c->idx_sorted.p, (uint32_t)std::min<uint64_t>(G * X3I_WG_CANDS, 0xFFFFFFFFull),
                     (unsigned long long)max_frames, (unsigned long long)wav_cap, (unsigned long long*)d_frame_offsets,
                     (unsigned long long*)d_wav_offsets, w.d_sum);
  hipLaunchKernelGGL(x3_index_finalize_kernel, dim3(1), dim3(64), 0, c->stream, xw, len, len + phantom, bl0,
                     (const X3Cand*)c->idx_sorted.p, (const unsigned long long*)d_wav_offsets, w.d_sum);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

static int index_dev_impl(x3_ctx* c, const uint8_t* d_x3, uint64_t len, uint64_t phantom, uint32_t bl0, uint64_t wav_cap,
                          uint64_t max_frames, uint64_t* d_frame_offsets, uint64_t* d_wav_offsets,
                          X3IndexSummary* result) {
  if (reinterpret_cast<uintptr_t>(d_x3) & 3u) return X3_ERR_BAD_ARG;
  const uint32_t* xw = reinterpret_cast<const uint32_t*>(d_x3);
  int rc;
  IndexWords w;
  if ((rc = index_words(c, len, &w))) return rc;
  // ---- the fast path (round 4): a stream that is ONE CLEAN CHAIN -- what an encoder writes -- needs no hash table and
  // no pointer doubling.  The scanning workgroups keep their candidates in stream order, two scans number them, and one
  // kernel checks all at once that the first frame sits at offset 0 and that every frame ends where the next begins
  // (x3_index_kernels.h).  Five launches and one trip to the host where the general walk below takes thirteen and two;
  // anything else -- a false candidate inside a payload, damage, a frame the walk does not step over -- sets pad2, and
  // the general walk takes the stream as before.
  if (w.grid && !c->opt.index_no_fast) {
    if ((rc = index_fast_launch(c, d_x3, len, phantom, bl0, wav_cap, max_frames, d_frame_offsets, d_wav_offsets, w))) return rc;
    if ((rc = index_summary(c, w.d_sum, result))) return rc;
    if (!result->pad2) {
      ++c->index_fast;
      return X3_OK;
    }
  }
  ++c->index_general;
  hipLaunchKernelGGL(x3_index_init_kernel, dim3(1), dim3(64), 0, c->stream, w.d_sum, w.d_count);
  // ONE pass over the stream: the candidates go into a buffer sized for a frame every 256 bytes (the context keeps
  // it; typical streams hold one every few kilobytes); only a stream with more than that is scanned a second time.
  unsigned int n_cand = 0;
  if (w.grid) {
    const uint64_t guess = std::max<uint64_t>(4096, len / 256 + 1024);
    if ((rc = ensure(c, c->idx_cand, (size_t)std::min<uint64_t>(guess, 0x7FFFFFFFull) * sizeof(X3Cand)))) return rc;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(c->idx_cand.cap / sizeof(X3Cand), 0x7FFFFFFFull);
    hipLaunchKernelGGL(x3_index_candidates_kernel<false>, dim3(w.grid), dim3(256), 0, c->stream, xw, len, len + phantom, bl0,
                       (X3Cand*)c->idx_cand.p, cap, w.d_count, (unsigned long long*)nullptr, (uint32_t*)nullptr);
    HIPCHK(c, hipMemcpyAsync(c->h_crc, w.d_count, sizeof n_cand, hipMemcpyDeviceToHost, c->stream));  // (pinned)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(&n_cand, c->h_crc, sizeof n_cand);
    if (n_cand > cap) {  // rare: denser than one frame per 256 bytes
      ++c->index_rescans;
      if ((rc = ensure(c, c->idx_cand, (size_t)n_cand * sizeof(X3Cand)))) return rc;
      HIPCHK(c, hipMemsetAsync(w.d_count, 0, sizeof(unsigned int), c->stream));
      hipLaunchKernelGGL(x3_index_candidates_kernel<false>, dim3(w.grid), dim3(256), 0, c->stream, xw, len, len + phantom, bl0,
                         (X3Cand*)c->idx_cand.p, n_cand, w.d_count, (unsigned long long*)nullptr, (uint32_t*)nullptr);
    }
  }
  c->index_last_cands = n_cand;
  if (n_cand) {
    uint32_t tsize = 1024;
    while (tsize < 2u * n_cand && tsize < 0x80000000u) tsize <<= 1;
    uint32_t levels = 1;
    while ((1ull << (levels - 1)) < n_cand) ++levels;  // the top level spans 2^(levels-1) >= n_cand >= any chain
    if ((rc = ensure(c, c->idx_keys, (size_t)tsize * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(c, c->idx_vals, (size_t)tsize * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->idx_J, (size_t)levels * n_cand * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->idx_S, (size_t)levels * n_cand * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(c, c->idx_L, (size_t)levels * n_cand * sizeof(uint32_t)))) return rc;
    X3Cand* cand = (X3Cand*)c->idx_cand.p;
    unsigned long long* keys = (unsigned long long*)c->idx_keys.p;
    uint32_t* vals = (uint32_t*)c->idx_vals.p;
    uint32_t* J = (uint32_t*)c->idx_J.p;
    unsigned long long* S = (unsigned long long*)c->idx_S.p;
    uint32_t* L = (uint32_t*)c->idx_L.p;
    HIPCHK(c, hipMemsetAsync(keys, 0, (size_t)tsize * sizeof(unsigned long long), c->stream));
    const unsigned cg = (n_cand + 255) / 256;
    hipLaunchKernelGGL(x3_index_hash_insert_kernel, dim3(cg), dim3(256), 0, c->stream, (const X3Cand*)cand, n_cand,
                       keys, vals, tsize - 1);
    hipLaunchKernelGGL(x3_index_succ_kernel, dim3(cg), dim3(256), 0, c->stream, (const X3Cand*)cand, n_cand,
                       (const unsigned long long*)keys, (const uint32_t*)vals, tsize - 1, J, S, L);
    uint32_t r = 1;
    for (; r + 4 <= levels; r += 4)  // four levels a launch
      hipLaunchKernelGGL(x3_index_double4_kernel, dim3(cg), dim3(256), 0, c->stream, n_cand,
                         (const uint32_t*)(J + (size_t)(r - 1) * n_cand),
                         (const unsigned long long*)(S + (size_t)(r - 1) * n_cand),
                         (const uint32_t*)(L + (size_t)(r - 1) * n_cand), J + (size_t)r * n_cand,
                         S + (size_t)r * n_cand, L + (size_t)r * n_cand);
    for (; r < levels; ++r)
      hipLaunchKernelGGL(x3_index_double_kernel, dim3(cg), dim3(256), 0, c->stream, n_cand,
                         (const uint32_t*)(J + (size_t)(r - 1) * n_cand),
                         (const unsigned long long*)(S + (size_t)(r - 1) * n_cand),
                         (const uint32_t*)(L + (size_t)(r - 1) * n_cand), J + (size_t)r * n_cand,
                         S + (size_t)r * n_cand, L + (size_t)r * n_cand);
    // start node and chain length stay on the device: the emit grid covers every candidate
    hipLaunchKernelGGL(x3_index_emit_kernel, dim3(cg), dim3(256), 0, c->stream, (const X3Cand*)cand, n_cand, levels,
                       (const uint32_t*)J, (const unsigned long long*)S, (unsigned long long)max_frames,
                       (unsigned long long)wav_cap, (unsigned long long*)d_frame_offsets,
                       (unsigned long long*)d_wav_offsets, w.d_sum, (const unsigned long long*)keys, (const uint32_t*)vals,
                       tsize - 1, (const uint32_t*)(L + (size_t)(levels - 1) * n_cand));
    hipLaunchKernelGGL(x3_index_finalize_kernel, dim3(1), dim3(64), 0, c->stream, xw, len, len + phantom, bl0,
                       (const X3Cand*)cand, (const unsigned long long*)d_wav_offsets, w.d_sum);
  } else {
    hipLaunchKernelGGL(x3_index_finalize_kernel, dim3(1), dim3(64), 0, c->stream, xw, len, len + phantom, bl0,
                       (const X3Cand*)nullptr, (const unsigned long long*)nullptr, w.d_sum);
  }
  HIPCHK(c, hipGetLastError());
  return index_summary(c, w.d_sum, result);
}

extern "C" int x3_index_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t len, uint64_t max_frames,
                            uint64_t* d_frame_offsets, uint64_t* d_wav_offsets, uint64_t* n_frames,
                            uint64_t* n_samples, int* terminal) {
  if (!c || (!d_x3 && len) || !d_frame_offsets || !d_wav_offsets) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  X3IndexSummary r;
  int rc = index_dev_impl(c, d_x3, len, 0, 0, ~0ull, max_frames, d_frame_offsets, d_wav_offsets, &r);
  if (rc) return rc;
  if (n_frames) *n_frames = r.n_frames;
  if (n_samples) *n_samples = r.n_samples;
  if (terminal) *terminal = r.terminal;
  return X3_OK;
}

// The walk of a whole stream into c->frame_off / c->wav_off, whose sizes are not known before the candidate count: a cap of
// 2^20 frames first, and a stream with more once again with its upper bound (every frame is at least 22 bytes).
static int index_all_frames(x3_ctx* c, const uint8_t* d_x3, uint64_t len, uint64_t phantom, uint32_t bl0, uint64_t wav_cap,
                            X3IndexSummary* r) {
  const uint64_t max_frames = len / 22 + 1;
  uint64_t cap_frames = std::min<uint64_t>(max_frames, 1u << 20);
  for (;;) {
    int rc;
    if ((rc = ensure(c, c->frame_off, (cap_frames + 1) * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(c, c->wav_off, cap_frames * sizeof(uint64_t)))) return rc;
    rc = index_dev_impl(c, d_x3, len, phantom, bl0, wav_cap, cap_frames, (uint64_t*)c->frame_off.p, (uint64_t*)c->wav_off.p, r);
    if (rc != X3_ERR_BAD_ARG || cap_frames == max_frames) return rc;
    cap_frames = max_frames;
  }
}

extern "C" int x3_decode_stream_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t len, const x3_params* p, int16_t* d_wav,
                                    uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok, uint64_t* frame_errors) {
  if (!c || !p || (!d_x3 && len) || (!d_wav && wav_cap)) return X3_ERR_BAD_ARG;
  if (n_out) *n_out = 0;
  if (frames_ok) *frames_ok = 0;
  if (frame_errors) *frame_errors = 0;
  HIPCHK(c, hipSetDevice(c->device));
  const unsigned long long replays0 = c->decode_replays;
  const int rc = decode_stream_dev_impl(c, d_x3, len, 0, p, d_wav, wav_cap, nullptr, n_out, frames_ok, frame_errors);
  c->last_decode_replays = c->decode_replays - replays0;   // (one launch, or the second of two trips)
  return rc;
}

// the walk on the GPU (x3_index_kernels.h), then one decode launch; `phantom` as in walk_host.  own_out: decode
// into this scratch buffer, sized once the index knows the sample count, instead of d_wav.
int decode_stream_dev_impl(x3_ctx* c, const uint8_t* d_x3, uint64_t len, uint64_t phantom, const x3_params* p,
                                  int16_t* d_wav, uint64_t wav_cap, DevBuf* own_out, uint64_t* n_out,
                                  uint64_t* frames_ok, uint64_t* frame_errors) {
  int rc;
  X3IndexSummary r;
  // ---- ONE trip to the host (round 5).  A stream that is one clean chain of frames -- what an encoder
  // writes -- is walked by five launches that leave the frame count on the device; the decoder, the check pass and the merge
  // are enqueued right behind them with a grid for an upper bound of the count (a frame per KiB of stream) and read the
  // count from there (the groups behind it leave at once), and ONE copy brings both summaries back.  Anything the walk's
  // summary then objects to -- not a clean chain, more frames than the bound, sample offsets off the 8-byte grid -- is done
  // again the old way (the walk, a trip, the decode, a trip): the speculative decode wrote nothing that is not rewritten.
  {
    const uint64_t bound = std::min<uint64_t>(std::min<uint64_t>(len / 22 + 1, 1u << 20), len / 1024 + 64);
    // (parameters of fewer than 2 048 samples a frame do not try: frames that short often come more than one per KiB of
    // stream, the bound below then fails, and every call would pay the speculative launches and a sync before it takes the
    // two trips anyway -- ADVICE r5.  The gate is the parameters', the bound the stream's: quiet or zero content at 2 048
    // samples or more can still give frames of ~300 bytes, and such a stream tries, misses the bound and takes two trips.)
    // The decoder must take the frame count from the device: decode_route of the speculative call below.
    X3DevParams dq;
    const bool try_one = !own_out && !c->opt.index_no_fast && !c->opt.two_trips && spf_of(p) >= 2048 && len >= 22 &&
                         (reinterpret_cast<uintptr_t>(d_x3) & 3u) == 0 &&
                         derive_params(p, &dq) == X3_OK &&
                         decode_route(dq, X3Geom{0, 0, 1, bound}, d_wav, true, true, 0, c->opt).device_count;
    if (try_one) {
      if ((rc = ensure(c, c->frame_off, (bound + 1) * sizeof(uint64_t)))) return rc;
      if ((rc = ensure(c, c->wav_off, bound * sizeof(uint64_t)))) return rc;
      IndexWords iw;
      if ((rc = index_words(c, len, &iw))) return rc;
      rc = index_fast_launch(c, d_x3, len, phantom, 0u, wav_cap, bound, (uint64_t*)c->frame_off.p, (uint64_t*)c->wav_off.p, iw);
      if (rc == X3_OK)
        rc = decode_dev_impl(c, d_x3, len, (const uint64_t*)c->frame_off.p, bound, nullptr, (const uint64_t*)c->wav_off.p, p,
                             d_wav, wav_cap, nullptr, true, false, nullptr, &iw.d_sum->n_frames);
      if (rc == X3_OK) {
        HIPCHK(c, hipMemcpyAsync(c->h_summary_init, iw.d_sum, sizeof(X3IndexSummary), hipMemcpyDeviceToHost, c->stream));  // (pinned)
        HIPCHK(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(X3DecodeSummary), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memcpy(&r, c->h_summary_init, sizeof r);
        c->decode_pending = false;
        if (!r.pad && !r.pad2 && !r.unaligned && r.n_frames <= bound) {
          ++c->index_fast;
          ++c->stream_one_trip;
          const uint64_t F1 = r.n_frames;
          if (F1 == 0) return r.terminal;
          uint64_t first_bad = c->h_summary->first_bad, before = c->h_summary->samples_before;
          int bad_status = c->h_summary->first_bad_status;
          if (first_bad < F1) {   // rare: a frame is bad -- its status and the samples of the good frames before it
            c->dec_frames = F1;
            c->decode_pending = true;
            if ((rc = x3_decode_result(c, &first_bad, &bad_status, &before))) return rc;   // (counts the replays)
          } else {
            c->last_decode_replays = c->h_summary->replays;
            c->decode_replays += c->h_summary->replays;
          }
          if (n_out) *n_out = before;
          if (frames_ok) *frames_ok = first_bad;
          return walk_result(F1, first_bad, bad_status, r.terminal, frame_errors);
        }
      } else if (rc != X3_ERR_BAD_ARG) {
        return rc;
      }
    }
  }
  if ((rc = index_all_frames(c, d_x3, len, phantom, p->block_len == 0 ? 1u : 0u, wav_cap, &r))) return rc;
  const uint64_t F = r.n_frames;
  const int terminal = r.terminal;
  if (F == 0) return terminal;
  const x3_params pp = decoder_params(p);
  if (own_out) {
    if ((rc = ensure(c, *own_out, (r.n_samples + 65536) * sizeof(int16_t)))) return rc;
    d_wav = (int16_t*)own_out->p;
    wav_cap = std::min<uint64_t>(wav_cap, r.n_samples + 65535);
  }
  if ((rc = decode_dev_impl(c, d_x3, len, (const uint64_t*)c->frame_off.p, F, nullptr, (const uint64_t*)c->wav_off.p,
                            &pp, d_wav, wav_cap, nullptr, r.unaligned == 0, p->block_len == 0)))
    return rc;
  uint64_t first_bad = 0, before = 0;
  int bad_status = 0;
  if ((rc = x3_decode_result(c, &first_bad, &bad_status, &before))) return rc;
  if (n_out) *n_out = before;
  if (frames_ok) *frames_ok = first_bad;
  return walk_result(F, first_bad, bad_status, terminal, frame_errors);
}


extern "C" int x3_decode_stream(x3_ctx* c, const uint8_t* x3, uint64_t len, const x3_params* p, int16_t* wav,
                                uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok, uint64_t* frame_errors) {
  if (!c) return X3_ERR_BAD_ARG;
  const unsigned long long replays0 = c->decode_replays;
  const int rc = decode_stream_impl(c, x3, len, 0, p, wav, wav_cap, n_out, frames_ok, frame_errors);
  c->last_decode_replays = c->decode_replays - replays0;   // (summed over the host chunks)
  return rc;
}

void walk_host(const uint8_t* buf, uint64_t buf_len, uint64_t real_total, uint64_t believed_total,
                      const x3_params* p, uint64_t wav_cap, uint64_t max_samples, HostWalk* w, uint32_t n_ch) {
  uint64_t pos = 0, remaining = believed_total, nsamp = 0;
  for (;;) {
    if (remaining <= 20) break;
    if (real_total - pos < 20) { w->terminal = X3_ERR_IO; break; }  // read_exact past the real end of the data
    if (buf_len - pos < 20) { w->need_more = true; break; }
    x3_frame_header h;
    int rc = read_frame_header_ch(buf + pos, 20, &h, n_ch);
    if (rc) { w->terminal = rc; break; }
    if (remaining - 20 < h.payload_len) break;
    // the buffer-size test comes before the payload is read (decodefile.rs:118-124): a payload that is both too
    // long and cut off by the real end of the data is FrameHeaderInvalidPayloadLen, not Io
    if (h.payload_len > X3_READ_BUFFER_SIZE) { w->terminal = X3_ERR_FRAME_HEADER_INVALID_PAYLOAD_LEN; break; }
    if (real_total - pos - 20 < h.payload_len) { w->terminal = X3_ERR_IO; break; }
    if (buf_len - pos - 20 < h.payload_len) { w->need_more = true; break; }
    if (h.samples == 0 || h.payload_len < 2 * n_ch || nsamp + h.samples > wav_cap || (p->block_len == 0 && h.samples > 1)) {
      // payload CRC is checked before decode_frame runs, so let the GPU look at this frame too:
      // it reports the CRC error if there is one, BAD_ARG (reference panic) otherwise
      w->offs.push_back(pos);
      w->woffs.push_back(nsamp);
      w->terminal = X3_ERR_BAD_ARG;
      pos += 20 + (uint64_t)h.payload_len;
      break;
    }
    if (nsamp + h.samples > max_samples && !w->offs.empty()) { w->need_more = true; break; }
    w->offs.push_back(pos);
    w->woffs.push_back(nsamp);
    nsamp += h.samples;
    pos += 20 + h.payload_len;
    remaining -= 20 + h.payload_len;
  }
  w->nsamp = nsamp;
  w->end_pos = pos;
}

// decode the frames a walk collected from host memory into host memory: H2D, one decode launch, D2H of the
// samples in front of the first frame that fails.  *first_bad == F: all of them decoded.
int decode_frames_host(x3_ctx* c, const uint8_t* x3, uint64_t len, const HostWalk& w, const x3_params* p,
                              int16_t* wav, uint64_t wav_cap, uint64_t* before, uint64_t* first_bad, int* bad_status,
                              bool download,  // !download: the samples stay in c->out (x3_mgpu_decode_stream)
                              const uint8_t* d_x3) {  // the frames' bytes are on the device already
  const uint64_t F = w.offs.size();
  *before = 0;
  *first_bad = 0;
  *bad_status = 0;
  if (F == 0) return X3_OK;
  int rc;
  if (!d_x3) {
    if ((rc = ensure(c, c->in, len + 16))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->in.p, x3, len, hipMemcpyHostToDevice, c->stream));
    d_x3 = (const uint8_t*)c->in.p;
  }
  if ((rc = ensure(c, c->frame_off, (F + 1) * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, c->wav_off, F * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, c->out, (w.nsamp + 65536) * sizeof(int16_t)))) return rc;
  // (through pinned memory: a copy from pageable memory is staged by the runtime under a lock it shares with the large
  // pageable copies the chunked front ends have in flight on other threads -- 0.2-0.4 ms per call when they collide)
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the copy before this one has left the pinned block)
  if (c->h_walk_cap < 2 * F * sizeof(uint64_t)) {
    if (c->h_walk) HIPCHK(c, hipHostFree(c->h_walk));
    c->h_walk = nullptr;
    c->h_walk_cap = 0;
    const size_t want = (2 * F * sizeof(uint64_t) * 5 / 4 + 4095) & ~(size_t)4095;
    HIPCHK(c, hipHostMalloc(&c->h_walk, want));
    c->h_walk_cap = want;
  }
  std::memcpy(c->h_walk, w.offs.data(), F * sizeof(uint64_t));
  std::memcpy((uint64_t*)c->h_walk + F, w.woffs.data(), F * sizeof(uint64_t));
  HIPCHK(c, hipMemcpyAsync(c->frame_off.p, c->h_walk, F * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->wav_off.p, (uint64_t*)c->h_walk + F, F * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  const x3_params pp = decoder_params(p);
  const uint64_t dev_wav_cap = std::min<uint64_t>(wav_cap, w.nsamp + 65535);
  bool aligned = true;
  for (uint64_t v : w.woffs) aligned = aligned && (v & 3ull) == 0;   // (rows on the 8-byte grid)
  if ((rc = decode_dev_impl(c, d_x3, len, (const uint64_t*)c->frame_off.p, F, nullptr,
                            (const uint64_t*)c->wav_off.p, &pp, (int16_t*)c->out.p, dev_wav_cap, nullptr, aligned,
                            p->block_len == 0)))
    return rc;
  if ((rc = x3_decode_result(c, first_bad, bad_status, before))) return rc;
  if (download && *before)
    HIPCHK(c, hipMemcpyAsync(wav, c->out.p, *before * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return X3_OK;
}

// how the walk ends when frame `first_bad` of F failed with `bad_status` (decodefile.rs:96-100, 128-135)
int walk_result(uint64_t F, uint64_t first_bad, int bad_status, int terminal, uint64_t* frame_errors) {
  if (first_bad < F) {
    if (bad_status == X3_ERR_OUT_OF_BOUNDS_INVERSE || bad_status == X3_ERR_FRAME_DECODE_INVALID_BPF) {
      if (frame_errors) *frame_errors = 1;  // counted, the walk ends quietly (decodefile.rs:129-135)
      return X3_OK;
    }
    return bad_status;  // payload CRC mismatch (hard error) or BAD_ARG (reference panic)
  }
  return terminal;
}

// x3_decode_stream on a LONG stream in host memory, in chunks of whole frames (the file pipeline's scheme in one
// context).  The samples are 79 % of the bytes this entry point moves (config 3) and the link carries both directions at
// once, so: one host thread walks the headers of chunk i+2 (decodefile.rs:105-121, one dependent cache miss per frame)
// and sends its bytes up, this one decodes chunk i+1 (a launch of a few thousand frames lasts as long as one group of 64
// does: 0.6 ms, whatever the GPU could do beside it), a third brings the samples of chunk i down.  Two device buffers
// take turns on either side of the decoder.
static int decode_stream_host_chunked(x3_ctx* c, const uint8_t* x3, uint64_t len, uint64_t phantom, const x3_params* p,
                                      uint64_t chunk_samples, bool grow, int16_t* wav, uint64_t wav_cap, uint64_t* n_out,
                                      uint64_t* frames_ok, uint64_t* frame_errors) {
  int rc = x3_pipe_streams(c);
  if (rc) return rc;
  struct Chunk { HostWalk hw; uint64_t a, sample_off; const uint8_t* d_x3; };
  struct Piece { const void* src; uint64_t sample_off, count; };
  X3Handoff<Chunk> ready;
  X3Handoff<Piece> down;
  X3Progress decoded, landed;
  hipError_t up_err = hipSuccess, dl_err = hipSuccess;
  std::thread uploader, downloader;
  try {
  uploader = std::thread([&] {
    hipError_t e = hipSuccess;
    try {
    e = hipSetDevice(c->device);
    uint64_t a = 0, sample_off = 0;
    for (uint64_t k = 0; e == hipSuccess; ++k) {
      { std::lock_guard<std::mutex> g(decoded.mu); if (decoded.stop) break; }
      Chunk ck;
      const uint64_t real_total = len - a;
      // grow: a short first chunk so that the downloads start early, then longer ones (x1.5 up to x8: a chunk's walk and
      // upload take 0.7 of the time its predecessor's samples need to come down) -- every chunk costs a launch set and a
      // handful of runtime calls whatever its size, and those calls now and then stall for milliseconds beside the
      // pageable copies of the other two threads
      uint64_t budget = chunk_samples;
      if (grow)
        for (uint64_t g = 0; g < k && budget < 8 * chunk_samples; ++g) budget += budget >> 1;
      walk_host(x3 + a, real_total, real_total, real_total + phantom, p, wav_cap - sample_off, budget, &ck.hw);
      ck.a = a;
      ck.sample_off = sample_off;
      ck.d_x3 = nullptr;
      const bool last = !ck.hw.need_more;
      if (!ck.hw.offs.empty()) {
        // this chunk's bytes go where those of chunk k-3 were: not before that chunk has been decoded
        if (k >= 3 && !decoded.wait_for(k - 2)) break;
        DevBuf& buf = (k % 3) ? c->in_more[k % 3 - 1] : c->in;
        if (buf.cap < ck.hw.end_pos + 16) {
          if (buf.p) e = x3_dfree(buf.p);
          buf.p = nullptr;
          buf.cap = 0;
          const size_t want = (size_t)((ck.hw.end_pos * (grow ? 2 : 1) + 16 + (ck.hw.end_pos >> 3) + 255) & ~255ull);
          if (e == hipSuccess) e = x3_dmalloc(&buf.p, want);
          if (e == hipSuccess) buf.cap = want;
        }
        if (e == hipSuccess) e = hipMemcpyAsync(buf.p, x3 + a, ck.hw.end_pos, hipMemcpyHostToDevice, c->ul_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->ul_stream);
        if (e != hipSuccess) break;
        ck.d_x3 = static_cast<const uint8_t*>(buf.p);
      }
      a += ck.hw.end_pos;
      sample_off += ck.hw.nsamp;
      ready.push(std::move(ck));
      if (last) break;
    }
    } catch (...) { e = hipErrorOutOfMemory; }   // (walk_host's vectors, the hand-off: never std::terminate -- ADVICE r3)
    up_err = e;
    ready.close();
  });
  downloader = std::thread([&] {
    hipError_t e = hipSuccess;
    try {
      e = hipSetDevice(c->device);
      Piece pc;
      while (down.pop(&pc)) {
        if (e == hipSuccess && pc.count) {
          e = hipMemcpyAsync(wav + pc.sample_off, pc.src, pc.count * sizeof(int16_t), hipMemcpyDeviceToHost, c->dl_stream);
          if (e == hipSuccess) e = hipStreamSynchronize(c->dl_stream);
        }
        landed.advance();
      }
    } catch (...) { e = hipErrorOutOfMemory; landed.halt(); }
    dl_err = e;
  });
  } catch (const std::system_error&) {  // no thread to be had: the caller takes the stream in one piece
    decoded.halt();
    if (uploader.joinable()) uploader.join();
    return X3_PIPE_UNAVAILABLE;
  }
  uint64_t total = 0, frames = 0, ferr = 0, k = 0;
  int result = X3_OK;
  bool ended = false;
  Chunk ck;
  try {   // (as in encode_host_chunked: nothing thrown may pass the joins below)
  while (!ended && ready.pop(&ck)) {
    const uint64_t F = ck.hw.offs.size();
    uint64_t before = 0, first_bad = 0;
    int bad_status = 0;
    if (F) {
      // the buffer this chunk decodes into was the source of the download three chunks back
      if (k >= 3) landed.wait_for(k - 2);
      DevBuf* turn = (k % 3) ? &c->out_more[k % 3 - 1] : nullptr;
      if (turn) std::swap(c->out, *turn);
      if (grow && c->out.cap < (ck.hw.nsamp + 65536) * sizeof(int16_t))  // (room for the longer chunks that follow)
        rc = ensure(c, c->out, (2 * ck.hw.nsamp + 65536) * sizeof(int16_t));
      if (rc == X3_OK)
        rc = decode_frames_host(c, nullptr, ck.hw.end_pos, ck.hw, p, nullptr, wav_cap - ck.sample_off, &before, &first_bad,
                                &bad_status, false, ck.d_x3);
      const void* src = c->out.p;
      if (turn) std::swap(c->out, *turn);
      if (rc) break;
      down.push({src, ck.sample_off, before});
      decoded.advance();
      ++k;
    }
    uint64_t fe = 0;
    result = walk_result(F, first_bad, bad_status, ck.hw.need_more ? X3_OK : ck.hw.terminal, &fe);
    ferr += fe;
    frames += first_bad < F ? first_bad : F;
    total = ck.sample_off + before;
    ended = first_bad < F || !ck.hw.need_more;
  }
  } catch (...) {
    c->last_error = "x3_decode_stream: out of host memory in the chunked pipeline";
    rc = X3_ERR_HIP;
  }
  decoded.halt();  // (an uploader that waits for a decode that will not come)
  try { while (ready.pop(&ck)) {} } catch (...) {}
  down.close();
  uploader.join();
  downloader.join();
  if (rc) return rc;
  if (!ended) HIPCHK(c, up_err);
  HIPCHK(c, dl_err);
  if (n_out) *n_out = total;
  if (frames_ok) *frames_ok = frames;
  if (frame_errors) *frame_errors = ferr;
  return result;
}

// `phantom`: bytes the reader BELIEVES remain beyond the real data; a read that runs past the real end is
// X3Error::Io.
int decode_stream_impl(x3_ctx* c, const uint8_t* x3, uint64_t len, uint64_t phantom, const x3_params* p,
                              int16_t* wav, uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok,
                              uint64_t* frame_errors) {
  if (!c || !p || (!x3 && len) || (!wav && wav_cap)) return X3_ERR_BAD_ARG;
  if (n_out) *n_out = 0;
  if (frames_ok) *frames_ok = 0;
  if (frame_errors) *frame_errors = 0;
  HIPCHK(c, hipSetDevice(c->device));
  // Long streams: the header chain is one dependent cache miss per frame on the host (10 ms for the 69 120
  // frames of config 3), and a few launches on the GPU once the bytes are there anyway.  Short ones: the
  // other way round.  Option "host_walk" = 0/1 forces one or the other (tests run both).
  bool gpu_walk = len >= (4u << 20);
  if (c->opt.host_walk >= 0) gpu_walk = c->opt.host_walk == 0;
  // long streams in chunks, downloads beside uploads (unless a test pins the walk to the GPU)
  if (c->opt.host_walk != 0 && c->opt.host_chunk_frames >= 0 && len > 20 &&
      (c->opt.host_chunk_frames > 0 || len >= (16u << 20))) {
    const uint64_t spf = std::max<uint64_t>(spf_of(p), 1);
    const uint64_t chunk = c->opt.host_chunk_frames > 0 ? (uint64_t)c->opt.host_chunk_frames * spf : 16ull << 20;
    const int rc = decode_stream_host_chunked(c, x3, len, phantom, p, std::max<uint64_t>(chunk, 1), c->opt.host_chunk_frames == 0,
                                              wav, wav_cap, n_out, frames_ok, frame_errors);
    if (rc != X3_PIPE_UNAVAILABLE) return rc;
  }
  if (gpu_walk && len > 0) {
    int rc = ensure(c, c->in, len + 16);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->in.p, x3, len, hipMemcpyHostToDevice, c->stream));
    uint64_t before = 0;
    rc = decode_stream_dev_impl(c, (const uint8_t*)c->in.p, len, phantom, p, nullptr, wav_cap, &c->out, &before,
                                frames_ok, frame_errors);
    if (before) HIPCHK(c, hipMemcpyAsync(wav, c->out.p, before * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_out) *n_out = before;
    return rc;
  }
  HostWalk w;
  walk_host(x3, len, len, len + phantom, p, wav_cap, ~0ull, &w);
  const uint64_t F = w.offs.size();
  if (F == 0) return w.terminal;
  uint64_t first_bad = 0, before = 0;
  int bad_status = 0;
  int rc = decode_frames_host(c, x3, len, w, p, wav, wav_cap, &before, &first_bad, &bad_status);
  if (rc) return rc;
  if (n_out) *n_out = before;
  if (frames_ok) *frames_ok = first_bad;
  return walk_result(F, first_bad, bad_status, w.terminal, frame_errors);
}

// single bare payload (decoder::decode_frame): wrap it in a frame header so that the one decode
// kernel serves both paths; decode_frame itself checks no CRC, so a correct one is supplied.

static int decode_frame_impl(x3_ctx* c, const uint8_t* payload, uint64_t len, int16_t* wav, uint64_t wav_cap,
                             const x3_params* p, uint64_t samples, uint64_t* n_out, bool use_cache) {
  if (!c || !p || !payload || !wav) return X3_ERR_BAD_ARG;
  if (n_out) *n_out = 0;
  if (len < 2 || samples == 0 || wav_cap < 1) return X3_ERR_BAD_ARG;  // reference panics
  // block_len == 0: every block is empty, the frame's fate is in its block type bits (x3_replay_frame) and no block
  // ever fails to fit
  const bool bl0 = p->block_len == 0 && samples > 1;
  if (samples > wav_cap && !bl0) {
    // decode_frame slices wav block by block (decoder.rs:49) and panics at the first block that does not fit -- but an
    // error in a block in front of that one is returned first.  The blocks in front of it are a frame of their own:
    const uint64_t bl = p->block_len ? p->block_len : 1;
    const uint64_t n_fit = 1 + ((wav_cap - 1) / bl) * bl;  // the first sample and the whole blocks that fit
    if (n_fit > 1) {
      std::vector<int16_t> tmp(n_fit);
      const int rc_fit = decode_frame_impl(c, payload, len, tmp.data(), n_fit, p, n_fit, nullptr, false);
      if (rc_fit != X3_OK) return rc_fit;
    }
    return X3_ERR_BAD_ARG;  // slice index panic
  }
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (bl0 || samples > 0xFFFF || len >= X3_FRAME_MAX_LENGTH || len > X3_READ_BUFFER_SIZE) {
    // not a frame the walk would hand over (decodefile.rs:118-121, x3.rs:145) and not one a header can describe, but
    // decode_frame itself has no such limits: the reference's reader, one thread (x3_decode_replay.h)
    if (samples > 0xFFFFFFFFull || len > 0xFFFFFFFFull) return X3_ERR_BAD_ARG;
    X3DevParams dpr;
    const x3_params pr = decoder_params(p);
    if ((rc = derive(&pr, 0, &dpr))) return rc;
    if (bl0) dpr.block_len = 0;
    if ((rc = ensure(c, c->in, len + 16))) return rc;
    if ((rc = ensure(c, c->out, (samples + 16) * sizeof(int16_t)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->in.p, payload, len, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(x3_replay_one_kernel, dim3(1), dim3(64), 0, c->stream, (const uint8_t*)c->in.p, (uint32_t)len,
                       (uint32_t)samples, dpr, (int16_t*)c->out.p, (int32_t*)c->d_crc);
    HIPCHK(c, hipGetLastError());
    int32_t st = 0;
    HIPCHK(c, hipMemcpyAsync(&st, c->d_crc, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (st != X3D_OK) return st;
    HIPCHK(c, hipMemcpyAsync(wav, c->out.p, samples * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_out) *n_out = samples;
    return X3_OK;
  }
  if (c->fcache && use_cache) {  // a frame of the stream announced with x3_decode_prefetch: decoded ahead, a window at a time
    rc = frame_cache_serve(c, payload, len, p, samples, wav);
    if (rc == X3_OK) {
      if (n_out) *n_out = samples;
      return X3_OK;
    }
    if (rc != X3_FRAME_CACHE_MISS) return rc;
  }
  if ((rc = ensure(c, c->in, 20 + len + 16))) return rc;
  if ((rc = ensure(c, c->frame_off, 2 * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, c->wav_off, sizeof(uint64_t)))) return rc;
  if ((rc = ensure(c, c->out, (samples + 16) * sizeof(int16_t)))) return rc;
  HIPCHK(c, hipMemcpyAsync((uint8_t*)c->in.p + 20, payload, len, hipMemcpyHostToDevice, c->stream));
  uint16_t pcrc = 0;
  if ((rc = crc_dev_async(c, (const uint8_t*)c->in.p + 20, len))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pcrc = *c->h_crc;
  uint8_t hdr[20];
  x3_write_frame_header(samples, 1, len, pcrc, hdr);
  const uint64_t zero = 0;
  HIPCHK(c, hipMemcpyAsync(c->in.p, hdr, 20, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->frame_off.p, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->wav_off.p, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
  const x3_params pp = decoder_params(p);
  if ((rc = decode_dev_impl(c, (const uint8_t*)c->in.p, 20 + len, (const uint64_t*)c->frame_off.p, 1, nullptr,
                            (const uint64_t*)c->wav_off.p, &pp, (int16_t*)c->out.p, samples, nullptr)))
    return rc;
  uint64_t first_bad = 0, before = 0;
  int bad_status = 0;
  if ((rc = x3_decode_result(c, &first_bad, &bad_status, &before))) return rc;
  if (first_bad == 0) return bad_status;
  HIPCHK(c, hipMemcpyAsync(wav, c->out.p, samples * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_out) *n_out = samples;
  return X3_OK;
}

extern "C" int x3_decode_frame(x3_ctx* c, const uint8_t* payload, uint64_t len, int16_t* wav, uint64_t wav_cap,
                               const x3_params* p, uint64_t samples, uint64_t* n_out) {
  return decode_frame_impl(c, payload, len, wav, wav_cap, p, samples, n_out, true);
}


#ifdef X3_DBG_STAMPS
// stamp builds: the decoders' per-phase clocks (this unit's copy of x3_dbg; tools/scratch/dbg_stamps_split.py)
extern "C" int x3_dbg_read(x3_ctx* c, unsigned long long* out, uint64_t n) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyFromSymbol(out, HIP_SYMBOL(x3_dbg), n * sizeof(unsigned long long)));
  return X3_OK;
}
#endif

#include "x3_bits.h"
#define X3_MC_DECODE
#include "x3_mc.h"

// ---- x3_place_buffers (include/x3hip.h, "Placement"): the round trip timed on every pair of candidate buffers
extern "C" int x3_place_buffers(x3_ctx* c, const int16_t* d_wav, uint64_t n, const x3_params* p, uint8_t* const* d_streams,
                                uint32_t n_streams, uint64_t cap, uint64_t* d_frame_offsets, int16_t* const* d_backs,
                                uint32_t n_backs, uint32_t warm, uint32_t steps, double* ms_per_step) {
  if (!c || !d_wav || !n || !p || !d_streams || !n_streams || !d_frame_offsets || !d_backs || !n_backs || !steps || !ms_per_step)
    return X3_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n_streams; ++i) if (!d_streams[i]) return X3_ERR_BAD_ARG;
  for (uint32_t j = 0; j < n_backs; ++j) if (!d_backs[j]) return X3_ERR_BAD_ARG;
  const uint64_t F = x3_num_frames(n, p);
  const x3_batch b{n, n, 1};
  int rc = X3_OK;
  auto trips = [&](uint8_t* d_out, int16_t* d_back, uint32_t k) -> int {
    for (uint32_t t = 0; t < k; ++t) {
      if ((rc = x3_encode_dev(c, d_wav, &b, p, d_out, cap, 0, d_frame_offsets))) return rc;
      if ((rc = x3_decode_dev(c, d_out, cap, d_frame_offsets, F, &b, nullptr, p, d_back, n, nullptr))) return rc;
    }
    uint64_t pos = 0, first_bad = 0, before = 0;
    int bad_status = 0;
    if ((rc = x3_encode_result(c, &pos, nullptr))) return rc;       // (ByteWriterInsufficientMemory: cap does not hold the stream)
    if ((rc = x3_decode_result(c, &first_bad, &bad_status, &before))) return rc;
    return bad_status ? bad_status : X3_OK;
  };
  // (the clocks and the caches of a process that has just started: the first pair would pay for them)
  if ((rc = trips(d_streams[0], d_backs[0], 6 * warm + 1))) return rc;
  for (uint32_t i = 0; i < n_streams; ++i) {
    for (uint32_t j = 0; j < n_backs; ++j) {
      if (warm && (rc = trips(d_streams[i], d_backs[j], warm))) return rc;   // (the decoder's pace controller settles)
      const auto t0 = std::chrono::steady_clock::now();
      if ((rc = trips(d_streams[i], d_backs[j], steps))) return rc;
      const auto t1 = std::chrono::steady_clock::now();
      ms_per_step[(size_t)i * n_backs + j] = std::chrono::duration<double, std::milli>(t1 - t0).count() / steps;
    }
  }
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// random access: sample offsets and windows (x3_decode_window_kernel.h)
// ------------------------------------------------------------------------------------------------
extern "C" int x3_sample_offsets_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                     uint64_t n_frames, uint64_t* d_sample_offsets) {
  if (!c || !d_x3 || !d_frame_offsets || !d_sample_offsets) return X3_ERR_BAD_ARG;
  if (!frame_table_args_ok(d_x3, d_frame_offsets, n_frames) || (reinterpret_cast<uintptr_t>(d_sample_offsets) & 7u))
    return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(x3_window_sample_offsets_kernel, dim3(1), dim3(1024), 0, c->stream, d_x3, x3_len, d_frame_offsets,
                     n_frames, d_sample_offsets);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

// ---- what the access calls share on the host (windows, ranges, levels; a stream's and a corpus's): the frames they read,
// the carver of their workspaces, the grids, the read-back of a result
// the pieces of one block, each a multiple of 256 bytes behind its base
struct BlockCarver {
  char* base; size_t at;
  template <class T> T* take(uint64_t count, size_t round = 256) {   // (round 1: the next piece follows directly)
    T* const piece = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + at);
    at = (at + count * sizeof(T) + round - 1) & ~(round - 1);
    return piece;
  }
};

// workgroups of a grid-stride kernel: one per `per_group` units, at most X3W_GRID_LIMIT (the counts are on the device)
static unsigned grid_for(uint64_t units, uint64_t per_group) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((units + per_group - 1) / per_group, X3W_GRID_LIMIT));
}

// The frames a call reads: the stream, its frame and sample offsets, the parameters, and the segment index as the kernels
// take it -- idx NULL and nseg 1 where there is no usable one (none given, or frames of one stretch).  max_frames: the most
// frames one window or range can cover, the stream's or the longest entry's.
struct FrameSource {
  const uint8_t* d_x3; uint64_t x3_len;
  const uint64_t* d_frame_offsets; const uint64_t* d_sample_offsets; uint64_t F;
  X3DevParams dp; uint64_t spf;
  const uint2* idx; uint32_t seg_blocks, nseg;
  uint64_t max_frames;
  void index(const uint64_t* d_seg_index, uint32_t sb) {
    seg_blocks = sb;
    nseg = d_seg_index ? seg_index_nseg(dp.blocks_per_frame, sb) : 1u;
    idx = nseg >= 2 ? reinterpret_cast<const uint2*>(d_seg_index) : nullptr;
  }
};

// ... of a caller's stream: the checks every stream entry point makes on its frame table, index and parameters
static int stream_source(const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets, const uint64_t* d_sample_offsets,
                         uint64_t n_frames, const x3_params* p, const uint64_t* d_seg_index, uint32_t seg_blocks, FrameSource* s) {
  if (!d_x3 || !d_frame_offsets || !d_sample_offsets || !p) return X3_ERR_BAD_ARG;
  if (!frame_table_args_ok(d_x3, d_frame_offsets, n_frames) || (reinterpret_cast<uintptr_t>(d_sample_offsets) & 7u))
    return X3_ERR_BAD_ARG;
  if (d_seg_index && !seg_index_args_ok(d_seg_index, seg_blocks)) return X3_ERR_BAD_ARG;
  s->d_x3 = d_x3, s->x3_len = x3_len;
  s->d_frame_offsets = d_frame_offsets, s->d_sample_offsets = d_sample_offsets, s->F = s->max_frames = n_frames;
  s->spf = spf_of(p);
  const int rc = derive_block_params(p, &s->dp);
  if (rc == X3_OK) s->index(d_seg_index, seg_blocks);
  return rc;
}

// The read-back of a pending call: its summary (`bytes` of it, in `ws`) to h and the wait for it; the slot is free again
static int pending_fetch(x3_ctx* c, x3_ctx::PendingCall& call, const DevBuf& ws, void* h, size_t bytes) {
  if (!call.pending) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(h, (char*)ws.p + call.sum_off, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  call.pending = false;
  return X3_OK;
}

// a summary's (n_bad, first = min(unit << 8 | status) over the bad units) as the result calls give them; none bad: the
// count of units and status 0
static void first_bad_of(uint64_t bad, uint64_t first, uint64_t count, uint64_t* n_bad, uint64_t* first_bad,
                         int* first_bad_status) {
  if (n_bad) *n_bad = bad;
  if (first_bad) *first_bad = bad ? (first >> 8) : count;
  if (first_bad_status) *first_bad_status = bad ? (int)(first & 0xFFu) : 0;
}

// the argument checks x3_decode_windows_dev and x3_corpus_windows_dev share
static bool windows_args_ok(uint64_t n_windows, uint32_t window_len, const void* d_out, int out_format, const uint64_t* d_starts,
                            const int32_t* d_status) {
  if (!d_starts || !d_out || !d_status) return false;
  if (window_len == 0 || n_windows == 0 || n_windows > (1ull << 40)) return false;
  if (out_format != X3_WINDOW_I16 && out_format != X3_WINDOW_F32) return false;
  const uint64_t esz = out_format == X3_WINDOW_F32 ? 4u : 2u;
  if (reinterpret_cast<uintptr_t>(d_out) % esz) return false;
  return (reinterpret_cast<uintptr_t>(d_starts) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d_status) & 3u) == 0;
}

// the rows of a ranges call (x3_decode_ranges_dev / x3_corpus_ranges_dev); a windows call has none: its rows are w * L
struct RangeRows {
  const uint32_t* d_lens;
  uint64_t row_stride, out_cap;
  uint64_t* d_out_offsets;
};

// The workspace (WinWs, x3_internal.h): plans, the two scans, per-frame verdicts, a block of replay scratch per window, the
// summary, the plan's starts; ranges: the scan of the lengths and the lengths that have room
uint32_t windows_scratch_per(uint32_t block_len) { return (block_len + 7u) & ~7u; }

size_t windows_carve(char* base, uint64_t n, uint64_t F, uint32_t scratch_per, bool ranges, WinWs* w) {
  BlockCarver k{base, 0};
  w->plan = k.take<X3WinPlan>(n);
  w->cov_off = k.take<unsigned long long>(n + 1);
  w->item_off = k.take<unsigned long long>(n + 1);
  w->fst = k.take<int32_t>(F);
  w->scratch = k.take<int16_t>(n * scratch_per);
  w->sum = k.take<X3WinSummary>(1);
  w->gstart = k.take<uint64_t>(n, ranges ? 256 : 1);   // (a windows call's block ends here)
  w->off = ranges ? k.take<unsigned long long>(n + 1) : nullptr;
  w->elen = ranges ? k.take<uint32_t>(n, 1) : nullptr;
  return k.at;
}

// The launch set of a windows or ranges call (x3_decode_window_kernel.h) behind its plan step: plan(grid, plan, gstart, sum)
// enqueues the plan kernel and returns the starts the decode and fix-up kernels read (the caller's, or the plan's gstart).
// rows: the geometry of a ranges call (the scan, decode and fix-up kernels are then the range siblings), NULL for windows of
// window_len; len_hint sizes the grids (the window length, or what a range can have on average).
template <class Plan>
static int windows_launch(x3_ctx* c, const FrameSource& s, uint64_t n, uint32_t window_len, const RangeRows* rows, void* d_out,
                          int out_format, int32_t* d_status, Plan plan_step) {
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t scratch_per = windows_scratch_per(s.dp.block_len);
  WinWs w;
  int rc;
  if ((rc = ensure(c, c->win_ws, windows_carve(nullptr, n, s.F, scratch_per, rows != nullptr, &w)))) return rc;
  windows_carve((char*)c->win_ws.p, n, s.F, scratch_per, rows != nullptr, &w);
  // grids: the plan covers the windows; the grid-stride kernels take as many groups as the work of full-length frames needs,
  // at most X3W_GRID_LIMIT (their counts are on the device).  Ranges: the lengths are device data; what fits the rows is
  // out_cap / n (packed) or the stride on average, and ranges without room cover nothing.  Both are the caller's words and
  // may be far above what is drawn: a length has 32 bits and a range covers no more frames than the stream (or the longest
  // entry) has, so a roomy buffer does not size the grids.
  const uint64_t len_hint = !rows ? window_len : std::min<uint64_t>(rows->row_stride ? rows->row_stride : rows->out_cap / n, 0xFFFFFFFFull);
  uint64_t frames_per = len_hint / (s.spf ? s.spf : 1) + 2;
  if (rows) frames_per = std::max<uint64_t>(1, std::min(frames_per, s.max_frames));
  const uint64_t* d_starts = plan_step(dim3(grid_for(n, 256)), w.plan, w.gstart, w.sum);
  // (ranges: n < 2^31 and frames_per < 2^32 + 3, the first product cannot wrap; the second is capped before it is formed)
  const uint64_t cov_hint = n * frames_per, item_hint = std::min<uint64_t>(cov_hint, 256ull * X3W_GRID_LIMIT) * s.nseg;
  const dim3 g_check(grid_for(cov_hint, 4)), g_decode(grid_for(item_hint, 256)), g_fix(grid_for(n, 4));
  if (rows)
    hipLaunchKernelGGL(x3_range_scan_kernel, dim3(1), dim3(1024), 0, c->stream, w.plan, n, rows->d_lens, rows->row_stride,
                       rows->out_cap, s.idx, s.seg_blocks, s.nseg, w.cov_off, w.item_off, w.off, w.elen, rows->d_out_offsets,
                       w.sum);
  else
    hipLaunchKernelGGL(x3_window_scan_kernel, dim3(1), dim3(1024), 0, c->stream, w.plan, n, s.idx, s.seg_blocks, s.nseg,
                       w.cov_off, w.item_off);
  hipLaunchKernelGGL(x3_window_check_kernel, g_check, dim3(256), 0, c->stream, s.d_x3, s.x3_len, s.d_frame_offsets,
                     s.d_sample_offsets, w.plan, n, w.cov_off, w.fst);
  auto decode_fixup = [&](auto g) {   // g: the rows, X3WinFixedGeo or X3WinRangeGeo
    using Geo = decltype(g);
    hipLaunchKernelGGL((x3_window_decode_kernel<Geo>), g_decode, dim3(256), 0, c->stream, s.d_x3, s.x3_len, s.d_frame_offsets,
                       s.d_sample_offsets, d_starts, (const X3WinPlan*)w.plan, n, g, (const unsigned long long*)w.item_off, s.dp,
                       s.idx, s.seg_blocks, s.nseg, d_out, out_format, w.fst);
    hipLaunchKernelGGL((x3_window_fixup_kernel<Geo>), g_fix, dim3(256), 0, c->stream, s.d_x3, s.d_frame_offsets,
                       s.d_sample_offsets, d_starts, (const X3WinPlan*)w.plan, n, g, s.dp, (const int32_t*)w.fst, d_out, out_format,
                       d_status, w.scratch, scratch_per, w.sum);
  };
  if (rows)
    decode_fixup(X3WinRangeGeo{(const uint32_t*)w.elen, (const unsigned long long*)w.off, rows->row_stride});
  else
    decode_fixup(X3WinFixedGeo{window_len});
  HIPCHK(c, hipGetLastError());
  c->windows.pending = true;
  c->windows.ranges = rows != nullptr;
  c->windows.count = n;
  c->windows.sum_off = (size_t)((char*)w.sum - (char*)c->win_ws.p);
  return X3_OK;
}

extern "C" int x3_decode_windows_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                     const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                     const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                     uint64_t n_windows, uint32_t window_len, void* d_out, int out_format, int32_t* d_status) {
  if (!c || !windows_args_ok(n_windows, window_len, d_out, out_format, d_starts, d_status)) return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = stream_source(d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, &s);
  if (rc) return rc;
  return windows_launch(c, s, n_windows, window_len, nullptr, d_out, out_format, d_status,
                        [&](dim3 grid, X3WinPlan* plan, uint64_t*, X3WinSummary* sum) -> const uint64_t* {
                          hipLaunchKernelGGL(x3_window_plan_kernel, grid, dim3(256), 0, c->stream, d_sample_offsets, n_frames,
                                             d_starts, n_windows, window_len, plan, sum);
                          return d_starts;
                        });
}

// the result of the pending windows (ranges: false) or ranges (true) call; a call of the other kind stays pending
static int windows_result(x3_ctx* c, bool ranges, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status,
                          uint64_t* total_samples) {
  if (!c || c->windows.ranges != ranges) return X3_ERR_BAD_ARG;
  X3WinSummary h{0, 0, 0, 0};
  const int rc = pending_fetch(c, c->windows, c->win_ws, &h, sizeof h);
  if (rc) return rc;
  c->last_window_replays = h.replays;
  first_bad_of(h.n_bad, h.first, c->windows.count, n_bad, first_bad, first_bad_status);
  if (total_samples) *total_samples = h.total;
  return X3_OK;
}

extern "C" int x3_decode_windows_result(x3_ctx* c, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status) {
  return windows_result(c, false, n_bad, first_bad, first_bad_status, nullptr);
}

// ranges: a length per range, rows packed or padded
// the argument checks x3_decode_ranges_dev and x3_corpus_ranges_dev share
static bool ranges_args_ok(const x3_ctx* c, uint64_t n_ranges, const uint32_t* d_lens, uint64_t row_stride, const void* d_out,
                           uint64_t out_cap, int out_format, const uint64_t* d_starts, const uint64_t* d_out_offsets,
                           const int32_t* d_status) {
  if (!d_starts || !d_lens || !d_out || !d_status || c->capturing) return false;
  if (n_ranges == 0 || n_ranges > 0x7FFFFFFFull) return false;
  if (out_format != X3_WINDOW_I16 && out_format != X3_WINDOW_F32) return false;
  const uint64_t esz = out_format == X3_WINDOW_F32 ? 4u : 2u;
  if (reinterpret_cast<uintptr_t>(d_out) % esz || out_cap > ~0ull / esz) return false;
  if (row_stride ? row_stride > out_cap / n_ranges : !d_out_offsets) return false;
  return (reinterpret_cast<uintptr_t>(d_starts) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d_lens) & 3u) == 0 &&
         (reinterpret_cast<uintptr_t>(d_out_offsets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d_status) & 3u) == 0;
}

extern "C" int x3_decode_ranges_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                    const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                    const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                    const uint32_t* d_lens, uint64_t n_ranges, uint64_t row_stride, void* d_out,
                                    uint64_t out_cap, int out_format, uint64_t* d_out_offsets, int32_t* d_status) {
  if (!c || !ranges_args_ok(c, n_ranges, d_lens, row_stride, d_out, out_cap, out_format, d_starts, d_out_offsets, d_status))
    return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = stream_source(d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, &s);
  if (rc) return rc;
  const RangeRows rows{d_lens, row_stride, out_cap, d_out_offsets};
  return windows_launch(c, s, n_ranges, 0, &rows, d_out, out_format, d_status,
                        [&](dim3 grid, X3WinPlan* plan, uint64_t*, X3WinSummary* sum) -> const uint64_t* {
                          hipLaunchKernelGGL(x3_range_plan_kernel, grid, dim3(256), 0, c->stream, d_sample_offsets, n_frames,
                                             d_starts, d_lens, n_ranges, plan, sum);
                          return d_starts;
                        });
}

extern "C" int x3_decode_ranges_result(x3_ctx* c, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status,
                                       uint64_t* total_samples) {
  return windows_result(c, true, n_bad, first_bad, first_bad_status, total_samples);
}

// ------------------------------------------------------------------------------------------------
// levels: per-bin min, max, count, sum and sum of squares without a sample buffer (x3_levels_kernel.h)
// ------------------------------------------------------------------------------------------------
// the argument checks x3_levels_dev and x3_corpus_levels_dev share
static bool levels_args_ok(const x3_ctx* c, const x3_level* d_levels, uint64_t n_rows, const int32_t* d_frame_status) {
  if (!d_levels || n_rows == 0 || n_rows > 0x7FFFFFFFull || c->capturing) return false;
  return (reinterpret_cast<uintptr_t>(d_levels) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d_frame_status) & 3u) == 0;
}

// the rows of n_samples positions: max(1, ceil(n_samples / bin_len)), one with bin_len 0
static uint64_t levels_rows_of(uint64_t n_samples, uint64_t bin_len) {
  return bin_len == 0 || n_samples == 0 ? 1 : n_samples / bin_len + (n_samples % bin_len ? 1 : 0);
}

// The workspace (LevWs, x3_internal.h): per-frame verdicts, plans, row counts and their scan; the partial rows; replay
// scratch; summary; row prefix.  The fix-up's waves: one block of replay scratch each, 32 MiB of it at most.
uint32_t levels_scratch_per(uint32_t block_len) { return (std::min<uint32_t>(block_len, 0x10000u) + 7u) & ~7u; }

uint64_t levels_fix_waves(uint64_t F, uint32_t scratch_per) {
  return std::max<uint64_t>(1, std::min<uint64_t>({(F + 3) / 4 * 4, 4096, (32ull << 20) / (2ull * scratch_per) / 4 * 4}));
}

size_t levels_carve(char* base, uint64_t F, uint64_t n_rows, uint64_t fix_waves, uint32_t scratch_per, uint64_t n_ent, LevWs* w,
                    uint64_t planes) {
  BlockCarver k{base, 0};
  w->fst = k.take<int32_t>(F);
  w->frames = k.take<X3LevFrame>(F);
  w->cnt = k.take<uint32_t>(F);
  w->row = k.take<unsigned long long>(F + 1);
  w->rows = k.take<x3_level>(planes * (n_rows + F));   // (a tone bank: a plane of n_rows + F rows per tone)
  w->scratch = k.take<int16_t>(std::max<uint64_t>(fix_waves, 4) * scratch_per);
  w->sum = k.take<X3LevSummary>(1);
  w->row_first = k.take<unsigned long long>(n_ent + 1, 1);
  w->tail = reinterpret_cast<int32_t*>(w->cnt);   // (the scan kernel is the row counts' last reader)
  return k.at;
}

static bool levels_signal_ok(int signal) { return signal == X3_LEVEL_SIGNAL_SAMPLES || signal == X3_LEVEL_SIGNAL_DIFF; }

// x3_level_fir as the kernels take it, the taps at and behind T zero; false: not 1 <= T <= 8, shift <= 15, sum |c| <= 32768
static bool levels_fir_taps(const x3_level_fir* fir, X3FirTaps* k) {
  if (!fir || fir->n_taps < 1 || fir->n_taps > X3L_FIR_TAPS || fir->shift > 15) return false;
  uint32_t mag = 0;
  for (uint32_t t = 0; t < X3L_FIR_TAPS; ++t) {
    k->c[t] = t < fir->n_taps ? fir->taps[t] : 0;
    mag += (uint32_t)std::abs(k->c[t]);
  }
  k->T = fir->n_taps, k->shift = fir->shift;
  return mag <= 32768u;
}

// x3_level_tone as the kernels take it; false: NULL, a NULL or misaligned table, reserved != 0
static bool levels_tone_arg(const x3_level_tone* tone, X3LevToneTail* t) {
  if (!tone || !tone->d_table || (reinterpret_cast<uintptr_t>(tone->d_table) & 3u) != 0 || tone->reserved != 0) return false;
  t->table = reinterpret_cast<const uint32_t*>(tone->d_table);
  t->step = tone->step;
  return true;
}

// x3_level_tone_bank as the kernels take it, the steps at and behind n_tones zero; false: NULL, n_tones not 1 .. 8,
// reserved != 0, a NULL or misaligned table
static bool levels_tone_bank_arg(const x3_level_tone_bank* bank, X3LevToneBankTail* t) {
  if (!bank || bank->n_tones < 1 || bank->n_tones > X3_TONE_BANK_MAX || bank->reserved != 0 || !bank->d_table ||
      (reinterpret_cast<uintptr_t>(bank->d_table) & 3u) != 0)
    return false;
  t->table = reinterpret_cast<const uint32_t*>(bank->d_table);
  t->n_tones = bank->n_tones;
  for (uint32_t i = 0; i < X3L_TONE_BANK; ++i) t->steps[i] = i < bank->n_tones ? bank->steps[i] : 0;
  t->rows_stride = t->levels_stride = 0;   // (levels_launch's)
  return true;
}
static_assert(X3_TONE_BANK_MAX == X3L_TONE_BANK, "the header's bank is the kernels'");
static_assert(sizeof(x3_tone_level) == sizeof(x3_level) && alignof(x3_tone_level) == alignof(x3_level) &&
                  offsetof(x3_tone_level, re) == offsetof(x3_level, sum_sq) && offsetof(x3_tone_level, im) == offsetof(x3_level, sum) &&
                  offsetof(x3_tone_level, min) == offsetof(x3_level, min) && offsetof(x3_tone_level, max) == offsetof(x3_level, max) &&
                  offsetof(x3_tone_level, n) == offsetof(x3_level, n),
              "x3_tone_level has x3_level's layout slot for slot");

// The signal of a levels or range-levels call: its kind and that kind's payload as the kernels take it.  Built only from an
// argument one of the four checks above has passed, so the launchers and the *_call helpers ask it and check nothing again.
struct LevSignal {
  enum Kind { SAMPLES, DIFF, FIR, TONE, BANK } kind;
  X3FirTaps fir{};            // FIR
  X3LevToneTail tone{};       // TONE: records hold re and im in x3_level's first two slots
  X3LevToneBankTail bank{};   // BANK, two tones or more: d_levels and the partial rows hold n_tones PLANES
  explicit LevSignal(int signal) : kind(signal == X3_LEVEL_SIGNAL_DIFF ? DIFF : SAMPLES) {}
  explicit LevSignal(const X3FirTaps& k) : kind(FIR), fir(k) {}
  explicit LevSignal(const X3LevToneTail& t) : kind(TONE), tone(t) {}
  // (a bank of one tone IS the tone call: here and nowhere else)
  explicit LevSignal(const X3LevToneBankTail& b) : kind(b.n_tones == 1 ? TONE : BANK), tone{b.table, b.steps[0]}, bank(b) {}

  uint64_t planes() const { return kind == BANK ? bank.n_tones : 1; }
  // a range's plan: a lead kernel behind it and tail[], lead[] in the workspace; the frames it may hold in front
  bool lead() const { return kind == DIFF || kind == FIR; }
  uint64_t lead_frames() const { return kind == FIR ? fir.T - 1 : kind == DIFF ? 1 : 0; }
  bool fir_ws() const { return kind == FIR; }   // an edge record per (frame, stretch) in a workspace of its own
  bool seam() const { return kind == DIFF || (kind == FIR && fir.T > 1); }   // a seam kernel behind the merge
};

// all planes of a bank in one launch of the adapter: n_tones * n_rows <= 2^31 - 1 (n_rows itself: levels_args_ok)
static bool levels_planes_ok(const LevSignal& g, uint64_t n_rows) { return n_rows <= 0x7FFFFFFFull / g.planes(); }

// The launch set of a levels call behind its prep step: prep(grid, row_first, fst, frames, cnt) enqueues the kernels that
// give every frame its position, its records and its row count.  n_ent: entries of a corpus call (their row prefix lives
// in the workspace), 0 for a stream.  g picks the instance of the accumulate and fix-up kernels and the seam kernel behind
// the merge, in the switch below: DIFF leaves every good frame's last sample in the workspace, FIR its edge records in
// fir_ws (lev_ws keeps its layout); a bank's accumulate instance is the smallest of NT = 2, 4, 8 that holds the tones, its
// fix-up's is NT = 8, and the merge kernel runs once per plane.
template <class Prep>
static int levels_launch(x3_ctx* c, const FrameSource& s, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                         int32_t* d_frame_status, uint64_t n_ent, const LevSignal& g, Prep prep) {
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t F = s.F, cap = n_rows + F, planes = g.planes();
  const uint32_t scratch_per = levels_scratch_per(s.dp.block_len);
  const uint64_t fix_waves = levels_fix_waves(F, scratch_per);
  LevWs w;
  int rc;
  if ((rc = ensure(c, c->lev_ws, levels_carve(nullptr, F, n_rows, fix_waves, scratch_per, n_ent, &w, planes)))) return rc;
  levels_carve((char*)c->lev_ws.p, F, n_rows, fix_waves, scratch_per, n_ent, &w, planes);
  if (g.fir_ws() && (rc = ensure(c, c->fir_ws, (size_t)(F * s.nseg) * sizeof(X3FirEdge)))) return rc;
  hipLaunchKernelGGL(x3_levels_init_kernel, dim3(grid_for(planes * (n_rows + cap), 256)), dim3(256), 0, c->stream, d_levels,
                     planes * n_rows, w.rows, planes * cap, w.sum);
  hipLaunchKernelGGL(x3_levels_check_kernel, dim3(grid_for(F, 4)), dim3(256), 0, c->stream, s.d_x3, s.x3_len, s.d_frame_offsets,
                     s.d_sample_offsets, F, w.fst);
  prep(dim3(grid_for(F, 256)), w.row_first, (const int32_t*)w.fst, w.frames, w.cnt);
  hipLaunchKernelGGL(x3_levels_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)w.cnt, F, cap, w.row, w.fst);
  // the two kernels that decode, for a signal; the merge; the signal's seam kernel
  auto run = [&](auto sig, auto fix, auto tail, auto seam) {
    hipLaunchKernelGGL(x3_levels_accum_kernel<decltype(sig)>, dim3(grid_for(F * s.nseg, 256)), dim3(256), 0, c->stream, s.d_x3, s.x3_len,
                       s.d_frame_offsets, F, s.dp, s.idx, s.seg_blocks, s.nseg, bin_len, (const X3LevFrame*)w.frames,
                       (const unsigned long long*)w.row, w.rows, w.fst, tail);
    hipLaunchKernelGGL(x3_levels_fixup_kernel<decltype(fix)>, dim3((unsigned)((fix_waves + 3) / 4)), dim3(256), 0, c->stream, s.d_x3,
                       s.d_frame_offsets, F, s.dp, bin_len, (const X3LevFrame*)w.frames, w.fst, d_levels, d_frame_status,
                       w.scratch, scratch_per, w.sum, tail);
    for (uint64_t t = 0; t < planes; ++t)   // (a plane's rows and records: the same frames, row scan and verdicts)
      hipLaunchKernelGGL(x3_levels_merge_kernel, dim3(grid_for(cap, 256)), dim3(256), 0, c->stream, (const X3LevFrame*)w.frames,
                         (const unsigned long long*)w.row, F, cap, (const x3_level*)w.rows + t * cap, (const int32_t*)w.fst,
                         d_levels + t * n_rows);
    if (g.seam()) seam();
  };
  auto no_seam = [] {};
  switch (g.kind) {
    case LevSignal::BANK: {
      X3LevToneBankTail t = g.bank;
      t.rows_stride = cap, t.levels_stride = n_rows;
      if (t.n_tones <= 2) run(X3LevToneBank<2>{}, X3LevToneBank<X3L_TONE_BANK>{}, t, no_seam);
      else if (t.n_tones <= 4) run(X3LevToneBank<4>{}, X3LevToneBank<X3L_TONE_BANK>{}, t, no_seam);
      else run(X3LevToneBank<X3L_TONE_BANK>{}, X3LevToneBank<X3L_TONE_BANK>{}, t, no_seam);
      break;
    }
    case LevSignal::TONE: run(X3LevTone{}, X3LevTone{}, g.tone, no_seam); break;
    case LevSignal::FIR:
      run(X3LevFir{}, X3LevFir{}, X3LevFirTail{g.fir, (X3FirEdge*)c->fir_ws.p, s.nseg}, [&] {
        hipLaunchKernelGGL(x3_levels_fir_seam_kernel, dim3(grid_for(F * s.nseg, 256)), dim3(256), 0, c->stream, F, s.dp.block_len,
                           s.idx, s.seg_blocks, s.nseg, bin_len, (const X3LevFrame*)w.frames, (const int32_t*)w.fst,
                           (const X3FirEdge*)c->fir_ws.p, s.nseg, g.fir, d_levels);
      });
      break;
    case LevSignal::DIFF:
      run(X3LevDiff{}, X3LevDiff{}, w.tail, [&] {
        if (F > 1)   // (one frame has no seam)
          hipLaunchKernelGGL(x3_levels_seam_kernel, dim3(grid_for(F, 256)), dim3(256), 0, c->stream, s.d_x3, s.x3_len,
                             s.d_frame_offsets, F, bin_len, (const X3LevFrame*)w.frames, (const int32_t*)w.fst,
                             (const int32_t*)w.tail, d_levels);
      });
      break;
    case LevSignal::SAMPLES: run(X3LevSamples{}, X3LevSamples{}, X3LevNoTail{}, no_seam); break;
  }
  HIPCHK(c, hipGetLastError());
  c->levels.pending = true;
  c->levels.count = F;
  c->levels.sum_off = (size_t)((char*)w.sum - (char*)c->lev_ws.p);
  return X3_OK;
}

// the stream form of the levels calls behind the check of the signal
static int stream_levels_call(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                              const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p, const uint64_t* d_seg_index,
                              uint32_t seg_blocks, uint64_t bin_len, x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status,
                              const LevSignal& g) {
  if (!levels_args_ok(c, d_levels, n_bins, d_frame_status) || !levels_planes_ok(g, n_bins)) return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = stream_source(d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, &s);
  if (rc) return rc;
  return levels_launch(c, s, bin_len, d_levels, n_bins, d_frame_status, 0, g,
                       [&](dim3 grid, unsigned long long*, const int32_t* fst, X3LevFrame* frames, uint32_t* cnt) {
                         hipLaunchKernelGGL(x3_levels_prep_kernel, grid, dim3(256), 0, c->stream, d_sample_offsets, n_frames,
                                            bin_len, n_bins, fst, frames, cnt);
                       });
}

extern "C" int x3_signal_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                    const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                    const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len, x3_level* d_levels,
                                    uint64_t n_bins, int32_t* d_frame_status, int signal) {
  if (!c || !levels_signal_ok(signal)) return X3_ERR_BAD_ARG;
  return stream_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, bin_len,
                            d_levels, n_bins, d_frame_status, LevSignal(signal));
}

extern "C" int x3_fir_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                 const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                 const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len, x3_level* d_levels,
                                 uint64_t n_bins, int32_t* d_frame_status, const x3_level_fir* fir) {
  X3FirTaps k;
  if (!c || !levels_fir_taps(fir, &k)) return X3_ERR_BAD_ARG;
  return stream_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, bin_len,
                            d_levels, n_bins, d_frame_status, LevSignal(k));
}

extern "C" int x3_tone_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                  const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                  const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len, x3_tone_level* d_levels,
                                  uint64_t n_bins, int32_t* d_frame_status, const x3_level_tone* tone) {
  X3LevToneTail t;
  if (!c || !levels_tone_arg(tone, &t)) return X3_ERR_BAD_ARG;
  return stream_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, bin_len,
                            reinterpret_cast<x3_level*>(d_levels), n_bins, d_frame_status, LevSignal(t));
}

// the bank: n_tones tone calls plane by plane in one pass
extern "C" int x3_tone_bank_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                       const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                       const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len, x3_tone_level* d_levels,
                                       uint64_t n_bins, int32_t* d_frame_status, const x3_level_tone_bank* bank) {
  X3LevToneBankTail t;
  if (!c || !levels_tone_bank_arg(bank, &t)) return X3_ERR_BAD_ARG;
  return stream_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, bin_len,
                            reinterpret_cast<x3_level*>(d_levels), n_bins, d_frame_status, LevSignal(t));
}

// the adapter: tone records -> the level records of the band (x3_tone_power_kernel); in place, or rows that do not overlap
extern "C" int x3_tone_power_levels_dev(x3_ctx* c, const x3_tone_level* d_tone, uint64_t n_rows, x3_level* d_levels) {
  if (!c || !d_tone || !d_levels || n_rows == 0 || n_rows > 0x7FFFFFFFull) return X3_ERR_BAD_ARG;
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_tone), b = reinterpret_cast<uintptr_t>(d_levels);
  const uintptr_t bytes = (uintptr_t)n_rows * sizeof(x3_level);
  if (((a | b) & 7u) != 0 || (a != b && a < b + bytes && b < a + bytes)) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(x3_tone_power_kernel, dim3(grid_for(n_rows, 256)), dim3(256), 0, c->stream,
                     reinterpret_cast<const x3_level*>(d_tone), n_rows, d_levels);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

extern "C" int x3_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                             const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                             const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len, x3_level* d_levels,
                             uint64_t n_bins, int32_t* d_frame_status) {
  return x3_signal_levels_dev(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, bin_len,
                              d_levels, n_bins, d_frame_status, X3_LEVEL_SIGNAL_SAMPLES);
}

extern "C" int x3_levels_result(x3_ctx* c, uint64_t* n_bad_frames, uint64_t* first_bad, int* first_bad_status) {
  if (!c) return X3_ERR_BAD_ARG;
  X3LevSummary h{0, 0, 0};
  const int rc = pending_fetch(c, c->levels, c->lev_ws, &h, sizeof h);
  if (rc) return rc;
  c->last_levels_replays = h.replays;
  first_bad_of(h.n_bad, h.first, c->levels.count, n_bad_frames, first_bad, first_bad_status);
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// the segment index by a walk (x3_seg_index_kernel.h)
// ------------------------------------------------------------------------------------------------
// One launch behind a 8-byte memset of the counter; nothing is allocated, nothing waits, no pending state is touched.
static int seg_index_launch(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets, uint64_t F,
                            const X3DevParams& dp, uint64_t* d_seg_index, uint32_t seg_blocks) {
  const uint32_t nseg = seg_index_nseg(dp.blocks_per_frame, seg_blocks);
  HIPCHK(c, hipMemsetAsync(c->d_seg_irregular, 0, sizeof(unsigned long long), c->stream));
  if (nseg < 2) return X3_OK;   // (x3_seg_index_entries() == 0: frames of one stretch have no index)
  const uint64_t groups = std::min<uint64_t>((F + 63) / 64, (uint64_t)c->n_cus * X3X_WAVES_PER_CU);
  hipLaunchKernelGGL(x3_seg_index_kernel, dim3((unsigned)groups), dim3(64), 0, c->stream, d_x3, x3_len, d_frame_offsets, F, dp,
                     reinterpret_cast<uint2*>(d_seg_index), seg_blocks, nseg, c->d_seg_irregular);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

extern "C" int x3_seg_index_build_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                      uint64_t n_frames, const x3_params* p, uint64_t* d_seg_index, uint32_t seg_blocks) {
  if (!c || !d_x3 || !d_frame_offsets || !p || !d_seg_index) return X3_ERR_BAD_ARG;
  if (!frame_table_args_ok(d_x3, d_frame_offsets, n_frames) || !seg_index_args_ok(d_seg_index, seg_blocks)) return X3_ERR_BAD_ARG;
  X3DevParams dp;
  int rc = derive_block_params(p, &dp);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return seg_index_launch(c, d_x3, x3_len, d_frame_offsets, n_frames, dp, d_seg_index, seg_blocks);
}

// ------------------------------------------------------------------------------------------------
// BATCHES OF STREAMS (include/x3hip.h; x3_streams_kernel.h)
// ------------------------------------------------------------------------------------------------
#include "x3_streams_kernel.h"

// ---- THE SEGMENTED WALK: every entry's frames by one launch set, for the batch decode and for the corpus build alike
static uint64_t seg_cands(uint64_t G) { return std::max<uint64_t>(G * X3I_WG_CANDS, 1); }   // candidate slots of G spans

int seg_entries(const uint64_t* offsets, const uint64_t* lengths, uint64_t n, uint64_t x3_len, std::vector<uint32_t>* span_first,
                uint64_t* G, uint64_t* bytes) {
  auto spans = [](uint64_t len) { return (len + X3T_SPAN_BYTES - 1) / X3T_SPAN_BYTES; };
  *G = *bytes = 0;
  for (uint64_t e = 0; e < n; ++e) {
    if (offsets[e] > x3_len || lengths[e] > x3_len - offsets[e]) return X3_ERR_BAD_ARG;
    *G += spans(lengths[e]);
    *bytes += lengths[e];
    if (*G > 0x7FFFFFFFull / X3I_WG_CANDS) return X3_ERR_BAD_ARG;   // (refused here: neither sum can wrap)
  }
  span_first->assign(n + 1, 0);
  for (uint64_t e = 0; e < n; ++e) (*span_first)[e + 1] = (*span_first)[e] + (uint32_t)spans(lengths[e]);
  return X3_OK;
}

size_t segwalk_carve(char* base, uint64_t n, uint64_t G, SegWalkWs* w) {
  const uint64_t cap = seg_cands(G);
  BlockCarver k{base, 0};
  w->eoff = k.take<uint64_t>(n, 1);   // eoff | elen | span_first back to back: segwalk_launch uploads them in one copy
  w->elen = k.take<uint64_t>(n, 1);
  w->span_first = k.take<uint32_t>(n + 1);
  w->isum = k.take<X3IndexSummary>(1);
  w->cnt = k.take<unsigned int>(G);
  w->base = k.take<uint32_t>(G);
  w->samp = k.take<unsigned long long>(G);
  w->sbase = k.take<unsigned long long>(G);
  w->cand = k.take<X3Cand>(cap);
  w->frame_off = k.take<unsigned long long>(cap);
  w->wav_off = k.take<unsigned long long>(cap);
  w->fent = k.take<uint32_t>(cap);
  w->ent_flags = k.take<uint32_t>(n);
  w->ent_end = k.take<unsigned long long>(n);
  w->ent_nsamp = k.take<unsigned long long>(n);
  return k.at;
}

// Enqueues the walk over a validated entry table: the table to the device (src_tab_upload), a clean summary and clean entry
// flags, then the candidates, the scans and the links; no kernel for a table without bytes.  row_len and x4 are those of the
// decode launch the frame table is for.  The INDEX form is row_len ~0 and no four-sample grid: every frame the walk steps
// over is live.
static int segwalk_launch(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* offsets, const uint64_t* lengths,
                          const std::vector<uint32_t>& span_first, uint64_t phantom, uint64_t row_len, uint32_t x4,
                          const SegWalkWs& w) {
  const uint64_t n = span_first.size() - 1, G = span_first[n];
  int rc;
  if ((rc = src_tab_upload(c, w.eoff, {{offsets, 8 * n}, {lengths, 8 * n}, {span_first.data(), 4 * (n + 1)}}))) return rc;
  HIPCHK(c, hipMemsetAsync(w.isum, 0, sizeof(X3IndexSummary), c->stream));
  HIPCHK(c, hipMemsetAsync(w.ent_flags, 0, 4 * n, c->stream));
  if (G) {
    hipLaunchKernelGGL(x3_streams_candidates_kernel, dim3((unsigned)G), dim3(256), 0, c->stream,
                       reinterpret_cast<const uint32_t*>(d_x3), x3_len, w.eoff, w.elen, w.span_first, (uint32_t)n, phantom,
                       w.cand, w.cnt, w.samp, w.ent_flags);
    hipLaunchKernelGGL(x3_index_chain_kernel, dim3(1), dim3(1024), 0, c->stream, w.cnt, w.samp, (uint32_t)G, w.base, w.sbase,
                       w.isum);
    hipLaunchKernelGGL(x3_streams_link_kernel, dim3((unsigned)G), dim3(64), 0, c->stream, w.cand, w.cnt, w.base, w.sbase, w.eoff,
                       w.span_first, (uint32_t)n, x3_len, row_len, x4, w.frame_off, w.wav_off, w.fent, w.ent_flags, w.ent_end,
                       w.ent_nsamp);
  }
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

// an entry of a batch on a 4-byte boundary of its own (st_one), for the walks that take one stream
static int entry_copy(x3_ctx* c, const uint8_t* d_x3, uint64_t off, uint64_t len) {
  const int rc = ensure(c, c->st_one, len + 64);
  if (rc == X3_OK && len) HIPCHK(c, hipMemcpyAsync(c->st_one.p, d_x3 + off, len, hipMemcpyDeviceToDevice, c->stream));
  return rc;
}

// ---- the batch decode.  A call's block (st_walk): the walk's workspace, then the call's own words (StreamsWs)
size_t streams_carve(char* base, uint64_t n, uint64_t G, StreamsWs* s) {
  BlockCarver k{base, segwalk_carve(base, n, G, s)};
  s->sum = k.take<X3StreamsSum>(1);
  s->status = k.take<int32_t>(seg_cands(G));
  s->ent_bad = k.take<unsigned long long>(n);
  s->nout = k.take<unsigned long long>(n);
  s->dirty = k.take<uint32_t>(n);
  return k.at;
}

// x3_streams_rows_kernel for either format: float32 rows from the int16 rows at ws, or int16 rows zeroed in place from
// their sample counts on (ws is not read)
static void streams_rows_launch(x3_ctx* c, dim3 grid, int fmt, const int16_t* ws, void* out, uint64_t n, uint64_t row_len,
                                const unsigned long long* nout, unsigned long long no_value, const X3StreamsSum* sum) {
  auto* const rows = fmt == X3_WINDOW_F32 ? x3_streams_rows_kernel<true> : x3_streams_rows_kernel<false>;
  hipLaunchKernelGGL(rows, grid, dim3(256), 0, c->stream, ws, out, n, row_len, nout, no_value, sum);
}

// the walk's candidate count and, with `sum`, the call's summary: one wait (through the pinned block, 128 bytes apart)
static int streams_fetch(x3_ctx* c, const StreamsWs& l, unsigned long long* total, X3StreamsSum* sum) {
  char* const h = (char*)c->h_summary_init;
  HIPCHK(c, hipMemcpyAsync(h, l.isum, sizeof(X3IndexSummary), hipMemcpyDeviceToHost, c->stream));
  if (sum) HIPCHK(c, hipMemcpyAsync(h + 128, l.sum, sizeof *sum, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *total = reinterpret_cast<const X3IndexSummary*>(h)->n_chain;
  if (sum) std::memcpy(sum, h + 128, sizeof *sum);
  return X3_OK;
}

// decode launch over frames [0, F) of the table (d_nf: the count on the device, or nullptr when F is the count), then the
// per-entry verdicts and the rows
static int streams_finish(x3_ctx* c, uint64_t F, bool device_count) {
  auto& s = c->streams;
  StreamsWs l;
  streams_carve((char*)c->st_walk.p, s.n, s.G, &l);
  const uint64_t total_samples = s.n * s.row_len;
  int16_t* d_wav = s.fmt == X3_WINDOW_F32 ? (int16_t*)c->st_ws.p : (int16_t*)s.d_out;
  const unsigned long long* d_nf = &l.isum->n_chain;
  int rc;
  if (F) {
    if ((rc = decode_dev_impl(c, s.d_x3, s.x3_len, (const uint64_t*)l.frame_off, F, nullptr, (const uint64_t*)l.wav_off, &s.p,
                              d_wav, total_samples, l.status, s.row_len % 4u == 0, false, nullptr,
                              device_count ? d_nf : nullptr)))
      return rc;
    c->decode_pending = false;   // (the merge kernel's summary is not this call's result)
    hipLaunchKernelGGL(x3_streams_firstbad_kernel, dim3((unsigned)std::min<uint64_t>((F + 255) / 256, 4096)), dim3(256), 0,
                       c->stream, l.status, l.fent, F, d_nf, l.ent_bad);
  }
  hipLaunchKernelGGL(x3_streams_resolve_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, c->stream,
                     reinterpret_cast<const uint32_t*>(s.d_x3), s.x3_len, l.eoff, l.elen, l.span_first, (uint32_t)s.n, s.phantom,
                     l.base, (uint32_t)s.G, d_nf, F, l.status, l.wav_off, l.ent_flags, l.ent_bad, l.ent_end, l.ent_nsamp,
                     s.row_len, s.d_results, l.nout, l.dirty, l.sum);
  const dim3 rg((unsigned)std::min<uint64_t>((s.row_len + 255) / 256, s.fmt == X3_WINDOW_F32 ? 64 : 8),
                (unsigned)std::min<uint64_t>(s.n, 65535));
  streams_rows_launch(c, rg, s.fmt, (const int16_t*)c->st_ws.p, s.d_out, s.n, s.row_len, l.nout, 0ull, l.sum);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

extern "C" int x3_decode_streams_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* offsets,
                                     const uint64_t* lengths, uint64_t n, uint32_t flags, const x3_params* p, void* d_out,
                                     uint64_t row_len, int out_format, x3_stream_result* d_results) {
  if (!c || !offsets || !lengths || !p || !d_out || !d_results || (!d_x3 && x3_len)) return X3_ERR_BAD_ARG;
  if (n == 0 || row_len == 0 || n > 0xFFFFFFF0ull || (flags & ~X3_STREAMS_ARCHIVE_FRAMES)) return X3_ERR_BAD_ARG;
  if (out_format != X3_WINDOW_I16 && out_format != X3_WINDOW_F32) return X3_ERR_BAD_ARG;
  const uint64_t ss = out_format == X3_WINDOW_F32 ? 4 : 2;
  if ((reinterpret_cast<uintptr_t>(d_x3) & 3u) || (reinterpret_cast<uintptr_t>(d_out) & (ss - 1)) ||
      (reinterpret_cast<uintptr_t>(d_results) & 7u))
    return X3_ERR_BAD_ARG;
  if (row_len > (~0ull / 4) / n) return X3_ERR_BAD_ARG;
  if (x3_params_validate(p) != X3_OK) return X3_ERR_BAD_ARG;
  std::vector<uint32_t> span_first;
  uint64_t G = 0, bytes = 0;
  if (seg_entries(offsets, lengths, n, x3_len, &span_first, &G, &bytes)) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  auto& s = c->streams;
  s.pending = false;
  s.d_x3 = d_x3;
  s.x3_len = x3_len;
  s.n = n;
  s.row_len = row_len;
  s.phantom = (flags & X3_STREAMS_ARCHIVE_FRAMES) ? 8 : 0;
  s.fmt = out_format;
  s.p = *p;
  s.d_out = d_out;
  s.d_results = d_results;
  s.G = G;
  s.off.assign(offsets, offsets + n);
  s.len.assign(lengths, lengths + n);
  c->decode_pending = false;
  // Block length 0 (frames of one sample, decided by block types alone) and option "index_no_fast": every entry takes the
  // general walk at result time.
  s.all_general = p->block_len == 0 || c->opt.index_no_fast != 0;
  int rc;
  StreamsWs l;
  if ((rc = ensure(c, c->st_walk, streams_carve(nullptr, n, G, &l)))) return rc;
  if (out_format == X3_WINDOW_F32 && (rc = ensure(c, c->st_ws, 2 * n * row_len + 64))) return rc;
  if (s.all_general) {
    s.pending = true;
    return X3_OK;
  }
  streams_carve((char*)c->st_walk.p, n, G, &l);
  const uint32_t x4 = row_len % 4u == 0 ? 1u : 0u;
  if ((rc = segwalk_launch(c, d_x3, x3_len, offsets, lengths, span_first, s.phantom, row_len, x4, l))) return rc;
  // the call's own clean state: its summary (bad_first = all ones) and the entries' first failing frames
  HIPCHK(c, hipMemsetAsync(l.sum, 0, sizeof(X3StreamsSum), c->stream));
  HIPCHK(c, hipMemsetAsync(&l.sum->bad_first, 0xFF, 8, c->stream));
  HIPCHK(c, hipMemsetAsync(l.ent_bad, 0xFF, 8 * n, c->stream));
  // The decode launch covers a bound on the frame count (a frame per KiB of entry, as x3_decode_stream_dev's one-trip
  // path bounds it) and reads the real count from the device; a batch with more is launched again, with the count, by
  // x3_decode_streams_result.  A decoder that cannot read the count from the device: one wait for it, here.
  X3DevParams dq;
  const uint64_t bound = std::min<uint64_t>(seg_cands(G), bytes / 1024 + n + 64);
  const bool dev_count = G && derive_params(p, &dq) == X3_OK &&
                         decode_route(dq, X3Geom{0, 0, 1, bound}, out_format == X3_WINDOW_F32 ? (const int16_t*)c->st_ws.p
                                                                                                : (const int16_t*)d_out,
                                      true, x4 != 0, 0, c->opt).device_count;
  unsigned long long F = bound;
  if (!G) F = 0;
  else if (!dev_count && (rc = streams_fetch(c, l, &F, nullptr))) return rc;
  if ((rc = streams_finish(c, F, dev_count))) return rc;
  s.pending = true;
  return X3_OK;
}

// one entry by x3_decode_stream_dev's own path (an aligned copy of its bytes), into its row: the general walk
static int streams_general(x3_ctx* c, uint64_t e, x3_stream_result* r) {
  auto& s = c->streams;
  const uint64_t len = s.len[e];
  int rc;
  if ((rc = entry_copy(c, s.d_x3, s.off[e], len))) return rc;
  int16_t* row;
  if (s.fmt == X3_WINDOW_F32) {
    if ((rc = ensure(c, c->st_row, 2 * s.row_len + 64))) return rc;
    row = (int16_t*)c->st_row.p;
  } else {
    row = (int16_t*)s.d_out + e * s.row_len;
  }
  uint64_t n_out = 0, fok = 0, ferr = 0;
  rc = decode_stream_dev_impl(c, (const uint8_t*)c->st_one.p, len, s.phantom, &s.p, row, s.row_len, nullptr, &n_out, &fok, &ferr);
  if (rc == X3_ERR_HIP) return rc;
  if (n_out > s.row_len) n_out = s.row_len;   // (cannot happen: wav_cap)
  r->n_out = n_out;
  r->frames_ok = fok;
  r->status = rc;
  r->frame_errors = (uint32_t)ferr;
  if (s.fmt == X3_WINDOW_F32)
    streams_rows_launch(c, dim3((unsigned)std::min<uint64_t>((s.row_len + 255) / 256, 1024), 1u), s.fmt, row,
                        (float*)s.d_out + e * s.row_len, 1, s.row_len, nullptr, n_out, nullptr);
  else if (n_out < s.row_len)
    HIPCHK(c, hipMemsetAsync(row + n_out, 0, 2 * (s.row_len - n_out), c->stream));
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

extern "C" int x3_decode_streams_result(x3_ctx* c, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status) {
  if (!c || !c->streams.pending) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  auto& s = c->streams;
  s.pending = false;
  std::vector<uint32_t> general;
  uint64_t nb = 0, fb = s.n;
  int fst = 0;
  if (s.all_general) {
    general.resize(s.n);
    for (uint64_t e = 0; e < s.n; ++e) general[e] = (uint32_t)e;
  } else {
    StreamsWs l;
    streams_carve((char*)c->st_walk.p, s.n, s.G, &l);
    X3StreamsSum sum;
    unsigned long long total = 0;
    int rc;
    if ((rc = streams_fetch(c, l, &total, &sum))) return rc;
    if (sum.over) {   // more frames than the launch covered: again, with the count
      HIPCHK(c, hipMemsetAsync(&l.sum->over, 0, 4, c->stream));
      if ((rc = streams_finish(c, total, false))) return rc;
      if ((rc = streams_fetch(c, l, &total, &sum))) return rc;
    }
    first_bad_of(sum.n_bad, sum.bad_first, s.n, &nb, &fb, &fst);
    if (sum.n_dirty) {
      general.resize(sum.n_dirty);
      HIPCHK(c, hipMemcpyAsync(general.data(), l.dirty, 4ull * sum.n_dirty, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  if (!general.empty()) {
    std::vector<x3_stream_result> res(general.size());
    for (size_t i = 0; i < general.size(); ++i) {
      int rc = streams_general(c, general[i], &res[i]);
      if (rc) return rc;
      if (res[i].status != 0) {
        ++nb;
        if (general[i] < fb) { fb = general[i]; fst = res[i].status; }
      }
      HIPCHK(c, hipMemcpyAsync(s.d_results + general[i], &res[i], sizeof res[i], hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // (res is read by the copies)
  }
  c->last_streams_general = general.size();
  c->streams_general += general.size();
  if (n_bad) *n_bad = nb;
  if (first_bad) *first_bad = fb;
  if (first_bad_status) *first_bad_status = fst;
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// CORPUS: windows of many streams (include/x3hip.h)
// ------------------------------------------------------------------------------------------------
struct x3_corpus {
  int device = 0;
  const uint8_t* d_x3 = nullptr;
  uint64_t x3_len = 0, n = 0, F = 0, total = 0;
  uint64_t max_frames = 0;             // the longest entry's frames (sizes the grids of a ranges call)
  x3_params p{};
  uint32_t seg_blocks = 0;             // in use (0: no index)
  uint64_t* d_frame_off = nullptr;     // F words (at least one): the frames' byte offsets in d_x3, entries in order
  uint64_t* d_so = nullptr;            // F + 1 words: x3_window_sample_offsets_kernel over that table
  x3_corpus_entry* d_ent = nullptr;    // n entries
  uint64_t* d_index = nullptr;         // the segment index (1 + F * (nseg - 1) words), or nullptr
  std::vector<x3_corpus_entry> ent;    // the entry table's host copy
};

extern "C" void x3_corpus_destroy(x3_corpus* k) {
  if (!k) return;
  int dev = -1;
  (void)hipGetDevice(&dev);
  (void)hipSetDevice(k->device);
  for (void* q : {(void*)k->d_frame_off, (void*)k->d_so, (void*)k->d_ent, (void*)k->d_index})
    if (q) (void)hipFree(q);
  if (dev >= 0) (void)hipSetDevice(dev);
  delete k;
}

// A device block of the build's own, freed on every way out (not st_walk: a build may run between a streams call and its result)
struct CorpusBlock {
  void* p = nullptr;
  ~CorpusBlock() { if (p) (void)hipFree(p); }
  template <class Carve> int alloc(x3_ctx* c, Carve carve) {   // carve(base): the pieces, and the bytes they take
    HIPCHK(c, hipMalloc(&p, carve(nullptr)));
    carve((char*)p);
    return X3_OK;
  }
};

// The entries the segmented walk left alone, by x3_index_dev's own path (its phantom bytes with the archive flag) on an
// aligned copy of each: frames (buffer offsets), count and how the walk ends.
static int corpus_general_walk(x3_ctx* c, const uint8_t* d_x3, uint64_t off, uint64_t len, uint64_t phantom,
                               std::vector<uint64_t>* frames, int* terminal) {
  int rc;
  if ((rc = entry_copy(c, d_x3, off, len))) return rc;
  X3IndexSummary r;
  if ((rc = index_all_frames(c, (const uint8_t*)c->st_one.p, len, phantom, 0u, ~0ull, &r))) return rc;
  frames->resize(r.n_frames);
  if (r.n_frames) {
    HIPCHK(c, hipMemcpy(frames->data(), c->frame_off.p, 8 * r.n_frames, hipMemcpyDeviceToHost));
    for (auto& f : *frames) f += off;
  }
  *terminal = r.terminal;
  return X3_OK;
}

// the recording decode: slices of frames into a scratch layout of its own (a frame's samples at a multiple of four), each
// slice's index slots copied into place -- what one recording call over the whole table leaves
#define X3K_RECORD_SCRATCH (256ull << 20)   // bytes of samples one slice decodes into
static int corpus_record(x3_ctx* c, x3_corpus* k, const X3DevParams& dp, uint32_t seg_blocks, CorpusBlock& blk) {
  const uint64_t F = k->F;
  const uint64_t nidx = seg_index_nseg(dp.blocks_per_frame, seg_blocks);
  const uint64_t pitch = ((uint64_t)dp.spf + 3) & ~3ull;
  const uint64_t S = std::min<uint64_t>(F, std::max<uint64_t>(X3K_RECORD_SCRATCH / 2 / pitch, 1));
  int rc;
  int16_t* wav;
  uint64_t *woff, *sidx;
  auto carve = [&](char* base) {
    BlockCarver q{base, 0};
    wav = q.take<int16_t>(S * pitch), woff = q.take<uint64_t>(S), sidx = q.take<uint64_t>(1 + S * (nidx - 1));
    return q.at;
  };
  if ((rc = blk.alloc(c, carve))) return rc;
  std::vector<uint64_t> h(S);
  for (uint64_t i = 0; i < S; ++i) h[i] = i * pitch;
  HIPCHK(c, hipMemcpy(woff, h.data(), 8 * S, hipMemcpyHostToDevice));
  if ((rc = ensure(c, c->dec_status, S * sizeof(int32_t)))) return rc;
  const X3SegSpec seg{sidx, seg_blocks, 2};
  c->last_corpus_slices = 0;
  for (uint64_t f0 = 0; f0 < F; f0 += S) {
    ++c->last_corpus_slices;
    const uint64_t m = std::min<uint64_t>(S, F - f0);
    if ((rc = decode_dev_impl(c, k->d_x3, k->x3_len, k->d_frame_off + f0, m, nullptr, woff, &k->p, wav, m * pitch,
                              (int32_t*)c->dec_status.p, true, false, &seg)))
      return rc;
    if (f0 == 0) HIPCHK(c, hipMemcpyAsync(k->d_index, sidx, 8, hipMemcpyDeviceToDevice, c->stream));   // (the header word)
    HIPCHK(c, hipMemcpyAsync(k->d_index + 1 + f0 * (nidx - 1), sidx + 1, 8 * m * (nidx - 1), hipMemcpyDeviceToDevice, c->stream));
  }
  c->decode_pending = false;   // (the recording's summary is no call's result)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return X3_OK;
}

static int corpus_build_impl(x3_ctx* c, x3_corpus* k, const uint64_t* offsets, const uint64_t* lengths,
                             const std::vector<uint32_t>& span_first, uint64_t phantom, uint32_t seg_blocks, bool index_walk) {
  const uint64_t n = k->n, G = span_first[n], cap = seg_cands(G);
  int rc;
  X3DevParams dp;
  if ((rc = derive_params(&k->p, &dp))) return rc;
  // ---- 1. every entry's frames: the segmented fast walk (x3_streams_kernel.h), all entries at once
  std::vector<unsigned long long> m(n, ~0ull);
  std::vector<int32_t> st(n, 0);
  const bool fast = G && !c->opt.index_no_fast;
  CorpusBlock walk_blk, record_blk;
  SegWalkWs w{};
  unsigned long long *ent_k0 = nullptr, *ent_m = nullptr;   // per entry: its first candidate, its frame count,
  int32_t* ent_st = nullptr;                                // how its walk ends
  if (fast) {
    auto carve = [&](char* base) {   // the walk's workspace, then the build's own words
      BlockCarver q{base, segwalk_carve(base, n, G, &w)};
      ent_k0 = q.take<unsigned long long>(n), ent_m = q.take<unsigned long long>(n), ent_st = q.take<int32_t>(n);
      return q.at;
    };
    if ((rc = walk_blk.alloc(c, carve))) return rc;
    if ((rc = segwalk_launch(c, k->d_x3, k->x3_len, offsets, lengths, span_first, phantom, ~0ull, 0u, w))) return rc;
    hipLaunchKernelGGL(x3_corpus_walk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const uint32_t*>(k->d_x3), k->x3_len, w.eoff, w.elen, w.span_first, (uint32_t)n, phantom,
                       w.base, (uint32_t)G, &w.isum->n_chain, w.ent_flags, w.ent_end, ent_k0, ent_m, ent_st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(m.data(), ent_m, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.data(), ent_st, 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // ---- the entries the fast walk could not vouch for (and, without it, every entry): the general walk, one by one
  k->ent.assign(n, x3_corpus_entry{0, 0, 0, 0, 0});
  std::vector<std::pair<uint64_t, std::vector<uint64_t>>> general;
  uint64_t F = 0;
  for (uint64_t e = 0; e < n; ++e) {
    x3_corpus_entry& en = k->ent[e];
    if (m[e] == ~0ull) {
      std::vector<uint64_t> fr;
      int term = 0;
      if ((rc = corpus_general_walk(c, k->d_x3, offsets[e], lengths[e], phantom, &fr, &term))) return rc;
      en.n_frames = fr.size();
      en.walk_status = term;
      en.general_walk = 1;
      general.emplace_back(e, std::move(fr));
    } else {
      en.n_frames = m[e];
      en.walk_status = st[e];
    }
    en.first_frame = F;
    F += en.n_frames;
    k->max_frames = std::max<uint64_t>(k->max_frames, en.n_frames);
  }
  if (F > 0x7FFFFFFFull) {
    c->last_error = "x3_corpus_build: more than 0x7FFFFFFF frames";
    return X3_ERR_BAD_ARG;
  }
  k->F = F;
  // ---- 2. one frame table, its sample offsets, the entries' sample counts
  HIPCHK(c, hipMalloc(&k->d_frame_off, 8 * std::max<uint64_t>(F, 1)));
  HIPCHK(c, hipMalloc(&k->d_so, 8 * (F + 1)));
  HIPCHK(c, hipMalloc(&k->d_ent, sizeof(x3_corpus_entry) * n));
  HIPCHK(c, hipMemcpyAsync(k->d_ent, k->ent.data(), sizeof(x3_corpus_entry) * n, hipMemcpyHostToDevice, c->stream));
  if (fast && F)
    hipLaunchKernelGGL(x3_corpus_compact_kernel, dim3((unsigned)std::min<uint64_t>((cap + 255) / 256, 4096)), dim3(256), 0,
                       c->stream, w.frame_off, w.fent, cap, &w.isum->n_chain, ent_k0, k->d_ent, F, k->d_frame_off);
  for (const auto& g : general)
    if (!g.second.empty())
      HIPCHK(c, hipMemcpyAsync(k->d_frame_off + k->ent[g.first].first_frame, g.second.data(), 8 * g.second.size(),
                               hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(x3_window_sample_offsets_kernel, dim3(1), dim3(1024), 0, c->stream, k->d_x3, k->x3_len,
                     (const uint64_t*)k->d_frame_off, F, k->d_so);
  hipLaunchKernelGGL(x3_corpus_samples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                     (const uint64_t*)k->d_so, F, k->d_ent, n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(k->ent.data(), k->d_ent, sizeof(x3_corpus_entry) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&k->total, k->d_so + F, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // ---- 3. the segment index: by one walk over the whole frame table for any parameters (X3_CORPUS_INDEX_WALK), or by
  // the recording decode where the parameters route to the decoder that records it
  const uint64_t nidx = F ? seg_index_nseg(dp.blocks_per_frame, seg_blocks) : 1;
  if (nidx >= 2 && (index_walk || decode_route(dp, X3Geom{0, 0, 1, F}, (const int16_t*)nullptr, true, true, 2, c->opt).kernel == X3_DEC_SPLIT)) {
    HIPCHK(c, hipMalloc(&k->d_index, 8 * (1 + F * (nidx - 1))));
    if (index_walk) {
      if ((rc = seg_index_launch(c, k->d_x3, k->x3_len, k->d_frame_off, F, dp, k->d_index, seg_blocks))) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if ((rc = corpus_record(c, k, dp, seg_blocks, record_blk))) {
      return rc;
    }
    k->seg_blocks = seg_blocks;
  }
  return X3_OK;
}

extern "C" int x3_corpus_build(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* offsets, const uint64_t* lengths,
                               uint64_t n, uint32_t flags, const x3_params* p, uint32_t seg_blocks, x3_corpus** out) {
  if (out) *out = nullptr;
  if (!c || !offsets || !lengths || !p || !out || (!d_x3 && x3_len)) return X3_ERR_BAD_ARG;
  if (n == 0 || n > 0xFFFFFFF0ull || (flags & ~(X3_STREAMS_ARCHIVE_FRAMES | X3_CORPUS_INDEX_WALK))) return X3_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(d_x3) & 3u) return X3_ERR_BAD_ARG;
  if (x3_params_validate(p) != X3_OK) return X3_ERR_BAD_ARG;
  if (p->block_len == 0 || p->blocks_per_frame == 0 || spf_of(p) > 0xFFFFFFFFull) return X3_ERR_BAD_ARG;   // (windows refuse them)
  if (seg_blocks && !seg_index_args_ok(nullptr, seg_blocks)) return X3_ERR_BAD_ARG;   // (0: no index; the table is the corpus's own)
  std::vector<uint32_t> span_first;
  uint64_t G = 0, bytes = 0;
  if (seg_entries(offsets, lengths, n, x3_len, &span_first, &G, &bytes)) return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  x3_corpus* k = new x3_corpus;
  k->device = c->device;
  k->d_x3 = d_x3;
  k->x3_len = x3_len;
  k->n = n;
  k->p = *p;
  c->decode_pending = false;
  c->last_corpus_slices = 0;
  const int rc = corpus_build_impl(c, k, offsets, lengths, span_first, (flags & X3_STREAMS_ARCHIVE_FRAMES) ? 8 : 0, seg_blocks,
                                   (flags & X3_CORPUS_INDEX_WALK) != 0);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the build may still run when its buffers go)
    x3_corpus_destroy(k);
    return rc;
  }
  *out = k;
  return X3_OK;
}

extern "C" int x3_corpus_info(const x3_corpus* k, uint64_t* n_entries, uint64_t* n_frames, uint64_t* total_samples,
                              uint32_t* seg_blocks_in_use) {
  if (!k) return X3_ERR_BAD_ARG;
  if (n_entries) *n_entries = k->n;
  if (n_frames) *n_frames = k->F;
  if (total_samples) *total_samples = k->total;
  if (seg_blocks_in_use) *seg_blocks_in_use = k->seg_blocks;
  return X3_OK;
}

extern "C" int x3_corpus_entries(const x3_corpus* k, x3_corpus_entry* out) {
  if (!k || !out) return X3_ERR_BAD_ARG;
  std::memcpy(out, k->ent.data(), sizeof(x3_corpus_entry) * k->n);
  return X3_OK;
}

extern "C" int x3_corpus_entries_dev(const x3_corpus* k, const x3_corpus_entry** d_entries) {
  if (!k || !d_entries) return X3_ERR_BAD_ARG;
  *d_entries = k->d_ent;
  return X3_OK;
}

extern "C" int x3_corpus_seg_index(const x3_corpus* k, const uint64_t** d_seg_index, uint64_t* n_words) {
  if (!k || !d_seg_index || !n_words) return X3_ERR_BAD_ARG;
  *d_seg_index = k->d_index;
  *n_words = k->d_index ? x3_seg_index_entries(k->F, &k->p, k->seg_blocks) : 0;
  return X3_OK;
}

// a corpus of another device is refused in `entry_point`'s name
static bool corpus_device_ok(x3_ctx* c, const x3_corpus* k, const char* entry_point) {
  if (c->device == k->device) return true;
  c->last_error = std::string(entry_point) + ": the corpus was built on another device";
  return false;
}

// The frames of a corpus for a call of this context
static int corpus_source(x3_ctx* c, const x3_corpus* k, const char* entry_point, FrameSource* s) {
  if (!corpus_device_ok(c, k, entry_point)) return X3_ERR_BAD_ARG;
  s->d_x3 = k->d_x3, s->x3_len = k->x3_len;
  s->d_frame_offsets = k->d_frame_off, s->d_sample_offsets = k->d_so, s->F = k->F, s->max_frames = k->max_frames;
  s->spf = spf_of(&k->p);
  const int rc = derive_params(&k->p, &s->dp);
  if (rc == X3_OK) s->index(k->d_index, k->seg_blocks);
  return rc;
}

extern "C" int x3_corpus_windows_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                     uint64_t n_windows, uint32_t window_len, void* d_out, int out_format, int32_t* d_status) {
  if (!c || !k || !d_entries || (reinterpret_cast<uintptr_t>(d_entries) & 3u)) return X3_ERR_BAD_ARG;
  if (!windows_args_ok(n_windows, window_len, d_out, out_format, d_starts, d_status)) return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = corpus_source(c, k, "x3_corpus_windows_dev", &s);
  if (rc) return rc;
  return windows_launch(c, s, n_windows, window_len, nullptr, d_out, out_format, d_status,
                        [&](dim3 grid, X3WinPlan* plan, uint64_t* gstart, X3WinSummary* sum) -> const uint64_t* {
                          hipLaunchKernelGGL(x3_corpus_plan_kernel, grid, dim3(256), 0, c->stream,
                                             k->d_ent, k->n, s.d_sample_offsets, s.F, d_entries,
                                             d_starts, n_windows, window_len, plan, gstart, sum);
                          return gstart;
                        });
}

extern "C" int x3_corpus_ranges_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                    const uint32_t* d_lens, uint64_t n_ranges, uint64_t row_stride, void* d_out,
                                    uint64_t out_cap, int out_format, uint64_t* d_out_offsets, int32_t* d_status) {
  if (!c || !k || !d_entries || (reinterpret_cast<uintptr_t>(d_entries) & 3u)) return X3_ERR_BAD_ARG;
  if (!ranges_args_ok(c, n_ranges, d_lens, row_stride, d_out, out_cap, out_format, d_starts, d_out_offsets, d_status))
    return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = corpus_source(c, k, "x3_corpus_ranges_dev", &s);
  if (rc) return rc;
  const RangeRows rows{d_lens, row_stride, out_cap, d_out_offsets};
  return windows_launch(c, s, n_ranges, 0, &rows, d_out, out_format, d_status,
                        [&](dim3 grid, X3WinPlan* plan, uint64_t* gstart, X3WinSummary* sum) -> const uint64_t* {
                          hipLaunchKernelGGL(x3_corpus_range_plan_kernel, grid, dim3(256), 0, c->stream,
                                             k->d_ent, k->n, s.d_sample_offsets, s.F, d_entries,
                                             d_starts, d_lens, n_ranges, plan, gstart, sum);
                          return gstart;
                        });
}

// the rows of entry e (levels_rows_of its samples) in front of each other, n_entries + 1 words to row_first if it is given;
// their sum
static uint64_t corpus_rows_total(const x3_corpus* k, uint64_t bin_len, uint64_t* row_first = nullptr) {
  uint64_t run = 0;
  for (uint64_t e = 0; e < k->n; ++e) {
    if (row_first) row_first[e] = run;
    run += levels_rows_of(k->ent[e].n_samples, bin_len);
  }
  if (row_first) row_first[k->n] = run;
  return run;
}

extern "C" int x3_corpus_levels_rows(const x3_corpus* k, uint64_t bin_len, uint64_t* row_first) {
  if (!k || !row_first) return X3_ERR_BAD_ARG;
  corpus_rows_total(k, bin_len, row_first);
  return X3_OK;
}

// The level records a call reads or writes (X3EvRows, x3_events_kernel.h), FrameSource's counterpart: what every such call
// checks behind its own arguments.  A stream's: one entry, its samples in *d_total on the device.
static int stream_rows(const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total, X3EvRows* q) {
  if (!d_total || (reinterpret_cast<uintptr_t>(d_total) & 7u)) return X3_ERR_BAD_ARG;
  *q = X3EvRows{d_levels, n_bins, bin_len, d_total, nullptr, 0, nullptr};
  return X3_OK;
}

// ... a corpus's, entry after entry: the corpus is this device's, n_rows is what the host's entry table gives (row_first:
// corpus_row_prefix, in the call's workspace)
static int corpus_rows(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len,
                       const char* entry_point, X3EvRows* q) {
  if (!corpus_device_ok(c, k, entry_point) || n_rows != corpus_rows_total(k, bin_len)) return X3_ERR_BAD_ARG;
  *q = X3EvRows{d_levels, n_rows, bin_len, nullptr, k->d_ent, k->n, nullptr};
  return X3_OK;
}

// ... of either: corpus_entry is the entry point's name of a corpus form (k), NULL for a stream form (d_total)
static int rows_of(x3_ctx* c, const x3_corpus* k, const char* corpus_entry, const x3_level* d_levels, uint64_t n_rows,
                   uint64_t bin_len, const uint64_t* d_total, X3EvRows* q) {
  return corpus_entry ? corpus_rows(c, k, d_levels, n_rows, bin_len, corpus_entry, q) : stream_rows(d_levels, n_rows, bin_len, d_total, q);
}

// the row prefix of a corpus call (k != NULL) by the device into its workspace, and into the call's rows
static void corpus_row_prefix(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, unsigned long long* row_first, X3EvRows* q = nullptr) {
  if (!k) return;
  hipLaunchKernelGGL(x3_corpus_levels_rows_kernel, dim3(1), dim3(1024), 0, c->stream, k->d_ent, k->n, bin_len, row_first);
  if (q) q->row_first = row_first;
}

static int corpus_levels_call(x3_ctx* c, const x3_corpus* k, const char* entry, uint64_t bin_len, x3_level* d_levels,
                              uint64_t n_rows, int32_t* d_frame_status, const LevSignal& g) {
  if (!c || !k || !levels_args_ok(c, d_levels, n_rows, d_frame_status) || !levels_planes_ok(g, n_rows)) return X3_ERR_BAD_ARG;
  FrameSource s;
  X3EvRows q;
  int rc;
  if ((rc = corpus_source(c, k, entry, &s))) return rc;
  if ((rc = corpus_rows(c, k, d_levels, n_rows, bin_len, entry, &q))) return rc;
  return levels_launch(c, s, bin_len, d_levels, n_rows, d_frame_status, k->n, g,
                       [&](dim3 grid, unsigned long long* row_first, const int32_t* fst, X3LevFrame* frames, uint32_t* cnt) {
                         corpus_row_prefix(c, k, bin_len, row_first);
                         hipLaunchKernelGGL(x3_corpus_levels_prep_kernel, grid, dim3(256), 0, c->stream,
                                            k->d_ent, k->n, (const unsigned long long*)row_first,
                                            s.d_sample_offsets, s.F, bin_len, n_rows, fst, frames, cnt);
                       });
}

extern "C" int x3_corpus_levels_dev(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                                    int32_t* d_frame_status) {
  return corpus_levels_call(c, k, "x3_corpus_levels_dev", bin_len, d_levels, n_rows, d_frame_status,
                            LevSignal(X3_LEVEL_SIGNAL_SAMPLES));
}

extern "C" int x3_corpus_signal_levels_dev(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                                           int32_t* d_frame_status, int signal) {
  if (!c || !levels_signal_ok(signal)) return X3_ERR_BAD_ARG;
  return corpus_levels_call(c, k, "x3_corpus_signal_levels_dev", bin_len, d_levels, n_rows, d_frame_status, LevSignal(signal));
}

extern "C" int x3_corpus_fir_levels_dev(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                                        int32_t* d_frame_status, const x3_level_fir* fir) {
  X3FirTaps taps;
  if (!c || !levels_fir_taps(fir, &taps)) return X3_ERR_BAD_ARG;
  return corpus_levels_call(c, k, "x3_corpus_fir_levels_dev", bin_len, d_levels, n_rows, d_frame_status, LevSignal(taps));
}

extern "C" int x3_corpus_tone_levels_dev(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_rows,
                                         int32_t* d_frame_status, const x3_level_tone* tone) {
  X3LevToneTail t;
  if (!c || !levels_tone_arg(tone, &t)) return X3_ERR_BAD_ARG;
  return corpus_levels_call(c, k, "x3_corpus_tone_levels_dev", bin_len, reinterpret_cast<x3_level*>(d_levels), n_rows,
                            d_frame_status, LevSignal(t));
}

extern "C" int x3_corpus_tone_bank_levels_dev(x3_ctx* c, const x3_corpus* k, uint64_t bin_len, x3_tone_level* d_levels,
                                              uint64_t n_rows, int32_t* d_frame_status, const x3_level_tone_bank* bank) {
  X3LevToneBankTail t;
  if (!c || !levels_tone_bank_arg(bank, &t)) return X3_ERR_BAD_ARG;
  return corpus_levels_call(c, k, "x3_corpus_tone_bank_levels_dev", bin_len, reinterpret_cast<x3_level*>(d_levels), n_rows,
                            d_frame_status, LevSignal(t));
}

// ------------------------------------------------------------------------------------------------
// events: runs of loud bins of level records as ranges (x3_events_kernel.h)
// ------------------------------------------------------------------------------------------------
static_assert(X3E_TILE == X3_EVENTS_TILE_ROWS, "the option \"events_tile_rows\" reports the kernels' tile");

// The workspace (EvWs, x3_internal.h): a byte per row; four words per tile; the run tables and the scan of their pieces (a
// row starts at most one run); the summary; a corpus's row prefix
size_t events_carve(char* base, uint64_t n_rows, uint64_t n_ent, EvWs* w) {
  BlockCarver k{base, 0};
  const uint64_t n_tiles = (n_rows + X3E_TILE - 1) / X3E_TILE;
  w->hot = k.take<uint8_t>(n_rows);
  w->tile_prev = k.take<uint32_t>(n_tiles);
  w->tile_next = k.take<uint32_t>(n_tiles);
  w->tile_ns = k.take<uint32_t>(n_tiles);
  w->tile_ne = k.take<uint32_t>(n_tiles);
  w->run_first = k.take<uint32_t>(n_rows);
  w->run_last = k.take<uint32_t>(n_rows);
  w->piece_off = k.take<unsigned long long>(n_rows + 1);
  w->sum = k.take<X3EvSummary>(1);
  w->row_first = k.take<unsigned long long>(n_ent + 1, 1);
  return k.at;
}

// The verdict of an events call with its four run values, checked, as the kernels take it (X3EvPlanes; LevSignal's
// counterpart): built at the entry point from the caller's rule, each constructor with the checks of its rule alone.  The
// run values' checks need bin_len, the planes' n_rows; ok stays false where anything is refused.
struct EvVerdict {
  X3EvPlanes pl{};   // (the values behind n_planes stay 0: never read)
  bool ok = false;

  // an x3_event_rule is one plane, needed, at the stride n_rows: plain (its own two values, not both 0, within their
  // limits) or adaptive (no values of its own; d_thr per entry)
  EvVerdict(const x3_event_rule* rule, bool adaptive, const x3_event_threshold* d_thr, uint64_t n_rows, uint64_t bin_len) {
    if (!rule || rule->reserved || !runs(rule->join_bins, rule->min_bins, rule->pad_bins, rule->max_bins, bin_len)) return;
    if (adaptive ? (rule->mean_sq_min != 0 || rule->peak_min != 0 || !thr(d_thr))
                 : ((rule->mean_sq_min == 0 && rule->peak_min == 0) || !values(rule->mean_sq_min, rule->peak_min)))
      return;
    pl.rule.n_planes = pl.rule.min_planes = 1;
    pl.rule.mean_sq_min[0] = rule->mean_sq_min;
    pl.rule.peak_min[0] = rule->peak_min;
    pl.stride = n_rows;
    ok = true;
  }

  // an x3_plane_event_rule: 1 .. 8 planes at plane_stride >= n_rows (n_rows' own limit: t * plane_stride + r stays below
  // 2^34 records, 2^39 bytes); min_planes of them `on` with the rule's values, or none with d_thr's
  EvVerdict(const x3_plane_event_rule* rule, const x3_event_threshold* d_thr, uint64_t plane_stride, uint64_t n_rows, uint64_t bin_len) {
    if (!rule || rule->reserved[0] || rule->reserved[1] ||
        !runs(rule->join_bins, rule->min_bins, rule->pad_bins, rule->max_bins, bin_len))
      return;
    if (rule->n_planes == 0 || rule->n_planes > X3_EVENT_PLANES_MAX || rule->min_planes == 0 || rule->min_planes > rule->n_planes ||
        plane_stride < n_rows || plane_stride > 0x7FFFFFFFull)
      return;
    uint32_t on = 0;
    for (uint32_t t = 0; t < rule->n_planes; ++t) {
      if (!values(rule->mean_sq_min[t], rule->peak_min[t])) return;
      on += (rule->mean_sq_min[t] || rule->peak_min[t]) ? 1u : 0u;
      pl.rule.mean_sq_min[t] = rule->mean_sq_min[t];
      pl.rule.peak_min[t] = rule->peak_min[t];
    }
    if (d_thr ? (on != 0 || !thr(d_thr)) : on < rule->min_planes) return;
    pl.rule.n_planes = rule->n_planes;
    pl.rule.min_planes = rule->min_planes;
    pl.stride = plane_stride;
    ok = true;
  }

  // what the five kernels between flag and emit take of it
  x3_event_rule run_rule() const { return x3_event_rule{0, 0, pl.rule.join_bins, pl.rule.min_bins, pl.rule.pad_bins, pl.rule.max_bins, 0}; }

 private:
  bool runs(uint32_t join_bins, uint32_t min_bins, uint32_t pad_bins, uint32_t max_bins, uint64_t bin_len) {
    if (bin_len == 0 || bin_len > 0xFFFFFFFFull || 2ull * pad_bins > join_bins || (uint64_t)max_bins * bin_len > 0xFFFFFFFFull) return false;
    pl.rule.join_bins = join_bins;
    pl.rule.min_bins = min_bins;
    pl.rule.pad_bins = pad_bins;
    pl.rule.max_bins = max_bins ? max_bins : (uint32_t)(0xFFFFFFFFull / bin_len);   // (never 0)
    return true;
  }
  static bool values(uint64_t mean_sq_min, uint32_t peak_min) { return mean_sq_min <= X3E_MEAN_SQ_MAX && peak_min <= X3E_PEAK_MAX; }
  bool thr(const x3_event_threshold* d_thr) {
    pl.thr = d_thr;
    return d_thr && !(reinterpret_cast<uintptr_t>(d_thr) & 7u);
  }
};

// The outputs of an events call: cap slots each (d_event_levels: per plane); d_entries of a corpus form alone; the mask
// and the event levels may be NULL
struct EvOut {
  uint32_t* d_entries;
  uint64_t* d_starts;
  uint32_t* d_lens;
  uint32_t* d_event_planes;
  x3_level* d_event_levels;
  uint64_t cap;
  uint64_t* d_count;
  bool ok(bool corpus) const {
    if (!d_starts || !d_lens || !d_count || (corpus && !d_entries) || cap == 0 || cap > 0x7FFFFFFFull) return false;
    const uintptr_t p8 = reinterpret_cast<uintptr_t>(d_starts) | reinterpret_cast<uintptr_t>(d_event_levels) |
                         reinterpret_cast<uintptr_t>(d_count);
    const uintptr_t p4 = reinterpret_cast<uintptr_t>(d_entries) | reinterpret_cast<uintptr_t>(d_lens) |
                         reinterpret_cast<uintptr_t>(d_event_planes);
    return !(p8 & 7u) && !(p4 & 3u);
  }
};

// The launch set of an events call.  q: the rows (its row_first is set here); k: the corpus of a corpus call, whose row
// prefix the levels' kernel computes into the workspace first.  The verdict picks the flag instance -- the values' source
// and the bound of the plane loop -- and the emit kernel; the five in between work on the hot bytes and the tile words,
// whatever made them, and take the four run values alone.
static int events_launch(x3_ctx* c, X3EvRows q, const x3_corpus* k, const EvVerdict& v, const EvOut& o) {
  using Flag = void (*)(X3EvRows, X3EvPlanes, uint64_t, uint8_t*, uint32_t*, uint32_t*);
  static const Flag flag[2][2] = {   // [the values are d_thr's][more planes than one]
      {x3_events_flag_kernel<false, 1>, x3_events_flag_kernel<false, X3_EVENT_PLANES_MAX>},
      {x3_events_flag_kernel<true, 1>, x3_events_flag_kernel<true, X3_EVENT_PLANES_MAX>}};
  HIPCHK(c, hipSetDevice(c->device));
  EvWs w;
  int rc;
  if ((rc = ensure(c, c->ev_ws, events_carve(nullptr, q.n_rows, q.n_ent, &w)))) return rc;
  events_carve((char*)c->ev_ws.p, q.n_rows, q.n_ent, &w);
  const uint64_t n_tiles = (q.n_rows + X3E_TILE - 1) / X3E_TILE;
  const dim3 g_tiles(grid_for(n_tiles, 1));
  const X3EvPlanes& pl = v.pl;
  const x3_event_rule rule = v.run_rule();
  const bool planes = pl.rule.n_planes > 1;
  corpus_row_prefix(c, k, q.bin_len, w.row_first, &q);
  hipLaunchKernelGGL(flag[pl.thr != nullptr][planes], g_tiles, dim3(256), 0, c->stream, q, pl, n_tiles, w.hot, w.tile_prev,
                     w.tile_next);
  hipLaunchKernelGGL(x3_events_near_kernel, dim3(1), dim3(1024), 0, c->stream, n_tiles, w.tile_prev, w.tile_next);
  hipLaunchKernelGGL(x3_events_mark_kernel, g_tiles, dim3(256), 0, c->stream, q, rule.join_bins, n_tiles, w.hot,
                     (const uint32_t*)w.tile_prev, (const uint32_t*)w.tile_next, w.tile_ns, w.tile_ne);
  hipLaunchKernelGGL(x3_events_count_kernel, dim3(1), dim3(1024), 0, c->stream, n_tiles, w.tile_ns, w.tile_ne, w.sum);
  hipLaunchKernelGGL(x3_events_table_kernel, g_tiles, dim3(256), 0, c->stream, q.n_rows, n_tiles, (const uint8_t*)w.hot,
                     (const uint32_t*)w.tile_ns, (const uint32_t*)w.tile_ne, w.run_first, w.run_last);
  hipLaunchKernelGGL(x3_events_runs_kernel, dim3(1), dim3(1024), 0, c->stream, q, rule, w.run_first, w.run_last, w.piece_off, w.sum,
                     o.d_count);
  // (the count is on the device: a wave per slot of the caller's arrays at most, grid-stride.  One plane and no mask: the
  // emit kernel that tests no record)
  if (planes || o.d_event_planes)
    hipLaunchKernelGGL(x3_plane_events_emit_kernel, dim3(grid_for(o.cap, 4)), dim3(256), 0, c->stream, q, pl,
                       (const uint32_t*)w.run_first, (const uint32_t*)w.run_last, (const unsigned long long*)w.piece_off,
                       (const X3EvSummary*)w.sum, o.cap, o.d_entries, o.d_starts, o.d_lens, o.d_event_planes, o.d_event_levels);
  else
    hipLaunchKernelGGL(x3_events_emit_kernel, dim3(grid_for(o.cap, 4)), dim3(256), 0, c->stream, q, rule, (const uint32_t*)w.run_first,
                       (const uint32_t*)w.run_last, (const unsigned long long*)w.piece_off, (const X3EvSummary*)w.sum, o.cap,
                       o.d_entries, o.d_starts, o.d_lens, o.d_event_levels);
  HIPCHK(c, hipGetLastError());
  c->events.pending = true;
  c->events.count = o.cap;
  c->events.sum_off = (size_t)((char*)w.sum - (char*)c->ev_ws.p);
  return X3_OK;
}

// One checked events call: the verdict and the outputs as the entry point has built them.  corpus_entry: the entry
// point's name of a corpus form (k, o.d_entries), NULL for a stream form (d_total).
static int events_call(x3_ctx* c, const x3_corpus* k, const char* corpus_entry, const x3_level* d_levels, uint64_t n_rows,
                       uint64_t bin_len, const uint64_t* d_total, const EvVerdict& v, const EvOut& o) {
  if (!c || c->capturing || (corpus_entry && !k) || !d_levels || (reinterpret_cast<uintptr_t>(d_levels) & 7u)) return X3_ERR_BAD_ARG;
  if (n_rows == 0 || n_rows > 0x7FFFFFFFull || !v.ok || !o.ok(corpus_entry != nullptr)) return X3_ERR_BAD_ARG;
  X3EvRows q;
  const int rc = rows_of(c, k, corpus_entry, d_levels, n_rows, bin_len, d_total, &q);
  if (rc) return rc;
  return events_launch(c, q, k, v, o);
}

extern "C" int x3_events_dev(x3_ctx* c, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                             const x3_event_rule* rule, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels,
                             uint64_t cap, uint64_t* d_count) {
  return events_call(c, nullptr, nullptr, d_levels, n_bins, bin_len, d_total, EvVerdict(rule, false, nullptr, n_bins, bin_len),
                     EvOut{nullptr, d_starts, d_lens, nullptr, d_event_levels, cap, d_count});
}

extern "C" int x3_corpus_events_dev(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len,
                                    const x3_event_rule* rule, uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens,
                                    x3_level* d_event_levels, uint64_t cap, uint64_t* d_count) {
  return events_call(c, k, "x3_corpus_events_dev", d_levels, n_rows, bin_len, nullptr, EvVerdict(rule, false, nullptr, n_rows, bin_len),
                     EvOut{d_entries, d_starts, d_lens, nullptr, d_event_levels, cap, d_count});
}

extern "C" int x3_events_adaptive_dev(x3_ctx* c, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                                      const x3_event_rule* rule, const x3_event_threshold* d_thr, uint64_t* d_starts,
                                      uint32_t* d_lens, x3_level* d_event_levels, uint64_t cap, uint64_t* d_count) {
  return events_call(c, nullptr, nullptr, d_levels, n_bins, bin_len, d_total, EvVerdict(rule, true, d_thr, n_bins, bin_len),
                     EvOut{nullptr, d_starts, d_lens, nullptr, d_event_levels, cap, d_count});
}

extern "C" int x3_corpus_events_adaptive_dev(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t n_rows,
                                             uint64_t bin_len, const x3_event_rule* rule, const x3_event_threshold* d_thr,
                                             uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels,
                                             uint64_t cap, uint64_t* d_count) {
  return events_call(c, k, "x3_corpus_events_adaptive_dev", d_levels, n_rows, bin_len, nullptr,
                     EvVerdict(rule, true, d_thr, n_rows, bin_len), EvOut{d_entries, d_starts, d_lens, nullptr, d_event_levels, cap, d_count});
}

// plane events: the same call on K planes of records
static_assert(sizeof(x3_plane_event_rule) == 128 && offsetof(x3_plane_event_rule, min_planes) == 4 &&
                  offsetof(x3_plane_event_rule, join_bins) == 8 && offsetof(x3_plane_event_rule, max_bins) == 20 &&
                  offsetof(x3_plane_event_rule, reserved) == 24 && offsetof(x3_plane_event_rule, mean_sq_min) == 32 &&
                  offsetof(x3_plane_event_rule, peak_min) == 96,
              "include/x3hip.h states this layout");

extern "C" int x3_plane_events_dev(x3_ctx* c, const x3_level* d_levels, uint64_t plane_stride, uint64_t n_bins, uint64_t bin_len,
                                   const uint64_t* d_total, const x3_plane_event_rule* rule, const x3_event_threshold* d_thr,
                                   uint64_t* d_starts, uint32_t* d_lens, uint32_t* d_event_planes, x3_level* d_event_levels,
                                   uint64_t cap, uint64_t* d_count) {
  return events_call(c, nullptr, nullptr, d_levels, n_bins, bin_len, d_total, EvVerdict(rule, d_thr, plane_stride, n_bins, bin_len),
                     EvOut{nullptr, d_starts, d_lens, d_event_planes, d_event_levels, cap, d_count});
}

extern "C" int x3_corpus_plane_events_dev(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t plane_stride,
                                          uint64_t n_rows, uint64_t bin_len, const x3_plane_event_rule* rule,
                                          const x3_event_threshold* d_thr, uint32_t* d_entries, uint64_t* d_starts,
                                          uint32_t* d_lens, uint32_t* d_event_planes, x3_level* d_event_levels, uint64_t cap,
                                          uint64_t* d_count) {
  return events_call(c, k, "x3_corpus_plane_events_dev", d_levels, n_rows, bin_len, nullptr,
                     EvVerdict(rule, d_thr, plane_stride, n_rows, bin_len),
                     EvOut{d_entries, d_starts, d_lens, d_event_planes, d_event_levels, cap, d_count});
}

extern "C" int x3_events_result(x3_ctx* c, uint64_t* count) {
  if (!c) return X3_ERR_BAD_ARG;
  X3EvSummary h{0, 0};
  const int rc = pending_fetch(c, c->events, c->ev_ws, &h, sizeof h);
  if (rc) return rc;
  if (count) *count = h.count;
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// level quantiles, thresholds from them, events with a threshold per entry (x3_quantiles_kernel.h)
// ------------------------------------------------------------------------------------------------
static_assert(X3Q_BINS == X3E_TILE, "a lane of a tile flushes one bin of the tile's histogram");
static_assert(sizeof(x3_threshold_rule) == 32 && sizeof(x3_event_threshold) == 16, "include/x3hip.h states these sizes");

// The workspace of a quantiles or thresholds call (QWs, x3_internal.h; the formula: x3_quantiles_kernel.h)
size_t quantiles_carve(char* base, uint64_t n_rows, uint64_t n_ent, uint32_t n_q, QWs* w) {
  BlockCarver k{base, 0};
  w->keys = k.take<uint2>(n_rows);
  w->hist = k.take<uint32_t>(n_ent * n_q * X3Q_BINS);
  w->slots = k.take<X3QSlot>(n_ent * n_q);
  w->val[0] = k.take<uint32_t>(n_ent);
  w->val[1] = k.take<uint32_t>(n_ent);
  w->counted = k.take<uint32_t>(n_ent);
  w->sum = k.take<X3QSummary>(1);
  w->row_first = k.take<unsigned long long>(n_ent + 1, 1);
  return k.at;
}

// the argument checks the quantiles and thresholds calls share
static bool quantiles_args_ok(const x3_ctx* c, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len) {
  if (!c || !d_levels || c->capturing) return false;
  if (bin_len == 0 || bin_len > 0xFFFFFFFFull || n_rows == 0 || n_rows > 0x7FFFFFFFull) return false;
  return (reinterpret_cast<uintptr_t>(d_levels) & 7u) == 0;
}

// One select: the n_q quantiles `ppm` of key `key` of every entry into values (n_ent * n_q words), K into counted
struct QRun { int key; uint32_t n_q; X3QPpm ppm; uint32_t* values; };

// The launch set of a quantiles call (runs[0], into the caller's arrays) or a thresholds call (one run per criterion that
// is on, into the workspace, then the map into d_thr).  q, k: as in events_launch.
static int quantiles_launch(x3_ctx* c, X3EvRows q, const x3_corpus* k, QRun* runs, uint32_t n_runs, uint32_t* d_counted,
                            const x3_threshold_rule* trule, x3_event_threshold* d_thr) {
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t n_ent = k ? k->n : 1u;
  const uint32_t n_q = runs[0].n_q;   // (a thresholds call: 1 in every run)
  QWs w;
  int rc;
  if ((rc = ensure(c, c->q_ws, quantiles_carve(nullptr, q.n_rows, n_ent, n_q, &w)))) return rc;
  quantiles_carve((char*)c->q_ws.p, q.n_rows, n_ent, n_q, &w);
  const uint64_t n_tiles = (q.n_rows + X3E_TILE - 1) / X3E_TILE;
  const dim3 g_rows(grid_for(q.n_rows, 256)), g_tiles(grid_for(n_tiles, 1)), g_ent(grid_for(n_ent, 1));
  corpus_row_prefix(c, k, q.bin_len, w.row_first, &q);
  uint32_t* const counted = trule ? w.counted : d_counted;
  for (uint32_t i = 0; i < n_runs; ++i) {
    const QRun& r = runs[i];
    const uint32_t passes = r.key == X3_LEVEL_KEY_PEAK ? 2u : 4u;
    uint32_t* const values = trule ? w.val[i] : r.values;
    X3QSummary* const sum = i ? nullptr : w.sum;   // (K is the same in every run: entries without rows are counted once)
    HIPCHK(c, hipMemsetAsync(w.hist, 0, (size_t)(n_ent * n_q * X3Q_BINS) * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(x3_quantiles_key_kernel, g_rows, dim3(256), 0, c->stream, q, r.key, w.keys, sum);
    for (uint32_t pass = 0; pass < passes; ++pass) {
      hipLaunchKernelGGL(x3_quantiles_hist_kernel, g_tiles, dim3(256), 0, c->stream, (const uint2*)w.keys, q.n_rows, n_tiles,
                         n_ent, n_q, pass, passes, (const X3QSlot*)w.slots, w.hist);
      hipLaunchKernelGGL(x3_quantiles_select_kernel, g_ent, dim3(64u * n_q), 0, c->stream, n_ent, n_q, r.ppm, pass, passes,
                         w.hist, w.slots, values, counted, sum);
    }
  }
  if (trule) {
    // (a criterion that is off has no run: its value is not read)
    const uint32_t* const vp = trule->peak_div ? w.val[0] : nullptr;
    const uint32_t* const vm = trule->mean_sq_div ? w.val[trule->peak_div ? 1 : 0] : nullptr;
    hipLaunchKernelGGL(x3_quantiles_map_kernel, dim3(grid_for(n_ent, 256)), dim3(256), 0, c->stream, n_ent, *trule, vp, vm,
                       (const uint32_t*)w.counted, d_thr);
  }
  HIPCHK(c, hipGetLastError());
  c->quantiles.pending = true;
  c->quantiles.count = n_ent;
  c->quantiles.sum_off = (size_t)((char*)w.sum - (char*)c->q_ws.p);
  return X3_OK;
}

static bool quantiles_run_ok(int key, const uint32_t* q_ppm, uint32_t n_q, uint32_t* d_values, uint32_t* d_counted, QRun* r) {
  if ((key != X3_LEVEL_KEY_PEAK && key != X3_LEVEL_KEY_MEAN_SQ) || !q_ppm || n_q == 0 || n_q > X3Q_MAX_Q) return false;
  if (!d_values || !d_counted || ((reinterpret_cast<uintptr_t>(d_values) | reinterpret_cast<uintptr_t>(d_counted)) & 3u)) return false;
  *r = QRun{key, n_q, {}, d_values};
  for (uint32_t j = 0; j < n_q; ++j) {
    if (q_ppm[j] > 1000000u) return false;
    r->ppm.v[j] = q_ppm[j];
  }
  return true;
}

// One checked quantiles (n_runs 1, into the caller's arrays) or thresholds call (trule, d_thr).  corpus_entry: as in
// events_call; n_runs 0: the wrapper has refused its runs.
static int quantiles_call(x3_ctx* c, const x3_corpus* k, const char* corpus_entry, const x3_level* d_levels, uint64_t n_rows,
                          uint64_t bin_len, const uint64_t* d_total, QRun* runs, uint32_t n_runs, uint32_t* d_counted,
                          const x3_threshold_rule* trule, x3_event_threshold* d_thr) {
  if ((corpus_entry && !k) || !quantiles_args_ok(c, d_levels, n_rows, bin_len) || !n_runs) return X3_ERR_BAD_ARG;
  X3EvRows q;
  const int rc = rows_of(c, k, corpus_entry, d_levels, n_rows, bin_len, d_total, &q);
  if (rc) return rc;
  return quantiles_launch(c, q, k, runs, n_runs, d_counted, trule, d_thr);
}

extern "C" int x3_level_quantiles_dev(x3_ctx* c, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                                      int key, const uint32_t* q_ppm, uint32_t n_q, uint32_t* d_values, uint32_t* d_counted) {
  QRun r;
  const uint32_t n = quantiles_run_ok(key, q_ppm, n_q, d_values, d_counted, &r) ? 1u : 0u;
  return quantiles_call(c, nullptr, nullptr, d_levels, n_bins, bin_len, d_total, &r, n, d_counted, nullptr, nullptr);
}

extern "C" int x3_corpus_level_quantiles_dev(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t n_rows,
                                             uint64_t bin_len, int key, const uint32_t* q_ppm, uint32_t n_q, uint32_t* d_values,
                                             uint32_t* d_counted) {
  QRun r;
  const uint32_t n = quantiles_run_ok(key, q_ppm, n_q, d_values, d_counted, &r) ? 1u : 0u;
  return quantiles_call(c, k, "x3_corpus_level_quantiles_dev", d_levels, n_rows, bin_len, nullptr, &r, n, d_counted, nullptr, nullptr);
}

// the runs of a thresholds call: one per criterion that is on, the peak's first; 0: refused
static uint32_t threshold_runs(const x3_threshold_rule* rule, const x3_event_threshold* d_thr, QRun runs[2]) {
  if (!rule || !d_thr || (reinterpret_cast<uintptr_t>(d_thr) & 7u)) return 0;
  uint32_t n = 0;
  if (rule->peak_div) {
    if (rule->peak_q_ppm > 1000000u) return 0;
    runs[n] = QRun{X3_LEVEL_KEY_PEAK, 1u, {}, nullptr};
    runs[n++].ppm.v[0] = rule->peak_q_ppm;
  }
  if (rule->mean_sq_div) {
    if (rule->mean_sq_q_ppm > 1000000u) return 0;
    runs[n] = QRun{X3_LEVEL_KEY_MEAN_SQ, 1u, {}, nullptr};
    runs[n++].ppm.v[0] = rule->mean_sq_q_ppm;
  }
  return n;
}

extern "C" int x3_level_thresholds_dev(x3_ctx* c, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                                       const x3_threshold_rule* rule, x3_event_threshold* d_thr) {
  QRun runs[2];
  const uint32_t n = threshold_runs(rule, d_thr, runs);
  return quantiles_call(c, nullptr, nullptr, d_levels, n_bins, bin_len, d_total, runs, n, nullptr, rule, d_thr);
}

extern "C" int x3_corpus_level_thresholds_dev(x3_ctx* c, const x3_corpus* k, const x3_level* d_levels, uint64_t n_rows,
                                              uint64_t bin_len, const x3_threshold_rule* rule, x3_event_threshold* d_thr) {
  QRun runs[2];
  const uint32_t n = threshold_runs(rule, d_thr, runs);
  return quantiles_call(c, k, "x3_corpus_level_thresholds_dev", d_levels, n_rows, bin_len, nullptr, runs, n, nullptr, rule, d_thr);
}

extern "C" int x3_level_quantiles_result(x3_ctx* c, uint64_t* n_empty, uint64_t* first_empty) {
  if (!c) return X3_ERR_BAD_ARG;
  X3QSummary h{0, 0};
  const uint64_t n_ent = c->quantiles.count;
  const int rc = pending_fetch(c, c->quantiles, c->q_ws, &h, sizeof h);
  if (rc) return rc;
  if (n_empty) *n_empty = h.n_empty;
  if (first_empty) *first_empty = h.n_empty ? h.first_empty : n_ent;
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// range levels: the level records of (entry, start, len) ranges (x3_range_levels_kernel.h)
// ------------------------------------------------------------------------------------------------
// the argument checks x3_range_levels_dev and x3_corpus_range_levels_dev share
static bool range_levels_args_ok(const x3_ctx* c, const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges,
                                 uint64_t row_stride, const x3_level* d_levels, uint64_t rows_cap, const uint64_t* d_row_offsets,
                                 const int32_t* d_status) {
  if (!d_starts || !d_lens || !d_levels || !d_status || c->capturing) return false;
  if (n_ranges == 0 || n_ranges > 0x7FFFFFFFull || rows_cap == 0 || rows_cap > 0x7FFFFFFFull) return false;
  if (row_stride ? row_stride > rows_cap / n_ranges : !d_row_offsets) return false;
  return ((reinterpret_cast<uintptr_t>(d_starts) | reinterpret_cast<uintptr_t>(d_levels) | reinterpret_cast<uintptr_t>(d_row_offsets)) & 7u) == 0 &&
         ((reinterpret_cast<uintptr_t>(d_lens) | reinterpret_cast<uintptr_t>(d_status)) & 3u) == 0;
}

// The pairs (range, covering frame) the workspace holds: all a call can have, or four times what disjoint ranges need
// (n_frames + n_ranges: sliding windows with up to 75 % overlap fit).  Pairs beyond it are the fix-up's: time, not results.
// lead_frames (1: X3_LEVEL_SIGNAL_DIFF; T - 1 <= 7: the FIR calls): a range may have that many more pairs, its lead frames
// -- frames of the same stream or entry, so n * max_frames still holds them all.
uint64_t range_levels_pairs(uint64_t n, uint64_t F, uint64_t max_frames, uint64_t lead_frames) {
  return std::min<uint64_t>(n * max_frames, 4 * (F + n) + lead_frames * n);   // (n < 2^31, max_frames <= F < 2^31: no wrap)
}

// The workspace (RLevWs, x3_internal.h): per range the plan, the two scans, the rows that have room, the plan's starts; per
// frame the verdicts; per pair its cut, the scan of the bin counts; the partial rows; replay scratch; the summary; diff
// (X3_LEVEL_SIGNAL_DIFF, and the FIR calls) only, behind it: per frame its last sample, per range its plan's lead frames
size_t range_levels_carve(char* base, uint64_t n, uint64_t F, uint64_t P, uint64_t rows_cap, uint64_t fix_waves,
                          uint32_t scratch_per, RLevWs* w, bool diff, uint64_t planes) {
  BlockCarver k{base, 0};
  w->plan = k.take<X3WinPlan>(n);
  w->cov_off = k.take<unsigned long long>(n + 1);
  w->row_off = k.take<unsigned long long>(n + 1);
  w->erows = k.take<uint32_t>(n);
  w->gstart = k.take<uint64_t>(n);
  w->fst = k.take<int32_t>(F);
  w->pairs = k.take<X3RLevPair>(P);
  w->prow = k.take<unsigned long long>(P + 1);
  w->rows = k.take<x3_level>(planes * (rows_cap + P));   // (a tone bank: a plane of rows_cap + P rows per tone)
  w->scratch = k.take<int16_t>(std::max<uint64_t>(fix_waves, 4) * scratch_per);
  w->sum = k.take<X3RLevSummary>(1, diff ? 256 : 1);
  w->tail = diff ? k.take<int32_t>(F) : nullptr;
  w->lead = diff ? k.take<uint32_t>(n, 1) : nullptr;
  return k.at;
}

// The launch set of a range-levels call behind its plan step: plan(grid, plan, gstart, sum) enqueues the ranges' plan kernel
// and returns the starts the later kernels read (the caller's, or the plan's gstart), as in windows_launch.  d_starts: the
// CALLER'S array, which the tone kernels read beside them.  d_ent, n_ent, d_entries: the corpus's table and the caller's
// entries for the lead kernels, NULL for a stream.  g picks the lead kernel, the instance of the accumulate and fix-up
// kernels and the seam kernel, in the switch below; DIFF and FIR share a workspace (tail[], lead[]), FIR leaves its edge
// records in fir_ws as in levels_launch and has a fix-up of its own; TONE has the SAMPLES call's P and workspace.
// BANK is TONE over g.planes() PLANES: d_levels holds that many planes of rows_cap records, the partial rows as many of cap;
// pairs, scans and verdicts are one plane's.  The accumulate instance is the smallest of NT = 2, 4, 8 that holds the tones,
// the fix-up's is NT = 8; x3_range_levels_planes_kernel writes the identities of the caller's planes 1 and up, and the init
// and merge kernels run once per plane on offset pointers.
template <class Plan>
static int range_levels_launch(x3_ctx* c, const FrameSource& s, const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n,
                               uint64_t bin_len, uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap,
                               uint64_t* d_row_offsets, int32_t* d_status, const LevSignal& g, const x3_corpus_entry* d_ent,
                               uint64_t n_ent, const uint32_t* d_entries, Plan plan_step) {
  const uint64_t lead_frames = g.lead_frames();
  HIPCHK(c, hipSetDevice(c->device));
  const uint64_t P = range_levels_pairs(n, s.F, s.max_frames, lead_frames), cap = rows_cap + P, planes = g.planes();
  const uint32_t scratch_per = levels_scratch_per(s.dp.block_len);
  const uint64_t fix_waves = levels_fix_waves(n, scratch_per);
  RLevWs w;
  int rc;
  if ((rc = ensure(c, c->rlev_ws, range_levels_carve(nullptr, n, s.F, P, rows_cap, fix_waves, scratch_per, &w, g.lead(), planes))))
    return rc;
  range_levels_carve((char*)c->rlev_ws.p, n, s.F, P, rows_cap, fix_waves, scratch_per, &w, g.lead(), planes);
  if (g.fir_ws() && (rc = ensure(c, c->fir_ws, (size_t)(s.F * s.nseg) * sizeof(X3FirEdge)))) return rc;
  // grids: the counts are on the device and every kernel walks them grid-stride.  What a range has on average is at most
  // rows_cap / n rows (or the stride) of bin_len positions: the caller's words, possibly far above what is drawn, so a range
  // covers no more frames than the stream (or the longest entry) has and a call no more pairs than P.
  const uint64_t rows_hint = row_stride ? row_stride : std::max<uint64_t>(rows_cap / n, 1);
  const uint64_t len_hint = bin_len && bin_len <= 0xFFFFFFFFull / rows_hint ? rows_hint * bin_len : 0xFFFFFFFFull;
  const uint64_t frames_per = std::max<uint64_t>(1, std::min(len_hint / (s.spf ? s.spf : 1) + 2 + lead_frames, s.max_frames));
  const uint64_t cov_hint = std::min(n * frames_per, P), item_hint = std::min<uint64_t>(cov_hint, 256ull * X3W_GRID_LIMIT) * s.nseg;
  // the caller's records: padded, all n * stride are written; packed, a range has no more rows than the frames it can cover
  // hold bins (one with bin_len 0 or above any length), so a roomy rows_cap does not size the prep, init and merge grids
  const uint64_t drawn_rows = row_stride ? rows_hint
                              : bin_len && bin_len <= 0xFFFFFFFFull ? std::min(rows_hint, frames_per * (s.spf ? s.spf : 1) / bin_len + 1) : 1;
  const uint64_t rec_hint = std::min(n * drawn_rows, rows_cap);
  const uint64_t* d_gstarts = plan_step(dim3(grid_for(n, 256)), w.plan, w.gstart, &w.sum->w);
  // everything behind the plan, for a signal: its lead kernel, the kernels all share, the two that decode, the merge, its seam
  auto run = [&](auto lead, auto sig, auto fix, auto tail, auto seam) {
    using Signal = decltype(sig);
    lead();
    hipLaunchKernelGGL(x3_range_levels_scan_kernel, dim3(1), dim3(1024), 0, c->stream, w.plan, n, d_lens, bin_len, row_stride, rows_cap,
                       w.cov_off, w.row_off, w.erows, d_row_offsets, w.sum);
    hipLaunchKernelGGL(x3_window_check_kernel, dim3(grid_for(cov_hint, 4)), dim3(256), 0, c->stream, s.d_x3, s.x3_len, s.d_frame_offsets,
                       s.d_sample_offsets, (const X3WinPlan*)w.plan, n, (const unsigned long long*)w.cov_off, w.fst);
    hipLaunchKernelGGL(x3_range_levels_prep_kernel, dim3(grid_for(std::max(cov_hint, rec_hint), 256)), dim3(256), 0, c->stream,
                       s.d_sample_offsets, d_gstarts, d_lens, (const X3WinPlan*)w.plan, n, (const unsigned long long*)w.cov_off,
                       (const unsigned long long*)w.row_off, (const uint32_t*)w.erows, bin_len, row_stride, rows_cap, P,
                       (const int32_t*)w.fst, w.pairs, d_levels);
    if (planes > 1)
      hipLaunchKernelGGL(x3_range_levels_planes_kernel, dim3(grid_for(rec_hint, 256)), dim3(256), 0, c->stream, n,
                         (const unsigned long long*)w.row_off, (const uint32_t*)w.erows, row_stride, rows_cap, (uint32_t)planes,
                         d_levels);
    hipLaunchKernelGGL(x3_range_levels_pair_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const X3RLevPair*)w.pairs,
                       (const unsigned long long*)w.cov_off, n, P, cap, w.prow, w.sum);
    for (uint64_t t = 0; t < planes; ++t)   // (a plane's rows and records: the same pairs, scans and verdicts)
      hipLaunchKernelGGL(x3_range_levels_init_kernel, dim3(grid_for(rec_hint + cov_hint, 256)), dim3(256), 0, c->stream,
                         (const unsigned long long*)w.cov_off, n, P, cap, (const unsigned long long*)w.prow, w.rows + t * cap);
    hipLaunchKernelGGL(x3_range_levels_accum_kernel<Signal>, dim3(grid_for(item_hint, 256)), dim3(256), 0, c->stream, s.d_x3, s.x3_len,
                       s.d_frame_offsets, s.dp, s.idx, s.seg_blocks, s.nseg, bin_len, (const unsigned long long*)w.cov_off, n, P, cap,
                       (const X3RLevPair*)w.pairs, (const unsigned long long*)w.prow, w.rows, w.fst, tail);
    auto fixup = [&](auto* kernel, auto... seg) {   // seg: what the FIR call's fix-up takes behind s.dp
      hipLaunchKernelGGL(kernel, dim3((unsigned)((fix_waves + 3) / 4)), dim3(256), 0, c->stream, s.d_x3, s.d_frame_offsets,
                         s.d_sample_offsets, d_gstarts, d_lens, (const X3WinPlan*)w.plan, n, s.dp, seg..., bin_len,
                         (const unsigned long long*)w.cov_off, (const unsigned long long*)w.row_off, (const uint32_t*)w.erows,
                         row_stride, P, cap, (const unsigned long long*)w.prow, (const int32_t*)w.fst, d_levels, d_status, w.scratch,
                         scratch_per, w.sum, tail, (const uint32_t*)w.lead);
    };
    if constexpr (std::is_same_v<Signal, X3LevFir>) fixup(x3_range_levels_fir_fixup_kernel, s.idx, s.seg_blocks, s.nseg);
    else fixup(x3_range_levels_fixup_kernel<decltype(fix)>);
    for (uint64_t t = 0; t < planes; ++t)
      hipLaunchKernelGGL(x3_range_levels_merge_kernel, dim3(grid_for(rec_hint + cov_hint, 256)), dim3(256), 0, c->stream,
                         (const X3RLevPair*)w.pairs, (const unsigned long long*)w.cov_off, n, P, cap,
                         (const unsigned long long*)w.prow, (const unsigned long long*)w.row_off, (const uint32_t*)w.erows,
                         row_stride, (const x3_level*)w.rows + t * cap, (const int32_t*)w.fst, d_levels + t * rows_cap);
    if (g.seam()) seam();
  };
  auto none = [] {};
  switch (g.kind) {
    case LevSignal::FIR:
      run([&] {
            hipLaunchKernelGGL(x3_range_levels_lead_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, s.d_sample_offsets,
                               d_ent, n_ent, d_entries, d_gstarts, d_lens, n, (uint32_t)lead_frames, w.plan, w.lead);
          },
          X3LevFir{}, X3LevFir{}, X3LevFirTail{g.fir, (X3FirEdge*)c->fir_ws.p, s.nseg}, [&] {
            hipLaunchKernelGGL(x3_range_levels_fir_seam_kernel, dim3(grid_for(item_hint, 256)), dim3(256), 0, c->stream,
                               s.dp.block_len, s.idx, s.seg_blocks, s.nseg, bin_len, (const X3RLevPair*)w.pairs,
                               (const unsigned long long*)w.cov_off, n, P, cap, (const unsigned long long*)w.prow,
                               (const unsigned long long*)w.row_off, (const uint32_t*)w.erows, row_stride, (const int32_t*)w.fst,
                               (const X3FirEdge*)c->fir_ws.p, s.nseg, g.fir, d_levels);
          });
      break;
    case LevSignal::TONE: run(none, X3LevTone{}, X3LevTone{}, X3LevToneTail{g.tone.table, g.tone.step, d_starts}, none); break;
    case LevSignal::DIFF:
      run([&] {
            hipLaunchKernelGGL(x3_range_levels_lead_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, s.d_sample_offsets, d_ent,
                               n_ent, d_entries, d_gstarts, d_lens, n, (uint32_t)lead_frames, w.plan, w.lead);
          },
          X3LevDiff{}, X3LevDiff{}, w.tail, [&] {
            hipLaunchKernelGGL(x3_range_levels_seam_kernel, dim3(grid_for(cov_hint, 256)), dim3(256), 0, c->stream, s.d_x3, s.x3_len,
                               s.d_frame_offsets, bin_len, (const X3RLevPair*)w.pairs, (const unsigned long long*)w.cov_off, n, P, cap,
                               (const unsigned long long*)w.prow, (const unsigned long long*)w.row_off, (const uint32_t*)w.erows,
                               row_stride, (const int32_t*)w.fst, (const int32_t*)w.tail, d_levels);
          });
      break;
    case LevSignal::SAMPLES: run(none, X3LevSamples{}, X3LevSamples{}, X3LevNoTail{}, none); break;
    case LevSignal::BANK: {
      X3LevToneBankTail t = g.bank;
      t.rows_stride = cap, t.levels_stride = rows_cap, t.starts = d_starts;
      using Fix = X3LevToneBank<X3L_TONE_BANK>;
      if (t.n_tones <= 2) run(none, X3LevToneBank<2>{}, Fix{}, t, none);
      else if (t.n_tones <= 4) run(none, X3LevToneBank<4>{}, Fix{}, t, none);
      else run(none, Fix{}, Fix{}, t, none);
      break;
    }
  }
  HIPCHK(c, hipGetLastError());
  c->range_levels.pending = true;
  c->range_levels.count = n;
  c->range_levels.sum_off = (size_t)((char*)w.sum - (char*)c->rlev_ws.p);
  return X3_OK;
}

// the stream form of the range-levels calls behind the check of the signal
static int stream_range_levels_call(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                    const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                    const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                    const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                    x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                    const LevSignal& g) {
  if (!range_levels_args_ok(c, d_starts, d_lens, n_ranges, row_stride, d_levels, rows_cap, d_row_offsets, d_status))
    return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = stream_source(d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, &s);
  if (rc) return rc;
  return range_levels_launch(c, s, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, g,
                             nullptr, 0, nullptr,
                             [&](dim3 grid, X3WinPlan* plan, uint64_t*, X3WinSummary* sum) -> const uint64_t* {
                               hipLaunchKernelGGL(x3_range_plan_kernel, grid, dim3(256), 0, c->stream, d_sample_offsets, n_frames,
                                                  d_starts, d_lens, n_ranges, plan, sum);
                               return d_starts;
                             });
}

extern "C" int x3_signal_range_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                          const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                          const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                          const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                          x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                          int signal) {
  if (!c || !levels_signal_ok(signal)) return X3_ERR_BAD_ARG;
  return stream_range_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, d_starts,
                                  d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                  LevSignal(signal));
}

extern "C" int x3_fir_range_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                       const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                       const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                       const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                       x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                       const x3_level_fir* fir) {
  X3FirTaps k;
  if (!c || !levels_fir_taps(fir, &k)) return X3_ERR_BAD_ARG;
  return stream_range_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, d_starts,
                                  d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, LevSignal(k));
}

extern "C" int x3_tone_range_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                        const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                        const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                        const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                        x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                        const x3_level_tone* tone) {
  X3LevToneTail t;
  if (!c || !levels_tone_arg(tone, &t)) return X3_ERR_BAD_ARG;
  return stream_range_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, d_starts,
                                  d_lens, n_ranges, bin_len, row_stride, reinterpret_cast<x3_level*>(d_levels), rows_cap,
                                  d_row_offsets, d_status, LevSignal(t));
}

// the bank: n_tones tone-range calls plane by plane (plane stride rows_cap) in one pass over the covering frames
extern "C" int x3_tone_bank_range_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                             const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                             const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                             const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                             x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                             int32_t* d_status, const x3_level_tone_bank* bank) {
  X3LevToneBankTail t;
  if (!c || !levels_tone_bank_arg(bank, &t)) return X3_ERR_BAD_ARG;
  const LevSignal g(t);
  if (!levels_planes_ok(g, rows_cap)) return X3_ERR_BAD_ARG;
  return stream_range_levels_call(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks, d_starts,
                                  d_lens, n_ranges, bin_len, row_stride, reinterpret_cast<x3_level*>(d_levels), rows_cap,
                                  d_row_offsets, d_status, g);
}

extern "C" int x3_range_levels_dev(x3_ctx* c, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                   const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                   const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                   const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                   x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status) {
  return x3_signal_range_levels_dev(c, d_x3, x3_len, d_frame_offsets, d_sample_offsets, n_frames, p, d_seg_index, seg_blocks,
                                    d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                    X3_LEVEL_SIGNAL_SAMPLES);
}

// (entry: the name errors carry -- the call the caller made; d_starts are entry-relative)
static int corpus_range_levels_call(x3_ctx* c, const x3_corpus* k, const char* entry, const uint32_t* d_entries,
                                    const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len,
                                    uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                    int32_t* d_status, const LevSignal& g) {
  if (!c || !k || !d_entries || (reinterpret_cast<uintptr_t>(d_entries) & 3u)) return X3_ERR_BAD_ARG;
  if (!range_levels_args_ok(c, d_starts, d_lens, n_ranges, row_stride, d_levels, rows_cap, d_row_offsets, d_status))
    return X3_ERR_BAD_ARG;
  FrameSource s;
  const int rc = corpus_source(c, k, entry, &s);
  if (rc) return rc;
  return range_levels_launch(c, s, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, g,
                             (const x3_corpus_entry*)k->d_ent, k->n, d_entries,
                             [&](dim3 grid, X3WinPlan* plan, uint64_t* gstart, X3WinSummary* sum) -> const uint64_t* {
                               hipLaunchKernelGGL(x3_corpus_range_plan_kernel, grid, dim3(256), 0, c->stream, k->d_ent, k->n,
                                                  s.d_sample_offsets, s.F, d_entries, d_starts, d_lens, n_ranges, plan, gstart,
                                                  sum);
                               return gstart;
                             });
}

extern "C" int x3_corpus_range_levels_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                          const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                          x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status) {
  return corpus_range_levels_call(c, k, "x3_corpus_range_levels_dev", d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride,
                                  d_levels, rows_cap, d_row_offsets, d_status, LevSignal(X3_LEVEL_SIGNAL_SAMPLES));
}

extern "C" int x3_corpus_signal_range_levels_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                                 const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                                 x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                                 int signal) {
  if (!c || !levels_signal_ok(signal)) return X3_ERR_BAD_ARG;
  return corpus_range_levels_call(c, k, "x3_corpus_signal_range_levels_dev", d_entries, d_starts, d_lens, n_ranges, bin_len,
                                  row_stride, d_levels, rows_cap, d_row_offsets, d_status, LevSignal(signal));
}

extern "C" int x3_corpus_fir_range_levels_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                              const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                              x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                              const x3_level_fir* fir) {
  X3FirTaps taps;
  if (!c || !levels_fir_taps(fir, &taps)) return X3_ERR_BAD_ARG;
  return corpus_range_levels_call(c, k, "x3_corpus_fir_range_levels_dev", d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride,
                                  d_levels, rows_cap, d_row_offsets, d_status, LevSignal(taps));
}

extern "C" int x3_corpus_tone_range_levels_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries, const uint64_t* d_starts,
                                               const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                               x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                               int32_t* d_status, const x3_level_tone* tone) {
  X3LevToneTail t;
  if (!c || !levels_tone_arg(tone, &t)) return X3_ERR_BAD_ARG;
  return corpus_range_levels_call(c, k, "x3_corpus_tone_range_levels_dev", d_entries, d_starts, d_lens, n_ranges, bin_len, row_stride,
                                  reinterpret_cast<x3_level*>(d_levels), rows_cap, d_row_offsets, d_status, LevSignal(t));
}

extern "C" int x3_corpus_tone_bank_range_levels_dev(x3_ctx* c, const x3_corpus* k, const uint32_t* d_entries,
                                                    const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges,
                                                    uint64_t bin_len, uint64_t row_stride, x3_tone_level* d_levels,
                                                    uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                                    const x3_level_tone_bank* bank) {
  X3LevToneBankTail t;
  if (!c || !levels_tone_bank_arg(bank, &t)) return X3_ERR_BAD_ARG;
  const LevSignal g(t);
  if (!levels_planes_ok(g, rows_cap)) return X3_ERR_BAD_ARG;
  return corpus_range_levels_call(c, k, "x3_corpus_tone_bank_range_levels_dev", d_entries, d_starts, d_lens, n_ranges, bin_len,
                                  row_stride, reinterpret_cast<x3_level*>(d_levels), rows_cap, d_row_offsets, d_status, g);
}

extern "C" int x3_range_levels_result(x3_ctx* c, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status,
                                      uint64_t* total_rows) {
  if (!c) return X3_ERR_BAD_ARG;
  X3RLevSummary h{{0, 0, 0, 0}, 0};
  const int rc = pending_fetch(c, c->range_levels, c->rlev_ws, &h, sizeof h);
  if (rc) return rc;
  c->last_range_levels_replays = h.w.replays;
  c->last_range_levels_overflow = h.overflow;
  first_bad_of(h.w.n_bad, h.w.first, c->range_levels.count, n_bad, first_bad, first_bad_status);
  if (total_rows) *total_rows = h.w.total;
  return X3_OK;
}

// ------------------------------------------------------------------------------------------------
// spectra: the exact integer STFT of int16 rows in HBM, on the matrix cores (x3_spectra_kernel.h)
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(x3_spectra_rule) == 24 && offsetof(x3_spectra_rule, hop) == 4 && offsetof(x3_spectra_rule, format) == 8 &&
                  offsetof(x3_spectra_rule, reserved) == 12 && offsetof(x3_spectra_rule, d_table) == 16,
              "include/x3hip.h states this layout");

// The workspace (SpecWs, x3_internal.h): per range the scan of the rows, the rows that are transformed and those that have
// room; the B operand of the rule's n_fft -- 2 * KT tiles of N / 64 steps, two planes of 64 lanes x 16 bytes each -- and its
// column sums; the summary
size_t spectra_carve(char* base, uint64_t n, uint32_t n_fft, SpecWs* w, bool frames) {
  BlockCarver k{base, 0};
  const uint64_t tiles = 2ull * ((n_fft / 2 + 1 + 15) / 16);
  w->row_off = k.take<unsigned long long>(n + 1);
  w->live = k.take<uint32_t>(n);
  w->wr = k.take<uint32_t>(n);
  w->basis = k.take<uint4>(tiles * (n_fft / 64) * 128);
  w->colsum = k.take<int32_t>(tiles * 16);
  w->frame_off = frames ? k.take<unsigned long long>(n + 1) : nullptr;
  w->sum = k.take<X3WinSummary>(1, 1);
  return k.at;
}

// what both calls refuse, in the header's order: the rule first, then everything else (d_out: the rows or the records)
static bool spectra_rule_ok(const x3_spectra_rule* rule) {
  if (!rule) return false;
  const uint32_t N = rule->n_fft;
  return !((N != 64 && N != 128 && N != 256 && N != 512 && N != 1024) || rule->hop == 0 || rule->hop > 0x7FFFFFFFu ||
           (rule->format != X3_SPECTRA_SUMS && rule->format != X3_SPECTRA_POWER) || rule->reserved || !rule->d_table ||
           (reinterpret_cast<uintptr_t>(rule->d_table) & 3u));
}

static bool spectra_args_ok(const x3_ctx* c, const int16_t* d_samples, const uint64_t* d_offsets, const uint32_t* d_lens,
                            const int32_t* d_in_status, uint64_t n_ranges, uint64_t row_stride, const void* d_out,
                            uint64_t rows_cap, const uint64_t* d_row_offsets, const int32_t* d_status) {
  if (n_ranges == 0 || n_ranges > 0x7FFFFFFFull || rows_cap == 0 || rows_cap > 0x7FFFFFFFull) return false;
  if (!d_samples || !d_offsets || !d_lens || !d_out || !d_status || c->capturing) return false;
  if (row_stride ? row_stride > rows_cap / n_ranges : !d_row_offsets) return false;
  return !((reinterpret_cast<uintptr_t>(d_samples) & 1u) ||
           ((reinterpret_cast<uintptr_t>(d_lens) | reinterpret_cast<uintptr_t>(d_in_status) | reinterpret_cast<uintptr_t>(d_status)) & 3u) ||
           ((reinterpret_cast<uintptr_t>(d_offsets) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_row_offsets)) & 7u));
}

static X3SpGeo spectra_geo(const x3_spectra_rule* rule) {
  X3SpGeo g{};
  g.N = rule->n_fft;
  while ((1u << g.lgN) < g.N) ++g.lgN;
  g.H = rule->hop;
  g.B = g.N / 2 + 1;
  g.KT = (g.B + 15) / 16;
  g.format = rule->format;
  return g;
}

extern "C" int x3_spectra_rows_dev(x3_ctx* c, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                                   const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges,
                                   const x3_spectra_rule* rule, uint64_t row_stride, void* d_out, uint64_t rows_cap,
                                   uint64_t* d_row_offsets, int32_t* d_status) {
  if (!c || !spectra_rule_ok(rule)) return X3_ERR_BAD_ARG;
  if (!spectra_args_ok(c, d_samples, d_offsets, d_lens, d_in_status, n_ranges, row_stride, d_out, rows_cap, d_row_offsets, d_status))
    return X3_ERR_BAD_ARG;
  const uint32_t N = rule->n_fft;
  HIPCHK(c, hipSetDevice(c->device));
  SpecWs w;
  int rc;
  if ((rc = ensure(c, c->spec_ws, spectra_carve(nullptr, n_ranges, N, &w)))) return rc;
  spectra_carve((char*)c->spec_ws.p, n_ranges, N, &w);
  const X3SpGeo g = spectra_geo(rule);
  hipLaunchKernelGGL(x3_spectra_plan_kernel, dim3(1), dim3(1024), 0, c->stream, d_offsets, d_lens, d_in_status, n_ranges,
                     samples_cap, g, row_stride, rows_cap, w.row_off, w.live, w.wr, d_row_offsets, d_status, w.sum);
  hipLaunchKernelGGL(x3_spectra_basis_kernel, dim3(grid_for(2ull * g.KT * (N / 64) * 64, 256)), dim3(256), 0, c->stream,
                     rule->d_table, g, w.basis, w.colsum);
  // (the rows are counted on the device: a workgroup per 16 or 32 of what the caller's rows hold at most, grid-stride.
  //  Packed, that is rows_cap -- the caller's word, possibly far above the rows that exist: the surplus workgroups, 4 096 at
  //  most, read row_off[n], find no tile of theirs and end)
  const uint64_t rows_hint = row_stride ? n_ranges * row_stride : rows_cap;
  auto transform = [&](auto* kernel, uint32_t row_tiles) {
    const size_t lds = 2u * 16u * (size_t)row_tiles * (N + 16u);
    hipLaunchKernelGGL(kernel, dim3(grid_for(rows_hint, 16u * row_tiles)), dim3(256), lds, c->stream, d_samples, d_offsets, n_ranges,
                       g, row_stride, rows_cap, (const unsigned long long*)w.row_off, (const uint32_t*)w.live,
                       (const uint32_t*)w.wr, (const uint4*)w.basis, (const int32_t*)w.colsum, d_out);
  };
  if (N <= 512) transform(x3_spectra_transform_kernel<2>, 2);   // (two row tiles share a load of the B operand; LDS: 33 KB at most)
  else transform(x3_spectra_transform_kernel<1>, 1);
  HIPCHK(c, hipGetLastError());
  c->spectra.pending = true;
  c->spectra.count = n_ranges;
  c->spectra.sum_off = (size_t)((char*)w.sum - (char*)c->spec_ws.p);
  return X3_OK;
}

// band levels (x3_spectra_levels_kernel.h): the rows call's pending slot and workspace, its basis kernel
// as it is, a plan, an init and a transform of its own
static_assert(sizeof(x3_spectra_fold) == 32 && offsetof(x3_spectra_fold, n_bands) == 4 && offsetof(x3_spectra_fold, plane_stride) == 8 &&
                  offsetof(x3_spectra_fold, d_bin_band) == 16 && offsetof(x3_spectra_fold, reserved) == 24,
              "include/x3hip.h states this layout");

extern "C" int x3_spectra_levels_dev(x3_ctx* c, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                                     const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges,
                                     const x3_spectra_rule* rule, const x3_spectra_fold* fold, uint64_t row_stride,
                                     x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status) {
  if (!c || !spectra_rule_ok(rule) || rule->format != X3_SPECTRA_POWER) return X3_ERR_BAD_ARG;
  const uint32_t N = rule->n_fft, B = N / 2 + 1;
  if (!fold || fold->frames_per_bin == 0 || fold->frames_per_bin > 0x7FFFFFFFu || fold->n_bands == 0 || fold->n_bands > B ||
      !fold->d_bin_band || (reinterpret_cast<uintptr_t>(fold->d_bin_band) & 3u) || fold->reserved ||
      (fold->plane_stride && fold->plane_stride < rows_cap))
    return X3_ERR_BAD_ARG;
  // (K <= 513: the product cannot wrap below plane strides of 2^54, and above 2^31 it fails the test either way)
  if (std::max(fold->plane_stride, rows_cap) > 0x7FFFFFFFull / fold->n_bands) return X3_ERR_BAD_ARG;
  if (!spectra_args_ok(c, d_samples, d_offsets, d_lens, d_in_status, n_ranges, row_stride, d_levels, rows_cap, d_row_offsets, d_status))
    return X3_ERR_BAD_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  SpecWs w;
  int rc;
  if ((rc = ensure(c, c->spec_ws, spectra_carve(nullptr, n_ranges, N, &w, true)))) return rc;
  spectra_carve((char*)c->spec_ws.p, n_ranges, N, &w, true);
  const X3SpGeo g = spectra_geo(rule);
  const X3SpFold fd{fold->frames_per_bin, fold->n_bands, fold->plane_stride ? fold->plane_stride : rows_cap};
  // LDS: the planes and 16 * MT * K accumulators of 8 bytes -- 99 584 bytes at n_fft 512 and 98 944 at 1 024 with K = B, past the
  // 64 KB a kernel gets unasked: the limit is raised before anything is enqueued
  const uint32_t row_tiles = N <= 512 ? 2u : 1u;   // (as the rows call: two row tiles share a load of the B operand)
  const size_t lds = 2u * 16u * (size_t)row_tiles * (N + 16u) + 16u * (size_t)row_tiles * fd.K * 8u;
  const void* const kernel = row_tiles == 2u ? reinterpret_cast<const void*>(x3_spectra_levels_transform_kernel<2>)
                                             : reinterpret_cast<const void*>(x3_spectra_levels_transform_kernel<1>);
  if (lds > 65536u) HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(x3_spectra_levels_plan_kernel, dim3(1), dim3(1024), 0, c->stream, d_offsets, d_lens, d_in_status, n_ranges,
                     samples_cap, g, fd.M, row_stride, rows_cap, w.row_off, w.frame_off, w.live, w.wr, d_row_offsets, d_status, w.sum);
  hipLaunchKernelGGL(x3_spectra_basis_kernel, dim3(grid_for(2ull * g.KT * (N / 64) * 64, 256)), dim3(256), 0, c->stream,
                     rule->d_table, g, w.basis, w.colsum);
  const uint64_t rows_hint = row_stride ? n_ranges * row_stride : rows_cap;
  hipLaunchKernelGGL(x3_spectra_levels_init_kernel, dim3(grid_for(rows_hint, 256), std::min<uint32_t>(fd.K, 16u)), dim3(256), 0,
                     c->stream, (const unsigned long long*)w.row_off, n_ranges, row_stride, rows_cap, fd, d_levels);
  // (the frames are counted on the device, at most frames_per_bin for each of the rows the caller's buffer holds: the surplus
  //  workgroups, 4 096 at most, read frame_off[n], find no tile of theirs and end)
  const uint64_t frames_hint = rows_hint * (uint64_t)fd.M;   // (below 2^62)
  auto transform = [&](auto* k) {
    hipLaunchKernelGGL(k, dim3(grid_for(frames_hint, 16u * row_tiles)), dim3(256), lds, c->stream, d_samples, d_offsets, n_ranges, g,
                       fd, row_stride, (const unsigned long long*)w.row_off, (const unsigned long long*)w.frame_off,
                       (const uint4*)w.basis, (const int32_t*)w.colsum, fold->d_bin_band, d_levels);
  };
  if (row_tiles == 2u) transform(x3_spectra_levels_transform_kernel<2>);
  else transform(x3_spectra_levels_transform_kernel<1>);
  HIPCHK(c, hipGetLastError());
  c->spectra.pending = true;
  c->spectra.count = n_ranges;
  c->spectra.sum_off = (size_t)((char*)w.sum - (char*)c->spec_ws.p);
  return X3_OK;
}

extern "C" int x3_spectra_result(x3_ctx* c, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status, uint64_t* total_rows) {
  if (!c) return X3_ERR_BAD_ARG;
  X3WinSummary h{0, 0, 0, 0};
  const int rc = pending_fetch(c, c->spectra, c->spec_ws, &h, sizeof h);
  if (rc) return rc;
  first_bad_of(h.n_bad, h.first, c->spectra.count, n_bad, first_bad, first_bad_status);
  if (total_rows) *total_rows = h.total;
  return X3_OK;
}
