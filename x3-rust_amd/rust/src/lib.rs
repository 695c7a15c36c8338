//! Drop-in for the encode/decode path of the `x3` crate (psiphi75/x3-rust 0.3.1), backed by libx3hip.so: HIP kernels
//! on an MI355X.  Module names, item names, argument lists and result types are the reference crate's, so a caller
//! switches by changing the dependency; the work behind every item runs on the GPU through the C ABI of
//! include/x3hip.h.  There is no CPU path: without a usable HIP device the first call fails with `X3Error::Hip`
//! (items whose reference signature has no error path panic with the library's message).
//!
//! The reference's functions take no device handle.  They run on a process-wide context ([`gpu::with_default`]:
//! device `$X3HIP_DEVICE` or 0, created on first use, serialized by a mutex); [`gpu::Gpu`] and the `*_on` variants
//! exist for callers that manage devices themselves.
//!
//! SOURCE ONLY -- the build container has no Rust toolchain; host/x3.hpp mirrors these shapes in C++ and
//! tests/host_cpp/test_x3_hpp.cpp compiles and runs them on the GPU.

pub mod ffi {
    //! `extern "C"` declarations of include/x3hip.h (the entry points this crate binds).
    use std::os::raw::{c_char, c_int, c_longlong, c_void};

    /// `x3_batch`: `n_clips` clips of `n_per_clip` samples, `clip_stride` samples apart
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct x3_batch {
        pub n_per_clip: u64,
        pub clip_stride: u64,
        pub n_clips: u64,
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct x3_params {
        pub block_len: u32,
        pub blocks_per_frame: u32,
        pub codes: [u32; 3],
        pub thresholds: [u32; 3],
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct x3_frame_header {
        pub source_id: u8,
        pub channels: u8,
        pub samples: u16,
        pub payload_len: u32,
        pub payload_crc: u16,
    }
    /// `x3_stream_result`: one entry of `x3_decode_streams_dev`
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct x3_stream_result {
        pub n_out: u64,
        pub frames_ok: u64,
        pub status: i32,
        pub frame_errors: u32,
    }
    /// `x3_corpus_entry`: one entry of a corpus (`x3_corpus_entries`)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default)]
    pub struct x3_corpus_entry {
        pub n_samples: u64,
        pub first_frame: u64,
        pub n_frames: u64,
        pub walk_status: i32,
        pub general_walk: u32,
    }
    /// `x3_level`: one bin of `x3_levels_dev` / `x3_corpus_levels_dev` (32 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_level {
        pub sum_sq: u64,
        pub sum: i64,
        pub min: i32,
        pub max: i32,
        pub n: u32,
        pub reserved: u32,
    }
    /// `x3_level_fir`: the taps and shift of `x3_fir_levels_dev` / `x3_corpus_fir_levels_dev` (24 bytes); taps at and behind
    /// `n_taps` are ignored
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_level_fir {
        pub n_taps: u32,
        pub shift: u32,
        pub taps: [i16; 8],
    }
    /// `x3_level_tone`: the oscillator of `x3_tone_levels_dev` / `x3_corpus_tone_levels_dev` (16 bytes); `d_table` is a
    /// device array of 1 024 (cos, sin) `i16` pairs, 4-byte aligned; `reserved` must be 0
    #[repr(C)]
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct x3_level_tone {
        pub step: u32,
        pub reserved: u32,
        pub d_table: *const i16,
    }
    /// `x3_level_tone_bank`: the oscillators of `x3_tone_bank_levels_dev` / `x3_corpus_tone_bank_levels_dev` against one
    /// table (48 bytes); `steps` behind `n_tones` (1 ..= 8) are never read; `reserved` must be 0
    #[repr(C)]
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub struct x3_level_tone_bank {
        pub n_tones: u32,
        pub reserved: u32,
        pub d_table: *const i16,
        pub steps: [u32; 8],
    }
    /// `x3_tone_level`: one bin of `x3_tone_levels_dev` / `x3_corpus_tone_levels_dev` (32 bytes, `x3_level`'s layout slot for
    /// slot)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_tone_level {
        pub re: i64,
        pub im: i64,
        pub min: i32,
        pub max: i32,
        pub n: u32,
        pub reserved: u32,
    }
    /// `x3_event_rule`: which bins are hot and how runs of them become events (`x3_events_dev`; 32 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_event_rule {
        pub mean_sq_min: u64,
        pub peak_min: u32,
        pub join_bins: u32,
        pub min_bins: u32,
        pub pad_bins: u32,
        pub max_bins: u32,
        pub reserved: u32,
    }
    /// `x3_threshold_rule`: per criterion `thr = clamp(floor(quantile(q_ppm) * mul / div) + add, 1, limit)`; `div == 0`: off
    /// (`x3_level_thresholds_dev`; 32 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_threshold_rule {
        pub peak_q_ppm: u32,
        pub peak_mul: u32,
        pub peak_div: u32,
        pub peak_add: u32,
        pub mean_sq_q_ppm: u32,
        pub mean_sq_mul: u32,
        pub mean_sq_div: u32,
        pub mean_sq_add: u32,
    }
    /// `x3_event_threshold`: the events rule's two values for one entry and its counting rows (16 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_event_threshold {
        pub mean_sq_min: u64,
        pub peak_min: u32,
        pub counted: u32,
    }
    /// `x3_plane_event_rule`: a row is hot when at least `min_planes` of `n_planes` planes are loud at it, each plane under
    /// its own two values (`x3_plane_events_dev`; 128 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
    pub struct x3_plane_event_rule {
        pub n_planes: u32,
        pub min_planes: u32,
        pub join_bins: u32,
        pub min_bins: u32,
        pub pad_bins: u32,
        pub max_bins: u32,
        pub reserved: [u32; 2],
        pub mean_sq_min: [u64; 8],
        pub peak_min: [u32; 8],
    }
    /// `x3_spectra_rule`: the transform of `x3_spectra_rows_dev` -- `n_fft` in 64 .. 1024 (a power of two), `hop` >= 1,
    /// `format` `X3_SPECTRA_SUMS` (0) or `X3_SPECTRA_POWER` (1), `d_table` a device table of 1 024 (cos, sin) i16 pairs (24 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct x3_spectra_rule {
        pub n_fft: u32,
        pub hop: u32,
        pub format: u32,
        pub reserved: u32,
        pub d_table: *const i16,
    }
    /// `x3_spectra_fold`: how `x3_spectra_levels_dev` folds the POWER words -- `frames_per_bin` consecutive frames into a time
    /// bin, bin k of a frame into band `d_bin_band[k]` (a device array of `n_fft / 2 + 1` u32 words, a word >= `n_bands`: no
    /// band), plane b of the records `b * plane_stride` records in (0: `rows_cap`) (32 bytes)
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct x3_spectra_fold {
        pub frames_per_bin: u32,
        pub n_bands: u32,
        pub plane_stride: u64,
        pub d_bin_band: *const u32,
        pub reserved: u64,
    }
    #[repr(C)]
    #[derive(Clone, Copy, Debug)]
    pub struct x3_rice_code {
        pub nsubs: u32,
        pub offset: u32,
        pub len: u32,
        pub inv_len: u32,
        pub code: *const u32,
        pub num_bits: *const u32,
        pub inv: *const i16,
    }
    macro_rules! opaque {
        ($($n:ident),*) => { $(#[repr(C)] pub struct $n { _private: [u8; 0] })* };
    }
    opaque!(x3_ctx, x3_bitreader, x3_bitpacker, x3_reader, x3_tuner, x3_corpus);

    extern "C" {
        pub fn x3_strerror(status: c_int) -> *const c_char;
        pub fn x3_ctx_create(device: c_int, ctx: *mut *mut x3_ctx) -> c_int;
        pub fn x3_ctx_create_on_stream(device: c_int, hip_stream: *mut c_void, ctx: *mut *mut x3_ctx) -> c_int;
        pub fn x3_ctx_destroy(ctx: *mut x3_ctx);
        pub fn x3_last_error(ctx: *const x3_ctx) -> *const c_char;
        pub fn x3_ctx_set_option(ctx: *mut x3_ctx, name: *const c_char, value: c_longlong) -> c_int;
        pub fn x3_params_validate(p: *const x3_params) -> c_int;
        pub fn x3_rice_code_get(code_number: u32, out: *mut x3_rice_code) -> c_int;
        pub fn x3_encode_bound(n: u64, p: *const x3_params) -> u64;
        pub fn x3_crc16(ctx: *mut x3_ctx, data: *const u8, n: u64, crc: *mut u16) -> c_int;
        pub fn x3_crc16_update(crc: u16, byte: u8) -> u16;
        pub fn x3_encode(ctx: *mut x3_ctx, wav: *const i16, n: u64, n_channels: u32, p: *const x3_params,
                         out: *mut u8, out_cap: u64, start_pos: u64, out_pos: *mut u64, stats: *mut u64) -> c_int;
        pub fn x3_encode_frame(ctx: *mut x3_ctx, wav: *const i16, n: u64, p: *const x3_params, out: *mut u8,
                               out_cap: u64, start_pos: u64, out_pos: *mut u64, stats: *mut u64) -> c_int;
        pub fn x3_write_frame_header(num_samples: u64, id: u8, payload_len: u64, payload_crc: u16, out: *mut u8);
        pub fn x3_read_frame_header(bytes: *const u8, len: u64, h: *mut x3_frame_header) -> c_int;
        pub fn x3_decode_frame(ctx: *mut x3_ctx, payload: *const u8, len: u64, wav: *mut i16, wav_cap: u64,
                               p: *const x3_params, samples: u64, n_out: *mut u64) -> c_int;
        pub fn x3_decode_prefetch(ctx: *mut x3_ctx, x3: *const u8, len: u64, p: *const x3_params) -> c_int;
        pub fn x3_decode_stream(ctx: *mut x3_ctx, x3: *const u8, len: u64, p: *const x3_params, wav: *mut i16,
                                wav_cap: u64, n_out: *mut u64, frames_ok: *mut u64, frame_errors: *mut u64) -> c_int;
        pub fn x3_encode_mc(ctx: *mut x3_ctx, wavs: *const *const i16, n_channels: u32, n: u64, p: *const x3_params,
                            out: *mut u8, out_cap: u64, start_pos: u64, out_pos: *mut u64, stats: *mut u64) -> c_int;
        pub fn x3_decode_stream_mc(ctx: *mut x3_ctx, x3: *const u8, len: u64, n_channels: u32, p: *const x3_params,
                                   wavs: *const *mut i16, wav_cap: u64, n_samples: *mut u64, frames_ok: *mut u64,
                                   frame_errors: *mut u64) -> c_int;
        pub fn x3_bitreader_new(ctx: *mut x3_ctx, array: *const u8, len: u64, br: *mut *mut x3_bitreader) -> c_int;
        pub fn x3_bitreader_read_nbits(br: *mut x3_bitreader, n: u32, value: *mut u32) -> c_int;
        pub fn x3_bitreader_count_zero_bits(br: *mut x3_bitreader, count: *mut u32) -> c_int;
        pub fn x3_bitreader_inc_bits(br: *mut x3_bitreader, n: u32) -> c_int;
        pub fn x3_bitreader_free(br: *mut x3_bitreader);
        pub fn x3_decode_block(br: *mut x3_bitreader, wav: *mut i16, n: u32, last_wav: *mut i16, p: *const x3_params) -> c_int;
        pub fn x3_bitpacker_new(ctx: *mut x3_ctx, out: *mut u8, out_cap: u64, start_pos: u64, bp: *mut *mut x3_bitpacker) -> c_int;
        pub fn x3_bitpacker_write_bits(bp: *mut x3_bitpacker, value: u64, num_bits: u32) -> c_int;
        pub fn x3_bitpacker_write_packed_zeros(bp: *mut x3_bitpacker, num_zeros: u32) -> c_int;
        pub fn x3_bitpacker_write_bytes(bp: *mut x3_bitpacker, array: *const u8, n: u64) -> c_int;
        pub fn x3_bitpacker_inc_counter_n_bytes(bp: *mut x3_bitpacker, n_bytes: u64) -> c_int;
        pub fn x3_bitpacker_word_align(bp: *mut x3_bitpacker) -> c_int;
        pub fn x3_bitpacker_finish(bp: *mut x3_bitpacker, len: *mut u64, crc: *mut u16, out_pos: *mut u64) -> c_int;
        pub fn x3_bitpacker_peek(bp: *const x3_bitpacker, len: *mut u64, crc: *mut u16) -> c_int;
        pub fn x3_bitpacker_take(bp: *mut x3_bitpacker, dst: *mut u8, dst_cap: u64, n_new: *mut u64, len: *mut u64,
                                 crc: *mut u16) -> c_int;
        pub fn x3_bitpacker_free(bp: *mut x3_bitpacker);
        // device-resident buffers (mod device)
        pub fn x3_num_frames(n: u64, p: *const x3_params) -> u64;
        pub fn x3_dev_alloc(ctx: *mut x3_ctx, bytes: u64, d_ptr: *mut *mut c_void) -> c_int;
        pub fn x3_dev_free(ctx: *mut x3_ctx, d_ptr: *mut c_void) -> c_int;
        pub fn x3_dev_upload(ctx: *mut x3_ctx, d_dst: *mut c_void, src: *const c_void, bytes: u64) -> c_int;
        pub fn x3_dev_download(ctx: *mut x3_ctx, dst: *mut c_void, d_src: *const c_void, bytes: u64) -> c_int;
        pub fn x3_seg_index_entries(n_frames: u64, p: *const x3_params, seg_blocks: u32) -> u64;
        pub fn x3_encode_dev(ctx: *mut x3_ctx, d_wav: *const i16, batch: *const x3_batch, p: *const x3_params, d_out: *mut u8,
                             out_cap: u64, start_pos: u64, d_frame_offsets: *mut u64) -> c_int;
        pub fn x3_encode_dev_seg(ctx: *mut x3_ctx, d_wav: *const i16, batch: *const x3_batch, p: *const x3_params, d_out: *mut u8,
                                 out_cap: u64, start_pos: u64, d_frame_offsets: *mut u64, d_seg_index: *mut u64,
                                 seg_blocks: u32) -> c_int;
        pub fn x3_encode_result(ctx: *mut x3_ctx, out_pos: *mut u64, stats: *mut u64) -> c_int;
        pub fn x3_decode_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64, n_frames: u64,
                             batch: *const x3_batch, d_wav_offsets: *const u64, p: *const x3_params, d_wav: *mut i16,
                             wav_cap: u64, d_status: *mut i32) -> c_int;
        pub fn x3_decode_dev_seg(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64, n_frames: u64,
                                 batch: *const x3_batch, d_wav_offsets: *const u64, p: *const x3_params, d_wav: *mut i16,
                                 wav_cap: u64, d_status: *mut i32, d_seg_index: *mut u64, seg_blocks: u32, record: c_int) -> c_int;
        pub fn x3_decode_result(ctx: *mut x3_ctx, first_bad: *mut u64, first_bad_status: *mut c_int, samples_before: *mut u64) -> c_int;
        pub fn x3_seg_index_build_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64, n_frames: u64,
                                      p: *const x3_params, d_seg_index: *mut u64, seg_blocks: u32) -> c_int;
        pub fn x3_sample_offsets_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64, n_frames: u64,
                                     d_sample_offsets: *mut u64) -> c_int;
        pub fn x3_decode_windows_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                     d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                     seg_blocks: u32, d_starts: *const u64, n_windows: u64, window_len: u32, d_out: *mut c_void,
                                     out_format: c_int, d_status: *mut i32) -> c_int;
        pub fn x3_decode_windows_result(ctx: *mut x3_ctx, n_bad: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int) -> c_int;
        pub fn x3_decode_ranges_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                    d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                    seg_blocks: u32, d_starts: *const u64, d_lens: *const u32, n_ranges: u64, row_stride: u64,
                                    d_out: *mut c_void, out_cap: u64, out_format: c_int, d_out_offsets: *mut u64,
                                    d_status: *mut i32) -> c_int;
        pub fn x3_decode_ranges_result(ctx: *mut x3_ctx, n_bad: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int,
                                       total_samples: *mut u64) -> c_int;
        pub fn x3_decode_streams_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, offsets: *const u64, lengths: *const u64,
                                     n_streams: u64, flags: u32, p: *const x3_params, d_out: *mut c_void, row_len: u64,
                                     out_format: c_int, d_results: *mut x3_stream_result) -> c_int;
        pub fn x3_decode_streams_result(ctx: *mut x3_ctx, n_bad: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int) -> c_int;
        pub fn x3_corpus_build(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, offsets: *const u64, lengths: *const u64,
                               n_entries: u64, flags: u32, p: *const x3_params, seg_blocks: u32, corpus: *mut *mut x3_corpus) -> c_int;
        pub fn x3_corpus_info(corpus: *const x3_corpus, n_entries: *mut u64, n_frames: *mut u64, total_samples: *mut u64,
                              seg_blocks_in_use: *mut u32) -> c_int;
        pub fn x3_corpus_entries(corpus: *const x3_corpus, out: *mut x3_corpus_entry) -> c_int;
        pub fn x3_corpus_seg_index(corpus: *const x3_corpus, d_seg_index: *mut *const u64, n_words: *mut u64) -> c_int;
        pub fn x3_corpus_entries_dev(corpus: *const x3_corpus, d_entries: *mut *const x3_corpus_entry) -> c_int;
        pub fn x3_corpus_windows_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32, d_starts: *const u64,
                                     n_windows: u64, window_len: u32, d_out: *mut c_void, out_format: c_int, d_status: *mut i32) -> c_int;
        pub fn x3_corpus_ranges_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32, d_starts: *const u64,
                                    d_lens: *const u32, n_ranges: u64, row_stride: u64, d_out: *mut c_void, out_cap: u64,
                                    out_format: c_int, d_out_offsets: *mut u64, d_status: *mut i32) -> c_int;
        pub fn x3_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                             d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                             seg_blocks: u32, bin_len: u64, d_levels: *mut x3_level, n_bins: u64, d_frame_status: *mut i32) -> c_int;
        pub fn x3_levels_result(ctx: *mut x3_ctx, n_bad_frames: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int) -> c_int;
        pub fn x3_corpus_levels_rows(corpus: *const x3_corpus, bin_len: u64, row_first: *mut u64) -> c_int;
        pub fn x3_corpus_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, bin_len: u64, d_levels: *mut x3_level, n_rows: u64,
                                    d_frame_status: *mut i32) -> c_int;
        pub fn x3_signal_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                    d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                    seg_blocks: u32, bin_len: u64, d_levels: *mut x3_level, n_bins: u64, d_frame_status: *mut i32,
                                    signal: c_int) -> c_int;
        pub fn x3_corpus_signal_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, bin_len: u64, d_levels: *mut x3_level,
                                           n_rows: u64, d_frame_status: *mut i32, signal: c_int) -> c_int;
        pub fn x3_fir_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                 d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                 seg_blocks: u32, bin_len: u64, d_levels: *mut x3_level, n_bins: u64, d_frame_status: *mut i32,
                                 fir: *const x3_level_fir) -> c_int;
        pub fn x3_corpus_fir_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, bin_len: u64, d_levels: *mut x3_level,
                                        n_rows: u64, d_frame_status: *mut i32, fir: *const x3_level_fir) -> c_int;
        pub fn x3_tone_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                  d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                  seg_blocks: u32, bin_len: u64, d_levels: *mut x3_tone_level, n_bins: u64,
                                  d_frame_status: *mut i32, tone: *const x3_level_tone) -> c_int;
        pub fn x3_corpus_tone_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, bin_len: u64, d_levels: *mut x3_tone_level,
                                         n_rows: u64, d_frame_status: *mut i32, tone: *const x3_level_tone) -> c_int;
        pub fn x3_tone_bank_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                       d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                       seg_blocks: u32, bin_len: u64, d_levels: *mut x3_tone_level, n_bins: u64,
                                       d_frame_status: *mut i32, bank: *const x3_level_tone_bank) -> c_int;
        pub fn x3_corpus_tone_bank_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, bin_len: u64, d_levels: *mut x3_tone_level,
                                              n_rows: u64, d_frame_status: *mut i32, bank: *const x3_level_tone_bank) -> c_int;
        pub fn x3_tone_power_levels_dev(ctx: *mut x3_ctx, d_tone: *const x3_tone_level, n_rows: u64, d_levels: *mut x3_level) -> c_int;
        pub fn x3_events_dev(ctx: *mut x3_ctx, d_levels: *const x3_level, n_bins: u64, bin_len: u64, d_total: *const u64,
                             rule: *const x3_event_rule, d_starts: *mut u64, d_lens: *mut u32, d_event_levels: *mut x3_level,
                             cap: u64, d_count: *mut u64) -> c_int;
        pub fn x3_corpus_events_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_levels: *const x3_level, n_rows: u64, bin_len: u64,
                                    rule: *const x3_event_rule, d_entries: *mut u32, d_starts: *mut u64, d_lens: *mut u32,
                                    d_event_levels: *mut x3_level, cap: u64, d_count: *mut u64) -> c_int;
        pub fn x3_events_result(ctx: *mut x3_ctx, count: *mut u64) -> c_int;
        pub fn x3_level_quantiles_dev(ctx: *mut x3_ctx, d_levels: *const x3_level, n_bins: u64, bin_len: u64, d_total: *const u64,
                                      key: c_int, q_ppm: *const u32, n_q: u32, d_values: *mut u32, d_counted: *mut u32) -> c_int;
        pub fn x3_corpus_level_quantiles_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_levels: *const x3_level, n_rows: u64,
                                             bin_len: u64, key: c_int, q_ppm: *const u32, n_q: u32, d_values: *mut u32,
                                             d_counted: *mut u32) -> c_int;
        pub fn x3_level_quantiles_result(ctx: *mut x3_ctx, n_empty: *mut u64, first_empty: *mut u64) -> c_int;
        pub fn x3_level_thresholds_dev(ctx: *mut x3_ctx, d_levels: *const x3_level, n_bins: u64, bin_len: u64, d_total: *const u64,
                                       rule: *const x3_threshold_rule, d_thr: *mut x3_event_threshold) -> c_int;
        pub fn x3_corpus_level_thresholds_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_levels: *const x3_level, n_rows: u64,
                                              bin_len: u64, rule: *const x3_threshold_rule, d_thr: *mut x3_event_threshold) -> c_int;
        pub fn x3_events_adaptive_dev(ctx: *mut x3_ctx, d_levels: *const x3_level, n_bins: u64, bin_len: u64, d_total: *const u64,
                                      rule: *const x3_event_rule, d_thr: *const x3_event_threshold, d_starts: *mut u64,
                                      d_lens: *mut u32, d_event_levels: *mut x3_level, cap: u64, d_count: *mut u64) -> c_int;
        pub fn x3_corpus_events_adaptive_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_levels: *const x3_level, n_rows: u64,
                                             bin_len: u64, rule: *const x3_event_rule, d_thr: *const x3_event_threshold,
                                             d_entries: *mut u32, d_starts: *mut u64, d_lens: *mut u32,
                                             d_event_levels: *mut x3_level, cap: u64, d_count: *mut u64) -> c_int;
        pub fn x3_plane_events_dev(ctx: *mut x3_ctx, d_levels: *const x3_level, plane_stride: u64, n_bins: u64, bin_len: u64,
                                   d_total: *const u64, rule: *const x3_plane_event_rule, d_thr: *const x3_event_threshold,
                                   d_starts: *mut u64, d_lens: *mut u32, d_event_planes: *mut u32,
                                   d_event_levels: *mut x3_level, cap: u64, d_count: *mut u64) -> c_int;
        pub fn x3_corpus_plane_events_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_levels: *const x3_level, plane_stride: u64,
                                          n_rows: u64, bin_len: u64, rule: *const x3_plane_event_rule,
                                          d_thr: *const x3_event_threshold, d_entries: *mut u32, d_starts: *mut u64,
                                          d_lens: *mut u32, d_event_planes: *mut u32, d_event_levels: *mut x3_level, cap: u64,
                                          d_count: *mut u64) -> c_int;
        pub fn x3_range_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                   d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                   seg_blocks: u32, d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                   row_stride: u64, d_levels: *mut x3_level, rows_cap: u64, d_row_offsets: *mut u64,
                                   d_status: *mut i32) -> c_int;
        pub fn x3_corpus_range_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32, d_starts: *const u64,
                                          d_lens: *const u32, n_ranges: u64, bin_len: u64, row_stride: u64, d_levels: *mut x3_level,
                                          rows_cap: u64, d_row_offsets: *mut u64, d_status: *mut i32) -> c_int;
        pub fn x3_signal_range_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                          d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                          seg_blocks: u32, d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                          row_stride: u64, d_levels: *mut x3_level, rows_cap: u64, d_row_offsets: *mut u64,
                                          d_status: *mut i32, signal: c_int) -> c_int;
        pub fn x3_corpus_signal_range_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32,
                                                 d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                                 row_stride: u64, d_levels: *mut x3_level, rows_cap: u64, d_row_offsets: *mut u64,
                                                 d_status: *mut i32, signal: c_int) -> c_int;
        pub fn x3_fir_range_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                       d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                       seg_blocks: u32, d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                       row_stride: u64, d_levels: *mut x3_level, rows_cap: u64, d_row_offsets: *mut u64,
                                       d_status: *mut i32, fir: *const x3_level_fir) -> c_int;
        pub fn x3_corpus_fir_range_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32,
                                              d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                              row_stride: u64, d_levels: *mut x3_level, rows_cap: u64, d_row_offsets: *mut u64,
                                              d_status: *mut i32, fir: *const x3_level_fir) -> c_int;
        pub fn x3_tone_range_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                        d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params, d_seg_index: *const u64,
                                        seg_blocks: u32, d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                        row_stride: u64, d_levels: *mut x3_tone_level, rows_cap: u64, d_row_offsets: *mut u64,
                                        d_status: *mut i32, tone: *const x3_level_tone) -> c_int;
        pub fn x3_corpus_tone_range_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32,
                                               d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                               row_stride: u64, d_levels: *mut x3_tone_level, rows_cap: u64,
                                               d_row_offsets: *mut u64, d_status: *mut i32, tone: *const x3_level_tone) -> c_int;
        pub fn x3_tone_bank_range_levels_dev(ctx: *mut x3_ctx, d_x3: *const u8, x3_len: u64, d_frame_offsets: *const u64,
                                             d_sample_offsets: *const u64, n_frames: u64, p: *const x3_params,
                                             d_seg_index: *const u64, seg_blocks: u32, d_starts: *const u64, d_lens: *const u32,
                                             n_ranges: u64, bin_len: u64, row_stride: u64, d_levels: *mut x3_tone_level,
                                             rows_cap: u64, d_row_offsets: *mut u64, d_status: *mut i32,
                                             bank: *const x3_level_tone_bank) -> c_int;
        pub fn x3_corpus_tone_bank_range_levels_dev(ctx: *mut x3_ctx, corpus: *const x3_corpus, d_entries: *const u32,
                                                    d_starts: *const u64, d_lens: *const u32, n_ranges: u64, bin_len: u64,
                                                    row_stride: u64, d_levels: *mut x3_tone_level, rows_cap: u64,
                                                    d_row_offsets: *mut u64, d_status: *mut i32,
                                                    bank: *const x3_level_tone_bank) -> c_int;
        pub fn x3_range_levels_result(ctx: *mut x3_ctx, n_bad: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int,
                                      total_rows: *mut u64) -> c_int;
        pub fn x3_spectra_rows_dev(ctx: *mut x3_ctx, d_samples: *const i16, samples_cap: u64, d_offsets: *const u64,
                                   d_lens: *const u32, d_in_status: *const i32, n_ranges: u64, rule: *const x3_spectra_rule,
                                   row_stride: u64, d_out: *mut c_void, rows_cap: u64, d_row_offsets: *mut u64,
                                   d_status: *mut i32) -> c_int;
        pub fn x3_spectra_levels_dev(ctx: *mut x3_ctx, d_samples: *const i16, samples_cap: u64, d_offsets: *const u64,
                                     d_lens: *const u32, d_in_status: *const i32, n_ranges: u64, rule: *const x3_spectra_rule,
                                     fold: *const x3_spectra_fold, row_stride: u64, d_levels: *mut x3_level, rows_cap: u64,
                                     d_row_offsets: *mut u64, d_status: *mut i32) -> c_int;
        pub fn x3_spectra_result(ctx: *mut x3_ctx, n_bad: *mut u64, first_bad: *mut u64, first_bad_status: *mut c_int,
                                 total_rows: *mut u64) -> c_int;
        pub fn x3_corpus_destroy(corpus: *mut x3_corpus);
        pub fn x3_place_buffers(ctx: *mut x3_ctx, d_wav: *const i16, n: u64, p: *const x3_params, d_streams: *const *mut u8,
                                n_streams: u32, cap: u64, d_frame_offsets: *mut u64, d_backs: *const *mut i16, n_backs: u32,
                                warm: u32, steps: u32, ms_per_step: *mut f64) -> c_int;
        pub fn x3_wav_to_x3a(ctx: *mut x3_ctx, wav_path: *const c_char, x3a_path: *const c_char, stats: *mut u64) -> c_int;
        // parameter tuning (not in the reference)
        pub fn x3_tune_candidate(index: u32, spf: u32, p: *mut x3_params) -> c_int;
        pub fn x3_tuner_create(ctx: *mut x3_ctx, spf: u32, t: *mut *mut x3_tuner) -> c_int;
        pub fn x3_tuner_add_dev(t: *mut x3_tuner, d_wav: *const i16, batch: *const x3_batch) -> c_int;
        pub fn x3_tuner_result(t: *mut x3_tuner, best: *mut x3_params, best_bytes: *mut u64, sizes: *mut u64) -> c_int;
        pub fn x3_tuner_max_payloads(t: *mut x3_tuner, payloads: *mut u32) -> c_int;
        pub fn x3_tuner_reset(t: *mut x3_tuner) -> c_int;
        pub fn x3_tuner_destroy(t: *mut x3_tuner);
        pub fn x3_tune(ctx: *mut x3_ctx, wav: *const i16, n: u64, spf: u32, best: *mut x3_params, best_bytes: *mut u64,
                       sizes: *mut u64) -> c_int;
        pub fn x3_x3a_encode_tuned(ctx: *mut x3_ctx, wav: *const i16, n: u64, sample_rate: u32, out: *mut u8, out_cap: u64,
                                   out_len: *mut u64, stats: *mut u64, chosen: *mut x3_params) -> c_int;
        pub fn x3_x3a_to_wav(ctx: *mut x3_ctx, x3a_path: *const c_char, wav_path: *const c_char, n_samples: *mut u64,
                             frame_errors: *mut u64) -> c_int;
        pub fn x3_reader_open(ctx: *mut x3_ctx, x3a_path: *const c_char, reader: *mut *mut x3_reader) -> c_int;
        pub fn x3_reader_spec(reader: *const x3_reader, sample_rate: *mut u32, p: *mut x3_params, channels: *mut u8) -> c_int;
        pub fn x3_reader_next_frame(reader: *mut x3_reader, wav: *mut i16, wav_cap: u64, n_out: *mut u64) -> c_int;
        pub fn x3_reader_frame_errors(reader: *const x3_reader) -> u64;
        pub fn x3_reader_close(reader: *mut x3_reader);
    }
}

pub mod error {
    //! `error::X3Error` with the reference's variants in the reference's order (src/error.rs:27-62), then the two
    //! codes the C ABI adds: `Hip` (a HIP call failed) and `BadArg` (the reference would have panicked).
    use crate::bitpacker::BitPackError;

    pub type Result<T> = core::result::Result<T, X3Error>;

    #[derive(Debug)]
    pub enum X3Error {
        Io(std::io::Error),
        Hound(hound::Error),
        BitPack(BitPackError),

        InvalidEncodingThresh,
        OutOfBoundsInverse,
        MoreThanOneChannel,

        ArchiveHeaderXMLInvalid,
        ArchiveHeaderXMLRiceCode,
        ArchiveHeaderXMLInvalidKey,

        FrameLength,

        FrameHeaderInvalidKey,
        FrameHeaderInvalidPayloadLen,
        FrameHeaderInvalidHeaderCRC,
        FrameHeaderInvalidPayloadCRC,

        FrameDecodeInvalidBlockLength,
        FrameDecodeInvalidIndex,
        FrameDecodeInvalidNTOGO,
        FrameDecodeInvalidFType,
        FrameDecodeInvalidRiceCode,
        FrameDecodeInvalidBPF,
        FrameDecodeUnexpectedEnd,

        ByteWriterInsufficientMemory,

        Hip,
        BadArg,
    }

    impl From<std::io::Error> for X3Error {
        fn from(err: std::io::Error) -> X3Error {
            X3Error::Io(err)
        }
    }
    impl From<hound::Error> for X3Error {
        fn from(err: hound::Error) -> X3Error {
            X3Error::Hound(err)
        }
    }
    impl From<BitPackError> for X3Error {
        fn from(err: BitPackError) -> X3Error {
            X3Error::BitPack(err)
        }
    }

    /// C ABI status (include/x3hip.h:30-61) -> X3Error; the payload-carrying variants get a generic payload
    pub(crate) fn from_status(rc: i32) -> X3Error {
        use X3Error::*;
        match rc {
            1 => Io(std::io::Error::new(std::io::ErrorKind::Other, "libx3hip: file I/O failed")),
            2 => Hound(hound::Error::FormatError("libx3hip: not a 16-bit PCM RIFF/WAVE file")),
            3 => BitPack(BitPackError::ArrayEndReached),
            4 => InvalidEncodingThresh,
            5 => OutOfBoundsInverse,
            6 => MoreThanOneChannel,
            7 => ArchiveHeaderXMLInvalid,
            8 => ArchiveHeaderXMLRiceCode,
            9 => ArchiveHeaderXMLInvalidKey,
            10 => FrameLength,
            11 => FrameHeaderInvalidKey,
            12 => FrameHeaderInvalidPayloadLen,
            13 => FrameHeaderInvalidHeaderCRC,
            14 => FrameHeaderInvalidPayloadCRC,
            15 => FrameDecodeInvalidBlockLength,
            16 => FrameDecodeInvalidIndex,
            17 => FrameDecodeInvalidNTOGO,
            18 => FrameDecodeInvalidFType,
            19 => FrameDecodeInvalidRiceCode,
            20 => FrameDecodeInvalidBPF,
            21 => FrameDecodeUnexpectedEnd,
            22 => ByteWriterInsufficientMemory,
            23 => Hip,
            _ => BadArg,
        }
    }
    pub(crate) fn check(rc: i32) -> Result<()> {
        if rc == 0 { Ok(()) } else { Err(from_status(rc)) }
    }
}

pub mod gpu {
    //! The device handle behind the reference-shaped functions.
    use crate::error::{self, X3Error};
    use crate::ffi;
    use std::sync::{Mutex, OnceLock};

    /// One GPU + stream + scratch (`x3_ctx`).
    pub struct Gpu(*mut ffi::x3_ctx);
    // the context is only ever used by one thread at a time (the default one sits behind a Mutex)
    unsafe impl Send for Gpu {}

    impl Gpu {
        pub fn new(device: i32) -> error::Result<Self> {
            let mut p = core::ptr::null_mut();
            error::check(unsafe { ffi::x3_ctx_create(device, &mut p) })?;
            Ok(Gpu(p))
        }
        pub fn raw(&self) -> *mut ffi::x3_ctx {
            self.0
        }
    }
    impl Drop for Gpu {
        fn drop(&mut self) {
            unsafe { ffi::x3_ctx_destroy(self.0) }
        }
    }

    static DEFAULT: OnceLock<Result<Mutex<Gpu>, i32>> = OnceLock::new();

    /// Run `f` on the process-wide context.  `Err(X3Error::Hip)` when there is no usable HIP device.
    pub fn with_default<T>(f: impl FnOnce(&Gpu) -> error::Result<T>) -> error::Result<T> {
        let slot = DEFAULT.get_or_init(|| {
            let device = std::env::var("X3HIP_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            let mut p = core::ptr::null_mut();
            match unsafe { ffi::x3_ctx_create(device, &mut p) } {
                0 => Ok(Mutex::new(Gpu(p))),
                rc => Err(rc),
            }
        });
        match slot {
            Ok(m) => f(&m.lock().unwrap_or_else(|e| e.into_inner())),
            Err(_) => Err(X3Error::Hip),
        }
    }
}

pub mod x3 {
    //! src/x3.rs
    use crate::error::{self, X3Error};
    use crate::ffi;
    use std::sync::OnceLock;

    /// src/x3.rs:24-27
    pub struct Decoder<'a> {
        pub channels: &'a [Channel<'a>],
        pub x3_inp: &'a mut [u8],
    }

    /// src/x3.rs:29-45
    pub struct Channel<'a> {
        pub id: u16,
        pub wav: &'a [i16],
        pub sample_rate: u32,
        pub params: Parameters,
    }
    impl<'a> Channel<'a> {
        pub fn new(id: u16, wav: &'a [i16], sample_rate: u32, params: Parameters) -> Self {
            Channel { id, wav, sample_rate, params }
        }
    }

    /// src/x3.rs:47-69
    pub struct IterChannel<I>
    where
        I: Iterator<Item = i16>,
    {
        pub id: u16,
        pub wav: I,
        pub sample_rate: u32,
        pub params: Parameters,
    }
    impl<I> IterChannel<I>
    where
        I: Iterator<Item = i16>,
    {
        pub fn new(id: u16, wav: impl IntoIterator<IntoIter = I>, sample_rate: u32, params: Parameters) -> Self {
            IterChannel { id, wav: wav.into_iter(), sample_rate, params }
        }
    }

    /// src/x3.rs:70-79
    pub struct X3aSpec {
        pub sample_rate: u32,
        pub params: Parameters,
        pub channels: u8,
    }

    /// src/x3.rs:81-88
    pub struct Parameters {
        pub block_len: usize,
        pub blocks_per_frame: usize,
        pub codes: [usize; 3],
        pub thresholds: [usize; 3],
        pub rice_codes: [&'static RiceCode; 3],
    }
    impl Parameters {
        pub const MAX_BLOCK_LENGTH: usize = 60;
        pub const WAV_BIT_SIZE: usize = 16;

        pub const DEFAULT_BLOCK_LENGTH: usize = 20;
        pub const DEFAULT_RICE_CODES: [usize; 3] = [0, 1, 3];
        pub const DEFAULT_THRESHOLDS: [usize; 3] = [3, 8, 20];
        pub const DEFAULT_BLOCKS_PER_FRAME: usize = 500;

        /// src/x3.rs:98-122: `InvalidEncodingThresh` if thresholds[k] > offset of code k for k = 0, 1; a code
        /// number > 3 panics on the table index, as in the reference
        pub fn new(block_len: usize, blocks_per_frame: usize, codes: [usize; 3], thresholds: [usize; 3])
                   -> Result<Self, X3Error> {
            let rice_codes = RiceCodes::get(codes);
            for k in 0..2 {
                if thresholds[k] > rice_codes[k].offset {
                    return Err(X3Error::InvalidEncodingThresh);
                }
            }
            Ok(Parameters { block_len, blocks_per_frame, codes, thresholds, rice_codes })
        }

        /// the C ABI's x3_params; values that do not fit 32 bits are `BadArg` (the kernels index with 32 bits)
        pub(crate) fn c(&self) -> error::Result<ffi::x3_params> {
            let n = |v: usize| u32::try_from(v).map_err(|_| X3Error::BadArg);
            Ok(ffi::x3_params {
                block_len: n(self.block_len)?,
                blocks_per_frame: n(self.blocks_per_frame)?,
                codes: [n(self.codes[0])?, n(self.codes[1])?, n(self.codes[2])?],
                thresholds: [n(self.thresholds[0])?, n(self.thresholds[1])?, n(self.thresholds[2])?],
            })
        }
        pub(crate) fn from_c(c: &ffi::x3_params) -> Self {
            let codes = [c.codes[0] as usize, c.codes[1] as usize, c.codes[2] as usize];
            Parameters {
                block_len: c.block_len as usize,
                blocks_per_frame: c.blocks_per_frame as usize,
                codes,
                thresholds: [c.thresholds[0] as usize, c.thresholds[1] as usize, c.thresholds[2] as usize],
                rice_codes: RiceCodes::get(codes),
            }
        }
    }
    impl Default for Parameters {
        fn default() -> Self {
            Parameters {
                block_len: Self::DEFAULT_BLOCK_LENGTH,
                blocks_per_frame: Self::DEFAULT_BLOCKS_PER_FRAME,
                codes: Self::DEFAULT_RICE_CODES,
                thresholds: Self::DEFAULT_THRESHOLDS,
                rice_codes: RiceCodes::get(Self::DEFAULT_RICE_CODES),
            }
        }
    }

    /// src/x3.rs:136-141
    pub struct Archive {}
    impl Archive {
        pub const ID: &'static [u8] = b"X3ARCHIV";
        pub const ID_LEN: usize = 8;
    }
    /// src/x3.rs:143-146
    pub struct Frame {}
    impl Frame {
        pub const MAX_LENGTH: usize = 0x7fe0;
    }
    /// src/x3.rs:148-184
    #[derive(Debug)]
    pub struct FrameHeader {
        pub source_id: u8,
        pub samples: u16,
        pub channels: u8,
        pub payload_len: usize,
        pub payload_crc: u16,
    }
    impl FrameHeader {
        pub const LENGTH: usize = 20;
        pub const KEY: u16 = 30771;
        pub const KEY_BUF: &'static [u8] = b"x3";
        pub const P_KEY: usize = 0;
        pub const P_SOURCE_ID: usize = 2;
        pub const P_CHANNELS: usize = 3;
        pub const P_SAMPLES: usize = 4;
        pub const P_PAYLOAD_SIZE: usize = 6;
        pub const P_TIME: usize = 8;
        pub const P_HEADER_CRC: usize = 16;
        pub const P_PAYLOAD_CRC: usize = 18;
    }

    /// src/x3.rs:187-194; the tables are the library's (x3_rice_code_get), static for the life of the process
    #[allow(dead_code)]
    pub struct RiceCode {
        pub nsubs: usize,
        pub offset: usize,
        pub code: &'static [usize],
        pub num_bits: &'static [usize],
        pub inv: &'static [i16],
        pub inv_len: usize,
    }
    /// src/x3.rs:196-260
    pub struct RiceCodes {}
    impl RiceCodes {
        fn table() -> &'static [RiceCode; 4] {
            static CODE: OnceLock<[RiceCode; 4]> = OnceLock::new();
            CODE.get_or_init(|| {
                core::array::from_fn(|k| {
                    let mut c = core::mem::MaybeUninit::<ffi::x3_rice_code>::uninit();
                    let rc = unsafe { ffi::x3_rice_code_get(k as u32, c.as_mut_ptr()) };
                    assert_eq!(rc, 0);
                    let c = unsafe { c.assume_init() };
                    let widen = |p: *const u32| -> &'static [usize] {
                        let s = unsafe { core::slice::from_raw_parts(p, c.len as usize) };
                        Box::leak(s.iter().map(|&v| v as usize).collect::<Vec<usize>>().into_boxed_slice())
                    };
                    RiceCode {
                        nsubs: c.nsubs as usize,
                        offset: c.offset as usize,
                        code: widen(c.code),
                        num_bits: widen(c.num_bits),
                        inv: unsafe { core::slice::from_raw_parts(c.inv, 60) },
                        inv_len: c.inv_len as usize,
                    }
                })
            })
        }
        pub fn get(code_list: [usize; 3]) -> [&'static RiceCode; 3] {
            let t = Self::table();
            [&t[code_list[0]], &t[code_list[1]], &t[code_list[2]]]
        }
    }
}

pub mod bytewriter {
    //! The crate's byte sinks.  The `ByteWriter` trait is the crate's public interface (five methods, src/bytewriter.rs:
    //! 14-22) and is repeated here so that this mirror compiles on its own; a maintainer who wires the FFI into the crate
    //! keeps the crate's own `src/bytewriter.rs` and drops this module.  The two sinks below are written
    //! for this mirror -- same observable behaviour: zero padding to an absolute position, `ByteWriterInsufficientMemory`
    //! when a slice is too short -- with one hidden, provided method added, through which the encoder hands a slice sink's
    //! memory to the library without an intermediate copy.
    use crate::error::{Result, X3Error};
    pub use std::io::{Seek, SeekFrom, Write};

    pub trait ByteWriter {
        fn align<const N: usize>(&mut self) -> Result<usize>;
        fn write_all(&mut self, value: impl AsRef<[u8]>) -> Result<()>;
        fn flush(&mut self) -> Result<()>;
        fn seek(&mut self, pos: SeekFrom) -> Result<u64>;
        fn stream_position(&mut self) -> Result<u64>;

        /// the whole backing memory of a slice sink (None for everything else)
        #[doc(hidden)]
        fn __x3hip_backing_slice(&mut self) -> Option<&mut [u8]> {
            None
        }
    }

    /// bytes missing from `at` to the next multiple of `n`
    fn gap(at: u64, n: usize) -> usize {
        let n = n as u64;
        ((n - at % n) % n) as usize
    }

    /// A sink over caller-owned memory: a cursor and the furthest byte ever written.
    pub struct SliceByteWriter<'a> {
        buf: &'a mut [u8],
        cursor: usize,
        high_water: usize,
    }

    impl<'a> SliceByteWriter<'a> {
        pub fn new(slice: &'a mut [u8]) -> Self {
            Self { buf: slice, cursor: 0, high_water: 0 }
        }

        /// the window [cursor, cursor + n) if the memory reaches that far
        fn claim(&mut self, n: usize) -> Result<&mut [u8]> {
            let end = self.cursor.checked_add(n).filter(|&e| e <= self.buf.len());
            match end {
                None => Err(X3Error::ByteWriterInsufficientMemory),
                Some(end) => {
                    let w = &mut self.buf[self.cursor..end];
                    self.cursor = end;
                    self.high_water = self.high_water.max(end);
                    Ok(w)
                }
            }
        }
    }

    impl<'a> ByteWriter for SliceByteWriter<'a> {
        fn align<const N: usize>(&mut self) -> Result<usize> {
            let pad = gap(self.cursor as u64, N);
            self.claim(pad)?.fill(0);
            Ok(pad)
        }

        fn write_all(&mut self, value: impl AsRef<[u8]>) -> Result<()> {
            let bytes = value.as_ref();
            self.claim(bytes.len())?.copy_from_slice(bytes);
            Ok(())
        }

        fn flush(&mut self) -> Result<()> {
            Ok(())
        }

        fn seek(&mut self, pos: SeekFrom) -> Result<u64> {
            // (a target in front of the memory wraps to a huge number, as `as usize` does in the crate: "insufficient")
            let target = match pos {
                SeekFrom::Start(to) => to as usize,
                SeekFrom::Current(by) => (self.cursor as i64).wrapping_add(by) as usize,
                SeekFrom::End(by) => (self.high_water as i64).wrapping_add(by) as usize,
            };
            if target > self.buf.len() {
                return Err(X3Error::ByteWriterInsufficientMemory);
            }
            self.cursor = target;
            self.high_water = self.high_water.max(target);
            Ok(target as u64)
        }

        fn stream_position(&mut self) -> Result<u64> {
            Ok(self.cursor as u64)
        }

        fn __x3hip_backing_slice(&mut self) -> Option<&mut [u8]> {
            Some(&mut *self.buf)
        }
    }

    /// A sink over anything that is `Write + Seek` (a file, a cursor): every call is the inner writer's.
    pub struct StreamByteWriter<'a, W: Write + Seek> {
        inner: &'a mut W,
    }

    impl<'a, W: Write + Seek> StreamByteWriter<'a, W> {
        pub fn new(writer: &'a mut W) -> Self {
            Self { inner: writer }
        }
    }

    impl<'a, W: Write + Seek> ByteWriter for StreamByteWriter<'a, W> {
        fn align<const N: usize>(&mut self) -> Result<usize> {
            let pad = gap(self.inner.stream_position()?, N);
            for _ in 0..pad {
                self.inner.write_all(&[0u8])?;
            }
            Ok(pad)
        }

        fn write_all(&mut self, value: impl AsRef<[u8]>) -> Result<()> {
            Ok(self.inner.write_all(value.as_ref())?)
        }

        fn flush(&mut self) -> Result<()> {
            Ok(self.inner.flush()?)
        }

        fn seek(&mut self, pos: SeekFrom) -> Result<u64> {
            Ok(self.inner.seek(pos)?)
        }

        fn stream_position(&mut self) -> Result<u64> {
            Ok(self.inner.stream_position()?)
        }
    }
}

pub mod crc {
    //! src/crc.rs
    use crate::{error, ffi, gpu};

    /// src/crc.rs:44-47
    pub fn update_crc16(crc: u16, data: &u8) -> u16 {
        unsafe { ffi::x3_crc16_update(crc, *data) }
    }
    /// src/crc.rs:49-58, computed on the GPU (segmented reduction).  The reference's signature has no error
    /// path: a HIP failure panics.
    pub fn crc16(data: &[u8]) -> u16 {
        gpu::with_default(|g| crc16_on(g, data)).expect("x3::crc::crc16: no usable HIP device")
    }
    pub fn crc16_on(gpu: &gpu::Gpu, data: &[u8]) -> error::Result<u16> {
        let mut c = 0u16;
        error::check(unsafe { ffi::x3_crc16(gpu.raw(), data.as_ptr(), data.len() as u64, &mut c) })?;
        Ok(c)
    }
}

pub mod bitpacker {
    //! src/bitpacker.rs:36-190.  Fields are recorded in the library and packed by a kernel (scan of the widths,
    //! fields OR-ed into place) when the packer flushes: on `word_align`, `inc_counter_n_bytes` and Drop, where the
    //! reference has handed every complete byte to the writer too.  `len()` / `crc()` are the reference's values
    //! between writes.  The frame encoder does not go through this type.
    use crate::bytewriter::{ByteWriter, SeekFrom};
    use crate::error::{self, Result, X3Error};
    use crate::{ffi, gpu};

    #[derive(Debug)]
    pub enum BitPackError {
        NotByteAligned,
        BoundaryReached,
        ArrayEndReached,
        ExceededBitBoundary,
    }

    pub struct BitPacker<'a, W: ByteWriter> {
        writer: &'a mut W,
        bp: *mut ffi::x3_bitpacker, // unbound packer (out = NULL): bytes come back through x3_bitpacker_take
        bits: usize,                // bits written since new()
        handed: usize,              // bytes the writer already has
    }

    impl<'a, W: ByteWriter> Drop for BitPacker<'a, W> {
        fn drop(&mut self) {
            if self.bits % 8 != 0 || self.bits / 8 > self.handed {
                let _ = self.flush();
            }
            unsafe { ffi::x3_bitpacker_free(self.bp) };
        }
    }

    impl<'a, W: ByteWriter> BitPacker<'a, W> {
        pub fn new(writer: &'a mut W) -> BitPacker<'a, W> {
            // word_align pads to an even ABSOLUTE writer position: the library needs the position at new()
            let start = writer.stream_position().unwrap_or(0);
            let mut bp = core::ptr::null_mut();
            gpu::with_default(|g| {
                error::check(unsafe { ffi::x3_bitpacker_new(g.raw(), core::ptr::null_mut(), 0, start, &mut bp) })
            })
            .expect("x3::bitpacker::BitPacker::new: no usable HIP device");
            BitPacker { writer, bp, bits: 0, handed: 0 }
        }

        pub fn crc(&self) -> u16 {
            let mut c = 0xffffu16;
            gpu::with_default(|_| error::check(unsafe { ffi::x3_bitpacker_peek(self.bp, core::ptr::null_mut(), &mut c) }))
                .expect("x3::bitpacker::BitPacker::crc: HIP error");
            c
        }

        /// flush (src/bitpacker.rs:79-86): a partial byte is zero-padded; every byte the writer does not have yet is
        /// packed on the GPU and written
        fn flush(&mut self) -> Result<()> {
            let pending = (self.bits + 7) / 8 - self.handed;
            let mut buf = vec![0u8; pending];
            let mut n_new = 0u64;
            gpu::with_default(|_| {
                error::check(unsafe {
                    ffi::x3_bitpacker_take(self.bp, buf.as_mut_ptr(), buf.len() as u64, &mut n_new,
                                           core::ptr::null_mut(), core::ptr::null_mut())
                })
            })?;
            self.bits = (self.bits + 7) & !7;
            self.handed += n_new as usize;
            self.writer.write_all(&buf[..n_new as usize])
        }

        pub fn len(&self) -> usize {
            self.bits / 8
        }

        pub fn write_bytes(&mut self, array: &[u8]) -> Result<()> {
            // src/bitpacker.rs:95-102: the array reaches the writer at once, in front of a partial byte that is still
            // in the packer -- x3_bitpacker_write_bytes keeps that order
            error::check(unsafe { ffi::x3_bitpacker_write_bytes(self.bp, array.as_ptr(), array.len() as u64) })?;
            self.bits += 8 * array.len();
            Ok(())
        }

        pub fn inc_counter_n_bytes(&mut self, n_bytes: usize) -> Result<()> {
            if self.bits % 8 != 0 {
                return Err(X3Error::BitPack(BitPackError::NotByteAligned));
            }
            self.flush()?;
            self.writer.seek(SeekFrom::Current(n_bytes as i64))?;
            Ok(())
        }

        pub fn word_align(&mut self) -> Result<()> {
            error::check(unsafe { ffi::x3_bitpacker_word_align(self.bp) })?;
            let mut len = 0u64;
            error::check(unsafe { ffi::x3_bitpacker_peek(self.bp, &mut len, core::ptr::null_mut()) })?;
            self.bits = len as usize * 8;
            self.flush()
        }

        pub fn write_bits(&mut self, value: usize, num_bits: usize) -> Result<()> {
            let n = u32::try_from(num_bits).map_err(|_| X3Error::BadArg)?;
            error::check(unsafe { ffi::x3_bitpacker_write_bits(self.bp, value as u64, n) })?;
            self.bits += num_bits;
            Ok(())
        }

        pub fn write_packed_zeros(&mut self, num_zeros: usize) -> Result<()> {
            let n = u32::try_from(num_zeros).map_err(|_| X3Error::BadArg)?;
            error::check(unsafe { ffi::x3_bitpacker_write_packed_zeros(self.bp, n) })?;
            self.bits += num_zeros;
            Ok(())
        }
    }
}

pub mod bitreader {
    //! src/bitreader.rs:51-176.  The array and the reader's state (idx, leading_word, rem_bit) live in device
    //! memory; each call runs the reference-exact reader there, reads past the end and the one-word peek of
    //! `count_zero_bits` included.  The frame decoders do not go through this type (they keep a bit window per
    //! lane in registers); it exists for callers of the reference's building blocks.
    use crate::{error, ffi, gpu};
    use core::marker::PhantomData;

    pub struct BitReader<'a> {
        pub(crate) br: *mut ffi::x3_bitreader,
        _array: PhantomData<&'a [u8]>,
    }

    impl<'a> Drop for BitReader<'a> {
        fn drop(&mut self) {
            unsafe { ffi::x3_bitreader_free(self.br) }
        }
    }

    impl<'a> BitReader<'a> {
        pub fn new(array: &'a [u8]) -> Self {
            let mut br = core::ptr::null_mut();
            gpu::with_default(|g| {
                error::check(unsafe { ffi::x3_bitreader_new(g.raw(), array.as_ptr(), array.len() as u64, &mut br) })
            })
            .expect("x3::bitreader::BitReader::new: no usable HIP device");
            BitReader { br, _array: PhantomData }
        }

        pub fn inc_bits(&mut self, n: usize) {
            gpu::with_default(|_| error::check(unsafe { ffi::x3_bitreader_inc_bits(self.br, n as u32) }))
                .expect("x3::bitreader::BitReader::inc_bits");
        }

        pub fn read_nbits(&mut self, n: usize) -> u32 {
            let mut v = 0u32;
            gpu::with_default(|_| error::check(unsafe { ffi::x3_bitreader_read_nbits(self.br, n as u32, &mut v) }))
                .expect("x3::bitreader::BitReader::read_nbits");
            v
        }

        pub fn count_zero_bits(&mut self) -> usize {
            let mut v = 0u32;
            gpu::with_default(|_| error::check(unsafe { ffi::x3_bitreader_count_zero_bits(self.br, &mut v) }))
                .expect("x3::bitreader::BitReader::count_zero_bits");
            v as usize
        }
    }
}

pub mod encoder {
    //! src/encoder.rs
    use crate::bytewriter::ByteWriter;
    use crate::error::{self, X3Error};
    use crate::{ffi, gpu, x3};
    use std::cell::Cell;

    thread_local! {
        static LAST_STATS: Cell<[usize; 6]> = const { Cell::new([0; 6]) };
    }
    /// Block counts by type (Rice-0, Rice-1, Rice-2, Rice-3, BFP, pass-through) of this thread's last `encode`:
    /// what the reference prints under `std` (src/encoder.rs:96-108) and otherwise drops.
    pub fn last_statistics() -> [usize; 6] {
        LAST_STATS.with(|s| s.get())
    }

    /// `encoder::encode` (src/encoder.rs:51-111).  The sample iterator is drained, the whole stream is produced
    /// by one GPU dispatch; frames, padding and bytes are those of the reference's frame loop.
    pub fn encode<'a, I, W: ByteWriter>(channels: &mut [&mut x3::IterChannel<I>], writer: &mut W) -> Result<(), X3Error>
    where
        I: Iterator<Item = i16>,
    {
        if channels.len() > 1 {
            return Err(X3Error::MoreThanOneChannel);
        }
        let ch = &mut channels[0];
        let wav: Vec<i16> = ch.wav.by_ref().collect();
        let mut stats = [0usize; 6];
        gpu::with_default(|g| encode_samples(g, &wav, writer, &ch.params, &mut stats, false))?;
        LAST_STATS.with(|s| s.set(stats));
        #[cfg(feature = "std")]
        {
            let total: f32 = stats.iter().sum::<usize>() as f32;
            println!("");
            println!("Statistics:");
            println!("  Rice-0: {:.4}%", (stats[0] as f32 / total) * 100.0);
            println!("  Rice-1: {:.4}%", (stats[1] as f32 / total) * 100.0);
            println!("  Rice-2: {:.4}%", (stats[2] as f32 / total) * 100.0);
            println!("  Rice-3: {:.4}%", (stats[3] as f32 / total) * 100.0);
            println!("  BFP: {:.4}%", (stats[4] as f32 / total) * 100.0);
            println!("  Pass-through {:.4}%", (stats[5] as f32 / total) * 100.0);
            println!("");
        }
        Ok(())
    }

    /// src/encoder.rs:122-162
    pub fn write_frame_header(num_samples: usize, id: u8, payload_len: usize, payload_crc: u16) -> [u8; x3::FrameHeader::LENGTH] {
        let mut h = [0u8; x3::FrameHeader::LENGTH];
        unsafe { ffi::x3_write_frame_header(num_samples as u64, id, payload_len as u64, payload_crc, h.as_mut_ptr()) };
        h
    }

    /// `encoder::encode_frame` (src/encoder.rs:175-214): one frame from `wav`, header included, at the writer's
    /// position padded to even; `stats` is added to.
    pub fn encode_frame<W: ByteWriter>(wav: &[i16], writer: &mut W, params: &x3::Parameters, stats: &mut [usize; 6])
                                       -> Result<(), X3Error> {
        gpu::with_default(|g| encode_samples(g, wav, writer, params, stats, true))
    }

    /// the same two on a context of the caller's
    pub fn encode_samples<W: ByteWriter>(gpu: &gpu::Gpu, wav: &[i16], writer: &mut W, params: &x3::Parameters,
                                         stats: &mut [usize; 6], one_frame: bool) -> Result<(), X3Error> {
        let p = params.c()?;
        let mut st = [0u64; 6];
        let mut pos = 0u64;
        let n = wav.len() as u64;
        let start = writer.stream_position()?;
        let call = |out: *mut u8, cap: u64, at: u64, pos: &mut u64, st: &mut [u64; 6]| unsafe {
            if one_frame {
                ffi::x3_encode_frame(gpu.raw(), wav.as_ptr(), n, &p, out, cap, at, pos, st.as_mut_ptr())
            } else {
                ffi::x3_encode(gpu.raw(), wav.as_ptr(), n, 1, &p, out, cap, at, pos, st.as_mut_ptr())
            }
        };
        let direct = match writer.__x3hip_backing_slice() {
            // a slice writer: the library writes into the caller's memory, behind the writer's position
            Some(slice) => Some(call(slice.as_mut_ptr(), slice.len() as u64, start, &mut pos, &mut st)),
            None => None,
        };
        match direct {
            Some(rc) => {
                // On ByteWriterInsufficientMemory the slice holds every frame that fits and *out_pos stands behind the last
                // of them (include/x3hip.h, x3_encode): the writer must stand there too before the error goes up, as the
                // reference's SliceByteWriter does after the frames it has taken (src/bytewriter.rs:86-99)
                if rc == 22 {
                    writer.seek(crate::bytewriter::SeekFrom::Start(pos))?;
                }
                error::check(rc)?;
                writer.seek(crate::bytewriter::SeekFrom::Start(pos))?;
            }
            None => {
                // any other writer: encode into a buffer that starts at the same parity, hand the bytes over
                let parity = start & 1;
                let slack = if one_frame { 3 * n + 64 } else { 64 };
                let mut buf = vec![0u8; (parity + unsafe { ffi::x3_encode_bound(n, &p) } + slack) as usize];
                error::check(call(buf.as_mut_ptr(), buf.len() as u64, parity, &mut pos, &mut st))?;
                writer.write_all(&buf[parity as usize..pos as usize])?;
            }
        }
        for k in 0..6 {
            stats[k] += st[k] as usize;
        }
        Ok(())
    }
}

pub mod decoder {
    //! src/decoder.rs
    use crate::bitreader::BitReader;
    use crate::error::{self, X3Error};
    use crate::x3::{self, FrameHeader};
    use crate::{ffi, gpu};

    /// src/decoder.rs:30-34
    pub enum FrameTest {
        IsFrame,
        EndOfBuffer,
        NotFrame,
    }

    /// `decoder::decode_frame` (src/decoder.rs:36-58): `x3_bytes` is one frame's payload, `samples` its header's
    /// sample count; `Ok(Some(samples written))`.  Loops over this function go through a frame cache in the
    /// library; whole streams belong to [`decode_stream`].
    pub fn decode_frame(x3_bytes: &mut [u8], wav_buf: &mut [i16], params: &x3::Parameters, samples: usize)
                        -> Result<Option<usize>, X3Error> {
        let p = params.c()?;
        let mut n = 0u64;
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_decode_frame(g.raw(), x3_bytes.as_ptr(), x3_bytes.len() as u64, wav_buf.as_mut_ptr(),
                                     wav_buf.len() as u64, &p, samples as u64, &mut n)
            })
        })?;
        Ok(Some(n as usize))
    }

    /// Not in the reference: announce the frame stream a loop over [`decode_frame`] is about to walk.  While the
    /// guard lives, calls whose payload lies in `x3` are served from windows of frames that are checked and decoded
    /// ahead on the GPU (a header parse and a memcpy per call) instead of one dispatch per call; the results are
    /// those of `decode_frame` alone.
    ///
    /// # Safety
    /// `decode_frame` wants `&mut [u8]` payloads, so the guard cannot hold a borrow of the buffer: the caller keeps
    /// `x3` alive and unchanged until the guard is dropped.
    pub unsafe fn prefetch(x3: &[u8], params: &x3::Parameters) -> Result<Prefetch, X3Error> {
        let p = params.c()?;
        gpu::with_default(|g| error::check(ffi::x3_decode_prefetch(g.raw(), x3.as_ptr(), x3.len() as u64, &p)))?;
        Ok(Prefetch(()))
    }
    pub struct Prefetch(());
    impl Drop for Prefetch {
        fn drop(&mut self) {
            let _ = gpu::with_default(|g| {
                error::check(unsafe { ffi::x3_decode_prefetch(g.raw(), core::ptr::null(), 0, core::ptr::null()) })
            });
        }
    }

    /// src/decoder.rs:69-118
    pub fn read_frame_header(bytes: &[u8]) -> Result<FrameHeader, X3Error> {
        let mut h = ffi::x3_frame_header::default();
        error::check(unsafe { ffi::x3_read_frame_header(bytes.as_ptr(), bytes.len() as u64, &mut h) })?;
        Ok(FrameHeader { source_id: h.source_id, samples: h.samples, channels: h.channels,
                         payload_len: h.payload_len as usize, payload_crc: h.payload_crc })
    }

    /// `decoder::decode_block` (src/decoder.rs:132-145): `wav.len()` samples from the reader's position
    pub fn decode_block(br: &mut BitReader, wav: &mut [i16], last_wav: &mut i16, params: &x3::Parameters)
                        -> Result<(), X3Error> {
        let p = params.c()?;
        let n = u32::try_from(wav.len()).map_err(|_| X3Error::BadArg)?;
        gpu::with_default(|_| error::check(unsafe { ffi::x3_decode_block(br.br, wav.as_mut_ptr(), n, last_wav, &p) }))
    }

    /// Not in the reference: the `X3aReader::decode_next_frame` loop (src/decodefile.rs:105-136, 200-209) over a
    /// frame stream in memory in one call -- (samples decoded, good frames, counted frame errors).
    pub fn decode_stream(x3: &[u8], params: &x3::Parameters, wav: &mut [i16]) -> Result<(usize, usize, usize), X3Error> {
        let p = params.c()?;
        let (mut n, mut ok, mut bad) = (0u64, 0u64, 0u64);
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_decode_stream(g.raw(), x3.as_ptr(), x3.len() as u64, &p, wav.as_mut_ptr(), wav.len() as u64,
                                      &mut n, &mut ok, &mut bad)
            })
        })?;
        Ok((n as usize, ok as usize, bad as usize))
    }
}

pub mod multichannel {
    //! Not in the reference crate, whose `encoder::encode` returns `MoreThanOneChannel` for more than one channel
    //! (src/encoder.rs:55-57) and whose reader refuses such frames (src/decoder.rs:90-94) -- as `encoder::encode` and
    //! `decoder::decode_stream` of this crate do.  The layout is the one the frame header's `<Num Channels>` and
    //! "pack the data block for each channel" (src/encoder.rs:197) foresee; include/x3hip.h, x3_mc.h.
    use crate::error::{self, X3Error};
    use crate::{ffi, gpu, x3};

    /// channels of equal length into `out[start_pos..]`; -> the writer's position behind the last frame
    pub fn encode(channels: &[&[i16]], params: &x3::Parameters, out: &mut [u8], start_pos: usize) -> Result<usize, X3Error> {
        let n = channels.first().ok_or(X3Error::BadArg)?.len();
        if channels.iter().any(|c| c.len() != n) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let ptrs: Vec<*const i16> = channels.iter().map(|c| c.as_ptr()).collect();
        let n_ch = u32::try_from(ptrs.len()).map_err(|_| X3Error::BadArg)?;
        let mut pos = 0u64;
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_encode_mc(g.raw(), ptrs.as_ptr(), n_ch, n as u64, &p, out.as_mut_ptr(), out.len() as u64,
                                  start_pos as u64, &mut pos, std::ptr::null_mut())
            })
        })?;
        Ok(pos as usize)
    }

    /// -> (samples per channel, good frames, counted frame errors); every channel slice must hold `wav_cap` samples
    pub fn decode_stream(x3: &[u8], params: &x3::Parameters, channels: &mut [&mut [i16]]) -> Result<(usize, usize, usize), X3Error> {
        let cap = channels.iter().map(|c| c.len()).min().ok_or(X3Error::BadArg)?;
        let p = params.c()?;
        let ptrs: Vec<*mut i16> = channels.iter_mut().map(|c| c.as_mut_ptr()).collect();
        let n_ch = u32::try_from(ptrs.len()).map_err(|_| X3Error::BadArg)?;
        let (mut n, mut ok, mut bad) = (0u64, 0u64, 0u64);
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_decode_stream_mc(g.raw(), x3.as_ptr(), x3.len() as u64, n_ch, &p, ptrs.as_ptr(), cap as u64, &mut n,
                                         &mut ok, &mut bad)
            })
        })?;
        Ok((n as usize, ok as usize, bad as usize))
    }
}

pub mod device {
    //! Not in the reference crate, which knows no device: samples and stream stay in HBM between encode and decode
    //! (`x3_encode_dev` / `x3_decode_dev`), optionally with the SEGMENT INDEX that lets a short stream decode on as many lanes
    //! as fill the GPU (`x3_encode_dev_seg` / `x3_decode_dev_seg`; a hint the decoder proves entry by entry).  The C++ mirror
    //! has the same module (host/x3.hpp, `x3::device`), tested in tests/host_cpp/test_x3_hpp.cpp.
    use crate::error::{self, X3Error};
    use crate::ffi;
    use crate::gpu::Gpu;
    use crate::x3;
    use std::os::raw::c_void;

    /// device memory of a context (`x3_dev_alloc`), freed with the value
    pub struct Buffer<'g> {
        gpu: &'g Gpu,
        p: *mut c_void,
        bytes: usize,
    }
    impl<'g> Buffer<'g> {
        pub fn new(gpu: &'g Gpu, bytes: usize) -> error::Result<Self> {
            let mut p = core::ptr::null_mut();
            error::check(unsafe { ffi::x3_dev_alloc(gpu.raw(), bytes as u64, &mut p) })?;
            Ok(Buffer { gpu, p, bytes })
        }
        pub fn len(&self) -> usize {
            self.bytes
        }
        pub fn is_empty(&self) -> bool {
            self.bytes == 0
        }
        pub fn as_ptr<T>(&self) -> *mut T {
            self.p as *mut T
        }
        pub fn upload<T: Copy>(&mut self, src: &[T]) -> error::Result<()> {
            let n = std::mem::size_of_val(src);
            if n > self.bytes {
                return Err(X3Error::BadArg);
            }
            error::check(unsafe { ffi::x3_dev_upload(self.gpu.raw(), self.p, src.as_ptr() as *const c_void, n as u64) })
        }
        pub fn download<T: Copy>(&self, dst: &mut [T]) -> error::Result<()> {
            let n = std::mem::size_of_val(dst);
            if n > self.bytes {
                return Err(X3Error::BadArg);
            }
            error::check(unsafe { ffi::x3_dev_download(self.gpu.raw(), dst.as_mut_ptr() as *mut c_void, self.p, n as u64) })
        }
    }
    impl Drop for Buffer<'_> {
        fn drop(&mut self) {
            unsafe { ffi::x3_dev_free(self.gpu.raw(), self.p) };
        }
    }

    /// an encoded batch in device memory: the stream, where its frames begin, and (`seg_blocks != 0`) the segment index
    pub struct EncodedStream<'g> {
        pub bytes: Buffer<'g>,
        pub frame_offsets: Buffer<'g>,
        pub seg_index: Option<Buffer<'g>>,
        pub len: usize,
        pub n_frames: usize,
        pub n_per_clip: usize,
        pub n_clips: usize,
        pub seg_blocks: u32,
        pub stats: [u64; 6],
    }

    /// `n_clips` clips of `n_per_clip` samples back to back in `d_wav`, each encoded as `encoder::encode` encodes a channel.
    /// `seg_blocks`: 0 = no index; a power of two >= 4 (32 for the default frames) = also leave the segment index.
    pub fn encode<'g>(gpu: &'g Gpu, d_wav: &Buffer<'g>, n_per_clip: usize, n_clips: usize, params: &x3::Parameters,
                      seg_blocks: u32) -> error::Result<EncodedStream<'g>> {
        if n_per_clip == 0 || n_clips == 0 || d_wav.len() < 2 * n_per_clip * n_clips {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let n_frames = unsafe { ffi::x3_num_frames(n_per_clip as u64, &p) } as usize * n_clips;
        let cap = unsafe { ffi::x3_encode_bound(n_per_clip as u64, &p) } as usize * n_clips;
        let bytes = Buffer::new(gpu, cap + 16)?;
        let frame_offsets = Buffer::new(gpu, 8 * (n_frames + 1))?;
        let n_idx = if seg_blocks != 0 { unsafe { ffi::x3_seg_index_entries(n_frames as u64, &p, seg_blocks) } as usize } else { 0 };
        let seg_index = if n_idx != 0 { Some(Buffer::new(gpu, 8 * n_idx)?) } else { None };
        let b = ffi::x3_batch { n_per_clip: n_per_clip as u64, clip_stride: n_per_clip as u64, n_clips: n_clips as u64 };
        error::check(unsafe {
            match &seg_index {
                Some(idx) => ffi::x3_encode_dev_seg(gpu.raw(), d_wav.as_ptr::<i16>(), &b, &p, bytes.as_ptr::<u8>(), cap as u64, 0,
                                                    frame_offsets.as_ptr::<u64>(), idx.as_ptr::<u64>(), seg_blocks),
                None => ffi::x3_encode_dev(gpu.raw(), d_wav.as_ptr::<i16>(), &b, &p, bytes.as_ptr::<u8>(), cap as u64, 0, frame_offsets.as_ptr::<u64>()),
            }
        })?;
        let mut pos = 0u64;
        let mut stats = [0u64; 6];
        error::check(unsafe { ffi::x3_encode_result(gpu.raw(), &mut pos, stats.as_mut_ptr()) })?;
        let seg_blocks = if seg_index.is_some() { seg_blocks } else { 0 };
        Ok(EncodedStream { bytes, frame_offsets, seg_index, len: pos as usize, n_frames, n_per_clip, n_clips, seg_blocks, stats })
    }

    /// ... and back: every clip's samples at `d_wav + clip * n_per_clip`; by the segment index when the stream has one.
    /// -> samples in front of the first frame that failed (all of them if none did); `Err` = that frame's status
    pub fn decode<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, d_wav: &mut Buffer<'g>) -> error::Result<usize> {
        let p = params.c()?;
        let b = ffi::x3_batch { n_per_clip: s.n_per_clip as u64, clip_stride: s.n_per_clip as u64, n_clips: s.n_clips as u64 };
        let wav_cap = (d_wav.len() / 2) as u64;
        error::check(unsafe {
            match &s.seg_index {
                Some(idx) => ffi::x3_decode_dev_seg(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(), s.n_frames as u64,
                                                    &b, core::ptr::null(), &p, d_wav.as_ptr::<i16>(), wav_cap, core::ptr::null_mut(),
                                                    idx.as_ptr::<u64>(), s.seg_blocks, 0),
                None => ffi::x3_decode_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(), s.n_frames as u64, &b,
                                           core::ptr::null(), &p, d_wav.as_ptr::<i16>(), wav_cap, core::ptr::null_mut()),
            }
        })?;
        let (mut first_bad, mut before, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_decode_result(gpu.raw(), &mut first_bad, &mut st, &mut before) })?;
        error::check(st)?;
        Ok(before as usize)
    }

    /// The segment index of a stream somebody else wrote (`x3_seg_index_build_dev`; not in the reference crate): a walk
    /// that stores no sample, for any block length, frame length and code set.  `d_frame_offsets`: `n_frames` byte offsets
    /// into `d_x3`.  -> the index (`None` where `seg_blocks` leaves a frame one stretch); asynchronous, it is only ever a
    /// hint and is for the window paths (`decode_windows`, `Corpus`).
    pub fn build_seg_index<'g>(gpu: &'g Gpu, d_x3: &Buffer<'g>, x3_len: usize, d_frame_offsets: &Buffer<'g>, n_frames: usize,
                               params: &x3::Parameters, seg_blocks: u32) -> error::Result<Option<Buffer<'g>>> {
        if x3_len > d_x3.len() || d_frame_offsets.len() < 8 * n_frames {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let n_idx = if seg_blocks != 0 { unsafe { ffi::x3_seg_index_entries(n_frames as u64, &p, seg_blocks) } as usize } else { 0 };
        if n_idx == 0 {
            return Ok(None);
        }
        let idx = Buffer::new(gpu, 8 * n_idx)?;
        error::check(unsafe {
            ffi::x3_seg_index_build_dev(gpu.raw(), d_x3.as_ptr::<u8>(), x3_len as u64, d_frame_offsets.as_ptr::<u64>(),
                                        n_frames as u64, &p, idx.as_ptr::<u64>(), seg_blocks)
        })?;
        Ok(Some(idx))
    }

    /// Give a stream that has no segment index (another encoder's, a block length the encoder does not index) one by a walk;
    /// `decode_windows` then decodes by it.
    pub fn index_by_walk<'g>(gpu: &'g Gpu, s: &mut EncodedStream<'g>, params: &x3::Parameters, seg_blocks: u32) -> error::Result<()> {
        s.seg_index = build_seg_index(gpu, &s.bytes, s.len, &s.frame_offsets, s.n_frames, params, seg_blocks)?;
        s.seg_blocks = if s.seg_index.is_some() { seg_blocks } else { 0 };
        Ok(())
    }

    /// output formats of `decode_windows`: int16 samples, or float32 = s / 32768 (exact)
    pub const WINDOW_I16: i32 = 0;
    pub const WINDOW_F32: i32 = 1;

    /// the stream's sample offsets (`x3_sample_offsets_dev`): `n_frames + 1` words, frame f's first sample and the total last
    pub fn sample_offsets<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>) -> error::Result<Buffer<'g>> {
        let so = Buffer::new(gpu, 8 * (s.n_frames + 1))?;
        error::check(unsafe {
            ffi::x3_sample_offsets_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(), s.n_frames as u64,
                                       so.as_ptr::<u64>())
        })?;
        Ok(so)
    }

    /// Random access (`x3_decode_windows_dev`; not in the reference crate, whose reader goes frame after frame): `n_windows`
    /// windows of `window_len` samples, window w = positions `[starts[w], starts[w] + window_len)` (`d_starts`: device u64s) as
    /// rows of `d_out` (`WINDOW_I16` / `WINDOW_F32`), `d_status[w]` = 0 or the first failing covering frame's status.  By the
    /// segment index when the stream has one.  Waits: -> (windows with status != 0, the first of them, its status)
    #[allow(clippy::too_many_arguments)]
    pub fn decode_windows<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                              d_starts: &Buffer<'g>, n_windows: usize, window_len: u32, d_out: &mut Buffer<'g>, out_format: i32,
                              d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32)> {
        let esz = if out_format == WINDOW_F32 { 4 } else { 2 };
        if d_starts.len() < 8 * n_windows || d_out.len() < esz * n_windows * window_len as usize || d_status.len() < 4 * n_windows {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        error::check(unsafe {
            ffi::x3_decode_windows_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                       sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                       d_starts.as_ptr::<u64>(), n_windows as u64, window_len, d_out.as_ptr::<c_void>(), out_format,
                                       d_status.as_ptr::<i32>())
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_decode_windows_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// Ranges (`x3_decode_ranges_dev`): windows with a length each, range w = positions `[starts[w], starts[w] + lens[w])`
    /// (`d_starts`: device u64s, `d_lens`: device u32s).  `row_stride` 0: rows packed at the exclusive sum of all lengths, which
    /// `d_out_offsets` (`n_ranges + 1` u64s, required) receives; a range without room in `out_cap` samples is `BadArg` and not
    /// written.  `row_stride` > 0: row w at `w * row_stride`, zeros behind its length.  Waits: -> (ranges with status != 0, the
    /// first of them, its status, the sum of all lengths)
    #[allow(clippy::too_many_arguments)]
    pub fn decode_ranges<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                             d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, row_stride: u64, d_out: &mut Buffer<'g>,
                             out_cap: u64, out_format: i32, d_out_offsets: Option<&mut Buffer<'g>>, d_status: &mut Buffer<'g>)
                             -> error::Result<(u64, u64, i32, u64)> {
        let esz = if out_format == WINDOW_F32 { 4 } else { 2 };
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges || (d_out.len() as u64) < esz * out_cap
            || d_status.len() < 4 * n_ranges || d_out_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_out_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_decode_ranges_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                      sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                      d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, row_stride,
                                      d_out.as_ptr::<c_void>(), out_cap, out_format, off, d_status.as_ptr::<i32>())
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_decode_ranges_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// One bin of `levels` / `Corpus::levels` (`x3_level`): `sum_sq`, `sum`, `min`, `max`, `n`; an empty bin holds the identities
    /// (`min` 32767, `max` -32768, `n` 0)
    pub type Level = ffi::x3_level;

    /// Levels (`x3_levels_dev`; not in the reference crate): min, max, count, sum and sum of squares of the samples per bin of
    /// `bin_len` positions (0: one bin) into `n_bins` records of `d_levels`, every one written, without a sample buffer.
    /// `d_frame_status` (`n_frames` x i32, optional): a frame with a status other than 0 adds nothing.  Waits: -> (frames with
    /// status != 0, the first of them, its status)
    #[allow(clippy::too_many_arguments)]
    pub fn levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>, bin_len: u64,
                      d_levels: &mut Buffer<'g>, n_bins: usize, d_frame_status: Option<&mut Buffer<'g>>) -> error::Result<(u64, u64, i32)> {
        signal_levels(gpu, s, params, sample_offsets, bin_len, d_levels, n_bins, d_frame_status, LevelSignal::Samples)
    }

    /// What `signal_levels` / `Corpus::signal_levels` bin (`X3_LEVEL_SIGNAL_*`): the samples, or their first difference clamped
    /// to 16 bits -- `x[i] - x[i-1]` at the position of sample i, across the seam of two frames that both have status 0; the
    /// first sample of a stream or entry adds nothing
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    #[repr(i32)]
    pub enum LevelSignal {
        Samples = 0,
        Diff = 1,
    }

    /// `levels` of a signal (`x3_signal_levels_dev`; not in the reference crate): arguments and result as `levels`
    #[allow(clippy::too_many_arguments)]
    pub fn signal_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>, bin_len: u64,
                             d_levels: &mut Buffer<'g>, n_bins: usize, d_frame_status: Option<&mut Buffer<'g>>, signal: LevelSignal)
                             -> error::Result<(u64, u64, i32)> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * s.n_frames) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_signal_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                      sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks, bin_len,
                                      d_levels.as_ptr::<Level>(), n_bins as u64, st_ptr, signal as std::os::raw::c_int)
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// An integer FIR filter in front of the levels (`x3_level_fir`): `y[i] = clamp((sum over t of taps[t] * x[i - t]) >> shift,
    /// 16 bits)`, counted where all `n_taps` positions lie in frames with status 0 of the same stream or entry.  1 .. 8 taps
    /// with sum |taps| <= 32768 and shift 0 .. 15; the calls refuse anything else
    pub type Fir = ffi::x3_level_fir;

    /// `Fir` of a slice of taps (at most 8 are taken; more make `n_taps` say so, and the calls refuse it)
    pub fn fir(taps: &[i16], shift: u32) -> Fir {
        let mut f = Fir { n_taps: taps.len() as u32, shift, taps: [0; 8] };
        for (d, s) in f.taps.iter_mut().zip(taps) {
            *d = *s;
        }
        f
    }

    /// `levels` behind an integer FIR filter (`x3_fir_levels_dev`; not in the reference crate): arguments and result as
    /// `levels`; `fir(&[1], 0)` gives its records, `fir(&[1, -1], 0)` those of `LevelSignal::Diff`
    #[allow(clippy::too_many_arguments)]
    pub fn fir_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>, bin_len: u64,
                          d_levels: &mut Buffer<'g>, n_bins: usize, d_frame_status: Option<&mut Buffer<'g>>, fir: &Fir)
                          -> error::Result<(u64, u64, i32)> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * s.n_frames) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_fir_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                   sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks, bin_len,
                                   d_levels.as_ptr::<Level>(), n_bins as u64, st_ptr, fir)
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// One bin of `tone_levels` / `Corpus::tone_levels` (`x3_tone_level`): `re` and `im`, the sums of sample times cos and
    /// sin of the oscillator's phase, and the samples' `min`, `max` and `n`
    pub type ToneLevel = ffi::x3_tone_level;

    /// The oscillator of `tone_levels` (`x3_level_tone`): position `i` has the phase `(i * step) mod 2^32`, whose top ten bits
    /// pick the table pair.  The table is 1 024 (cos, sin) `i16` pairs in a device buffer of the caller's (`tone_table()`
    /// uploaded, or any other contents)
    #[derive(Clone, Copy)]
    pub struct Tone<'a, 'g> {
        pub step: u32,
        pub table: &'a Buffer<'g>,
    }

    impl Tone<'_, '_> {
        fn c(&self) -> error::Result<ffi::x3_level_tone> {
            if self.table.len() < 4096 {
                return Err(X3Error::BadArg);
            }
            Ok(ffi::x3_level_tone { step: self.step, reserved: 0, d_table: self.table.as_ptr::<i16>() as *const i16 })
        }
    }

    /// The usual table: `(round(32767 cos(2 pi k / 1024)), round(32767 sin(2 pi k / 1024)))` at pair `k`, 2 048 values
    pub fn tone_table() -> Vec<i16> {
        let mut t = Vec::with_capacity(2048);
        for k in 0..1024 {
            let a = 2.0 * core::f64::consts::PI * (k as f64) / 1024.0;
            t.push((32767.0 * a.cos()).round() as i16);
            t.push((32767.0 * a.sin()).round() as i16);
        }
        t
    }

    /// Tone levels (`x3_tone_levels_dev`; not in the reference crate): arguments and result as `levels`, the records
    /// `ToneLevel`s
    #[allow(clippy::too_many_arguments)]
    pub fn tone_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>, bin_len: u64,
                           d_levels: &mut Buffer<'g>, n_bins: usize, d_frame_status: Option<&mut Buffer<'g>>, tone: &Tone<'_, 'g>)
                           -> error::Result<(u64, u64, i32)> {
        if d_levels.len() < core::mem::size_of::<ToneLevel>() * n_bins || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * s.n_frames) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let t = tone.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_tone_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                    sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks, bin_len,
                                    d_levels.as_ptr::<ToneLevel>(), n_bins as u64, st_ptr, &t)
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// The oscillators of `tone_bank_levels` (`x3_level_tone_bank`): 1 ..= 8 steps against one table, a device buffer as
    /// `Tone`'s
    #[derive(Clone, Copy)]
    pub struct ToneBank<'a, 'g> {
        pub steps: &'a [u32],
        pub table: &'a Buffer<'g>,
    }

    impl ToneBank<'_, '_> {
        fn c(&self) -> error::Result<ffi::x3_level_tone_bank> {
            if self.steps.is_empty() || self.steps.len() > 8 || self.table.len() < 4096 {
                return Err(X3Error::BadArg);
            }
            let mut steps = [0u32; 8];
            steps[..self.steps.len()].copy_from_slice(self.steps);
            Ok(ffi::x3_level_tone_bank { n_tones: self.steps.len() as u32, reserved: 0, d_table: self.table.as_ptr::<i16>() as *const i16, steps })
        }
    }

    /// Tone bank levels (`x3_tone_bank_levels_dev`; not in the reference crate): `tone_levels` for every step of the bank in
    /// one pass over the stream; `d_levels` holds `bank.steps.len()` planes of `n_bins` `ToneLevel`s, plane `t` what
    /// `tone_levels` writes for step `t`
    #[allow(clippy::too_many_arguments)]
    pub fn tone_bank_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>, bin_len: u64,
                                d_levels: &mut Buffer<'g>, n_bins: usize, d_frame_status: Option<&mut Buffer<'g>>,
                                bank: &ToneBank<'_, 'g>) -> error::Result<(u64, u64, i32)> {
        let b = bank.c()?;
        if d_levels.len() < core::mem::size_of::<ToneLevel>() * n_bins * bank.steps.len()
            || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * s.n_frames) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_tone_bank_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                         sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks, bin_len,
                                         d_levels.as_ptr::<ToneLevel>(), n_bins as u64, st_ptr, &b)
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// The adapter into the chain (`x3_tone_power_levels_dev`): the first `n_rows` tone records of `d_tone` -> the `Level`
    /// records of the band in `d_levels` (`None`: in place), which `events` and the quantiles calls take.  Asynchronous on the
    /// context's stream
    pub fn tone_power_levels<'g>(gpu: &'g Gpu, d_tone: &mut Buffer<'g>, n_rows: usize, d_levels: Option<&mut Buffer<'g>>)
                                 -> error::Result<()> {
        let bytes = core::mem::size_of::<Level>() * n_rows;
        if d_tone.len() < bytes || d_levels.as_ref().map_or(false, |b| b.len() < bytes) {
            return Err(X3Error::BadArg);
        }
        let src = d_tone.as_ptr::<ToneLevel>();
        let dst = match d_levels { Some(b) => b.as_ptr::<Level>(), None => src as *mut Level };
        error::check(unsafe { ffi::x3_tone_power_levels_dev(gpu.raw(), src as *const ToneLevel, n_rows as u64, dst) })
    }

    /// The rule of `events` / `Corpus::events` (`x3_event_rule`): a bin is hot when `sum_sq >= mean_sq_min * n` or `max(max,
    /// -min) >= peak_min` (0: off); hot bins with at most `join_bins` cold ones between them are one run; runs of fewer than
    /// `min_bins` bins are dropped; `pad_bins` on both sides (`2 * pad_bins <= join_bins`); pieces of `max_bins` (0: no cut)
    pub type EventRule = ffi::x3_event_rule;

    /// Events (`x3_events_dev`; not in the reference crate): the runs of hot bins of `n_bins` level records (as `levels` writes
    /// them) as `cap` slots of `d_starts` (u64), `d_lens` (u32) and, optionally, merged records in `d_event_levels`; `d_count`
    /// (one u64) receives the number found, which may exceed `cap`.  Slots behind the events are zero-length ranges: the arrays
    /// go to `decode_ranges` with `n_ranges = cap` as they are.  `sample_offsets`: the stream's (its last word is the sample
    /// count the rows are clipped to).  Waits: -> the events found
    #[allow(clippy::too_many_arguments)]
    pub fn events<'g>(gpu: &'g Gpu, d_levels: &Buffer<'g>, n_bins: usize, bin_len: u64, sample_offsets: &Buffer<'g>, n_frames: usize,
                      rule: &EventRule, d_starts: &mut Buffer<'g>, d_lens: &mut Buffer<'g>, d_event_levels: Option<&mut Buffer<'g>>,
                      cap: usize, d_count: &mut Buffer<'g>) -> error::Result<u64> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || sample_offsets.len() < 8 * (n_frames + 1)
            || d_starts.len() < 8 * cap || d_lens.len() < 4 * cap || d_count.len() < 8
            || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * cap) {
            return Err(X3Error::BadArg);
        }
        let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_events_dev(gpu.raw(), d_levels.as_ptr::<Level>() as *const Level, n_bins as u64, bin_len,
                               (sample_offsets.as_ptr::<u64>() as *const u64).add(n_frames), rule, d_starts.as_ptr::<u64>(),
                               d_lens.as_ptr::<u32>(), el_ptr, cap as u64, d_count.as_ptr::<u64>())
        })?;
        let mut count = 0u64;
        error::check(unsafe { ffi::x3_events_result(gpu.raw(), &mut count) })?;
        Ok(count)
    }

    /// The key of a level record the quantiles are taken of: `max(max, -min)` or `floor(sum_sq / n)` -- the largest `peak_min` /
    /// `mean_sq_min` at which the events rule still calls the bin hot
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub enum LevelKey {
        Peak = 0,
        MeanSq = 1,
    }
    /// `x3_threshold_rule`: per criterion `(q_ppm, mul, div, add)`, `div == 0`: off
    pub type ThresholdRule = ffi::x3_threshold_rule;
    /// `x3_event_threshold`: `mean_sq_min`, `peak_min` (0: off) and `counted` of one entry
    pub type EventThreshold = ffi::x3_event_threshold;

    /// Level quantiles (`x3_level_quantiles_dev`; not in the reference crate): quantile j (`q_ppm[j]` millionths, 1 .. 8 of
    /// them) of the keys of the counting rows (inside the stream, `n != 0`) of `n_bins` level records into `d_values` (u32 per
    /// quantile), their number K into `d_counted` (one u32): `sorted(keys)[(K - 1) * q / 1_000_000]`, 0 when K == 0.
    /// `sample_offsets` as in `events`.  Waits: -> (entries without a counting row, the first of them or 1)
    #[allow(clippy::too_many_arguments)]
    pub fn level_quantiles<'g>(gpu: &'g Gpu, d_levels: &Buffer<'g>, n_bins: usize, bin_len: u64, sample_offsets: &Buffer<'g>,
                               n_frames: usize, key: LevelKey, q_ppm: &[u32], d_values: &mut Buffer<'g>, d_counted: &mut Buffer<'g>)
                               -> error::Result<(u64, u64)> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || sample_offsets.len() < 8 * (n_frames + 1)
            || d_values.len() < 4 * q_ppm.len() || d_counted.len() < 4 {
            return Err(X3Error::BadArg);
        }
        error::check(unsafe {
            ffi::x3_level_quantiles_dev(gpu.raw(), d_levels.as_ptr::<Level>() as *const Level, n_bins as u64, bin_len,
                                        (sample_offsets.as_ptr::<u64>() as *const u64).add(n_frames), key as i32, q_ppm.as_ptr(),
                                        q_ppm.len() as u32, d_values.as_ptr::<u32>(), d_counted.as_ptr::<u32>())
        })?;
        let (mut n_empty, mut first) = (0u64, 0u64);
        error::check(unsafe { ffi::x3_level_quantiles_result(gpu.raw(), &mut n_empty, &mut first) })?;
        Ok((n_empty, first))
    }

    /// Thresholds from quantiles (`x3_level_thresholds_dev`): one `EventThreshold` into `d_thr` (16 bytes) by `rule`.  Waits:
    /// -> as `level_quantiles`
    pub fn level_thresholds<'g>(gpu: &'g Gpu, d_levels: &Buffer<'g>, n_bins: usize, bin_len: u64, sample_offsets: &Buffer<'g>,
                                n_frames: usize, rule: &ThresholdRule, d_thr: &mut Buffer<'g>) -> error::Result<(u64, u64)> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || sample_offsets.len() < 8 * (n_frames + 1)
            || d_thr.len() < core::mem::size_of::<EventThreshold>() {
            return Err(X3Error::BadArg);
        }
        error::check(unsafe {
            ffi::x3_level_thresholds_dev(gpu.raw(), d_levels.as_ptr::<Level>() as *const Level, n_bins as u64, bin_len,
                                         (sample_offsets.as_ptr::<u64>() as *const u64).add(n_frames), rule,
                                         d_thr.as_ptr::<EventThreshold>())
        })?;
        let (mut n_empty, mut first) = (0u64, 0u64);
        error::check(unsafe { ffi::x3_level_quantiles_result(gpu.raw(), &mut n_empty, &mut first) })?;
        Ok((n_empty, first))
    }

    /// Events with the rule's two values (both 0 in `rule`) taken from the `EventThreshold` in `d_thr`
    /// (`x3_events_adaptive_dev`); otherwise as `events`.  Waits: -> the events found
    #[allow(clippy::too_many_arguments)]
    pub fn events_adaptive<'g>(gpu: &'g Gpu, d_levels: &Buffer<'g>, n_bins: usize, bin_len: u64, sample_offsets: &Buffer<'g>,
                               n_frames: usize, rule: &EventRule, d_thr: &Buffer<'g>, d_starts: &mut Buffer<'g>,
                               d_lens: &mut Buffer<'g>, d_event_levels: Option<&mut Buffer<'g>>, cap: usize,
                               d_count: &mut Buffer<'g>) -> error::Result<u64> {
        if d_levels.len() < core::mem::size_of::<Level>() * n_bins || sample_offsets.len() < 8 * (n_frames + 1)
            || d_thr.len() < core::mem::size_of::<EventThreshold>()
            || d_starts.len() < 8 * cap || d_lens.len() < 4 * cap || d_count.len() < 8
            || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * cap) {
            return Err(X3Error::BadArg);
        }
        let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_events_adaptive_dev(gpu.raw(), d_levels.as_ptr::<Level>() as *const Level, n_bins as u64, bin_len,
                                        (sample_offsets.as_ptr::<u64>() as *const u64).add(n_frames), rule,
                                        d_thr.as_ptr::<EventThreshold>() as *const EventThreshold, d_starts.as_ptr::<u64>(),
                                        d_lens.as_ptr::<u32>(), el_ptr, cap as u64, d_count.as_ptr::<u64>())
        })?;
        let mut count = 0u64;
        error::check(unsafe { ffi::x3_events_result(gpu.raw(), &mut count) })?;
        Ok(count)
    }

    /// The rule of `plane_events` / `corpus_plane_events` (`x3_plane_event_rule`): a row is hot when at least `min_planes` of
    /// `n_planes` planes are loud at it, plane t under `mean_sq_min[t]` and `peak_min[t]`; the other four as in `EventRule`
    pub type PlaneEventRule = ffi::x3_plane_event_rule;

    /// Plane events (`x3_plane_events_dev`; not in the reference crate): the events of the rows that are loud in at least
    /// `rule.min_planes` of `rule.n_planes` planes of `n_bins` level records, plane t at `d_levels + t * plane_stride` records.
    /// `d_thr`: `None`, or an `EventThreshold` per plane (then `rule` carries no values).  Beside `events`' outputs:
    /// `d_event_planes` (u32, `cap` elements, optional): bit t set when plane t is loud in the event; `d_event_levels`
    /// (optional): `n_planes` planes of `cap` records.  Waits: -> the events found
    #[allow(clippy::too_many_arguments)]
    pub fn plane_events<'g>(gpu: &'g Gpu, d_levels: &Buffer<'g>, plane_stride: usize, n_bins: usize, bin_len: u64,
                            sample_offsets: &Buffer<'g>, n_frames: usize, rule: &PlaneEventRule, d_thr: Option<&Buffer<'g>>,
                            d_starts: &mut Buffer<'g>, d_lens: &mut Buffer<'g>, d_event_planes: Option<&mut Buffer<'g>>,
                            d_event_levels: Option<&mut Buffer<'g>>, cap: usize, d_count: &mut Buffer<'g>) -> error::Result<u64> {
        let k = rule.n_planes as usize;
        if k == 0 || k > 8 || plane_stride < n_bins
            || d_levels.len() < core::mem::size_of::<Level>() * ((k - 1) * plane_stride + n_bins)
            || sample_offsets.len() < 8 * (n_frames + 1)
            || d_thr.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<EventThreshold>() * k)
            || d_starts.len() < 8 * cap || d_lens.len() < 4 * cap || d_count.len() < 8
            || d_event_planes.as_ref().map_or(false, |b| b.len() < 4 * cap)
            || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * k * cap) {
            return Err(X3Error::BadArg);
        }
        let thr_ptr = match d_thr { Some(b) => b.as_ptr::<EventThreshold>() as *const EventThreshold, None => core::ptr::null() };
        let ep_ptr = match d_event_planes { Some(b) => b.as_ptr::<u32>(), None => core::ptr::null_mut() };
        let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_plane_events_dev(gpu.raw(), d_levels.as_ptr::<Level>() as *const Level, plane_stride as u64, n_bins as u64,
                                     bin_len, (sample_offsets.as_ptr::<u64>() as *const u64).add(n_frames), rule, thr_ptr,
                                     d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), ep_ptr, el_ptr, cap as u64,
                                     d_count.as_ptr::<u64>())
        })?;
        let mut count = 0u64;
        error::check(unsafe { ffi::x3_events_result(gpu.raw(), &mut count) })?;
        Ok(count)
    }

    /// Range levels (`x3_range_levels_dev`; not in the reference crate): the `Level` records of range w = positions
    /// `[starts[w], starts[w] + lens[w])`, bins of `bin_len` positions counted from the range's own start (0: one bin), max(1,
    /// ceil(len / bin_len)) rows each.  A frame with a status other than 0 adds nothing and gives the range its status.
    /// `row_stride` 0: rows packed at the exclusive sum of all row counts, which `d_row_offsets` (`n_ranges + 1` u64s,
    /// required) receives; a range without room in `rows_cap` records is `BadArg` and not written.  `row_stride` > 0: range w
    /// at `w * row_stride`, identities behind its rows.  The arrays `events` wrote go in as they are.  Waits: -> (ranges with
    /// status != 0, the first of them, its status, the sum of all row counts)
    #[allow(clippy::too_many_arguments)]
    pub fn range_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                            d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, bin_len: u64, row_stride: u64,
                            d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                            d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
        signal_range_levels(gpu, s, params, sample_offsets, d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap,
                            d_row_offsets, d_status, LevelSignal::Samples)
    }

    /// `range_levels` of a signal (`x3_signal_range_levels_dev`; not in the reference crate): arguments and result as
    /// `range_levels`.  `LevelSignal::Diff`: the stream's first difference cut to the ranges -- the difference at a range's
    /// first position counts (its earlier sample lies in front of the range), statuses are those of `LevelSignal::Samples`
    #[allow(clippy::too_many_arguments)]
    pub fn signal_range_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                                   d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, bin_len: u64, row_stride: u64,
                                   d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                   d_status: &mut Buffer<'g>, signal: LevelSignal) -> error::Result<(u64, u64, i32, u64)> {
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_levels.len() as u64) < core::mem::size_of::<Level>() as u64 * rows_cap
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_signal_range_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                            sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                            d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, bin_len, row_stride,
                                            d_levels.as_ptr::<Level>(), rows_cap, off, d_status.as_ptr::<i32>(), signal as std::os::raw::c_int)
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_range_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// `range_levels` of the stream's FIR signal (`x3_fir_range_levels_dev`; not in the reference crate): arguments and result
    /// as `range_levels`.  The call cuts the filtered stream, it does not filter the cut: a range's first T - 1 positions
    /// count (their earlier samples lie in front of the range), statuses are those of `range_levels`
    #[allow(clippy::too_many_arguments)]
    pub fn fir_range_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                                d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, bin_len: u64, row_stride: u64,
                                d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                d_status: &mut Buffer<'g>, fir: &Fir) -> error::Result<(u64, u64, i32, u64)> {
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_levels.len() as u64) < core::mem::size_of::<Level>() as u64 * rows_cap
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_fir_range_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                         sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                         d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, bin_len, row_stride,
                                         d_levels.as_ptr::<Level>(), rows_cap, off, d_status.as_ptr::<i32>(), fir)
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_range_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// `range_levels` of the stream's tone signal (`x3_tone_range_levels_dev`; not in the reference crate): arguments and
    /// result as `range_levels`, the records `ToneLevel`s.  The call cuts the stream's signal, it does not restart the
    /// oscillator: position `i` of the stream has the phase `(i * step) mod 2^32` wherever the range begins, so compare band
    /// power (`tone_power_levels`, which takes the records packed or padded), not the raw sums, across ranges
    #[allow(clippy::too_many_arguments)]
    pub fn tone_range_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                                 d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, bin_len: u64, row_stride: u64,
                                 d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                 d_status: &mut Buffer<'g>, tone: &Tone<'_, 'g>) -> error::Result<(u64, u64, i32, u64)> {
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_levels.len() as u64) < core::mem::size_of::<ToneLevel>() as u64 * rows_cap
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let t = tone.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_tone_range_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                          sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                          d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, bin_len, row_stride,
                                          d_levels.as_ptr::<ToneLevel>(), rows_cap, off, d_status.as_ptr::<i32>(), &t)
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_range_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// `tone_range_levels` for every step of a bank from one decode of the covering frames (`x3_tone_bank_range_levels_dev`;
    /// not in the reference crate): `d_levels` holds `bank.steps.len()` planes of `rows_cap` `ToneLevel`s, plane `t` -- at
    /// record `t * rows_cap` -- what `tone_range_levels` writes for step `t`; row offsets, statuses and the result exist once
    /// (the total is one plane's).  Records the call does not write stay untouched in every plane
    #[allow(clippy::too_many_arguments)]
    pub fn tone_bank_range_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                                      d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, bin_len: u64, row_stride: u64,
                                      d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                      d_status: &mut Buffer<'g>, bank: &ToneBank<'_, 'g>) -> error::Result<(u64, u64, i32, u64)> {
        let b = bank.c()?;
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_levels.len() as u64) < core::mem::size_of::<ToneLevel>() as u64 * rows_cap * bank.steps.len() as u64
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_tone_bank_range_levels_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                               sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                               d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, bin_len,
                                               row_stride, d_levels.as_ptr::<ToneLevel>(), rows_cap, off,
                                               d_status.as_ptr::<i32>(), &b)
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_range_levels_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// `spectra_rows` format: rows of `n_fft / 2 + 1` (re, im) i64 pairs
    pub const SPECTRA_SUMS: u32 = 0;
    /// `spectra_rows` format: rows of `n_fft / 2 + 1` u32 band powers, the tone adapter's `ms` at `n = n_fft`
    pub const SPECTRA_POWER: u32 = 1;

    /// The rule of `spectra_rows` / `range_spectra` (`x3_spectra_rule`): `n_fft` in {64, 128, 256, 512, 1024}, `hop` in
    /// 1 ..= 2^31 - 1, `power` for `SPECTRA_POWER` rows, and a device table of 1 024 (cos, sin) i16 pairs (`Tone`'s)
    #[derive(Clone, Copy)]
    pub struct SpectraRule<'t, 'g> {
        pub n_fft: u32,
        pub hop: u32,
        pub power: bool,
        pub table: &'t Buffer<'g>,
    }

    impl<'t, 'g> SpectraRule<'t, 'g> {
        /// bins of a row: `n_fft / 2 + 1`
        pub fn bins(&self) -> usize { self.n_fft as usize / 2 + 1 }
        /// bytes of a row
        pub fn row_bytes(&self) -> usize { self.bins() * if self.power { 4 } else { 16 } }
        /// whole frames of a row of `len` samples
        pub fn rows(&self, len: u64) -> u64 {
            if len < self.n_fft as u64 || self.hop == 0 { 0 } else { (len - self.n_fft as u64) / self.hop as u64 + 1 }
        }
        fn c(&self) -> error::Result<ffi::x3_spectra_rule> {
            if self.table.len() < 4096 { return Err(X3Error::BadArg); }
            Ok(ffi::x3_spectra_rule { n_fft: self.n_fft, hop: self.hop, format: if self.power { SPECTRA_POWER } else { SPECTRA_SUMS },
                                      reserved: 0, d_table: self.table.as_ptr::<i16>() as *const i16 })
        }
    }

    /// Spectra (`x3_spectra_rows_dev`; not in the reference crate): the exact integer STFT of the i16 rows `d_lens[w]` samples
    /// at `d_samples + d_offsets[w]`, as `decode_ranges` wrote them, on the matrix cores; the oscillator restarts at every
    /// frame.  `d_in_status`: the ranges call's statuses or `None`.  `row_stride` 0: range w's rows packed at
    /// `d_row_offsets[w]` (`n_ranges + 1` u64s, required); > 0: rows at `w * row_stride`, zeros behind the range's last.  A
    /// range with a status has rows of zeros only.  Waits: -> (ranges with status != 0, the first of them, its status, all rows)
    #[allow(clippy::too_many_arguments)]
    pub fn spectra_rows<'g>(gpu: &'g Gpu, d_samples: &Buffer<'g>, samples_cap: u64, d_offsets: &Buffer<'g>, d_lens: &Buffer<'g>,
                            d_in_status: Option<&Buffer<'g>>, n_ranges: usize, rule: &SpectraRule<'_, 'g>, row_stride: u64,
                            d_out: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                            d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
        let r = rule.c()?;
        if (d_samples.len() as u64) < 2 * samples_cap || d_offsets.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_out.len() as u64) < rule.row_bytes() as u64 * rows_cap || d_status.len() < 4 * n_ranges
            || d_in_status.map_or(false, |b| b.len() < 4 * n_ranges)
            || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let ins = d_in_status.map_or(core::ptr::null(), |b| b.as_ptr::<i32>() as *const i32);
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_spectra_rows_dev(gpu.raw(), d_samples.as_ptr::<i16>(), samples_cap, d_offsets.as_ptr::<u64>(),
                                     d_lens.as_ptr::<u32>(), ins, n_ranges as u64, &r, row_stride, d_out.as_ptr::<c_void>(),
                                     rows_cap, off, d_status.as_ptr::<i32>())
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_spectra_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// Range spectra: `x3_decode_ranges_dev` (packed i16 into `d_samples`, offsets to `d_sample_row_offsets`) and
    /// `x3_spectra_rows_dev` on those rows behind it on the same stream, in place on `d_status`, no host trip and no wait in
    /// between; the caller keeps the cut samples.  Waits for both: -> as `spectra_rows`
    #[allow(clippy::too_many_arguments)]
    pub fn range_spectra<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                             d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, rule: &SpectraRule<'_, 'g>,
                             d_samples: &mut Buffer<'g>, samples_cap: u64, d_sample_row_offsets: &mut Buffer<'g>, row_stride: u64,
                             d_out: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                             d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
        let r = rule.c()?;
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges || (d_samples.len() as u64) < 2 * samples_cap
            || d_sample_row_offsets.len() < 8 * (n_ranges + 1) || (d_out.len() as u64) < rule.row_bytes() as u64 * rows_cap
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_decode_ranges_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                      sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                      d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, 0,
                                      d_samples.as_ptr::<c_void>(), samples_cap, WINDOW_I16, d_sample_row_offsets.as_ptr::<u64>(),
                                      d_status.as_ptr::<i32>())
        })?;
        let rc = unsafe {
            ffi::x3_spectra_rows_dev(gpu.raw(), d_samples.as_ptr::<i16>(), samples_cap, d_sample_row_offsets.as_ptr::<u64>(),
                                     d_lens.as_ptr::<u32>(), d_status.as_ptr::<i32>(), n_ranges as u64, &r, row_stride,
                                     d_out.as_ptr::<c_void>(), rows_cap, off, d_status.as_ptr::<i32>())
        };
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_decode_ranges_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        error::check(rc)?;
        error::check(unsafe { ffi::x3_spectra_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// The fold of `spectra_levels` / `range_band_levels` (`x3_spectra_fold`): `frames_per_bin` in 1 ..= 2^31 - 1 consecutive
    /// frames make a time bin, `n_bands` in 1 ..= `n_fft / 2 + 1` bands, `bin_band` a device array of `n_fft / 2 + 1` u32 words
    /// (the band of every bin; a word >= `n_bands`: no band), `plane_stride` records between two planes (0: `rows_cap`)
    #[derive(Clone, Copy)]
    pub struct SpectraFold<'t, 'g> {
        pub frames_per_bin: u32,
        pub n_bands: u32,
        pub plane_stride: u64,
        pub bin_band: &'t Buffer<'g>,
    }

    impl<'t, 'g> SpectraFold<'t, 'g> {
        /// time bins of a range of `rows` frames
        pub fn time_bins(&self, rows: u64) -> u64 {
            if self.frames_per_bin == 0 { 0 } else { (rows + self.frames_per_bin as u64 - 1) / self.frames_per_bin as u64 }
        }
        /// bytes of the records: `n_bands` planes, the last one `rows_cap` records long
        pub fn level_bytes(&self, rows_cap: u64) -> u64 {
            let ps = if self.plane_stride == 0 { rows_cap } else { self.plane_stride };
            32 * ((self.n_bands as u64).saturating_sub(1) * ps + rows_cap)
        }
        fn c(&self, rule: &SpectraRule<'_, 'g>) -> error::Result<ffi::x3_spectra_fold> {
            if self.bin_band.len() < 4 * rule.bins() || !rule.power { return Err(X3Error::BadArg); }
            Ok(ffi::x3_spectra_fold { frames_per_bin: self.frames_per_bin, n_bands: self.n_bands, plane_stride: self.plane_stride,
                                      d_bin_band: self.bin_band.as_ptr::<u32>() as *const u32, reserved: 0 })
        }
    }

    /// Band levels (`x3_spectra_levels_dev`; not in the reference crate): `spectra_rows`' POWER words (`rule.power`) folded
    /// into `fold.n_bands` bands and summed over `fold.frames_per_bin` consecutive frames, one `x3_level` per (time bin, band)
    /// and no row per frame.  The rows of a range are its time bins, laid as `spectra_rows` lays its rows; plane b is band b at
    /// `b * plane_stride` records of `d_levels`; every record the call owns is written, the identity where no frame falls.
    /// Waits: -> (ranges with status != 0, the first of them, its status, all time bins)
    #[allow(clippy::too_many_arguments)]
    pub fn spectra_levels<'g>(gpu: &'g Gpu, d_samples: &Buffer<'g>, samples_cap: u64, d_offsets: &Buffer<'g>, d_lens: &Buffer<'g>,
                              d_in_status: Option<&Buffer<'g>>, n_ranges: usize, rule: &SpectraRule<'_, 'g>,
                              fold: &SpectraFold<'_, 'g>, row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64,
                              d_row_offsets: Option<&mut Buffer<'g>>, d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
        let r = rule.c()?;
        let f = fold.c(rule)?;
        if (d_samples.len() as u64) < 2 * samples_cap || d_offsets.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges
            || (d_levels.len() as u64) < fold.level_bytes(rows_cap) || d_status.len() < 4 * n_ranges
            || d_in_status.map_or(false, |b| b.len() < 4 * n_ranges)
            || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let ins = d_in_status.map_or(core::ptr::null(), |b| b.as_ptr::<i32>() as *const i32);
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_spectra_levels_dev(gpu.raw(), d_samples.as_ptr::<i16>(), samples_cap, d_offsets.as_ptr::<u64>(),
                                       d_lens.as_ptr::<u32>(), ins, n_ranges as u64, &r, &f, row_stride,
                                       d_levels.as_ptr::<ffi::x3_level>(), rows_cap, off, d_status.as_ptr::<i32>())
        })?;
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_spectra_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// Range band levels: `range_spectra` with `x3_spectra_levels_dev` in the place of `x3_spectra_rows_dev`.  (The whole-stream
    /// loop over chunks of ranges, `band_levels`, is the Python mirror's only.)  Waits for both: -> as `spectra_levels`
    #[allow(clippy::too_many_arguments)]
    pub fn range_band_levels<'g>(gpu: &'g Gpu, s: &EncodedStream<'g>, params: &x3::Parameters, sample_offsets: &Buffer<'g>,
                                 d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n_ranges: usize, rule: &SpectraRule<'_, 'g>,
                                 fold: &SpectraFold<'_, 'g>, d_samples: &mut Buffer<'g>, samples_cap: u64,
                                 d_sample_row_offsets: &mut Buffer<'g>, row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64,
                                 d_row_offsets: Option<&mut Buffer<'g>>, d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
        let r = rule.c()?;
        let f = fold.c(rule)?;
        if d_starts.len() < 8 * n_ranges || d_lens.len() < 4 * n_ranges || (d_samples.len() as u64) < 2 * samples_cap
            || d_sample_row_offsets.len() < 8 * (n_ranges + 1) || (d_levels.len() as u64) < fold.level_bytes(rows_cap)
            || d_status.len() < 4 * n_ranges || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n_ranges + 1)) {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        let idx = match &s.seg_index { Some(i) => i.as_ptr::<u64>() as *const u64, None => core::ptr::null() };
        let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
        error::check(unsafe {
            ffi::x3_decode_ranges_dev(gpu.raw(), s.bytes.as_ptr::<u8>(), s.len as u64, s.frame_offsets.as_ptr::<u64>(),
                                      sample_offsets.as_ptr::<u64>(), s.n_frames as u64, &p, idx, s.seg_blocks,
                                      d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n_ranges as u64, 0,
                                      d_samples.as_ptr::<c_void>(), samples_cap, WINDOW_I16, d_sample_row_offsets.as_ptr::<u64>(),
                                      d_status.as_ptr::<i32>())
        })?;
        let rc = unsafe {
            ffi::x3_spectra_levels_dev(gpu.raw(), d_samples.as_ptr::<i16>(), samples_cap, d_sample_row_offsets.as_ptr::<u64>(),
                                       d_lens.as_ptr::<u32>(), d_status.as_ptr::<i32>(), n_ranges as u64, &r, &f, row_stride,
                                       d_levels.as_ptr::<ffi::x3_level>(), rows_cap, off, d_status.as_ptr::<i32>())
        };
        let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
        error::check(unsafe { ffi::x3_decode_ranges_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        error::check(rc)?;
        error::check(unsafe { ffi::x3_spectra_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
        Ok((n_bad, first_bad, st, total))
    }

    /// `decode_streams` flag: the entries are the frame part of .x3a archives (walked with the reader's 8 phantom bytes)
    pub const STREAMS_ARCHIVE_FRAMES: u32 = 1;
    /// `Corpus::build` flag: the segment index by `x3_seg_index_build_dev` -- for every parameter set, not only where a
    /// decoder records one (block length 20, the default codes); `decode_streams` refuses it
    pub const CORPUS_INDEX_WALK: u32 = 0x100;

    /// A batch of independent streams (`x3_decode_streams_dev`; not in the reference crate, which reads one file): entry s =
    /// bytes `[offsets[s], offsets[s] + lengths[s])` of `d_x3`, decoded into row s of `d_out` (`offsets.len()` rows of
    /// `row_len` samples, `WINDOW_I16` / `WINDOW_F32`, zeros behind each entry's samples) with `x3_decode_stream_dev`'s results
    /// per entry in `d_results` (`x3_stream_result` each).  Waits: -> (entries with status != 0, the first of them, its status)
    #[allow(clippy::too_many_arguments)]
    pub fn decode_streams<'g>(gpu: &'g Gpu, d_x3: &Buffer<'g>, x3_len: usize, offsets: &[u64], lengths: &[u64], flags: u32,
                              params: &x3::Parameters, d_out: &mut Buffer<'g>, row_len: usize, out_format: i32,
                              d_results: &mut Buffer<'g>) -> error::Result<(u64, u64, i32)> {
        let n = offsets.len();
        let esz = if out_format == WINDOW_F32 { 4 } else { 2 };
        if lengths.len() != n || x3_len > d_x3.len() || d_out.len() < esz * n * row_len
            || d_results.len() < core::mem::size_of::<ffi::x3_stream_result>() * n {
            return Err(X3Error::BadArg);
        }
        let p = params.c()?;
        error::check(unsafe {
            ffi::x3_decode_streams_dev(gpu.raw(), d_x3.as_ptr::<u8>(), x3_len as u64, offsets.as_ptr(), lengths.as_ptr(), n as u64,
                                       flags, &p, d_out.as_ptr::<c_void>(), row_len as u64, out_format,
                                       d_results.as_ptr::<ffi::x3_stream_result>())
        })?;
        let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
        error::check(unsafe { ffi::x3_decode_streams_result(gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
        Ok((n_bad, first_bad, st))
    }

    /// Windows of many streams (`x3_corpus_build`; not in the reference crate): an index built once over the entries of
    /// `d_x3` (as in `decode_streams`), after which window w is samples `[d_starts[w], d_starts[w] + window_len)` of entry
    /// `d_entries[w]`.  The corpus borrows `d_x3`; dropping it frees the index.
    pub struct Corpus<'g> {
        gpu: &'g Gpu,
        raw: *mut ffi::x3_corpus,
        _bytes: core::marker::PhantomData<&'g Buffer<'g>>,
    }

    impl<'g> Corpus<'g> {
        /// Synchronous.  `seg_blocks`: 0 = no segment index (32 is the usual choice); it is only ever a hint.  `flags`: 0,
        /// `STREAMS_ARCHIVE_FRAMES`, `CORPUS_INDEX_WALK` or both.
        #[allow(clippy::too_many_arguments)]
        pub fn build(gpu: &'g Gpu, d_x3: &'g Buffer<'g>, x3_len: usize, offsets: &[u64], lengths: &[u64], flags: u32,
                     params: &x3::Parameters, seg_blocks: u32) -> error::Result<Corpus<'g>> {
            if lengths.len() != offsets.len() || x3_len > d_x3.len() {
                return Err(X3Error::BadArg);
            }
            let p = params.c()?;
            let mut raw: *mut ffi::x3_corpus = core::ptr::null_mut();
            error::check(unsafe {
                ffi::x3_corpus_build(gpu.raw(), d_x3.as_ptr::<u8>(), x3_len as u64, offsets.as_ptr(), lengths.as_ptr(),
                                     offsets.len() as u64, flags, &p, seg_blocks, &mut raw)
            })?;
            Ok(Corpus { gpu, raw, _bytes: core::marker::PhantomData })
        }

        /// -> (entries, frames, samples in all, segment index blocks in use)
        pub fn info(&self) -> (u64, u64, u64, u32) {
            let (mut n, mut f, mut t, mut sb) = (0u64, 0u64, 0u64, 0u32);
            unsafe { ffi::x3_corpus_info(self.raw, &mut n, &mut f, &mut t, &mut sb) };
            (n, f, t, sb)
        }

        pub fn entries(&self) -> Vec<ffi::x3_corpus_entry> {
            let mut v = vec![ffi::x3_corpus_entry::default(); self.info().0 as usize];
            unsafe { ffi::x3_corpus_entries(self.raw, v.as_mut_ptr()) };
            v
        }

        /// The recorded segment index: (device pointer the corpus owns, words), or (null, 0) without one
        pub fn seg_index(&self) -> (*const u64, u64) {
            let (mut d, mut n): (*const u64, u64) = (core::ptr::null(), 0);
            unsafe { ffi::x3_corpus_seg_index(self.raw, &mut d, &mut n) };
            (d, n)
        }

        /// `n` windows of `window_len` samples (`d_entries`: n x u32, `d_starts`: n x u64, `d_out`: n x window_len samples of
        /// `out_format`, `d_status`: n x i32).  Waits: -> (windows with status != 0, the first of them, its status)
        #[allow(clippy::too_many_arguments)]
        pub fn windows(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, n: usize, window_len: u32, d_out: &mut Buffer<'g>,
                       out_format: i32, d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32)> {
            let esz = if out_format == WINDOW_F32 { 4 } else { 2 };
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_out.len() < esz * n * window_len as usize
                || d_status.len() < 4 * n {
                return Err(X3Error::BadArg);
            }
            error::check(unsafe {
                ffi::x3_corpus_windows_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(),
                                           n as u64, window_len, d_out.as_ptr::<c_void>(), out_format, d_status.as_ptr::<i32>())
            })?;
            let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
            error::check(unsafe { ffi::x3_decode_windows_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
            Ok((n_bad, first_bad, st))
        }

        /// Ranges of entries (`x3_corpus_ranges_dev`): range w = samples `[starts[w], starts[w] + lens[w])` of entry
        /// `entries[w]`; layout, capacity and result as `decode_ranges`
        #[allow(clippy::too_many_arguments)]
        pub fn ranges(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize, row_stride: u64,
                      d_out: &mut Buffer<'g>, out_cap: u64, out_format: i32, d_out_offsets: Option<&mut Buffer<'g>>,
                      d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
            let esz = if out_format == WINDOW_F32 { 4 } else { 2 };
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_lens.len() < 4 * n || (d_out.len() as u64) < esz * out_cap
                || d_status.len() < 4 * n || d_out_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n + 1)) {
                return Err(X3Error::BadArg);
            }
            let off = d_out_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
            error::check(unsafe {
                ffi::x3_corpus_ranges_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(),
                                          d_lens.as_ptr::<u32>(), n as u64, row_stride, d_out.as_ptr::<c_void>(), out_cap,
                                          out_format, off, d_status.as_ptr::<i32>())
            })?;
            let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
            error::check(unsafe { ffi::x3_decode_ranges_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
            Ok((n_bad, first_bad, st, total))
        }
    }

    impl<'g> Corpus<'g> {
        /// Entry e's records of `levels` are `[row_first[e], row_first[e + 1])`: max(1, ceil(n_samples / bin_len)) each, one with
        /// `bin_len` 0 (`x3_corpus_levels_rows`; `n_entries + 1` words)
        pub fn levels_rows(&self, bin_len: u64) -> Vec<u64> {
            let mut v = vec![0u64; self.info().0 as usize + 1];
            unsafe { ffi::x3_corpus_levels_rows(self.raw, bin_len, v.as_mut_ptr()) };
            v
        }

        /// Levels of every entry (`x3_corpus_levels_dev`), positions relative to the entry; `d_levels` holds `n_rows` =
        /// `levels_rows(bin_len)`'s last word records, `d_frame_status` one i32 per frame of the corpus (optional).  Waits: ->
        /// (frames with status != 0, the first of them, its status)
        pub fn levels(&self, bin_len: u64, d_levels: &mut Buffer<'g>, n_rows: usize, d_frame_status: Option<&mut Buffer<'g>>)
                      -> error::Result<(u64, u64, i32)> {
            self.signal_levels(bin_len, d_levels, n_rows, d_frame_status, LevelSignal::Samples)
        }

        /// `levels` of a signal (`x3_corpus_signal_levels_dev`): arguments and result as `levels`; no difference crosses from
        /// one entry into the next
        pub fn signal_levels(&self, bin_len: u64, d_levels: &mut Buffer<'g>, n_rows: usize, d_frame_status: Option<&mut Buffer<'g>>,
                             signal: LevelSignal) -> error::Result<(u64, u64, i32)> {
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows
                || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * self.info().1 as usize) {
                return Err(X3Error::BadArg);
            }
            let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_signal_levels_dev(self.gpu.raw(), self.raw, bin_len, d_levels.as_ptr::<Level>(), n_rows as u64, st_ptr,
                                                 signal as std::os::raw::c_int)
            })?;
            let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
            error::check(unsafe { ffi::x3_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
            Ok((n_bad, first_bad, st))
        }
    }

    impl<'g> Corpus<'g> {
        /// `levels` behind an integer FIR filter (`x3_corpus_fir_levels_dev`): arguments and result as `levels`; no history
        /// crosses from one entry into the next
        pub fn fir_levels(&self, bin_len: u64, d_levels: &mut Buffer<'g>, n_rows: usize, d_frame_status: Option<&mut Buffer<'g>>,
                          fir: &Fir) -> error::Result<(u64, u64, i32)> {
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows
                || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * self.info().1 as usize) {
                return Err(X3Error::BadArg);
            }
            let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_fir_levels_dev(self.gpu.raw(), self.raw, bin_len, d_levels.as_ptr::<Level>(), n_rows as u64, st_ptr, fir)
            })?;
            let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
            error::check(unsafe { ffi::x3_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
            Ok((n_bad, first_bad, st))
        }

        /// Tone levels of every entry (`x3_corpus_tone_levels_dev`): `levels`' rows as `ToneLevel`s; the phase restarts at 0
        /// with every entry
        pub fn tone_levels(&self, bin_len: u64, d_levels: &mut Buffer<'g>, n_rows: usize, d_frame_status: Option<&mut Buffer<'g>>,
                           tone: &Tone<'_, 'g>) -> error::Result<(u64, u64, i32)> {
            if d_levels.len() < core::mem::size_of::<ToneLevel>() * n_rows
                || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * self.info().1 as usize) {
                return Err(X3Error::BadArg);
            }
            let t = tone.c()?;
            let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_tone_levels_dev(self.gpu.raw(), self.raw, bin_len, d_levels.as_ptr::<ToneLevel>(), n_rows as u64, st_ptr, &t)
            })?;
            let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
            error::check(unsafe { ffi::x3_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
            Ok((n_bad, first_bad, st))
        }

        /// Tone bank levels of every entry (`x3_corpus_tone_bank_levels_dev`): `bank.steps.len()` planes of `tone_levels`'
        /// `n_rows` records; every entry starts at phase 0 in every plane
        pub fn tone_bank_levels(&self, bin_len: u64, d_levels: &mut Buffer<'g>, n_rows: usize, d_frame_status: Option<&mut Buffer<'g>>,
                                bank: &ToneBank<'_, 'g>) -> error::Result<(u64, u64, i32)> {
            let b = bank.c()?;
            if d_levels.len() < core::mem::size_of::<ToneLevel>() * n_rows * bank.steps.len()
                || d_frame_status.as_ref().map_or(false, |b| b.len() < 4 * self.info().1 as usize) {
                return Err(X3Error::BadArg);
            }
            let st_ptr = match d_frame_status { Some(b) => b.as_ptr::<i32>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_tone_bank_levels_dev(self.gpu.raw(), self.raw, bin_len, d_levels.as_ptr::<ToneLevel>(), n_rows as u64, st_ptr, &b)
            })?;
            let (mut n_bad, mut first_bad, mut st) = (0u64, 0u64, 0);
            error::check(unsafe { ffi::x3_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st) })?;
            Ok((n_bad, first_bad, st))
        }

        /// Events of every entry (`x3_corpus_events_dev`) over the `n_rows` records `levels` wrote: as `device::events`, with
        /// the events' entries in `d_entries` (u32); the arrays go to `ranges` with `n_ranges = cap` as they are.  Waits: ->
        /// the events found
        #[allow(clippy::too_many_arguments)]
        pub fn events(&self, d_levels: &Buffer<'g>, n_rows: usize, bin_len: u64, rule: &EventRule, d_entries: &mut Buffer<'g>,
                      d_starts: &mut Buffer<'g>, d_lens: &mut Buffer<'g>, d_event_levels: Option<&mut Buffer<'g>>, cap: usize,
                      d_count: &mut Buffer<'g>) -> error::Result<u64> {
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows || d_entries.len() < 4 * cap || d_starts.len() < 8 * cap
                || d_lens.len() < 4 * cap || d_count.len() < 8
                || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * cap) {
                return Err(X3Error::BadArg);
            }
            let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_events_dev(self.gpu.raw(), self.raw, d_levels.as_ptr::<Level>() as *const Level, n_rows as u64, bin_len,
                                          rule, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), el_ptr,
                                          cap as u64, d_count.as_ptr::<u64>())
            })?;
            let mut count = 0u64;
            error::check(unsafe { ffi::x3_events_result(self.gpu.raw(), &mut count) })?;
            Ok(count)
        }
    }

    impl<'g> Corpus<'g> {
        /// Level quantiles of every entry (`x3_corpus_level_quantiles_dev`) over the `n_rows` records `levels` wrote: as
        /// `device::level_quantiles`, `d_values` u32 `[n_entries * q_ppm.len()]`, `d_counted` u32 `[n_entries]`.  Waits: ->
        /// (entries without a counting row, the first of them or the entry count)
        #[allow(clippy::too_many_arguments)]
        pub fn level_quantiles(&self, d_levels: &Buffer<'g>, n_rows: usize, bin_len: u64, key: LevelKey, q_ppm: &[u32],
                               d_values: &mut Buffer<'g>, d_counted: &mut Buffer<'g>) -> error::Result<(u64, u64)> {
            let n_ent = self.info().0 as usize;
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows || d_values.len() < 4 * n_ent * q_ppm.len()
                || d_counted.len() < 4 * n_ent {
                return Err(X3Error::BadArg);
            }
            error::check(unsafe {
                ffi::x3_corpus_level_quantiles_dev(self.gpu.raw(), self.raw, d_levels.as_ptr::<Level>() as *const Level, n_rows as u64,
                                                   bin_len, key as i32, q_ppm.as_ptr(), q_ppm.len() as u32,
                                                   d_values.as_ptr::<u32>(), d_counted.as_ptr::<u32>())
            })?;
            let (mut n_empty, mut first) = (0u64, 0u64);
            error::check(unsafe { ffi::x3_level_quantiles_result(self.gpu.raw(), &mut n_empty, &mut first) })?;
            Ok((n_empty, first))
        }

        /// Thresholds of every entry (`x3_corpus_level_thresholds_dev`): `n_entries` `EventThreshold` records into `d_thr`.
        /// Waits: -> as `level_quantiles`
        pub fn level_thresholds(&self, d_levels: &Buffer<'g>, n_rows: usize, bin_len: u64, rule: &ThresholdRule,
                                d_thr: &mut Buffer<'g>) -> error::Result<(u64, u64)> {
            let n_ent = self.info().0 as usize;
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows || d_thr.len() < core::mem::size_of::<EventThreshold>() * n_ent {
                return Err(X3Error::BadArg);
            }
            error::check(unsafe {
                ffi::x3_corpus_level_thresholds_dev(self.gpu.raw(), self.raw, d_levels.as_ptr::<Level>() as *const Level, n_rows as u64,
                                                    bin_len, rule, d_thr.as_ptr::<EventThreshold>())
            })?;
            let (mut n_empty, mut first) = (0u64, 0u64);
            error::check(unsafe { ffi::x3_level_quantiles_result(self.gpu.raw(), &mut n_empty, &mut first) })?;
            Ok((n_empty, first))
        }

        /// Events with entry e's two values in `d_thr[e]` (`x3_corpus_events_adaptive_dev`; both 0 in `rule`); otherwise as
        /// `events`.  Waits: -> the events found
        #[allow(clippy::too_many_arguments)]
        pub fn events_adaptive(&self, d_levels: &Buffer<'g>, n_rows: usize, bin_len: u64, rule: &EventRule, d_thr: &Buffer<'g>,
                               d_entries: &mut Buffer<'g>, d_starts: &mut Buffer<'g>, d_lens: &mut Buffer<'g>,
                               d_event_levels: Option<&mut Buffer<'g>>, cap: usize, d_count: &mut Buffer<'g>) -> error::Result<u64> {
            let n_ent = self.info().0 as usize;
            if d_levels.len() < core::mem::size_of::<Level>() * n_rows || d_thr.len() < core::mem::size_of::<EventThreshold>() * n_ent
                || d_entries.len() < 4 * cap || d_starts.len() < 8 * cap || d_lens.len() < 4 * cap || d_count.len() < 8
                || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * cap) {
                return Err(X3Error::BadArg);
            }
            let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
            error::check(unsafe {
                ffi::x3_corpus_events_adaptive_dev(self.gpu.raw(), self.raw, d_levels.as_ptr::<Level>() as *const Level, n_rows as u64,
                                                   bin_len, rule, d_thr.as_ptr::<EventThreshold>() as *const EventThreshold,
                                                   d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), el_ptr,
                                                   cap as u64, d_count.as_ptr::<u64>())
            })?;
            let mut count = 0u64;
            error::check(unsafe { ffi::x3_events_result(self.gpu.raw(), &mut count) })?;
            Ok(count)
        }
    }

    /// Plane events of every entry (`x3_corpus_plane_events_dev`) over `rule.n_planes` planes of the `n_rows` records
    /// `Corpus::levels` lays: as `device::plane_events`, with the events' entries in `d_entries`; `d_thr`: `None`, or
    /// `n_planes * n_entries` records laid plane-major.  Waits: -> the events found
    #[allow(clippy::too_many_arguments)]
    pub fn corpus_plane_events<'g>(corpus: &Corpus<'g>, d_levels: &Buffer<'g>, plane_stride: usize, n_rows: usize, bin_len: u64,
                                   rule: &PlaneEventRule, d_thr: Option<&Buffer<'g>>, d_entries: &mut Buffer<'g>,
                                   d_starts: &mut Buffer<'g>, d_lens: &mut Buffer<'g>, d_event_planes: Option<&mut Buffer<'g>>,
                                   d_event_levels: Option<&mut Buffer<'g>>, cap: usize,
                                   d_count: &mut Buffer<'g>) -> error::Result<u64> {
        let (k, n_ent) = (rule.n_planes as usize, corpus.info().0 as usize);
        if k == 0 || k > 8 || plane_stride < n_rows
            || d_levels.len() < core::mem::size_of::<Level>() * ((k - 1) * plane_stride + n_rows)
            || d_thr.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<EventThreshold>() * k * n_ent)
            || d_entries.len() < 4 * cap || d_starts.len() < 8 * cap || d_lens.len() < 4 * cap || d_count.len() < 8
            || d_event_planes.as_ref().map_or(false, |b| b.len() < 4 * cap)
            || d_event_levels.as_ref().map_or(false, |b| b.len() < core::mem::size_of::<Level>() * k * cap) {
            return Err(X3Error::BadArg);
        }
        let thr_ptr = match d_thr { Some(b) => b.as_ptr::<EventThreshold>() as *const EventThreshold, None => core::ptr::null() };
        let ep_ptr = match d_event_planes { Some(b) => b.as_ptr::<u32>(), None => core::ptr::null_mut() };
        let el_ptr = match d_event_levels { Some(b) => b.as_ptr::<Level>(), None => core::ptr::null_mut() };
        error::check(unsafe {
            ffi::x3_corpus_plane_events_dev(corpus.gpu.raw(), corpus.raw, d_levels.as_ptr::<Level>() as *const Level,
                                            plane_stride as u64, n_rows as u64, bin_len, rule, thr_ptr, d_entries.as_ptr::<u32>(),
                                            d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), ep_ptr, el_ptr, cap as u64,
                                            d_count.as_ptr::<u64>())
        })?;
        let mut count = 0u64;
        error::check(unsafe { ffi::x3_events_result(corpus.gpu.raw(), &mut count) })?;
        Ok(count)
    }

    impl<'g> Corpus<'g> {
        /// Range levels of entries (`x3_corpus_range_levels_dev`): the records of range w = samples `[starts[w], starts[w] +
        /// lens[w])` of entry `entries[w]`; bins, layout, capacity and result as `device::range_levels`.  The arrays `events`
        /// wrote go in as they are
        #[allow(clippy::too_many_arguments)]
        pub fn range_levels(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize, bin_len: u64,
                            row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                            d_status: &mut Buffer<'g>) -> error::Result<(u64, u64, i32, u64)> {
            self.signal_range_levels(d_entries, d_starts, d_lens, n, bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status,
                                     LevelSignal::Samples)
        }

        /// `range_levels` of a signal (`x3_corpus_signal_range_levels_dev`): arguments and result as `range_levels`; no
        /// difference crosses from one entry into the next
        #[allow(clippy::too_many_arguments)]
        pub fn signal_range_levels(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize, bin_len: u64,
                                   row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                   d_status: &mut Buffer<'g>, signal: LevelSignal) -> error::Result<(u64, u64, i32, u64)> {
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_lens.len() < 4 * n
                || (d_levels.len() as u64) < core::mem::size_of::<Level>() as u64 * rows_cap
                || d_status.len() < 4 * n || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n + 1)) {
                return Err(X3Error::BadArg);
            }
            let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
            error::check(unsafe {
                ffi::x3_corpus_signal_range_levels_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(),
                                                       d_lens.as_ptr::<u32>(), n as u64, bin_len, row_stride,
                                                       d_levels.as_ptr::<Level>(), rows_cap, off, d_status.as_ptr::<i32>(),
                                                       signal as std::os::raw::c_int)
            })?;
            let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
            error::check(unsafe { ffi::x3_range_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
            Ok((n_bad, first_bad, st, total))
        }

        /// `range_levels` of each entry's FIR signal (`x3_corpus_fir_range_levels_dev`): arguments and result as
        /// `range_levels`; no filter history crosses from one entry into the next
        #[allow(clippy::too_many_arguments)]
        pub fn fir_range_levels(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize, bin_len: u64,
                                row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                d_status: &mut Buffer<'g>, fir: &Fir) -> error::Result<(u64, u64, i32, u64)> {
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_lens.len() < 4 * n
                || (d_levels.len() as u64) < core::mem::size_of::<Level>() as u64 * rows_cap
                || d_status.len() < 4 * n || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n + 1)) {
                return Err(X3Error::BadArg);
            }
            let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
            error::check(unsafe {
                ffi::x3_corpus_fir_range_levels_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(),
                                                    d_lens.as_ptr::<u32>(), n as u64, bin_len, row_stride,
                                                    d_levels.as_ptr::<Level>(), rows_cap, off, d_status.as_ptr::<i32>(), fir)
            })?;
            let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
            error::check(unsafe { ffi::x3_range_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
            Ok((n_bad, first_bad, st, total))
        }

        /// `range_levels` of each entry's tone signal (`x3_corpus_tone_range_levels_dev`): arguments and result as
        /// `range_levels`, the records `ToneLevel`s; starts count from the entry's first position and so does the phase
        #[allow(clippy::too_many_arguments)]
        pub fn tone_range_levels(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize, bin_len: u64,
                                 row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64, d_row_offsets: Option<&mut Buffer<'g>>,
                                 d_status: &mut Buffer<'g>, tone: &Tone<'_, 'g>) -> error::Result<(u64, u64, i32, u64)> {
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_lens.len() < 4 * n
                || (d_levels.len() as u64) < core::mem::size_of::<ToneLevel>() as u64 * rows_cap
                || d_status.len() < 4 * n || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n + 1)) {
                return Err(X3Error::BadArg);
            }
            let t = tone.c()?;
            let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
            error::check(unsafe {
                ffi::x3_corpus_tone_range_levels_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(), d_starts.as_ptr::<u64>(),
                                                     d_lens.as_ptr::<u32>(), n as u64, bin_len, row_stride,
                                                     d_levels.as_ptr::<ToneLevel>(), rows_cap, off, d_status.as_ptr::<i32>(), &t)
            })?;
            let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
            error::check(unsafe { ffi::x3_range_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
            Ok((n_bad, first_bad, st, total))
        }

        /// `tone_range_levels` for every step of a bank (`x3_corpus_tone_bank_range_levels_dev`): `bank.steps.len()` planes of
        /// `rows_cap` `ToneLevel`s; starts count from the entry's first position and so does the phase, in every plane
        #[allow(clippy::too_many_arguments)]
        pub fn tone_bank_range_levels(&self, d_entries: &Buffer<'g>, d_starts: &Buffer<'g>, d_lens: &Buffer<'g>, n: usize,
                                      bin_len: u64, row_stride: u64, d_levels: &mut Buffer<'g>, rows_cap: u64,
                                      d_row_offsets: Option<&mut Buffer<'g>>, d_status: &mut Buffer<'g>,
                                      bank: &ToneBank<'_, 'g>) -> error::Result<(u64, u64, i32, u64)> {
            let b = bank.c()?;
            if d_entries.len() < 4 * n || d_starts.len() < 8 * n || d_lens.len() < 4 * n
                || (d_levels.len() as u64) < core::mem::size_of::<ToneLevel>() as u64 * rows_cap * bank.steps.len() as u64
                || d_status.len() < 4 * n || d_row_offsets.as_ref().map_or(false, |b| b.len() < 8 * (n + 1)) {
                return Err(X3Error::BadArg);
            }
            let off = d_row_offsets.map_or(core::ptr::null_mut(), |b| b.as_ptr::<u64>());
            error::check(unsafe {
                ffi::x3_corpus_tone_bank_range_levels_dev(self.gpu.raw(), self.raw, d_entries.as_ptr::<u32>(),
                                                          d_starts.as_ptr::<u64>(), d_lens.as_ptr::<u32>(), n as u64, bin_len,
                                                          row_stride, d_levels.as_ptr::<ToneLevel>(), rows_cap, off,
                                                          d_status.as_ptr::<i32>(), &b)
            })?;
            let (mut n_bad, mut first_bad, mut st, mut total) = (0u64, 0u64, 0, 0u64);
            error::check(unsafe { ffi::x3_range_levels_result(self.gpu.raw(), &mut n_bad, &mut first_bad, &mut st, &mut total) })?;
            Ok((n_bad, first_bad, st, total))
        }
    }

    impl Drop for Corpus<'_> {
        fn drop(&mut self) {
            unsafe { ffi::x3_corpus_destroy(self.raw) };
        }
    }

    /// Placement (`x3_place_buffers`; profiles/r6/decoder_modes.txt): the round trip timed on every pair of candidate buffers --
    /// `ms[i * backs.len() + j]` for `(streams[i], backs[j])`, `cap` bytes of room in every stream buffer.  A pipeline that keeps its
    /// buffers calls this once and keeps the pair that runs best.
    pub fn place_buffers<'g>(gpu: &'g Gpu, d_wav: &Buffer<'g>, n: usize, params: &x3::Parameters, streams: &[&Buffer<'g>], cap: usize,
                             frame_offsets: &mut Buffer<'g>, backs: &[&Buffer<'g>], warm: u32, steps: u32) -> error::Result<Vec<f64>> {
        let p = params.c()?;
        let s: Vec<*mut u8> = streams.iter().map(|b| b.as_ptr::<u8>()).collect();
        let k: Vec<*mut i16> = backs.iter().map(|b| b.as_ptr::<i16>()).collect();
        let mut ms = vec![0f64; s.len() * k.len()];
        error::check(unsafe {
            ffi::x3_place_buffers(gpu.raw(), d_wav.as_ptr::<i16>(), n as u64, &p, s.as_ptr(), s.len() as u32, cap as u64,
                                  frame_offsets.as_ptr::<u64>(), k.as_ptr(), k.len() as u32, warm, steps, ms.as_mut_ptr())
        })?;
        Ok(ms)
    }
}

pub mod encodefile {
    //! src/encodefile.rs:48-77, streamed through the GPU in chunks
    use crate::error::{self, X3Error};
    use crate::{ffi, gpu};
    use std::{ffi::CString, path};

    pub(crate) fn c_path<P: AsRef<path::Path>>(p: P) -> Result<CString, X3Error> {
        let bad = || X3Error::Io(std::io::Error::new(std::io::ErrorKind::InvalidInput, "path is not UTF-8 / has a NUL"));
        CString::new(p.as_ref().to_str().ok_or_else(bad)?).map_err(|_| bad())
    }

    pub fn wav_to_x3a<P: AsRef<path::Path>>(wav_filename: P, x3a_filename: P) -> Result<(), X3Error> {
        let (a, b) = (c_path(wav_filename)?, c_path(x3a_filename)?);
        let mut stats = [0u64; 6];
        gpu::with_default(|g| error::check(unsafe { ffi::x3_wav_to_x3a(g.raw(), a.as_ptr(), b.as_ptr(), stats.as_mut_ptr()) }))?;
        // the block `encoder::encode` prints under `std` (src/encoder.rs:96-108)
        let t = stats.iter().sum::<u64>() as f32;
        let pc = |k: usize| (stats[k] as f32 / t) * 100.0;
        println!("\nStatistics:\n  Rice-0: {:.4}%\n  Rice-1: {:.4}%\n  Rice-2: {:.4}%\n  Rice-3: {:.4}%\n  BFP: {:.4}%\n  Pass-through {:.4}%\n",
                 pc(0), pc(1), pc(2), pc(3), pc(4), pc(5));
        Ok(())
    }
}

pub mod tune {
    //! Parameter tuning (not in the reference; include/x3hip.h, "parameter tuning"): the exact encoded size of an input
    //! under each of the 2 184 safe parameter sets, in one pass on the GPU, and the .x3a encode that uses the smallest.
    use crate::error::{self, X3Error};
    use crate::x3::Parameters;
    use crate::{ffi, gpu};

    pub const CANDIDATES: usize = 2184;
    pub const DEFAULT_INDEX: usize = 1188;
    pub const DEFAULT_SPF: u32 = 10000;

    fn zero_params() -> ffi::x3_params {
        ffi::x3_params { block_len: 0, blocks_per_frame: 0, codes: [0; 3], thresholds: [0; 3] }
    }

    /// candidate `index` of the grid at frame length `spf`
    pub fn candidate(index: u32, spf: u32) -> Result<Parameters, X3Error> {
        let mut p = zero_params();
        error::check(unsafe { ffi::x3_tune_candidate(index, spf, &mut p) })?;
        Ok(Parameters::from_c(&p))
    }

    /// the chosen set (smallest total; ties: the default set, else the lowest index), its total and every candidate's total
    pub fn tune(wav: &[i16], spf: u32) -> Result<(Parameters, u64, Vec<u64>), X3Error> {
        let mut p = zero_params();
        let mut best = 0u64;
        let mut sizes = vec![0u64; CANDIDATES];
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_tune(g.raw(), wav.as_ptr(), wav.len() as u64, spf, &mut p, &mut best, sizes.as_mut_ptr())
            })
        })?;
        Ok((Parameters::from_c(&p), best, sizes))
    }

    /// `wav_to_x3a` in memory with the tuned parameters: the archive bytes and the parameters its header records
    pub fn x3a_encode_tuned(wav: &[i16], sample_rate: u32) -> Result<(Vec<u8>, Parameters), X3Error> {
        let mut out = vec![0u8; 1024 + 20 * (wav.len() / 40 + 1) + 2 * wav.len() + 64];
        let mut len = 0u64;
        let mut stats = [0u64; 6];
        let mut p = zero_params();
        gpu::with_default(|g| {
            error::check(unsafe {
                ffi::x3_x3a_encode_tuned(g.raw(), wav.as_ptr(), wav.len() as u64, sample_rate, out.as_mut_ptr(),
                                         out.len() as u64, &mut len, stats.as_mut_ptr(), &mut p)
            })
        })?;
        out.truncate(len as usize);
        Ok((out, Parameters::from_c(&p)))
    }
}

pub mod decodefile {
    //! src/decodefile.rs
    use crate::encodefile::c_path;
    use crate::error::{self, X3Error};
    use crate::x3::{Parameters, X3aSpec};
    use crate::{ffi, gpu};
    use std::path;

    pub const X3_READ_BUFFER_SIZE: usize = 1024 * 24;
    pub const X3_WRITE_BUFFER_SIZE: usize = X3_READ_BUFFER_SIZE * 8;

    /// src/decodefile.rs:47-136.  Behind `decode_next_frame` the library decodes windows of frames ahead on the
    /// GPU and hands them out one per call, with the reference's per-call results.
    pub struct X3aReader {
        reader: *mut ffi::x3_reader,
        spec: X3aSpec,
    }
    impl Drop for X3aReader {
        fn drop(&mut self) {
            unsafe { ffi::x3_reader_close(self.reader) }
        }
    }
    impl X3aReader {
        pub fn open<P: AsRef<path::Path>>(filename: P) -> Result<Self, X3Error> {
            let name = c_path(filename)?;
            let mut reader = core::ptr::null_mut();
            gpu::with_default(|g| error::check(unsafe { ffi::x3_reader_open(g.raw(), name.as_ptr(), &mut reader) }))?;
            let mut p = ffi::x3_params { block_len: 0, blocks_per_frame: 0, codes: [0; 3], thresholds: [0; 3] };
            let (mut sample_rate, mut channels) = (0u32, 0u8);
            unsafe { ffi::x3_reader_spec(reader, &mut sample_rate, &mut p, &mut channels) };
            Ok(X3aReader { reader, spec: X3aSpec { sample_rate, params: Parameters::from_c(&p), channels } })
        }

        pub fn spec(&self) -> &X3aSpec {
            &self.spec
        }

        /// src/decodefile.rs:105-136: `Ok(Some(samples))`, `Ok(None)` at the end of the data / for a payload that
        /// runs past it / for a frame that fails to decode (counted), or the frame's error
        pub fn decode_next_frame(&mut self, wav_buf: &mut [i16; X3_WRITE_BUFFER_SIZE]) -> Result<Option<usize>, X3Error> {
            let mut n = 0u64;
            gpu::with_default(|_| {
                error::check(unsafe {
                    ffi::x3_reader_next_frame(self.reader, wav_buf.as_mut_ptr(), X3_WRITE_BUFFER_SIZE as u64, &mut n)
                })
            })?;
            Ok(if n == 0 { None } else { Some(n as usize) })
        }

        /// frames that failed to decode so far (the reference keeps this private and prints each one)
        pub fn frame_errors(&self) -> usize {
            unsafe { ffi::x3_reader_frame_errors(self.reader) as usize }
        }
    }

    /// src/decodefile.rs:189-212
    pub fn x3a_to_wav<P: AsRef<path::Path>>(x3a_filename: P, wav_filename: P) -> Result<(), X3Error> {
        let (a, b) = (c_path(x3a_filename)?, c_path(wav_filename)?);
        let (mut n, mut bad) = (0u64, 0u64);
        gpu::with_default(|g| error::check(unsafe { ffi::x3_x3a_to_wav(g.raw(), a.as_ptr(), b.as_ptr(), &mut n, &mut bad) }))
    }
}
