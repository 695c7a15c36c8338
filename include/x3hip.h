/*
 * x3hip.h -- C ABI of the MI355X-native X3 encoder/decoder (libx3hip.so).
 *
 * This is the drop-in boundary for the encode/decode hot path of the psiphi75/x3-rust crate
 * (SURVEY.md section 8b).  The reference has no FFI layer of its own: the boundary is its public Rust
 * API, so every entry point below names the Rust item it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the `extern "C"` block + safe wrappers a crate
 * maintainer would add; x3-rust_amd/host/x3.hpp is the same surface for C++ callers and
 * x3-rust_amd/x3hip/ the ctypes binding used by tests and bench.py.
 *
 * Rules of the ABI
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns an int status: 0 = OK, otherwise the 1-based variant index of the
 *     reference's `enum X3Error` (src/error.rs:27-62), or X3_ERR_HIP / X3_ERR_BAD_ARG.
 *     X3_ERR_BAD_ARG is returned where the reference would panic; the library never aborts.
 *   - all bulk work (prediction filter, Rice/BFP/literal coding, bit packing, payload CRC,
 *     stream compaction, decoding) runs in HIP kernels on the context's GPU.  There is no CPU
 *     fallback: without a usable HIP device x3_ctx_create fails with X3_ERR_HIP.
 *   - a context is single-threaded; use one per GPU / per host thread.
 *   - `*_dev` entry points take DEVICE pointers, enqueue on the context's stream and do not
 *     synchronise; x3_ctx_sync() / x3_*_result() wait.
 */
#ifndef X3HIP_H
#define X3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
/* order = `enum X3Error`, src/error.rs:27-62 */
enum x3_status {
  X3_OK = 0,
  X3_ERR_IO = 1,
  X3_ERR_HOUND = 2,
  X3_ERR_BITPACK = 3,
  X3_ERR_INVALID_ENCODING_THRESH = 4,
  X3_ERR_OUT_OF_BOUNDS_INVERSE = 5,
  X3_ERR_MORE_THAN_ONE_CHANNEL = 6,
  X3_ERR_ARCHIVE_HEADER_XML_INVALID = 7,
  X3_ERR_ARCHIVE_HEADER_XML_RICE_CODE = 8,
  X3_ERR_ARCHIVE_HEADER_XML_INVALID_KEY = 9,
  X3_ERR_FRAME_LENGTH = 10,
  X3_ERR_FRAME_HEADER_INVALID_KEY = 11,
  X3_ERR_FRAME_HEADER_INVALID_PAYLOAD_LEN = 12,
  X3_ERR_FRAME_HEADER_INVALID_HEADER_CRC = 13,
  X3_ERR_FRAME_HEADER_INVALID_PAYLOAD_CRC = 14,
  X3_ERR_FRAME_DECODE_INVALID_BLOCK_LENGTH = 15,
  X3_ERR_FRAME_DECODE_INVALID_INDEX = 16,
  X3_ERR_FRAME_DECODE_INVALID_NTOGO = 17,
  X3_ERR_FRAME_DECODE_INVALID_FTYPE = 18,
  X3_ERR_FRAME_DECODE_INVALID_RICE_CODE = 19,
  X3_ERR_FRAME_DECODE_INVALID_BPF = 20,
  X3_ERR_FRAME_DECODE_UNEXPECTED_END = 21,
  X3_ERR_BYTE_WRITER_INSUFFICIENT_MEMORY = 22,
  X3_ERR_HIP = 23,    /* a HIP call failed; see x3_last_error() */
  X3_ERR_BAD_ARG = 24 /* the reference would panic (index out of range, 0 samples, ...) or the
                         argument is outside what the GPU path supports */
};

const char* x3_strerror(int status);

/* ------------------------------------------------------------------ types */

/* x3::Parameters (src/x3.rs:81-134); rice_codes[] is derived from codes[]. */
typedef struct x3_params {
  uint32_t block_len;        /* DEFAULT_BLOCK_LENGTH 20, MAX_BLOCK_LENGTH 60 */
  uint32_t blocks_per_frame; /* DEFAULT_BLOCKS_PER_FRAME 500 */
  uint32_t codes[3];         /* DEFAULT_RICE_CODES {0,1,3} */
  uint32_t thresholds[3];    /* DEFAULT_THRESHOLDS {3,8,20} */
} x3_params;

/* x3::FrameHeader (src/x3.rs:148-184) */
typedef struct x3_frame_header {
  uint8_t source_id;
  uint8_t channels;
  uint16_t samples;
  uint32_t payload_len;
  uint16_t payload_crc;
} x3_frame_header;

#define X3_FRAME_HEADER_LENGTH 20   /* FrameHeader::LENGTH */
#define X3_FRAME_KEY 0x7833         /* FrameHeader::KEY "x3" */
#define X3_FRAME_MAX_LENGTH 0x7fe0  /* Frame::MAX_LENGTH */
#define X3_READ_BUFFER_SIZE 24576   /* decodefile.rs:44 */

typedef struct x3_ctx x3_ctx;

/* ------------------------------------------------------------------ context */

/* Create a context on HIP device `device` with its own non-blocking stream. */
int x3_ctx_create(int device, x3_ctx** ctx);
/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
int x3_ctx_create_on_stream(int device, void* hip_stream, x3_ctx** ctx);
void x3_ctx_destroy(x3_ctx* ctx);
int x3_ctx_sync(x3_ctx* ctx);
/* Text of the last HIP failure seen by this context ("" if none). */
const char* x3_last_error(const x3_ctx* ctx);

/* Tuning / testing knobs of a context.  Each has an X3HIP_* environment variable that gives its initial value;
 * the environment is read ONCE, in x3_ctx_create -- no later call looks at it.
 *   "two_pass" (X3HIP_TWO_PASS)            1: always encode with the two-pass kernels (no persistent grid)
 *   "stream_wgs" (X3HIP_STREAM_WGS)        workgroups per CU of the single-pass encoder, 0 = derived from occupancy
 *   "decode_single" (X3HIP_DECODE_SINGLE)  1: single-wave decoder kernels only
 *   "decode_blocks" (X3HIP_DECODE_BLOCKS)  1: block length 20 on round 6's block-per-lane decoder (a walker wave finds where the
 *                                          blocks begin, three decoder waves decode a block per lane) where the three-wave
 *                                          kernel would run; same results, 0.78-0.82 against 0.65-0.69 ms on config 3.  Block
 *                                          lengths 10 and 40 take that decoder by default ("decode_blocks_off" = 1: not).
 *                                          Read-only "decode_kernel_in_use": 3 = block per lane, 2 = three waves per 64
 *                                          frames, 1 / 0 = single wave
 *   (environment only) X3HIP_SPIN_WAIT=1   the process's waits for the GPU spin instead of sleeping (hipDeviceScheduleSpin,
 *                                          process-wide, effective when x3_ctx_create is the process's first use of the
 *                                          device): calls that end with a trip to the host come back ~20 us sooner
 *                                          (x3_decode_stream_dev on config 3: 0.82 -> 0.79 ms), a core is busy meanwhile
 *   (environment only) X3HIP_FENCE=16      debugging: every device buffer of the library (its own and x3_dev_alloc's) is
 *                                          mapped with unmapped pages on both sides and ends, rounded up to that many bytes,
 *                                          at the end of its mapping; X3HIP_FENCE_FILL=<byte> fills it.  The kernels read
 *                                          aligned 16-byte chunks, so 16 is the tightest fence (csrc/x3_fence.h)
 *   "wav_offsets_x4"                       1: a promise -- every d_wav_offsets[] passed to x3_decode_dev is a multiple of
 *                                          four samples (rows on 8-byte boundaries): such calls then take the three-wave
 *                                          decoder like the other layouts do; an offset that breaks the promise garbles
 *                                          its frame's samples AND may clobber up to three samples in front of the frame's
 *                                          range (the rows leave in whole 8-byte pieces from the piece their first sample
 *                                          lies in): the promise is the caller's to keep
 *   "host_walk" (X3HIP_HOST_WALK)          frame walk of x3_decode_stream: 1 host, 0 GPU, -1 by stream size
 *   "host_chunk_frames" (X3HIP_HOST_CHUNK_FRAMES)  x3_encode and x3_decode_stream take a long host buffer in chunks of whole
 *                                           frames, downloads beside uploads: 0 = on (x3_encode from 32 Mi samples in chunks of
 *                                           16 Mi; x3_decode_stream from 16 MiB of stream in chunks that grow from 16 Mi to
 *                                           128 Mi samples), N > 0 = chunks of N frames whatever the length (tests), -1 = one
 *                                           piece.  A call that goes in chunks starts two helper threads for its duration
 *                                           (pageable copies hold their caller); the results are the same either way.
 *   "file_chunk_frames" (X3HIP_FILE_CHUNK_FRAMES), "file_workers" (X3HIP_FILE_WORKERS)   x3_wav_to_x3a / x3_x3a_to_wav
 *   "file_tune" (X3HIP_FILE_TUNE)          1: x3_wav_to_x3a makes one tuning pass over the WAV's samples first and writes the
 *                                          archive with the parameters x3_tune chooses (section "parameter tuning"); 0
 *                                          (default): the reference's defaults, byte for byte
 *   "reader_window_frames" (X3HIP_READER_WINDOW_FRAMES)   frames x3_reader decodes ahead per launch set
 *   "check_main" (X3HIP_CHECK_MAIN)        1: the check pass on the context's stream, the decoder on the side stream (experiment)
 *   "check_wgs", "check_prio", "check_first"   grid, queue priority and launch order of the check pass (experiments)
 *   "verbose" (X3HIP_VERBOSE)
 * x3_ctx_get_option also reads "encode_fallbacks" (launches of the single-pass encoder that timed out waiting for
 * a non-resident workgroup and were redone by the two-pass kernels), "stream_wgs_in_use", and "encode_pace" /
 * "decode_pace": what the slowest workgroup of the last encoder / decoder launch achieved, in 10 ns ticks per frame /
 * in shader clocks per 16 blocks -- the next launch paces its waves' priorities by it (x3_encode_stream2_kernel.h,
 * x3_decode_split_kernel.h); reading them synchronizes.
 * Read-only "last_decode_replays": frames the fast decoders handed to the reference's own reader (a decode error, a zero
 * run of 32 bits or more, or a read behind the payload's last byte: x3_decode_replay.h) -- of the launch the last
 * x3_decode_result read, or of the last x3_decode_stream (summed over its chunks), x3_decode_stream_dev or
 * x3_decode_stream_mc as a whole (there: the frames its per-thread kernel decoded, all of them with "mc_decode_threads" = 1).
 * A stream an encoder wrote has none.  Read-only "last_window_replays": the (window, covering frame) pairs the last
 * x3_decode_windows_dev re-decoded that way, read after x3_decode_windows_result.
 * The GPU frame walk (x3_index_dev, x3_decode_stream_dev, x3_decode_stream of 4-16 MiB): "index_no_fast" = 1 skips its
 * fast path (one clean chain of frames) and takes the general one (candidates, hash table, pointer doubling) every time.
 * Read-only counters: "index_fast_walks" / "index_general_walks" (walks each path has served), "stream_one_trip"
 * (x3_decode_stream_dev calls served with one trip to the host), "last_index_candidates" (valid headers at any byte offset
 * that the last general walk found; 0 before the first) and "index_rescans" (general walks that found more candidates than
 * their first buffer held and scanned the stream a second time).
 * x3_decode_streams_dev: read-only "streams_general_walks" (entries so far that the segmented fast walk left to the
 * general walk) and "last_streams_general_walks" (of the last x3_decode_streams_result).
 * x3_levels_dev / x3_corpus_levels_dev: read-only "last_levels_replays" (frames of the last call that were decoded through
 * the reference's reader instead of by stretches: flagged ones, and frames whose offsets are out of order; read after
 * x3_levels_result).
 * x3_events_dev / x3_corpus_events_dev: read-only "events_tile_rows" (rows a workgroup of the events kernels takes at a
 * time; for tests that lay rows at tile edges).
 * x3_range_levels_dev / x3_corpus_range_levels_dev: read-only "last_range_levels_replays" (the (range, covering frame)
 * pairs of the last call that its fix-up decoded through the reference's reader) and "last_range_levels_overflow" (its pairs
 * that had no partial rows in the workspace: those beyond the P pairs it holds, and those whose bins end behind its rows; the
 * fix-up decodes them where their frame passed its check, so the two need not be equal); read after x3_range_levels_result.
 * x3_corpus_build: read-only "last_corpus_record_slices" (slices of frames the last build recorded its segment index in;
 * 0 without an index).
 * x3_seg_index_build_dev: read-only "last_seg_index_irregular" (frames of the last build -- x3_corpus_build's with
 * X3_CORPUS_INDEX_WALK included -- whose walk stopped early: they have no valid entry from there on; reading it synchronizes).
 * Unknown name: X3_ERR_BAD_ARG. */
int x3_ctx_set_option(x3_ctx* ctx, const char* name, long long value);
int x3_ctx_get_option(const x3_ctx* ctx, const char* name, long long* value);

/* HIP-event timing of individual kernels on the context's stream (bench.py's roofline leg).
 * which: 0 = encode kernel, 1 = decode kernel, 2 = frame-size kernel, 3 = scan kernel,
 *        4 = frame check (header + payload CRC) kernel, 5 = the encoder's dense pass (frames the wave encoder's LDS image
 *        does not hold: x3_encode_dev below).  Every timed kernel costs a marker behind its dispatch packet (~5 us each,
 *        five a round trip); option "kernel_timing_mask" (bit k = kernel id k, default all) chooses which ones carry them. */
int x3_ctx_enable_kernel_timing(x3_ctx* ctx, int enable);
int x3_ctx_kernel_time(x3_ctx* ctx, int which, double* total_ms, uint64_t* launches); /* syncs */
int x3_ctx_reset_kernel_time(x3_ctx* ctx);
/* Every timed launch's own time in ms, oldest first (which as above; 5 = the encoder's dense pass): *launches = how many
 * there are, the first min(cap, *launches) are written.  Syncs. */
int x3_ctx_kernel_times(x3_ctx* ctx, int which, double* ms, uint64_t cap, uint64_t* launches);
/* The launch log the kernels keep themselves: the last (up to 256) launches of the decoder (which = 1) or the wave
 * encoder (which = 0), oldest first, four words each: the pace the launch aimed at and the pace its slowest group
 * achieved (10 ns ticks per 16 blocks; decoder only, else 0), the shader clock in kHz that workgroup 0 measured over
 * its life (shader ticks against the constant 100 MHz clock), and that life in 10 ns ticks.  Syncs.  For benchmarks:
 * a reader of the line can tell a slow box (clock) from a controller that has not settled (target vs achieved). */
int x3_ctx_launch_log(x3_ctx* ctx, int which, uint32_t* out /* 4 * cap_entries */, uint64_t cap_entries, uint64_t* n_entries);

/* ------------------------------------------------------------------ x3.rs */

/* `impl Default for Parameters`, src/x3.rs:124-134 */
void x3_params_default(x3_params* p);
/* `Parameters::new`, src/x3.rs:98-122: INVALID_ENCODING_THRESH if thresholds[k] > offset of
 * code k for k = 0,1 (the reference checks only those two); BAD_ARG for a code > 3. */
int x3_params_validate(const x3_params* p);
/* `RiceCode` / `RiceCodes::get`, src/x3.rs:187-260: the code table Parameters.rice_codes[k] points at.  `code` and
 * `num_bits` have `len` entries indexed by (difference + offset); `inv` has 60 entries of which inv_len are in use.  The
 * pointers are to static read-only tables of the library (host memory; the kernels derive the same values arithmetically).
 * BAD_ARG for a code number > 3 (the reference panics on the index). */
typedef struct x3_rice_code {
  uint32_t nsubs, offset, len, inv_len;
  const uint32_t* code;
  const uint32_t* num_bits;
  const int16_t* inv;
} x3_rice_code;
int x3_rice_code_get(uint32_t code_number, x3_rice_code* out);
/* number of frames `encode` cuts n samples into (encoder.rs:61-73) */
uint64_t x3_num_frames(uint64_t n, const x3_params* p);
/* worst-case bytes `encode` can produce for n samples (all-literal frames) */
uint64_t x3_encode_bound(uint64_t n, const x3_params* p);

/* ------------------------------------------------------------------ crc.rs */

/* `crc::crc16`, src/crc.rs:49-58 -- computed on the GPU as a segmented reduction. */
int x3_crc16(x3_ctx* ctx, const uint8_t* data, uint64_t n, uint16_t* crc);
int x3_crc16_dev(x3_ctx* ctx, const uint8_t* d_data, uint64_t n, uint16_t* crc); /* syncs */
/* `crc::update_crc16`, src/crc.rs:44-47 -- one byte, host arithmetic. */
uint16_t x3_crc16_update(uint16_t crc, uint8_t byte);

/* ------------------------------------------------------------------ encoder.rs */

/* `encoder::encode` into a `SliceByteWriter` (src/encoder.rs:51-111, bytewriter.rs:27-100).
 * wav[0..n) is the single channel's samples (`x3::Channel::wav` / a collected `IterChannel`);
 * n_channels is `channels.len()` (>1 -> MORE_THAN_ONE_CHANNEL, 0 -> BAD_ARG).  The writer is
 * out[0..out_cap) positioned at start_pos; frames are appended back to back, each preceded by
 * zero padding to an even ABSOLUTE position.  *out_pos receives `writer.stream_position()`.
 * stats[6] (may be NULL) receives the per-sample block-type counts the reference prints
 * (Rice nsubs 0..3, BFP = 4, literal = 5; encoder.rs:96-108,199).
 * On BYTE_WRITER_INSUFFICIENT_MEMORY the slice holds what the reference's holds (bytewriter.rs:86-99,
 * encoder.rs:67-73): every frame that fits, complete and in place (and the pad byte in front of
 * the first one); *out_pos = the end of the last of them, nothing behind it is touched (the
 * reference goes on into the frame that does not fit and leaves some of its payload bytes without
 * a header there).  x3_ctx_get_option("encode_needed_pos") says where the whole stream would have
 * ended. */
int x3_encode(x3_ctx* ctx, const int16_t* wav, uint64_t n, uint32_t n_channels, const x3_params* p,
              uint8_t* out, uint64_t out_cap, uint64_t start_pos, uint64_t* out_pos, uint64_t stats[6]);

/* `encoder::encode_frame` (src/encoder.rs:175-214): exactly one frame from wav[0..n), n >= 1. */
int x3_encode_frame(x3_ctx* ctx, const int16_t* wav, uint64_t n, const x3_params* p, uint8_t* out,
                    uint64_t out_cap, uint64_t start_pos, uint64_t* out_pos, uint64_t stats[6]);

/* `encoder::write_frame_header` (src/encoder.rs:122-162); 20 bytes of host arithmetic. */
void x3_write_frame_header(uint64_t num_samples, uint8_t id, uint64_t payload_len, uint16_t payload_crc,
                           uint8_t out[X3_FRAME_HEADER_LENGTH]);

/* Batched `encode`: `count` independent clips (BASELINE config 5).  Clip c is wavs[c][0..ns[c]).
 * The clips' streams are written back to back into out[0..out_cap); clip_offsets[count+1]
 * receives where each starts/ends (all even).  Equivalent to `count` calls of x3_encode. */
int x3_encode_batch(x3_ctx* ctx, const int16_t* const* wavs, const uint64_t* ns, uint64_t count,
                    const x3_params* p, uint8_t* out, uint64_t out_cap, uint64_t* clip_offsets,
                    uint64_t stats[6]);

/* ------------------------------------------------------------------ decoder.rs / decodefile.rs */

/* `decoder::read_frame_header` (src/decoder.rs:69-118); 20 bytes of host arithmetic.
 * Check order: length, header CRC, key, channels <= 1, payload_len < Frame::MAX_LENGTH. */
int x3_read_frame_header(const uint8_t* bytes, uint64_t len, x3_frame_header* h);

/* `decoder::decode_frame` (src/decoder.rs:36-58): payload[0..len) -> wav[0..samples).
 * Does not check any CRC (the reference does not either).  wav_cap = `wav_buf.len()`: a buffer shorter than `samples`
 * is the reference's slice-index panic (X3_ERR_BAD_ARG) at the first block that does not fit -- unless a block in
 * front of it fails, whose error comes first, as in the reference (decoder.rs:49).  Payloads and sample counts beyond
 * what a frame header or the walk's read buffer allow (>= 32 736 / > 24 576 bytes, > 65 535 samples) are decoded too,
 * by the reference-exact reader on one GPU thread: correct, slow. */
int x3_decode_frame(x3_ctx* ctx, const uint8_t* payload, uint64_t len, int16_t* wav, uint64_t wav_cap,
                    const x3_params* p, uint64_t samples, uint64_t* n_out);

/* The frame walk of `X3aReader::decode_next_frame` looped as `x3a_to_wav` does
 * (src/decodefile.rs:93-136,200-209) over an in-memory frame stream x3[0..len) (no archive
 * header): stop at end of data, at the first hard error (returned), or at the first frame whose
 * payload fails to decode (counted in *frame_errors, return 0).  wav receives the samples of
 * the frames before the stop; *n_out their count; *frames_ok the number of good frames.
 * (Streams of 4 MiB and more are uploaded first and walked on the GPU, x3_index_dev's way; shorter ones are
 * walked on the host.  Same results either way.)  wav_cap is this API's, not the reference's (x3a_to_wav writes to a
 * file): a frame that does not fit behind the samples so far ends the walk with X3_ERR_BAD_ARG once its CRCs have
 * passed -- also when an early block of that very frame would not have decoded. */
int x3_decode_stream(x3_ctx* ctx, const uint8_t* x3, uint64_t len, const x3_params* p, int16_t* wav,
                     uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok, uint64_t* frame_errors);

/* ------------------------------------------------------------------ multi-channel (extension) */

/* NOT in the reference: `encoder::encode` returns MoreThanOneChannel for more than one channel (src/encoder.rs:55-57) and
 * `read_frame_header` refuses frames that announce more than one (src/decoder.rs:90-94) -- and so do x3_encode /
 * x3_decode_stream and every other entry point above.  These two follow what the format foresees: the frame header's
 * <Num Channels> (src/x3.rs:155-156, src/encoder.rs:134) and "pack the data block for each channel" (src/encoder.rs:197):
 * <Audio State> = the first sample of each channel; then for every block index the block of channel 0 .. n-1, each coded
 * as a mono block against its own channel; header byte 3 = n_channels, `samples` = samples per channel.  With
 * n_channels = 1 the bytes are x3_encode's.  wavs[k] = channel k, n samples each (host memory).  n_channels <= 8; a frame
 * whose payload would pass the 24 KB a reader takes is X3_ERR_FRAME_LENGTH (choose shorter frames).
 * On BYTE_WRITER_INSUFFICIENT_MEMORY x3_encode_mc keeps x3_encode's prefix guarantee: every frame that fits is in out,
 * complete and in place (with the pad byte in front of the first one), *out_pos = the end of the last of them, and
 * nothing behind it or in front of start_pos is touched.
 * x3_decode_stream_mc walks, checks and decodes such a stream (x3_decode_stream's rules; a frame must announce exactly
 * n_channels) into wavs[k][0 .. *n_samples). */
int x3_encode_mc(x3_ctx* ctx, const int16_t* const* wavs, uint32_t n_channels, uint64_t n, const x3_params* p, uint8_t* out,
                 uint64_t out_cap, uint64_t start_pos, uint64_t* out_pos, uint64_t stats[6]);
int x3_decode_stream_mc(x3_ctx* ctx, const uint8_t* x3, uint64_t len, uint32_t n_channels, const x3_params* p,
                        int16_t* const* wavs, uint64_t wav_cap, uint64_t* n_samples, uint64_t* frames_ok,
                        uint64_t* frame_errors);

/* ------------------------------------------------------------------ bitreader.rs / bitpacker.rs / decode_block */

/* The reference's small public items, for callers and known-answer tests written against them (x3_bits.h: not how the
 * bulk paths work, and a call per field is not how a GPU should be driven -- but what they compute is computed by
 * this library on the GPU, not by a CPU re-implementation).
 * `BitReader` (src/bitreader.rs:51-176): state and a copy of the array live in device memory; each call runs the
 * reference-exact reader (one thread) and brings the result back.  x3_bitreader_state: the reference's private
 * fields (idx, leading_word, rem_bit), for tests that assert on them. */
typedef struct x3_bitreader x3_bitreader;
int x3_bitreader_new(x3_ctx* ctx, const uint8_t* array, uint64_t len, x3_bitreader** br);
int x3_bitreader_read_nbits(x3_bitreader* br, uint32_t n, uint32_t* value);
int x3_bitreader_count_zero_bits(x3_bitreader* br, uint32_t* count);
int x3_bitreader_inc_bits(x3_bitreader* br, uint32_t n);
int x3_bitreader_state(const x3_bitreader* br, uint64_t* idx, uint32_t* leading_word, uint32_t* rem_bit);
void x3_bitreader_free(x3_bitreader* br);
/* Not in the reference: announce a frame stream in host memory (frames back to back, no archive header) whose frames
 * will be handed to x3_decode_frame one by one, as a loop over `decode_frame` does.  Calls whose payload lies in the
 * announced buffer are then served from windows of frames that are walked, checked and decoded ahead in one launch
 * set (a header parse and a memcpy per call instead of a dispatch per call); every other call, and every frame the
 * window did not decode cleanly, takes the per-call path: the results are those of x3_decode_frame without the
 * announcement.  The buffer must stay unchanged until the next x3_decode_prefetch (x3 = NULL drops it) or
 * x3_ctx_destroy. */
int x3_decode_prefetch(x3_ctx* ctx, const uint8_t* x3, uint64_t len, const x3_params* p);

/* `decoder::decode_block` (src/decoder.rs:132-145): wav[0..n) from the reader's position, *last_wav in and out.
 * n <= 60 (MAX_BLOCK_LENGTH); n == 0 is the reference's empty slice (type bits read; a BFP block then fails or panics). */
int x3_decode_block(x3_bitreader* br, int16_t* wav, uint32_t n, int16_t* last_wav, const x3_params* p);
/* `BitPacker` (src/bitpacker.rs:46-177) over a slice writer at start_pos: write_bits / write_packed_zeros / word_align
 * are recorded; x3_bitpacker_finish (= flush, what Drop does) zero-pads a partial byte, packs all recorded fields on the
 * GPU (scan of the field widths, fields OR-ed into place), writes the bytes not handed over yet behind start_pos and
 * returns the reference's len() and crc() at that point (cumulative since new(); CRC-16 init 0xFFFF) and the writer's
 * position; writing may go on from the next byte.  x3_bitpacker_peek = len() / crc() between writes: complete bytes
 * so far and their CRC, nothing written.  A packer over any other ByteWriter is made with out = NULL, out_cap = 0
 * (start_pos = the writer's position: word_align needs its parity) and flushed with x3_bitpacker_take, which delivers
 * the bytes not handed over yet into dst[0, *n_new) for the caller to pass on. */
typedef struct x3_bitpacker x3_bitpacker;
int x3_bitpacker_new(x3_ctx* ctx, uint8_t* out, uint64_t out_cap, uint64_t start_pos, x3_bitpacker** bp);
int x3_bitpacker_write_bits(x3_bitpacker* bp, uint64_t value, uint32_t num_bits);
int x3_bitpacker_write_packed_zeros(x3_bitpacker* bp, uint32_t num_zeros);
/* BitPacker::write_bytes (bitpacker.rs:95-102): the bytes go to the writer at once -- in front of a partial byte the packer
 * still holds -- and count in len() and crc(); BitPacker::inc_counter_n_bytes (:112-118): the writer skips n bytes, len()
 * and crc() stay (X3_ERR_BITPACK = BitPackError::NotByteAligned off a byte boundary; slice-bound packers only). */
int x3_bitpacker_write_bytes(x3_bitpacker* bp, const uint8_t* array, uint64_t n);
int x3_bitpacker_inc_counter_n_bytes(x3_bitpacker* bp, uint64_t n_bytes);
int x3_bitpacker_word_align(x3_bitpacker* bp);
int x3_bitpacker_finish(x3_bitpacker* bp, uint64_t* len, uint16_t* crc, uint64_t* out_pos);
int x3_bitpacker_peek(const x3_bitpacker* bp, uint64_t* len, uint16_t* crc);
int x3_bitpacker_take(x3_bitpacker* bp, uint8_t* dst, uint64_t dst_cap, uint64_t* n_new, uint64_t* len, uint16_t* crc);
void x3_bitpacker_free(x3_bitpacker* bp);

/* ------------------------------------------------------------------ .x3a archive (encodefile.rs / decodefile.rs) */

/* `create_archive_header` (src/encodefile.rs:82-138): "X3ARCHIV" + a frame header with id 0 / 0 samples
 * + the XML configuration (zero-padded to even length).  Host arithmetic.  *out_len = bytes written. */
int x3_archive_header_write(uint32_t sample_rate, const x3_params* p, uint8_t* out, uint64_t out_cap,
                            uint64_t* out_len);
/* `read_archive_header` + `parse_xml` (src/decodefile.rs:142-176,232-303).  *header_size is what the
 * reference returns (20 + XML payload, NOT counting the 8-byte id); the audio frames start at
 * 8 + *header_size.  blocks_per_frame is the default (the XML does not carry it). */
int x3_archive_header_read(const uint8_t* bytes, uint64_t len, uint32_t* sample_rate, x3_params* p,
                           uint8_t* channels, uint64_t* header_size);
/* `wav_to_x3a` without the file I/O (src/encodefile.rs:48-77): archive header + `encode` of one 16-bit
 * mono channel with default parameters, into out[0..out_cap). */
int x3_x3a_encode(x3_ctx* ctx, const int16_t* wav, uint64_t n, uint32_t sample_rate, uint8_t* out,
                  uint64_t out_cap, uint64_t* out_len, uint64_t stats[6]);
/* `x3a_to_wav` without the file I/O (src/decodefile.rs:189-212 with X3aReader, :59-136): archive header,
 * then the frame walk with the reader's own byte accounting. */
int x3_x3a_decode(x3_ctx* ctx, const uint8_t* x3a, uint64_t len, int16_t* wav, uint64_t wav_cap,
                  uint64_t* n_out, uint32_t* sample_rate, uint64_t* frames_ok, uint64_t* frame_errors);

/* The file level: `encodefile::wav_to_x3a` (src/encodefile.rs:48-77) and `decodefile::x3a_to_wav`
 * (src/decodefile.rs:189-227) -- what the reference's CLI calls (src/bin/x3.rs:79-80).  Streaming: the file
 * moves through the GPU in chunks of whole frames (pread -> pinned staging -> H2D -> kernels -> D2H ->
 * pwrite, neighbouring chunks overlapped on a few worker contexts), so memory is bounded whatever the
 * file size; the bytes written are those of x3_x3a_encode / x3_x3a_decode on the whole file.
 * WAV container as `hound` 3.4.0 handles it for the only format the reference accepts: 16-bit integer PCM,
 * one channel (anything else: X3_ERR_BAD_ARG, where the reference asserts); output is hound's canonical
 * 44-byte header + samples.  A file that cannot be opened or read: X3_ERR_IO (the reference unwraps);
 * an output .wav that cannot be created: X3_ERR_HOUND (`WavWriter::create(..)?`).
 * x3_x3a_to_wav leaves, like the reference's dropped WavWriter, a valid WAV of the samples in front of the
 * frame that ended the walk, also when it returns an error.
 * Tuning (x3_ctx_set_option): "file_chunk_frames" (default 800 frames = 16 MB of samples), "file_workers"
 * (default 4; the workers' contexts share the single-pass encoder through a gate -- one chunk's encode launch at a time,
 * uploads, downloads and file I/O side by side). */
int x3_wav_to_x3a(x3_ctx* ctx, const char* wav_path, const char* x3a_path, uint64_t stats[6]);
int x3_x3a_to_wav(x3_ctx* ctx, const char* x3a_path, const char* wav_path, uint64_t* n_samples,
                  uint64_t* frame_errors);

/* `X3aReader` (src/decodefile.rs:47-137): open / spec / decode_next_frame -- one frame per call, for callers written
 * against the reference's incremental reader.  A call that finds nothing prepared decodes a window of frames ahead in
 * one launch set (option "reader_window_frames", default 4096) and the following calls are a header parse and a
 * memcpy.  x3_reader_next_frame = `decode_next_frame`: *n_out = the frame's sample count (Ok(Some(n))), or 0 with
 * X3_OK for Ok(None) -- end of the data, a payload that runs past it, or a frame that fails to decode (counted:
 * x3_reader_frame_errors) -- or an error status; as in the reference the reader has then consumed the frame and a
 * further call goes on behind it.  wav needs room for the frame (<= 65535 samples).  x3_reader_open_mem reads an
 * archive that is in memory (borrowed: it must outlive the reader). */
typedef struct x3_reader x3_reader;
int x3_reader_open(x3_ctx* ctx, const char* x3a_path, x3_reader** reader);
int x3_reader_open_mem(x3_ctx* ctx, const uint8_t* x3a, uint64_t len, x3_reader** reader);
int x3_reader_spec(const x3_reader* reader, uint32_t* sample_rate, x3_params* p, uint8_t* channels);
int x3_reader_next_frame(x3_reader* reader, int16_t* wav, uint64_t wav_cap, uint64_t* n_out);
uint64_t x3_reader_frame_errors(const x3_reader* reader);
uint64_t x3_reader_position(const x3_reader* reader); /* byte offset in the archive of the next frame header */
void x3_reader_close(x3_reader* reader);

/* ------------------------------------------------------------------ device-resident API */

/* Geometry of a uniform batch resident in HBM: n_clips clips of n_per_clip samples, clip c
 * starting at d_wav + c*clip_stride (samples).  A single stream is n_clips = 1. */
typedef struct x3_batch {
  uint64_t n_per_clip;
  uint64_t clip_stride;
  uint64_t n_clips;
} x3_batch;

/* Encode a device-resident batch into d_out[0..out_cap) starting at start_pos (even or odd; an
 * odd start is zero-padded to even as the reference does).  d_frame_offsets (may be NULL)
 * receives F+1 byte offsets: frame f occupies [d_frame_offsets[f], d_frame_offsets[f+1]).
 * Asynchronous; results via x3_encode_result().
 *   Content: frames whose payload does not fit the wave encoder's LDS image (more than 9 728 bytes: loud or noisy
 * material) are written by a dense pass that follows the encode kernel IN THE SAME STREAM, at the offsets that kernel
 * assigned -- whatever is enqueued on the context's stream behind this call (x3_decode_dev, a copy) finds the whole
 * stream, with or without x3_encode_result() in between; no call is encoded twice for its content (until round 3 the
 * whole call was encoded again inside x3_encode_result).  Options "last_dense_frames", "encode_dense_frames" count such
 * frames, "enc_gen_in_use" says which kernel served the last call -- 3 the wave encoder, 2 the second generation, 1 the
 * general kernel in one pass (any block length: sizes by decoupled look-back), 0 the same kernel in two passes (option
 * "two_pass", or what a launch falls back to whose waits gave up) -- (a call with more than a quarter of dense
 * frames makes the context's next call start on the second-generation kernel: a speed hint, the bytes are the same).
 *   Layout: the results never depend on it, the kernels that serve a call do.  block_len 20, 10 or 40 with frames of at most
 * 10 240 samples (512 blocks of 20), d_wav on a dword boundary and (for n_clips > 1) a clip_stride that is a multiple of four samples take the single-pass
 * encoders; x3_decode_dev takes the three-wave decoder when its output begins on an 8-byte boundary and the stride is a
 * multiple of four samples (rows on 16-byte boundaries leave in 16-byte pieces, on 8-byte ones in 8-byte pieces, always
 * as whole 128-byte lines).  Anything else -- other block lengths or code sets, longer frames, odd strides -- is served by
 * the general kernels, three to eight times slower ("GPU-path limits").
 *   Residency: the default-geometry encoder is a persistent grid whose workgroups wait for each other's frame
 * sizes; on a GPU that this context does not have to itself a launch can find them not all resident, gives up after a
 * bounded wait (15-30 ms: a stall of that length per call on a GPU shared with another process's long kernels), and
 * x3_encode_result() then re-encodes with the general kernels (option "encode_fallbacks" counts
 * these).  That re-run reads d_wav again and rewrites d_out[start_pos ..): d_wav and d_out must stay untouched until
 * x3_encode_result() has returned, and the stream is only trusted once it has returned X3_OK (launching x3_decode_dev
 * on the same context in between is fine -- same stream -- as long as its result is only used after that). */
int x3_encode_dev(x3_ctx* ctx, const int16_t* d_wav, const x3_batch* batch, const x3_params* p,
                  uint8_t* d_out, uint64_t out_cap, uint64_t start_pos, uint64_t* d_frame_offsets);
/* The same for frames taken from anywhere in a device buffer: frame f is the src_samples[f] samples
 * (1 .. block_len * blocks_per_frame) at d_wav + src_offsets[f]; the stream holds them in this order.  A batch of clips of
 * DIFFERENT lengths is such a list (each clip cut into frames as encoder::encode cuts it, encoder.rs:61-73: full frames and
 * a last short one), one launch set for all of them instead of one per clip; d_frame_offsets[F + 1] then gives every clip's
 * byte range.  src_offsets / src_samples are HOST arrays (checked and copied here); offsets that are all even take the
 * single-pass encoders.  Asynchronous like x3_encode_dev; results via x3_encode_result().  One exception to "does not
 * synchronise": the table travels through ONE pinned block per context, so a call waits on the host until the table copy
 * of the context's previous x3_encode_frames_dev / x3_decode_streams_dev has run -- it waits out whatever stands in front
 * of that copy in the stream, nothing behind it. */
int x3_encode_frames_dev(x3_ctx* ctx, const int16_t* d_wav, const uint64_t* src_offsets, const uint32_t* src_samples,
                         uint64_t n_frames, const x3_params* p, uint8_t* d_out, uint64_t out_cap, uint64_t start_pos,
                         uint64_t* d_frame_offsets);
/* Waits for the last x3_encode_dev / x3_encode_frames_dev; status is X3_OK, BYTE_WRITER_INSUFFICIENT_MEMORY or BAD_ARG.
 * On BYTE_WRITER_INSUFFICIENT_MEMORY *out_pos = the position the whole stream would have reached, d_frame_offsets holds
 * every frame's offset as if there had been room, and d_out holds every frame that fits (offset + size <= out_cap),
 * complete and in place -- the prefix the reference's slice keeps; a frame that does not fit is not written at all. */
int x3_encode_result(x3_ctx* ctx, uint64_t* out_pos, uint64_t stats[6]);

/* Decode F frames of a device-resident stream.  d_frame_offsets[f] = byte offset of frame f's
 * header in d_x3 (F entries used).  Frame f's samples go to d_wav + d_wav_offsets[f] when
 * d_wav_offsets != NULL, else to the position implied by `batch` and p (the layout
 * x3_encode_dev consumed).  Every frame's header CRC, key, channel count, length and payload CRC
 * are verified on the GPU; d_status (F int32, may be NULL -> internal) receives a status per frame.
 * Asynchronous; results via x3_decode_result(). */
int x3_decode_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                  uint64_t n_frames, const x3_batch* batch, const uint64_t* d_wav_offsets,
                  const x3_params* p, int16_t* d_wav, uint64_t wav_cap, int32_t* d_status);
/* ---- The SEGMENT INDEX: decoding a frame on more than one lane.
 * A frame is one serial bit stream (decoder.rs:36-58), so a stream of few frames cannot be decoded faster than one
 * frame's walk, however many lanes there are.  But a block depends only on the bit position it starts at and on the
 * sample in front of it.  The segment index holds both for every `seg_blocks`-th block of every frame: entry
 * [1 + f * (nseg - 1) + j - 1], j = 1 .. nseg - 1 with nseg = ceil(blocks_per_frame / seg_blocks), is the 64-bit word
 * {bits 0..31: bit offset of block seg_blocks * j's header from the start of frame f's payload; bits 32..47: the
 * sample in front of that block; bit 48: entry valid}.  The encoder knows it (x3_encode_dev_seg), and so does a
 * decoder that has been through the stream once (record = 1).  With it, x3_decode_dev_seg decodes nseg stretches of
 * every frame side by side.  The index is NOT part of the .x3a format and is never trusted: every stretch checks where
 * it ended -- bit position and last sample -- against the next entry, which proves (by induction from the frame's
 * first block) that the frame decoded as the serial walk decodes it; a frame with a missing, implausible or
 * contradicted entry goes through the reference's reader, as frames with decode errors do.  A wrong or stale index
 * costs time, never correctness.  Word 0 is a header (who fills the index says so there, and with what seg_blocks; an
 * index without it decodes frame by frame).  The decoder takes as many stretches per frame as fill the GPU -- every
 * entry for a stream of a few dozen frames, every second or fourth for a few hundred, none when the frames alone fill
 * it (option "seg_stretches" overrides; "last_seg_stretches" reports).  seg_blocks: a multiple of 4;
 * d_seg_index: x3_seg_index_entries() words of 8 bytes, 8-byte aligned; NULL = x3_decode_dev / x3_encode_dev.
 * (Layouts the three-wave decoder does not take -- see x3_encode_dev, "Layout" -- decode frame by frame and record
 * nothing: entries stay invalid.) */
uint64_t x3_seg_index_entries(uint64_t n_frames, const x3_params* p, uint32_t seg_blocks);
/* x3_encode_dev that also fills the segment index (seg_blocks: a power of two >= 4; 32 or 64 for 500-block frames).  Only
 * the default-geometry encoder fills it; any other layout leaves an index that says "none" and decodes frame by frame. */
int x3_encode_dev_seg(x3_ctx* ctx, const int16_t* d_wav, const x3_batch* batch, const x3_params* p,
                      uint8_t* d_out, uint64_t out_cap, uint64_t start_pos, uint64_t* d_frame_offsets,
                      uint64_t* d_seg_index, uint32_t seg_blocks);
int x3_decode_dev_seg(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                      uint64_t n_frames, const x3_batch* batch, const uint64_t* d_wav_offsets,
                      const x3_params* p, int16_t* d_wav, uint64_t wav_cap, int32_t* d_status,
                      uint64_t* d_seg_index, uint32_t seg_blocks, int record);
/* The segment index of a stream somebody else wrote, WITHOUT decoding it: a kernel that walks every frame's codewords and
 * adds up their values but stores no sample (csrc/x3_seg_index_kernel.h) -- a frame per lane, one
 * 8-byte entry per seg_blocks blocks.  For ANY x3_params that x3_decode_windows_dev accepts: block lengths other than 20,
 * any blocks_per_frame, any code set and thresholds, frames shorter than the parameters' frame (entries at or behind a
 * frame's last block stay invalid), frames anywhere in d_x3.  d_frame_offsets: n_frames byte offsets into d_x3, as the
 * device decode calls take.  d_seg_index: x3_seg_index_entries() words, 8-byte aligned; EVERY word is written (the header
 * word, invalid entries as zero), so the buffer need not be cleared.  seg_blocks as x3_decode_dev_seg accepts it (a
 * multiple of 4, <= 3 200); where it leaves a frame one stretch (x3_seg_index_entries() == 0) nothing is written.
 *   Asynchronous on the context's stream: one launch, no host trip, no workspace, nothing allocated; the pending state of
 * x3_decode_dev and of the window calls is left alone.  Offsets, headers and bytes are untrusted: nothing outside
 * [d_x3, d_x3 + x3_len) (and the 16-byte chunks that hold its bytes) is read, nothing outside d_seg_index's words is
 * written.  A frame that is irregular in a way the fast decoders flag (decode error, BFP width <= 5, a zero run of 32 bits
 * or more, a block that ends behind the payload) has no valid entry from that point on and is counted in the read-only
 * option "last_seg_index_irregular"; it gets no status here -- the consumers' check and fix-up passes give it one.  CRCs
 * are not verified.  X3_ERR_BAD_ARG (nothing enqueued) for a NULL or misaligned pointer, n_frames == 0 or above
 * 0x7FFFFFFF, a seg_blocks that x3_decode_dev_seg refuses and parameters that x3_decode_windows_dev refuses.
 *   The walk-built index is for the WINDOW paths (x3_decode_windows_dev, x3_corpus_windows_dev), which decode any block
 * length by it.  Out of scope: x3_decode_dev_seg still decodes frame by frame off block length 20 and the default codes
 * whatever index it is given (the block-per-lane decoder has no stretch mode), and x3_encode_dev_seg still fills none
 * there. */
int x3_seg_index_build_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                           uint64_t n_frames, const x3_params* p, uint64_t* d_seg_index, uint32_t seg_blocks);
/* ---- Placement (round 6).  Where the x3 stream and where the decoded samples lie in HBM decides the decode phase's pace by
 * up to 10 % -- per PAIR of buffers, reproducibly within a process, and by nothing their addresses show
 * (profiles/r6/decoder_modes.txt).  A pipeline that keeps its buffers allocates a few candidates once and keeps the pair that
 * runs best; this is the measuring loop: for every pair (d_streams[i], d_backs[j]) `warm` untimed and `steps` timed round
 * trips -- x3_encode_dev of the n samples at d_wav into d_streams[i] (capacity cap each; d_frame_offsets: x3_num_frames + 1
 * words), x3_decode_dev of that stream into d_backs[j] (n samples each) -- and ms_per_step[i * n_backs + j] = host wall time
 * per round trip, synchronised.  The samples at d_wav should be of the kind the pipeline will see (the pace follows the
 * stream's density).  X3_ERR_* if a round trip fails or its stream does not decode; the caller frees what it does not keep.
 * (No counterpart in the reference: a property of the device.) */
int x3_place_buffers(x3_ctx* ctx, const int16_t* d_wav, uint64_t n, const x3_params* p, uint8_t* const* d_streams,
                     uint32_t n_streams, uint64_t cap, uint64_t* d_frame_offsets, int16_t* const* d_backs, uint32_t n_backs,
                     uint32_t warm, uint32_t steps, double* ms_per_step);
/* ---- HIP graphs: a launch-bound sequence of device calls, recorded once and replayed with one host call.
 * A short stream's encode + decode is a dozen launches, memsets and event operations of a few microseconds each around
 * kernels of 40-60 us: the host's share of such a step is a third.  Between x3_graph_begin and x3_graph_end the ASYNCHRONOUS
 * device calls of this context -- x3_encode_dev[_seg], x3_encode_frames_dev, x3_decode_dev[_seg] -- are recorded (stream
 * capture on the context's stream; the check pass's side stream joins through its events) instead of launched; nothing
 * may allocate meanwhile, so the same calls must have been made once before, and no call that waits for the GPU
 * (x3_*_result, x3_ctx_sync, the host-buffer entry points) may be made inside.  x3_graph_launch enqueues the whole
 * sequence on the context's stream; x3_encode_result / x3_decode_result then report on the calls in it as if they had just
 * been made.  The graph holds the pointers and sizes the calls were recorded with: replaying it means the same buffers
 * with new contents.  (The decoder's paced priorities follow launch history through a per-launch tag; replays carry
 * one tag and run as a context's first launch does: a graph is for launches too short to be paced.)
 *   MEASURED (round 5, ROCm 7.0.2, profiles/r5/hip_graph_replay.txt): on this stack a replay is SLOWER than the same calls
 * issued back to back on the stream -- config 2's encode + decode by stretches 0.134 against 0.128 ms a step, a 500-frame
 * stream 0.33 against 0.095 -- the runtime executes a captured graph node by node with a barrier behind each.  The entry
 * points are kept (bit-exact, tested) for stacks where that changes; nothing in the library or bench.py uses them.
 *   EXPERIMENTAL: not part of the drop-in surface (the reference has nothing like it), and may go.
 *   A call that fails inside a recording (X3_ERR_BAD_ARG from a buffer that would have to grow, a HIP error) leaves the
 * capture open: end it with x3_graph_end -- it reports the failure or hands back a graph to destroy -- before the context
 * is used again.  x3_graph_begin changes nothing of the context unless the capture has begun. */
typedef struct x3_graph x3_graph;
int x3_graph_begin(x3_ctx* ctx);
int x3_graph_end(x3_ctx* ctx, x3_graph** graph);
int x3_graph_launch(x3_ctx* ctx, x3_graph* graph);
void x3_graph_destroy(x3_graph* graph);
/* Waits for the last x3_decode_dev: index and status of the first frame whose status != 0
 * (first_bad = n_frames, status 0 if all frames are good) and the total samples of good frames
 * before it. */
int x3_decode_result(x3_ctx* ctx, uint64_t* first_bad, int* first_bad_status, uint64_t* samples_before);

/* GPU-side frame walk of a device-resident stream whose frame offsets are not known (SURVEY 8f.2;
 * X3aReader::decode_next_frame, src/decodefile.rs:105-121 + decoder::read_frame_header, src/decoder.rs:69-118):
 * every byte offset is tested for a valid frame header in parallel, the chain off -> off + 20 + payload_len is
 * resolved by pointer doubling.  d_frame_offsets[0..*n_frames) receives the byte offsets of the frames the walk
 * pushes, d_wav_offsets their exclusive sample offsets (both need room for max_frames entries); *terminal is
 * how the walk ends behind them: X3_OK (data exhausted / payload runs past the end), a header error, or
 * X3_ERR_FRAME_HEADER_INVALID_PAYLOAD_LEN.  Synchronous. */
int x3_index_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t len, uint64_t max_frames, uint64_t* d_frame_offsets,
                 uint64_t* d_wav_offsets, uint64_t* n_frames, uint64_t* n_samples, int* terminal);
/* x3_decode_stream for device buffers: index (above) + decode, nothing crosses PCIe but the summary.  Same
 * results and status as x3_decode_stream on the same bytes; samples go to d_wav[0..*n_out).  A stream that is one clean
 * chain of frames (what an encoder writes) takes ONE trip to the host: the decode launches are enqueued behind the walk's
 * and read the frame count from device memory (option "two_trips" = 1: wait for the walk first, as before round 5; a
 * stream the walk objects to, or one with more than a frame per KiB, is done that way by itself). */
int x3_decode_stream_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t len, const x3_params* p, int16_t* d_wav,
                         uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok, uint64_t* frame_errors);

/* ---- RANDOM ACCESS (no counterpart in the reference: decodefile.rs reads frame after frame).  A WINDOW is (start, L): the
 * samples at positions [start, start + L) of a mono stream, where the position of sample i of frame f is
 * sample_offsets[f] + i -- frames' samples back to back, what x3_decode_stream returns for a clean stream.  The work of a
 * call follows its windows, not the stream: per window the frames that cover it, each checked (header, payload CRC, and its
 * header's sample count against sample_offsets[f + 1] - sample_offsets[f]: a mismatch means the offsets are not this
 * stream's, X3_ERR_BAD_ARG, as is a frame whose offset or payload lies past x3_len) and decoded by the stretches of the
 * segment index (x3_decode_dev_seg) -- every stretch of a covering frame, those in front of the window being the proof
 * chain of those inside it.  The index is a hint as there:
 * without it (NULL, or a header word that says "none") frames decode whole, one lane each, with the same results.
 * Window status (d_status, one int32 per window): 0 when every covering frame checks and decodes; otherwise the status
 * x3_decode_dev gives the FIRST covering frame that fails -- the window's samples in front of that frame are exact, the
 * rest are 0.  A window off the end (start + L > total, any wild start) is X3_ERR_BAD_ARG and zeros; the call itself does
 * not fail.  Offsets, starts and index are untrusted: a wild value is a frame error or a slower path, never a read outside
 * [d_x3, d_x3 + x3_len) or a write outside d_out.  Multi-channel frames fail as in x3_decode_dev.  DESIGN.md section 10. */
/* Fill sample_offsets[0..n_frames] (n_frames + 1 words: exclusive prefix of the frame headers' sample counts, last = total)
 * for frames whose byte offsets are known (the encoder's d_frame_offsets, or x3_index_dev's); a header that does not lie
 * inside the stream counts 0.  Asynchronous. */
int x3_sample_offsets_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                          uint64_t n_frames, uint64_t* d_sample_offsets);
/* n_windows windows of window_len samples each, window w = positions [d_starts[w], d_starts[w] + window_len), written
 * row-major to d_out (n_windows x window_len; out_format X3_WINDOW_I16 / X3_WINDOW_F32, d_out aligned to the sample size);
 * d_status: n_windows int32.  d_seg_index / seg_blocks as for x3_decode_dev_seg (NULL / 0: none).  Asynchronous on the
 * context's stream, one launch set and no host round trip; the pending state of an earlier x3_decode_dev is left as it
 * is.  X3_ERR_BAD_ARG (nothing enqueued) for window_len == 0, n_windows == 0, an unknown format, a misaligned pointer,
 * and seg_blocks as x3_decode_dev_seg refuses it. */
int x3_decode_windows_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                          const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                          const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                          uint64_t n_windows, uint32_t window_len, void* d_out, int out_format, int32_t* d_status);
/* Waits for the last x3_decode_windows_dev: windows with status != 0, the first of them (n_windows if none) and its status. */
int x3_decode_windows_result(x3_ctx* ctx, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status);
/* RANGES: windows with a length each.  Range w = positions [d_starts[w], d_starts[w] + d_lens[w]) (device arrays: uint64 /
 * uint32; positions as above).  Row and status of range w are exactly what x3_decode_windows_dev gives the single window
 * (d_starts[w], window_len = d_lens[w]) of the same stream: the exact prefix in front of the first covering frame that
 * fails, zeros behind it and that frame's status; a range off the end (start + len > total, any wild start) is
 * X3_ERR_BAD_ARG and zeros.  d_lens[w] == 0 is legal: status 0 when start <= total, X3_ERR_BAD_ARG otherwise, no frame is
 * covered, nothing of the row is written (start + len - 1 is never formed for it).
 *   PACKED (row_stride == 0): row w begins at off[w], the exclusive sum of ALL lengths -- those of bad ranges too, so the
 * layout depends on the lengths alone.  d_out_offsets (required) receives off[0 .. n_ranges], the last being the total.  A
 * range with off[w] + d_lens[w] > out_cap is X3_ERR_BAD_ARG and none of its samples is written; ranges that fit are
 * complete, and x3_decode_ranges_result reports the total, so a caller can grow d_out and repeat the call.
 *   PADDED (row_stride > 0): row w begins at w * row_stride and [d_lens[w], row_stride) of EVERY row is written as zero.
 * A range with d_lens[w] > row_stride is X3_ERR_BAD_ARG and a row of zeros.  n_ranges * row_stride > out_cap fails the
 * call.  d_out_offsets may be NULL; when given it receives w * row_stride (n_ranges + 1 words).
 *   out_cap counts samples of out_format.  Starts and lengths are untrusted like everything the window calls take: nothing
 * outside d_out[0 .. out_cap), d_status[0 .. n_ranges) and d_out_offsets[0 .. n_ranges] is written, nothing outside
 * [d_x3, d_x3 + x3_len) is read; the sums of the lengths are 64-bit and cannot wrap (n_ranges <= 0x7FFFFFFF, 32-bit lengths).
 *   Asynchronous on the context's stream: one launch set, no host trip, nothing allocated after the first call of a size.
 * The call shares the window calls' workspace and pending slot: a ranges call REPLACES the state of a pending
 * x3_decode_windows_dev / x3_corpus_windows_dev and the other way round (the kernels are ordered on the stream; only the
 * summary of the earlier call is lost).  x3_decode_ranges_result belongs to the last ranges call, x3_decode_windows_result to
 * the last windows call; each is X3_ERR_BAD_ARG when the pending call is of the other kind.  The pending states of
 * x3_decode_dev and of the levels calls are left alone.  X3_ERR_BAD_ARG with nothing enqueued for n_ranges == 0 or above
 * 0x7FFFFFFF, a NULL or misaligned pointer (d_out_offsets: NULL only when padded), an unknown format, a seg_blocks that
 * x3_decode_dev_seg refuses, parameters that x3_decode_windows_dev refuses, and a context that is recording a graph.
 * DESIGN.md section 16. */
int x3_decode_ranges_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                         const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                         const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                         const uint32_t* d_lens, uint64_t n_ranges, uint64_t row_stride, void* d_out, uint64_t out_cap,
                         int out_format, uint64_t* d_out_offsets, int32_t* d_status);
/* Waits for the last x3_decode_ranges_dev / x3_corpus_ranges_dev: ranges with status != 0, the first of them (n_ranges if
 * none), its status, and the sum of all lengths (what a packed d_out must hold for no range to be refused). */
int x3_decode_ranges_result(x3_ctx* ctx, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status,
                            uint64_t* total_samples);
/* out_format of x3_decode_windows_dev */
#define X3_WINDOW_I16 0     /* int16 samples */
#define X3_WINDOW_F32 1     /* float32 samples, s / 32768.0f (exact) */

/* ---- LEVELS (no counterpart in the reference): min, max, count, sum and sum of squares of the samples per BIN of sample
 * positions, computed from the stream in device memory without a sample buffer -- overviews, peak / RMS per clip, "where is
 * anything loud".  All five are integers: the records are exact and do not depend on any order of execution.
 *   Positions are the window calls': sample i of frame f is at d_sample_offsets[f] + i.  Bin b covers positions
 * [b * bin_len, (b + 1) * bin_len); bin_len == 0 means one bin for everything.
 *   A frame's STATUS (d_frame_status[f], when given) is the status x3_decode_windows_dev gives a window that is exactly that
 * frame: its header check, its payload CRC, its header's sample count against the offsets (a mismatch, or an offset or
 * payload past x3_len: X3_ERR_BAD_ARG), then decoder::decode_frame.  A frame with status 0 adds EVERY one of its samples to
 * the bins they fall in; a frame with any other status adds NOTHING, also when its first blocks decode cleanly.  Positions
 * at or beyond n_bins * bin_len are not counted.  EVERY one of the n_bins records is written (the caller need not clear
 * them; a bin that no sample falls in holds the identities); nothing outside d_levels[0 .. n_bins) and
 * d_frame_status[0 .. n_frames) is written, nothing outside [d_x3, d_x3 + x3_len) is read: offsets, sample offsets, index
 * and bytes are untrusted exactly as in x3_decode_windows_dev.  The segment index is a hint that changes time, never
 * results; without one (NULL, or a header word that says "none") a frame is one stretch.  n counts modulo 2^32.
 *   How: the window path's check and stretches, with a consumer that keeps a bin in registers.
 * Stretches add to rows of the frame's own in a workspace of (n_bins + n_frames) records; only a frame whose every stretch
 * has been proven is added to d_levels, a flagged one goes through the reference's reader first.
 *   Asynchronous on the context's stream: one launch set, no host trip, nothing allocated after the first call of a size
 * (the workspace grows like the windows').  The pending states of x3_decode_dev and of the window calls are left alone.
 * X3_ERR_BAD_ARG with nothing enqueued for n_bins == 0 or above 0x7FFFFFFF, n_frames == 0 or above 0x7FFFFFFF, NULL or
 * misaligned pointers (d_levels: 8 bytes; d_frame_status may be NULL), a seg_blocks that x3_decode_dev_seg refuses,
 * parameters that x3_decode_windows_dev refuses, and a context that is recording a graph. */
typedef struct x3_level {      /* 32 bytes, 8-byte aligned */
  uint64_t sum_sq;             /* sum of s*s */
  int64_t  sum;                /* sum of s   */
  int32_t  min, max;           /* n == 0: 32767 / -32768 (the identities) */
  uint32_t n;                  /* samples counted into this bin */
  uint32_t reserved;           /* 0 */
} x3_level;
int x3_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                  const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                  const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len,
                  x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status);
/* Waits for the last x3_levels_dev / x3_corpus_levels_dev: frames with status != 0, the first of them (the frame count if
 * none) and its status. */
int x3_levels_result(x3_ctx* ctx, uint64_t* n_bad_frames, uint64_t* first_bad, int* first_bad_status);

/* ---- BATCHES OF STREAMS (no counterpart in the reference: decodefile.rs reads one file).  Entry s of a call is the bytes
 * [offsets[s], offsets[s] + lengths[s]) of d_x3 -- any byte offset; entries may overlap or repeat, and a batch that
 * x3_encode_frames_dev wrote back to back is taken as it is.  All entries share one x3_params.  Each entry's results are
 * exactly those of ONE call on that entry alone, with wav_cap = row_len:
 *   flags 0:                         x3_decode_stream_dev(entry, p, row_len)
 *   X3_STREAMS_ARCHIVE_FRAMES:       the frame walk of x3_x3a_decode on the archive whose frame part the entry is (the
 *                                    reader believes in 8 bytes more than there are: decodefile.rs:62-66)
 * -- status, n_out, frames_ok and frame_errors for every kind of damage, multi-channel frames included.  Row s of d_out
 * (n_streams x row_len samples, out_format X3_WINDOW_I16 / X3_WINDOW_F32) holds that call's samples in [0, n_out) and
 * zeros in [n_out, row_len); d_results[s] its x3_stream_result.  Nothing outside d_out's n_streams x row_len samples or
 * d_results is written, nothing outside the entries (and the dwords that hold their bytes) is read.
 *   How: every entry's frames are found on the GPU in one launch set, all entries at once (a segmented form of the frame
 * walk's fast path: DESIGN.md section 12), then decoded by x3_decode_dev's kernels with the frame count read from device
 * memory -- no host trip.  Where the decoder the parameters route to cannot take its count from there (single-wave
 * decoders: codes other than the defaults, row_len not a multiple of 4), the call waits once for the count.  An entry the
 * fast walk cannot vouch for (not one clean chain of frames from its first byte: junk, damage, a truncated last frame, a
 * frame that does not fit its row) is walked again by x3_decode_stream_dev's own path inside x3_decode_streams_result and
 * decoded into its row there; read-only options "streams_general_walks" / "last_streams_general_walks" count such entries.
 *   Asynchronous on the context's stream; d_out and d_results are final once x3_decode_streams_result has returned (d_x3
 * must stay untouched until then).  Replaces the pending state of an earlier x3_decode_dev, as x3_decode_stream_dev does.
 * offsets / lengths are HOST arrays, checked and copied here (through the context's one pinned block: a call waits on the
 * host for the table copy of the previous x3_decode_streams_dev / x3_encode_frames_dev, as described there).
 * X3_ERR_BAD_ARG with nothing enqueued for n_streams == 0, row_len == 0, an unknown out_format or flag, d_x3 not on a
 * 4-byte boundary, d_out not on its sample size's boundary, d_results not on an 8-byte one, an entry outside [0, x3_len),
 * and parameters x3_params_validate refuses. */
#define X3_STREAMS_ARCHIVE_FRAMES 1u   /* entries are the frame part of .x3a archives: walked as X3aReader walks them */
#define X3_CORPUS_INDEX_WALK 0x100u    /* x3_corpus_build only (below): the segment index by x3_seg_index_build_dev */
typedef struct x3_stream_result {
  uint64_t n_out;        /* samples of the entry (x3_decode_stream_dev's *n_out) */
  uint64_t frames_ok;    /* its *frames_ok */
  int32_t status;        /* its return value */
  uint32_t frame_errors; /* its *frame_errors */
} x3_stream_result;
int x3_decode_streams_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* offsets,
                          const uint64_t* lengths, uint64_t n_streams, uint32_t flags, const x3_params* p, void* d_out,
                          uint64_t row_len, int out_format, x3_stream_result* d_results);
/* Waits for the last x3_decode_streams_dev, walks the entries the fast walk left alone: entries with status != 0, the
 * first of them (n_streams if none) and its status. */
int x3_decode_streams_result(x3_ctx* ctx, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status);

/* ---- CORPUS: windows of many streams (no counterpart in the reference).  An index built once over the entries of one
 * device buffer (as in x3_decode_streams_dev: any byte offset, overlaps and repeats, one x3_params), after which a window is
 * addressed as (entry, start).  Take entry e alone, its bytes in a buffer of their own: its frames are those x3_index_dev
 * finds (X3_STREAMS_ARCHIVE_FRAMES: those of x3_x3a_decode's walk, which believes in 8 bytes more), its sample offsets
 * those of x3_sample_offsets_dev.  Window (e, s) of x3_corpus_windows_dev is then exactly what x3_decode_windows_dev with
 * start s returns on that entry: the same row, the same status, zeros behind the first failing covering frame.  The
 * segment index is a hint: it changes time, never results.  One exception, for bytes changed after
 * the build: a frame is bounded by d_x3's x3_len, not by its entry's end, so a header rewritten with a valid header CRC
 * and a payload that now runs past its entry gives the status of that payload's check where the entry alone gives
 * X3_ERR_BAD_ARG (every read still stays inside [d_x3, d_x3 + x3_len)). */
typedef struct x3_corpus x3_corpus;
typedef struct x3_corpus_entry {
  uint64_t n_samples;    /* positions of the entry: x3_sample_offsets_dev's total over its frames */
  uint64_t first_frame;  /* its frames are [first_frame, first_frame + n_frames) of the corpus's frame table */
  uint64_t n_frames;
  int32_t walk_status;   /* how its walk ended behind those frames (x3_index_dev's *terminal) */
  uint32_t general_walk; /* 1: the fast walk could not vouch for it; the general walk found its frames */
} x3_corpus_entry;
/* Synchronous.  offsets / lengths: HOST arrays into d_x3.  flags: 0, X3_STREAMS_ARCHIVE_FRAMES, X3_CORPUS_INDEX_WALK or
 * both.  seg_blocks: 0 = no segment index, else as x3_decode_dev_seg accepts it.  Without X3_CORPUS_INDEX_WALK it is
 * recorded by one decode of the corpus where the parameters route to a decoder that records (block length 20, the default
 * codes), and kept nowhere else (seg_blocks_in_use 0).  With the flag it is built by ONE x3_seg_index_build_dev over the
 * corpus's frame table, for every parameter set (seg_blocks_in_use = seg_blocks unless frames are one stretch; no scratch
 * rows, "last_corpus_record_slices" 0).
 * d_x3 is referenced, not copied: it must outlive the corpus.  The build ends the pending state of an earlier
 * x3_decode_dev, as x3_decode_stream_dev does.  X3_ERR_BAD_ARG, with nothing left allocated, for n_entries == 0 or above
 * 0xFFFFFFF0, an entry outside [0, x3_len), an unknown flag, d_x3 not on a 4-byte boundary, parameters that
 * x3_params_validate or x3_decode_windows_dev refuses, a seg_blocks that x3_decode_dev_seg refuses, and more than
 * 0x7FFFFFFF frames in all. */
int x3_corpus_build(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* offsets, const uint64_t* lengths,
                    uint64_t n_entries, uint32_t flags, const x3_params* p, uint32_t seg_blocks, x3_corpus** corpus);
int x3_corpus_info(const x3_corpus* corpus, uint64_t* n_entries, uint64_t* n_frames, uint64_t* total_samples,
                   uint32_t* seg_blocks_in_use);
/* the entry table (host array of n_entries) */
int x3_corpus_entries(const x3_corpus* corpus, x3_corpus_entry* out);
/* The device copy of the entry table the corpus calls read (device memory the corpus owns, n_entries records).  Nothing
 * trusts it: written to after the build it can move or empty entries, give statuses or slower paths, never an access outside
 * the caller's buffers -- which is what a test of that claim needs the pointer for.  The pointer is const because no caller
 * has a reason to write there; one who casts it away and writes gets exactly that outcome, by design, for every corpus call
 * enqueued afterwards, until the corpus is freed (the host copy x3_corpus_entries returns is not changed by it). */
int x3_corpus_entries_dev(const x3_corpus* corpus, const x3_corpus_entry** d_entries);
/* The segment index the build recorded (device memory the corpus owns; layout as x3_decode_dev_seg's, over the corpus's frame
 * table): *d_seg_index and *n_words, or NULL and 0 without one. */
int x3_corpus_seg_index(const x3_corpus* corpus, const uint64_t** d_seg_index, uint64_t* n_words);
/* Window w = samples [d_starts[w], d_starts[w] + window_len) of entry d_entries[w] (device arrays: uint32 / uint64).  Rows,
 * formats, d_status and x3_decode_windows_result as for x3_decode_windows_dev; a window whose entry is not in the corpus,
 * or that runs past its entry's n_samples (it never runs into the next entry), is X3_ERR_BAD_ARG and zeros.  Asynchronous,
 * one launch set, no host trip; leaves a pending x3_decode_dev alone.  Nothing is trusted -- tables, entries, starts, bytes
 * changed after the build: they can give a status or a slower path, never a read outside [d_x3, d_x3 + x3_len) or a
 * write outside d_out / d_status.  X3_ERR_BAD_ARG with nothing enqueued for the arguments x3_decode_windows_dev refuses,
 * d_entries not on a 4-byte boundary, and a context on another device than the build's. */
int x3_corpus_windows_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                          uint64_t n_windows, uint32_t window_len, void* d_out, int out_format, int32_t* d_status);
/* Range w = samples [d_starts[w], d_starts[w] + d_lens[w]) of entry d_entries[w].  Layout (packed / padded), out_cap,
 * d_out_offsets, zero lengths, refusals and x3_decode_ranges_result as for x3_decode_ranges_dev; entries and the end of an
 * entry as for x3_corpus_windows_dev (a range never runs into the next entry; with d_lens[w] == 0 the status is 0 when the
 * entry is in the corpus and start <= its n_samples).  Each result equals x3_decode_ranges_dev on that entry alone. */
int x3_corpus_ranges_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                         const uint32_t* d_lens, uint64_t n_ranges, uint64_t row_stride, void* d_out, uint64_t out_cap,
                         int out_format, uint64_t* d_out_offsets, int32_t* d_status);
/* LEVELS of every entry of a corpus.  Entry e has max(1, ceil(n_samples[e] / bin_len)) rows (one with bin_len == 0), the
 * rows lie entry after entry; x3_corpus_levels_rows writes that prefix (HOST array of n_entries + 1 words, from the entry
 * table).  Positions are relative to the entry, and entry e's rows are exactly what x3_levels_dev gives on that entry alone
 * with its own frame table, n_bins = its rows.  d_frame_status: one int32 per frame of the corpus's frame table, or NULL.
 * The corpus's own segment index is used when it has one.  Contract and refusals as for x3_levels_dev (n_rows for n_bins);
 * also X3_ERR_BAD_ARG with nothing enqueued when n_rows is not the prefix's last word, and for a context on another device
 * than the build's.  x3_levels_result as there. */
int x3_corpus_levels_rows(const x3_corpus* corpus, uint64_t bin_len, uint64_t* row_first);
int x3_corpus_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                         int32_t* d_frame_status);
/* ---- SIGNAL LEVELS (no counterpart in the reference): the levels of the samples' FIRST DIFFERENCE -- a one-tap high-pass
 * in front of the detection chain at no extra read.  `signal` selects what is binned; any other
 * value is X3_ERR_BAD_ARG with nothing enqueued.
 *   X3_LEVEL_SIGNAL_SAMPLES: the records of x3_levels_dev / x3_corpus_levels_dev on the same arguments, field for field.
 *   X3_LEVEL_SIGNAL_DIFF: positions, bins, n_bins * bin_len, frame statuses and "every record is written" are exactly
 * x3_levels_dev's.  What the position of sample i of frame f adds:
 *     i >= 1: y = clamp(x_f[i] - x_f[i-1], -32768, 32767), counted iff frame f has status 0;
 *     i == 0: y = clamp(x_f[0] - x_{f-1}[last], -32768, 32767), counted iff f >= 1, frames f - 1 and f BOTH have status 0
 *             and, in the corpus form, both belong to the same entry.  (A checked frame's sample count equals
 *             d_sample_offsets[f + 1] - d_sample_offsets[f], so two good neighbours in the table are always adjacent in
 *             position: the two samples are neighbours of the signal.)
 * Otherwise the position adds nothing and n is not incremented: the first sample of a stream or entry has no difference,
 * and a failed frame takes both of its seams with it, the one in front of it and the one behind it.  n counts differences: a
 * clean stream or entry of N samples has records whose n sum to N - 1.  Empty bins hold the identities.
 *   y is an int16 signal like any other: the records obey what x3_events_dev, x3_level_quantiles_dev,
 * x3_level_thresholds_dev and x3_events_adaptive_dev rely on (|y| <= 32768, sum_sq / n <= 1 << 30) and go into them unchanged.
 *   Argument checks, the asynchronous contract, x3_levels_result and the option "last_levels_replays" are those of
 * x3_levels_dev / x3_corpus_levels_dev.  The segment index stays a hint: the sample in front of a stretch comes from the
 * index entry, and an entry with a wrong sample is contradicted by the stretch that ends there, as a wrong bit position is. */
int x3_signal_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                         const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                         const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len,
                         x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, int signal);
int x3_corpus_signal_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                                int32_t* d_frame_status, int signal);
#define X3_LEVEL_SIGNAL_SAMPLES 0   /* the signals of x3_signal_levels_dev */
#define X3_LEVEL_SIGNAL_DIFF 1
/* ---- FIR LEVELS (no counterpart in the reference): the levels of an INTEGER FIR-FILTERED signal -- a band picked in front
 * of the detection chain at no extra read and no sample buffer.  `fir` is a host struct, read at
 * the call.  For a position i of a stream or corpus entry:
 *     acc  = sum over t < T of c[t] * x[i - t], in int32;
 *     y[i] = clamp(acc >> shift, -32768, 32767), where >> is arithmetic (floor).
 *   The call is X3_ERR_BAD_ARG with nothing enqueued unless 1 <= T <= 8, shift <= 15 and sum |c[t]| <= 32768.  That bound
 * on the taps gives |acc| <= 32768 * 32768 = 2^30: 32-bit arithmetic is exact.  A NULL fir is refused first, the way an
 * unknown signal is; everything else is refused as in x3_levels_dev / x3_corpus_levels_dev.
 *   Positions, bins, n_bins * bin_len, frame statuses, "every record is written", x3_levels_result, the pending slot and
 * the option "last_levels_replays" are those of the levels calls.
 *   THE HISTORY RULE.  Position i adds y[i] to its bin if and only if all T positions i - T + 1 .. i exist in the same
 * stream or entry (i >= T - 1) and every one of them lies in a frame with status 0.  Otherwise the position adds nothing
 * and n is not incremented: a failed frame takes its own positions and the T - 1 positions behind it, and a clean stream
 * or entry of N samples has records whose n sum to max(0, N - T + 1).  No history crosses from one entry into the next.
 *   Two identities follow: {T = 1, c = {1}, shift = 0} gives the records of X3_LEVEL_SIGNAL_SAMPLES, and
 * {T = 2, c = {1, -1}, shift = 0} those of X3_LEVEL_SIGNAL_DIFF, field for field.
 *   y is an int16 signal like any other: the records go into the events, quantiles, thresholds and ranges calls unchanged.
 * The segment index stays a hint and nothing new rests on it: a stretch forms only the outputs whose whole history it
 * decoded itself, and the positions at a stretch's front are formed behind it from the stretches' first and last samples.
 * That takes a workspace of 32 bytes per (frame, stretch), allocated at the first FIR call of a size and kept. */
typedef struct x3_level_fir {
  uint32_t n_taps;      /* T: 1 .. 8 */
  uint32_t shift;       /* 0 .. 15 */
  int16_t  taps[8];     /* c[0 .. T-1]; entries at and behind T are ignored */
} x3_level_fir;
int x3_fir_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                      const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                      const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len,
                      x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, const x3_level_fir* fir);
int x3_corpus_fir_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows,
                             int32_t* d_frame_status, const x3_level_fir* fir);
/* ---- TONE LEVELS (no counterpart in the reference): per bin, the QUADRATURE SUMS of the samples against one oscillator --
 * the one-bin DFT (Goertzel) detector of a narrow band, which no filter of eight taps can pick, at no extra read and no
 * sample buffer.  `tone` is a host struct, copied at the call; d_table is a caller-owned DEVICE array
 * of 1 024 (cos, sin) int16 pairs (2 048 int16, 4 096 bytes, 4-byte aligned), read when the kernels run like every other
 * device input.  Any contents are legal: the call defines nothing by floating point.  The usual table, which the mirrors
 * supply, is (round(32767 * cos(2 pi k / 1024)), round(32767 * sin(2 pi k / 1024))) at pair k.
 *   Position i of a stream or of a corpus entry has the phase ph(i) = (i * step) mod 2^32 -- every entry starts at phase 0 --
 * and the table pair k(i) = ph(i) >> 22; step = round(f / fs * 2^32) puts the oscillator at frequency f.  The record of a bin
 * is x3_tone_level, which has x3_level's layout slot for slot:
 *     re = sum of x[i] * cos[k(i)],  im = sum of x[i] * sin[k(i)]   over the bin's positions in frames with status 0;
 *     min, max, n: field for field those of the bin's x3_levels_dev record.
 * An empty bin is {0, 0, 32767, -32768, 0, 0}.  |x * w| <= 2^30 and n < 2^32: the int64 sums are exact, in any order.
 *   Positions, bins, bin_len 0 (one bin), n_bins * bin_len, "every record is written", a failed frame adding nothing,
 * d_frame_status, x3_levels_result, the pending slot, the option "last_levels_replays", the segment index as a hint only and
 * the asynchronous contract are those of x3_levels_dev / x3_corpus_levels_dev.  A NULL tone, a NULL or misaligned d_table or
 * reserved != 0 is X3_ERR_BAD_ARG with nothing enqueued, checked before every other argument.
 *   Two identities: a table of all (1, 0) gives re == the sum of x3_levels_dev's record and im == 0, with its min, max and
 * n; step 0 with the usual table gives re == 32767 * that sum and im == 0. */
typedef struct x3_level_tone {
  uint32_t step;            /* phase per position, in units of 2^-32 turns */
  uint32_t reserved;        /* 0 */
  const int16_t* d_table;   /* device: 1 024 pairs (cos, sin) */
} x3_level_tone;
typedef struct x3_tone_level {  /* 32 bytes, 8-byte aligned: x3_level with re for sum_sq and im for sum */
  int64_t  re;                 /* sum of x * cos[k] */
  int64_t  im;                 /* sum of x * sin[k] */
  int32_t  min, max;           /* of the samples; n == 0: 32767 / -32768 */
  uint32_t n;                  /* samples counted into this bin */
  uint32_t reserved;           /* 0 */
} x3_tone_level;
int x3_tone_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                       const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                       const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len,
                       x3_tone_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, const x3_level_tone* tone);
int x3_corpus_tone_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_rows,
                              int32_t* d_frame_status, const x3_level_tone* tone);
/* THE ADAPTER into the detection chain: n_rows tone records -> the x3_level records of the BAND'S LEVEL, which the events,
 * quantiles and thresholds calls take unchanged.  One elementwise kernel on the context's stream, asynchronous, with no
 * result call and no pending state.  d_levels == d_tone (in place) is allowed; any other overlap, a NULL or misaligned
 * (8 bytes) pointer, n_rows == 0 or n_rows > 2^31 - 1 is X3_ERR_BAD_ARG.  Per record, in integers (>> is arithmetic, isqrt
 * the floor square root), n == 0 giving {0, 0, 32767, -32768, 0, 0}:
 *     e = max(0, bitlen(n) - 15);  a = re >> (15 + e);  b = im >> (15 + e);  P = a * a + b * b  (below 2^62);
 *     m = n >> e;  ms = min(2^30, floor(floor(2 * P / m) / m));  peak = min(32767, isqrt(2 * ms));
 *     -> {sum_sq = ms * n, sum = 0, min = -peak, max = peak, n = n, reserved = 0}.
 * For a tone of amplitude A at the oscillator's frequency ms is about A * A / 2, the tone's mean square, and peak about A.
 * At DC (step 0) and at Nyquist (step 2^31) the two quadrature sums do not halve the power between them: the estimate is
 * TWICE the component's mean square there.  |min|, |max| <= 32768 and sum_sq / n <= 2^30 hold as for any x3_level record;
 * merged event records then carry the event's mean band level.  The records of x3_tone_range_levels_dev /
 * x3_corpus_tone_range_levels_dev, packed or padded, go through this call unchanged: n_rows of them, whatever range they
 * belong to; a padded layout's rows behind a range's last are empty records (n == 0) and come out as the identity. */
int x3_tone_power_levels_dev(x3_ctx* ctx, const x3_tone_level* d_tone, uint64_t n_rows, x3_level* d_levels);
/* ---- TONE BANK LEVELS: up to X3_TONE_BANK_MAX oscillators against ONE table in ONE pass over the stream -- a band spectrum
 * per bin (third-octave levels, a pinger at one of several frequencies) for one decode instead of one per band (DESIGN.md
 * section 26).  `bank` is a host struct, copied at the call; d_table is x3_level_tone's, read when the kernels run.
 *   ONE RULE: the bank is n_tones tone calls laid PLANE BY PLANE.  d_levels holds n_tones * n_bins records (n_tones * n_rows
 * for a corpus); plane t is the n_bins records at d_levels + t * n_bins, byte for byte what x3_tone_levels_dev /
 * x3_corpus_tone_levels_dev writes for {steps[t], 0, d_table} with the same other arguments: re, im, the samples' min, max
 * and n, reserved 0.  In a corpus every entry starts at phase 0 in every plane, and the rows of an entry are those of the
 * single call (x3_corpus_levels_rows) in every plane.  So every plane goes as it lies into x3_events_dev, the quantile and
 * threshold calls and their corpus forms, and ALL planes go through x3_tone_power_levels_dev in one launch of
 * n_tones * n_bins rows.  Equal steps in two slots are legal and give equal planes.  n_tones == 1 IS the single call.
 *   d_frame_status, x3_levels_result, the pending slot, "last_levels_replays", "every record is written", a failed frame
 * adding nothing (to no plane), the segment index as a hint only and the asynchronous contract are the single call's; the
 * statuses never depend on the bank.  X3_ERR_BAD_ARG with nothing enqueued, checked before every other argument: a NULL
 * bank, n_tones 0 or above X3_TONE_BANK_MAX, reserved != 0, a NULL or misaligned (4 bytes) d_table.  Also refused:
 * n_tones * n_bins > 2^31 - 1, and everything the single call refuses.  The workspace holds n_tones planes of partial rows.
 *   COST (one MI355X): a bank of 2 / 4 / 8 tones takes 1.13 x / 1.38 x / 1.87 x the single call's time
 * where as many single calls take 2 x / 4 x / 8 x.  A call with 3 or 5 .. 7 tones runs the kernel of 4 or 8 and costs what
 * that costs.  X3_TONE_BANK_MAX is 8 because the 8-tone kernel, at 4 waves per SIMD, still measured 1.5 x FASTER than two
 * calls of 4; the call does not split wide banks. */
#define X3_TONE_BANK_MAX 8
typedef struct x3_level_tone_bank {
  uint32_t n_tones;                  /* 1 .. X3_TONE_BANK_MAX */
  uint32_t reserved;                 /* 0 */
  const int16_t* d_table;            /* device: x3_level_tone's table, ONE for all tones */
  uint32_t steps[X3_TONE_BANK_MAX];  /* steps[t], t < n_tones; the rest is never read */
} x3_level_tone_bank;
int x3_tone_bank_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                            const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                            const uint64_t* d_seg_index, uint32_t seg_blocks, uint64_t bin_len,
                            x3_tone_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, const x3_level_tone_bank* bank);
int x3_corpus_tone_bank_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, uint64_t bin_len, x3_tone_level* d_levels,
                                   uint64_t n_rows, int32_t* d_frame_status, const x3_level_tone_bank* bank);
/* ---- EVENTS (no counterpart in the reference): runs of loud bins of level records as ranges (entry, start, len), found on
 * the device -- the link between the levels calls and the ranges calls, with no host trip.
 *   Row b of d_levels is a bin of bin_len positions as x3_levels_dev / x3_corpus_levels_dev write it.  A bin is HOT when
 * its n != 0 and sum_sq >= mean_sq_min * n (mean_sq_min != 0) or max(max, -min) >= peak_min (peak_min != 0); a bin with
 * n == 0 -- every bin of a frame that failed -- is never hot.  A RUN is a maximal set of hot bins of ONE entry whose gaps
 * are at most join_bins cold bins; it spans [first hot, last hot].  Runs of fewer than min_bins bins are dropped and do not
 * exist for anything that follows.  A kept run is padded by pad_bins bins on both sides, clipped to its entry's rows, to bins
 * [b0, b1), and cut into pieces of max_bins bins, the last one shorter.  Piece [p0, p1) is the EVENT start = p0 * bin_len,
 * len = min(p1 * bin_len, n_samples) - start, positions relative to the entry.  2 * pad_bins <= join_bins leaves a cold bin
 * between padded runs: events are disjoint and strictly increasing in (entry, start).  An event's x3_level is the merge of
 * the records of ALL its bins, padding included, from the identities on: sum_sq, sum and n added (n modulo 2^32), min and
 * max taken.  Everything is integer arithmetic; the result is exact. */
typedef struct x3_event_rule {   /* 32 bytes */
  uint64_t mean_sq_min;  /* 0: off.  A bin is hot when sum_sq >= mean_sq_min * n          (<= 1 << 30) */
  uint32_t peak_min;     /* 0: off.  A bin is hot when max(max, -min) >= peak_min         (<= 32768)   */
  uint32_t join_bins;    /* hot bins with at most this many cold bins between them are one run */
  uint32_t min_bins;     /* runs spanning fewer bins (first hot .. last hot) are dropped; 0 and 1: none */
  uint32_t pad_bins;     /* bins added on both sides of a kept run, clipped to the entry; 2 * pad_bins <= join_bins */
  uint32_t max_bins;     /* a longer event is cut into pieces of max_bins, the last one shorter; 0: floor(0xFFFFFFFF / bin_len) */
  uint32_t reserved;     /* 0 */
} x3_event_rule;
/* The stream form: ONE entry.  d_total: a device pointer to one word, the stream's sample count (d_sample_offsets +
 * n_frames is the natural argument); it is untrusted, the rows counted are min(n_bins, ceil(*d_total / bin_len)).
 *   Outputs (device arrays of cap elements): d_starts (uint64), d_lens (uint32), d_event_levels (x3_level; may be NULL);
 * d_count (one uint64) receives the number of events FOUND, which may exceed cap -- the caller grows the arrays and repeats,
 * as with the packed ranges.  Slots [0, min(count, cap)) hold the first events in order; EVERY slot behind them up to cap
 * is written as the filler (entry 0, start 0, len 0, the identity record), so the arrays can go to x3_decode_ranges_dev with
 * n_ranges = cap as they are: a filler range has status 0 and writes nothing.  Nothing outside these arrays is written,
 * nothing outside d_levels[0 .. n_bins) and *d_total is read.
 *   Asynchronous on the context's stream: one launch set, no host trip, nothing allocated after the first call of a size.
 * The call has a pending slot and a workspace of its own; the states of x3_decode_dev, the window / ranges calls and the
 * levels calls are left alone.  X3_ERR_BAD_ARG with nothing enqueued for bin_len == 0 or above 0xFFFFFFFF, both criteria
 * 0, mean_sq_min above 1 << 30, peak_min above 32768, 2 * pad_bins > join_bins, max_bins * bin_len > 0xFFFFFFFF,
 * reserved != 0, cap == 0 or above 0x7FFFFFFF, n_bins == 0 or above 0x7FFFFFFF, a NULL or misaligned pointer (8 bytes;
 * d_lens 4) other than d_event_levels, and a context that is recording a graph. */
int x3_events_dev(x3_ctx* ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                  const x3_event_rule* rule, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels, uint64_t cap,
                  uint64_t* d_count);
/* The corpus form: rows as x3_corpus_levels_dev lays them (n_rows must be x3_corpus_levels_rows' last word, as there); the
 * row prefix is computed on the device from the corpus's entry table, an entry's rows are clipped to n_rows.  Entry e's
 * events are exactly x3_events_dev's on that entry's rows alone with *d_total = its n_samples; d_entries (uint32, cap
 * elements, required) receives the events' entries.  Otherwise as x3_events_dev; also X3_ERR_BAD_ARG with nothing enqueued
 * for a context on another device than the build's.  The arrays go to x3_corpus_ranges_dev as they are. */
int x3_corpus_events_dev(x3_ctx* ctx, const x3_corpus* corpus, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len,
                         const x3_event_rule* rule, uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens,
                         x3_level* d_event_levels, uint64_t cap, uint64_t* d_count);
/* Waits for the last x3_events_dev / x3_corpus_events_dev: the number of events found (what d_count holds). */
int x3_events_result(x3_ctx* ctx, uint64_t* count);
/* ---- LEVEL QUANTILES AND ADAPTIVE THRESHOLDS (no counterpart in the reference): the threshold the events rule needs, chosen
 * on the device per entry, so that levels -> thresholds -> events -> ranges never leaves HBM.
 *   ROWS AND ENTRIES are exactly the events calls': the stream form is one entry of min(n_bins, ceil(*d_total / bin_len))
 * rows (d_total untrusted), the corpus form has the rows of x3_corpus_levels_dev, the row prefix computed on the device from
 * the corpus's entry table and clipped to n_rows.  A row COUNTS for its entry when it lies in one and its n != 0; K(e) is the
 * number of counting rows of entry e.
 *   KEYS.  X3_LEVEL_KEY_PEAK: max(max, -min), 0 .. 32768.  X3_LEVEL_KEY_MEAN_SQ: floor(sum_sq / n), 0 .. 1 << 30.  These are
 * the largest peak_min / mean_sq_min at which the events rule still calls the row hot (sum_sq >= m * n is
 * floor(sum_sq / n) >= m), so a quantile of keys is directly a threshold.  A key outside its range (hand-made records) is
 * clamped into it.
 *   QUANTILES.  q_ppm: a HOST array of n_q values (1 .. 8) in millionths, each <= 1000000, in any order, duplicates
 * allowed.  d_values[e * n_q + j] (uint32) is the key of rank floor((K(e) - 1) * q_ppm[j] / 1000000), 0-based, among the
 * entry's counting keys in ascending order -- np.sort(keys)[(K - 1) * q // 1000000], no interpolation, exact -- or 0 when
 * K(e) == 0.  d_counted[e] (uint32) is K(e).  Nothing else is written; nothing outside d_levels[0 .. n_rows), *d_total and
 * the corpus's tables is read.
 *   Asynchronous on the context's stream: one launch set, no host trip, nothing allocated after the first call of a size
 * (a workspace of 8 bytes a row and 1 KiB per entry and quantile).  The calls have a pending slot and a workspace of their
 * own: the states of x3_decode_dev, the window / ranges calls, the levels, events and range-levels calls are left alone.
 * X3_ERR_BAD_ARG with nothing enqueued, and an earlier pending result left as it was, for bin_len == 0 or above 0xFFFFFFFF,
 * n_bins == 0 or above 0x7FFFFFFF, an unknown key, n_q outside 1 .. 8, a q_ppm above 1000000, a NULL or misaligned pointer
 * (d_levels, d_total: 8 bytes; d_values, d_counted: 4), a context that is recording a graph, and (corpus form) a context on
 * another device than the build's or n_rows other than x3_corpus_levels_rows' last word. */
int x3_level_quantiles_dev(x3_ctx* ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                           int key, const uint32_t* q_ppm, uint32_t n_q, uint32_t* d_values, uint32_t* d_counted);
/* The corpus form: n_entries * n_q values, n_entries counts. */
int x3_corpus_level_quantiles_dev(x3_ctx* ctx, const x3_corpus* corpus, const x3_level* d_levels, uint64_t n_rows,
                                  uint64_t bin_len, int key, const uint32_t* q_ppm, uint32_t n_q, uint32_t* d_values,
                                  uint32_t* d_counted);
/* Waits for the last quantiles or thresholds call: the number of entries with K == 0 and the first of them (the entry count
 * if none). */
int x3_level_quantiles_result(x3_ctx* ctx, uint64_t* n_empty, uint64_t* first_empty);
/* THRESHOLDS from quantiles: per entry, for a criterion that is on (its div != 0) and K(e) > 0,
 * thr = clamp(floor(value * mul / div) + add, 1, limit), value the quantile q_ppm of the criterion's key, limit 32768 (peak)
 * or 1 << 30 (mean square), in 64-bit arithmetic that cannot wrap; for a criterion that is off, or K(e) == 0, thr = 0.
 * "6 dB over the median mean square" is {mean_sq_q_ppm = 500000, mean_sq_mul = 4, mean_sq_div = 1, mean_sq_add = 0}.
 * d_thr (8-byte aligned) receives ONE record (stream form) or n_entries records (corpus form); counted is K(e).  Contract,
 * refusals and result call as for the quantiles calls; also X3_ERR_BAD_ARG for both criteria off and a q_ppm above 1000000
 * of a criterion that is on. */
#define X3_LEVEL_KEY_PEAK 0      /* the keys of x3_level_quantiles_dev */
#define X3_LEVEL_KEY_MEAN_SQ 1
typedef struct x3_threshold_rule {   /* 32 bytes */
  uint32_t peak_q_ppm, peak_mul, peak_div, peak_add;             /* peak_div == 0: criterion off */
  uint32_t mean_sq_q_ppm, mean_sq_mul, mean_sq_div, mean_sq_add; /* mean_sq_div == 0: off */
} x3_threshold_rule;
typedef struct x3_event_threshold {  /* 16 bytes, per entry */
  uint64_t mean_sq_min;  /* 0: off for this entry */
  uint32_t peak_min;     /* 0: off for this entry */
  uint32_t counted;      /* K(e) */
} x3_event_threshold;
int x3_level_thresholds_dev(x3_ctx* ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                            const x3_threshold_rule* rule, x3_event_threshold* d_thr);
int x3_corpus_level_thresholds_dev(x3_ctx* ctx, const x3_corpus* corpus, const x3_level* d_levels, uint64_t n_rows,
                                   uint64_t bin_len, const x3_threshold_rule* rule, x3_event_threshold* d_thr);
/* EVENTS with a threshold per entry: x3_events_dev / x3_corpus_events_dev with the rule's two values taken from d_thr[e]
 * (device memory, 8-byte aligned, 1 record or n_entries) for the rows of entry e.  rule->mean_sq_min and rule->peak_min must
 * both be 0 (anything else: X3_ERR_BAD_ARG).  d_thr is untrusted: a value above its limit makes that criterion never hot,
 * both values 0 leave the entry without hot rows, counted is ignored.  Everything behind "hot" is the events' definition word
 * for word -- runs, min_bins, padding, pieces, fillers, d_count -- and x3_events_result serves these calls: they share the
 * events' pending slot and workspace.  With every d_thr[e] = (m, p) the arrays are those of the events call with that rule. */
int x3_events_adaptive_dev(x3_ctx* ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                           const x3_event_rule* rule, const x3_event_threshold* d_thr, uint64_t* d_starts, uint32_t* d_lens,
                           x3_level* d_event_levels, uint64_t cap, uint64_t* d_count);
int x3_corpus_events_adaptive_dev(x3_ctx* ctx, const x3_corpus* corpus, const x3_level* d_levels, uint64_t n_rows,
                                  uint64_t bin_len, const x3_event_rule* rule, const x3_event_threshold* d_thr,
                                  uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels,
                                  uint64_t cap, uint64_t* d_count);
/* ---- PLANE EVENTS (no counterpart in the reference): runs of bins that are loud in at least k of K planes of level records
 * -- the bands of a tone bank, or the samples' records beside their first difference's -- as ONE ordered, disjoint list of
 * ranges (entry, start, len), found on the device.  One rule: plane events are the EVENTS above on
 * one synthetic row verdict; everything behind "hot" is x3_events_dev's definition word for word.
 *   INPUT.  d_levels holds n_planes (1 .. X3_EVENT_PLANES_MAX) planes of x3_level records: plane t is the n_bins records
 * (n_rows for a corpus) at d_levels + t * plane_stride, plane_stride >= n_bins, in records -- what x3_tone_bank_levels_dev
 * and x3_tone_power_levels_dev over all planes write with plane_stride = n_bins.  Every plane has the rows and entries of
 * the events calls: the stream form one entry of min(n_bins, ceil(*d_total / bin_len)) rows, the corpus form
 * x3_corpus_levels_rows' layout.  Records between n_bins and plane_stride are never read.
 *   LOUD.  Plane t is loud at row b when record (t, b) has n != 0 and sum_sq >= mean_sq_min[t] * n (mean_sq_min[t] != 0) or
 * max(max, -min) >= peak_min[t] (peak_min[t] != 0).  A plane with both values 0 is never loud.
 *   HOT.  Row b is hot when it lies in an entry and at least min_planes planes are loud at b: min_planes == 1 is the union of
 * the planes' loud rows, min_planes == n_planes their intersection.  Runs, join_bins, min_bins, pad_bins, clipping to the
 * entry, pieces of max_bins, start, len, order and disjointness, d_count possibly above cap and the fillers are the EVENTS'
 * on these hot rows.
 *   PER EVENT, beside entry, start and len: d_event_planes[i] (uint32, cap elements, may be NULL): bit t is set when plane t
 * is loud in at least one row of the piece, padding rows included -- a padding row loud in fewer than min_planes planes still
 * sets its bits; a piece of a cut run that holds padding or gap rows alone may have no bit set.  d_event_levels (may be
 * NULL): n_planes planes of cap records, plane stride cap; record (t, i) is the merge of plane t's records over the piece's
 * rows.  Fillers: mask 0 and the identity record in every plane.
 *   THRESHOLDS PER ENTRY.  d_thr is NULL or a device array (8-byte aligned) of x3_event_threshold laid plane-major:
 * n_planes records for the stream form, n_planes * n_entries for the corpus form, d_thr[t * n_entries + e] for plane t of
 * entry e -- what n_planes calls of x3_level_thresholds_dev / x3_corpus_level_thresholds_dev write at d_thr + t * n_entries
 * (they may be enqueued back to back; their pending slot is simply overwritten).  With d_thr the rule's mean_sq_min[] and
 * peak_min[] must all be 0.  d_thr is untrusted exactly as in x3_events_adaptive_dev: a value above its limit makes that
 * criterion never loud, both values 0 leave that plane of that entry never loud, counted is ignored.
 *   n_planes == 1, min_planes == 1 gives byte for byte the arrays of x3_events_dev / x3_corpus_events_dev with the rule
 * {mean_sq_min[0], peak_min[0], ...}, and with d_thr those of the adaptive calls.
 *   Asynchronous on the context's stream: one launch set, no host trip.  The calls share the events' pending slot and
 * workspace, as the adaptive calls do (x3_events_result waits); the workspace does not depend on n_planes.  The rule is
 * copied at the call; records and d_thr are read when the kernels run.  X3_ERR_BAD_ARG with nothing enqueued, and an earlier
 * pending result left as it was, for everything x3_events_dev / x3_corpus_events_dev refuses, n_planes 0 or above 8,
 * min_planes 0 or above n_planes, reserved != 0, plane_stride < n_bins or above 0x7FFFFFFF, a mean_sq_min[t] above 1 << 30 or a peak_min[t] above
 * 32768 for t < n_planes, without d_thr fewer than min_planes planes with a criterion on, with d_thr any non-zero value in
 * the rule or a misaligned d_thr, and a misaligned d_event_planes (4 bytes).  Values behind n_planes are never read. */
#define X3_EVENT_PLANES_MAX 8
typedef struct x3_plane_event_rule {          /* 128 bytes */
  uint32_t n_planes;                          /* 1 .. X3_EVENT_PLANES_MAX */
  uint32_t min_planes;                        /* 1 .. n_planes: a row is hot when so many planes are loud at it */
  uint32_t join_bins, min_bins, pad_bins, max_bins;   /* x3_event_rule's, same meaning and limits */
  uint32_t reserved[2];                       /* 0 */
  uint64_t mean_sq_min[X3_EVENT_PLANES_MAX];  /* per plane; 0: off; entries behind n_planes are never read */
  uint32_t peak_min[X3_EVENT_PLANES_MAX];     /* per plane; 0: off */
} x3_plane_event_rule;
int x3_plane_events_dev(x3_ctx* ctx, const x3_level* d_levels, uint64_t plane_stride, uint64_t n_bins, uint64_t bin_len,
                        const uint64_t* d_total, const x3_plane_event_rule* rule, const x3_event_threshold* d_thr,
                        uint64_t* d_starts, uint32_t* d_lens, uint32_t* d_event_planes, x3_level* d_event_levels,
                        uint64_t cap, uint64_t* d_count);
int x3_corpus_plane_events_dev(x3_ctx* ctx, const x3_corpus* corpus, const x3_level* d_levels, uint64_t plane_stride,
                               uint64_t n_rows, uint64_t bin_len, const x3_plane_event_rule* rule,
                               const x3_event_threshold* d_thr, uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens,
                               uint32_t* d_event_planes, x3_level* d_event_levels, uint64_t cap, uint64_t* d_count);
/* ---- RANGE LEVELS (no counterpart in the reference): the level records of ranges (entry, start, len), bins counted from
 * each range's own start -- a second look inside events at finer bins, a zoomed overview, peak and RMS of any sample-exact
 * cut.  The work follows the ranges (their covering frames), not the stream.
 *   RANGE AND BINS.  Range w is positions [d_starts[w], d_starts[w] + d_lens[w]) exactly as x3_decode_ranges_dev defines
 * them (the corpus form: relative to entry d_entries[w], as x3_corpus_ranges_dev).  Bin b of range w covers positions
 * [start + b * bin_len, start + (b + 1) * bin_len) cut to the range.  bin_len == 0 is one bin; a length has 32 bits, so any
 * bin_len >= 2^32 is one bin too.
 *   ROWS.  Range w has R(w) = max(1, ceil(d_lens[w] / bin_len)) rows, 1 with bin_len == 0: the rule x3_corpus_levels_dev has
 * for entries.  R(w) depends on the length alone, for bad ranges too.
 *   SAMPLES COUNTED.  A sample is added to its bin when the frame that holds it has status 0 -- the status a window that is
 * exactly that frame gets from x3_decode_windows_dev.  Any other frame adds nothing, also when some of its blocks decode
 * cleanly.  This is x3_levels_dev's rule, not the ranges' "prefix, then zeros": n tells what was counted, and the range
 * (0, total) at the same bin_len equals x3_levels_dev's records on the same stream, damaged frames included.
 *   STATUS.  d_status[w] is the status of the first covering frame, in frame order, that is not 0, and 0 if there is none.
 * A range with start > total or len > total - start is X3_ERR_BAD_ARG, and so is an entry outside the corpus; all rows of
 * such a range are the identity {0, 0, 32767, -32768, 0, 0}.  A length of 0 with start <= total is status 0 and one identity
 * row (start + len - 1 is never formed).
 *   PACKED (row_stride == 0): range w's rows begin at row_off[w], the exclusive sum of ALL R(w).  d_row_offsets (required)
 * receives row_off[0 .. n_ranges].  A range with row_off[w] + R(w) > rows_cap is X3_ERR_BAD_ARG and none of its records is
 * written; what fits is complete, and x3_range_levels_result reports the total, so a caller grows d_levels and repeats.
 *   PADDED (row_stride > 0): range w's rows begin at w * row_stride, and records [R(w), row_stride) of every row are the
 * identity.  R(w) > row_stride is X3_ERR_BAD_ARG and a row of identities.  n_ranges * row_stride > rows_cap fails the call.
 * d_row_offsets may be NULL; when given it receives w * row_stride (n_ranges + 1 words).
 *   Every record of a range that has room is written, with identities where nothing falls.  All five quantities are
 * integers: the records are exact whatever the order of execution; n counts modulo 2^32.  Nothing outside
 * d_levels[0 .. rows_cap), d_status[0 .. n_ranges) and d_row_offsets[0 .. n_ranges] is written, nothing outside
 * [d_x3, d_x3 + x3_len) is read: starts, lengths, offsets, sample offsets, index and bytes are untrusted as in
 * x3_decode_ranges_dev.  The segment index is a hint that changes time, never results.
 *   How: the ranges' plan and check, x3_levels_dev's consumer.  A PAIR is (range, covering frame); its stretches add to rows
 * of the pair's own in a workspace, and only a frame whose every stretch has been proven is added to d_levels; a flagged one
 * goes through the reference's reader.  The workspace holds P = min(n_ranges * max frames of a range, 4 * (n_frames +
 * n_ranges)) pairs and rows_cap + P partial rows; pairs beyond either go through the reader too (time, never a result).
 *   Asynchronous on the context's stream: one launch set, no host trip, nothing allocated after the first call of a size.
 * The call has a pending slot and a workspace of its own: the states of x3_decode_dev, the window / ranges calls, the levels
 * calls and the events calls are left alone.  X3_ERR_BAD_ARG with nothing enqueued for n_ranges == 0 or above 0x7FFFFFFF,
 * rows_cap == 0 or above 0x7FFFFFFF, a NULL or misaligned pointer (d_starts, d_levels, d_row_offsets: 8 bytes; d_lens,
 * d_entries, d_status: 4; d_row_offsets NULL only when padded), a seg_blocks or parameters that x3_decode_ranges_dev refuses,
 * a context that is recording a graph, and (corpus form) a context on another device than the build's. */
int x3_range_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                        const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                        const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                        const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                        x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status);
/* The corpus form: range w lies in entry d_entries[w]; each result equals x3_range_levels_dev on that entry alone.  The
 * arrays x3_corpus_events_dev wrote go in as they are (a filler is a zero-length range: one identity row, status 0). */
int x3_corpus_range_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                               const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                               x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status);
/* Waits for the last x3_range_levels_dev / x3_corpus_range_levels_dev: ranges with status != 0, the first of them (n_ranges
 * if none), its status, and the sum of all R(w) (what a packed d_levels must hold for no range to be refused). */
int x3_range_levels_result(x3_ctx* ctx, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status, uint64_t* total_rows);
/* ---- SIGNAL RANGE LEVELS: the range-levels calls with the signal of x3_signal_levels_dev, so that events found on the first
 * difference can be looked at again on the signal they were found on.  The arguments of
 * x3_range_levels_dev / x3_corpus_range_levels_dev plus a last `signal`; any value but the two below is X3_ERR_BAD_ARG with
 * nothing enqueued, tested before every other argument.
 *   X3_LEVEL_SIGNAL_SAMPLES: the bytes of x3_range_levels_dev / x3_corpus_range_levels_dev, which are this form.
 *   X3_LEVEL_SIGNAL_DIFF: ONE RULE -- the call cuts the stream's (or entry's) difference signal; it does not difference the
 * cut.  With y the signal x3_signal_levels_dev defines on the stream or entry that holds the range (y[pos] = clamp(x[pos] -
 * x[pos - 1], -32768, 32767); counted inside a frame iff the frame has status 0, at a frame's sample 0 iff the frame and the
 * one in front of it both have status 0 and belong to the same entry, never at the first position of a stream or entry),
 * range w has the records of the SAMPLES form with y[start + r] in place of x[start + r], r in [0, len).  Rows R(w), bins
 * from the range's start, packed and padded layouts, row offsets, rows_cap rules, refusals and identities are unchanged.
 *   - The difference at the range's own first position IS counted when y counts it: its x[pos - 1] lies outside the range,
 *     and possibly in the frame in front of the first covering frame (the LEAD FRAME).
 *   - The range (0, total) at bin length b equals x3_signal_levels_dev(..., X3_LEVEL_SIGNAL_DIFF) at b, record for record,
 *     damaged frames included.
 *   - A range whose start and length are multiples of b equals the slice of those records, the last record cut to the
 *     range's length.
 *   - d_status[w] is exactly the SAMPLES form's: the status of the first covering frame in frame order that is not 0.  The
 *     lead frame never gives the range its status; if it fails, the one seam it shares with the range is not counted ("a
 *     failed frame takes both of its seams with it").
 *   - n counts differences: a clean range (0, N) over a clean entry of N samples has n == N - 1 in all; a clean range that
 *     does not start at the entry's first position has n == len.
 *   - The records are int16-signal records (the identity for empty bins, peak <= 32768): they go into the events,
 *     quantiles and thresholds calls unchanged.
 *   x3_range_levels_result, the pending slot, the workspace and the options "last_range_levels_replays" /
 * "last_range_levels_overflow" are shared with the SAMPLES form; a lead-frame pair that the fix-up decodes counts as a
 * replay.  With DIFF the workspace holds one more pair per range (the second arm of P is 4 * (n_frames + n_ranges) +
 * n_ranges), a word per frame (its last sample) and a word per range. */
int x3_signal_range_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                               const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                               const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                               const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                               x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status, int signal);
int x3_corpus_signal_range_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                                      const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                      x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                      int signal);
/* ---- FIR RANGE LEVELS: the range-levels calls on the FIR signal of x3_fir_levels_dev, so that events found behind a filter
 * can be looked at again on the signal they were found on.  The arguments of x3_range_levels_dev /
 * x3_corpus_range_levels_dev plus a last `fir`, validated by the rule of x3_fir_levels_dev (1 .. 8 taps, shift <= 15, sum |c|
 * <= 32768); a NULL or invalid fir is X3_ERR_BAD_ARG with nothing enqueued, tested before every other argument.
 *   ONE RULE -- the call cuts the stream's (or entry's) FIR signal; it does not filter the cut.  With y the signal
 * x3_fir_levels_dev defines on the stream or entry that holds the range (y[i] = clamp((sum over t < T of c[t] * x[i - t]) >>
 * shift, -32768, 32767); counted by THE HISTORY RULE: all T positions i - T + 1 .. i exist in the same stream or entry and
 * lie in frames with status 0), range w has the records of x3_range_levels_dev with y[start + r] in place of x[start + r],
 * r in [0, len).  Rows R(w), bins from the range's start, packed and padded layouts, row offsets, rows_cap rules, refusals
 * and identities are unchanged.
 *   - The first T - 1 positions of a range ARE counted when y counts them: their earlier samples lie in front of the range,
 *     possibly in up to T - 1 frames in front of the first covering frame (LEAD FRAMES; a frame can be one sample long).
 *   - The range (0, total) at bin length b equals x3_fir_levels_dev at b, record for record, damaged frames included.
 *   - A range whose start and length are multiples of b equals the slice of those records, the last record cut to the
 *     range's length.
 *   - Taps {1} give the bytes (records, offsets, statuses) of x3_range_levels_dev; taps {1, -1} give the bytes of
 *     x3_signal_range_levels_dev(..., X3_LEVEL_SIGNAL_DIFF).
 *   - d_status[w] is exactly the SAMPLES form's: the status of the first covering frame in frame order that is not 0.  A
 *     lead frame never gives the range a status; a lead frame that fails takes away the range positions whose taps reach it
 *     or reach past it, and nothing else.
 *   - n counts filter outputs: a clean range that starts at least T - 1 positions into a clean entry has n == len in all.
 *   - The records are int16-signal records: they go into the events, quantiles and thresholds calls unchanged.
 *   x3_range_levels_result, the pending slot, the workspace and the options "last_range_levels_replays" /
 * "last_range_levels_overflow" are shared with the other forms; a lead-frame pair that the fix-up decodes counts as a replay.
 * The workspace holds up to T - 1 more pairs per range (the second arm of P is 4 * (n_frames + n_ranges) + (T - 1) *
 * n_ranges) and, beside it, the 32-byte edge record per (frame, stretch) of x3_fir_levels_dev. */
int x3_fir_range_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                            const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                            const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                            const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                            x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                            const x3_level_fir* fir);
int x3_corpus_fir_range_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                                   const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                   x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                   const x3_level_fir* fir);
/* ---- TONE RANGE LEVELS: the range-levels calls on the tone signal of x3_tone_levels_dev, so that events found in a band
 * can be looked at again, at finer bins, in that band.  The arguments of x3_range_levels_dev /
 * x3_corpus_range_levels_dev with x3_tone_level records and a last `tone`, validated by the rule of x3_tone_levels_dev: a
 * NULL tone, a NULL or misaligned (4 bytes) d_table or reserved != 0 is X3_ERR_BAD_ARG with nothing enqueued, tested before
 * every other argument.  The struct is copied at the call; the table is read when the kernels run.
 *   ONE RULE -- the call cuts the stream's (or entry's) tone signal; it does NOT restart the oscillator at the range.
 * Position i of the stream or entry that holds the range has the phase ph(i) = (i * step) mod 2^32 and the table pair
 * k(i) = ph(i) >> 22, exactly as in x3_tone_levels_dev: every corpus entry starts at phase 0 and i is counted from the entry's
 * first position.  Range w = (start, len) has the records of x3_range_levels_dev with
 *     re = sum of x[start + r] * cos[k(start + r)],  im = sum of x[start + r] * sin[k(start + r)]
 * over the positions of a bin that lie in frames with status 0, and min, max, n field for field those of the SAMPLES
 * range-levels record.  An empty bin is {0, 0, 32767, -32768, 0, 0}.
 *   - The range (0, total) at bin length b equals x3_tone_levels_dev at b, record for record, damaged frames included.
 *   - A range whose start and length are multiples of b equals the slice of those records, the last record cut to the range.
 *   - A table of all (1, 0) gives re == the sum of the SAMPLES range-levels record and im == 0, with its min, max and n;
 *     step 0 with the usual table gives re == 32767 * that sum.
 *   - d_status[w], row offsets, R(w), packed and padded layouts, rows_cap rules, refusals, zero-length ranges and identities
 *     are x3_range_levels_dev's byte for byte; the status never depends on the tone.
 *   - THE PHASE IS THE STREAM'S: two ranges of equal length at different starts over identical samples differ in re and im
 *     (by the rotation through the phase between their starts, up to the table's rounding).  Across ranges compare BAND
 *     POWER -- re^2 + im^2, or the records x3_tone_power_levels_dev makes of them -- never the raw sums.
 *   x3_range_levels_result, the pending slot, the workspace and the options "last_range_levels_replays" /
 * "last_range_levels_overflow" are shared with the other forms; P is the SAMPLES form's (there are no lead frames) and there
 * is no workspace beyond it.  Packed or padded, the records go through x3_tone_power_levels_dev unchanged. */
int x3_tone_range_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                             const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                             const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                             const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                             x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                             const x3_level_tone* tone);
int x3_corpus_tone_range_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries, const uint64_t* d_starts,
                                    const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                    x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                    const x3_level_tone* tone);
/* ---- TONE BANK RANGE LEVELS: the range-levels calls on up to X3_TONE_BANK_MAX tones at once, so that events found in
 * several bands by one x3_tone_bank_levels_dev pass can be looked at again, at finer bins, in ALL those bands for one decode
 * of the covering frames instead of one per band.  The arguments of x3_tone_range_levels_dev /
 * x3_corpus_tone_range_levels_dev with `bank` (x3_level_tone_bank, above) where `tone` stands.
 *   ONE RULE: the bank is n_tones tone-range calls laid PLANE BY PLANE, with plane stride rows_cap.  d_levels holds
 * n_tones * rows_cap x3_tone_level records; plane t is the rows_cap records at d_levels + t * rows_cap, byte for byte what
 * x3_tone_range_levels_dev (or the corpus form) writes into a buffer of rows_cap records for {steps[t], 0, d_table} with the
 * same other arguments.  Records a call does not write stay untouched in EVERY plane: those of ranges without room when
 * packed, those behind n_ranges * row_stride when padded.
 *   - d_row_offsets, d_status and x3_range_levels_result exist once and are the single call's; total_rows is ONE plane's.
 *     The status never depends on the bank; "last_range_levels_replays" and "last_range_levels_overflow" have the values of
 *     one tone call with the same arguments.
 *   - The oscillators are not restarted at a range: position i of the stream or entry has the phase (i * steps[t]) mod 2^32
 *     in plane t, and every corpus entry starts at phase 0.  (The product is formed in 64 bits and truncated per slot as in
 *     the single call; positions past 2^32 are the single call's, per slot.)
 *   - A plane does not depend on the other steps; permuting the steps permutes the planes; equal steps give equal planes;
 *     min, max and n are the same in all planes.  n_tones == 1 IS x3_tone_range_levels_dev.
 *   - The range (0, total) at bin length b equals x3_tone_bank_levels_dev at b, plane for plane, damaged frames included.
 *   - All planes go through x3_tone_power_levels_dev in ONE launch of n_tones * rows_cap rows -- when every record of
 *     every plane is defined: the untouched ones are the caller's bytes (zero them first: a zero record has n == 0 and comes
 *     out as the identity).
 *   X3_ERR_BAD_ARG with nothing enqueued, tested before every other argument: a NULL bank, n_tones 0 or above
 * X3_TONE_BANK_MAX, reserved != 0, a NULL or misaligned (4 bytes) d_table; then n_tones * rows_cap > 2^31 - 1; then
 * everything x3_range_levels_dev refuses.  The struct is copied at the call, steps behind n_tones are never read, and the
 * table is read when the kernels run.  The pending slot, the asynchronous contract and "a failed frame adds nothing, to no
 * plane" are the other forms'.  The workspace is shared with them and holds n_tones * (rows_cap + P) partial rows, P the
 * SAMPLES form's: there are no lead frames.  A call with 3 or 5 .. 7 tones runs the kernel of 4 or 8 (DESIGN.md section 27
 * has the cost). */
int x3_tone_bank_range_levels_dev(x3_ctx* ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                                  const uint64_t* d_sample_offsets, uint64_t n_frames, const x3_params* p,
                                  const uint64_t* d_seg_index, uint32_t seg_blocks, const uint64_t* d_starts,
                                  const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride,
                                  x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                                  const x3_level_tone_bank* bank);
int x3_corpus_tone_bank_range_levels_dev(x3_ctx* ctx, const x3_corpus* corpus, const uint32_t* d_entries,
                                         const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges, uint64_t bin_len,
                                         uint64_t row_stride, x3_tone_level* d_levels, uint64_t rows_cap,
                                         uint64_t* d_row_offsets, int32_t* d_status, const x3_level_tone_bank* bank);
/* ---- SPECTRA (no counterpart in the reference): the exact integer STFT of int16 rows that lie in HBM as
 * x3_decode_ranges_dev / x3_corpus_ranges_dev wrote them -- what an event looks like, every bin of every frame, where the
 * tone bank stops at eight frequencies.  The products run on the matrix cores
 * (v_mfma_i32_16x16x64_i8: a 16 x 16 bit product is four 8 x 8 bit ones), the results are integers held with ==.
 *   THE RULE is a host struct, copied at the call: n_fft = N in {64, 128, 256, 512, 1024}, hop = H in 1 .. 2^31 - 1, and
 * d_table, x3_level_tone's caller-owned device table of 1 024 (cos, sin) int16 pairs, read when the kernels run; any
 * contents are legal.  B = N / 2 + 1 bins.  For a row of len samples x[0 .. len):
 *     R = 0 when len < N, else (len - N) / H + 1 frames -- whole frames only, there is no partial last frame;
 *     frame r is x[r * H .. r * H + N);  bin k <= N / 2 of it is
 *     re = sum over n < N of x[r * H + n] * cos[((n * k) mod N) * (1024 / N)],   im = the same against sin,
 * int64 and exact, |re| <= N * 2^30.  THE OSCILLATOR RESTARTS AT EVERY FRAME, as in any STFT: unlike the tone range-levels
 * calls, which cut the stream's phase, equal samples give equal spectra wherever the row begins.  When a frame's first
 * sample sits at a position p0 of its stream or entry with p0 mod N == 0, bin k equals re and im of
 * x3_tone_range_levels_dev on the range (p0, N) with bin_len = N, step = k * 2^32 / N and the same table (and plane t of
 * the bank call with steps[t] = k_t * 2^32 / N); a table of all (1, 0) gives re == the frame's sum of samples, im == 0.
 *   FORMATS.  X3_SPECTRA_SUMS: an output row is B pairs (re, im) of int64, 16 * B bytes.  X3_SPECTRA_POWER: B uint32,
 * each x3_tone_power_levels_dev's ms at n = N, word for word: a = re >> 15; b = im >> 15; P = a * a + b * b;
 * ms = min(2^30, floor(floor(2 * P / N) / N)) -- on an aligned frame that record's sum_sq / n.
 *   ROWS IN.  Row w is d_lens[w] samples at d_samples + d_offsets[w]; d_offsets[n_ranges] is never read, so a padded
 * layout's w * stride serves as well as a packed call's offsets.  d_in_status is the ranges call's status array, or NULL
 * for "all 0"; it may equal d_status (in place).  Offsets, lengths and statuses are device data and untrusted.
 *   d_status[w] is, in this order: the in-status when it is not 0; X3_ERR_BAD_ARG when d_offsets[w] + d_lens[w] >
 * samples_cap; X3_ERR_BAD_ARG when the range's rows do not fit (below); else 0.  A range whose status is not 0 has rows
 * of zeros only -- the zeros the ranges call leaves behind a failed frame are never transformed -- and R(w) follows from
 * the length alone, for such ranges too.
 *   ROWS OUT, by x3_range_levels_dev's layout rules.  PACKED (row_stride == 0): range w's rows begin at row
 * d_row_offsets[w], the exclusive sum of all R(w) (n_ranges + 1 words, required); a range that ends past rows_cap is
 * X3_ERR_BAD_ARG and nothing of it is written; x3_spectra_result reports the total, so a caller grows d_out and repeats.
 * PADDED (row_stride > 0): rows begin at w * row_stride, rows [R(w), row_stride) are zeros; R(w) > row_stride is
 * X3_ERR_BAD_ARG and a row block of zeros; n_ranges * row_stride > rows_cap fails the call; d_row_offsets may be NULL.
 *   Nothing outside d_out[0 .. rows_cap) rows, d_status[0 .. n_ranges) and d_row_offsets[0 .. n_ranges] is written,
 * nothing outside d_samples[0 .. samples_cap) and the table is read.  Asynchronous on the context's stream: one launch set,
 * no host trip, nothing allocated after the first call of a size; the call has its own pending slot and workspace and
 * leaves the states of every other call alone.  x3_spectra_result waits: ranges with status != 0, the first of them
 * (n_ranges if none) with its status, and the sum of all R(w); X3_ERR_BAD_ARG when no call is pending.
 *   X3_ERR_BAD_ARG with nothing enqueued, the rule's checks before every other argument: a NULL rule, an n_fft outside
 * the five values, hop == 0 or above 2^31 - 1, an unknown format, reserved != 0, a NULL or misaligned (4 bytes) d_table;
 * then n_ranges == 0 or above 0x7FFFFFFF, rows_cap == 0 or above 0x7FFFFFFF, a NULL or misaligned pointer (d_samples: 2
 * bytes; d_lens, d_in_status, d_status: 4; d_offsets, d_out, d_row_offsets: 8; d_row_offsets NULL only when padded), a
 * context that is recording a graph.  No window function, no transform above 1 024 or off the powers of two. */
#define X3_SPECTRA_SUMS  0
#define X3_SPECTRA_POWER 1
typedef struct x3_spectra_rule {   /* 24 bytes, host struct, copied at the call */
  uint32_t n_fft, hop, format, reserved /* 0 */;
  const int16_t* d_table;          /* device, 4-byte aligned, read when the kernels run */
} x3_spectra_rule;
int x3_spectra_rows_dev(x3_ctx* ctx, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                        const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges, const x3_spectra_rule* rule,
                        uint64_t row_stride, void* d_out, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status);
int x3_spectra_result(x3_ctx* ctx, uint64_t* n_bad, uint64_t* first_bad, int* first_bad_status, uint64_t* total_rows);
/* ---- SPECTRA, BAND LEVELS: the POWER words of x3_spectra_rows_dev folded into bands and summed over consecutive frames,
 * written as planes of x3_level -- the record x3_events_dev, x3_plane_events_dev, the quantiles and the thresholds calls
 * take -- and no row per frame anywhere.  The rule, B = n_fft / 2 + 1, R(w) and the POWER word
 * ms[w][r][k] of frame r, bin k are x3_spectra_rows_dev's; rule->format must be X3_SPECTRA_POWER.
 *   THE FOLD is a host struct, copied at the call: frames_per_bin = M in 1 .. 2^31 - 1, n_bands = K in 1 .. B, and
 * d_bin_band, B uint32 words in device memory (4-byte aligned, read when the kernels run): word k is the band of bin k, any
 * value >= K means "bin k is in no band".  Any contents are legal; bands need not be contiguous; a band may have no bin.
 *   Range w has T(w) = ceil(R(w) / M) time bins; time bin j holds frames [j * M, min((j + 1) * M, R(w))), the last one
 * possibly fewer than M.  For band b and frame r
 *     bp[r][b] = min(2^30, sum over k with bin_band[k] == b of ms[w][r][k])       (the sum in 64 bits, the clamp per frame)
 * and the record of (w, j, b) is n = the frames of the time bin, sum_sq = the sum of their bp, sum = 0,
 * max = min(32767, isqrt(2 * the largest bp among them)), min = -max, reserved = 0: the tone adapter's shape
 * (x3_tone_power_levels_dev), the peak taken over frames, sum_sq / n <= 2^30.  With M = 1 and bin_band[k] = k a record's
 * sum_sq is the POWER word, and on an aligned frame sum_sq / n, max and min are the adapter's at that step (which counts
 * the frame's n_fft samples where this call counts one frame).  Where the call owns a
 * record and no frame falls into it, it holds the identity {0, 0, 32767, -32768, 0, 0}.
 *   LAYOUT.  The rows of a range are its time bins, laid by x3_spectra_rows_dev's rules with T(w) for R(w): packed at the
 * exclusive sum of T(w) (d_row_offsets, n_ranges + 1 words), or padded to row_stride with identity records behind T(w);
 * a range whose rows have no room is X3_ERR_BAD_ARG.  The K bands are K planes, plane b at d_levels + b * plane_stride
 * records; plane_stride 0 means rows_cap.  In every plane the call writes every record of rows [0, min(total, rows_cap))
 * when packed and of [0, n_ranges * row_stride) when padded; a range with a status has identity records only; records
 * between rows_cap and plane_stride are never touched.  Statuses, d_in_status (in place allowed), d_row_offsets, the
 * untrusted offsets and lengths and the asynchronous contract are x3_spectra_rows_dev's, word for word; the pending slot
 * and the workspace are shared with it, and x3_spectra_result serves the result with total_rows = the sum of T(w).
 *   X3_ERR_BAD_ARG with nothing enqueued, in this order: the rule's checks (and a format other than X3_SPECTRA_POWER);
 * then a NULL fold, frames_per_bin == 0 or above 2^31 - 1, n_bands == 0 or above B, a NULL or misaligned d_bin_band,
 * reserved != 0, a non-zero plane_stride below rows_cap, n_bands * max(plane_stride, rows_cap) > 2^31 - 1; then everything
 * x3_spectra_rows_dev refuses (d_levels in the place of d_out). */
typedef struct x3_spectra_fold {     /* 32 bytes, host struct, copied at the call */
  uint32_t frames_per_bin, n_bands;
  uint64_t plane_stride;             /* records; 0: rows_cap */
  const uint32_t* d_bin_band;        /* device, n_fft / 2 + 1 words, 4-byte aligned, read when the kernels run */
  uint64_t reserved;                 /* 0 */
} x3_spectra_fold;
int x3_spectra_levels_dev(x3_ctx* ctx, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                          const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges, const x3_spectra_rule* rule,
                          const x3_spectra_fold* fold, uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap,
                          uint64_t* d_row_offsets, int32_t* d_status);
void x3_corpus_destroy(x3_corpus* corpus);

/* ------------------------------------------------------------------ multi-GPU (no reference analogue) */

/* Frames are independent and 20 + even bytes long, so GPU g encodes a contiguous range of whole frames into its own
 * sub-stream and the sub-streams concatenate without padding; the only coupling is each sub-stream's byte offset.
 * RCCL over xGMI (librccl is opened at run time, on first use): an all-gather of the lengths (8 bytes per rank), and
 * for the reassembly on one rank a grouped ncclSend / ncclRecv, every peer on its own link to the root.
 *
 * x3_shard: ONE rank of a group -- one process (or thread) per GPU, the way torch.distributed.run starts bench.py.
 * Rank 0 makes the id, the others get it out of band; x3_shard_create blocks until all `world` ranks have joined
 * (ncclCommInitRank) and ties the shard to the context's device and stream. */
typedef struct x3_shard x3_shard;
#define X3_SHARD_ID_BYTES 128
int x3_shard_unique_id(uint8_t id[X3_SHARD_ID_BYTES]);
int x3_shard_create(x3_ctx* ctx, const uint8_t id[X3_SHARD_ID_BYTES], int rank, int world, x3_shard** shard);
void x3_shard_destroy(x3_shard* shard);
int x3_shard_rank(const x3_shard* shard);
int x3_shard_world(const x3_shard* shard);
/* Host arithmetic of the sharding.  Rank r owns frames [first, first + count): contiguous, the remainder spread one
 * frame each over the first ranks; samples accordingly (the stream's last frame may be short); starts[r] = exclusive
 * scan of the lengths, starts[world] = total. */
void x3_shard_frame_range(uint64_t n_frames, int rank, int world, uint64_t* first, uint64_t* count);
void x3_shard_sample_range(uint64_t n_samples, const x3_params* p, int rank, int world, uint64_t* first, uint64_t* count);
void x3_shard_offsets(const uint64_t* lengths, int world, uint64_t* starts /* world + 1 */);
/* Step 1, after x3_encode_dev of this rank's samples: all-gather of the sub-stream lengths.  d_len: DEVICE pointer to
 * this rank's length (the last frame offset x3_encode_dev wrote, for a sub-stream that starts at 0); d_lengths:
 * device array of `world` entries or NULL for the shard's own.  Asynchronous on the context's stream.
 * x3_shard_exchange_length_value: the same for a length the host holds.  x3_shard_lengths waits and copies the
 * shard's own array to the host. */
int x3_shard_exchange_lengths(x3_shard* shard, const uint64_t* d_len, uint64_t* d_lengths);
int x3_shard_exchange_length_value(x3_shard* shard, uint64_t len, uint64_t* d_lengths);
int x3_shard_lengths(x3_shard* shard, uint64_t* lengths /* host, world */);
/* Step 2 (optional: a deployment that writes the file in parallel, or decodes where it encoded, never needs it): the
 * whole stream on `root`, d_dst[starts[r] ..) = rank r's d_sub[0 .. lengths[r]).  lengths: host array, identical on
 * all ranks.  d_dst only counts on the root; dst_cap is the ROOT's capacity: every rank that passes it (non-zero) comes
 * to the same verdict before anything is sent, a rank that passes 0 does not check (and would be left waiting in its
 * send if the root refused: size the destination from the lengths first).  Asynchronous on the context's stream. */
int x3_shard_gather(x3_shard* shard, const uint8_t* d_sub, const uint64_t* lengths, int root, uint8_t* d_dst,
                    uint64_t dst_cap, uint64_t* total);
/* The same reassembly beside the context's work: starts behind everything enqueued on the context's stream so far, runs
 * on the shard's own stream and communicator (ncclCommSplit), and the context may go on with its next batch -- into
 * ANOTHER output buffer: d_sub and d_dst stay untouched until x3_shard_gather_wait (on_stream != 0: the context's
 * stream waits, the host does not; 0: the host waits).  One reassembly in flight per shard.  No reference analogue. */
int x3_shard_gather_async(x3_shard* shard, const uint8_t* d_sub, const uint64_t* lengths, int root, uint8_t* d_dst,
                          uint64_t dst_cap, uint64_t* total);
int x3_shard_gather_wait(x3_shard* shard, int on_stream);
/* Step 2, SHARDED: no rank takes in the whole stream.  `encodefile::wav_to_x3a` writes one file through one BufWriter
 * (src/encodefile.rs:66-74); with the frames on N GPUs the equivalent is N writers into ONE file: rank r's sub-stream
 * goes to byte base + starts[r] (x3_shard_offsets) of `fd` -- every rank passes a descriptor of the same file, `base` =
 * what precedes the frames (the archive header, x3_archive_header_write).  Starts behind everything enqueued on the
 * context's stream so far, brings this rank's bytes down over its own host link in 16 MiB pieces (two pinned buffers, a
 * piece is written while the next one is on its way) and returns when they are in the file (pwrite; no fsync).
 * X3_ERR_IO when a write fails.  The single-root reassembly above is bound by the root's seven xGMI links whatever N is;
 * this form scales with the ranks. */
int x3_shard_write_at(x3_shard* shard, const uint8_t* d_sub, const uint64_t* lengths, int fd, uint64_t base,
                      uint64_t* total);

/* x3_mgpu: all GPUs from ONE process -- a context, a shard and a host thread per device.  x3_mgpu_encode /
 * x3_mgpu_decode_stream take and return the same host buffers, bytes and status as x3_encode / x3_decode_stream
 * (encoder::encode, src/encoder.rs:51-111; the walk of src/decodefile.rs:105-136): the samples are dealt out by frame
 * ranges, every GPU encodes its range, the lengths are exchanged and every device copies its sub-stream straight to its
 * place in the caller's host buffer (no reassembly on one GPU first: the destination is host memory);
 * decoding walks the header chain once, deals the frames out and copies every GPU's samples straight to their place
 * (no collective).  x3_mgpu_ctx / x3_mgpu_shard hand out the per-device objects for device-resident use. */
typedef struct x3_mgpu x3_mgpu;
int x3_mgpu_create(const int* devices, int n, x3_mgpu** m);
void x3_mgpu_destroy(x3_mgpu* m);
int x3_mgpu_devices(const x3_mgpu* m);
x3_ctx* x3_mgpu_ctx(x3_mgpu* m, int g);
x3_shard* x3_mgpu_shard(x3_mgpu* m, int g); /* NULL when the group has one GPU */
const char* x3_mgpu_last_error(const x3_mgpu* m);
int x3_mgpu_encode(x3_mgpu* m, const int16_t* wav, uint64_t n, uint32_t n_channels, const x3_params* p, uint8_t* out,
                   uint64_t out_cap, uint64_t start_pos, uint64_t* out_pos, uint64_t stats[6]);
int x3_mgpu_decode_stream(x3_mgpu* m, const uint8_t* x3, uint64_t len, const x3_params* p, int16_t* wav,
                          uint64_t wav_cap, uint64_t* n_out, uint64_t* frames_ok, uint64_t* frame_errors);

/* ------------------------------------------------------------------ parameter tuning (NOT in the reference) */

/* The reference's wav_to_x3a always writes the default parameters (src/encodefile.rs:57), but the archive XML records
 * <BLKLEN> and <T> (:102-111) and parse_xml reads them back (src/decodefile.rs:232-303).  These entry points find, for
 * one input, the parameter set that encodes it in the fewest bytes -- exactly: a candidate's size is the number of
 * bytes x3_encode_dev writes for it from start_pos 0 -- in one read of the samples on the GPU (csrc/x3_tune_kernel.h).
 *
 * CANDIDATES (2 184): the sets the reference decoder reads back exactly, its encoder takes without a panic and the
 * single-pass encoders take: codes (0, 1, 3); block length 10, 20 or 40 (g = 0, 1, 2); t0 in 0..6, t1 in t0..10,
 * t2 in 15..27 (stream-safe for codes (0, 1, 3), t2 >= 15 so that no BFP block is 5 bits wide or less, t0 <= t1 as
 * the decoder never reads thresholds) -- 728 triples per block length.  Candidate index = g * 728 + the rank of
 * (t0, t1, t2) in lexicographic order; the default set (20; 3, 8, 20) is index 1188.  All candidates share the frame
 * length spf (samples per frame; blocks_per_frame = spf / block_len): a multiple of 40 in 40 ..= 10 240.
 * CHOICE: the smallest total; among equal totals the default set if it is one of them, else the lowest index. */

/* Candidate `index` (< X3_TUNE_CANDIDATES) at frame length spf as x3_params.  Host arithmetic.  BAD_ARG for a bad
 * index or spf, or p = NULL. */
int x3_tune_candidate(uint32_t index, uint32_t spf, x3_params* p);
#define X3_TUNE_CANDIDATES 2184
#define X3_TUNE_DEFAULT_INDEX 1188
#define X3_TUNE_DEFAULT_SPF 10000

/* An accumulating tuner: per-candidate 64-bit byte totals (and largest frame payloads) on the context's device.
 * x3_tuner_create(ctx, spf, &t): an empty tuner at frame length spf (BAD_ARG as x3_tune_candidate).
 * x3_tuner_add_dev(t, d_wav, batch): adds the encoded sizes of a device-resident batch (x3_encode_dev's layout:
 *   batch->n_clips clips of batch->n_per_clip samples, clip c at d_wav + c * clip_stride samples).  Enqueued on the
 *   context's stream, no sync.  Every clip is cut into frames from its own start, so the totals of several calls equal
 *   those of one encode of the whole input only when every chunk but the last is whole frames (a multiple of spf
 *   samples): that is the caller's to keep, it cannot be checked.  BAD_ARG, with nothing enqueued and the totals as they
 *   were, for t, d_wav or batch NULL, d_wav not 2-byte aligned, 0 samples or 0 clips, or (n_clips > 1) a clip_stride
 *   smaller than n_per_clip.  d_wav must stay unchanged until the next x3_tuner_result.
 * x3_tuner_result(t, best, best_bytes, sizes): syncs; *best = the chosen candidate (the rule above), *best_bytes its
 *   total, sizes[0 .. 2184) every candidate's total (each may be NULL).  A tuner that has been given nothing reports
 *   totals of 0 and the default set.
 * x3_tuner_max_payloads(t, payloads): syncs; payloads[0 .. 2184) = each candidate's largest frame payload in bytes.
 * x3_tuner_reset empties the totals; x3_tuner_destroy waits for the context's stream and frees the tuner. */
typedef struct x3_tuner x3_tuner;
int x3_tuner_create(x3_ctx* ctx, uint32_t spf, x3_tuner** t);
int x3_tuner_add_dev(x3_tuner* t, const int16_t* d_wav, const x3_batch* batch);
int x3_tuner_result(x3_tuner* t, x3_params* best, uint64_t* best_bytes, uint64_t* sizes);
int x3_tuner_max_payloads(x3_tuner* t, uint32_t* payloads);
int x3_tuner_reset(x3_tuner* t);
void x3_tuner_destroy(x3_tuner* t);

/* The same for wav[0..n) in host memory (n >= 1), taken through the device in chunks of whole frames.  Syncs. */
int x3_tune(x3_ctx* ctx, const int16_t* wav, uint64_t n, uint32_t spf, x3_params* best, uint64_t* best_bytes,
            uint64_t* sizes);

/* x3_x3a_encode with the parameters x3_tune chooses at spf = X3_TUNE_DEFAULT_SPF: the archive header records the chosen
 * BLKLEN and T, the stream follows.  *chosen (may be NULL) receives them (the defaults for n = 0).  The reference's
 * x3a_to_wav reads such an archive back unchanged. */
int x3_x3a_encode_tuned(x3_ctx* ctx, const int16_t* wav, uint64_t n, uint32_t sample_rate, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_len, uint64_t stats[6], x3_params* chosen);

/* ------------------------------------------------------------------ synthetic inputs (bench/tests) */

/* Seeded, integer-only signal generators.  kind: 0 zeros, 1 white i16 noise,
 * 2 hydrophone-like noise (coloured noise + swell + sparse clicks), 3 fixed-point sine,
 * 4 +-2 LSB random walk.  Sample i depends only on (kind, seed, start+i): the host and device
 * versions are bit-identical and any sub-range can be generated independently. */
int x3_synth(int kind, uint64_t seed, uint64_t start, uint64_t n, int16_t* out);
int x3_synth_dev(x3_ctx* ctx, int kind, uint64_t seed, uint64_t start, uint64_t n, int16_t* d_out);

/* device memory helpers so that ctypes/FFI callers need no HIP binding of their own */
int x3_dev_alloc(x3_ctx* ctx, uint64_t bytes, void** d_ptr);
int x3_dev_free(x3_ctx* ctx, void* d_ptr);
int x3_dev_upload(x3_ctx* ctx, void* d_dst, const void* src, uint64_t bytes);   /* syncs */
int x3_dev_download(x3_ctx* ctx, void* dst, const void* d_src, uint64_t bytes); /* syncs */

#ifdef __cplusplus
}
#endif
#endif
