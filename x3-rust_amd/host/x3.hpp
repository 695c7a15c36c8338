// x3.hpp -- host-side mirror of the psiphi75/x3-rust public API on top of the C ABI (include/x3hip.h).
//
// The reference is a Rust crate; this image has no Rust toolchain, so the host layer above the
// C ABI is written in C++ with the reference's module / item names and argument meaning:
//
//   reference (Rust)                                   here (C++)
//   ------------------------------------------------   ---------------------------------------------
//   x3::Parameters::{default,new}     x3.rs:81-134      x3::Parameters{}, x3::Parameters::create()
//   x3::Channel / x3::IterChannel     x3.rs:29-69       x3::Channel, x3::IterChannel<It>
//   x3::FrameHeader / Frame / Archive x3.rs:136-184     x3::FrameHeader, x3::Frame, x3::Archive
//   error::X3Error                    error.rs:27-62    x3::X3Error (same variant order)
//   bytewriter::{ByteWriter,SliceByteWriter,StreamByteWriter}  bytewriter.rs:14-165   x3::bytewriter::*
//   crc::{crc16,update_crc16}         crc.rs:44-58      x3::crc::*
//   encoder::{encode,encode_frame,write_frame_header}  encoder.rs:51-214   x3::encoder::*
//   decoder::{read_frame_header,decode_frame}          decoder.rs:36-118   x3::decoder::*
//   x3::RiceCode / RiceCodes::get     x3.rs:187-260     x3::RiceCode, x3::RiceCodes::get, Parameters::rice_codes
//   decoder::decode_block             decoder.rs:132-145     x3::decoder::decode_block
//   bitreader::BitReader              bitreader.rs:51-176    x3::bitreader::BitReader
//   bitpacker::BitPacker              bitpacker.rs:46-190    x3::bitpacker::BitPacker
//   decodefile::X3aReader             decodefile.rs:47-136   x3::decodefile::X3aReader
//   X3aReader::decode_next_frame loop decodefile.rs:105-136,200-209        x3::decoder::decode_stream
//
// Every function exists twice: with the reference's own argument list (it then runs on x3::default_context(), a
// process-wide context on device $X3HIP_DEVICE or 0, created on first use and serialized by a mutex), and with a
// leading `Context&` for callers that manage devices and streams themselves.
//
// Every bulk call goes to libx3hip.so (HIP kernels on the MI355X); nothing here computes on the CPU
// beyond argument marshalling.  BitPacker / BitReader are handles to device state: their bit work runs in
// kernels too (x3_bits.h) -- they exist for callers of the reference's building blocks, the frame kernels
// do not go through them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <array>
#include <cstdlib>
#include <iterator>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/x3hip.h"

namespace x3 {

// error.rs:27-62 (Ok added as 0; Hip / BadArg appended for the C ABI)
enum class X3Error : int {
  Ok = 0, Io, Hound, BitPack, InvalidEncodingThresh, OutOfBoundsInverse, MoreThanOneChannel,
  ArchiveHeaderXMLInvalid, ArchiveHeaderXMLRiceCode, ArchiveHeaderXMLInvalidKey, FrameLength,
  FrameHeaderInvalidKey, FrameHeaderInvalidPayloadLen, FrameHeaderInvalidHeaderCRC, FrameHeaderInvalidPayloadCRC,
  FrameDecodeInvalidBlockLength, FrameDecodeInvalidIndex, FrameDecodeInvalidNTOGO, FrameDecodeInvalidFType,
  FrameDecodeInvalidRiceCode, FrameDecodeInvalidBPF, FrameDecodeUnexpectedEnd, ByteWriterInsufficientMemory,
  Hip, BadArg
};
inline const char* to_string(X3Error e) { return x3_strerror(static_cast<int>(e)); }

// One GPU + stream + scratch (x3_ctx).  Creation throws when no HIP device is usable: there is no CPU path.
class Context {
 public:
  explicit Context(int device = 0) {
    int rc = x3_ctx_create(device, &ctx_);
    if (rc) throw std::runtime_error("x3::Context: no usable HIP device (libx3hip has no CPU fallback)");
  }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  ~Context() { x3_ctx_destroy(ctx_); }
  x3_ctx* raw() const { return ctx_; }

 private:
  x3_ctx* ctx_ = nullptr;
};

// The context behind the reference-shaped overloads (those without a Context& argument).  One per process, made on
// first use; `lock()` serializes callers, a context is not re-entrant.
inline Context& default_context() {
  static Context ctx([] {
    const char* e = std::getenv("X3HIP_DEVICE");
    return e ? std::atoi(e) : 0;
  }());
  return ctx;
}
inline std::mutex& default_context_mutex() {
  static std::mutex m;
  return m;
}
struct MaybeLock {  // locks the default context's mutex for handles that were made on it
  explicit MaybeLock(std::mutex* m) : m_(m) { if (m_) m_->lock(); }
  ~MaybeLock() { if (m_) m_->unlock(); }
  MaybeLock(const MaybeLock&) = delete;
  MaybeLock& operator=(const MaybeLock&) = delete;
  std::mutex* m_;
};
#define X3_WITH_DEFAULT_CONTEXT(expr)                               \
  do {                                                              \
    std::lock_guard<std::mutex> lk_(::x3::default_context_mutex()); \
    ::x3::Context& ctx = ::x3::default_context();                   \
    return (expr);                                                  \
  } while (0)

// x3.rs:187-194.  The tables live in the library (x3_rice_code_get); `code`/`num_bits` have `len` entries.
struct RiceCode {
  size_t nsubs = 0, offset = 0;
  const uint32_t* code = nullptr;
  const uint32_t* num_bits = nullptr;
  const int16_t* inv = nullptr;
  size_t inv_len = 0;
  size_t len = 0;  // entries in code / num_bits (the slices' .len() in the reference)
};
// x3.rs:196-260
struct RiceCodes {
  static const RiceCode* code(size_t k) {
    static const std::array<RiceCode, 4> t = [] {
      std::array<RiceCode, 4> a;
      for (uint32_t i = 0; i < 4; ++i) {
        x3_rice_code c;
        x3_rice_code_get(i, &c);
        a[i].nsubs = c.nsubs; a[i].offset = c.offset; a[i].code = c.code; a[i].num_bits = c.num_bits;
        a[i].inv = c.inv; a[i].inv_len = c.inv_len; a[i].len = c.len;
      }
      return a;
    }();
    if (k > 3) throw std::out_of_range("RiceCodes::get: code number > 3 (the reference panics on the index)");
    return &t[k];
  }
  static std::array<const RiceCode*, 3> get(const size_t (&code_list)[3]) {
    return {code(code_list[0]), code(code_list[1]), code(code_list[2])};
  }
};

// x3.rs:81-134
struct Parameters {
  static constexpr size_t MAX_BLOCK_LENGTH = 60;
  static constexpr size_t WAV_BIT_SIZE = 16;
  static constexpr size_t DEFAULT_BLOCK_LENGTH = 20;
  static constexpr size_t DEFAULT_BLOCKS_PER_FRAME = 500;
  size_t block_len = DEFAULT_BLOCK_LENGTH;
  size_t blocks_per_frame = DEFAULT_BLOCKS_PER_FRAME;
  size_t codes[3] = {0, 1, 3};
  size_t thresholds[3] = {3, 8, 20};
  std::array<const RiceCode*, 3> rice_codes = {RiceCodes::code(0), RiceCodes::code(1), RiceCodes::code(3)};

  // Parameters::new (x3.rs:98-122)
  static X3Error create(size_t block_len, size_t blocks_per_frame, const size_t (&codes)[3],
                        const size_t (&thresholds)[3], Parameters* out) {
    Parameters p;
    p.block_len = block_len;
    p.blocks_per_frame = blocks_per_frame;
    for (int k = 0; k < 3; ++k) { p.codes[k] = codes[k]; p.thresholds[k] = thresholds[k]; }
    x3_params c = p.c_params();
    int rc = x3_params_validate(&c);
    if (rc) return static_cast<X3Error>(rc);
    p.rice_codes = RiceCodes::get(p.codes);
    *out = p;
    return X3Error::Ok;
  }
  x3_params c_params() const {
    x3_params c;
    c.block_len = (uint32_t)block_len;
    c.blocks_per_frame = (uint32_t)blocks_per_frame;
    for (int k = 0; k < 3; ++k) { c.codes[k] = (uint32_t)codes[k]; c.thresholds[k] = (uint32_t)thresholds[k]; }
    return c;
  }
  static Parameters from_c(const x3_params& c) {
    Parameters p;
    p.block_len = c.block_len;
    p.blocks_per_frame = c.blocks_per_frame;
    for (int k = 0; k < 3; ++k) { p.codes[k] = c.codes[k]; p.thresholds[k] = c.thresholds[k]; }
    p.rice_codes = RiceCodes::get(p.codes);
    return p;
  }
};

// x3.rs:29-45: slice-based channel
struct Channel {
  uint16_t id;
  const int16_t* wav;
  size_t len;
  uint32_t sample_rate;
  Parameters params;
  Channel(uint16_t id_, const int16_t* wav_, size_t len_, uint32_t rate, Parameters p)
      : id(id_), wav(wav_), len(len_), sample_rate(rate), params(p) {}
};

// x3.rs:47-69: iterator-based channel (what encoder::encode takes at this commit)
template <class It>
struct IterChannel {
  uint16_t id;
  It wav, wav_end;
  uint32_t sample_rate;
  Parameters params;
  IterChannel(uint16_t id_, It b, It e, uint32_t rate, Parameters p)
      : id(id_), wav(b), wav_end(e), sample_rate(rate), params(p) {}
};

// x3.rs:70-79
struct X3aSpec {
  uint32_t sample_rate;
  Parameters params;
  uint8_t channels;
};

struct Archive {  // x3.rs:136-141
  static constexpr const char* ID = "X3ARCHIV";
  static constexpr size_t ID_LEN = 8;
};
struct Frame {  // x3.rs:143-146
  static constexpr size_t MAX_LENGTH = 0x7fe0;
};
struct FrameHeader {  // x3.rs:148-184
  uint8_t source_id = 0;
  uint16_t samples = 0;
  uint8_t channels = 0;
  size_t payload_len = 0;
  uint16_t payload_crc = 0;
  static constexpr size_t LENGTH = 20;
  static constexpr uint16_t KEY = 30771;
  static constexpr size_t P_KEY = 0, P_SOURCE_ID = 2, P_CHANNELS = 3, P_SAMPLES = 4, P_PAYLOAD_SIZE = 6, P_TIME = 8,
                          P_HEADER_CRC = 16, P_PAYLOAD_CRC = 18;
};

namespace bytewriter {
enum class SeekFrom { Start, Current, End };

// bytewriter.rs:14-22
struct ByteWriter {
  virtual ~ByteWriter() = default;
  virtual X3Error align(size_t n, size_t* written = nullptr) = 0;
  virtual X3Error write_all(const uint8_t* v, size_t n) = 0;
  virtual X3Error flush() = 0;
  virtual X3Error seek(SeekFrom from, int64_t pos, uint64_t* out = nullptr) = 0;
  virtual X3Error stream_position(uint64_t* pos) = 0;
};

// bytewriter.rs:27-100
class SliceByteWriter : public ByteWriter {
 public:
  SliceByteWriter(uint8_t* slice, size_t len) : slice_(slice), len_(len) {}
  X3Error align(size_t n, size_t* written = nullptr) override {
    size_t residual = p_byte_ % n;
    if (written) *written = residual ? n - residual : 0;
    if (!residual) return X3Error::Ok;
    std::vector<uint8_t> z(n - residual, 0);
    return write_all(z.data(), z.size());
  }
  X3Error write_all(const uint8_t* v, size_t n) override {
    if (n > len_ - p_byte_) return X3Error::ByteWriterInsufficientMemory;
    std::memcpy(slice_ + p_byte_, v, n);
    p_byte_ += n;
    if (p_byte_ > stream_length_) stream_length_ = p_byte_;
    return X3Error::Ok;
  }
  X3Error flush() override { return X3Error::Ok; }
  X3Error seek(SeekFrom from, int64_t pos, uint64_t* out = nullptr) override {
    size_t abs_pos = from == SeekFrom::Start ? (size_t)pos
                     : from == SeekFrom::Current ? (size_t)((int64_t)p_byte_ + pos)
                                                 : (size_t)((int64_t)stream_length_ + pos);
    if (abs_pos > len_) return X3Error::ByteWriterInsufficientMemory;
    p_byte_ = abs_pos;
    if (p_byte_ > stream_length_) stream_length_ = p_byte_;
    if (out) *out = p_byte_;
    return X3Error::Ok;
  }
  X3Error stream_position(uint64_t* pos) override { *pos = p_byte_; return X3Error::Ok; }
  // direct access for the zero-copy encode path
  uint8_t* data() { return slice_; }
  size_t capacity() const { return len_; }
  size_t position() const { return p_byte_; }
  void advance_to(size_t pos) { p_byte_ = pos; if (p_byte_ > stream_length_) stream_length_ = p_byte_; }

 private:
  uint8_t* slice_;
  size_t len_;
  size_t p_byte_ = 0, stream_length_ = 0;
};

// bytewriter.rs:106-165 over any seekable std::ostream
class StreamByteWriter : public ByteWriter {
 public:
  explicit StreamByteWriter(std::ostream& os) : os_(os) {}
  X3Error align(size_t n, size_t* written = nullptr) override {
    uint64_t pos = 0;
    stream_position(&pos);
    size_t residual = pos % n;
    if (written) *written = residual ? n - residual : 0;
    if (!residual) return X3Error::Ok;
    std::vector<uint8_t> z(n - residual, 0);
    return write_all(z.data(), z.size());
  }
  X3Error write_all(const uint8_t* v, size_t n) override {
    os_.write(reinterpret_cast<const char*>(v), (std::streamsize)n);
    return os_ ? X3Error::Ok : X3Error::Io;
  }
  X3Error flush() override { os_.flush(); return os_ ? X3Error::Ok : X3Error::Io; }
  X3Error seek(SeekFrom from, int64_t pos, uint64_t* out = nullptr) override {
    os_.seekp(pos, from == SeekFrom::Start ? std::ios::beg : from == SeekFrom::Current ? std::ios::cur : std::ios::end);
    if (!os_) return X3Error::Io;
    if (out) *out = (uint64_t)os_.tellp();
    return X3Error::Ok;
  }
  X3Error stream_position(uint64_t* pos) override { *pos = (uint64_t)os_.tellp(); return X3Error::Ok; }

 private:
  std::ostream& os_;
};
}  // namespace bytewriter

namespace crc {
// crc.rs:44-47
inline uint16_t update_crc16(uint16_t c, uint8_t data) { return x3_crc16_update(c, data); }
// crc.rs:49-58 (GPU segmented reduction)
inline X3Error crc16(Context& ctx, const uint8_t* data, size_t n, uint16_t* out) {
  return static_cast<X3Error>(x3_crc16(ctx.raw(), data, n, out));
}
inline uint16_t crc16(const uint8_t* data, size_t n) {  // the reference's own signature: no error path
  std::lock_guard<std::mutex> lk(default_context_mutex());
  uint16_t c = 0;
  if (x3_crc16(default_context().raw(), data, n, &c)) throw std::runtime_error(x3_last_error(default_context().raw()));
  return c;
}
}  // namespace crc

// bitpacker.rs:46-190 (the subset the encoder uses: write_bits, write_packed_zeros, word_align, len, crc; dropping
// it flushes).  The fields are packed by a kernel when the packer is finished or dropped.
namespace bitpacker {
class BitPacker {
 public:
  // BitPacker::new(&mut SliceByteWriter): packs into the slice from the writer's position on
  explicit BitPacker(bytewriter::SliceByteWriter& writer) : BitPacker(default_context(), writer) {
    mu_ = &default_context_mutex();
  }
  BitPacker(Context& ctx, bytewriter::SliceByteWriter& writer) : writer_(writer) {
    MaybeLock lk(&ctx == &default_context() ? &default_context_mutex() : nullptr);
    int rc = x3_bitpacker_new(ctx.raw(), writer.data(), writer.capacity(), writer.position(), &bp_);
    if (rc) throw std::runtime_error("x3::bitpacker::BitPacker: x3_bitpacker_new failed");
  }
  BitPacker(const BitPacker&) = delete;
  BitPacker& operator=(const BitPacker&) = delete;
  ~BitPacker() {  // Drop (bitpacker.rs:56-62) flushes
    finish();
    x3_bitpacker_free(bp_);
  }
  X3Error write_bits(size_t value, size_t num_bits) {
    return static_cast<X3Error>(x3_bitpacker_write_bits(bp_, value, (uint32_t)num_bits));
  }
  X3Error write_packed_zeros(size_t num_zeros) {
    return static_cast<X3Error>(x3_bitpacker_write_packed_zeros(bp_, (uint32_t)num_zeros));
  }
  X3Error word_align() { return static_cast<X3Error>(x3_bitpacker_word_align(bp_)); }
  // write_bytes (bitpacker.rs:95-102) and inc_counter_n_bytes (:112-118)
  X3Error write_bytes(const uint8_t* array, size_t n) { return static_cast<X3Error>(x3_bitpacker_write_bytes(bp_, array, n)); }
  X3Error inc_counter_n_bytes(size_t n_bytes) { return static_cast<X3Error>(x3_bitpacker_inc_counter_n_bytes(bp_, n_bytes)); }
  // flush (bitpacker.rs:79-86): a partial byte is zero-padded, the packing kernel runs, the writer moves on
  X3Error finish() {
    MaybeLock lk(mu_);
    uint64_t pos = 0, len = 0;
    uint16_t crc = 0;
    int rc = x3_bitpacker_finish(bp_, &len, &crc, &pos);
    if (rc == 0) writer_.advance_to((size_t)pos);
    return static_cast<X3Error>(rc);
  }
  // len() / crc() (bitpacker.rs:75-90): complete bytes so far and their CRC-16
  size_t len() const {
    uint64_t n = 0;
    x3_bitpacker_peek(bp_, &n, nullptr);
    return (size_t)n;
  }
  uint16_t crc() const {
    MaybeLock lk(mu_);
    uint16_t c = 0;
    if (x3_bitpacker_peek(bp_, nullptr, &c)) throw std::runtime_error("x3::bitpacker::BitPacker::crc: HIP error");
    return c;
  }

 private:
  bytewriter::SliceByteWriter& writer_;
  x3_bitpacker* bp_ = nullptr;
  std::mutex* mu_ = nullptr;
};
}  // namespace bitpacker

// bitreader.rs:51-176
namespace bitreader {
class BitReader {
 public:
  BitReader(const uint8_t* array, size_t len) : BitReader(default_context(), array, len) { mu_ = &default_context_mutex(); }
  BitReader(Context& ctx, const uint8_t* array, size_t len) {
    MaybeLock lk(&ctx == &default_context() ? &default_context_mutex() : nullptr);
    if (x3_bitreader_new(ctx.raw(), array, len, &br_)) throw std::runtime_error("x3::bitreader::BitReader: x3_bitreader_new failed");
  }
  BitReader(const BitReader&) = delete;
  BitReader& operator=(const BitReader&) = delete;
  ~BitReader() { x3_bitreader_free(br_); }
  void inc_bits(size_t n) {
    MaybeLock lk(mu_);
    check(x3_bitreader_inc_bits(br_, (uint32_t)n));
  }
  uint32_t read_nbits(size_t n) {
    MaybeLock lk(mu_);
    uint32_t v = 0;
    check(x3_bitreader_read_nbits(br_, (uint32_t)n, &v));
    return v;
  }
  size_t count_zero_bits() {
    MaybeLock lk(mu_);
    uint32_t v = 0;
    check(x3_bitreader_count_zero_bits(br_, &v));
    return v;
  }
  x3_bitreader* raw() { return br_; }
  std::mutex* mutex() { return mu_; }

 private:
  static void check(int rc) {
    if (rc) throw std::runtime_error(std::string("x3::bitreader::BitReader: ") + x3_strerror(rc));
  }
  x3_bitreader* br_ = nullptr;
  std::mutex* mu_ = nullptr;
};
}  // namespace bitreader

namespace encoder {
using bytewriter::ByteWriter;
using bytewriter::SliceByteWriter;

// encoder.rs:122-162
inline void write_frame_header(size_t num_samples, uint8_t id, size_t payload_len, uint16_t payload_crc,
                               uint8_t (&out)[FrameHeader::LENGTH]) {
  x3_write_frame_header(num_samples, id, payload_len, payload_crc, out);
}

namespace detail {
// the reference prints this block after encode() when built with std (encoder.rs:96-108)
inline void print_stats(const uint64_t (&stats)[6]) {
  float t = (float)(stats[0] + stats[1] + stats[2] + stats[3] + stats[4] + stats[5]);
  std::printf("\nStatistics:\n  Rice-0: %.4f%%\n  Rice-1: %.4f%%\n  Rice-2: %.4f%%\n  Rice-3: %.4f%%\n  BFP: %.4f%%\n"
              "  Pass-through %.4f%%\n\n",
              stats[0] / t * 100.0f, stats[1] / t * 100.0f, stats[2] / t * 100.0f, stats[3] / t * 100.0f,
              stats[4] / t * 100.0f, stats[5] / t * 100.0f);
}

inline X3Error encode_samples(Context& ctx, const int16_t* wav, size_t n, size_t n_channels, const Parameters& params,
                              ByteWriter& writer, bool one_frame, uint64_t (&stats)[6]) {
  x3_params c = params.c_params();
  uint64_t pos = 0;
  if (auto* sw = dynamic_cast<SliceByteWriter*>(&writer)) {  // write straight into the caller's slice
    int rc = one_frame ? x3_encode_frame(ctx.raw(), wav, n, &c, sw->data(), sw->capacity(), sw->position(), &pos, stats)
                       : x3_encode(ctx.raw(), wav, n, (uint32_t)n_channels, &c, sw->data(), sw->capacity(),
                                   sw->position(), &pos, stats);
    // (on ByteWriterInsufficientMemory too: the slice holds every frame that fits and *out_pos stands behind the last of
    // them -- include/x3hip.h, x3_encode -- and so must the writer, as the reference's SliceByteWriter does after the frames
    // it has taken: src/bytewriter.rs:86-99)
    if (rc == 0 || rc == static_cast<int>(X3Error::ByteWriterInsufficientMemory)) sw->advance_to((size_t)pos);
    return static_cast<X3Error>(rc);
  }
  uint64_t start = 0;
  writer.stream_position(&start);
  const uint64_t parity = start & 1;  // only the parity of the absolute position matters (encoder.rs:182)
  std::vector<uint8_t> buf((size_t)(parity + x3_encode_bound(n, &c) + 64 + 3 * (one_frame ? n : 0)));
  int rc = one_frame ? x3_encode_frame(ctx.raw(), wav, n, &c, buf.data(), buf.size(), parity, &pos, stats)
                     : x3_encode(ctx.raw(), wav, n, (uint32_t)n_channels, &c, buf.data(), buf.size(), parity, &pos, stats);
  if (rc) return static_cast<X3Error>(rc);
  return writer.write_all(buf.data() + parity, (size_t)(pos - parity));
}
}  // namespace detail

// encoder::encode over slice channels (README shape): channels.len() > 1 -> MoreThanOneChannel (encoder.rs:55-57)
inline X3Error encode(Context& ctx, const Channel* const* channels, size_t n_channels, ByteWriter& writer,
                      bool print_statistics = false) {
  if (n_channels > 1) return X3Error::MoreThanOneChannel;
  if (n_channels == 0) return X3Error::BadArg;
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
  const Channel& ch = *channels[0];
  X3Error e = detail::encode_samples(ctx, ch.wav, ch.len, n_channels, ch.params, writer, false, stats);
  if (e == X3Error::Ok && print_statistics) detail::print_stats(stats);
  return e;
}

// encoder::encode over iterator channels (encoder.rs:51-54): the iterator is collected, dispatched, written
template <class It>
inline X3Error encode(Context& ctx, IterChannel<It>* const* channels, size_t n_channels, ByteWriter& writer,
                      bool print_statistics = false) {
  if (n_channels > 1) return X3Error::MoreThanOneChannel;
  if (n_channels == 0) return X3Error::BadArg;
  std::vector<int16_t> wav(channels[0]->wav, channels[0]->wav_end);
  channels[0]->wav = channels[0]->wav_end;  // the reference consumes the iterator
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
  X3Error e = detail::encode_samples(ctx, wav.data(), wav.size(), n_channels, channels[0]->params, writer, false, stats);
  if (e == X3Error::Ok && print_statistics) detail::print_stats(stats);
  return e;
}

// encoder::encode_frame (encoder.rs:175-214)
inline X3Error encode_frame(Context& ctx, const int16_t* wav, size_t n, ByteWriter& writer, const Parameters& params,
                            uint64_t (&stats)[6]) {
  uint64_t st[6] = {0, 0, 0, 0, 0, 0};
  X3Error e = detail::encode_samples(ctx, wav, n, 1, params, writer, true, st);
  if (e == X3Error::Ok)
    for (int i = 0; i < 6; ++i) stats[i] += st[i];
  return e;
}

// the reference's own argument lists (encoder.rs:51, :175): no context, statistics printed as the `std` build does
inline X3Error encode(const Channel* const* channels, size_t n_channels, ByteWriter& writer) {
  X3_WITH_DEFAULT_CONTEXT(encode(ctx, channels, n_channels, writer, true));
}
template <class It>
inline X3Error encode(IterChannel<It>* const* channels, size_t n_channels, ByteWriter& writer) {
  X3_WITH_DEFAULT_CONTEXT(encode(ctx, channels, n_channels, writer, true));
}
inline X3Error encode_frame(const int16_t* wav, size_t n, ByteWriter& writer, const Parameters& params, uint64_t (&stats)[6]) {
  X3_WITH_DEFAULT_CONTEXT(encode_frame(ctx, wav, n, writer, params, stats));
}
}  // namespace encoder

namespace decoder {
// decoder.rs:69-118
inline X3Error read_frame_header(const uint8_t* bytes, size_t len, FrameHeader* out) {
  x3_frame_header h;
  int rc = x3_read_frame_header(bytes, len, &h);
  if (rc) return static_cast<X3Error>(rc);
  out->source_id = h.source_id;
  out->samples = h.samples;
  out->channels = h.channels;
  out->payload_len = h.payload_len;
  out->payload_crc = h.payload_crc;
  return X3Error::Ok;
}

// decoder.rs:36-58: returns the number of samples written in *n_out (the reference's Some(p_wav))
inline X3Error decode_frame(Context& ctx, const uint8_t* x3_bytes, size_t len, int16_t* wav_buf, size_t wav_cap,
                            const Parameters& params, size_t samples, size_t* n_out) {
  x3_params c = params.c_params();
  uint64_t n = 0;
  int rc = x3_decode_frame(ctx.raw(), x3_bytes, len, wav_buf, wav_cap, &c, samples, &n);
  if (n_out) *n_out = (size_t)n;
  return static_cast<X3Error>(rc);
}

inline X3Error decode_frame(const uint8_t* x3_bytes, size_t len, int16_t* wav_buf, size_t wav_cap, const Parameters& params,
                            size_t samples, size_t* n_out) {
  X3_WITH_DEFAULT_CONTEXT(decode_frame(ctx, x3_bytes, len, wav_buf, wav_cap, params, samples, n_out));
}

// Not in the reference: announce the frame stream a loop over decode_frame is about to walk (x3_decode_prefetch): the
// calls are then served from windows decoded ahead instead of one dispatch each.  nullptr drops the announcement; the
// buffer must stay unchanged while it stands.
inline X3Error prefetch(Context& ctx, const uint8_t* x3, size_t len, const Parameters& params) {
  x3_params c = params.c_params();
  return static_cast<X3Error>(x3_decode_prefetch(ctx.raw(), x3, len, &c));
}
inline X3Error prefetch(const uint8_t* x3, size_t len, const Parameters& params) {
  X3_WITH_DEFAULT_CONTEXT(prefetch(ctx, x3, len, params));
}

// decoder.rs:132-145: one block of wav_len samples from the reader's position; *last_wav is read and updated
inline X3Error decode_block(bitreader::BitReader& br, int16_t* wav, size_t wav_len, int16_t* last_wav, const Parameters& params) {
  MaybeLock lk(br.mutex());
  x3_params c = params.c_params();
  return static_cast<X3Error>(x3_decode_block(br.raw(), wav, (uint32_t)wav_len, last_wav, &c));
}

// the X3aReader::decode_next_frame loop (decodefile.rs:105-136, 200-209) over an in-memory frame stream
struct StreamResult {
  uint64_t samples = 0, frames_ok = 0, frame_errors = 0;
};
inline X3Error decode_stream(Context& ctx, const uint8_t* x3, size_t len, const Parameters& params, int16_t* wav,
                             size_t wav_cap, StreamResult* res) {
  x3_params c = params.c_params();
  StreamResult r;
  int rc = x3_decode_stream(ctx.raw(), x3, len, &c, wav, wav_cap, &r.samples, &r.frames_ok, &r.frame_errors);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
inline X3Error decode_stream(const uint8_t* x3, size_t len, const Parameters& params, int16_t* wav, size_t wav_cap,
                             StreamResult* res) {
  X3_WITH_DEFAULT_CONTEXT(decode_stream(ctx, x3, len, params, wav, wav_cap, res));
}
// the same walk for a stream that is already in HBM: frame index and decode on the device (x3_index_dev)
inline X3Error decode_stream_dev(Context& ctx, const uint8_t* d_x3, size_t len, const Parameters& params, int16_t* d_wav,
                                 size_t wav_cap, StreamResult* res) {
  x3_params c = params.c_params();
  StreamResult r;
  int rc = x3_decode_stream_dev(ctx.raw(), d_x3, len, &c, d_wav, wav_cap, &r.samples, &r.frames_ok, &r.frame_errors);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
}  // namespace decoder

// Device-resident encode / decode (NOT in the crate, which knows no device): samples and stream stay in HBM between the two
// (x3_encode_dev / x3_decode_dev), optionally with the SEGMENT INDEX that lets a short stream decode on as many lanes as fill
// the GPU (x3_encode_dev_seg / x3_decode_dev_seg; the index is a hint the decoder proves entry by entry).
namespace device {
// device memory of a context (x3_dev_alloc): movable, freed with the object
class Buffer {
 public:
  Buffer() = default;
  Buffer(Context& ctx, size_t bytes) : ctx_(&ctx), bytes_(bytes) {
    if (x3_dev_alloc(ctx.raw(), bytes, &p_) != X3_OK) { p_ = nullptr; bytes_ = 0; }
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { reset(); ctx_ = o.ctx_; p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
    return *this;
  }
  ~Buffer() { reset(); }
  void reset() { if (p_) x3_dev_free(ctx_->raw(), p_); p_ = nullptr; bytes_ = 0; }
  bool ok() const { return p_ != nullptr; }
  size_t size() const { return bytes_; }
  void* data() const { return p_; }
  template <typename T> T* as() const { return static_cast<T*>(p_); }
  X3Error upload(const void* src, size_t bytes) {
    return bytes <= bytes_ ? static_cast<X3Error>(x3_dev_upload(ctx_->raw(), p_, src, bytes)) : X3Error::BadArg;
  }
  X3Error download(void* dst, size_t bytes) const {
    return bytes <= bytes_ ? static_cast<X3Error>(x3_dev_download(ctx_->raw(), dst, p_, bytes)) : X3Error::BadArg;
  }

 private:
  Context* ctx_ = nullptr;
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// an encoded batch in device memory: the stream, where its frames begin, and (seg_blocks != 0) the segment index
struct EncodedStream {
  Buffer bytes, frame_offsets, seg_index;
  size_t len = 0;          // bytes of the stream
  size_t n_frames = 0;
  size_t n_per_clip = 0, n_clips = 1;
  uint32_t seg_blocks = 0;
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
};

// n_clips clips of n_per_clip samples each, back to back in d_wav, each encoded like encoder::encode encodes a channel.
// seg_blocks: 0 = no index; a power of two >= 4 (32 for the default 500-block frames) = also leave the segment index.
inline X3Error encode(Context& ctx, const int16_t* d_wav, size_t n_per_clip, size_t n_clips, const Parameters& params,
                      uint32_t seg_blocks, EncodedStream* out) {
  if (!out || !d_wav || n_per_clip == 0 || n_clips == 0) return X3Error::BadArg;
  const x3_params c = params.c_params();
  EncodedStream e;
  e.n_per_clip = n_per_clip;
  e.n_clips = n_clips;
  e.n_frames = static_cast<size_t>(x3_num_frames(n_per_clip, &c)) * n_clips;
  const size_t cap = static_cast<size_t>(x3_encode_bound(n_per_clip, &c)) * n_clips;
  e.bytes = Buffer(ctx, cap + 16);
  e.frame_offsets = Buffer(ctx, 8 * (e.n_frames + 1));
  const uint64_t n_idx = seg_blocks ? x3_seg_index_entries(e.n_frames, &c, seg_blocks) : 0;
  if (n_idx) {
    e.seg_index = Buffer(ctx, 8 * n_idx);
    e.seg_blocks = seg_blocks;
  }
  if (!e.bytes.ok() || !e.frame_offsets.ok() || (n_idx && !e.seg_index.ok())) return X3Error::Hip;
  const x3_batch b{n_per_clip, n_per_clip, n_clips};
  int rc = n_idx ? x3_encode_dev_seg(ctx.raw(), d_wav, &b, &c, e.bytes.as<uint8_t>(), cap, 0, e.frame_offsets.as<uint64_t>(),
                                     e.seg_index.as<uint64_t>(), seg_blocks)
                 : x3_encode_dev(ctx.raw(), d_wav, &b, &c, e.bytes.as<uint8_t>(), cap, 0, e.frame_offsets.as<uint64_t>());
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  uint64_t pos = 0;
  rc = x3_encode_result(ctx.raw(), &pos, e.stats);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  e.len = static_cast<size_t>(pos);
  *out = std::move(e);
  return X3Error::Ok;
}

// ... and back: the samples of every clip at d_wav + clip * n_per_clip.  By the segment index when the stream has one.
// res->frames_ok = the first frame that failed (n_frames if none), frame_errors = its status.
inline X3Error decode(Context& ctx, const EncodedStream& s, const Parameters& params, int16_t* d_wav, size_t wav_cap,
                      decoder::StreamResult* res) {
  if (!d_wav || !s.bytes.ok() || !s.frame_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  const x3_batch b{s.n_per_clip, s.n_per_clip, s.n_clips};
  int rc = s.seg_blocks ? x3_decode_dev_seg(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(), s.n_frames, &b,
                                            nullptr, &c, d_wav, wav_cap, nullptr, s.seg_index.as<uint64_t>(), s.seg_blocks, 0)
                        : x3_decode_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(), s.n_frames, &b,
                                        nullptr, &c, d_wav, wav_cap, nullptr);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  uint64_t first_bad = 0, before = 0;
  int st = 0;
  rc = x3_decode_result(ctx.raw(), &first_bad, &st, &before);
  if (res) { res->samples = before; res->frames_ok = first_bad; res->frame_errors = static_cast<uint64_t>(st); }
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  return static_cast<X3Error>(st);
}

// The segment index of a stream somebody else wrote (x3_seg_index_build_dev): a walk that stores no sample, for any block
// length, frame length and code set.  d_frame_offsets: n_frames byte offsets into d_x3.  *out stays empty where seg_blocks
// leaves a frame one stretch.  Asynchronous; the index is only ever a hint and serves the window paths.
inline X3Error build_seg_index(Context& ctx, const uint8_t* d_x3, uint64_t x3_len, const uint64_t* d_frame_offsets,
                               uint64_t n_frames, const Parameters& params, uint32_t seg_blocks, Buffer* out) {
  if (!out) return X3Error::BadArg;
  const x3_params c = params.c_params();
  const uint64_t n_idx = seg_blocks ? x3_seg_index_entries(n_frames, &c, seg_blocks) : 0;
  *out = Buffer();
  if (!n_idx) return X3Error::Ok;
  Buffer idx(ctx, 8 * n_idx);
  if (!idx.ok()) return X3Error::Hip;
  const int rc = x3_seg_index_build_dev(ctx.raw(), d_x3, x3_len, d_frame_offsets, n_frames, &c, idx.as<uint64_t>(), seg_blocks);
  if (rc == X3_OK) *out = std::move(idx);
  return static_cast<X3Error>(rc);
}
// ... for a stream that has none (another encoder's, a block length the encoder does not index): decode_windows then
// decodes by it
inline X3Error index_by_walk(Context& ctx, EncodedStream* s, const Parameters& params, uint32_t seg_blocks) {
  if (!s || !s->bytes.ok() || !s->frame_offsets.ok()) return X3Error::BadArg;
  const X3Error rc = build_seg_index(ctx, s->bytes.as<uint8_t>(), s->len, s->frame_offsets.as<uint64_t>(), s->n_frames, params,
                                     seg_blocks, &s->seg_index);
  s->seg_blocks = rc == X3Error::Ok && s->seg_index.ok() ? seg_blocks : 0;
  return rc;
}

// Random access (x3_decode_windows_dev): n_windows windows of window_len samples, window w = positions [d_starts[w], d_starts[w] +
// window_len) of the stream, as rows of d_out (X3_WINDOW_I16 / X3_WINDOW_F32); d_status[w] = 0 or the first failing covering
// frame's status.  The stream's sample offsets are made once (sample_offsets); the segment index, where the stream has one,
// is the hint the stretches start from.  Waits for the call: res = windows with status != 0, the first, its status.
struct WindowsResult {
  uint64_t n_bad = 0, first_bad = 0;
  int first_bad_status = 0;
};
inline X3Error sample_offsets(Context& ctx, const EncodedStream& s, Buffer* d_sample_offsets) {
  if (!d_sample_offsets || !s.bytes.ok() || !s.frame_offsets.ok()) return X3Error::BadArg;
  *d_sample_offsets = Buffer(ctx, 8 * (s.n_frames + 1));
  if (!d_sample_offsets->ok()) return X3Error::Hip;
  return static_cast<X3Error>(x3_sample_offsets_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(),
                                                    s.n_frames, d_sample_offsets->as<uint64_t>()));
}
inline X3Error decode_windows(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                              const uint64_t* d_starts, size_t n_windows, uint32_t window_len, void* d_out, int out_format,
                              int32_t* d_status, WindowsResult* res) {
  if (!s.bytes.ok() || !s.frame_offsets.ok() || !d_sample_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  int rc = x3_decode_windows_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(),
                                 d_sample_offsets.as<uint64_t>(), s.n_frames, &c,
                                 s.seg_blocks ? s.seg_index.as<uint64_t>() : nullptr, s.seg_blocks, d_starts, n_windows,
                                 window_len, d_out, out_format, d_status);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  WindowsResult r;
  rc = x3_decode_windows_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}

// Ranges (x3_decode_ranges_dev): windows with a length each, range w = positions [d_starts[w], d_starts[w] + d_lens[w]).
// row_stride 0: rows packed at the exclusive sum of all lengths, written to d_out_offsets (n_ranges + 1 words, required); a
// range without room in out_cap samples is BadArg and not written.  row_stride > 0: row w at w * row_stride with zeros
// behind its length (d_out_offsets may be nullptr).  Row and status of a range are the single window's of that length.
// Waits for the call: res = ranges with status != 0, the first, its status, and the sum of all lengths.
struct RangesResult : WindowsResult {
  uint64_t total_samples = 0;
};
inline X3Error decode_ranges(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                             const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, uint64_t row_stride, void* d_out,
                             uint64_t out_cap, int out_format, uint64_t* d_out_offsets, int32_t* d_status, RangesResult* res) {
  if (!s.bytes.ok() || !s.frame_offsets.ok() || !d_sample_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  int rc = x3_decode_ranges_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(),
                                d_sample_offsets.as<uint64_t>(), s.n_frames, &c,
                                s.seg_blocks ? s.seg_index.as<uint64_t>() : nullptr, s.seg_blocks, d_starts, d_lens, n_ranges,
                                row_stride, d_out, out_cap, out_format, d_out_offsets, d_status);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  RangesResult r;
  rc = x3_decode_ranges_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status, &r.total_samples);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}

struct RangeLevelsResult : WindowsResult {   // (device::range_levels, below)
  uint64_t total_rows = 0;
};

namespace detail {
// the second half of every levels and range-levels wrapper: rc is the call's; on X3_OK waits for its result into *res
inline X3Error levels_result(Context& ctx, int rc, WindowsResult* res) {
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  WindowsResult r;
  rc = x3_levels_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
inline X3Error levels_result(Context& ctx, int rc, RangeLevelsResult* res) {
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  RangeLevelsResult r;
  rc = x3_range_levels_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status, &r.total_rows);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
// the stream forms: call(the nine arguments every stream entry point begins with) -> rc, then levels_result
template <class Result, class Call>
X3Error stream_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets, Result* res,
                      Call call) {
  if (!s.bytes.ok() || !s.frame_offsets.ok() || !d_sample_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  return levels_result(ctx,
                       call(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(), d_sample_offsets.as<uint64_t>(),
                            s.n_frames, &c, s.seg_blocks ? s.seg_index.as<uint64_t>() : nullptr, s.seg_blocks),
                       res);
}
}   // namespace detail

// Levels (x3_levels_dev): min, max, count, sum and sum of squares of the samples per bin of bin_len positions (0: one bin),
// n_bins records in d_levels, every one written; d_frame_status (n_frames int32, may be nullptr): a frame with a status
// other than 0 adds nothing.  No sample buffer.  Waits for the call: res = frames with status != 0, the first, its status.
// signal (x3_signal_levels_dev): the samples, or their first difference clamped to 16 bits -- x[i] - x[i-1] at the position
// of sample i, across the seam of two frames that both have status 0; the first sample of a stream or entry adds nothing.
enum class LevelSignal : int { Samples = X3_LEVEL_SIGNAL_SAMPLES, Diff = X3_LEVEL_SIGNAL_DIFF };

inline X3Error levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                      uint64_t bin_len, x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, WindowsResult* res,
                      LevelSignal signal = LevelSignal::Samples) {
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_signal_levels_dev(st..., bin_len, d_levels, n_bins, d_frame_status, static_cast<int>(signal));
  });
}

// An integer FIR filter in front of the levels (x3_fir_levels_dev): y[i] = clamp((sum over t of taps[t] * x[i - t]) >> shift,
// 16 bits), counted where all taps.size() positions lie in frames with status 0 of the same stream or entry.  1 .. 8 taps with
// sum |taps| <= 32768 and shift 0 .. 15: anything else is BadArg at the call.  {1} gives the levels, {1, -1} LevelSignal::Diff.
struct Fir {
  std::vector<int16_t> taps;
  uint32_t shift = 0;
  x3_level_fir c_fir() const {   // (more than 8 taps: n_taps says so and the call refuses it)
    x3_level_fir f{};
    f.n_taps = static_cast<uint32_t>(taps.size());
    f.shift = shift;
    for (size_t t = 0; t < taps.size() && t < 8; ++t) f.taps[t] = taps[t];
    return f;
  }
};

inline X3Error levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                      uint64_t bin_len, x3_level* d_levels, uint64_t n_bins, int32_t* d_frame_status, WindowsResult* res,
                      const Fir& fir) {
  const x3_level_fir f = fir.c_fir();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_fir_levels_dev(st..., bin_len, d_levels, n_bins, d_frame_status, &f);
  });
}

// One oscillator in front of the levels (x3_level_tone): position i has the phase (i * step) mod 2^32, and a bin's record
// (x3_tone_level) holds re and im, the sums of sample times cos and sin of the phase's table pair, and the samples' min, max
// and n.  d_table: 1 024 (cos, sin) int16 pairs in device memory, the caller's, alive until the call has run; usual_table()
// is the one the Python mirror supplies.  step = round(f / fs * 2^32) puts the oscillator at f.
struct Tone {
  uint32_t step = 0;
  const int16_t* d_table = nullptr;
  x3_level_tone c_tone() const { return x3_level_tone{step, 0, d_table}; }
  static std::vector<int16_t> usual_table() {   // (round(32767 cos(2 pi k / 1024)), round(32767 sin(2 pi k / 1024))) at pair k
    std::vector<int16_t> t(2048);
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < 1024; ++k) {
      t[2 * k] = static_cast<int16_t>(std::lround(32767.0 * std::cos(two_pi * k / 1024.0)));
      t[2 * k + 1] = static_cast<int16_t>(std::lround(32767.0 * std::sin(two_pi * k / 1024.0)));
    }
    return t;
  }
};

// Tone levels (x3_tone_levels_dev): device::levels' arguments with tone records and a Tone.  Waits for the call.
inline X3Error tone_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                           uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_bins, int32_t* d_frame_status,
                           WindowsResult* res, const Tone& tone) {
  const x3_level_tone t = tone.c_tone();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_tone_levels_dev(st..., bin_len, d_levels, n_bins, d_frame_status, &t);
  });
}

// Up to X3_TONE_BANK_MAX oscillators against one table in one pass (x3_level_tone_bank): plane t of the records is what
// tone_levels writes for Tone{steps[t], d_table}.
struct ToneBank {
  std::vector<uint32_t> steps;   // 1 .. X3_TONE_BANK_MAX
  const int16_t* d_table = nullptr;
  bool ok() const { return !steps.empty() && steps.size() <= X3_TONE_BANK_MAX; }
  x3_level_tone_bank c_bank() const {   // (ok() only)
    x3_level_tone_bank b{static_cast<uint32_t>(steps.size()), 0, d_table, {0}};
    for (size_t t = 0; t < steps.size(); ++t) b.steps[t] = steps[t];
    return b;
  }
};

// Tone bank levels (x3_tone_bank_levels_dev): tone_levels' arguments with bank.steps.size() planes of n_bins records in
// d_levels, plane t at d_levels + t * n_bins.  All planes go through tone_power_levels at once.  Waits for the call.
inline X3Error tone_bank_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                                uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_bins, int32_t* d_frame_status,
                                WindowsResult* res, const ToneBank& bank) {
  if (!bank.ok()) return X3Error::BadArg;
  const x3_level_tone_bank b = bank.c_bank();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_tone_bank_levels_dev(st..., bin_len, d_levels, n_bins, d_frame_status, &b);
  });
}

// The adapter into the chain (x3_tone_power_levels_dev): n_rows tone records -> the level records of the band, which
// device::events and the quantiles calls take; d_levels may be d_tone's bytes (in place).  Asynchronous on the context's
// stream: the calls behind it are ordered after it.
inline X3Error tone_power_levels(Context& ctx, const x3_tone_level* d_tone, uint64_t n_rows, x3_level* d_levels) {
  return static_cast<X3Error>(x3_tone_power_levels_dev(ctx.raw(), d_tone, n_rows, d_levels));
}

// Events (x3_events_dev): the runs of hot bins of n_bins level records (as device::levels writes them; bins of bin_len
// positions) under `rule`, as cap slots of (d_starts, d_lens, d_event_levels or nullptr); d_count receives the number found,
// which may exceed cap; every slot behind the events is a zero-length range, so the arrays go to device::decode_ranges with
// n_ranges = cap as they are.  d_total: device pointer to the stream's sample count (the last word of the sample offsets).
// Waits for the call: *count = the events found.
inline X3Error events(Context& ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                      const x3_event_rule& rule, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels, uint64_t cap,
                      uint64_t* d_count, uint64_t* count) {
  int rc = x3_events_dev(ctx.raw(), d_levels, n_bins, bin_len, d_total, &rule, d_starts, d_lens, d_event_levels, cap, d_count);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
}

// Level quantiles (x3_level_quantiles_dev): the quantiles q_ppm (millionths, 1 .. 8 of them, host array) of the keys
// (X3_LEVEL_KEY_PEAK: max(max, -min); X3_LEVEL_KEY_MEAN_SQ: floor(sum_sq / n)) of the counting rows of n_bins level records
// into d_values (uint32, q_ppm.size() words) and their number into d_counted (one uint32); value j is
// sorted(keys)[(K - 1) * q_ppm[j] / 1000000], 0 when K == 0.  Waits for the call: res = entries without a counting row and
// the first of them (the entry count if none).
struct QuantilesResult {
  uint64_t n_empty = 0, first_empty = 0;
};
inline X3Error level_quantiles(Context& ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                               int key, const std::vector<uint32_t>& q_ppm, uint32_t* d_values, uint32_t* d_counted,
                               QuantilesResult* res) {
  int rc = x3_level_quantiles_dev(ctx.raw(), d_levels, n_bins, bin_len, d_total, key, q_ppm.data(), (uint32_t)q_ppm.size(), d_values,
                                  d_counted);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  QuantilesResult r;
  rc = x3_level_quantiles_result(ctx.raw(), &r.n_empty, &r.first_empty);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}

// Thresholds from quantiles (x3_level_thresholds_dev): one x3_event_threshold at d_thr, per criterion of `rule` that is on
// clamp(floor(quantile * mul / div) + add, 1, limit), 0 for one that is off or without a counting row.  Waits for the call.
inline X3Error level_thresholds(Context& ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                                const x3_threshold_rule& rule, x3_event_threshold* d_thr, QuantilesResult* res) {
  int rc = x3_level_thresholds_dev(ctx.raw(), d_levels, n_bins, bin_len, d_total, &rule, d_thr);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  QuantilesResult r;
  rc = x3_level_quantiles_result(ctx.raw(), &r.n_empty, &r.first_empty);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}

// Events with the rule's two values (both 0 in `rule`) taken from the record at d_thr (x3_events_adaptive_dev); otherwise as
// device::events.  Waits for the call.
inline X3Error events_adaptive(Context& ctx, const x3_level* d_levels, uint64_t n_bins, uint64_t bin_len, const uint64_t* d_total,
                               const x3_event_rule& rule, const x3_event_threshold* d_thr, uint64_t* d_starts, uint32_t* d_lens,
                               x3_level* d_event_levels, uint64_t cap, uint64_t* d_count, uint64_t* count) {
  int rc = x3_events_adaptive_dev(ctx.raw(), d_levels, n_bins, bin_len, d_total, &rule, d_thr, d_starts, d_lens, d_event_levels, cap,
                                  d_count);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
}

// The rule of plane_events (x3_plane_event_rule): a row is hot when at least min_planes planes are loud at it, plane t under
// mean_sq_min[t] and peak_min[t] (0: off; both empty: the values come from d_thr); the other four as in x3_event_rule.
// planes: the number of planes when there are no values.
struct PlaneEventRule {
  std::vector<uint64_t> mean_sq_min;
  std::vector<uint32_t> peak_min;
  uint32_t min_planes = 1, join_bins = 0, min_bins = 0, pad_bins = 0, max_bins = 0, planes = 0;
  size_t n_planes() const {
    const size_t k = mean_sq_min.size() > peak_min.size() ? mean_sq_min.size() : peak_min.size();
    return k > planes ? k : planes;
  }
  bool ok() const {
    const size_t k = n_planes();
    return k >= 1 && k <= X3_EVENT_PLANES_MAX && (mean_sq_min.empty() || mean_sq_min.size() == k) &&
           (peak_min.empty() || peak_min.size() == k);
  }
  x3_plane_event_rule c_rule() const {
    x3_plane_event_rule r{};
    r.n_planes = (uint32_t)n_planes();
    r.min_planes = min_planes;
    r.join_bins = join_bins;
    r.min_bins = min_bins;
    r.pad_bins = pad_bins;
    r.max_bins = max_bins;
    for (size_t t = 0; t < mean_sq_min.size() && t < X3_EVENT_PLANES_MAX; ++t) r.mean_sq_min[t] = mean_sq_min[t];
    for (size_t t = 0; t < peak_min.size() && t < X3_EVENT_PLANES_MAX; ++t) r.peak_min[t] = peak_min[t];
    return r;
  }
};

// Plane events (x3_plane_events_dev): the events of the rows that are loud in at least rule.min_planes of the rule's planes
// of n_bins level records, plane t at d_levels + t * plane_stride records (what device::tone_bank_levels and
// tone_power_levels over all planes write with plane_stride = n_bins).  d_thr: nullptr, or one x3_event_threshold per plane
// and a rule without values.  Beside device::events' outputs: d_event_planes (uint32, cap elements, or nullptr): bit t set
// when plane t is loud in the event; d_event_levels (or nullptr): a plane of cap merged records per plane.  Waits for the
// call: *count = the events found.
inline X3Error plane_events(Context& ctx, const x3_level* d_levels, uint64_t plane_stride, uint64_t n_bins, uint64_t bin_len,
                            const uint64_t* d_total, const PlaneEventRule& rule, const x3_event_threshold* d_thr,
                            uint64_t* d_starts, uint32_t* d_lens, uint32_t* d_event_planes, x3_level* d_event_levels, uint64_t cap,
                            uint64_t* d_count, uint64_t* count) {
  if (!rule.ok()) return X3Error::BadArg;
  const x3_plane_event_rule r = rule.c_rule();
  int rc = x3_plane_events_dev(ctx.raw(), d_levels, plane_stride, n_bins, bin_len, d_total, &r, d_thr, d_starts, d_lens,
                               d_event_planes, d_event_levels, cap, d_count);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
}

// Range levels (x3_range_levels_dev): the x3_level records of range w = positions [d_starts[w], d_starts[w] + d_lens[w]), bins
// of bin_len positions counted from the range's own start (0: one bin), max(1, ceil(len / bin_len)) rows each; a frame with a
// status other than 0 adds nothing and gives the range its status.  row_stride 0: rows packed at the exclusive sum of all row
// counts, written to d_row_offsets (n_ranges + 1 words, required); a range without room in rows_cap records is BadArg and not
// written.  row_stride > 0: range w at w * row_stride with identities behind its rows (d_row_offsets may be nullptr).  The
// arrays device::events wrote go in as they are.  Waits for the call: res = ranges with status != 0, the first, its status,
// and the sum of all row counts.  signal (x3_signal_range_levels_dev): LevelSignal::Diff gives the records of the stream's
// first difference cut to the ranges -- the difference at a range's first position counts, statuses are the Samples form's.
inline X3Error range_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                            const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, uint64_t bin_len,
                            uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                            RangeLevelsResult* res, LevelSignal signal = LevelSignal::Samples) {
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_signal_range_levels_dev(st..., d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                                      d_status, static_cast<int>(signal));
  });
}
// FIR range levels (x3_fir_range_levels_dev): range_levels of the stream's FIR signal (device::levels with a Fir) cut to the
// ranges -- the call cuts the filtered stream, it does not filter the cut: a range's first T - 1 positions count, their
// earlier samples lie in front of the range; statuses are the Samples form's.  An invalid fir is BadArg.
inline X3Error fir_range_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                                const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, uint64_t bin_len,
                                uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                int32_t* d_status, const Fir& fir, RangeLevelsResult* res) {
  const x3_level_fir f = fir.c_fir();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_fir_range_levels_dev(st..., d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                                   d_status, &f);
  });
}
// Tone range levels (x3_tone_range_levels_dev): range_levels with tone records, the stream's tone signal (device::tone_levels)
// cut to the ranges -- the call cuts the stream's signal, it does not restart the oscillator: position i of the stream has the
// phase (i * step) mod 2^32 wherever the range begins, so compare band power (tone_power_levels), not raw sums, across
// ranges; statuses are the Samples form's.  A Tone without a table is BadArg.  Packed or padded, the records go through
// tone_power_levels unchanged.
inline X3Error tone_range_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                                 const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, uint64_t bin_len,
                                 uint64_t row_stride, x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                 int32_t* d_status, const Tone& tone, RangeLevelsResult* res) {
  const x3_level_tone t = tone.c_tone();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_tone_range_levels_dev(st..., d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap, d_row_offsets,
                                    d_status, &t);
  });
}
// Tone bank range levels (x3_tone_bank_range_levels_dev): tone_range_levels for every step of the bank from one decode of the
// covering frames.  d_levels holds bank.steps.size() planes of rows_cap records, plane t at d_levels + t * rows_cap what
// tone_range_levels writes for Tone{steps[t], d_table}; row offsets, statuses and the result exist once (total_rows is one
// plane's).  Records the call does not write stay untouched in every plane; where every record is defined, all planes go
// through tone_power_levels at once.  Waits for the call.
inline X3Error tone_bank_range_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                                      const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, uint64_t bin_len,
                                      uint64_t row_stride, x3_tone_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                      int32_t* d_status, const ToneBank& bank, RangeLevelsResult* res) {
  if (!bank.ok()) return X3Error::BadArg;
  const x3_level_tone_bank b = bank.c_bank();
  return detail::stream_levels(ctx, s, params, d_sample_offsets, res, [&](auto... st) {
    return x3_tone_bank_range_levels_dev(st..., d_starts, d_lens, n_ranges, bin_len, row_stride, d_levels, rows_cap,
                                         d_row_offsets, d_status, &b);
  });
}

// The rule of spectra_rows (x3_spectra_rule): n_fft in {64, 128, 256, 512, 1024}, hop 1 .. 2^31 - 1, power: rows of uint32
// band powers (X3_SPECTRA_POWER) or of (re, im) int64 pairs (X3_SPECTRA_SUMS); d_table: a device table of 1 024 (cos, sin)
// int16 pairs, Tone's.  bins() = n_fft / 2 + 1 words or pairs a row; rows(len) = the whole frames of a row of len samples.
struct SpectraRule {
  uint32_t n_fft = 256, hop = 256;
  bool power = true;
  const int16_t* d_table = nullptr;
  uint32_t bins() const { return n_fft / 2 + 1; }
  uint64_t rows(uint64_t len) const { return len < n_fft || !hop ? 0 : (len - n_fft) / hop + 1; }
  x3_spectra_rule c_rule() const {
    x3_spectra_rule r{};
    r.n_fft = n_fft, r.hop = hop, r.format = power ? X3_SPECTRA_POWER : X3_SPECTRA_SUMS, r.d_table = d_table;
    return r;
  }
};
struct SpectraResult : WindowsResult {
  uint64_t total_rows = 0;
};
// Spectra (x3_spectra_rows_dev): the exact integer STFT of the int16 rows d_lens[w] samples at d_samples + d_offsets[w], as
// decode_ranges wrote them (d_in_status: its statuses or nullptr; may equal d_status).  The oscillator restarts at every
// frame.  row_stride 0: range w's rows packed at d_row_offsets[w] (n_ranges + 1 words, required), a range without room in
// rows_cap rows is BadArg and not written; row_stride > 0: rows at w * row_stride, zeros behind the range's last.  A range
// with a status has rows of zeros only.  Waits for the call: res = ranges with status != 0, the first, its status, all rows.
inline X3Error spectra_rows(Context& ctx, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                            const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges, const SpectraRule& rule,
                            uint64_t row_stride, void* d_out, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                            SpectraResult* res) {
  const x3_spectra_rule r = rule.c_rule();
  int rc = x3_spectra_rows_dev(ctx.raw(), d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, &r, row_stride, d_out,
                               rows_cap, d_row_offsets, d_status);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  SpectraResult q;
  rc = x3_spectra_result(ctx.raw(), &q.n_bad, &q.first_bad, &q.first_bad_status, &q.total_rows);
  if (res) *res = q;
  return static_cast<X3Error>(rc);
}
// The fold of spectra_levels (x3_spectra_fold): frames_per_bin consecutive frames make a time bin, bin k of a frame goes to
// band d_bin_band[k] (a device array of rule.bins() uint32 words; a word >= n_bands: no band), plane b of the records lies
// plane_stride records behind plane b - 1 (0: rows_cap).  time_bins(rows) = the time bins of a range of `rows` frames.
struct SpectraFold {
  uint32_t frames_per_bin = 1, n_bands = 1;
  uint64_t plane_stride = 0;
  const uint32_t* d_bin_band = nullptr;
  uint64_t time_bins(uint64_t rows) const { return frames_per_bin ? (rows + frames_per_bin - 1) / frames_per_bin : 0; }
  x3_spectra_fold c_fold() const {
    x3_spectra_fold f{};
    f.frames_per_bin = frames_per_bin, f.n_bands = n_bands, f.plane_stride = plane_stride, f.d_bin_band = d_bin_band;
    return f;
  }
};
// Band levels (x3_spectra_levels_dev): spectra_rows' POWER words (rule.power must be true) folded into fold.n_bands bands and
// summed over fold.frames_per_bin consecutive frames, one x3_level per (time bin, band) and no row per frame: n = the frames,
// sum_sq = the sum of their band powers (each clamped to 2^30), max = -min = the loudest frame's peak.  The rows of a range
// are its time bins, laid as spectra_rows lays its rows; plane b is band b, at d_levels + b * plane_stride.  Every record the
// call owns is written, the identity where no frame falls.  Waits for the call: res as spectra_rows, total_rows = all time bins.
inline X3Error spectra_levels(Context& ctx, const int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_offsets,
                              const uint32_t* d_lens, const int32_t* d_in_status, uint64_t n_ranges, const SpectraRule& rule,
                              const SpectraFold& fold, uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap,
                              uint64_t* d_row_offsets, int32_t* d_status, SpectraResult* res) {
  const x3_spectra_rule r = rule.c_rule();
  const x3_spectra_fold f = fold.c_fold();
  int rc = x3_spectra_levels_dev(ctx.raw(), d_samples, samples_cap, d_offsets, d_lens, d_in_status, n_ranges, &r, &f, row_stride,
                                 d_levels, rows_cap, d_row_offsets, d_status);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  SpectraResult q;
  rc = x3_spectra_result(ctx.raw(), &q.n_bad, &q.first_bad, &q.first_bad_status, &q.total_rows);
  if (res) *res = q;
  return static_cast<X3Error>(rc);
}
namespace detail {
// the ranges call (packed int16) has been enqueued with rc: the spectra call -- the levels call when there is a fold, d_out
// then being its records -- behind it on the same stream, in place on its statuses, no wait in between; then both results
inline X3Error spectra_behind_ranges(Context& ctx, int rc, int16_t* d_samples, uint64_t samples_cap, const uint64_t* d_sample_offsets,
                                     const uint32_t* d_lens, uint64_t n_ranges, const SpectraRule& rule, uint64_t row_stride,
                                     void* d_out, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status, SpectraResult* res,
                                     const SpectraFold* fold = nullptr) {
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  const x3_spectra_rule r = rule.c_rule();
  const x3_spectra_fold f = fold ? fold->c_fold() : x3_spectra_fold{};
  const int rc2 = fold ? x3_spectra_levels_dev(ctx.raw(), d_samples, samples_cap, d_sample_offsets, d_lens, d_status, n_ranges, &r, &f,
                                               row_stride, static_cast<x3_level*>(d_out), rows_cap, d_row_offsets, d_status)
                       : x3_spectra_rows_dev(ctx.raw(), d_samples, samples_cap, d_sample_offsets, d_lens, d_status, n_ranges, &r,
                                             row_stride, d_out, rows_cap, d_row_offsets, d_status);
  RangesResult rr;
  rc = x3_decode_ranges_result(ctx.raw(), &rr.n_bad, &rr.first_bad, &rr.first_bad_status, &rr.total_samples);
  if (rc2 != X3_OK) return static_cast<X3Error>(rc2);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  SpectraResult q;
  rc = x3_spectra_result(ctx.raw(), &q.n_bad, &q.first_bad, &q.first_bad_status, &q.total_rows);
  if (res) *res = q;
  return static_cast<X3Error>(rc);
}
}  // namespace detail
// Range spectra: decode_ranges (packed int16 into d_samples, samples_cap samples, offsets to d_sample_row_offsets, n_ranges + 1
// words) and spectra_rows on those rows behind it, no host trip and no wait in between; the caller keeps the cut samples.
// d_status holds the ranges call's statuses first and the spectra call's at the end.  Waits for both.
inline X3Error range_spectra(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                             const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, const SpectraRule& rule,
                             int16_t* d_samples, uint64_t samples_cap, uint64_t* d_sample_row_offsets, uint64_t row_stride,
                             void* d_out, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status, SpectraResult* res) {
  if (!s.bytes.ok() || !s.frame_offsets.ok() || !d_sample_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  const int rc = x3_decode_ranges_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(),
                                      d_sample_offsets.as<uint64_t>(), s.n_frames, &c,
                                      s.seg_blocks ? s.seg_index.as<uint64_t>() : nullptr, s.seg_blocks, d_starts, d_lens, n_ranges,
                                      0, d_samples, samples_cap, X3_WINDOW_I16, d_sample_row_offsets, d_status);
  return detail::spectra_behind_ranges(ctx, rc, d_samples, samples_cap, d_sample_row_offsets, d_lens, n_ranges, rule, row_stride,
                                       d_out, rows_cap, d_row_offsets, d_status, res);
}
// Range band levels: range_spectra with spectra_levels in the place of spectra_rows -- the records of the ranges' time bins
// and bands in d_levels, fold.n_bands planes.  (The whole-stream loop over chunks of ranges is the Python mirror's only.)
inline X3Error range_band_levels(Context& ctx, const EncodedStream& s, const Parameters& params, const Buffer& d_sample_offsets,
                                 const uint64_t* d_starts, const uint32_t* d_lens, size_t n_ranges, const SpectraRule& rule,
                                 const SpectraFold& fold, int16_t* d_samples, uint64_t samples_cap, uint64_t* d_sample_row_offsets,
                                 uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap, uint64_t* d_row_offsets,
                                 int32_t* d_status, SpectraResult* res) {
  if (!s.bytes.ok() || !s.frame_offsets.ok() || !d_sample_offsets.ok()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  const int rc = x3_decode_ranges_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(),
                                      d_sample_offsets.as<uint64_t>(), s.n_frames, &c,
                                      s.seg_blocks ? s.seg_index.as<uint64_t>() : nullptr, s.seg_blocks, d_starts, d_lens, n_ranges,
                                      0, d_samples, samples_cap, X3_WINDOW_I16, d_sample_row_offsets, d_status);
  return detail::spectra_behind_ranges(ctx, rc, d_samples, samples_cap, d_sample_row_offsets, d_lens, n_ranges, rule, row_stride,
                                       d_levels, rows_cap, d_row_offsets, d_status, res, &fold);
}

// A batch of independent streams (x3_decode_streams_dev): entry s = bytes [offsets[s], offsets[s] + lengths[s]) of d_x3 (flags:
// X3_STREAMS_ARCHIVE_FRAMES for the frame parts of .x3a archives), decoded into row s of d_out (offsets.size() rows of row_len
// samples, X3_WINDOW_I16 / X3_WINDOW_F32, zeros behind each entry's samples); d_results[s] = x3_decode_stream_dev's results on
// that entry alone.  Waits for the call: res = entries with status != 0, the first, its status.
inline X3Error decode_streams(Context& ctx, const uint8_t* d_x3, uint64_t x3_len, const std::vector<uint64_t>& offsets,
                              const std::vector<uint64_t>& lengths, uint32_t flags, const Parameters& params, void* d_out,
                              uint64_t row_len, int out_format, x3_stream_result* d_results, WindowsResult* res) {
  if (offsets.size() != lengths.size()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  int rc = x3_decode_streams_dev(ctx.raw(), d_x3, x3_len, offsets.data(), lengths.data(), offsets.size(), flags, &c, d_out,
                                 row_len, out_format, d_results);
  if (rc != X3_OK) return static_cast<X3Error>(rc);
  WindowsResult r;
  rc = x3_decode_streams_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}

// Windows of many streams (x3_corpus_build / x3_corpus_windows_dev): an index built once over the entries of d_x3 (as in
// decode_streams; d_x3 must outlive the corpus), after which window w is samples [d_starts[w], d_starts[w] + window_len) of
// entry d_entries[w].  RAII: the index is freed with the object.
class Corpus {
 public:
  Corpus() = default;
  Corpus(const Corpus&) = delete;
  Corpus& operator=(const Corpus&) = delete;
  Corpus(Corpus&& o) noexcept : raw_(o.raw_) { o.raw_ = nullptr; }
  Corpus& operator=(Corpus&& o) noexcept {
    if (this != &o) {
      reset();
      raw_ = o.raw_;
      o.raw_ = nullptr;
    }
    return *this;
  }
  ~Corpus() { reset(); }
  // Synchronous.  seg_blocks: 0 = no segment index (it is only ever a hint).  index_walk: the index by
  // x3_seg_index_build_dev (X3_CORPUS_INDEX_WALK) -- for every parameter set, where the default records one at block length
  // 20 and the default codes only.
  X3Error build(Context& ctx, const uint8_t* d_x3, uint64_t x3_len, const std::vector<uint64_t>& offsets,
                const std::vector<uint64_t>& lengths, uint32_t flags, const Parameters& params, uint32_t seg_blocks = 32,
                bool index_walk = false) {
    if (offsets.size() != lengths.size()) return X3Error::BadArg;
    reset();
    const x3_params c = params.c_params();
    if (index_walk) flags |= X3_CORPUS_INDEX_WALK;
    return static_cast<X3Error>(x3_corpus_build(ctx.raw(), d_x3, x3_len, offsets.data(), lengths.data(), offsets.size(), flags,
                                                &c, seg_blocks, &raw_));
  }
  bool ok() const { return raw_ != nullptr; }
  uint64_t n_entries() const { uint64_t v = 0; x3_corpus_info(raw_, &v, nullptr, nullptr, nullptr); return v; }
  uint64_t n_frames() const { uint64_t v = 0; x3_corpus_info(raw_, nullptr, &v, nullptr, nullptr); return v; }
  uint64_t total_samples() const { uint64_t v = 0; x3_corpus_info(raw_, nullptr, nullptr, &v, nullptr); return v; }
  uint32_t seg_blocks_in_use() const { uint32_t v = 0; x3_corpus_info(raw_, nullptr, nullptr, nullptr, &v); return v; }
  std::vector<x3_corpus_entry> entries() const {
    std::vector<x3_corpus_entry> v(raw_ ? n_entries() : 0);
    if (raw_) x3_corpus_entries(raw_, v.data());
    return v;
  }
  // Waits for the call: res = windows with status != 0, the first, its status.
  X3Error windows(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, uint64_t n_windows, uint32_t window_len,
                  void* d_out, int out_format, int32_t* d_status, WindowsResult* res) const {
    int rc = x3_corpus_windows_dev(ctx.raw(), raw_, d_entries, d_starts, n_windows, window_len, d_out, out_format, d_status);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    WindowsResult r;
    rc = x3_decode_windows_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status);
    if (res) *res = r;
    return static_cast<X3Error>(rc);
  }
  // Ranges of entries (x3_corpus_ranges_dev): range w = samples [d_starts[w], d_starts[w] + d_lens[w]) of entry d_entries[w];
  // layout, capacity and result as device::decode_ranges.  Waits for the call.
  X3Error ranges(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges,
                 uint64_t row_stride, void* d_out, uint64_t out_cap, int out_format, uint64_t* d_out_offsets, int32_t* d_status,
                 RangesResult* res) const {
    int rc = x3_corpus_ranges_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges, row_stride, d_out, out_cap, out_format,
                                  d_out_offsets, d_status);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    RangesResult r;
    rc = x3_decode_ranges_result(ctx.raw(), &r.n_bad, &r.first_bad, &r.first_bad_status, &r.total_samples);
    if (res) *res = r;
    return static_cast<X3Error>(rc);
  }
  // Range spectra of entries: ranges (packed int16) and device::spectra_rows behind it, as device::range_spectra.
  X3Error range_spectra(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens, uint64_t n_ranges,
                        const SpectraRule& rule, int16_t* d_samples, uint64_t samples_cap, uint64_t* d_sample_row_offsets,
                        uint64_t row_stride, void* d_out, uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status,
                        SpectraResult* res) const {
    const int rc = x3_corpus_ranges_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges, 0, d_samples, samples_cap,
                                        X3_WINDOW_I16, d_sample_row_offsets, d_status);
    return detail::spectra_behind_ranges(ctx, rc, d_samples, samples_cap, d_sample_row_offsets, d_lens, n_ranges, rule, row_stride,
                                         d_out, rows_cap, d_row_offsets, d_status, res);
  }
  // Range band levels of entries: ranges (packed int16) and device::spectra_levels behind it, as device::range_band_levels.
  X3Error range_band_levels(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens,
                            uint64_t n_ranges, const SpectraRule& rule, const SpectraFold& fold, int16_t* d_samples,
                            uint64_t samples_cap, uint64_t* d_sample_row_offsets, uint64_t row_stride, x3_level* d_levels,
                            uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status, SpectraResult* res) const {
    const int rc = x3_corpus_ranges_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges, 0, d_samples, samples_cap,
                                        X3_WINDOW_I16, d_sample_row_offsets, d_status);
    return detail::spectra_behind_ranges(ctx, rc, d_samples, samples_cap, d_sample_row_offsets, d_lens, n_ranges, rule, row_stride,
                                         d_levels, rows_cap, d_row_offsets, d_status, res, &fold);
  }
  // Levels of every entry (x3_corpus_levels_dev): entry e's records are [row_first[e], row_first[e + 1]) of d_levels, positions
  // relative to the entry; levels_rows(bin_len) is that prefix, d_levels holds its last word of records.  Waits for the call.
  // signal: as device::levels (x3_corpus_signal_levels_dev); no difference crosses from one entry into the next.
  std::vector<uint64_t> levels_rows(uint64_t bin_len) const {
    std::vector<uint64_t> v(raw_ ? n_entries() + 1 : 0);
    if (raw_) x3_corpus_levels_rows(raw_, bin_len, v.data());
    return v;
  }
  X3Error levels(Context& ctx, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows, int32_t* d_frame_status,
                 WindowsResult* res, LevelSignal signal = LevelSignal::Samples) const {
    return detail::levels_result(ctx, x3_corpus_signal_levels_dev(ctx.raw(), raw_, bin_len, d_levels, n_rows, d_frame_status,
                                  static_cast<int>(signal)), res);
  }
  // ... behind an integer FIR filter (x3_corpus_fir_levels_dev): as device::levels with a Fir; no history crosses from one
  // entry into the next.
  X3Error levels(Context& ctx, uint64_t bin_len, x3_level* d_levels, uint64_t n_rows, int32_t* d_frame_status,
                 WindowsResult* res, const Fir& fir) const {
    const x3_level_fir f = fir.c_fir();
    return detail::levels_result(ctx, x3_corpus_fir_levels_dev(ctx.raw(), raw_, bin_len, d_levels, n_rows, d_frame_status, &f),
                                  res);
  }
  // Tone levels of every entry (x3_corpus_tone_levels_dev): levels()' rows as tone records; the phase restarts at 0 with
  // every entry.  Waits for the call.
  X3Error tone_levels(Context& ctx, uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_rows, int32_t* d_frame_status,
                      WindowsResult* res, const Tone& tone) const {
    const x3_level_tone t = tone.c_tone();
    return detail::levels_result(ctx, x3_corpus_tone_levels_dev(ctx.raw(), raw_, bin_len, d_levels, n_rows, d_frame_status, &t),
                                  res);
  }
  // Tone bank levels of every entry (x3_corpus_tone_bank_levels_dev): bank.steps.size() planes of tone_levels()' n_rows
  // records, plane t at d_levels + t * n_rows; every entry starts at phase 0 in every plane.  Waits for the call.
  X3Error tone_bank_levels(Context& ctx, uint64_t bin_len, x3_tone_level* d_levels, uint64_t n_rows, int32_t* d_frame_status,
                           WindowsResult* res, const ToneBank& bank) const {
    if (!bank.ok()) return X3Error::BadArg;
    const x3_level_tone_bank b = bank.c_bank();
    return detail::levels_result(ctx, x3_corpus_tone_bank_levels_dev(ctx.raw(), raw_, bin_len, d_levels, n_rows, d_frame_status,
                                  &b), res);
  }
  // Events of every entry (x3_corpus_events_dev) over the n_rows records levels() wrote: as device::events, with the events'
  // entries in d_entries; the arrays go to ranges() with n_ranges = cap as they are.  Waits for the call.
  X3Error events(Context& ctx, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len, const x3_event_rule& rule,
                 uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens, x3_level* d_event_levels, uint64_t cap,
                 uint64_t* d_count, uint64_t* count) const {
    int rc = x3_corpus_events_dev(ctx.raw(), raw_, d_levels, n_rows, bin_len, &rule, d_entries, d_starts, d_lens, d_event_levels,
                                  cap, d_count);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
  }
  // Level quantiles of every entry (x3_corpus_level_quantiles_dev) over the n_rows records levels() wrote: as
  // device::level_quantiles, d_values n_entries * q_ppm.size() words, d_counted n_entries.  Waits for the call.
  X3Error level_quantiles(Context& ctx, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len, int key,
                          const std::vector<uint32_t>& q_ppm, uint32_t* d_values, uint32_t* d_counted, QuantilesResult* res) const {
    int rc = x3_corpus_level_quantiles_dev(ctx.raw(), raw_, d_levels, n_rows, bin_len, key, q_ppm.data(), (uint32_t)q_ppm.size(),
                                           d_values, d_counted);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    QuantilesResult r;
    rc = x3_level_quantiles_result(ctx.raw(), &r.n_empty, &r.first_empty);
    if (res) *res = r;
    return static_cast<X3Error>(rc);
  }
  // Thresholds of every entry (x3_corpus_level_thresholds_dev): n_entries records at d_thr.  Waits for the call.
  X3Error level_thresholds(Context& ctx, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len, const x3_threshold_rule& rule,
                           x3_event_threshold* d_thr, QuantilesResult* res) const {
    int rc = x3_corpus_level_thresholds_dev(ctx.raw(), raw_, d_levels, n_rows, bin_len, &rule, d_thr);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    QuantilesResult r;
    rc = x3_level_quantiles_result(ctx.raw(), &r.n_empty, &r.first_empty);
    if (res) *res = r;
    return static_cast<X3Error>(rc);
  }
  // Events with entry e's two values at d_thr[e] (x3_corpus_events_adaptive_dev); otherwise as events().  Waits for the call.
  X3Error events_adaptive(Context& ctx, const x3_level* d_levels, uint64_t n_rows, uint64_t bin_len, const x3_event_rule& rule,
                          const x3_event_threshold* d_thr, uint32_t* d_entries, uint64_t* d_starts, uint32_t* d_lens,
                          x3_level* d_event_levels, uint64_t cap, uint64_t* d_count, uint64_t* count) const {
    int rc = x3_corpus_events_adaptive_dev(ctx.raw(), raw_, d_levels, n_rows, bin_len, &rule, d_thr, d_entries, d_starts, d_lens,
                                           d_event_levels, cap, d_count);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
  }
  // Plane events of every entry (x3_corpus_plane_events_dev) over the rule's planes of the n_rows records levels() lays: as
  // device::plane_events, with the events' entries in d_entries; d_thr: nullptr, or n_planes * n_entries records laid
  // plane-major.  Waits for the call.
  X3Error plane_events(Context& ctx, const x3_level* d_levels, uint64_t plane_stride, uint64_t n_rows, uint64_t bin_len,
                       const PlaneEventRule& rule, const x3_event_threshold* d_thr, uint32_t* d_entries, uint64_t* d_starts,
                       uint32_t* d_lens, uint32_t* d_event_planes, x3_level* d_event_levels, uint64_t cap, uint64_t* d_count,
                       uint64_t* count) const {
    if (!rule.ok()) return X3Error::BadArg;
    const x3_plane_event_rule r = rule.c_rule();
    int rc = x3_corpus_plane_events_dev(ctx.raw(), raw_, d_levels, plane_stride, n_rows, bin_len, &r, d_thr, d_entries, d_starts,
                                        d_lens, d_event_planes, d_event_levels, cap, d_count);
    if (rc != X3_OK) return static_cast<X3Error>(rc);
    return static_cast<X3Error>(x3_events_result(ctx.raw(), count));
  }
  // Range levels of entries (x3_corpus_range_levels_dev): the records of range w = samples [d_starts[w], d_starts[w] +
  // d_lens[w]) of entry d_entries[w]; bins, layout, capacity and result as device::range_levels; the arrays events() wrote go
  // in as they are.  signal: as there (x3_corpus_signal_range_levels_dev).  Waits for the call.
  X3Error range_levels(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens,
                       uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap,
                       uint64_t* d_row_offsets, int32_t* d_status, RangeLevelsResult* res,
                       LevelSignal signal = LevelSignal::Samples) const {
    return detail::levels_result(ctx, x3_corpus_signal_range_levels_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges,
                                  bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, static_cast<int>(signal)), res);
  }
  // FIR range levels of entries (x3_corpus_fir_range_levels_dev): as device::fir_range_levels; no filter history crosses from
  // one entry into the next.  Waits for the call.
  X3Error fir_range_levels(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens,
                           uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride, x3_level* d_levels, uint64_t rows_cap,
                           uint64_t* d_row_offsets, int32_t* d_status, const Fir& fir, RangeLevelsResult* res) const {
    const x3_level_fir f = fir.c_fir();
    return detail::levels_result(ctx, x3_corpus_fir_range_levels_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges,
                                  bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, &f), res);
  }
  // Tone range levels of entries (x3_corpus_tone_range_levels_dev): as device::tone_range_levels; starts count from the
  // entry's first position and so does the phase, 0 there.  Waits for the call.
  X3Error tone_range_levels(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens,
                            uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride, x3_tone_level* d_levels, uint64_t rows_cap,
                            uint64_t* d_row_offsets, int32_t* d_status, const Tone& tone, RangeLevelsResult* res) const {
    const x3_level_tone t = tone.c_tone();
    return detail::levels_result(ctx, x3_corpus_tone_range_levels_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges,
                                  bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, &t), res);
  }
  // Tone bank range levels of entries (x3_corpus_tone_bank_range_levels_dev): as device::tone_bank_range_levels --
  // bank.steps.size() planes of rows_cap records; starts count from the entry's first position and so does the phase, 0
  // there in every plane.  Waits for the call.
  X3Error tone_bank_range_levels(Context& ctx, const uint32_t* d_entries, const uint64_t* d_starts, const uint32_t* d_lens,
                                 uint64_t n_ranges, uint64_t bin_len, uint64_t row_stride, x3_tone_level* d_levels,
                                 uint64_t rows_cap, uint64_t* d_row_offsets, int32_t* d_status, const ToneBank& bank,
                                 RangeLevelsResult* res) const {
    if (!bank.ok()) return X3Error::BadArg;
    const x3_level_tone_bank b = bank.c_bank();
    return detail::levels_result(ctx, x3_corpus_tone_bank_range_levels_dev(ctx.raw(), raw_, d_entries, d_starts, d_lens, n_ranges,
                                  bin_len, row_stride, d_levels, rows_cap, d_row_offsets, d_status, &b), res);
  }
  // the recorded segment index (device memory the corpus owns), nullptr and 0 words without one
  const uint64_t* seg_index(uint64_t* n_words) const {
    const uint64_t* d = nullptr;
    uint64_t n = 0;
    if (raw_) x3_corpus_seg_index(raw_, &d, &n);
    if (n_words) *n_words = n;
    return d;
  }
  const x3_corpus* raw() const { return raw_; }

 private:
  void reset() {
    if (raw_) x3_corpus_destroy(raw_);
    raw_ = nullptr;
  }
  x3_corpus* raw_ = nullptr;
};

// Placement (x3_place_buffers; profiles/r6/decoder_modes.txt): the round trip timed on every pair of candidate buffers --
// ms[i * backs.size() + j] for (streams[i], backs[j]).  A pipeline that keeps its buffers calls this once and keeps the
// pair that runs best; what it does not keep it frees.
inline X3Error place_buffers(Context& ctx, const int16_t* d_wav, size_t n, const Parameters& params,
                             const std::vector<uint8_t*>& streams, size_t cap, uint64_t* d_frame_offsets,
                             const std::vector<int16_t*>& backs, std::vector<double>* ms, uint32_t warm = 4, uint32_t steps = 8) {
  if (!ms || streams.empty() || backs.empty()) return X3Error::BadArg;
  const x3_params c = params.c_params();
  ms->assign(streams.size() * backs.size(), 0.0);
  return static_cast<X3Error>(x3_place_buffers(ctx.raw(), d_wav, n, &c, streams.data(), static_cast<uint32_t>(streams.size()), cap,
                                               d_frame_offsets, backs.data(), static_cast<uint32_t>(backs.size()), warm, steps,
                                               ms->data()));
}

// Parameter tuning (NOT in the crate; include/x3hip.h, "parameter tuning"): per-candidate exact encoded sizes of
// device-resident batches, accumulated.  Choice: the smallest total; among equal totals the default set, else the lowest
// index.
class Tuner {
 public:
  Tuner(Context& ctx, uint32_t spf = X3_TUNE_DEFAULT_SPF) { rc_ = static_cast<X3Error>(x3_tuner_create(ctx.raw(), spf, &t_)); }
  Tuner(const Tuner&) = delete;
  Tuner& operator=(const Tuner&) = delete;
  ~Tuner() { x3_tuner_destroy(t_); }
  X3Error status() const { return rc_; }
  // every chunk but the last must be whole frames for the totals to be those of one encode of the whole input
  X3Error add(const int16_t* d_wav, size_t n_per_clip, size_t n_clips = 1, size_t clip_stride = 0) {
    const x3_batch b{n_per_clip, clip_stride ? clip_stride : n_per_clip, n_clips};
    return static_cast<X3Error>(x3_tuner_add_dev(t_, d_wav, &b));
  }
  // syncs; sizes (may be null) receives every candidate's total
  X3Error result(Parameters* best, uint64_t* best_bytes, std::vector<uint64_t>* sizes = nullptr) {
    x3_params c;
    if (sizes) sizes->assign(X3_TUNE_CANDIDATES, 0);
    const int rc = x3_tuner_result(t_, &c, best_bytes, sizes ? sizes->data() : nullptr);
    if (rc == X3_OK && best) *best = Parameters::from_c(c);
    return static_cast<X3Error>(rc);
  }
  X3Error reset() { return static_cast<X3Error>(x3_tuner_reset(t_)); }

 private:
  x3_tuner* t_ = nullptr;
  X3Error rc_ = X3Error::Ok;
};
}  // namespace device

// x3_tune on host samples: the chosen parameters, their total and (sizes != null) every candidate's total
inline X3Error tune(Context& ctx, const int16_t* wav, size_t n, Parameters* best, uint64_t* best_bytes = nullptr,
                    std::vector<uint64_t>* sizes = nullptr, uint32_t spf = X3_TUNE_DEFAULT_SPF) {
  x3_params c;
  if (sizes) sizes->assign(X3_TUNE_CANDIDATES, 0);
  const int rc = x3_tune(ctx.raw(), wav, n, spf, &c, best_bytes, sizes ? sizes->data() : nullptr);
  if (rc == X3_OK && best) *best = Parameters::from_c(c);
  return static_cast<X3Error>(rc);
}
// candidate `index` of the grid at frame length spf
inline X3Error tune_candidate(uint32_t index, Parameters* out, uint32_t spf = X3_TUNE_DEFAULT_SPF) {
  x3_params c;
  const int rc = x3_tune_candidate(index, spf, &c);
  if (rc == X3_OK && out) *out = Parameters::from_c(c);
  return static_cast<X3Error>(rc);
}

// Multi-channel extension (x3_mc.h; NOT in the crate, whose encode() returns MoreThanOneChannel for more than one channel
// and whose reader refuses such frames -- as encoder::encode and decoder::decode_stream above do): the layout the frame
// header's <Num Channels> and "pack the data block for each channel" (encoder.rs:197) foresee.  Channels of equal length.
namespace multichannel {
inline X3Error encode(Context& ctx, const Channel* const* channels, size_t n_channels, bytewriter::SliceByteWriter& writer,
                      uint64_t (&stats)[6]) {
  if (n_channels == 0) return X3Error::BadArg;
  std::vector<const int16_t*> wavs(n_channels);
  for (size_t k = 0; k < n_channels; ++k) {
    if (channels[k]->len != channels[0]->len) return X3Error::BadArg;
    wavs[k] = channels[k]->wav;
  }
  x3_params c = channels[0]->params.c_params();
  uint64_t pos = 0;
  int rc = x3_encode_mc(ctx.raw(), wavs.data(), (uint32_t)n_channels, channels[0]->len, &c, writer.data(), writer.capacity(),
                        writer.position(), &pos, stats);
  if (rc == 0) writer.advance_to((size_t)pos);
  return static_cast<X3Error>(rc);
}
inline X3Error decode_stream(Context& ctx, const uint8_t* x3, size_t len, size_t n_channels, const Parameters& params,
                             int16_t* const* wavs, size_t wav_cap, decoder::StreamResult* res) {
  x3_params c = params.c_params();
  decoder::StreamResult r;
  int rc = x3_decode_stream_mc(ctx.raw(), x3, len, (uint32_t)n_channels, &c, wavs, wav_cap, &r.samples, &r.frames_ok,
                               &r.frame_errors);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
}  // namespace multichannel

// encodefile.rs / decodefile.rs without the files: the .x3a archive header and the whole-buffer conversions
namespace archive {
struct X3aSpec {  // decodefile.rs:36-43
  uint32_t sample_rate = 0;
  Parameters params;
  uint8_t channels = 0;
};
// create_archive_header (encodefile.rs:82-138); returns the header length through *out_len
inline X3Error create_archive_header(uint32_t sample_rate, const Parameters& params, uint8_t* out, size_t cap,
                                     size_t* out_len) {
  x3_params c = params.c_params();
  uint64_t n = 0;
  int rc = x3_archive_header_write(sample_rate, &c, out, cap, &n);
  if (out_len) *out_len = (size_t)n;
  return static_cast<X3Error>(rc);
}
// read_archive_header (decodefile.rs:142-176): header_size = 20 + XML, audio frames start at 8 + header_size
inline X3Error read_archive_header(const uint8_t* bytes, size_t len, X3aSpec* spec, size_t* header_size) {
  x3_params c;
  uint64_t hs = 0;
  X3aSpec s;
  int rc = x3_archive_header_read(bytes, len, &s.sample_rate, &c, &s.channels, &hs);
  if (rc == X3_OK) {
    s.params = Parameters::from_c(c);
    if (spec) *spec = s;
    if (header_size) *header_size = (size_t)hs;
  }
  return static_cast<X3Error>(rc);
}
// wav_to_x3a (encodefile.rs:48-77) / x3a_to_wav (decodefile.rs:189-212) on buffers
inline X3Error wav_to_x3a(Context& ctx, const int16_t* wav, size_t n, uint32_t sample_rate, uint8_t* out, size_t cap,
                          size_t* out_len) {
  uint64_t len = 0;
  int rc = x3_x3a_encode(ctx.raw(), wav, n, sample_rate, out, cap, &len, nullptr);
  if (out_len) *out_len = (size_t)len;
  return static_cast<X3Error>(rc);
}
inline X3Error x3a_to_wav(Context& ctx, const uint8_t* x3a, size_t len, int16_t* wav, size_t wav_cap,
                          uint32_t* sample_rate, decoder::StreamResult* res) {
  decoder::StreamResult r;
  int rc = x3_x3a_decode(ctx.raw(), x3a, len, wav, wav_cap, &r.samples, sample_rate, &r.frames_ok, &r.frame_errors);
  if (res) *res = r;
  return static_cast<X3Error>(rc);
}
}  // namespace archive

// the file level, under the reference's module names (encodefile.rs:48-77, decodefile.rs:189-227): what
// src/bin/x3.rs:79-80 calls.  Streamed through the GPU in chunks (x3hip.h).
namespace encodefile {
inline X3Error wav_to_x3a(Context& ctx, const char* wav_filename, const char* x3a_filename, bool print_statistics = true) {
  uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
  const int rc = x3_wav_to_x3a(ctx.raw(), wav_filename, x3a_filename, stats);
  if (rc == X3_OK && print_statistics) encoder::detail::print_stats(stats);
  return static_cast<X3Error>(rc);
}
inline X3Error wav_to_x3a(const char* wav_filename, const char* x3a_filename) {  // encodefile.rs:48
  X3_WITH_DEFAULT_CONTEXT(wav_to_x3a(ctx, wav_filename, x3a_filename, true));
}
}  // namespace encodefile
namespace decodefile {
constexpr size_t READ_BUFFER_SIZE = X3_READ_BUFFER_SIZE;       // decodefile.rs:44 (X3_READ_BUFFER_SIZE is the C macro)
constexpr size_t X3_WRITE_BUFFER_SIZE = READ_BUFFER_SIZE * 8;  // decodefile.rs:45

// decodefile.rs:47-136.  open() reads the archive header; decode_next_frame() hands out one frame per call with the
// reference's per-call results: Ok + *some + *n = samples (Ok(Some(n)), n >= 1), Ok + !*some (Ok(None): end of the
// data, a payload that runs past it, or a frame that failed to decode -- counted in frame_errors()), or the error the
// reference returns for that frame (header CRC, key, payload CRC ...), after which a further call goes on behind it.
// Behind it the library decodes windows of frames ahead on the GPU (x3_reader.h).
class X3aReader {
 public:
  static X3Error open(const char* filename, X3aReader* out) { return open(default_context(), filename, out, &default_context_mutex()); }
  static X3Error open(Context& ctx, const char* filename, X3aReader* out, std::mutex* mu = nullptr) {
    MaybeLock lk(mu);
    out->close_locked();
    out->mu_ = mu;
    int rc = x3_reader_open(ctx.raw(), filename, &out->r_);
    if (rc) return static_cast<X3Error>(rc);
    x3_params c;
    x3_reader_spec(out->r_, &out->spec_.sample_rate, &c, &out->spec_.channels);
    out->spec_.params = Parameters::from_c(c);
    return X3Error::Ok;
  }
  X3aReader() = default;
  X3aReader(const X3aReader&) = delete;
  X3aReader& operator=(const X3aReader&) = delete;
  ~X3aReader() {
    MaybeLock lk(mu_);
    close_locked();
  }
  const X3aSpec& spec() const { return spec_; }
  X3Error decode_next_frame(int16_t (&wav_buf)[X3_WRITE_BUFFER_SIZE], size_t* n, bool* some) {
    MaybeLock lk(mu_);
    uint64_t got = 0;
    int rc = x3_reader_next_frame(r_, wav_buf, X3_WRITE_BUFFER_SIZE, &got);
    *some = rc == X3_OK && got != 0;
    *n = (size_t)got;
    return static_cast<X3Error>(rc);
  }
  size_t frame_errors() const { return r_ ? (size_t)x3_reader_frame_errors(r_) : 0; }

 private:
  void close_locked() {
    if (r_) x3_reader_close(r_);
    r_ = nullptr;
  }
  x3_reader* r_ = nullptr;
  std::mutex* mu_ = nullptr;
  X3aSpec spec_{0, Parameters{}, 0};
};

inline X3Error x3a_to_wav(Context& ctx, const char* x3a_filename, const char* wav_filename, uint64_t* samples = nullptr,
                          uint64_t* frame_errors = nullptr) {
  return static_cast<X3Error>(x3_x3a_to_wav(ctx.raw(), x3a_filename, wav_filename, samples, frame_errors));
}
inline X3Error x3a_to_wav(const char* x3a_filename, const char* wav_filename) {  // decodefile.rs:189
  X3_WITH_DEFAULT_CONTEXT(x3a_to_wav(ctx, x3a_filename, wav_filename, nullptr, nullptr));
}
}  // namespace decodefile
}  // namespace x3
