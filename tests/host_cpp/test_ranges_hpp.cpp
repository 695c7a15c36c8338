// Exercises x3::device::decode_ranges and x3::device::Corpus::ranges of x3-rust_amd/host/x3.hpp (x3_decode_ranges_dev /
// x3_corpus_ranges_dev) on the base stream of tests/test_gpu_ranges.py: 2 137 samples in frames of 400 (block length 20, 20
// blocks a frame) with a walk-built index, packed and padded rows in both formats against the samples the stream was encoded
// from, a range off the end, a length of 0, a packed capacity that refuses the last range.  Needs a GPU.
// usage: test_ranges_hpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../x3-rust_amd/host/x3.hpp"

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

int main() {
  x3::Context ctx(0);
  const x3_params cp{20, 20, {0, 1, 3}, {3, 8, 20}};
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 2137;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 1616, 0, n, wav.data()) == 0);
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 0, &s) == x3::X3Error::Ok);
  CHECK(s.n_frames == 6);
  CHECK(x3::device::index_by_walk(ctx, &s, params, 4) == x3::X3Error::Ok && s.seg_blocks == 4);
  x3::device::Buffer d_so;
  CHECK(x3::device::sample_offsets(ctx, s, &d_so) == x3::X3Error::Ok);
  const std::vector<uint64_t> starts = {0, 399, 2000, 2137, 1737, 5, 1};
  const std::vector<uint32_t> lens = {400, 3, 137, 0, 400, 0, 2137};     // (1, 2137) runs off the end
  const size_t W = starts.size();
  std::vector<uint64_t> off(W + 1, 0);
  for (size_t w = 0; w < W; ++w) off[w + 1] = off[w] + lens[w];
  x3::device::Buffer d_starts(ctx, 8 * W), d_lens(ctx, 4 * W), d_status(ctx, 4 * W), d_off(ctx, 8 * (W + 1));
  CHECK(d_starts.upload(starts.data(), 8 * W) == x3::X3Error::Ok && d_lens.upload(lens.data(), 4 * W) == x3::X3Error::Ok);
  // one corpus entry: the stream itself
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, {0}, {s.len}, 0, params, 4, true) == x3::X3Error::Ok);
  const std::vector<uint32_t> entries(W, 0);
  x3::device::Buffer d_entries(ctx, 4 * W);
  CHECK(d_entries.upload(entries.data(), 4 * W) == x3::X3Error::Ok);
  const uint64_t stride = 512;
  for (int form = 0; form < 2; ++form)
    for (uint64_t row_stride : {(uint64_t)0, stride})
      for (int fmt : {X3_WINDOW_I16, X3_WINDOW_F32}) {
        const size_t esz = fmt == X3_WINDOW_F32 ? 4 : 2;
        // packed: room for everything but the last range
        const uint64_t cap = row_stride ? W * row_stride : off[W] - 1;
        x3::device::Buffer d_out(ctx, esz * cap);
        std::vector<uint8_t> out(esz * cap, 0x5A);
        CHECK(d_out.upload(out.data(), out.size()) == x3::X3Error::Ok);
        x3::device::RangesResult r;
        if (form == 0)
          CHECK(x3::device::decode_ranges(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, row_stride,
                                          d_out.data(), cap, fmt, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r) == x3::X3Error::Ok);
        else
          CHECK(corpus.ranges(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, row_stride,
                              d_out.data(), cap, fmt, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r) == x3::X3Error::Ok);
        CHECK(r.n_bad == 1 && r.first_bad == W - 1 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_samples == off[W]);
        std::vector<int32_t> st(W);
        std::vector<uint64_t> got_off(W + 1);
        CHECK(d_status.download(st.data(), 4 * W) == x3::X3Error::Ok && d_off.download(got_off.data(), 8 * (W + 1)) == x3::X3Error::Ok);
        CHECK(d_out.download(out.data(), out.size()) == x3::X3Error::Ok);
        auto at = [&](uint64_t i) -> float {
          return fmt == X3_WINDOW_F32 ? reinterpret_cast<const float*>(out.data())[i]
                                      : (float)reinterpret_cast<const int16_t*>(out.data())[i] / 32768.0f;
        };
        for (size_t w = 0; w <= W; ++w) CHECK(got_off[w] == (row_stride ? w * row_stride : off[w]));
        for (size_t w = 0; w < W; ++w) {
          const bool bad = w == W - 1;      // off the end (and, packed, without room; padded, longer than the stride)
          CHECK(st[w] == (bad ? X3_ERR_BAD_ARG : 0));
          const uint64_t base = got_off[w], end = row_stride ? row_stride : lens[w];
          if (bad && !row_stride) continue;   // (no room: not written)
          for (uint64_t i = 0; i < end; ++i) {
            const int16_t want = bad || i >= lens[w] ? 0 : wav[starts[w] + i];
            CHECK(at(base + i) == (float)want / 32768.0f);
          }
        }
      }
  std::printf("test_ranges_hpp: ok\n");
  return 0;
}
