// Exercises the trailing device::LevelSignal of x3::device::range_levels and x3::device::Corpus::range_levels of
// x3-rust_amd/host/x3.hpp (x3_signal_range_levels_dev / x3_corpus_signal_range_levels_dev) on the base stream of
// tests/test_gpu_range_levels.py: 2 137 samples in frames of 400 (block length 20, 20 blocks a frame) with a walk-built index.
// LevelSignal::Diff: packed and padded records at three bin lengths against a loop over the positions -- the difference at
// every position but the stream's first, the one at a range's own first position included (ranges that start at a frame's
// first sample, inside a frame and at a stretch's first sample).  LevelSignal::Samples and the defaulted argument: the same
// bytes.  Needs a GPU.
// usage: test_signal_range_levels_hpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../x3-rust_amd/host/x3.hpp"

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      std::exit(1);                                                           \
    }                                                                         \
  } while (0)

static bool same(const x3_level& a, const x3_level& b) {
  return a.sum_sq == b.sum_sq && a.sum == b.sum && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == b.reserved;
}

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
  const std::vector<uint64_t> starts = {0, 399, 2000, 2137, 400, 5, 81, 800, 0, 1};
  const std::vector<uint32_t> lens = {400, 3, 137, 0, 400, 0, 700, 1, 2137, 2137};     // (1, 2137) runs off the end
  const size_t W = starts.size();
  x3::device::Buffer d_starts(ctx, 8 * W), d_lens(ctx, 4 * W), d_status(ctx, 4 * W), d_off(ctx, 8 * (W + 1));
  CHECK(d_starts.upload(starts.data(), 8 * W) == x3::X3Error::Ok && d_lens.upload(lens.data(), 4 * W) == x3::X3Error::Ok);
  // one corpus entry: the stream itself
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, {0}, {s.len}, 0, params, 4, true) == x3::X3Error::Ok);
  const std::vector<uint32_t> entries(W, 0);
  x3::device::Buffer d_entries(ctx, 4 * W);
  CHECK(d_entries.upload(entries.data(), 4 * W) == x3::X3Error::Ok);
  const x3_level id{0, 0, 32767, -32768, 0, 0};
  for (int form = 0; form < 2; ++form)
    for (uint64_t bin_len : {(uint64_t)0, (uint64_t)7, (uint64_t)400})
      for (int padded = 0; padded < 2; ++padded) {
        std::vector<uint64_t> rows(W), off(W + 1, 0);
        for (size_t w = 0; w < W; ++w) {
          rows[w] = bin_len && lens[w] ? (lens[w] + bin_len - 1) / bin_len : 1;
          off[w + 1] = off[w] + rows[w];
        }
        const uint64_t row_stride = padded ? rows[W - 2] : 0;     // (the whole stream's rows: the most any range has)
        // packed: room for everything but the last range
        const uint64_t cap = padded ? W * row_stride : off[W] - 1;
        x3::device::Buffer d_levels(ctx, sizeof(x3_level) * cap);
        std::vector<x3_level> out(cap);
        std::memset(out.data(), 0x5A, sizeof(x3_level) * cap);
        CHECK(d_levels.upload(out.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
        x3::device::RangeLevelsResult r;
        const auto diff = x3::device::LevelSignal::Diff;
        if (form == 0)
          CHECK(x3::device::range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, bin_len,
                                         row_stride, d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(),
                                         &r, diff) == x3::X3Error::Ok);
        else
          CHECK(corpus.range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, bin_len,
                                    row_stride, d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(),
                                    &r, diff) == x3::X3Error::Ok);
        CHECK(r.n_bad == 1 && r.first_bad == W - 1 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);
        std::vector<int32_t> st(W);
        std::vector<uint64_t> got_off(W + 1);
        CHECK(d_status.download(st.data(), 4 * W) == x3::X3Error::Ok && d_off.download(got_off.data(), 8 * (W + 1)) == x3::X3Error::Ok);
        CHECK(d_levels.download(out.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
        for (size_t w = 0; w <= W; ++w) CHECK(got_off[w] == (padded ? w * row_stride : off[w]));
        for (size_t w = 0; w < W; ++w) {
          const bool bad = w == W - 1;      // off the end (and, packed, without room)
          CHECK(st[w] == (bad ? X3_ERR_BAD_ARG : 0));
          if (bad && !padded) {             // (no room: not written)
            for (uint64_t i = got_off[w]; i < cap; ++i) CHECK(reinterpret_cast<const uint8_t*>(&out[i])[0] == 0x5A);
            continue;
          }
          std::vector<x3_level> want(padded ? row_stride : rows[w], id);
          for (uint64_t i = 0; !bad && i < lens[w]; ++i) {
            if (starts[w] + i == 0) continue;     // (the stream's first position has no difference)
            x3_level& b = want[bin_len ? i / bin_len : 0];
            const int32_t v = std::min(std::max((int32_t)wav[starts[w] + i] - (int32_t)wav[starts[w] + i - 1], -32768), 32767);
            b.sum_sq += (uint64_t)(v * v);
            b.sum += v;
            b.min = std::min(b.min, v);
            b.max = std::max(b.max, v);
            ++b.n;
          }
          for (size_t i = 0; i < want.size(); ++i) CHECK(same(out[got_off[w] + i], want[i]));
        }
      }
  // LevelSignal::Samples, and no argument at all: the same bytes
  {
    const uint64_t cap = 64;
    std::vector<x3_level> a(cap), b(cap);
    for (int form = 0; form < 2; ++form)
      for (int given = 0; given < 2; ++given) {
        std::vector<x3_level>& out = given ? a : b;
        std::memset(out.data(), 0x5A, sizeof(x3_level) * cap);
        x3::device::Buffer d_levels(ctx, sizeof(x3_level) * cap);
        CHECK(d_levels.upload(out.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
        x3::device::RangeLevelsResult r;
        const auto smp = x3::device::LevelSignal::Samples;
        x3::X3Error rc;
        if (form == 0 && given)
          rc = x3::device::range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 400, 0,
                                        d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r, smp);
        else if (form == 0)
          rc = x3::device::range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 400, 0,
                                        d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r);
        else if (given)
          rc = corpus.range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 400, 0,
                                   d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r, smp);
        else
          rc = corpus.range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 400, 0,
                                   d_levels.as<x3_level>(), cap, d_off.as<uint64_t>(), d_status.as<int32_t>(), &r);
        CHECK(rc == x3::X3Error::Ok && r.n_bad == 1 && r.first_bad == W - 1);
        CHECK(d_levels.download(out.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
        if (given) CHECK(std::memcmp(a.data(), b.data(), sizeof(x3_level) * cap) == 0);
      }
    CHECK(a[0].n == 400);     // (0, 400) at bins of 400: the samples, not their differences
  }
  long long replays = -1, overflow = -1;
  CHECK(x3_ctx_get_option(ctx.raw(), "last_range_levels_replays", &replays) == 0 && replays == 0);
  CHECK(x3_ctx_get_option(ctx.raw(), "last_range_levels_overflow", &overflow) == 0 && overflow == 0);
  std::printf("test_signal_range_levels_hpp: ok\n");
  return 0;
}
