// Exercises x3::device::fir_range_levels and x3::device::Corpus::fir_range_levels of x3-rust_amd/host/x3.hpp
// (x3_fir_range_levels_dev / x3_corpus_fir_range_levels_dev) on the base stream of tests/test_gpu_range_levels.py: 2 137
// samples in frames of 400 (block length 20, 20 blocks a frame) with a walk-built index.  Packed and padded records at three
// bin lengths against a loop over the positions: y[i] = clamp((sum of taps[t] * x[i - t]) >> shift) at every position from
// T - 1 on, a range's own first positions included (ranges that start at a frame's first sample, T - 1 behind it, inside a
// frame and at a stretch's first sample).  {1} and {1, -1}: the bytes of LevelSignal::Samples and LevelSignal::Diff.  Needs a
// GPU.
// usage: test_fir_range_levels_hpp
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
  using x3::device::Fir;
  using x3::device::LevelSignal;
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
  const std::vector<uint64_t> starts = {0, 399, 2000, 2137, 400, 5, 81, 800, 0, 1, 406, 407, 87};
  const std::vector<uint32_t> lens = {400, 3, 137, 0, 400, 0, 700, 1, 2137, 2137, 9, 9, 2};     // (1, 2137) runs off the end
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
  const std::vector<Fir> firs = {Fir{{1, 0, -1}, 0}, Fir{{-3000, 9000, -200, 7, 5000, -8000, 1, 6560}, 7}, Fir{{16384, -16384}, 0}};
  auto layout = [&](uint64_t bin_len, bool padded, std::vector<uint64_t>* rows, std::vector<uint64_t>* off, uint64_t* stride,
                    uint64_t* cap) {
    rows->assign(W, 0);
    off->assign(W + 1, 0);
    uint64_t most = 1;
    for (size_t w = 0; w < W; ++w) {
      (*rows)[w] = bin_len ? std::max<uint64_t>(1, (lens[w] + bin_len - 1) / bin_len) : 1;
      (*off)[w + 1] = (*off)[w] + (*rows)[w];
      most = std::max(most, (*rows)[w]);
    }
    *stride = padded ? most : 0;
    *cap = padded ? most * W : (*off)[W];
  };
  for (const Fir& fir : firs)
    for (int form = 0; form < 2; ++form)
      for (uint64_t bin_len : {(uint64_t)0, (uint64_t)7, (uint64_t)400})
        for (int padded = 0; padded < 2; ++padded) {
          std::vector<uint64_t> rows, off;
          uint64_t stride, cap;
          layout(bin_len, padded, &rows, &off, &stride, &cap);
          x3::device::Buffer d_lv(ctx, sizeof(x3_level) * cap);
          x3::device::RangeLevelsResult r;
          const x3::X3Error e =
              form == 0 ? x3::device::fir_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, bin_len,
                                                       stride, d_lv.as<x3_level>(), cap, padded ? nullptr : d_off.as<uint64_t>(),
                                                       d_status.as<int32_t>(), fir, &r)
                        : corpus.fir_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W,
                                                  bin_len, stride, d_lv.as<x3_level>(), cap, padded ? nullptr : d_off.as<uint64_t>(),
                                                  d_status.as<int32_t>(), fir, &r);
          CHECK(e == x3::X3Error::Ok);
          CHECK(r.n_bad == 1 && r.first_bad == 9 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);
          std::vector<x3_level> lv(cap);
          std::vector<int32_t> st(W);
          CHECK(d_lv.download(lv.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
          CHECK(d_status.download(st.data(), 4 * W) == x3::X3Error::Ok);
          const size_t T = fir.taps.size();
          for (size_t w = 0; w < W; ++w) {
            CHECK(st[w] == (w == 9 ? X3_ERR_BAD_ARG : 0));
            const uint64_t base = padded ? w * stride : off[w];
            std::vector<x3_level> want(padded ? stride : rows[w], id);
            for (uint64_t r0 = 0; w != 9 && r0 < lens[w]; ++r0) {
              const uint64_t i = starts[w] + r0;
              if (i < T - 1) continue;
              int32_t acc = 0;
              for (size_t t = 0; t < T; ++t) acc += (int32_t)fir.taps[t] * (int32_t)wav[i - t];
              const int32_t y = std::min(std::max(acc >> fir.shift, -32768), 32767);   // (>> of a negative int: arithmetic here)
              x3_level& b = want[bin_len ? r0 / bin_len : 0];
              b.sum_sq += (uint64_t)((int64_t)y * y);
              b.sum += y;
              b.min = std::min(b.min, y);
              b.max = std::max(b.max, y);
              ++b.n;
            }
            for (size_t k = 0; k < want.size(); ++k) CHECK(same(lv[base + k], want[k]));
          }
          long long replays = -1;
          CHECK(x3_ctx_get_option(ctx.raw(), "last_range_levels_replays", &replays) == X3_OK && replays == 0);
        }
  // {1} and {1, -1}: the bytes of the Samples and the Diff form
  const LevelSignal signals[2] = {LevelSignal::Samples, LevelSignal::Diff};
  const Fir same_as[2] = {Fir{{1}, 0}, Fir{{1, -1}, 0}};
  {
    std::vector<uint64_t> rows, off;
    uint64_t stride, cap;
    layout(7, false, &rows, &off, &stride, &cap);
    x3::device::Buffer d_a(ctx, sizeof(x3_level) * cap), d_b(ctx, sizeof(x3_level) * cap), d_sa(ctx, 4 * W), d_sb(ctx, 4 * W);
    std::vector<x3_level> a(cap), b(cap);
    std::vector<int32_t> sa(W), sb(W);
    x3::device::RangeLevelsResult r;
    for (int k = 0; k < 2; ++k) {
      CHECK(x3::device::range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0, d_a.as<x3_level>(),
                                     cap, d_off.as<uint64_t>(), d_sa.as<int32_t>(), &r, signals[k]) == x3::X3Error::Ok);
      CHECK(x3::device::fir_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                         d_b.as<x3_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(), same_as[k], &r) ==
            x3::X3Error::Ok);
      CHECK(d_a.download(a.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok && d_b.download(b.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
      CHECK(d_sa.download(sa.data(), 4 * W) == x3::X3Error::Ok && d_sb.download(sb.data(), 4 * W) == x3::X3Error::Ok);
      // (a range that is refused keeps its records unwritten in both: compare what the layout says is written)
      for (size_t w = 0; w < W; ++w) {
        CHECK(sa[w] == sb[w]);
        CHECK(std::memcmp(&a[off[w]], &b[off[w]], sizeof(x3_level) * rows[w]) == 0);
      }
    }
    // refused: no taps, nine taps, shift 16, sum |c| = 32769 -- in front of every other argument
    for (const Fir& bad : {Fir{{}, 0}, Fir{{1, 1, 1, 1, 1, 1, 1, 1, 1}, 0}, Fir{{1}, 16}, Fir{{16384, -16384, 1}, 0}}) {
      CHECK(x3::device::fir_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                         d_b.as<x3_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
      CHECK(corpus.fir_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                    d_b.as<x3_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
    }
  }
  std::printf("test_fir_range_levels_hpp ok\n");
  return 0;
}
