// Exercises x3::device::Fir with x3::device::levels and x3::device::Corpus::levels of x3-rust_amd/host/x3.hpp
// (x3_fir_levels_dev, x3_corpus_fir_levels_dev): the records of a stream the encoder wrote are the sums, extremes and counts
// of y[i] = clamp((sum of taps[t] * x[i - t]) >> shift) over the samples it was encoded from, counted from position T - 1 on
// and across frame seams; {1} and {1, -1} are the records of LevelSignal::Samples and LevelSignal::Diff byte for byte; a
// corpus that holds the stream twice has no history across its entries.  Needs a GPU.   usage: test_fir_levels_hpp
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

// positions [a, b) of w behind the filter, none in front of position T - 1
static x3_level reference(const std::vector<int16_t>& w, size_t a, size_t b, const x3::device::Fir& fir) {
  x3_level r{0, 0, 32767, -32768, 0, 0};
  const size_t T = fir.taps.size();
  for (size_t i = std::max(a, T - 1); i < std::min(b, w.size()); ++i) {
    int32_t acc = 0;
    for (size_t t = 0; t < T; ++t) acc += (int32_t)fir.taps[t] * (int32_t)w[i - t];
    const int32_t s = std::min(std::max(acc >> fir.shift, -32768), 32767);   // (>> of a negative int: arithmetic here)
    r.sum_sq += (uint64_t)((int64_t)s * s);
    r.sum += s;
    r.min = std::min(r.min, s);
    r.max = std::max(r.max, s);
    ++r.n;
  }
  return r;
}

static bool same(const x3_level& a, const x3_level& b) {
  return a.sum_sq == b.sum_sq && a.sum == b.sum && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == 0;
}

int main() {
  using x3::device::Fir;
  using x3::device::LevelSignal;
  static_assert(sizeof(x3_level_fir) == 24, "x3_level_fir: two words and eight taps");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 23457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7102, 0, n, wav.data()) == 0);
  for (size_t i = 9990; i < 10030; ++i) wav[i] = (i & 1) ? 32767 : -32768;   // full-scale alternation across a frame seam
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  CHECK(s.seg_blocks == 32 && s.n_frames == 3);
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const uint64_t bin_len = 1001;
  const size_t n_bins = (n + bin_len - 1) / bin_len;
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * n_bins), d_st(ctx, 4 * s.n_frames);
  x3::device::WindowsResult r;
  std::vector<x3_level> lv(n_bins), other(n_bins);
  const std::vector<Fir> firs = {Fir{{1, -2, 1}, 0}, Fir{{1, 0, -1}, 0}, Fir{{1, 1, 1, 1}, 2}, Fir{{16384, -16384}, 0},
                                 Fir{{-3000, 9000, -200, 7, 5000, -8000, 1, 6560}, 7}, Fir{{0, 0, 0, 0, 0, 0, 0, 1}, 0}};
  for (const Fir& fir : firs) {
    CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, d_st.as<int32_t>(), &r, fir) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == s.n_frames && r.first_bad_status == 0);
    long long replays = -1;
    CHECK(x3_ctx_get_option(ctx.raw(), "last_levels_replays", &replays) == X3_OK && replays == 0);
    CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    uint64_t counted = 0;
    for (size_t b = 0; b < n_bins; ++b) {
      CHECK(same(lv[b], reference(wav, b * bin_len, (b + 1) * bin_len, fir)));
      counted += lv[b].n;
    }
    CHECK(counted == n - fir.taps.size() + 1);
    // one bin, no status array
    CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, fir) == x3::X3Error::Ok && r.n_bad == 0);
    CHECK(d_lv.download(lv.data(), sizeof(x3_level)) == x3::X3Error::Ok && same(lv[0], reference(wav, 0, n, fir)));
  }
  std::vector<int32_t> st(s.n_frames, -1);
  CHECK(d_st.download(st.data(), 4 * s.n_frames) == x3::X3Error::Ok);
  for (int32_t v : st) CHECK(v == 0);
  // the two identities, byte for byte
  const LevelSignal signals[2] = {LevelSignal::Samples, LevelSignal::Diff};
  const Fir same_as[2] = {Fir{{1}, 0}, Fir{{1, -1}, 0}};
  for (int k = 0; k < 2; ++k) {
    CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r, signals[k]) == x3::X3Error::Ok);
    CHECK(d_lv.download(other.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r, same_as[k]) == x3::X3Error::Ok);
    CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    CHECK(std::memcmp(lv.data(), other.data(), sizeof(x3_level) * n_bins) == 0);
  }
  // refused: no taps, nine taps, shift 16, sum |c| = 32769, no bins
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, Fir{{}, 0}) == x3::X3Error::BadArg);
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, Fir{{1, 1, 1, 1, 1, 1, 1, 1, 1}, 0}) == x3::X3Error::BadArg);
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, Fir{{1}, 16}) == x3::X3Error::BadArg);
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, Fir{{16384, -16384, 1}, 0}) == x3::X3Error::BadArg);
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 0, nullptr, &r, firs[0]) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice: each entry starts without history
  const std::vector<uint64_t> offs = {0, 0}, lens = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[0] == 0 && rf[1] == n_bins && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_level) * rf[2]);
  std::vector<x3_level> rows(rf[2]);
  const Fir& f8 = firs[4];
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2] - 1, nullptr, &r, f8) == x3::X3Error::BadArg);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r, Fir{{1}, 16}) == x3::X3Error::BadArg);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r, f8) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(r.first_bad == corpus.n_frames());
  CHECK(d_rows.download(rows.data(), sizeof(x3_level) * rf[2]) == x3::X3Error::Ok);
  for (size_t b = 0; b < 2 * n_bins; ++b) CHECK(same(rows[b], reference(wav, (b % n_bins) * bin_len, (b % n_bins + 1) * bin_len, f8)));
  std::printf("test_fir_levels_hpp ok\n");
  return 0;
}
