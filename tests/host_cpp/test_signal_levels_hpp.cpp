// Exercises the signal argument of x3::device::levels and x3::device::Corpus::levels of x3-rust_amd/host/x3.hpp
// (x3_signal_levels_dev, x3_corpus_signal_levels_dev): with LevelSignal::Diff the records of a stream the encoder wrote are
// the sums, extremes and counts of the clamped first difference of the samples it was encoded from, frame seams included,
// and a corpus that holds the stream twice has no difference across its entries; LevelSignal::Samples and the default are
// the records of the samples.  Needs a GPU.   usage: test_signal_levels_hpp
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

// positions [a, b) of w: the samples, or (diff) the clamped difference to the sample in front, none at position 0
static x3_level reference(const std::vector<int16_t>& w, size_t a, size_t b, bool diff) {
  x3_level r{0, 0, 32767, -32768, 0, 0};
  for (size_t i = a; i < std::min(b, w.size()); ++i) {
    if (diff && i == 0) continue;
    const int32_t s = diff ? std::min(std::max((int32_t)w[i] - (int32_t)w[i - 1], -32768), 32767) : (int32_t)w[i];
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
  using x3::device::LevelSignal;
  static_assert((int)LevelSignal::Samples == X3_LEVEL_SIGNAL_SAMPLES && (int)LevelSignal::Diff == X3_LEVEL_SIGNAL_DIFF, "the C ABI's values");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 43457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7101, 0, n, wav.data()) == 0);
  for (size_t i = 20000; i < 20040; ++i) wav[i] = (i & 1) ? 32767 : -32768;   // full-scale alternation across a frame seam
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  CHECK(s.seg_blocks == 32 && s.n_frames == 5);
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const uint64_t bin_len = 1001;
  const size_t n_bins = (n + bin_len - 1) / bin_len;
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * n_bins), d_st(ctx, 4 * s.n_frames);
  x3::device::WindowsResult r;
  std::vector<x3_level> lv(n_bins), plain(n_bins);
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, d_st.as<int32_t>(), &r, LevelSignal::Diff) ==
        x3::X3Error::Ok);
  CHECK(r.n_bad == 0 && r.first_bad == s.n_frames && r.first_bad_status == 0);
  long long replays = -1;
  CHECK(x3_ctx_get_option(ctx.raw(), "last_levels_replays", &replays) == X3_OK && replays == 0);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
  uint64_t counted = 0;
  for (size_t b = 0; b < n_bins; ++b) {
    CHECK(same(lv[b], reference(wav, b * bin_len, (b + 1) * bin_len, true)));
    counted += lv[b].n;
  }
  CHECK(counted == n - 1);
  CHECK(lv[20000 / bin_len].min == -32768 && lv[20000 / bin_len].max == 32767);
  std::vector<int32_t> st(s.n_frames, -1);
  CHECK(d_st.download(st.data(), 4 * s.n_frames) == x3::X3Error::Ok);
  for (int32_t v : st) CHECK(v == 0);
  // Samples, and the default: the records of the samples, byte for byte
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r, LevelSignal::Samples) == x3::X3Error::Ok);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r) == x3::X3Error::Ok);
  CHECK(d_lv.download(plain.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
  CHECK(std::memcmp(lv.data(), plain.data(), sizeof(x3_level) * n_bins) == 0);
  for (size_t b = 0; b < n_bins; ++b) CHECK(same(plain[b], reference(wav, b * bin_len, (b + 1) * bin_len, false)));
  // one bin, no status array
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, LevelSignal::Diff) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level)) == x3::X3Error::Ok && same(lv[0], reference(wav, 0, n, true)));
  // refused: no bins; a signal the library does not know
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 0, nullptr, &r, LevelSignal::Diff) == x3::X3Error::BadArg);
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r, static_cast<LevelSignal>(2)) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice: each entry starts without a difference
  const std::vector<uint64_t> offs = {0, 0}, lens = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[0] == 0 && rf[1] == n_bins && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_level) * rf[2]);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2] - 1, nullptr, &r, LevelSignal::Diff) == x3::X3Error::BadArg);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r, LevelSignal::Diff) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(r.first_bad == corpus.n_frames());
  std::vector<x3_level> rows(rf[2]);
  CHECK(d_rows.download(rows.data(), sizeof(x3_level) * rf[2]) == x3::X3Error::Ok);
  for (size_t b = 0; b < 2 * n_bins; ++b) CHECK(same(rows[b], reference(wav, (b % n_bins) * bin_len, (b % n_bins + 1) * bin_len, true)));
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(d_rows.download(rows.data(), sizeof(x3_level) * rf[2]) == x3::X3Error::Ok);
  for (size_t b = 0; b < 2 * n_bins; ++b) CHECK(same(rows[b], plain[b % n_bins]));
  std::printf("test_signal_levels_hpp ok\n");
  return 0;
}
