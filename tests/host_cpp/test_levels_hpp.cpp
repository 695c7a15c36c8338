// Exercises x3::device::levels and x3::device::Corpus::levels of x3-rust_amd/host/x3.hpp (x3_levels_dev,
// x3_corpus_levels_rows, x3_corpus_levels_dev): the records of a stream the encoder wrote are the sums, extremes and counts
// of the samples it was encoded from, per bin and for a corpus that holds it twice.  Needs a GPU.   usage: test_levels_hpp
#include <algorithm>
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

static x3_level reference(const std::vector<int16_t>& w, size_t a, size_t b) {
  x3_level r{0, 0, 32767, -32768, 0, 0};
  for (size_t i = a; i < std::min(b, w.size()); ++i) {
    const int32_t s = w[i];
    r.sum_sq += (uint64_t)(s * s);
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
  static_assert(sizeof(x3_level) == 32, "x3_level is 32 bytes");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 43457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7101, 0, n, wav.data()) == 0);
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
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
  CHECK(r.n_bad == 0 && r.first_bad == s.n_frames && r.first_bad_status == 0);
  long long replays = -1;
  CHECK(x3_ctx_get_option(ctx.raw(), "last_levels_replays", &replays) == X3_OK && replays == 0);
  std::vector<x3_level> lv(n_bins);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
  for (size_t b = 0; b < n_bins; ++b) CHECK(same(lv[b], reference(wav, b * bin_len, (b + 1) * bin_len)));
  std::vector<int32_t> st(s.n_frames, -1);
  CHECK(d_st.download(st.data(), 4 * s.n_frames) == x3::X3Error::Ok);
  for (int32_t v : st) CHECK(v == 0);
  // one bin, no status array
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 1, nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level)) == x3::X3Error::Ok && same(lv[0], reference(wav, 0, n)));
  // refused: no bins
  CHECK(x3::device::levels(ctx, s, params, so, 0, d_lv.as<x3_level>(), 0, nullptr, &r) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice
  const std::vector<uint64_t> offs = {0, 0}, lens = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[0] == 0 && rf[1] == n_bins && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_level) * rf[2]);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2] - 1, nullptr, &r) == x3::X3Error::BadArg);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(r.first_bad == corpus.n_frames());
  std::vector<x3_level> rows(rf[2]);
  CHECK(d_rows.download(rows.data(), sizeof(x3_level) * rf[2]) == x3::X3Error::Ok);
  for (size_t b = 0; b < 2 * n_bins; ++b) CHECK(same(rows[b], reference(wav, (b % n_bins) * bin_len, (b % n_bins + 1) * bin_len)));
  std::printf("test_levels_hpp ok\n");
  return 0;
}
