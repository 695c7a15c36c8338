// Exercises x3::device::Tone with x3::device::tone_levels, x3::device::Corpus::tone_levels and x3::device::tone_power_levels
// of x3-rust_amd/host/x3.hpp (x3_tone_levels_dev, x3_corpus_tone_levels_dev, x3_tone_power_levels_dev): the records of a
// stream the encoder wrote are the sums of sample times cos and sin of the phase's table pair over the samples it was encoded
// from, with the samples' extremes and counts; a table of all (1, 0) gives the sum of the levels records; the adapter's
// records are the header's integers, in place and out of place; a corpus that holds the stream twice restarts the phase.
// Needs a GPU.   usage: test_tone_levels_hpp
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

// positions [a, b) of w against the oscillator
static x3_tone_level reference(const std::vector<int16_t>& w, size_t a, size_t b, uint32_t step, const std::vector<int16_t>& tab) {
  x3_tone_level r{0, 0, 32767, -32768, 0, 0};
  for (size_t i = a; i < std::min(b, w.size()); ++i) {
    const uint32_t ph = (uint32_t)((uint64_t)i * step);
    const uint32_t k = ph >> 22;
    const int32_t s = w[i];
    r.re += (int64_t)s * tab[2 * k];
    r.im += (int64_t)s * tab[2 * k + 1];
    r.min = std::min(r.min, s);
    r.max = std::max(r.max, s);
    ++r.n;
  }
  return r;
}

static uint64_t isqrt(uint64_t x) {
  uint64_t r = 0;
  while ((r + 1) * (r + 1) <= x) ++r;
  return r;
}

// the adapter's record by the header's definition
static x3_level power(const x3_tone_level& t) {
  if (t.n == 0) return x3_level{0, 0, 32767, -32768, 0, 0};
  int bits = 0;
  while (bits < 32 && (t.n >> bits)) ++bits;
  const int e = std::max(0, bits - 15);
  const int64_t a = t.re >> (15 + e), b = t.im >> (15 + e);   // (>> of a negative value: arithmetic here)
  const uint64_t P = (uint64_t)(a * a) + (uint64_t)(b * b);
  const uint64_t m = t.n >> e;
  const uint64_t ms = std::min<uint64_t>((2 * P / m) / m, 1ull << 30);
  const int32_t peak = (int32_t)std::min<uint64_t>(isqrt(2 * ms), 32767);
  return x3_level{ms * t.n, 0, -peak, peak, t.n, 0};
}

static bool same(const x3_tone_level& a, const x3_tone_level& b) {
  return a.re == b.re && a.im == b.im && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == 0;
}
static bool same(const x3_level& a, const x3_level& b) {
  return a.sum_sq == b.sum_sq && a.sum == b.sum && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == 0;
}

int main() {
  using x3::device::Tone;
  static_assert(sizeof(x3_level_tone) == 16, "x3_level_tone: two words and a pointer");
  static_assert(sizeof(x3_tone_level) == sizeof(x3_level), "x3_tone_level has x3_level's size");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 23457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7102, 0, n, wav.data()) == 0);
  for (size_t i = 9990; i < 10030; ++i) wav[i] = (i & 1) ? 32767 : -32768;   // full scale across a frame seam
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  CHECK(s.seg_blocks == 32 && s.n_frames == 3);
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const std::vector<int16_t> usual = Tone::usual_table();
  CHECK(usual.size() == 2048 && usual[0] == 32767 && usual[1] == 0 && usual[512] == 0 && usual[513] == 32767 && usual[1024] == -32767);
  std::vector<int16_t> ones(2048, 0);
  for (size_t k = 0; k < 1024; ++k) ones[2 * k] = 1;
  x3::device::Buffer d_usual(ctx, 4096), d_ones(ctx, 4096);
  CHECK(d_usual.upload(usual.data(), 4096) == x3::X3Error::Ok && d_ones.upload(ones.data(), 4096) == x3::X3Error::Ok);
  const uint64_t bin_len = 1001;
  const size_t n_bins = (n + bin_len - 1) / bin_len;
  x3::device::Buffer d_tl(ctx, sizeof(x3_tone_level) * n_bins), d_lv(ctx, sizeof(x3_level) * n_bins), d_st(ctx, 4 * s.n_frames);
  x3::device::WindowsResult r;
  std::vector<x3_tone_level> tl(n_bins);
  std::vector<x3_level> lv(n_bins), lv2(n_bins);
  const uint32_t steps[] = {0u, 1u << 30, 1u << 31, 0xFFFFFFFFu, 350898828u};
  for (uint32_t step : steps) {
    const Tone tone{step, d_usual.as<int16_t>()};
    CHECK(x3::device::tone_levels(ctx, s, params, so, bin_len, d_tl.as<x3_tone_level>(), n_bins, d_st.as<int32_t>(), &r, tone) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == s.n_frames && r.first_bad_status == 0);
    long long replays = -1;
    CHECK(x3_ctx_get_option(ctx.raw(), "last_levels_replays", &replays) == X3_OK && replays == 0);
    CHECK(d_tl.download(tl.data(), sizeof(x3_tone_level) * n_bins) == x3::X3Error::Ok);
    uint64_t counted = 0;
    for (size_t b = 0; b < n_bins; ++b) {
      CHECK(same(tl[b], reference(wav, b * bin_len, (b + 1) * bin_len, step, usual)));
      counted += tl[b].n;
    }
    CHECK(counted == n);
    // the adapter out of place, then in place
    CHECK(x3::device::tone_power_levels(ctx, d_tl.as<x3_tone_level>(), n_bins, d_lv.as<x3_level>()) == x3::X3Error::Ok);
    CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    CHECK(x3::device::tone_power_levels(ctx, d_tl.as<x3_tone_level>(), n_bins, reinterpret_cast<x3_level*>(d_tl.data())) == x3::X3Error::Ok);
    CHECK(d_tl.download(lv2.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    for (size_t b = 0; b < n_bins; ++b) CHECK(same(lv[b], power(tl[b])) && same(lv2[b], lv[b]));
    // one bin, no status array
    CHECK(x3::device::tone_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, tone) == x3::X3Error::Ok && r.n_bad == 0);
    CHECK(d_tl.download(tl.data(), sizeof(x3_tone_level)) == x3::X3Error::Ok && same(tl[0], reference(wav, 0, n, step, usual)));
  }
  std::vector<int32_t> st(s.n_frames, -1);
  CHECK(d_st.download(st.data(), 4 * s.n_frames) == x3::X3Error::Ok);
  for (int32_t v : st) CHECK(v == 0);
  // a table of all (1, 0): re is the sum of the levels records, im is 0, min, max and n are theirs
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r) == x3::X3Error::Ok);
  CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
  CHECK(x3::device::tone_levels(ctx, s, params, so, bin_len, d_tl.as<x3_tone_level>(), n_bins, nullptr, &r, Tone{12345u, d_ones.as<int16_t>()}) == x3::X3Error::Ok);
  CHECK(d_tl.download(tl.data(), sizeof(x3_tone_level) * n_bins) == x3::X3Error::Ok);
  for (size_t b = 0; b < n_bins; ++b)
    CHECK(tl[b].re == lv[b].sum && tl[b].im == 0 && tl[b].min == lv[b].min && tl[b].max == lv[b].max && tl[b].n == lv[b].n);
  // refused: no table, a table at an odd address, no bins; an adapter whose rows overlap without being the same
  const Tone good{350898828u, d_usual.as<int16_t>()};
  CHECK(x3::device::tone_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, Tone{1u, nullptr}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, Tone{1u, d_usual.as<int16_t>() + 1}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 0, nullptr, &r, good) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_power_levels(ctx, d_tl.as<x3_tone_level>(), 4, reinterpret_cast<x3_level*>(d_tl.data()) + 1) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_power_levels(ctx, d_tl.as<x3_tone_level>(), 0, d_lv.as<x3_level>()) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice: each entry starts at phase 0
  const std::vector<uint64_t> offs = {0, 0}, lens = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[0] == 0 && rf[1] == n_bins && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_tone_level) * rf[2]);
  std::vector<x3_tone_level> rows(rf[2]);
  CHECK(corpus.tone_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2] - 1, nullptr, &r, good) == x3::X3Error::BadArg);
  CHECK(corpus.tone_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2], nullptr, &r, Tone{1u, nullptr}) == x3::X3Error::BadArg);
  CHECK(corpus.tone_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2], nullptr, &r, good) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(r.first_bad == corpus.n_frames());
  CHECK(d_rows.download(rows.data(), sizeof(x3_tone_level) * rf[2]) == x3::X3Error::Ok);
  for (size_t b = 0; b < 2 * n_bins; ++b)
    CHECK(same(rows[b], reference(wav, (b % n_bins) * bin_len, (b % n_bins + 1) * bin_len, good.step, usual)));
  std::printf("test_tone_levels_hpp ok\n");
  return 0;
}
