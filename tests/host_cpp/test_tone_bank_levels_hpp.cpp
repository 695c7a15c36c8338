// Exercises x3::device::ToneBank with x3::device::tone_bank_levels and x3::device::Corpus::tone_bank_levels of
// x3-rust_amd/host/x3.hpp (x3_tone_bank_levels_dev, x3_corpus_tone_bank_levels_dev): plane t of the records of a stream the
// encoder wrote is the sums of sample times cos and sin of the phase's table pair at steps[t] over the samples it was encoded
// from, with the samples' extremes and counts -- and byte for byte what x3::device::tone_levels writes for that step; all
// planes go through the adapter in one launch; a corpus that holds the stream twice restarts the phase in every plane.
// Needs a GPU.   usage: test_tone_bank_levels_hpp
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

static bool same(const x3_tone_level& a, const x3_tone_level& b) {
  return a.re == b.re && a.im == b.im && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == 0;
}

int main() {
  using x3::device::Tone;
  using x3::device::ToneBank;
  static_assert(X3_TONE_BANK_MAX == 8, "eight oscillators at most");
  static_assert(sizeof(x3_level_tone_bank) == 48, "x3_level_tone_bank: two words, a pointer, eight steps");
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
  x3::device::Buffer d_usual(ctx, 4096);
  CHECK(d_usual.upload(usual.data(), 4096) == x3::X3Error::Ok);
  const uint64_t bin_len = 1001;
  const size_t n_bins = (n + bin_len - 1) / bin_len;
  const std::vector<uint32_t> all = {350898828u, 0u, 1u << 30, 350898828u, 1u << 31, 0xFFFFFFFFu, 2718281829u, 1u};
  x3::device::Buffer d_tl(ctx, sizeof(x3_tone_level) * n_bins * 8), d_one(ctx, sizeof(x3_tone_level) * n_bins);
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * n_bins * 8), d_st(ctx, 4 * s.n_frames);
  x3::device::WindowsResult r;
  std::vector<x3_tone_level> tl(n_bins * 8), one(n_bins);
  for (size_t k : {1u, 2u, 3u, 4u, 5u, 8u}) {
    const ToneBank bank{std::vector<uint32_t>(all.begin(), all.begin() + k), d_usual.as<int16_t>()};
    CHECK(bank.ok() && bank.c_bank().n_tones == k && bank.c_bank().reserved == 0);
    CHECK(x3::device::tone_bank_levels(ctx, s, params, so, bin_len, d_tl.as<x3_tone_level>(), n_bins, d_st.as<int32_t>(), &r, bank) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == s.n_frames && r.first_bad_status == 0);
    long long replays = -1;
    CHECK(x3_ctx_get_option(ctx.raw(), "last_levels_replays", &replays) == X3_OK && replays == 0);
    CHECK(d_tl.download(tl.data(), sizeof(x3_tone_level) * n_bins * k) == x3::X3Error::Ok);
    for (size_t t = 0; t < k; ++t) {
      uint64_t counted = 0;
      for (size_t b = 0; b < n_bins; ++b) {
        CHECK(same(tl[t * n_bins + b], reference(wav, b * bin_len, (b + 1) * bin_len, all[t], usual)));
        counted += tl[t * n_bins + b].n;
      }
      CHECK(counted == n);
      // ... and the single call's bytes
      CHECK(x3::device::tone_levels(ctx, s, params, so, bin_len, d_one.as<x3_tone_level>(), n_bins, nullptr, &r, Tone{all[t], d_usual.as<int16_t>()}) == x3::X3Error::Ok);
      CHECK(d_one.download(one.data(), sizeof(x3_tone_level) * n_bins) == x3::X3Error::Ok);
      CHECK(std::memcmp(one.data(), tl.data() + t * n_bins, sizeof(x3_tone_level) * n_bins) == 0);
    }
    // all planes through the adapter in one launch: plane by plane the single plane's records
    CHECK(x3::device::tone_power_levels(ctx, d_tl.as<x3_tone_level>(), k * n_bins, d_lv.as<x3_level>()) == x3::X3Error::Ok);
    std::vector<x3_level> lv(k * n_bins), lv1(n_bins);
    CHECK(d_lv.download(lv.data(), sizeof(x3_level) * n_bins * k) == x3::X3Error::Ok);
    CHECK(x3::device::tone_power_levels(ctx, d_one.as<x3_tone_level>(), n_bins, reinterpret_cast<x3_level*>(d_one.data())) == x3::X3Error::Ok);
    CHECK(d_one.download(lv1.data(), sizeof(x3_level) * n_bins) == x3::X3Error::Ok);
    CHECK(std::memcmp(lv1.data(), lv.data() + (k - 1) * n_bins, sizeof(x3_level) * n_bins) == 0);
    // one bin, no status array
    CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, bank) == x3::X3Error::Ok && r.n_bad == 0);
    CHECK(d_tl.download(tl.data(), sizeof(x3_tone_level) * k) == x3::X3Error::Ok);
    for (size_t t = 0; t < k; ++t) CHECK(same(tl[t], reference(wav, 0, n, all[t], usual)));
  }
  std::vector<int32_t> st(s.n_frames, -1);
  CHECK(d_st.download(st.data(), 4 * s.n_frames) == x3::X3Error::Ok);
  for (int32_t v : st) CHECK(v == 0);
  // refused: no steps, nine steps, no table, a table at an odd address, no bins
  const ToneBank good{{350898828u, 1u << 30, 2718281829u}, d_usual.as<int16_t>()};
  std::vector<uint32_t> nine(9, 1u);
  CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, ToneBank{{}, d_usual.as<int16_t>()}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, ToneBank{nine, d_usual.as<int16_t>()}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, ToneBank{{1u, 2u}, nullptr}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &r, ToneBank{{1u, 2u}, d_usual.as<int16_t>() + 1}) == x3::X3Error::BadArg);
  CHECK(x3::device::tone_bank_levels(ctx, s, params, so, 0, d_tl.as<x3_tone_level>(), 0, nullptr, &r, good) == x3::X3Error::BadArg);
  x3_level_tone_bank raw = good.c_bank();
  raw.reserved = 1;
  CHECK(x3_tone_bank_levels_dev(ctx.raw(), s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(), so.as<uint64_t>(), s.n_frames,
                                &cp, nullptr, 0, 0, d_tl.as<x3_tone_level>(), 1, nullptr, &raw) == X3_ERR_BAD_ARG);
  // a corpus that holds the stream twice: each entry starts at phase 0 in every plane, the plane stride is the corpus's rows
  const std::vector<uint64_t> offs = {0, 0}, lens = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[0] == 0 && rf[1] == n_bins && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_tone_level) * rf[2] * 3);
  std::vector<x3_tone_level> rows(rf[2] * 3);
  CHECK(corpus.tone_bank_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2] - 1, nullptr, &r, good) == x3::X3Error::BadArg);
  CHECK(corpus.tone_bank_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2], nullptr, &r, ToneBank{{1u, 2u}, nullptr}) == x3::X3Error::BadArg);
  CHECK(corpus.tone_bank_levels(ctx, bin_len, d_rows.as<x3_tone_level>(), rf[2], nullptr, &r, good) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(r.first_bad == corpus.n_frames());
  CHECK(d_rows.download(rows.data(), sizeof(x3_tone_level) * rf[2] * 3) == x3::X3Error::Ok);
  for (size_t t = 0; t < 3; ++t)
    for (size_t b = 0; b < 2 * n_bins; ++b)
      CHECK(same(rows[t * rf[2] + b], reference(wav, (b % n_bins) * bin_len, (b % n_bins + 1) * bin_len, good.steps[t], usual)));
  std::printf("test_tone_bank_levels_hpp ok\n");
  return 0;
}
