// Exercises x3::device::tone_bank_range_levels and x3::device::Corpus::tone_bank_range_levels of x3-rust_amd/host/x3.hpp
// (x3_tone_bank_range_levels_dev / x3_corpus_tone_bank_range_levels_dev) on the base stream of tests/test_gpu_range_levels.py:
// 2 137 samples in frames of 400 (block length 20, 20 blocks a frame) with a walk-built index.  The mirror forwards the bank and
// the PLANE STRIDE: plane t of the records lies at d_levels + t * rows_cap and is, byte for byte, what
// x3::device::tone_range_levels writes for Tone{steps[t], table} into a buffer of rows_cap records, packed and padded, with
// rows_cap above the rows drawn -- the records behind them keep the caller's bytes in every plane -- and against a loop over
// the positions.  A corpus that holds the stream twice: the phase is 0 at every entry in every plane.  Needs a GPU.
// usage: test_tone_bank_range_levels_hpp
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

static bool same(const x3_tone_level& a, const x3_tone_level& b) {
  return a.re == b.re && a.im == b.im && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == b.reserved;
}

int main() {
  using x3::device::Tone;
  using x3::device::ToneBank;
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
  const std::vector<uint64_t> starts = {0, 399, 2000, 2137, 400, 5, 81, 800, 0, 1, 401, 82, 1024};
  const std::vector<uint32_t> lens = {400, 3, 137, 0, 400, 0, 700, 1, 2137, 2137, 9, 9, 400};     // (1, 2137) runs off the end
  const size_t W = starts.size();
  x3::device::Buffer d_starts(ctx, 8 * W), d_lens(ctx, 4 * W), d_status(ctx, 4 * W), d_status1(ctx, 4 * W), d_off(ctx, 8 * (W + 1)),
      d_off1(ctx, 8 * (W + 1));
  CHECK(d_starts.upload(starts.data(), 8 * W) == x3::X3Error::Ok && d_lens.upload(lens.data(), 4 * W) == x3::X3Error::Ok);
  x3::device::Corpus corpus;   // two entries: the stream itself, twice
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, {0, 0}, {s.len, s.len}, 0, params, 4, true) == x3::X3Error::Ok);
  std::vector<uint32_t> entries(W);
  for (size_t w = 0; w < W; ++w) entries[w] = (uint32_t)(w & 1);
  x3::device::Buffer d_entries(ctx, 4 * W);
  CHECK(d_entries.upload(entries.data(), 4 * W) == x3::X3Error::Ok);
  const std::vector<int16_t> usual = Tone::usual_table();
  x3::device::Buffer d_usual(ctx, 4096);
  CHECK(d_usual.upload(usual.data(), 4096) == x3::X3Error::Ok);
  const std::vector<uint32_t> all = {350898828u, 0u, 1u << 30, 350898828u, 1u << 31, 0xFFFFFFFFu, 2718281829u, 1u << 22};
  const x3_tone_level id{0, 0, 32767, -32768, 0, 0};
  for (size_t K : {1u, 2u, 3u, 4u, 5u, 8u})
    for (int form = 0; form < 2; ++form)
      for (uint64_t bin_len : {(uint64_t)0, (uint64_t)7, (uint64_t)400})
        for (int padded = 0; padded < 2; ++padded) {
          std::vector<uint64_t> rows(W), off(W + 1, 0);
          uint64_t most = 1;
          for (size_t w = 0; w < W; ++w) {
            rows[w] = bin_len ? std::max<uint64_t>(1, (lens[w] + bin_len - 1) / bin_len) : 1;
            off[w + 1] = off[w] + rows[w];
            most = std::max(most, rows[w]);
          }
          const uint64_t stride = padded ? most : 0, drawn = padded ? most * W : off[W], cap = drawn + 3;   // three records nobody's
          const ToneBank bank{std::vector<uint32_t>(all.begin(), all.begin() + K), d_usual.as<int16_t>()};
          CHECK(bank.ok() && bank.c_bank().n_tones == K);
          std::vector<x3_tone_level> fill(K * cap), lv(K * cap), one(cap);
          std::memset(fill.data(), 0x5A, sizeof(x3_tone_level) * K * cap);
          x3::device::Buffer d_lv(ctx, sizeof(x3_tone_level) * K * cap), d_one(ctx, sizeof(x3_tone_level) * cap);
          CHECK(d_lv.upload(fill.data(), sizeof(x3_tone_level) * K * cap) == x3::X3Error::Ok);
          x3::device::RangeLevelsResult r, r1;
          const x3::X3Error e =
              form == 0 ? x3::device::tone_bank_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W,
                                                             bin_len, stride, d_lv.as<x3_tone_level>(), cap,
                                                             padded ? nullptr : d_off.as<uint64_t>(), d_status.as<int32_t>(), bank, &r)
                        : corpus.tone_bank_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W,
                                                        bin_len, stride, d_lv.as<x3_tone_level>(), cap,
                                                        padded ? nullptr : d_off.as<uint64_t>(), d_status.as<int32_t>(), bank, &r);
          CHECK(e == x3::X3Error::Ok);
          CHECK(r.n_bad == 1 && r.first_bad == 9 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);   // one plane's
          std::vector<int32_t> st(W), st1(W);
          CHECK(d_lv.download(lv.data(), sizeof(x3_tone_level) * K * cap) == x3::X3Error::Ok);
          CHECK(d_status.download(st.data(), 4 * W) == x3::X3Error::Ok);
          for (size_t t = 0; t < K; ++t) {
            const x3_tone_level* plane = lv.data() + t * cap;                  // the plane stride is rows_cap
            // ... the single call's bytes, into a buffer of rows_cap records filled the same way
            CHECK(d_one.upload(fill.data(), sizeof(x3_tone_level) * cap) == x3::X3Error::Ok);
            const Tone tone{all[t], d_usual.as<int16_t>()};
            const x3::X3Error e1 =
                form == 0 ? x3::device::tone_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, bin_len,
                                                          stride, d_one.as<x3_tone_level>(), cap, padded ? nullptr : d_off1.as<uint64_t>(),
                                                          d_status1.as<int32_t>(), tone, &r1)
                          : corpus.tone_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W,
                                                     bin_len, stride, d_one.as<x3_tone_level>(), cap,
                                                     padded ? nullptr : d_off1.as<uint64_t>(), d_status1.as<int32_t>(), tone, &r1);
            CHECK(e1 == x3::X3Error::Ok && r1.n_bad == r.n_bad && r1.first_bad == r.first_bad && r1.total_rows == r.total_rows);
            CHECK(d_one.download(one.data(), sizeof(x3_tone_level) * cap) == x3::X3Error::Ok);
            CHECK(std::memcmp(one.data(), plane, sizeof(x3_tone_level) * cap) == 0);
            CHECK(d_status1.download(st1.data(), 4 * W) == x3::X3Error::Ok && st1 == st);
            // ... and a loop over the positions
            for (size_t w = 0; w < W; ++w) {
              CHECK(st[w] == (w == 9 ? X3_ERR_BAD_ARG : 0));
              const uint64_t base = padded ? w * stride : off[w];
              std::vector<x3_tone_level> want(padded ? stride : rows[w], id);
              for (uint64_t r0 = 0; w != 9 && r0 < lens[w]; ++r0) {
                const uint64_t i = starts[w] + r0;                     // the position in the stream, or in either entry
                const uint32_t k = (uint32_t)(i * (uint64_t)all[t]) >> 22;
                const int32_t x = wav[i];
                x3_tone_level& b = want[bin_len ? r0 / bin_len : 0];
                b.re += (int64_t)x * usual[2 * k];
                b.im += (int64_t)x * usual[2 * k + 1];
                b.min = std::min(b.min, x);
                b.max = std::max(b.max, x);
                ++b.n;
              }
              for (size_t k = 0; k < want.size(); ++k) CHECK(same(plane[base + k], want[k]));
            }
            CHECK(std::memcmp(plane + drawn, fill.data(), sizeof(x3_tone_level) * 3) == 0);   // untouched, in every plane
          }
          long long replays = -1;
          CHECK(x3_ctx_get_option(ctx.raw(), "last_range_levels_replays", &replays) == X3_OK && replays == 0);
        }
  // refused in front of every other argument (no ranges): no steps, nine steps, no table, a table at an odd address
  {
    x3::device::Buffer d_lv(ctx, sizeof(x3_tone_level) * 8 * 16);
    x3::device::RangeLevelsResult r;
    std::vector<uint32_t> nine(9, 1u);
    for (const ToneBank& bad : {ToneBank{{}, d_usual.as<int16_t>()}, ToneBank{nine, d_usual.as<int16_t>()}, ToneBank{{1u, 2u}, nullptr},
                                ToneBank{{1u, 2u}, d_usual.as<int16_t>() + 1}}) {
      CHECK(x3::device::tone_bank_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), 0, 7, 1,
                                               d_lv.as<x3_tone_level>(), 16, nullptr, d_status.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
      CHECK(corpus.tone_bank_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), 0, 7, 1,
                                          d_lv.as<x3_tone_level>(), 16, nullptr, d_status.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
    }
    const ToneBank good{{350898828u, 1u << 30, 2718281829u}, d_usual.as<int16_t>()};
    CHECK(x3::device::tone_bank_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), 0, 7, 1,
                                             d_lv.as<x3_tone_level>(), 16, nullptr, d_status.as<int32_t>(), good, &r) == x3::X3Error::BadArg);
    // n_tones * rows_cap above 2^31 - 1, by argument only
    CHECK(x3::device::tone_bank_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                             d_lv.as<x3_tone_level>(), 715827883ull, d_off.as<uint64_t>(), d_status.as<int32_t>(), good,
                                             &r) == x3::X3Error::BadArg);
    x3_level_tone_bank raw = good.c_bank();
    raw.reserved = 1;
    CHECK(x3_corpus_tone_bank_range_levels_dev(ctx.raw(), corpus.raw(), d_entries.as<uint32_t>(), d_starts.as<uint64_t>(),
                                               d_lens.as<uint32_t>(), 1, 0, 0, d_lv.as<x3_tone_level>(), 16, d_off.as<uint64_t>(),
                                               d_status.as<int32_t>(), &raw) == X3_ERR_BAD_ARG);
  }
  std::printf("test_tone_bank_range_levels_hpp ok\n");
  return 0;
}
