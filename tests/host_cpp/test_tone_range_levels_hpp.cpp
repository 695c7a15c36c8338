// Exercises x3::device::tone_range_levels and x3::device::Corpus::tone_range_levels of x3-rust_amd/host/x3.hpp
// (x3_tone_range_levels_dev / x3_corpus_tone_range_levels_dev) on the base stream of tests/test_gpu_range_levels.py: 2 137
// samples in frames of 400 (block length 20, 20 blocks a frame) with a walk-built index.  Packed and padded records at three
// bin lengths and five steps against a loop over the positions: position i of the STREAM has the phase (i * step) mod 2^32
// wherever the range begins (ranges that start at a frame's first sample, one either side of it, inside a frame and at a
// stretch's first sample).  A corpus that holds the stream twice: ranges of the second entry have the first's records, the
// phase is 0 at every entry.  A table of all (1, 0): the sums of LevelSignal::Samples.  The adapter takes the records packed
// and padded.  Needs a GPU.
// usage: test_tone_range_levels_hpp
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
  x3::device::Buffer d_starts(ctx, 8 * W), d_lens(ctx, 4 * W), d_status(ctx, 4 * W), d_off(ctx, 8 * (W + 1));
  CHECK(d_starts.upload(starts.data(), 8 * W) == x3::X3Error::Ok && d_lens.upload(lens.data(), 4 * W) == x3::X3Error::Ok);
  // two corpus entries: the stream itself, twice
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, {0, 0}, {s.len, s.len}, 0, params, 4, true) == x3::X3Error::Ok);
  std::vector<uint32_t> entries(W);
  for (size_t w = 0; w < W; ++w) entries[w] = (uint32_t)(w & 1);
  x3::device::Buffer d_entries(ctx, 4 * W);
  CHECK(d_entries.upload(entries.data(), 4 * W) == x3::X3Error::Ok);
  const std::vector<int16_t> usual = Tone::usual_table();
  std::vector<int16_t> ones(2048, 0), odd(2048);
  for (size_t k = 0; k < 1024; ++k) ones[2 * k] = 1;
  for (size_t k = 0; k < 2048; ++k) odd[k] = (int16_t)((k * 40503u + 977u) & 0xFFFFu);     // any contents are legal
  x3::device::Buffer d_usual(ctx, 4096), d_ones(ctx, 4096), d_odd(ctx, 4096);
  CHECK(d_usual.upload(usual.data(), 4096) == x3::X3Error::Ok && d_ones.upload(ones.data(), 4096) == x3::X3Error::Ok &&
        d_odd.upload(odd.data(), 4096) == x3::X3Error::Ok);
  const x3_tone_level id{0, 0, 32767, -32768, 0, 0};
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
  const uint32_t steps[] = {0u, 350898828u, 1u << 31, 0xFFFFFFFFu, 1u << 22};
  for (uint32_t step : steps)
    for (int form = 0; form < 2; ++form)
      for (uint64_t bin_len : {(uint64_t)0, (uint64_t)7, (uint64_t)400})
        for (int padded = 0; padded < 2; ++padded) {
          const bool use_odd = step == 0xFFFFFFFFu;
          const std::vector<int16_t>& tab = use_odd ? odd : usual;
          const Tone tone{step, (use_odd ? d_odd : d_usual).as<int16_t>()};
          std::vector<uint64_t> rows, off;
          uint64_t stride, cap;
          layout(bin_len, padded, &rows, &off, &stride, &cap);
          x3::device::Buffer d_lv(ctx, sizeof(x3_tone_level) * cap);
          x3::device::RangeLevelsResult r;
          const x3::X3Error e =
              form == 0 ? x3::device::tone_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, bin_len,
                                                        stride, d_lv.as<x3_tone_level>(), cap, padded ? nullptr : d_off.as<uint64_t>(),
                                                        d_status.as<int32_t>(), tone, &r)
                        : corpus.tone_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W,
                                                   bin_len, stride, d_lv.as<x3_tone_level>(), cap,
                                                   padded ? nullptr : d_off.as<uint64_t>(), d_status.as<int32_t>(), tone, &r);
          CHECK(e == x3::X3Error::Ok);
          CHECK(r.n_bad == 1 && r.first_bad == 9 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);
          std::vector<x3_tone_level> lv(cap);
          std::vector<int32_t> st(W);
          CHECK(d_lv.download(lv.data(), sizeof(x3_tone_level) * cap) == x3::X3Error::Ok);
          CHECK(d_status.download(st.data(), 4 * W) == x3::X3Error::Ok);
          for (size_t w = 0; w < W; ++w) {
            CHECK(st[w] == (w == 9 ? X3_ERR_BAD_ARG : 0));
            const uint64_t base = padded ? w * stride : off[w];
            std::vector<x3_tone_level> want(padded ? stride : rows[w], id);
            for (uint64_t r0 = 0; w != 9 && r0 < lens[w]; ++r0) {
              const uint64_t i = starts[w] + r0;                     // the position in the stream, or in either entry
              const uint32_t k = (uint32_t)(i * (uint64_t)step) >> 22;
              const int32_t x = wav[i];
              x3_tone_level& b = want[bin_len ? r0 / bin_len : 0];
              b.re += (int64_t)x * tab[2 * k];
              b.im += (int64_t)x * tab[2 * k + 1];
              b.min = std::min(b.min, x);
              b.max = std::max(b.max, x);
              ++b.n;
            }
            for (size_t k = 0; k < want.size(); ++k) CHECK(same(lv[base + k], want[k]));
          }
          long long replays = -1;
          CHECK(x3_ctx_get_option(ctx.raw(), "last_range_levels_replays", &replays) == X3_OK && replays == 0);
          // the adapter takes the records as they lie, packed or padded: every record's n is kept, an empty one is the identity
          x3::device::Buffer d_band(ctx, sizeof(x3_level) * cap);
          std::vector<x3_level> band(cap);
          CHECK(x3::device::tone_power_levels(ctx, d_lv.as<x3_tone_level>(), cap, d_band.as<x3_level>()) == x3::X3Error::Ok);
          CHECK(d_band.download(band.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok);
          for (size_t k = 0; k < cap; ++k) {
            CHECK(band[k].n == lv[k].n && band[k].sum == 0 && band[k].min == -band[k].max - (lv[k].n ? 0 : 1));
          }
        }
  // a table of all (1, 0): re is the sum of the Samples form, im is 0; statuses and the other fields are its own
  {
    std::vector<uint64_t> rows, off;
    uint64_t stride, cap;
    layout(7, false, &rows, &off, &stride, &cap);
    x3::device::Buffer d_a(ctx, sizeof(x3_level) * cap), d_b(ctx, sizeof(x3_tone_level) * cap), d_sa(ctx, 4 * W), d_sb(ctx, 4 * W);
    std::vector<x3_level> a(cap);
    std::vector<x3_tone_level> b(cap);
    std::vector<int32_t> sa(W), sb(W);
    x3::device::RangeLevelsResult r;
    CHECK(x3::device::range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0, d_a.as<x3_level>(),
                                   cap, d_off.as<uint64_t>(), d_sa.as<int32_t>(), &r) == x3::X3Error::Ok);
    CHECK(x3::device::tone_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                        d_b.as<x3_tone_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(),
                                        Tone{350898828u, d_ones.as<int16_t>()}, &r) == x3::X3Error::Ok);
    CHECK(d_a.download(a.data(), sizeof(x3_level) * cap) == x3::X3Error::Ok && d_b.download(b.data(), sizeof(x3_tone_level) * cap) == x3::X3Error::Ok);
    CHECK(d_sa.download(sa.data(), 4 * W) == x3::X3Error::Ok && d_sb.download(sb.data(), 4 * W) == x3::X3Error::Ok);
    for (size_t w = 0; w < W; ++w) {
      CHECK(sa[w] == sb[w]);
      for (uint64_t k = off[w]; k < off[w + 1]; ++k)
        CHECK(b[k].re == a[k].sum && b[k].im == 0 && b[k].min == a[k].min && b[k].max == a[k].max && b[k].n == a[k].n);
    }
    // refused: no table, a table at an odd address -- in front of every other argument (no ranges, no records)
    for (const Tone& bad : {Tone{1u, nullptr}, Tone{1u, d_usual.as<int16_t>() + 1}}) {
      CHECK(x3::device::tone_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                          d_b.as<x3_tone_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
      CHECK(corpus.tone_range_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, 7, 0,
                                     d_b.as<x3_tone_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(), bad, &r) == x3::X3Error::BadArg);
    }
    CHECK(x3::device::tone_range_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), 0, 7, 0,
                                        d_b.as<x3_tone_level>(), cap, d_off.as<uint64_t>(), d_sb.as<int32_t>(),
                                        Tone{1u, d_usual.as<int16_t>()}, &r) == x3::X3Error::BadArg);
  }
  std::printf("test_tone_range_levels_hpp ok\n");
  return 0;
}
