// Exercises x3::device::SpectraFold, x3::device::spectra_levels, x3::device::range_band_levels and
// x3::device::Corpus::range_band_levels of x3-rust_amd/host/x3.hpp (x3_spectra_levels_dev behind x3_decode_ranges_dev /
// x3_corpus_ranges_dev) on the base stream of tests/test_gpu_range_levels.py: 2 137 samples in frames of 400 with a
// walk-built index.  Every record of every plane is held with == against a loop over the frames' samples in int64: the band
// sums with their clamp, the time bins, packed and padded, a range off the end (its status, identity records), records
// nobody's keep the caller's bytes -- those between rows_cap and the plane stride among them.  Needs a GPU.
// usage: test_spectra_levels_hpp
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

static uint32_t isqrt64(uint64_t x) {
  uint32_t r = 0;
  for (int b = 31; b >= 0; --b) {
    const uint64_t t = (uint64_t)r | (1ull << b);
    if (t * t <= x) r = (uint32_t)t;
  }
  return r;
}

static bool same(const x3_level& a, const x3_level& b) {
  return a.sum_sq == b.sum_sq && a.sum == b.sum && a.min == b.min && a.max == b.max && a.n == b.n && a.reserved == b.reserved;
}

int main() {
  using x3::device::SpectraFold;
  using x3::device::SpectraRule;
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
  CHECK(x3::device::index_by_walk(ctx, &s, params, 4) == x3::X3Error::Ok && s.seg_blocks == 4);
  x3::device::Buffer d_so;
  CHECK(x3::device::sample_offsets(ctx, s, &d_so) == x3::X3Error::Ok);
  const std::vector<uint64_t> starts = {0, 399, 2000, 1, 801, 2100};
  const std::vector<uint32_t> lens = {400, 63, 137, 2137, 700, 37};     // (1, 2137) runs off the end; 63 and 37: no whole frame
  const size_t W = starts.size();
  uint64_t n_samples = 0;
  for (uint32_t v : lens) n_samples += v;
  x3::device::Buffer d_starts(ctx, 8 * W), d_lens(ctx, 4 * W), d_status(ctx, 4 * W), d_soff(ctx, 8 * (W + 1)), d_roff(ctx, 8 * (W + 1)),
      d_samples(ctx, 2 * n_samples), d_entries(ctx, 4 * W);
  CHECK(d_starts.upload(starts.data(), 8 * W) == x3::X3Error::Ok && d_lens.upload(lens.data(), 4 * W) == x3::X3Error::Ok);
  x3::device::Corpus corpus;   // two entries: the stream itself, twice
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, {0, 0}, {s.len, s.len}, 0, params, 4, true) == x3::X3Error::Ok);
  std::vector<uint32_t> entries(W);
  for (size_t w = 0; w < W; ++w) entries[w] = (uint32_t)(w & 1);
  CHECK(d_entries.upload(entries.data(), 4 * W) == x3::X3Error::Ok);
  const std::vector<int16_t> usual = Tone::usual_table();
  x3::device::Buffer d_usual(ctx, 4096);
  CHECK(d_usual.upload(usual.data(), 4096) == x3::X3Error::Ok);
  const x3_level identity{0, 0, 32767, -32768, 0, 0};
  for (uint32_t n_fft : {64u, 128u})
    for (uint32_t hop : {n_fft, 40u})
      for (uint32_t per_bin : {1u, 3u})
        for (int form = 0; form < 2; ++form)
          for (int padded = 0; padded < 2; ++padded) {
            SpectraRule rule;
            rule.n_fft = n_fft, rule.hop = hop, rule.power = true, rule.d_table = d_usual.as<int16_t>();
            const uint32_t B = rule.bins(), K = 5;
            // five bands, not contiguous; band 3 has no bin; some bins are in no band
            std::vector<uint32_t> map(B);
            for (uint32_t k = 0; k < B; ++k) map[k] = k % 7 == 3 ? 0xFFFFFFFFu : (k % 7 == 5 ? K : (k * 3) % 5 == 3 ? 4 : (k * 3) % 5);
            x3::device::Buffer d_map(ctx, 4 * B);
            CHECK(d_map.upload(map.data(), 4 * B) == x3::X3Error::Ok);
            std::vector<uint64_t> frames(W), bins(W), off(W + 1, 0);
            uint64_t most = 1;
            SpectraFold fold;
            fold.frames_per_bin = per_bin, fold.n_bands = K, fold.d_bin_band = d_map.as<uint32_t>();
            for (size_t w = 0; w < W; ++w) {
              frames[w] = rule.rows(lens[w]);
              bins[w] = fold.time_bins(frames[w]);
              CHECK(bins[w] == (frames[w] + per_bin - 1) / per_bin);
              off[w + 1] = off[w] + bins[w];
              most = std::max(most, bins[w]);
            }
            const uint64_t stride = padded ? most : 0, drawn = padded ? most * W : off[W], cap = drawn + 2;   // two rows nobody's
            const uint64_t ps = cap + 3;                                                                      // ... and three between planes
            fold.plane_stride = ps;
            CHECK(fold.c_fold().plane_stride == ps && fold.c_fold().reserved == 0 && fold.c_fold().n_bands == K);
            std::vector<x3_level> got(K * ps);
            std::vector<uint8_t> fill(sizeof(x3_level) * K * ps, 0x5A);
            x3::device::Buffer d_lv(ctx, fill.size());
            CHECK(d_lv.upload(fill.data(), fill.size()) == x3::X3Error::Ok);
            x3::device::SpectraResult r;
            const x3::X3Error e =
                form == 0 ? x3::device::range_band_levels(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, rule, fold,
                                                          d_samples.as<int16_t>(), n_samples, d_soff.as<uint64_t>(), stride,
                                                          d_lv.as<x3_level>(), cap, padded ? nullptr : d_roff.as<uint64_t>(),
                                                          d_status.as<int32_t>(), &r)
                          : corpus.range_band_levels(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, rule,
                                                     fold, d_samples.as<int16_t>(), n_samples, d_soff.as<uint64_t>(), stride,
                                                     d_lv.as<x3_level>(), cap, padded ? nullptr : d_roff.as<uint64_t>(),
                                                     d_status.as<int32_t>(), &r);
            CHECK(e == x3::X3Error::Ok);
            CHECK(r.n_bad == 1 && r.first_bad == 3 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);
            std::vector<int32_t> st(W);
            std::vector<uint64_t> roff(W + 1);
            CHECK(d_lv.download(got.data(), fill.size()) == x3::X3Error::Ok && d_status.download(st.data(), 4 * W) == x3::X3Error::Ok);
            if (!padded) CHECK(d_roff.download(roff.data(), 8 * (W + 1)) == x3::X3Error::Ok && roff == off);
            for (size_t w = 0; w < W; ++w) {
              CHECK(st[w] == (w == 3 ? X3_ERR_BAD_ARG : 0));
              const uint64_t base = padded ? w * stride : off[w], written = padded ? stride : bins[w];
              for (uint64_t j = 0; j < written; ++j)
                for (uint32_t b = 0; b < K; ++b) {
                  x3_level want = identity;
                  if (w != 3 && j < bins[w]) {
                    uint64_t sum = 0, top = 0;
                    uint32_t cnt = 0;
                    for (uint64_t q = j * per_bin; q < std::min<uint64_t>((j + 1) * per_bin, frames[w]); ++q, ++cnt) {
                      uint64_t bp = 0;
                      for (uint32_t k = 0; k < B; ++k) {
                        if (map[k] != b) continue;
                        int64_t re = 0, im = 0;
                        for (uint32_t i = 0; i < n_fft; ++i) {
                          const uint32_t idx = ((i * k) % n_fft) * (1024 / n_fft);
                          const int64_t x = wav[starts[w] + q * hop + i];
                          re += x * usual[2 * idx];
                          im += x * usual[2 * idx + 1];
                        }
                        const int64_t a = re >> 15, c = im >> 15;
                        bp += std::min<uint64_t>(((uint64_t)(2 * (a * a + c * c)) / n_fft) / n_fft, 1ull << 30);
                      }
                      bp = std::min<uint64_t>(bp, 1ull << 30);
                      sum += bp;
                      top = std::max(top, bp);
                    }
                    const int32_t peak = (int32_t)std::min<uint32_t>(isqrt64(2 * top), 32767);
                    want = x3_level{sum, 0, -peak, peak, cnt, 0};
                  }
                  CHECK(same(got[b * ps + base + j], want));
                }
            }
            for (uint32_t b = 0; b < K; ++b)                                                     // untouched: behind the drawn rows
              CHECK(std::memcmp(&got[b * ps + drawn], fill.data(), sizeof(x3_level) * (ps - drawn)) == 0);
            if (per_bin == 3) CHECK(got[3 * ps].sum_sq == 0 && got[3 * ps].n == 3 && got[3 * ps].max == 0);   // the band without a bin
          }
  // spectra_levels on rows of the caller's own, and the fold's refusals behind the rule's
  {
    SpectraRule rule;
    rule.n_fft = 64, rule.hop = 64, rule.power = true, rule.d_table = d_usual.as<int16_t>();
    std::vector<uint32_t> map(33);
    for (uint32_t k = 0; k < 33; ++k) map[k] = k;
    x3::device::Buffer d_map(ctx, 4 * 33 + 4);
    CHECK(d_map.upload(map.data(), 4 * 33) == x3::X3Error::Ok);
    SpectraFold fold;
    fold.frames_per_bin = 1, fold.n_bands = 33, fold.d_bin_band = d_map.as<uint32_t>();
    const uint64_t offs[2] = {1, 1000};
    const uint32_t ln[2] = {128, 64};
    x3::device::Buffer d_o(ctx, 16), d_l(ctx, 8), d_lv(ctx, 32 * 33 * 3), d_pw(ctx, 4 * 33 * 3), d_st(ctx, 8), d_ro(ctx, 24);
    CHECK(d_o.upload(offs, 16) == x3::X3Error::Ok && d_l.upload(ln, 8) == x3::X3Error::Ok);
    x3::device::SpectraResult r;
    CHECK(x3::device::spectra_levels(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, rule, fold, 0,
                                     d_lv.as<x3_level>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == 2 && r.total_rows == 3);
    CHECK(x3::device::spectra_rows(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, rule, 0,
                                   d_pw.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
    std::vector<x3_level> lv(33 * 3);
    std::vector<uint32_t> pw(33 * 3);
    CHECK(d_lv.download(lv.data(), 32 * 33 * 3) == x3::X3Error::Ok && d_pw.download(pw.data(), 4 * 33 * 3) == x3::X3Error::Ok);
    for (uint32_t k = 0; k < 33; ++k)
      for (uint32_t q = 0; q < 3; ++q)      // one frame per bin, a band per bin: sum_sq is the POWER word
        CHECK(lv[k * 3 + q].sum_sq == pw[q * 33 + k] && lv[k * 3 + q].n == 1 && lv[k * 3 + q].max == -lv[k * 3 + q].min);
    for (int bad = 0; bad < 8; ++bad) {
      SpectraRule q = rule;
      SpectraFold f = fold;
      if (bad == 0) q.power = false;
      if (bad == 1) q.n_fft = 96;
      if (bad == 2) f.frames_per_bin = 0;
      if (bad == 3) f.n_bands = 34;
      if (bad == 4) f.n_bands = 0;
      if (bad == 5) f.d_bin_band = nullptr;
      if (bad == 6) f.d_bin_band = reinterpret_cast<const uint32_t*>(d_map.as<uint8_t>() + 2);
      if (bad == 7) f.plane_stride = 2;
      CHECK(x3::device::spectra_levels(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, q, f, 0,
                                       d_lv.as<x3_level>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::BadArg);
    }
    x3_spectra_rule raw = rule.c_rule();
    x3_spectra_fold rawf = fold.c_fold();
    rawf.reserved = 1;
    CHECK(x3_spectra_levels_dev(ctx.raw(), d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, &raw, &rawf, 0,
                                d_lv.as<x3_level>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>()) == X3_ERR_BAD_ARG);
    CHECK(x3_spectra_levels_dev(ctx.raw(), d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, &raw, nullptr, 0,
                                d_lv.as<x3_level>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>()) == X3_ERR_BAD_ARG);
  }
  std::printf("test_spectra_levels_hpp ok\n");
  return 0;
}
