// Exercises x3::device::SpectraRule, x3::device::spectra_rows, x3::device::range_spectra and
// x3::device::Corpus::range_spectra of x3-rust_amd/host/x3.hpp (x3_spectra_rows_dev behind x3_decode_ranges_dev /
// x3_corpus_ranges_dev) on the base stream of tests/test_gpu_range_levels.py: 2 137 samples in frames of 400 with a
// walk-built index.  Every word is held with == against a loop over the frames' samples in int64: the sums, the powers, packed
// and padded, the cut samples the caller keeps, a range off the end (its status, rows of zeros), rows nobody's keep the
// caller's bytes.  Needs a GPU.
// usage: test_spectra_hpp
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

int main() {
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
  for (uint32_t n_fft : {64u, 128u})
    for (uint32_t hop : {n_fft, 40u})
      for (int power = 0; power < 2; ++power)
        for (int form = 0; form < 2; ++form)
          for (int padded = 0; padded < 2; ++padded) {
            SpectraRule rule;
            rule.n_fft = n_fft, rule.hop = hop, rule.power = power != 0, rule.d_table = d_usual.as<int16_t>();
            CHECK(rule.bins() == n_fft / 2 + 1 && rule.c_rule().format == (uint32_t)(power ? X3_SPECTRA_POWER : X3_SPECTRA_SUMS));
            const uint32_t B = rule.bins();
            std::vector<uint64_t> rows(W), off(W + 1, 0);
            uint64_t most = 1;
            for (size_t w = 0; w < W; ++w) {
              rows[w] = rule.rows(lens[w]);
              off[w + 1] = off[w] + rows[w];
              if (rows[w] > most) most = rows[w];
            }
            const uint64_t stride = padded ? most : 0, drawn = padded ? most * W : off[W], cap = drawn + 2;   // two rows nobody's
            const size_t row_bytes = (size_t)B * (power ? 4 : 16);
            std::vector<uint8_t> fill(row_bytes * cap, 0x5A), got(row_bytes * cap);
            x3::device::Buffer d_out(ctx, row_bytes * cap);
            CHECK(d_out.upload(fill.data(), fill.size()) == x3::X3Error::Ok);
            x3::device::SpectraResult r;
            const x3::X3Error e =
                form == 0 ? x3::device::range_spectra(ctx, s, params, d_so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, rule,
                                                      d_samples.as<int16_t>(), n_samples, d_soff.as<uint64_t>(), stride, d_out.as<uint8_t>(),
                                                      cap, padded ? nullptr : d_roff.as<uint64_t>(), d_status.as<int32_t>(), &r)
                          : corpus.range_spectra(ctx, d_entries.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), W, rule,
                                                 d_samples.as<int16_t>(), n_samples, d_soff.as<uint64_t>(), stride, d_out.as<uint8_t>(), cap,
                                                 padded ? nullptr : d_roff.as<uint64_t>(), d_status.as<int32_t>(), &r);
            CHECK(e == x3::X3Error::Ok);
            CHECK(r.n_bad == 1 && r.first_bad == 3 && r.first_bad_status == X3_ERR_BAD_ARG && r.total_rows == off[W]);
            std::vector<int32_t> st(W);
            std::vector<uint64_t> soff(W + 1), roff(W + 1);
            std::vector<int16_t> cut(n_samples);
            CHECK(d_out.download(got.data(), got.size()) == x3::X3Error::Ok && d_status.download(st.data(), 4 * W) == x3::X3Error::Ok);
            CHECK(d_soff.download(soff.data(), 8 * (W + 1)) == x3::X3Error::Ok && d_samples.download(cut.data(), 2 * n_samples) == x3::X3Error::Ok);
            if (!padded) CHECK(d_roff.download(roff.data(), 8 * (W + 1)) == x3::X3Error::Ok && roff == off);
            for (size_t w = 0; w < W; ++w) {
              CHECK(st[w] == (w == 3 ? X3_ERR_BAD_ARG : 0));
              if (w != 3) CHECK(std::memcmp(cut.data() + soff[w], wav.data() + starts[w], 2 * lens[w]) == 0);   // the cut samples
              const uint64_t base = padded ? w * stride : off[w], written = padded ? stride : rows[w];
              for (uint64_t q = 0; q < written; ++q)
                for (uint32_t k = 0; k < B; ++k) {
                  int64_t re = 0, im = 0;
                  if (w != 3 && q < rows[w])
                    for (uint32_t i = 0; i < n_fft; ++i) {
                      const uint32_t idx = ((i * k) % n_fft) * (1024 / n_fft);
                      const int64_t x = wav[starts[w] + q * hop + i];
                      re += x * usual[2 * idx];
                      im += x * usual[2 * idx + 1];
                    }
                  const uint8_t* at = got.data() + (base + q) * row_bytes;
                  if (power) {
                    const int64_t a = re >> 15, b = im >> 15;
                    uint64_t ms = ((uint64_t)(2 * (a * a + b * b)) / n_fft) / n_fft;
                    if (ms > (1ull << 30)) ms = 1ull << 30;
                    uint32_t v;
                    std::memcpy(&v, at + 4 * k, 4);
                    CHECK(v == (uint32_t)ms);
                  } else {
                    int64_t v[2];
                    std::memcpy(v, at + 16 * k, 16);
                    CHECK(v[0] == re && v[1] == im);
                  }
                }
            }
            CHECK(std::memcmp(got.data() + drawn * row_bytes, fill.data(), 2 * row_bytes) == 0);   // untouched
          }
  // spectra_rows on rows of the caller's own, and the rule's refusals in front of every other argument
  {
    SpectraRule rule;
    rule.n_fft = 64, rule.hop = 64, rule.power = false, rule.d_table = d_usual.as<int16_t>();
    const uint64_t offs[2] = {1, 1000};
    const uint32_t ln[2] = {128, 64};
    x3::device::Buffer d_o(ctx, 16), d_l(ctx, 8), d_out(ctx, 16 * 33 * 3), d_st(ctx, 8), d_ro(ctx, 24);
    CHECK(d_o.upload(offs, 16) == x3::X3Error::Ok && d_l.upload(ln, 8) == x3::X3Error::Ok);
    x3::device::SpectraResult r;
    CHECK(x3::device::spectra_rows(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, rule, 0,
                                   d_out.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == 2 && r.total_rows == 3);
    std::vector<int64_t> got(2 * 33 * 3);
    CHECK(d_out.download(got.data(), 16 * 33 * 3) == x3::X3Error::Ok);
    int64_t dc = 0;
    for (uint32_t i = 0; i < 64; ++i) dc += (int64_t)wav[1000 + i] * usual[0];
    CHECK(got[2 * 33 * 2] == dc && got[2 * 33 * 2 + 1] == 0);      // bin 0 of the third row: 32767 * the frame's sum, im 0
    for (int bad = 0; bad < 4; ++bad) {
      SpectraRule q = rule;
      if (bad == 0) q.n_fft = 96;
      if (bad == 1) q.hop = 0;
      if (bad == 2) q.d_table = nullptr;
      if (bad == 3) q.d_table = d_usual.as<int16_t>() + 1;
      CHECK(x3::device::spectra_rows(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 0, q, 0,
                                     d_out.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::BadArg);
    }
    // a context that is recording a graph refuses the good call; the workspace exists already, so only that check can
    CHECK(x3_graph_begin(ctx.raw()) == X3_OK);
    const x3::X3Error rec = x3::device::spectra_rows(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2,
                                                     rule, 0, d_out.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r);
    x3_graph* g = nullptr;
    if (x3_graph_end(ctx.raw(), &g) == X3_OK && g) x3_graph_destroy(g);
    CHECK(rec == x3::X3Error::BadArg);
    CHECK(x3::device::spectra_rows(ctx, d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, rule, 0,
                                   d_out.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
    x3_spectra_rule raw = rule.c_rule();
    raw.reserved = 1;
    CHECK(x3_spectra_rows_dev(ctx.raw(), d_wav.as<int16_t>(), n, d_o.as<uint64_t>(), d_l.as<uint32_t>(), nullptr, 2, &raw, 0,
                              d_out.as<uint8_t>(), 3, d_ro.as<uint64_t>(), d_st.as<int32_t>()) == X3_ERR_BAD_ARG);
  }
  std::printf("test_spectra_hpp ok\n");
  return 0;
}
