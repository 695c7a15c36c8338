// Exercises x3::device::level_quantiles, level_thresholds, events_adaptive and the x3::device::Corpus members of the same
// names in x3-rust_amd/host/x3.hpp (x3_level_quantiles_dev, x3_level_thresholds_dev, x3_events_adaptive_dev, their corpus
// forms, x3_level_quantiles_result) on hand-made level records: quantiles against std::sort, the threshold map, and a corpus
// of two entries with different noise floors whose loud rows only the per-entry thresholds find.  Needs a GPU.
// usage: test_thresholds_hpp
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

static uint32_t peak_key(const x3_level& r) {
  return (uint32_t)std::min<int64_t>(std::max<int64_t>(std::max<int64_t>(r.max, -(int64_t)r.min), 0), 32768);
}
static uint32_t mean_sq_key(const x3_level& r) { return (uint32_t)std::min<uint64_t>(r.sum_sq / r.n, 1ull << 30); }

// sorted(keys)[(K - 1) * q / 1000000] over the counting rows [a, b)
static uint32_t quantile(const std::vector<x3_level>& lv, size_t a, size_t b, int key, uint32_t q, uint32_t* counted) {
  std::vector<uint32_t> k;
  for (size_t i = a; i < b; ++i)
    if (lv[i].n) k.push_back(key == X3_LEVEL_KEY_PEAK ? peak_key(lv[i]) : mean_sq_key(lv[i]));
  std::sort(k.begin(), k.end());
  *counted = (uint32_t)k.size();
  return k.empty() ? 0u : k[(uint64_t)(k.size() - 1) * q / 1000000u];
}

int main() {
  static_assert(sizeof(x3_threshold_rule) == 32 && sizeof(x3_event_threshold) == 16, "sizes of include/x3hip.h");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  // two clips of silence, 300 and 523 rows of 4 positions: entry 0 quiet (noise floor 10), entry 1 loud (noise floor 1000)
  const uint64_t bin_len = 4;
  const size_t rows0 = 300, rows1 = 523, n0 = 4 * rows0 - 1, n1 = 4 * rows1, n_rows = rows0 + rows1;
  std::vector<int16_t> wav(n0 + n1, 0);
  x3::device::Buffer d_wav(ctx, 2 * wav.size());
  CHECK(d_wav.upload(wav.data(), 2 * wav.size()) == x3::X3Error::Ok);
  x3::device::EncodedStream s0, s1;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n0, 1, params, 0, &s0) == x3::X3Error::Ok);
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n1, 1, params, 0, &s1) == x3::X3Error::Ok);
  std::vector<uint8_t> b0(s0.len), b1(s1.len), both;
  CHECK(s0.bytes.download(b0.data(), s0.len) == x3::X3Error::Ok && s1.bytes.download(b1.data(), s1.len) == x3::X3Error::Ok);
  both = b0;
  both.insert(both.end(), b1.begin(), b1.end());
  both.resize(both.size() + 16, 0);
  x3::device::Buffer d_x3(ctx, both.size());
  CHECK(d_x3.upload(both.data(), both.size()) == x3::X3Error::Ok);
  const std::vector<uint64_t> offs = {0, s0.len}, lns = {s0.len, s1.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, d_x3.as<uint8_t>(), both.size(), offs, lns, 0, params, 0, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[1] == rows0 && rf[2] == n_rows);
  // hand-made records: a noise floor per entry, a burst of 4 x the floor in rows 100 .. 109 of each, some rows uncounted
  std::vector<x3_level> lv(n_rows);
  uint32_t seed = 12345;
  for (size_t r = 0; r < n_rows; ++r) {
    seed = seed * 1664525u + 1013904223u;
    const bool second = r >= rows0;
    const size_t rel = second ? r - rows0 : r;
    const int32_t floor = second ? 1000 : 10, amp = (rel >= 100 && rel < 110 ? 4 * floor : floor) + (int32_t)((seed >> 16) % (uint32_t)floor) / 2;
    const uint32_t n = 1 + (seed >> 8) % 7;
    lv[r] = x3_level{(uint64_t)amp * amp * n / 2 + (seed & 1), 0, r % 2 ? -amp : -1, r % 2 ? 1 : amp, rel % 37 == 5 ? 0u : n, 0};
  }
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * n_rows), d_tot(ctx, 8);
  CHECK(d_lv.upload(lv.data(), sizeof(x3_level) * n_rows) == x3::X3Error::Ok);
  const std::vector<uint32_t> q = {500000, 0, 1000000, 999999, 123456, 0};
  x3::device::Buffer d_val(ctx, 4 * 2 * q.size()), d_k(ctx, 4 * 2), d_thr(ctx, 16 * 2);
  x3::device::QuantilesResult qr;
  std::vector<uint32_t> val(2 * q.size()), k(2);
  // the stream form on the first entry's rows, a total that leaves the last 9 rows out
  const uint64_t total = 4 * (rows0 - 9) - 2;
  CHECK(d_tot.upload(&total, 8) == x3::X3Error::Ok);
  for (int key : {X3_LEVEL_KEY_PEAK, X3_LEVEL_KEY_MEAN_SQ}) {
    CHECK(x3::device::level_quantiles(ctx, d_lv.as<x3_level>(), rows0, bin_len, d_tot.as<uint64_t>(), key, q, d_val.as<uint32_t>(),
                                      d_k.as<uint32_t>(), &qr) == x3::X3Error::Ok);
    CHECK(qr.n_empty == 0 && qr.first_empty == 1);
    CHECK(d_val.download(val.data(), 4 * q.size()) == x3::X3Error::Ok && d_k.download(k.data(), 4) == x3::X3Error::Ok);
    for (size_t j = 0; j < q.size(); ++j) {
      uint32_t kk;
      CHECK(val[j] == quantile(lv, 0, rows0 - 9, key, q[j], &kk) && k[0] == kk);
    }
    // the corpus form: both entries
    CHECK(corpus.level_quantiles(ctx, d_lv.as<x3_level>(), n_rows, bin_len, key, q, d_val.as<uint32_t>(), d_k.as<uint32_t>(), &qr) ==
          x3::X3Error::Ok);
    CHECK(qr.n_empty == 0 && qr.first_empty == 2);
    CHECK(d_val.download(val.data(), 4 * 2 * q.size()) == x3::X3Error::Ok && d_k.download(k.data(), 8) == x3::X3Error::Ok);
    for (size_t e = 0; e < 2; ++e)
      for (size_t j = 0; j < q.size(); ++j) {
        uint32_t kk;
        CHECK(val[e * q.size() + j] == quantile(lv, rf[e], rf[e + 1], key, q[j], &kk) && k[e] == kk);
      }
  }
  // thresholds: twice the median peak plus 1; a quarter of the 90 % mean square, floored
  const x3_threshold_rule trule{500000, 2, 1, 1, 900000, 1, 4, 0};
  std::vector<x3_event_threshold> thr(2);
  CHECK(corpus.level_thresholds(ctx, d_lv.as<x3_level>(), n_rows, bin_len, trule, d_thr.as<x3_event_threshold>(), &qr) == x3::X3Error::Ok);
  CHECK(d_thr.download(thr.data(), 32) == x3::X3Error::Ok);
  for (size_t e = 0; e < 2; ++e) {
    uint32_t kk;
    const uint64_t p = quantile(lv, rf[e], rf[e + 1], X3_LEVEL_KEY_PEAK, 500000, &kk);
    const uint64_t m = quantile(lv, rf[e], rf[e + 1], X3_LEVEL_KEY_MEAN_SQ, 900000, &kk);
    CHECK(thr[e].peak_min == std::min<uint64_t>(2 * p + 1, 32768) && thr[e].mean_sq_min == std::max<uint64_t>(m / 4, 1) && thr[e].counted == kk);
  }
  CHECK(thr[0].peak_min < 40 && thr[1].peak_min > 2000);
  // the stream form writes one record; the smallest peak (at least 10) times 4 000 is clamped to the limit
  x3_event_threshold one;
  uint32_t k_stream;
  (void)quantile(lv, 0, rows0 - 9, X3_LEVEL_KEY_PEAK, 0, &k_stream);
  CHECK(x3::device::level_thresholds(ctx, d_lv.as<x3_level>(), rows0, bin_len, d_tot.as<uint64_t>(), x3_threshold_rule{0, 4000, 1, 0, 0, 0, 0, 0},
                                     d_thr.as<x3_event_threshold>(), &qr) == x3::X3Error::Ok);
  CHECK(d_thr.download(&one, 16) == x3::X3Error::Ok && one.peak_min == 32768 && one.mean_sq_min == 0 && one.counted == k_stream);
  CHECK(x3::device::level_thresholds(ctx, d_lv.as<x3_level>(), rows0, bin_len, d_tot.as<uint64_t>(), x3_threshold_rule{0, 1, 0, 0, 0, 1, 0, 0},
                                     d_thr.as<x3_event_threshold>(), &qr) == x3::X3Error::BadArg);
  // adaptive events with the peak thresholds alone: the burst of each entry, and nothing else; one global threshold (the
  // quiet entry's) marks the loud entry hot end to end
  const x3_threshold_rule prule{500000, 2, 1, 1, 0, 0, 0, 0};
  CHECK(corpus.level_thresholds(ctx, d_lv.as<x3_level>(), n_rows, bin_len, prule, d_thr.as<x3_event_threshold>(), &qr) == x3::X3Error::Ok);
  CHECK(d_thr.download(thr.data(), 32) == x3::X3Error::Ok && thr[0].mean_sq_min == 0 && thr[1].mean_sq_min == 0);
  const uint64_t cap = 8;
  const x3_event_rule rule{0, 0, 2, 0, 0, 0, 0};
  x3::device::Buffer d_ent(ctx, 4 * cap), d_starts(ctx, 8 * cap), d_lens(ctx, 4 * cap), d_cnt(ctx, 8);
  uint64_t count = ~0ull;
  CHECK(corpus.events_adaptive(ctx, d_lv.as<x3_level>(), n_rows, bin_len, rule, d_thr.as<x3_event_threshold>(), d_ent.as<uint32_t>(),
                               d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  std::vector<uint32_t> ent(cap), lens(cap);
  std::vector<uint64_t> starts(cap);
  CHECK(d_ent.download(ent.data(), 4 * cap) == x3::X3Error::Ok && d_starts.download(starts.data(), 8 * cap) == x3::X3Error::Ok);
  CHECK(d_lens.download(lens.data(), 4 * cap) == x3::X3Error::Ok);
  CHECK(count == 2 && ent[0] == 0 && ent[1] == 1 && starts[0] == 400 && starts[1] == 400 && lens[0] == 40 && lens[1] == 40);
  for (size_t i = 2; i < cap; ++i) CHECK(ent[i] == 0 && starts[i] == 0 && lens[i] == 0);
  x3_event_rule global = rule;
  global.peak_min = thr[0].peak_min;
  CHECK(corpus.events(ctx, d_lv.as<x3_level>(), n_rows, bin_len, global, d_ent.as<uint32_t>(), d_starts.as<uint64_t>(),
                      d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  CHECK(d_ent.download(ent.data(), 4 * cap) == x3::X3Error::Ok && d_starts.download(starts.data(), 8 * cap) == x3::X3Error::Ok);
  CHECK(d_lens.download(lens.data(), 4 * cap) == x3::X3Error::Ok);
  CHECK(count == 2 && ent[1] == 1 && starts[1] == 0 && lens[1] == n1);
  // the stream form reads one record; a rule that carries a value of its own is refused
  CHECK(x3::device::events_adaptive(ctx, d_lv.as<x3_level>(), rows0, bin_len, d_tot.as<uint64_t>(), rule, d_thr.as<x3_event_threshold>(),
                                    d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  CHECK(d_starts.download(starts.data(), 8) == x3::X3Error::Ok && d_lens.download(lens.data(), 4) == x3::X3Error::Ok);
  CHECK(count == 1 && starts[0] == 400 && lens[0] == 40);
  CHECK(x3::device::events_adaptive(ctx, d_lv.as<x3_level>(), rows0, bin_len, d_tot.as<uint64_t>(), global, d_thr.as<x3_event_threshold>(),
                                    d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::BadArg);
  std::printf("test_thresholds_hpp ok\n");
  return 0;
}
