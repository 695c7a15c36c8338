// Exercises x3::device::events and x3::device::Corpus::events of x3-rust_amd/host/x3.hpp (x3_events_dev, x3_corpus_events_dev,
// x3_events_result): levels, events and ranges of a stream with loud bursts, and of a corpus that holds it twice, against a
// serial detector over the samples it was encoded from; the filler slots are zero-length ranges with status 0.  Needs a GPU.
// usage: test_events_hpp
#include <algorithm>
#include <cmath>
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

struct Event { uint64_t start; uint32_t len; };

// peak rule only, min_bins 0: hot bins, runs joined over `join` cold bins, padded, clipped, cut into pieces of max_bins
static std::vector<Event> detect(const std::vector<int16_t>& w, uint64_t bl, const x3_event_rule& k) {
  const size_t rows = (w.size() + bl - 1) / bl;
  std::vector<char> hot(rows, 0);
  for (size_t i = 0; i < w.size(); ++i)
    if ((uint32_t)std::abs((int)w[i]) >= k.peak_min) hot[i / bl] = 1;
  std::vector<Event> ev;
  for (size_t b = 0; b < rows;) {
    if (!hot[b]) { ++b; continue; }
    size_t last = b;
    for (size_t c = b + 1; c < rows && c - last - 1 <= k.join_bins; ++c)
      if (hot[c]) last = c;
    const size_t b0 = b - std::min<size_t>(k.pad_bins, b), b1 = std::min<size_t>(last + 1 + k.pad_bins, rows);
    for (size_t p0 = b0; p0 < b1; p0 += k.max_bins) {
      const size_t p1 = std::min<size_t>(p0 + k.max_bins, b1);
      ev.push_back(Event{p0 * bl, (uint32_t)(std::min<uint64_t>(p1 * bl, w.size()) - p0 * bl)});
    }
    b = last + 1;
  }
  return ev;
}

int main() {
  static_assert(sizeof(x3_event_rule) == 32, "x3_event_rule is 32 bytes");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 43457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7117, 0, n, wav.data()) == 0);
  for (auto& v : wav) v = (int16_t)(v >> 6);
  const size_t bursts[][2] = {{0, 700}, {9990, 30}, {15000, 9000}, {30000, 10}, {43000, 457}};
  for (auto& b : bursts)
    for (size_t i = 0; i < b[1]; ++i) wav[b[0] + i] = (int16_t)(9000.0 * std::sin(0.37 * (double)i));
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const uint64_t bin_len = 500, cap = 32, stride = 3000;
  const size_t n_bins = (n + bin_len - 1) / bin_len;
  const x3_event_rule rule{0, 8000, 4, 0, 2, 6, 0};
  const std::vector<Event> want = detect(wav, bin_len, rule);
  CHECK(want.size() >= 6 && want.size() < cap);
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * n_bins), d_starts(ctx, 8 * cap), d_lens(ctx, 4 * cap), d_el(ctx, 32 * cap), d_cnt(ctx, 8);
  x3::device::Buffer d_out(ctx, 2 * cap * stride), d_status(ctx, 4 * cap);
  x3::device::WindowsResult r;
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  uint64_t count = ~0ull;
  CHECK(x3::device::events(ctx, d_lv.as<x3_level>(), n_bins, bin_len, so.as<uint64_t>() + s.n_frames, rule, d_starts.as<uint64_t>(),
                           d_lens.as<uint32_t>(), d_el.as<x3_level>(), cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  CHECK(count == want.size());
  std::vector<uint64_t> starts(cap);
  std::vector<uint32_t> lens(cap);
  std::vector<x3_level> el(cap);
  uint64_t dev_count = 0;
  CHECK(d_starts.download(starts.data(), 8 * cap) == x3::X3Error::Ok && d_lens.download(lens.data(), 4 * cap) == x3::X3Error::Ok);
  CHECK(d_el.download(el.data(), 32 * cap) == x3::X3Error::Ok && d_cnt.download(&dev_count, 8) == x3::X3Error::Ok);
  CHECK(dev_count == count);
  for (size_t i = 0; i < cap; ++i) {
    const Event e = i < want.size() ? want[i] : Event{0, 0};
    CHECK(starts[i] == e.start && lens[i] == e.len);
    uint32_t cnt = 0;
    int32_t mx = -32768;
    for (uint64_t g = e.start; g < e.start + e.len; ++g) { ++cnt; mx = std::max<int32_t>(mx, wav[g]); }
    CHECK(el[i].n == cnt && el[i].max == mx && (i < want.size() || (el[i].min == 32767 && el[i].sum == 0 && el[i].sum_sq == 0)));
  }
  // the arrays as they are, n_ranges = cap
  x3::device::RangesResult rr;
  CHECK(x3::device::decode_ranges(ctx, s, params, so, d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), cap, stride, d_out.as<void>(),
                                  cap * stride, X3_WINDOW_I16, nullptr, d_status.as<int32_t>(), &rr) == x3::X3Error::Ok);
  CHECK(rr.n_bad == 0);
  std::vector<int16_t> out(cap * stride);
  CHECK(d_out.download(out.data(), 2 * cap * stride) == x3::X3Error::Ok);
  for (size_t i = 0; i < cap; ++i)
    for (size_t t = 0; t < stride; ++t) CHECK(out[i * stride + t] == (t < lens[i] ? wav[starts[i] + t] : 0));
  // refusals: both criteria off; padding wider than half the join
  x3_event_rule bad = rule;
  bad.peak_min = 0;
  CHECK(x3::device::events(ctx, d_lv.as<x3_level>(), n_bins, bin_len, so.as<uint64_t>() + s.n_frames, bad, d_starts.as<uint64_t>(),
                           d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::BadArg);
  bad = rule;
  bad.pad_bins = 3;
  CHECK(x3::device::events(ctx, d_lv.as<x3_level>(), n_bins, bin_len, so.as<uint64_t>() + s.n_frames, bad, d_starts.as<uint64_t>(),
                           d_lens.as<uint32_t>(), nullptr, cap, d_cnt.as<uint64_t>(), &count) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice: every event twice, entries 0 then 1; a cap below the count
  const std::vector<uint64_t> offs = {0, 0}, lns = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lns, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_level) * rf[2]), d_ent(ctx, 4 * cap);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  const uint64_t small = want.size() + 2;
  CHECK(corpus.events(ctx, d_rows.as<x3_level>(), rf[2] - 1, bin_len, rule, d_ent.as<uint32_t>(), d_starts.as<uint64_t>(),
                      d_lens.as<uint32_t>(), nullptr, small, d_cnt.as<uint64_t>(), &count) == x3::X3Error::BadArg);
  CHECK(corpus.events(ctx, d_rows.as<x3_level>(), rf[2], bin_len, rule, d_ent.as<uint32_t>(), d_starts.as<uint64_t>(),
                      d_lens.as<uint32_t>(), nullptr, small, d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  CHECK(count == 2 * want.size());
  std::vector<uint32_t> ent(small);
  CHECK(d_ent.download(ent.data(), 4 * small) == x3::X3Error::Ok && d_starts.download(starts.data(), 8 * small) == x3::X3Error::Ok);
  CHECK(d_lens.download(lens.data(), 4 * small) == x3::X3Error::Ok);
  for (size_t i = 0; i < small; ++i) {
    const Event e = want[i % want.size()];
    CHECK(ent[i] == i / want.size() && starts[i] == e.start && lens[i] == e.len);
  }
  CHECK(corpus.ranges(ctx, d_ent.as<uint32_t>(), d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), small, stride, d_out.as<void>(),
                      cap * stride, X3_WINDOW_I16, nullptr, d_status.as<int32_t>(), &rr) == x3::X3Error::Ok && rr.n_bad == 0);
  std::printf("test_events_hpp ok\n");
  return 0;
}
