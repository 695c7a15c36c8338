// Exercises x3::device::plane_events and x3::device::Corpus::plane_events of x3-rust_amd/host/x3.hpp (x3_plane_events_dev,
// x3_corpus_plane_events_dev, x3_events_result) on two planes of one stream: the levels of its samples and the levels of
// their first difference.  "Loud in either" and "loud in both" against a serial detector over the samples the stream was
// encoded from, with the mask of the planes loud in each event; the corpus holds the stream twice.  Needs a GPU.
// usage: test_plane_events_hpp
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

struct Event { uint64_t start; uint32_t len; uint32_t mask; };

// peak criteria only, join_bins 0, no padding, no cut: runs of rows at which at least min_planes of the two planes are loud
static std::vector<Event> detect(const std::vector<int16_t>& w, uint64_t bl, uint32_t peak_x, uint32_t peak_d, uint32_t min_planes) {
  const size_t rows = (w.size() + bl - 1) / bl;
  std::vector<uint32_t> loud(rows, 0);
  for (size_t i = 0; i < w.size(); ++i) {
    if ((uint32_t)std::abs((int)w[i]) >= peak_x) loud[i / bl] |= 1u;
    if (i > 0) {
      const int d = std::min(std::max((int)w[i] - (int)w[i - 1], -32768), 32767);
      if ((uint32_t)std::abs(d) >= peak_d) loud[i / bl] |= 2u;
    }
  }
  std::vector<Event> ev;
  for (size_t b = 0; b < rows;) {
    const auto hot = [&](size_t r) { return (loud[r] & 1u) + (loud[r] >> 1) >= min_planes; };
    if (!hot(b)) { ++b; continue; }
    size_t e = b;
    uint32_t mask = 0;
    for (; e < rows && hot(e); ++e) mask |= loud[e];
    ev.push_back(Event{b * bl, (uint32_t)(std::min<uint64_t>(e * bl, w.size()) - b * bl), mask});
    b = e;
  }
  return ev;
}

int main() {
  static_assert(sizeof(x3_plane_event_rule) == 128, "x3_plane_event_rule is 128 bytes");
  x3::Context ctx(0);
  x3_params cp;
  x3_params_default(&cp);
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 43457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7117, 0, n, wav.data()) == 0);
  for (auto& v : wav) v = (int16_t)(v >> 6);
  // slow loud swells (loud in the samples alone), fast small chirps (in the difference alone), and both at once
  for (size_t i = 0; i < 3000; ++i) wav[5000 + i] = (int16_t)(9000.0 * std::sin(0.002 * (double)i));
  for (size_t i = 0; i < 2000; ++i) wav[15000 + i] = (int16_t)((i & 1) ? 1500 : -1500);
  for (size_t i = 0; i < 2500; ++i) wav[25000 + i] = (int16_t)((i & 1) ? 9000 : -9000);
  for (size_t i = 0; i < 457; ++i) wav[43000 + i] = (int16_t)(9000.0 * std::sin(0.002 * (double)i));
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const uint64_t bin_len = 500, cap = 16;
  const size_t n_bins = (n + bin_len - 1) / bin_len, stride = n_bins + 3;
  const uint32_t peak_x = 8000, peak_d = 2500;
  x3::device::Buffer d_lv(ctx, sizeof(x3_level) * 2 * stride), d_starts(ctx, 8 * cap), d_lens(ctx, 4 * cap), d_mask(ctx, 4 * cap);
  x3::device::Buffer d_el(ctx, 32 * 2 * cap), d_cnt(ctx, 8);
  x3::device::WindowsResult r;
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>(), n_bins, nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(x3::device::levels(ctx, s, params, so, bin_len, d_lv.as<x3_level>() + stride, n_bins, nullptr, &r,
                           x3::device::LevelSignal::Diff) == x3::X3Error::Ok && r.n_bad == 0);
  x3::device::PlaneEventRule rule;
  rule.peak_min = {peak_x, peak_d};
  std::vector<uint64_t> starts(cap);
  std::vector<uint32_t> lens(cap), mask(cap);
  std::vector<x3_level> el(2 * cap);
  for (uint32_t min_planes = 1; min_planes <= 2; ++min_planes) {
    rule.min_planes = min_planes;
    const std::vector<Event> want = detect(wav, bin_len, peak_x, peak_d, min_planes);
    CHECK(want.size() >= (min_planes == 1 ? 4u : 1u) && want.size() < cap);
    uint64_t count = ~0ull, dev_count = 0;
    CHECK(x3::device::plane_events(ctx, d_lv.as<x3_level>(), stride, n_bins, bin_len, so.as<uint64_t>() + s.n_frames, rule, nullptr,
                                   d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), d_mask.as<uint32_t>(), d_el.as<x3_level>(), cap,
                                   d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
    CHECK(count == want.size());
    CHECK(d_starts.download(starts.data(), 8 * cap) == x3::X3Error::Ok && d_lens.download(lens.data(), 4 * cap) == x3::X3Error::Ok);
    CHECK(d_mask.download(mask.data(), 4 * cap) == x3::X3Error::Ok && d_el.download(el.data(), 32 * 2 * cap) == x3::X3Error::Ok);
    CHECK(d_cnt.download(&dev_count, 8) == x3::X3Error::Ok && dev_count == count);
    uint32_t seen = 0;
    for (size_t i = 0; i < cap; ++i) {
      const Event e = i < want.size() ? want[i] : Event{0, 0, 0};
      CHECK(starts[i] == e.start && lens[i] == e.len && mask[i] == e.mask);
      seen |= mask[i];
      int32_t mx = -32768;
      for (uint64_t g = e.start; g < e.start + e.len; ++g) mx = std::max<int32_t>(mx, wav[g]);
      CHECK(el[i].n == e.len && el[i].max == mx);                            // plane 0: the samples of the event
      CHECK(el[cap + i].n == e.len - (e.start == 0 && e.len ? 1u : 0u));      // plane 1: no difference at position 0
      CHECK(i < want.size() || (el[i].min == 32767 && el[cap + i].min == 32767 && el[cap + i].max == -32768));
    }
    CHECK(seen == 3u);
  }
  // refusals of the mirror and of the call: values that are not one per plane; a stride below the rows; min_planes above K
  uint64_t count = 0;
  x3::device::PlaneEventRule bad = rule;
  bad.mean_sq_min = {1, 2, 3};
  CHECK(!bad.ok());
  CHECK(x3::device::plane_events(ctx, d_lv.as<x3_level>(), stride, n_bins, bin_len, so.as<uint64_t>() + s.n_frames, bad, nullptr,
                                 d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, nullptr, cap, d_cnt.as<uint64_t>(),
                                 &count) == x3::X3Error::BadArg);
  CHECK(x3::device::plane_events(ctx, d_lv.as<x3_level>(), n_bins - 1, n_bins, bin_len, so.as<uint64_t>() + s.n_frames, rule, nullptr,
                                 d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, nullptr, cap, d_cnt.as<uint64_t>(),
                                 &count) == x3::X3Error::BadArg);
  bad = rule;
  bad.min_planes = 3;
  CHECK(x3::device::plane_events(ctx, d_lv.as<x3_level>(), stride, n_bins, bin_len, so.as<uint64_t>() + s.n_frames, bad, nullptr,
                                 d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, nullptr, cap, d_cnt.as<uint64_t>(),
                                 &count) == x3::X3Error::BadArg);
  // a corpus that holds the stream twice: every event twice, entries 0 then 1; a cap below the count, no masks, no levels
  const std::vector<uint64_t> offs = {0, 0}, lns = {s.len, s.len};
  x3::device::Corpus corpus;
  CHECK(corpus.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lns, 0, params, 32, true) == x3::X3Error::Ok);
  const std::vector<uint64_t> rf = corpus.levels_rows(bin_len);
  CHECK(rf.size() == 3 && rf[2] == 2 * n_bins);
  x3::device::Buffer d_rows(ctx, sizeof(x3_level) * 2 * rf[2]), d_ent(ctx, 4 * cap);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>(), rf[2], nullptr, &r) == x3::X3Error::Ok && r.n_bad == 0);
  CHECK(corpus.levels(ctx, bin_len, d_rows.as<x3_level>() + rf[2], rf[2], nullptr, &r, x3::device::LevelSignal::Diff) ==
            x3::X3Error::Ok && r.n_bad == 0);
  rule.min_planes = 1;
  const std::vector<Event> want = detect(wav, bin_len, peak_x, peak_d, 1);
  const uint64_t small = want.size() + 2;
  CHECK(small <= cap);
  CHECK(corpus.plane_events(ctx, d_rows.as<x3_level>(), rf[2], rf[2] - 1, bin_len, rule, nullptr, d_ent.as<uint32_t>(),
                            d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), nullptr, nullptr, small, d_cnt.as<uint64_t>(),
                            &count) == x3::X3Error::BadArg);
  CHECK(corpus.plane_events(ctx, d_rows.as<x3_level>(), rf[2], rf[2], bin_len, rule, nullptr, d_ent.as<uint32_t>(),
                            d_starts.as<uint64_t>(), d_lens.as<uint32_t>(), d_mask.as<uint32_t>(), nullptr, small,
                            d_cnt.as<uint64_t>(), &count) == x3::X3Error::Ok);
  CHECK(count == 2 * want.size());
  std::vector<uint32_t> ent(small);
  CHECK(d_ent.download(ent.data(), 4 * small) == x3::X3Error::Ok && d_starts.download(starts.data(), 8 * small) == x3::X3Error::Ok);
  CHECK(d_lens.download(lens.data(), 4 * small) == x3::X3Error::Ok && d_mask.download(mask.data(), 4 * small) == x3::X3Error::Ok);
  for (size_t i = 0; i < small; ++i) {
    const Event e = want[i % want.size()];
    CHECK(ent[i] == i / want.size() && starts[i] == e.start && lens[i] == e.len && mask[i] == e.mask);
  }
  std::printf("test_plane_events_hpp ok\n");
  return 0;
}
