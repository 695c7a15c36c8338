// Exercises x3::device::Corpus of x3-rust_amd/host/x3.hpp (x3_corpus_build / x3_corpus_windows_dev): a small ragged corpus,
// windows in both formats against the samples they were encoded from, a window one sample past its entry, an entry number
// past the corpus, and a move of the RAII handle.  Needs a GPU.   usage: test_corpus_hpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
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
  x3::Context ctx(0);
  x3::Parameters params;
  const x3_params cp = params.c_params();
  const std::vector<size_t> ns = {25000, 1, 10000, 47123};
  std::vector<std::vector<int16_t>> wavs;
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offs, lens;
  for (size_t i = 0; i < ns.size(); ++i) {
    std::vector<int16_t> w(ns[i]);
    CHECK(x3_synth(2, 0x6900 + i, 0, ns[i], w.data()) == 0);
    std::vector<uint8_t> out(x3_encode_bound(ns[i], &cp) + 64);
    uint64_t pos = 0;
    CHECK(x3_encode(ctx.raw(), w.data(), ns[i], 1, &cp, out.data(), out.size(), 0, &pos, nullptr) == X3_OK);
    if (!(blob.size() & 1)) blob.push_back(0x78);   // (odd offsets)
    offs.push_back(blob.size());
    lens.push_back(pos);
    blob.insert(blob.end(), out.begin(), out.begin() + pos);
    wavs.push_back(w);
  }
  x3::device::Buffer d_x3(ctx, blob.size() + 16);
  CHECK(d_x3.upload(blob.data(), blob.size()) == x3::X3Error::Ok);
  x3::device::Corpus built;
  CHECK(built.build(ctx, d_x3.as<uint8_t>(), blob.size(), offs, lens, 0, params) == x3::X3Error::Ok);
  x3::device::Corpus corpus(std::move(built));
  CHECK(!built.ok() && corpus.ok());
  CHECK(corpus.n_entries() == ns.size() && corpus.seg_blocks_in_use() == 32);
  CHECK(corpus.total_samples() == 25000 + 1 + 10000 + 47123);
  uint64_t nw = 0;
  CHECK(corpus.seg_index(&nw) != nullptr && nw == x3_seg_index_entries(corpus.n_frames(), &cp, 32));
  const std::vector<x3_corpus_entry> ent = corpus.entries();
  for (size_t i = 0; i < ns.size(); ++i) CHECK(ent[i].n_samples == ns[i] && ent[i].walk_status == 0 && ent[i].general_walk == 0);
  const uint32_t L = 5000;
  const std::vector<uint32_t> e = {3, 0, 2, 3, 0, 9};
  const std::vector<uint64_t> st = {42123, 0, 5000, 42124, 20000, 0};
  const std::vector<int32_t> want_st = {0, 0, 0, X3_ERR_BAD_ARG, 0, X3_ERR_BAD_ARG};
  const size_t n = e.size();
  x3::device::Buffer d_e(ctx, 4 * n), d_s(ctx, 8 * n), d_st(ctx, 4 * n);
  CHECK(d_e.upload(e.data(), 4 * n) == x3::X3Error::Ok && d_s.upload(st.data(), 8 * n) == x3::X3Error::Ok);
  for (int fmt : {X3_WINDOW_I16, X3_WINDOW_F32}) {
    const size_t esz = fmt == X3_WINDOW_F32 ? 4 : 2;
    x3::device::Buffer d_out(ctx, esz * n * L);
    x3::device::WindowsResult r;
    CHECK(corpus.windows(ctx, d_e.as<uint32_t>(), d_s.as<uint64_t>(), n, L, d_out.data(), fmt, d_st.as<int32_t>(), &r) ==
          x3::X3Error::Ok);
    CHECK(r.n_bad == 2 && r.first_bad == 3 && r.first_bad_status == X3_ERR_BAD_ARG);
    std::vector<uint8_t> rows(esz * n * L);
    std::vector<int32_t> got_st(n);
    CHECK(d_out.download(rows.data(), rows.size()) == x3::X3Error::Ok);
    CHECK(d_st.download(got_st.data(), 4 * n) == x3::X3Error::Ok);
    for (size_t i = 0; i < n; ++i) {
      CHECK(got_st[i] == want_st[i]);
      for (uint32_t j = 0; j < L; ++j) {
        const int16_t want = want_st[i] == 0 ? wavs[e[i]][st[i] + j] : 0;
        if (fmt == X3_WINDOW_I16) {
          int16_t got;
          std::memcpy(&got, rows.data() + 2 * (i * L + j), 2);
          CHECK(got == want);
        } else {
          float got;
          std::memcpy(&got, rows.data() + 4 * (i * L + j), 4);
          CHECK(got == (float)want / 32768.0f);
        }
      }
    }
  }
  std::printf("test_corpus_hpp ok\n");
  return 0;
}
