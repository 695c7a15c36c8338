// Exercises x3::device::build_seg_index, index_by_walk and Corpus::build(..., index_walk) of x3-rust_amd/host/x3.hpp
// (x3_seg_index_build_dev, X3_CORPUS_INDEX_WALK): a stream at block length 40, which no encoder or decoder indexes, gets an
// index by the walk; windows by it are the samples it was encoded from.  Needs a GPU.   usage: test_seg_index_hpp
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
  x3_params cp;
  x3_params_default(&cp);
  cp.block_len = 40;
  cp.blocks_per_frame = 250;
  const x3::Parameters params = x3::Parameters::from_c(cp);
  const size_t n = 123457;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x7100, 0, n, wav.data()) == 0);
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 0, &s) == x3::X3Error::Ok);
  CHECK(s.seg_blocks == 0 && s.n_frames == 13);
  CHECK(x3::device::index_by_walk(ctx, &s, params, 32) == x3::X3Error::Ok);
  CHECK(s.seg_blocks == 32 && s.seg_index.ok() && s.seg_index.size() == 8 * x3_seg_index_entries(s.n_frames, &cp, 32));
  long long irregular = -1;
  CHECK(x3_ctx_get_option(ctx.raw(), "last_seg_index_irregular", &irregular) == X3_OK && irregular == 0);
  std::vector<uint64_t> idx(s.seg_index.size() / 8);
  CHECK(s.seg_index.download(idx.data(), s.seg_index.size()) == x3::X3Error::Ok);
  CHECK(idx[0] == (0x58335347ull | (32ull << 32)));
  for (size_t f = 0; f + 1 < s.n_frames; ++f)
    for (size_t q = 0; q < 7; ++q) CHECK((idx[1 + 7 * f + q] >> 48) == 1);   // every entry of a full frame is valid
  // frames of one stretch: no index
  x3::device::Buffer none;
  CHECK(x3::device::build_seg_index(ctx, s.bytes.as<uint8_t>(), s.len, s.frame_offsets.as<uint64_t>(), s.n_frames, params, 252,
                                    &none) == x3::X3Error::Ok && !none.ok());
  // windows by the built index
  x3::device::Buffer so;
  CHECK(x3::device::sample_offsets(ctx, s, &so) == x3::X3Error::Ok);
  const uint32_t L = 9000;
  const std::vector<uint64_t> st = {0, 9999, 61234, n - L};
  x3::device::Buffer d_s(ctx, 8 * st.size()), d_st(ctx, 4 * st.size()), d_out(ctx, 2 * st.size() * L);
  CHECK(d_s.upload(st.data(), 8 * st.size()) == x3::X3Error::Ok);
  x3::device::WindowsResult r;
  CHECK(x3::device::decode_windows(ctx, s, params, so, d_s.as<uint64_t>(), st.size(), L, d_out.data(), X3_WINDOW_I16,
                                   d_st.as<int32_t>(), &r) == x3::X3Error::Ok);
  long long replays = -1;
  CHECK(r.n_bad == 0 && x3_ctx_get_option(ctx.raw(), "last_window_replays", &replays) == X3_OK && replays == 0);
  std::vector<int16_t> rows(st.size() * L);
  CHECK(d_out.download(rows.data(), 2 * rows.size()) == x3::X3Error::Ok);
  for (size_t i = 0; i < st.size(); ++i) CHECK(std::memcmp(&rows[i * L], &wav[st[i]], 2 * L) == 0);
  // the corpus option
  std::vector<uint8_t> bytes(s.len);
  CHECK(s.bytes.download(bytes.data(), s.len) == x3::X3Error::Ok);
  const std::vector<uint64_t> offs = {0}, lens = {s.len};
  x3::device::Corpus plain, walked;
  CHECK(plain.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params) == x3::X3Error::Ok);
  CHECK(plain.seg_blocks_in_use() == 0);
  CHECK(walked.build(ctx, s.bytes.as<uint8_t>(), s.len, offs, lens, 0, params, 32, true) == x3::X3Error::Ok);
  CHECK(walked.seg_blocks_in_use() == 32 && walked.n_frames() == s.n_frames);
  uint64_t nw = 0;
  const uint64_t* d_idx = walked.seg_index(&nw);
  CHECK(d_idx != nullptr && nw == idx.size());
  std::vector<uint64_t> cidx(nw);
  CHECK(x3_dev_download(ctx.raw(), cidx.data(), d_idx, 8 * nw) == X3_OK && cidx == idx);
  std::printf("test_seg_index_hpp ok\n");
  return 0;
}
