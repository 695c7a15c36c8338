// Exercises x3::device::decode_streams of x3-rust_amd/host/x3.hpp (x3_decode_streams_dev): a small ragged batch of
// streams in both formats against the samples they were encoded from, and one damaged entry between clean ones.  Needs a
// GPU.   usage: test_streams_hpp
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
  x3::Context ctx(0);
  x3::Parameters params;
  const x3_params cp = params.c_params();
  const std::vector<size_t> ns = {25000, 1, 10000, 47123};
  const uint64_t row_len = 48000;
  std::vector<std::vector<int16_t>> wavs;
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offs, lens;
  for (size_t i = 0; i < ns.size(); ++i) {
    std::vector<int16_t> w(ns[i]);
    CHECK(x3_synth(2, 0x5900 + i, 0, ns[i], w.data()) == 0);
    std::vector<uint8_t> out(x3_encode_bound(ns[i], &cp) + 64);
    uint64_t pos = 0;
    CHECK(x3_encode(ctx.raw(), w.data(), ns[i], 1, &cp, out.data(), out.size(), 0, &pos, nullptr) == X3_OK);
    if (blob.size() & 1) blob.push_back(0);
    offs.push_back(blob.size());
    lens.push_back(pos);
    blob.insert(blob.end(), out.begin(), out.begin() + pos);
    wavs.push_back(w);
  }
  const size_t n = ns.size();
  x3::device::Buffer d_x3(ctx, blob.size() + 16), d_res(ctx, sizeof(x3_stream_result) * n);
  CHECK(d_x3.upload(blob.data(), blob.size()) == x3::X3Error::Ok);
  for (int fmt : {X3_WINDOW_I16, X3_WINDOW_F32}) {
    const size_t esz = fmt == X3_WINDOW_F32 ? 4 : 2;
    x3::device::Buffer d_out(ctx, esz * n * row_len);
    x3::device::WindowsResult r;
    CHECK(x3::device::decode_streams(ctx, d_x3.as<uint8_t>(), blob.size(), offs, lens, 0, params, d_out.data(), row_len, fmt,
                                     d_res.as<x3_stream_result>(), &r) == x3::X3Error::Ok);
    CHECK(r.n_bad == 0 && r.first_bad == n);
    std::vector<uint8_t> rows(esz * n * row_len);
    std::vector<x3_stream_result> res(n);
    CHECK(d_out.download(rows.data(), rows.size()) == x3::X3Error::Ok);
    CHECK(d_res.download(res.data(), sizeof(x3_stream_result) * n) == x3::X3Error::Ok);
    for (size_t i = 0; i < n; ++i) {
      CHECK(res[i].status == 0 && res[i].n_out == ns[i] && res[i].frame_errors == 0);
      for (uint64_t j = 0; j < row_len; ++j) {
        const int16_t want = j < ns[i] ? wavs[i][j] : 0;
        if (fmt == X3_WINDOW_I16) {
          int16_t got;
          std::memcpy(&got, rows.data() + 2 * (i * row_len + j), 2);
          CHECK(got == want);
        } else {
          float got;
          std::memcpy(&got, rows.data() + 4 * (i * row_len + j), 4);
          CHECK(got == (float)want / 32768.0f);
        }
      }
    }
  }
  // a flipped bit in the second frame's header CRC of entry 2: its first frame stays, the walk stops with the header error
  std::vector<uint8_t> bad = blob;
  const uint64_t f1 = offs[3] + 20 + ((uint64_t)bad[offs[3] + 6] << 8 | bad[offs[3] + 7]);
  bad[f1 + 16] ^= 0x01;
  CHECK(d_x3.upload(bad.data(), bad.size()) == x3::X3Error::Ok);
  x3::device::Buffer d_out(ctx, 2 * n * row_len);
  x3::device::WindowsResult r;
  CHECK(x3::device::decode_streams(ctx, d_x3.as<uint8_t>(), bad.size(), offs, lens, 0, params, d_out.data(), row_len,
                                   X3_WINDOW_I16, d_res.as<x3_stream_result>(), &r) == x3::X3Error::Ok);
  CHECK(r.n_bad == 1 && r.first_bad == 3 && r.first_bad_status == X3_ERR_FRAME_HEADER_INVALID_HEADER_CRC);
  std::vector<x3_stream_result> res(n);
  CHECK(d_res.download(res.data(), sizeof(x3_stream_result) * n) == x3::X3Error::Ok);
  CHECK(res[3].n_out == 10000 && res[3].frames_ok == 1 && res[3].status == X3_ERR_FRAME_HEADER_INVALID_HEADER_CRC);
  CHECK(res[0].status == 0 && res[0].n_out == ns[0]);
  std::printf("test_streams_hpp ok\n");
  return 0;
}
