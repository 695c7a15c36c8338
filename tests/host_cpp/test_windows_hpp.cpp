// Exercises x3::device::sample_offsets / decode_windows of x3-rust_amd/host/x3.hpp (random access, x3_decode_windows_dev):
// a stream encoded with its segment index, windows of both formats against the samples it was encoded from, a window off
// the end.  Needs a GPU.   usage: test_windows_hpp
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

int main() {
  x3::Context ctx(0);
  x3::Parameters params;
  const size_t n = 321000;
  const uint32_t L = 4000;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(2, 0x5835, 0, n, wav.data()) == 0);
  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::EncodedStream s;
  CHECK(x3::device::encode(ctx, d_wav.as<int16_t>(), n, 1, params, 32, &s) == x3::X3Error::Ok);
  x3::device::Buffer d_so;
  CHECK(x3::device::sample_offsets(ctx, s, &d_so) == x3::X3Error::Ok);
  const std::vector<uint64_t> starts = {0, 9998, 123456, n - L, n - L + 1};
  x3::device::Buffer d_starts(ctx, 8 * starts.size()), d_status(ctx, 4 * starts.size());
  CHECK(d_starts.upload(starts.data(), 8 * starts.size()) == x3::X3Error::Ok);
  for (int fmt : {X3_WINDOW_I16, X3_WINDOW_F32}) {
    const size_t esz = fmt == X3_WINDOW_F32 ? 4 : 2;
    x3::device::Buffer d_out(ctx, esz * starts.size() * L);
    x3::device::WindowsResult r;
    CHECK(x3::device::decode_windows(ctx, s, params, d_so, d_starts.as<uint64_t>(), starts.size(), L, d_out.data(), fmt,
                                     d_status.as<int32_t>(), &r) == x3::X3Error::Ok);
    CHECK(r.n_bad == 1 && r.first_bad == 4 && r.first_bad_status == X3_ERR_BAD_ARG);
    std::vector<int32_t> st(starts.size());
    CHECK(d_status.download(st.data(), 4 * st.size()) == x3::X3Error::Ok);
    std::vector<uint8_t> out(esz * starts.size() * L);
    CHECK(d_out.download(out.data(), out.size()) == x3::X3Error::Ok);
    for (size_t w = 0; w < starts.size(); ++w) {
      const bool off_end = starts[w] + L > n;
      CHECK(st[w] == (off_end ? X3_ERR_BAD_ARG : 0));
      for (uint32_t i = 0; i < L; ++i) {
        const int16_t want = off_end ? 0 : wav[starts[w] + i];
        if (fmt == X3_WINDOW_F32) CHECK(reinterpret_cast<const float*>(out.data())[w * L + i] == (float)want / 32768.0f);
        else CHECK(reinterpret_cast<const int16_t*>(out.data())[w * L + i] == want);
      }
    }
  }
  std::printf("test_windows_hpp: ok\n");
  return 0;
}
