// Exercises x3::tune, x3::tune_candidate and x3::device::Tuner of x3-rust_amd/host/x3.hpp (parameter tuning): the tuner's
// table against the host-buffer entry point, chunks of whole frames against the whole input, reset, the chosen set against
// an encode with it, and a refused argument.  Needs a GPU.   usage: test_tune_hpp
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
  const size_t n = 254321;
  std::vector<int16_t> wav(n);
  CHECK(x3_synth(4, 0x58330001, 0, n, wav.data()) == 0);   // +-2 LSB random walk

  x3::Parameters best;
  uint64_t best_bytes = 0;
  std::vector<uint64_t> sizes;
  CHECK(x3::tune(ctx, wav.data(), n, &best, &best_bytes, &sizes) == x3::X3Error::Ok);
  CHECK(sizes.size() == X3_TUNE_CANDIDATES && best_bytes > 0 && best_bytes <= sizes[X3_TUNE_DEFAULT_INDEX]);
  for (uint64_t s : sizes) CHECK(s >= best_bytes);

  x3::device::Buffer d_wav(ctx, 2 * n);
  CHECK(d_wav.upload(wav.data(), 2 * n) == x3::X3Error::Ok);
  x3::device::Tuner t(ctx);
  CHECK(t.status() == x3::X3Error::Ok);
  CHECK(t.add(d_wav.as<int16_t>(), 100000) == x3::X3Error::Ok);             // whole frames ...
  CHECK(t.add(d_wav.as<int16_t>() + 100000, n - 100000) == x3::X3Error::Ok); // ... then the rest
  x3::Parameters b2;
  uint64_t bb2 = 0;
  std::vector<uint64_t> s2;
  CHECK(t.result(&b2, &bb2, &s2) == x3::X3Error::Ok);
  CHECK(s2 == sizes && bb2 == best_bytes && b2.block_len == best.block_len);
  for (int k = 0; k < 3; ++k) CHECK(b2.thresholds[k] == best.thresholds[k]);
  CHECK(t.add(d_wav.as<int16_t>(), 1000, 2, 999) == x3::X3Error::BadArg);   // stride smaller than the clip
  CHECK(t.reset() == x3::X3Error::Ok);
  CHECK(t.result(nullptr, &bb2, &s2) == x3::X3Error::Ok && bb2 == 0);

  // an encode with the chosen set writes exactly best_bytes
  std::vector<uint8_t> out(4 * n + 4096);
  const x3_params c = best.c_params();
  uint64_t pos = 0;
  CHECK(x3_encode(ctx.raw(), wav.data(), n, 1, &c, out.data(), out.size(), 0, &pos, nullptr) == X3_OK);
  CHECK(pos == best_bytes);

  x3::Parameters p;
  CHECK(x3::tune_candidate(X3_TUNE_DEFAULT_INDEX, &p) == x3::X3Error::Ok && p.block_len == 20 && p.thresholds[2] == 20);
  CHECK(x3::tune_candidate(X3_TUNE_CANDIDATES, &p) == x3::X3Error::BadArg);
  std::printf("test_tune_hpp ok: block length %zu, thresholds (%zu, %zu, %zu), %llu bytes (default %llu)\n", best.block_len,
              best.thresholds[0], best.thresholds[1], best.thresholds[2], (unsigned long long)best_bytes,
              (unsigned long long)sizes[X3_TUNE_DEFAULT_INDEX]);
  return 0;
}
