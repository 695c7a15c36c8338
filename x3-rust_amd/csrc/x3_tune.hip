// x3_tune.hip -- parameter tuning of libx3hip.so: the candidate grid, the accumulating tuner on device buffers, x3_tune on
// a host buffer and the tuned .x3a encode (C ABI: include/x3hip.h, "Parameter tuning"; kernel: x3_tune_kernel.h).
#include "x3_internal.h"
#include <unistd.h>
#include "x3_tune_kernel.h"

#define X3T_DEFAULT_INDEX 1188u   // (20; 3, 8, 20): 728 + rank of (3, 8, 20) = 728 + 390 + 5 * 13 + 5

struct x3_tuner {
  x3_ctx* c;
  uint32_t spf;
  unsigned long long* d_tot;   // X3T_CANDIDATES byte totals, then X3T_CANDIDATES uint32 largest payloads
};

static bool spf_ok(uint32_t spf) { return spf >= 40u && spf <= 10240u && spf % 40u == 0u; }

extern "C" int x3_tune_candidate(uint32_t index, uint32_t spf, x3_params* p) {
  if (!p || !spf_ok(spf) || index >= X3T_CANDIDATES) return X3_ERR_BAD_ARG;
  const uint32_t g = index / X3T_TRIPLES;
  uint32_t t0 = 0, rem = index % X3T_TRIPLES;
  while (rem >= (11u - t0) * 13u) rem -= (11u - t0++) * 13u;
  p->block_len = 10u << g;
  p->blocks_per_frame = spf / p->block_len;
  p->codes[0] = 0; p->codes[1] = 1; p->codes[2] = 3;
  p->thresholds[0] = t0;
  p->thresholds[1] = t0 + rem / 13u;
  p->thresholds[2] = 15u + rem % 13u;
  return X3_OK;
}

static int tuner_clear(x3_tuner* t) {
  x3_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(t->d_tot, 0, X3T_CANDIDATES * (sizeof(unsigned long long) + sizeof(uint32_t)), c->stream));
  return X3_OK;
}

extern "C" int x3_tuner_create(x3_ctx* c, uint32_t spf, x3_tuner** out) {
  if (!c || !out || !spf_ok(spf)) return X3_ERR_BAD_ARG;
  *out = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  x3_tuner* t = new x3_tuner{c, spf, nullptr};
  if (x3_dmalloc(&t->d_tot, X3T_CANDIDATES * (sizeof(unsigned long long) + sizeof(uint32_t))) != hipSuccess) {
    c->last_error = "x3_tuner_create: device allocation failed";
    delete t;
    return X3_ERR_HIP;
  }
  const int rc = tuner_clear(t);
  if (rc) {
    (void)x3_dfree(t->d_tot);
    delete t;
    return rc;
  }
  *out = t;
  return X3_OK;
}

extern "C" void x3_tuner_destroy(x3_tuner* t) {
  if (!t) return;
  (void)hipSetDevice(t->c->device);
  (void)hipStreamSynchronize(t->c->stream);
  (void)x3_dfree(t->d_tot);
  delete t;
}

extern "C" int x3_tuner_reset(x3_tuner* t) {
  if (!t) return X3_ERR_BAD_ARG;
  return tuner_clear(t);
}

extern "C" int x3_tuner_add_dev(x3_tuner* t, const int16_t* d_wav, const x3_batch* b) {
  if (!t || !d_wav || !b) return X3_ERR_BAD_ARG;
  if (((uintptr_t)d_wav & 1u) != 0) return X3_ERR_BAD_ARG;   // samples on their own 2-byte boundaries
  if (b->n_per_clip == 0 || b->n_clips == 0) return X3_ERR_BAD_ARG;
  if (b->n_clips > 1 && b->clip_stride < b->n_per_clip) return X3_ERR_BAD_ARG;
  const uint64_t fpc = (b->n_per_clip + t->spf - 1) / t->spf;
  if (fpc > 0xFFFFFFFFull || b->n_clips > (~0ull >> 2) / fpc) return X3_ERR_BAD_ARG;
  x3_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  X3TuneArgs a;
  a.wav = d_wav;
  a.n_per_clip = b->n_per_clip;
  a.clip_stride = b->n_clips > 1 ? b->clip_stride : 0;
  a.n_frames = fpc * b->n_clips;
  a.spf = t->spf;
  a.fpc = (uint32_t)fpc;
  a.tot = t->d_tot;
  a.maxpay = reinterpret_cast<uint32_t*>(t->d_tot + X3T_CANDIDATES);
  const uint64_t nwg = std::min<uint64_t>((uint64_t)std::max(c->n_cus, 1), (a.n_frames + X3T_WAVES - 1) / X3T_WAVES);
  hipLaunchKernelGGL(x3_tune_kernel, dim3((unsigned)nwg), dim3(X3T_THREADS), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return X3_OK;
}

extern "C" int x3_tuner_result(x3_tuner* t, x3_params* best, uint64_t* best_bytes, uint64_t* sizes) {
  if (!t) return X3_ERR_BAD_ARG;
  x3_ctx* c = t->c;
  std::vector<unsigned long long> h(X3T_CANDIDATES);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(h.data(), t->d_tot, X3T_CANDIDATES * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the smallest total; among equal ones the default set, else the lowest index
  uint32_t k = X3T_DEFAULT_INDEX;
  for (uint32_t i = 0; i < X3T_CANDIDATES; ++i)
    if (h[i] < h[k]) k = i;   // (k starts at the default; a later equal total never replaces an earlier one)
  if (best) (void)x3_tune_candidate(k, t->spf, best);
  if (best_bytes) *best_bytes = h[k];
  if (sizes)
    for (uint32_t i = 0; i < X3T_CANDIDATES; ++i) sizes[i] = h[i];
  return X3_OK;
}

extern "C" int x3_tuner_max_payloads(x3_tuner* t, uint32_t* payloads) {
  if (!t || !payloads) return X3_ERR_BAD_ARG;
  x3_ctx* c = t->c;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(payloads, t->d_tot + X3T_CANDIDATES, X3T_CANDIDATES * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return X3_OK;
}

// a host buffer in chunks of whole frames through the context's input buffer
static int tune_host(x3_ctx* c, const int16_t* wav, uint64_t n, x3_tuner* t) {
  const uint64_t chunk = std::max<uint64_t>(1, (16ull << 20) / t->spf) * t->spf;
  if (ensure(c, c->in, std::min(n, chunk) * sizeof(int16_t))) return X3_ERR_HIP;
  for (uint64_t at = 0; at < n; at += chunk) {
    const uint64_t len = std::min(chunk, n - at);
    HIPCHK(c, hipMemcpyAsync(c->in.p, wav + at, len * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    const x3_batch b{len, len, 1};
    const int rc = x3_tuner_add_dev(t, static_cast<const int16_t*>(c->in.p), &b);
    if (rc) return rc;
  }
  return X3_OK;
}

extern "C" int x3_tune(x3_ctx* c, const int16_t* wav, uint64_t n, uint32_t spf, x3_params* best, uint64_t* best_bytes,
                       uint64_t* sizes) {
  if (!c || !wav || n == 0 || !spf_ok(spf)) return X3_ERR_BAD_ARG;
  x3_tuner* t = nullptr;
  int rc = x3_tuner_create(c, spf, &t);
  if (rc) return rc;
  rc = tune_host(c, wav, n, t);
  if (!rc) rc = x3_tuner_result(t, best, best_bytes, sizes);
  x3_tuner_destroy(t);
  return rc;
}

int tune_fd(x3_ctx* c, int fd, uint64_t data_off, uint64_t n, x3_params* best) {
  x3_tuner* t = nullptr;
  int rc = x3_tuner_create(c, X3_TUNE_DEFAULT_SPF, &t);
  if (rc) return rc;
  const uint64_t chunk = (16ull << 20) / X3_TUNE_DEFAULT_SPF * X3_TUNE_DEFAULT_SPF;   // whole frames
  std::vector<int16_t> buf(std::min(n, chunk));
  for (uint64_t at = 0; at < n && !rc; at += chunk) {
    const uint64_t len = std::min(chunk, n - at);
    uint64_t got = 0;
    while (got < 2 * len) {
      const ssize_t r = ::pread(fd, reinterpret_cast<char*>(buf.data()) + got, 2 * len - got, (off_t)(data_off + 2 * at + got));
      if (r <= 0) break;
      got += (uint64_t)r;
    }
    if (got < 2 * len) {
      rc = X3_ERR_IO;
      break;
    }
    rc = tune_host(c, buf.data(), len, t);   // (WAV samples are little-endian, as is the host)
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = X3_ERR_HIP;   // the buffer is read again next
  }
  if (!rc) rc = x3_tuner_result(t, best, nullptr, nullptr);
  x3_tuner_destroy(t);
  return rc;
}

extern "C" int x3_x3a_encode_tuned(x3_ctx* c, const int16_t* wav, uint64_t n, uint32_t sample_rate, uint8_t* out,
                                   uint64_t out_cap, uint64_t* out_len, uint64_t stats[6], x3_params* chosen) {
  if (!c || (!wav && n) || (!out && out_cap)) return X3_ERR_BAD_ARG;
  x3_params p;
  x3_params_default(&p);
  if (n) {
    const int rc = x3_tune(c, wav, n, X3_TUNE_DEFAULT_SPF, &p, nullptr, nullptr);
    if (rc) return rc;
  }
  if (chosen) *chosen = p;
  uint64_t hlen = 0;
  int rc = x3_archive_header_write(sample_rate, &p, out, out_cap, &hlen);
  if (out_len) *out_len = hlen;
  if (rc) return rc;
  uint64_t pos = hlen;
  rc = x3_encode(c, wav, n, 1, &p, out, out_cap, hlen, &pos, stats);
  if (out_len) *out_len = pos;
  return rc;
}
