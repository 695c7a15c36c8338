// The kernel a decode or encode call takes (decode_route, encode_route: x3_internal.h), over a grid of parameters, layouts,
// pointer alignments and options, against the rules written out below.  Host code only: no context, no GPU.
// Prints "ok decode=<cases> encode=<cases>", or the first cases that disagree and exits 1.
#include <cstdio>
#include <cstdint>

#include "x3_internal.h"

static const uint32_t CODES[][3] = {{0, 1, 3}, {1, 1, 3}, {2, 1, 3}, {3, 1, 3}, {0, 0, 0}, {0, 2, 3}};
static const uint32_t THRESHOLDS[][3] = {{3, 8, 20}, {6, 10, 27}, {6, 10, 28}, {2, 4, 6}, {9, 4, 20}};
static const uint32_t BLOCK_LENGTHS[] = {10, 13, 20, 40};
static const uint32_t BLOCKS_PER_FRAME[] = {1, 2, 3, 4, 100, 103, 511, 513};   // spf = 0, 4, 8 mod 16, 2 mod 4, ...
static const uint64_t STRIDE_PAD[] = {0, 1, 2, 4, 8, 16};                      // clip stride - samples per clip
static const uintptr_t WAV_ALIGN[] = {2, 4, 8, 16};
static const uintptr_t WAV_BASE = 0x7f0000000000ull;                           // (a pointer value, never dereferenced)

static int failures = 0;
static void fail(const char* what) {
  if (++failures <= 20) std::printf("%s\n", what);
}

// ---- decoder.  Kernels: 3 block per lane, 2 three waves, 1 single wave (branch-free), 0 single wave (general) -- the table
// of tests/test_gpu_code_sets.py, expected_kernel, plus the layouts and the segment index.
static int want_kernel(const uint32_t* codes, uint32_t bl, bool rows8, bool single, bool blocks, bool blocks_off, int seg_mode) {
  if (codes[0] > 1) return 0;                       // a Rice codeword of codes 2 and 3 can pass 32 bits
  if (codes[1] != 1 || codes[2] != 3 || single || !rows8) return 1;
  if (bl == 20) return blocks && seg_mode == 0 ? 3 : 2;
  if (bl == 10 || bl == 40) return blocks_off ? 1 : 3;
  return 1;
}

static long check_decode() {
  long n = 0;
  for (const auto& codes : CODES)
    for (uint32_t bl : BLOCK_LENGTHS)
      for (uint32_t bpf : BLOCKS_PER_FRAME) {
        const x3_params p{bl, bpf, {codes[0], codes[1], codes[2]}, {3, 8, 20}};
        const uint64_t spf = (uint64_t)bl * bpf;
        X3DevParams dp;
        if (derive(&p, spf, &dp)) { fail("derive"); continue; }
        // layouts: 0 = uniform batch, 1 = caller's offsets, 2 = caller's offsets that are multiples of four samples
        for (int layout = 0; layout < 3; ++layout)
          for (uint64_t clips : {1ull, 3ull})
            for (uint64_t tail : {0ull, 3ull})                 // (samples missing from a clip's last frame)
              for (uint64_t pad : STRIDE_PAD) {
                if (layout && (clips > 1 || tail || pad)) continue;
                if (clips == 1 && pad) continue;
                const uint64_t n_per_clip = 5 * spf - tail, stride = n_per_clip + pad;
                const uint64_t fpc = (n_per_clip + spf - 1) / spf;
                X3Geom g{0, 0, 1, 5};
                if (layout == 0) g = X3Geom{n_per_clip, stride, (uint32_t)fpc, fpc * clips};
                for (uintptr_t a : WAV_ALIGN) {
                  const int16_t* wav = reinterpret_cast<const int16_t*>(WAV_BASE + a);
                  // rows on 8-byte boundaries: the pointer, and every frame start a multiple of four samples -- frames of a
                  // multiple of four samples in clips at a stride of one, or offsets the caller vouches for
                  const bool rows8 = a % 8 == 0 && (layout == 0 ? spf % 4 == 0 && (clips == 1 || stride % 4 == 0) : layout == 2);
                  for (int seg_mode = 0; seg_mode < 3; ++seg_mode)
                    for (int opt = 0; opt < 8; ++opt) {
                      X3Opts o;
                      o.decode_single = opt & 1;
                      o.decode_blocks = (opt >> 1) & 1;
                      o.decode_blocks_off = (opt >> 2) & 1;
                      const DecodeRoute r = decode_route(dp, g, wav, layout != 0, layout == 2, seg_mode, o);
                      const int want = want_kernel(codes, bl, rows8, o.decode_single, o.decode_blocks, o.decode_blocks_off, seg_mode);
                      // the frame count from device memory: the block-length-20 decoders (the one-trip walk's decode)
                      const bool want_dev = bl == 20 && want >= 2;
                      const uint32_t want_unit = want == 3 ? (bl == 10 ? 10u : 20u) : 0u;
                      const uint32_t want_upb = want == 3 ? (bl == 40 ? 2u : 1u) : 0u;
                      ++n;
                      if (r.kernel != want || r.device_count != want_dev || r.unit != want_unit || r.upb != want_upb) {
                        char msg[320];
                        std::snprintf(msg, sizeof msg,
                                      "decode codes %u%u%u bl %u bpf %u layout %d clips %llu tail %llu pad %llu align %u seg %d "
                                      "opt %d: kernel %d <%u,%u> dev %d, want %d <%u,%u> dev %d",
                                      codes[0], codes[1], codes[2], bl, bpf, layout, (unsigned long long)clips,
                                      (unsigned long long)tail, (unsigned long long)pad, (unsigned)a, seg_mode, opt, r.kernel,
                                      r.unit, r.upb, (int)r.device_count, want, want_unit, want_upb, (int)want_dev);
                        fail(msg);
                      }
                    }
                }
              }
      }
  return n;
}

// ---- encoder.  Generations: 3 wave, 2 second generation, 1 look-back, 0 two passes -- tests/test_gpu_code_sets.py,
// expected_gen, plus the layouts, the LDS of a second-generation workgroup and the context's state.
static const uint32_t RICE_OFFSET[4] = {6, 11, 20, 28}, RICE_LEN[4] = {14, 22, 40, 56};

// no block can need a difference outside its code's table (a block of max |d| = m takes code[(m > thr0) + (m > thr1)])
static bool stream_safe(const uint32_t* codes, const uint32_t* thr) {
  for (uint32_t m = 0; m <= thr[2]; ++m) {
    const uint32_t c = codes[(m > thr[0]) + (m > thr[1])];
    if (m > RICE_OFFSET[c] || m > RICE_LEN[c] - RICE_OFFSET[c] - 1) return false;
  }
  return true;
}

static int want_gen(const uint32_t* codes, const uint32_t* thr, uint32_t bl, uint64_t spf, uint64_t n, bool layout_ok,
                    size_t smem2, const X3Opts& o, bool prefer_gen2, bool force_two_pass) {
  if (o.two_pass || force_two_pass) return 0;
  if ((bl != 10 && bl != 20 && bl != 40) || spf % 4 || ((spf < n ? spf : n) + 18) / 20 > 512 || !layout_ok ||
      !stream_safe(codes, thr) || smem2 > 160 * 1024)
    return 1;
  return o.enc_gen == 3 && o.stream_wgs == 0 && !prefer_gen2 ? 3 : 2;
}

static long check_encode() {
  long n = 0;
  for (const auto& codes : CODES)
    for (const auto& thr : THRESHOLDS)
      for (uint32_t bl : BLOCK_LENGTHS)
        for (uint32_t bpf : BLOCKS_PER_FRAME) {
          const x3_params p{bl, bpf, {codes[0], codes[1], codes[2]}, {thr[0], thr[1], thr[2]}};
          const uint64_t spf = (uint64_t)bl * bpf;
          // layouts: 0 = uniform batch, 1 = frame table of even offsets, 2 = of offsets not all even
          for (int layout = 0; layout < 3; ++layout)
            for (uint64_t clips : {1ull, 3ull})
              for (uint64_t n_per_clip : {5 * spf, 3 * spf - 2, (uint64_t)10000})
                for (uint64_t pad : STRIDE_PAD) {
                  if (layout && (clips > 1 || pad || n_per_clip != 5 * spf)) continue;
                  if (clips == 1 && pad) continue;
                  // (a frame table: n_frames clips of at most one frame each, at a stride of 0)
                  const x3_batch b = layout ? x3_batch{spf, 0, 7} : x3_batch{n_per_clip, n_per_clip + pad, clips};
                  const X3FrameTable tab{nullptr, nullptr, layout == 1};
                  for (uintptr_t a : WAV_ALIGN) {
                    const int16_t* wav = reinterpret_cast<const int16_t*>(WAV_BASE + a);
                    // frames on dword boundaries: the pointer, clips at a stride of a multiple of four samples, even
                    // offsets in a frame table (spf: in want_gen)
                    const bool layout_ok = a % 4 == 0 && (layout ? layout == 1 : clips == 1 || (n_per_clip + pad) % 4 == 0);
                    for (size_t smem2 : {(size_t)40 * 1024, (size_t)160 * 1024, (size_t)160 * 1024 + 1})
                      for (int opt = 0; opt < 32; ++opt) {
                        X3Opts o;
                        o.two_pass = opt & 1;
                        o.enc_gen = (opt & 2) ? 2 : 3;
                        o.stream_wgs = (opt & 4) ? 2 : 0;
                        const bool prefer_gen2 = (opt & 8) != 0, force_two_pass = (opt & 16) != 0;
                        const EncodeRoute r = encode_route(&p, spf, &b, layout ? &tab : nullptr, wav, smem2, o, prefer_gen2,
                                                           force_two_pass);
                        const int want = want_gen(codes, thr, bl, spf, b.n_per_clip, layout_ok, smem2, o, prefer_gen2,
                                                  force_two_pass);
                        const uint32_t want_bl = want >= 2 ? bl : 0u;
                        ++n;
                        if (r.gen != want || (want >= 2 && r.bl != want_bl)) {
                          char msg[320];
                          std::snprintf(msg, sizeof msg,
                                        "encode codes %u%u%u thr %u,%u,%u bl %u bpf %u layout %d clips %llu n %llu pad %llu "
                                        "align %u smem2 %zu opt %d: gen %d bl %u, want %d bl %u",
                                        codes[0], codes[1], codes[2], thr[0], thr[1], thr[2], bl, bpf, layout,
                                        (unsigned long long)clips, (unsigned long long)n_per_clip, (unsigned long long)pad,
                                        (unsigned)a, smem2, opt, r.gen, r.bl, want, want_bl);
                          fail(msg);
                        }
                      }
                  }
                }
        }
  return n;
}

int main() {
  const long nd = check_decode();
  const long ne = check_encode();
  if (failures) {
    std::printf("FAILED %d of %ld cases\n", failures, nd + ne);
    return 1;
  }
  std::printf("ok decode=%ld encode=%ld\n", nd, ne);
  return 0;
}
