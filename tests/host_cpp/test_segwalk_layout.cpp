// The segmented walk's entry table and workspace (seg_entries, segwalk_carve, streams_carve: x3_internal.h) on the CPU:
// span counts against their formula, the refusals, and the carved pieces -- disjoint, aligned for their elements, long
// enough for what the kernels of x3_streams_kernel.h index, inside the returned size, the entry table in ONE piece (it
// goes up in one copy); the batch decode's block: the same walk pieces, its own behind them.  The workspaces of the windows /
// ranges calls and of the levels calls (windows_carve, levels_carve): every piece's offset and the total against the chains
// of rounded offsets that laid them out before there was a carver, written out below -- the layout must not move, a
// same-size workspace keeps the context's allocations where they are.  Host code only: no context.
// Prints "ok tables=<cases> carves=<cases> windows=<cases> levels=<cases>", or the first cases that disagree and exits 1.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "x3_internal.h"

// (as x3_streams_kernel.h and x3_index_kernels.h have them: kernel headers, which a host-only driver cannot include)
static const uint64_t SPAN_BYTES = 65536, WG_CANDS = 256;
struct X3Cand { unsigned long long off; uint32_t plen_kind, samples; };
struct X3StreamsSum { unsigned long long bad_first; unsigned int n_bad, n_dirty, over, pad[3]; };
// (as x3_decode_window_kernel.h and x3_levels_kernel.h have them)
struct X3WinPlan { uint64_t fa; uint32_t ncov; int32_t status; };
struct X3WinSummary { unsigned long long n_bad, first, replays, total; };
struct X3LevSummary { unsigned long long n_bad, first, replays; };
struct X3LevFrame { uint64_t pos, obase, nlim, b0; };

static const uint64_t NS[] = {1, 2, 3, 7, 8, 1000};
static const uint64_t LENGTHS[] = {0, 1, 21, 65535, 65536, 65537, 3 * 65536};
static const uintptr_t BASE = 0x7f0000000000ull;   // (a pointer value, never dereferenced)

static int failures = 0;
static void fail(const char* what, uint64_t n, uint64_t variant) {
  if (++failures <= 20) std::printf("%s: n %llu variant %llu\n", what, (unsigned long long)n, (unsigned long long)variant);
}

static uint64_t rnd(uint64_t& s) {   // xorshift64
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

struct Piece { const char* name; uintptr_t at; uint64_t count, size, align; };

static long check_carve(uint64_t n, uint64_t G, uint64_t variant) {
  SegWalkWs w0, w1;
  StreamsWs w, s0;
  const size_t walk_total = segwalk_carve(reinterpret_cast<char*>(BASE), n, G, &w1);
  const size_t total = streams_carve(reinterpret_cast<char*>(BASE), n, G, &w);
  if (segwalk_carve(nullptr, n, G, &w0) != walk_total || streams_carve(nullptr, n, G, &s0) != total)
    fail("size without a base differs", n, variant);
  const uint64_t cap = G * WG_CANDS > 1 ? G * WG_CANDS : 1;
  // the table is what segwalk_launch copies to eoff in one piece: 8n + 8n + 4(n + 1) bytes, nothing in between
  if (reinterpret_cast<uintptr_t>(w1.elen) != reinterpret_cast<uintptr_t>(w1.eoff) + 8 * n ||
      reinterpret_cast<uintptr_t>(w1.span_first) != reinterpret_cast<uintptr_t>(w1.elen) + 8 * n)
    fail("entry table not in one piece", n, variant);
#define PIECE(field, count) {#field, reinterpret_cast<uintptr_t>(w.field), count, sizeof(*w.field), alignof(decltype(*w.field))}
  // the batch decode's block: the walk's pieces where the walk's own carve puts them, inside ITS size, then the call's words
  const Piece pieces[] = {PIECE(eoff, n), PIECE(elen, n), PIECE(span_first, n + 1), PIECE(isum, 1), PIECE(cnt, G), PIECE(base, G),
                          PIECE(samp, G), PIECE(sbase, G), PIECE(cand, cap), PIECE(frame_off, cap), PIECE(wav_off, cap),
                          PIECE(fent, cap), PIECE(ent_flags, n), PIECE(ent_end, n), PIECE(ent_nsamp, n),
                          PIECE(sum, 1), PIECE(status, cap), PIECE(ent_bad, n), PIECE(nout, n), PIECE(dirty, n)};
#undef PIECE
  const uintptr_t* const pa = reinterpret_cast<const uintptr_t*>(static_cast<const SegWalkWs*>(&w));
  const uintptr_t* const pb = reinterpret_cast<const uintptr_t*>(&w1);
  for (size_t i = 0; i < sizeof(SegWalkWs) / sizeof(uintptr_t); ++i)
    if (pa[i] != pb[i]) fail("walk pieces differ between the two carves", n, variant);
  for (size_t i = 0; i < 15; ++i)
    if (pieces[i].at + pieces[i].count * pieces[i].size > BASE + walk_total) fail("walk piece behind the walk's size", n, variant);
  for (size_t i = 15; i < 20; ++i)
    if (pieces[i].at < BASE + walk_total) fail("own piece inside the walk's size", n, variant);
  for (const Piece& a : pieces) {
    const uintptr_t end = a.at + a.count * a.size;
    if (a.at % a.align) fail(a.name, n, variant);                      // aligned for its element
    if (a.at < BASE || end > BASE + total) fail(a.name, n, variant);   // inside the block
    for (const Piece& b : pieces)                                      // disjoint from every other piece
      if (&a != &b && a.at < b.at + b.count * b.size && b.at < end) fail(a.name, n, variant);
  }
  return 1;
}

// every piece where the chain of offsets puts it, aligned for its element, inside the block and disjoint from the others
struct Placed { const char* name; const void* at; uint64_t want_off, count, size, align; };
static void check_placed(const Placed* pieces, size_t n_pieces, size_t total, size_t want_total, uint64_t a, uint64_t b) {
  if (total != want_total) fail("total", a, b);
  for (size_t i = 0; i < n_pieces; ++i) {
    const Placed& p = pieces[i];
    const uintptr_t at = reinterpret_cast<uintptr_t>(p.at), end = at + p.count * p.size;
    if (at != BASE + p.want_off) fail(p.name, a, b);
    if (at % p.align) fail(p.name, a, b);
    if (at < BASE || end > BASE + total) fail(p.name, a, b);
    for (size_t j = 0; j < n_pieces; ++j) {
      const uintptr_t bt = reinterpret_cast<uintptr_t>(pieces[j].at);
      if (i != j && at < bt + pieces[j].count * pieces[j].size && bt < end) fail(p.name, a, b);
    }
  }
}
#define PLACED(w, field, off, count) {#field, (w).field, off, count, sizeof(*(w).field), alignof(decltype(*(w).field))}
static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }

static const uint64_t WIN_N[] = {1, 2, 255, 256, 257, 1000, (1ull << 20) + 1};
static const uint64_t FRAMES[] = {1, 63, 64, 65, 69120};
static const uint32_t BLOCK_LENS[] = {1, 10, 20, 40, 70000};

// the windows' and the ranges' block: plans, two scans, verdicts, scratch, summary, starts (the end of a windows call's
// block, not rounded); ranges: the scan of the lengths and the lengths that have room
static long check_windows(uint64_t n, uint64_t F, uint32_t block_len, bool ranges) {
  const uint32_t scratch_per = (block_len + 7u) & ~7u;
  if (windows_scratch_per(block_len) != scratch_per) fail("windows_scratch_per", n, block_len);
  const uint64_t nr = ranges ? n : 0;
  const size_t o_plan = 0, o_cov = up(o_plan + n * sizeof(X3WinPlan)), o_item = up(o_cov + (n + 1) * 8),
               o_fst = up(o_item + (n + 1) * 8), o_scr = up(o_fst + F * 4), o_sum = up(o_scr + n * scratch_per * 2),
               o_gs = up(o_sum + sizeof(X3WinSummary)), end_gs = o_gs + n * 8, o_off = up(end_gs), o_elen = up(o_off + (nr + 1) * 8),
               want_total = ranges ? o_elen + nr * 4 : end_gs;
  WinWs w, w0;
  const size_t total = windows_carve(reinterpret_cast<char*>(BASE), n, F, scratch_per, ranges, &w);
  if (windows_carve(nullptr, n, F, scratch_per, ranges, &w0) != total) fail("size without a base differs", n, F);
  const Placed pieces[] = {PLACED(w, plan, o_plan, n), PLACED(w, cov_off, o_cov, n + 1), PLACED(w, item_off, o_item, n + 1),
                           PLACED(w, fst, o_fst, F), PLACED(w, scratch, o_scr, n * scratch_per), PLACED(w, sum, o_sum, 1),
                           PLACED(w, gstart, o_gs, n), PLACED(w, off, o_off, n + 1), PLACED(w, elen, o_elen, n)};
  check_placed(pieces, ranges ? 9 : 7, total, want_total, n, F);
  if (!ranges && (w.off || w.elen)) fail("range pieces of a windows call", n, F);
  return 1;
}

// the levels' block: verdicts, plans, row counts and their scan, the partial rows, scratch, summary, the entries' row prefix
static long check_levels(uint64_t F, uint32_t block_len, uint64_t n_rows, uint64_t n_ent) {
  const uint32_t scratch_per = ((block_len < 0x10000u ? block_len : 0x10000u) + 7u) & ~7u;
  uint64_t fix_waves = (F + 3) / 4 * 4;
  if (fix_waves > 4096) fix_waves = 4096;
  if (fix_waves > (32ull << 20) / (2ull * scratch_per) / 4 * 4) fix_waves = (32ull << 20) / (2ull * scratch_per) / 4 * 4;
  if (fix_waves < 1) fix_waves = 1;
  if (levels_scratch_per(block_len) != scratch_per) fail("levels_scratch_per", F, block_len);
  if (levels_fix_waves(F, scratch_per) != fix_waves) fail("levels_fix_waves", F, block_len);
  const uint64_t cap = n_rows + F, scr = (fix_waves > 4 ? fix_waves : 4) * scratch_per;
  const size_t o_fst = 0, o_fr = up(o_fst + F * 4), o_cnt = up(o_fr + F * sizeof(X3LevFrame)), o_row = up(o_cnt + F * 4),
               o_rows = up(o_row + (F + 1) * 8), o_scr = up(o_rows + cap * sizeof(x3_level)), o_sum = up(o_scr + scr * 2),
               o_rf = up(o_sum + sizeof(X3LevSummary)), want_total = o_rf + (n_ent + 1) * 8;
  LevWs w, w0;
  const size_t total = levels_carve(reinterpret_cast<char*>(BASE), F, n_rows, fix_waves, scratch_per, n_ent, &w);
  if (levels_carve(nullptr, F, n_rows, fix_waves, scratch_per, n_ent, &w0) != total) fail("size without a base differs", F, n_rows);
  const Placed pieces[] = {PLACED(w, fst, o_fst, F), PLACED(w, frames, o_fr, F), PLACED(w, cnt, o_cnt, F),
                           PLACED(w, row, o_row, F + 1), PLACED(w, rows, o_rows, cap), PLACED(w, scratch, o_scr, scr),
                           PLACED(w, sum, o_sum, 1), PLACED(w, row_first, o_rf, n_ent + 1)};
  check_placed(pieces, 8, total, want_total, F, n_rows);
  return 1;
}

int main() {
  long tables = 0, carves = 0, windows = 0, levels = 0;
  for (uint64_t F : FRAMES)
    for (uint32_t bl : BLOCK_LENS) {
      for (uint64_t n : WIN_N)
        for (int ranges = 0; ranges < 2; ++ranges) windows += check_windows(n, F, bl, ranges != 0);
      for (uint64_t n_rows : {(uint64_t)1, F, 3 * F + 1})
        for (uint64_t n_ent : {(uint64_t)0, (uint64_t)1, (uint64_t)1000}) levels += check_levels(F, bl, n_rows, n_ent);
    }
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  for (uint64_t n : NS)
    for (uint64_t variant = 0; variant < 40; ++variant) {
      // lengths: all zero (no span at all), all of one kind, then random draws; offsets: random with overlaps, and repeats
      std::vector<uint64_t> off(n), len(n);
      uint64_t x3_len = 0;
      for (uint64_t e = 0; e < n; ++e) {
        len[e] = variant == 0 ? 0 : variant <= 7 ? LENGTHS[variant - 1] : LENGTHS[rnd(seed) % 7];
        off[e] = e && rnd(seed) % 4 == 0 ? off[e - 1] : rnd(seed) % 200000;
        if (off[e] + len[e] > x3_len) x3_len = off[e] + len[e];
      }
      std::vector<uint32_t> sf;
      uint64_t G = ~0ull, bytes = ~0ull, want_G = 0, want_bytes = 0;
      ++tables;
      if (seg_entries(off.data(), len.data(), n, x3_len, &sf, &G, &bytes) != X3_OK) { fail("refused", n, variant); continue; }
      if (sf.size() != n + 1) { fail("span_first size", n, variant); continue; }
      for (uint64_t e = 0; e < n; ++e) {
        if (sf[e] != want_G) fail("span_first", n, variant);
        want_G += (len[e] + SPAN_BYTES - 1) / SPAN_BYTES;
        want_bytes += len[e];
      }
      if (sf[n] != want_G || G != want_G || bytes != want_bytes) fail("G or bytes", n, variant);
      if (variant == 0 && G != 0) fail("G of empty entries", n, variant);
      // one byte past the end of the buffer: the last entry that reaches it, by its length and by its offset
      for (uint64_t e = 0; e < n; ++e)
        if (off[e] + len[e] == x3_len) {
          uint64_t g2, b2;
          ++len[e];
          if (seg_entries(off.data(), len.data(), n, x3_len, &sf, &g2, &b2) != X3_ERR_BAD_ARG) fail("length past x3_len", n, variant);
          --len[e];
          const uint64_t o = off[e];
          off[e] = x3_len + 1;
          if (seg_entries(off.data(), len.data(), n, x3_len, &sf, &g2, &b2) != X3_ERR_BAD_ARG) fail("offset past x3_len", n, variant);
          off[e] = o;
          break;
        }
      carves += check_carve(n, G, variant);
    }
  // the bound on G: 0x7FFFFFFF / X3I_WG_CANDS spans pass, one more is refused (nothing is dereferenced: lengths alone)
  const uint64_t g_max = 0x7FFFFFFFull / WG_CANDS;
  for (uint64_t n : {(uint64_t)1, (uint64_t)3}) {
    std::vector<uint64_t> off(n, 0), len(n, (g_max / n) * SPAN_BYTES);
    len[0] += (g_max % n) * SPAN_BYTES;
    std::vector<uint32_t> sf;
    uint64_t G = 0, bytes = 0;
    ++tables;
    if (seg_entries(off.data(), len.data(), n, len[0], &sf, &G, &bytes) != X3_OK || G != g_max) fail("G at the bound", n, 0);
    else carves += check_carve(n, G, 1000);
    len[n - 1] += 1;
    if (seg_entries(off.data(), len.data(), n, len[0] + 1, &sf, &G, &bytes) != X3_ERR_BAD_ARG) fail("G past the bound", n, 0);
  }
  if (failures) {
    std::printf("FAILED %d checks\n", failures);
    return 1;
  }
  std::printf("ok tables=%ld carves=%ld windows=%ld levels=%ld\n", tables, carves, windows, levels);
  return 0;
}
