// The segmented walk's entry table and workspace (seg_entries, segwalk_carve, streams_carve: x3_internal.h) on the CPU:
// span counts against their formula, the refusals, and the carved pieces -- disjoint, aligned for their elements, long
// enough for what the kernels of x3_streams_kernel.h index, inside the returned size, the entry table in ONE piece (it
// goes up in one copy); the batch decode's block: the same walk pieces, its own behind them.  The workspaces of the windows /
// ranges calls, the levels calls, the events calls, the range-levels calls and the quantiles / thresholds calls (windows_carve,
// levels_carve, events_carve, range_levels_carve with range_levels_pairs, quantiles_carve): every piece's offset and the
// total against the chains of rounded offsets that laid them out before there was a carver (or, for the later three, that
// their first carve gave), written out below -- the layout must not move, a same-size workspace keeps the context's
// allocations where they are.  Host code only: no context.
// Prints "ok tables=<cases> carves=<cases> windows=<cases> levels=<cases> events=<cases> range_levels=<cases>
// quantiles=<cases>", or the first cases that disagree and exits 1.
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
// (as x3_events_kernel.h, x3_range_levels_kernel.h and x3_quantiles_kernel.h have them)
struct X3EvSummary { unsigned long long count, n_runs; };
struct X3RLevPair { uint64_t f; uint32_t w, lo, hi, r0, b0, cnt; };
struct X3RLevSummary { X3WinSummary w; unsigned long long overflow; };
struct X3QSlot { uint32_t prefix, rank; };
struct X3QSummary { unsigned long long n_empty, first_empty; };

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

// the events' block: a byte per row, four words per tile of 256 rows, the run tables and the scan of their pieces, the
// summary, the entries' row prefix
static long check_events(uint64_t n_rows, uint64_t n_ent) {
  const uint64_t nt = (n_rows + X3_EVENTS_TILE_ROWS - 1) / X3_EVENTS_TILE_ROWS;
  const size_t o_hot = 0, o_tp = up(o_hot + n_rows), o_tn = up(o_tp + nt * 4), o_ns = up(o_tn + nt * 4), o_ne = up(o_ns + nt * 4),
               o_rf = up(o_ne + nt * 4), o_rl = up(o_rf + n_rows * 4), o_po = up(o_rl + n_rows * 4), o_sum = up(o_po + (n_rows + 1) * 8),
               o_rowf = up(o_sum + sizeof(X3EvSummary)), want_total = o_rowf + (n_ent + 1) * 8;
  EvWs w, w0;
  const size_t total = events_carve(reinterpret_cast<char*>(BASE), n_rows, n_ent, &w);
  if (events_carve(nullptr, n_rows, n_ent, &w0) != total) fail("size without a base differs", n_rows, n_ent);
  const Placed pieces[] = {PLACED(w, hot, o_hot, n_rows), PLACED(w, tile_prev, o_tp, nt), PLACED(w, tile_next, o_tn, nt),
                           PLACED(w, tile_ns, o_ns, nt), PLACED(w, tile_ne, o_ne, nt), PLACED(w, run_first, o_rf, n_rows),
                           PLACED(w, run_last, o_rl, n_rows), PLACED(w, piece_off, o_po, n_rows + 1), PLACED(w, sum, o_sum, 1),
                           PLACED(w, row_first, o_rowf, n_ent + 1)};
  check_placed(pieces, 10, total, want_total, n_rows, n_ent);
  return 1;
}

// the range levels' block: per range the plan, two scans, the rows that have room, the plan's starts; per frame the verdicts;
// per pair its cut and the scan of the bin counts; the partial rows; scratch; the summary (the end, not rounded).  P: the
// pairs, n * max_frames or 4 * (F + n), whichever is less; *arm: which it was
static long check_range_levels(uint64_t n, uint64_t F, uint64_t max_frames, uint64_t rows_cap, uint32_t block_len, int* arm) {
  const uint64_t P = n * max_frames < 4 * (F + n) ? n * max_frames : 4 * (F + n);
  *arm = n * max_frames < 4 * (F + n) ? 0 : 1;
  if (range_levels_pairs(n, F, max_frames) != P) fail("range_levels_pairs", n, F);
  const uint32_t scratch_per = levels_scratch_per(block_len);   // (pinned by check_levels)
  const uint64_t fix_waves = levels_fix_waves(n, scratch_per), scr = (fix_waves > 4 ? fix_waves : 4) * scratch_per;
  const size_t o_plan = 0, o_cov = up(o_plan + n * sizeof(X3WinPlan)), o_row = up(o_cov + (n + 1) * 8), o_er = up(o_row + (n + 1) * 8),
               o_gs = up(o_er + n * 4), o_fst = up(o_gs + n * 8), o_pairs = up(o_fst + F * 4), o_prow = up(o_pairs + P * sizeof(X3RLevPair)),
               o_rows = up(o_prow + (P + 1) * 8), o_scr = up(o_rows + (rows_cap + P) * sizeof(x3_level)), o_sum = up(o_scr + scr * 2),
               want_total = o_sum + sizeof(X3RLevSummary);
  RLevWs w, w0;
  const size_t total = range_levels_carve(reinterpret_cast<char*>(BASE), n, F, P, rows_cap, fix_waves, scratch_per, &w);
  if (range_levels_carve(nullptr, n, F, P, rows_cap, fix_waves, scratch_per, &w0) != total) fail("size without a base differs", n, F);
  const Placed pieces[] = {PLACED(w, plan, o_plan, n), PLACED(w, cov_off, o_cov, n + 1), PLACED(w, row_off, o_row, n + 1),
                           PLACED(w, erows, o_er, n), PLACED(w, gstart, o_gs, n), PLACED(w, fst, o_fst, F), PLACED(w, pairs, o_pairs, P),
                           PLACED(w, prow, o_prow, P + 1), PLACED(w, rows, o_rows, rows_cap + P), PLACED(w, scratch, o_scr, scr),
                           PLACED(w, sum, o_sum, 1)};
  check_placed(pieces, 11, total, want_total, n, F);
  return 1;
}

// the quantiles' block: (key, entry) per row, 256 bins and (prefix, rank) per (entry, j), the two values and K per entry,
// the summary, the entries' row prefix
static long check_quantiles(uint64_t n_rows, uint64_t n_ent, uint32_t n_q) {
  const size_t o_keys = 0, o_hist = up(o_keys + n_rows * 8), o_slots = up(o_hist + n_ent * n_q * 256 * 4),
               o_v0 = up(o_slots + n_ent * n_q * sizeof(X3QSlot)), o_v1 = up(o_v0 + n_ent * 4), o_cnt = up(o_v1 + n_ent * 4),
               o_sum = up(o_cnt + n_ent * 4), o_rowf = up(o_sum + sizeof(X3QSummary)), want_total = o_rowf + (n_ent + 1) * 8;
  QWs w, w0;
  const size_t total = quantiles_carve(reinterpret_cast<char*>(BASE), n_rows, n_ent, n_q, &w);
  if (quantiles_carve(nullptr, n_rows, n_ent, n_q, &w0) != total) fail("size without a base differs", n_rows, n_ent);
  const Placed pieces[] = {PLACED(w, keys, o_keys, n_rows), PLACED(w, hist, o_hist, n_ent * n_q * 256), PLACED(w, slots, o_slots, n_ent * n_q),
                           PLACED(w, val[0], o_v0, n_ent), PLACED(w, val[1], o_v1, n_ent), PLACED(w, counted, o_cnt, n_ent),
                           PLACED(w, sum, o_sum, 1), PLACED(w, row_first, o_rowf, n_ent + 1)};
  check_placed(pieces, 8, total, want_total, n_rows, n_ent);
  return 1;
}

// rows around the rounding of 256 bytes (a byte, 4 and 8 bytes a row) and around one, two and 256 tiles of 256 rows
static const uint64_t ROWS[] = {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 1000003};

int main() {
  long tables = 0, carves = 0, windows = 0, levels = 0, events = 0, range_levels = 0, quantiles = 0;
  for (uint64_t n_rows : ROWS)
    for (uint64_t n_ent : {(uint64_t)0, (uint64_t)1, (uint64_t)1000}) {
      events += check_events(n_rows, n_ent);
      for (uint32_t n_q : {1u, 8u}) quantiles += check_quantiles(n_rows, n_ent, n_q);
    }
  long arms[2] = {0, 0};
  for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)1000})
    for (uint64_t F : FRAMES)
      for (uint64_t max_frames : {(uint64_t)1, (F + 1) / 2, F})
        for (uint64_t rows_cap : {(uint64_t)1, n, 3 * n + 1})
          for (uint32_t bl : {10u, 70000u}) {
            int arm;
            range_levels += check_range_levels(n, F, max_frames, rows_cap, bl, &arm);
            ++arms[arm];
          }
  if (!arms[0] || !arms[1]) fail("range_levels_pairs: one arm of the min was never taken", arms[0], arms[1]);
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
  std::printf("ok tables=%ld carves=%ld windows=%ld levels=%ld events=%ld range_levels=%ld quantiles=%ld\n", tables, carves, windows,
              levels, events, range_levels, quantiles);
  return 0;
}
