// Host driver of tests/test_beam_pages_host.py: seeded random schedules over BeamPages (csrc/beam_pages.hpp), the page book of
// both beam searches, shaped like the searches' use of it - groups of `beam` rows that start (empty, or on a shared prefilled
// prompt), write one position per step, are re-indexed with repeated parents, lose rows and finish.  After EVERY operation the
// whole book is checked against the table.  Exit status 0: every check held.
#include "../taiwan_tongues_asr_ce_amd/csrc/beam_pages.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using ttasr_detail::BeamPages;

static const char* g_what = "";
static long g_step = 0;

#define CHECK(cond)                                                                                                   \
  do {                                                                                                                \
    if (!(cond)) { std::fprintf(stderr, "FAILED %s (%s, step %ld, line %d)\n", #cond, g_what, g_step, __LINE__); std::exit(1); } \
  } while (0)

// refcnt[p] = the number of table entries holding p; the free list = the pages with count 0, each once, descending
static void check_book(const BeamPages& bp) {
  std::vector<int> n(bp.n_pages, 0);
  CHECK((int)bp.tbl.size() == bp.rows * bp.pps && (int)bp.refcnt.size() == bp.n_pages);
  for (int32_t p : bp.tbl) { CHECK(p >= -1 && p < bp.n_pages); if (p >= 0) n[p]++; }
  size_t n_free = 0;
  for (int p = 0; p < bp.n_pages; ++p) { CHECK(bp.refcnt[p] == n[p]); n_free += n[p] == 0; }
  CHECK(bp.free_pages.size() == n_free);
  for (size_t i = 0; i < bp.free_pages.size(); ++i) {
    CHECK(n[bp.free_pages[i]] == 0);
    CHECK(i == 0 || bp.free_pages[i] < bp.free_pages[i - 1]);
  }
  std::vector<int32_t> up(bp.tbl.size(), -7);
  bp.write_upload(up.data());
  for (size_t i = 0; i < up.size(); ++i) CHECK(up[i] == (bp.tbl[i] < 0 ? 0 : bp.tbl[i]));
  CHECK(bp.peek_free(n_free + 1) == nullptr);
  const size_t k = n_free / 2;
  const int32_t* tail = bp.peek_free(k);
  CHECK(tail != nullptr);
  for (size_t i = 0; i < k; ++i) CHECK(tail[i] == bp.free_pages[n_free - k + i]);
}

// make_private with its contract: the write page is the row's alone afterwards; a shared page was split into exactly one pair
// (old, new) whose source is still referenced; anything else appends nothing
static bool checked_make_private(BeamPages& bp, int row, int pos) {
  g_what = "make_private";
  const size_t e = (size_t)row * bp.pps + pos / BeamPages::kPageTokens;
  const int32_t old = bp.tbl[e];
  const bool shared = old >= 0 && bp.refcnt[old] > 1, kept = old >= 0 && bp.refcnt[old] == 1;
  const std::vector<int32_t> before = bp.tbl;
  std::vector<int32_t> pairs = {-5, -6};   // earlier pairs of the step stay
  const bool ok = bp.make_private(row, pos, pairs);
  if (!ok) {
    CHECK(bp.tbl == before && pairs.size() == 2 && bp.free_pages.empty());
    check_book(bp);
    return false;
  }
  const int32_t pg = bp.tbl[e];
  CHECK(pg >= 0 && bp.refcnt[pg] == 1);
  CHECK(pairs[0] == -5 && pairs[1] == -6);
  if (shared) {
    CHECK(pairs.size() == 4 && pairs[2] == old && pairs[3] == pg && pg != old && bp.refcnt[old] >= 1);
  } else {
    CHECK(pairs.size() == 2);
    CHECK(kept ? pg == old : true);
  }
  for (size_t i = 0; i < before.size(); ++i) CHECK(i == e || bp.tbl[i] == before[i]);
  check_book(bp);
  return true;
}

// One schedule: `groups` groups of `beam` rows over a pool of rows x pps pages (what a context holds), `steps` steps.
static void run_schedule(unsigned seed, int beam, int groups, int steps) {
  std::mt19937 rng(seed);
  auto draw = [&](int n) { return (int)(rng() % (unsigned)n); };
  const int pps = 28, rows = beam * groups, last_pos = pps * BeamPages::kPageTokens - 1;
  BeamPages bp;
  g_what = "reset";
  bp.reset(rows, pps, rows * pps);
  check_book(bp);
  CHECK((int)bp.free_pages.size() == rows * pps && bp.free_pages.back() == 0);
  std::vector<int> pos(groups, -1);   // -1: the group is idle
  for (g_step = 0; g_step < steps; ++g_step) {
    // idle groups start: from position 0, or behind a prompt of `pre` positions prefilled into pages its rows share
    for (int g = 0; g < groups; ++g) {
      if (pos[g] >= 0 || draw(4) != 0) continue;
      pos[g] = 0;
      if (draw(2)) {
        g_what = "share_fresh";
        const int pre = 1 + draw(200);
        for (int q = 0; q < (pre + 15) / 16; ++q) {
          const int32_t pg = bp.share_fresh(g * beam, beam, q);
          CHECK(pg >= 0 && bp.refcnt[pg] == beam);
          for (int b = 0; b < beam; ++b) CHECK(bp.tbl[(size_t)(g * beam + b) * pps + q] == pg);
          check_book(bp);
        }
        pos[g] = pre;
      }
    }
    // every live row writes its group's position: with rows <= n_pages / pps the pool never reports empty
    for (int g = 0; g < groups; ++g)
      for (int b = 0; pos[g] >= 0 && b < beam; ++b) CHECK(checked_make_private(bp, g * beam + b, pos[g]));
    // selection: the rows of a live group continue parents drawn with repeats from the group, the others keep their lists
    if (draw(10) < 7) {
      g_what = "reindex";
      std::vector<int> src(rows);
      for (int r = 0; r < rows; ++r) src[r] = pos[r / beam] >= 0 ? (r / beam) * beam + draw(beam) : r;
      const std::vector<int32_t> before = bp.tbl;
      bp.reindex(src);
      for (int r = 0; r < rows; ++r)
        for (int q = 0; q < pps; ++q) CHECK(bp.tbl[(size_t)r * pps + q] == before[(size_t)src[r] * pps + q]);
      check_book(bp);
    }
    g_what = "drop_row";
    for (int g = 0; g < groups; ++g) {
      if (pos[g] < 0) continue;
      if (draw(50) == 0) {   // one row loses its list and goes on from fresh pages
        const int r = g * beam + draw(beam);
        bp.drop_row(r);
        for (int q = 0; q < pps; ++q) CHECK(bp.tbl[(size_t)r * pps + q] == -1);
        check_book(bp);
      }
      if (++pos[g] > last_pos || draw(40) == 0) {   // the group finishes: its pages go back, it restarts later
        for (int b = 0; b < beam; ++b) { bp.drop_row(g * beam + b); check_book(bp); }
        pos[g] = -1;
      }
    }
  }
  g_what = "recount";
  const BeamPages before = bp;
  bp.recount();
  CHECK(bp.refcnt == before.refcnt && bp.free_pages == before.free_pages && bp.tbl == before.tbl);
}

// A pool smaller than the rows need: the book must report it (false / -1), stay consistent and change nothing.
static void run_exhaustion() {
  const int beam = 5, pps = 28;
  BeamPages bp;
  bp.reset(beam, pps, 10);
  bool ran_out = false;
  for (int pos = 0; pos < pps * BeamPages::kPageTokens && !ran_out; ++pos)
    for (int b = 0; b < beam && !ran_out; ++b) ran_out = !checked_make_private(bp, b, pos);
  g_what = "exhaustion";
  CHECK(ran_out && bp.free_pages.empty());
  CHECK(!checked_make_private(bp, 0, 3 * BeamPages::kPageTokens));   // again: still false, still consistent
  CHECK(bp.share_fresh(0, beam, 20) == -1);
  check_book(bp);
  bp.drop_row(1);   // pages come back: the next request is served
  check_book(bp);
  CHECK(checked_make_private(bp, 0, 3 * BeamPages::kPageTokens));
  // a shared page cannot be split without a free page either
  bp.reset(2, pps, 1);
  CHECK(bp.share_fresh(0, 2, 0) == 0);
  CHECK(!checked_make_private(bp, 0, 5));
}

int main() {
  const int beams[4] = {1, 3, 5, 7}, n_groups[8] = {6, 1, 6, 2, 3, 5, 4, 6};   // every beam, 1 to 6 groups
  for (int i = 0; i < 8; ++i) {
    const int beam = beams[i % 4], groups = n_groups[i];
    run_schedule(1000u + i, beam, groups, 2000);
    std::printf("schedule %d: beam %d, %d groups, 2000 steps ok\n", i, beam, groups);
  }
  run_exhaustion();
  std::printf("exhaustion ok\n");
  return 0;
}
