// The paged-row book of both beam searches (beam_search_impl and the beam session): which KV pages every row's positions live
// in, how many rows reference each page, and which pages are free.  Host code only (no HIP include: tests/beam_pages_driver.cpp
// compiles it alone).  Hypotheses that share a prefix share its pages; a row gets a private copy of a shared page before it
// writes into it (copy-on-write, the (old, new) pairs go to launch_copy_pages).  Every operation leaves the counts and the free
// list consistent with the table: refcnt[p] = the number of table entries holding p, free_pages = the pages with count 0 in
// descending order, so that pages are taken lowest id first.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace ttasr_detail {

struct BeamPages {
  static constexpr int kPageTokens = 16;   // positions per KV page
  int rows = 0, pps = 0, n_pages = 0;
  std::vector<int32_t> tbl;         // [rows][pps] page of positions 16 j .. 16 j + 15 of the row, or -1
  std::vector<int32_t> refcnt;      // [n_pages]
  std::vector<int32_t> free_pages;  // descending; taken from the back

  void reset(int rows_, int pages_per_seq, int n_pages_) {
    rows = rows_; pps = pages_per_seq; n_pages = n_pages_;
    tbl.assign((size_t)rows * pps, -1);
    recount();
  }

  // The page that position `pos` of `row` writes must exist and be private to the row.  A page boundary always finds the entry
  // empty (entries past a row's position are never set); a page shared after a re-index is split, and (old, new) is appended to
  // `pairs`.  false: the pool is empty (nothing has changed then).
  bool make_private(int row, int pos, std::vector<int32_t>& pairs) {
    int32_t& pg = tbl[(size_t)row * pps + pos / kPageTokens];
    if (pg >= 0 && refcnt[pg] == 1) return true;
    if (free_pages.empty()) return false;
    const int32_t np = free_pages.back(); free_pages.pop_back();
    refcnt[np] = 1;
    if (pg >= 0) { pairs.push_back(pg); pairs.push_back(np); refcnt[pg]--; }
    pg = np;
    return true;
  }

  // Entry j of rows row0 .. row0 + n - 1 (all empty) becomes ONE fresh page: the rows of a clip share their prefilled prompt.
  // Returns the page, or -1 when the pool is empty.
  int32_t share_fresh(int row0, int n, int j) {
    if (free_pages.empty()) return -1;
    const int32_t pg = free_pages.back(); free_pages.pop_back();
    for (int r = row0; r < row0 + n; ++r) tbl[(size_t)r * pps + j] = pg;
    refcnt[pg] = n;
    return pg;
  }

  // After candidate selection: row r continues the hypothesis of row src[r] and inherits its page list (src: [rows], parents may repeat).
  void reindex(const std::vector<int>& src) {
    std::vector<int32_t> ntbl(tbl.size());
    for (int r = 0; r < rows; ++r) std::copy_n(&tbl[(size_t)src[r] * pps], pps, &ntbl[(size_t)r * pps]);
    tbl.swap(ntbl);
    recount();
  }

  // A finished row gives its pages back.
  void drop_row(int row) {
    for (int j = 0; j < pps; ++j) {
      int32_t& pg = tbl[(size_t)row * pps + j];
      if (pg >= 0 && --refcnt[pg] == 0)
        free_pages.insert(std::upper_bound(free_pages.begin(), free_pages.end(), pg, std::greater<int32_t>()), pg);
      pg = -1;
    }
  }

  // Reference counts and free list from the table (every entry counts).
  void recount() {
    refcnt.assign(n_pages, 0);
    for (int32_t p : tbl) if (p >= 0) refcnt[p]++;
    free_pages.clear();
    for (int p = n_pages - 1; p >= 0; --p) if (refcnt[p] == 0) free_pages.push_back(p);
  }

  // The table as the device reads it: unused entries clamped to a valid page id.
  void write_upload(int32_t* dst) const {
    for (size_t i = 0; i < tbl.size(); ++i) dst[i] = tbl[i] < 0 ? 0 : tbl[i];
  }

  // The n pages that would be taken next, without taking them (the session's alignment pass borrows them between two steps);
  // nullptr when fewer than n are free.
  const int32_t* peek_free(size_t n) const { return n <= free_pages.size() ? free_pages.data() + (free_pages.size() - n) : nullptr; }
};

}  // namespace ttasr_detail
