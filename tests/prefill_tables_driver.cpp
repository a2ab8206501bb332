// Host driver of tests/test_session_prefill_host.py: the rule, the pass split and the packed-row tables of a session's admission
// passes (csrc/prefill_tables.hpp) against hand-written cases.  Exit status 0: every check held.
#include "../taiwan_tongues_asr_ce_amd/csrc/prefill_tables.hpp"

#include <cstdio>
#include <cstdlib>
#include <numeric>

using namespace ttasr_detail;

#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    if (!(cond)) { std::fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); }   \
  } while (0)

struct Built { std::vector<int32_t> rows, slots, seqs, items; PrefillCounts n; };

static Built build(const std::vector<int>& len, const std::vector<int>& slot, int pps) {
  std::vector<std::vector<int32_t>> tok(len.size()), pg(len.size());
  std::vector<PrefillSeq> sq;
  int rows = 0, items = 0;
  for (size_t s = 0; s < len.size(); ++s) {
    tok[s].resize(len[s]);
    for (int t = 0; t < len[s]; ++t) tok[s][t] = 1000 * (int)(s + 1) + t;
    pg[s].resize((len[s] + 15) / 16);
    for (size_t j = 0; j < pg[s].size(); ++j) pg[s][j] = slot[s] * pps + (int)j;
    sq.push_back(PrefillSeq{slot[s], len[s], tok[s].data(), pg[s].data()});
    rows += len[s]; items += prefill_items_of(len[s]);
  }
  Built b;
  b.rows.assign((size_t)rows * 3, -7); b.slots.assign(rows, -7); b.seqs.assign(len.size() * (3 + pps), -7); b.items.assign((size_t)items * 3, -7);
  b.n = prefill_build_tables(sq.data(), (int)sq.size(), pps, b.rows.data(), b.slots.data(), b.seqs.data(), b.items.data());
  CHECK(b.n.rows == rows && b.n.seqs == (int)len.size() && b.n.items == items);
  CHECK(prefill_table_words(rows, (int)len.size(), items, pps) == b.rows.size() + b.slots.size() + b.seqs.size() + b.items.size());
  return b;
}

int main() {
  // ---- the rule ----
  CHECK(session_prefill_positions(64, 61, 8, false) == 61);      // no-speech wanted: stops at <|startoftranscript|>
  CHECK(session_prefill_positions(64, -1, 8, false) == 63);      // not wanted: everything but the last prompt token
  CHECK(session_prefill_positions(9, -1, 8, false) == 8 && session_prefill_positions(8, -1, 8, false) == 0);   // p >= N
  CHECK(session_prefill_positions(64, 5, 8, false) == 0);        // sot too early: forced
  CHECK(session_prefill_positions(64, 61, 0, false) == 0);       // option off
  CHECK(session_prefill_positions(64, 61, 8, true) == 0);        // a placeholder clip is never prefilled
  CHECK(session_prefill_positions(2, -1, 1, false) == 1 && session_prefill_positions(1, -1, 1, false) == 0);
  // ---- lengths 1, 128, 129 and 446 in one table set (pages_per_seq 28) ----
  const int pps = 28;
  const std::vector<int> len{1, 128, 129, 446}, slot{3, 0, 7, 2};
  const Built b = build(len, slot, pps);
  CHECK(b.n.rows == 704 && b.n.items == 1 + 1 + 2 + 4);
  const int first[4] = {0, 1, 129, 258};
  for (int s = 0; s < 4; ++s) {
    const int32_t* e = &b.seqs[(size_t)s * (3 + pps)];
    CHECK(e[0] == slot[s] && e[1] == first[s] && e[2] == len[s]);
    for (int j = 0; j < pps; ++j) CHECK(e[3 + j] == (j < (len[s] + 15) / 16 ? slot[s] * pps + j : 0));
    for (int t = 0; t < len[s]; ++t) {
      const int32_t* r = &b.rows[(size_t)(first[s] + t) * 3];
      CHECK(r[0] == s && r[1] == t && r[2] == 1000 * (s + 1) + t && b.slots[first[s] + t] == slot[s]);
    }
  }
  const int want_items[8][3] = {{0, 0, 1}, {1, 1, 128}, {2, 129, 128}, {2, 257, 1}, {3, 258, 128}, {3, 386, 128}, {3, 514, 128}, {3, 642, 62}};
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 3; ++k) CHECK(b.items[3 * i + k] == want_items[i][k]);
  // a sequence's items depend on its own length only: the same sequence alone gives the same blocks, shifted to row 0
  const Built alone = build({129}, {7}, pps);
  CHECK(alone.items == (std::vector<int32_t>{0, 0, 128, 0, 128, 1}));
  // ---- the split at the workspace's rows: whole sequences, in order ----
  CHECK(prefill_pass_split({446, 446, 223}, kPrefillRowCap) == (std::vector<int>{0, 1, 2, 3}));
  CHECK(prefill_pass_split({1, 31, 32, 33, 127, 128, 129, 223}, kPrefillRowCap) == (std::vector<int>{0, 7, 8}));
  CHECK(prefill_pass_split({256, 256, 1}, kPrefillRowCap) == (std::vector<int>{0, 2, 3}));     // exactly the cap fits
  CHECK(prefill_pass_split({200, 200}, kPrefillRowCap) == (std::vector<int>{0, 2}));
  CHECK(prefill_pass_split({}, kPrefillRowCap) == (std::vector<int>{0}));
  CHECK(kPrefillRowCap == 512 && kPrefillBlock == 128 && prefill_items_of(446) == 4 && prefill_items_of(128) == 1);
  std::puts("prefill tables: ok");
  return 0;
}
