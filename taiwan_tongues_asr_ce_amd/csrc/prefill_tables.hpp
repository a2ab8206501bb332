// Prompt prefill at a session's admission (option "session_prefill"): the per-clip rule and the tables
// that drive the packed rows of an admission pass.  Host code only (no HIP include: tests/prefill_tables_driver.cpp compiles it
// alone).
//
// Rows of a pass are PACKED: sequence after sequence, no padding to the longest.  Three tables describe them:
//   rows   [n_rows][3]                {sequence, position, token} of every packed row
//   seqs   [n_seqs][3 + pages_per_seq] {cross-KV slot, first packed row, length, page of positions 16 j .. 16 j + 15} per sequence
//   items  [n_items][3]               {sequence, first packed query row, rows} per attention work item: a sequence is cut into
//                                     blocks of kPrefillBlock rows - a function of its own length only, never of the pass
// plus slots [n_rows], the cross-KV slot of every packed row (what the per-row cross-attention of the f32 engine reads).
// All indices are local to the pass.  An admission that holds more than kPrefillRowCap rows is cut into several passes by whole
// sequences (prefill_pass_split); a sequence never exceeds the cap (n_text_ctx - 2 <= 446 positions).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ttasr_detail {

constexpr int kPrefillRowCap = 512;   // rows of the context's prefill workspace
constexpr int kPrefillBlock = 128;    // query rows of one cross-attention work item (four waves x 32 MFMA columns)
constexpr int kPrefillPageTokens = 16;

// The rule, per clip and from the clip's own prompt only: how many leading prompt positions an admission pass computes (the row
// or group then starts stepping at that position with prompt[p]); 0 = the clip is forced token by token.  sot_index < 0: the
// no-speech probability is not wanted; otherwise the <|startoftranscript|> position stays a real step.  A clip that carries the
// language placeholder is never prefilled (its detect step rewrites position 0 of its pages).
inline int session_prefill_positions(int prompt_len, int sot_index, int threshold, bool placeholder) {
  if (threshold <= 0 || placeholder) return 0;
  int p = prompt_len - 1;
  if (sot_index >= 0) p = std::min(p, sot_index);
  return p >= threshold ? p : 0;
}

// Sequences [cut[k], cut[k + 1]) form pass k: whole sequences in order, as many as fit `cap` rows.
inline std::vector<int> prefill_pass_split(const std::vector<int>& len, int cap) {
  std::vector<int> cut{0};
  int rows = 0;
  for (int i = 0; i < (int)len.size(); ++i) {
    if (rows > 0 && rows + len[i] > cap) { cut.push_back(i); rows = 0; }
    rows += len[i];
  }
  if (!len.empty()) cut.push_back((int)len.size());
  return cut;
}

struct PrefillSeq {        // one sequence of an admission: positions 0 .. len - 1 of a clip's prompt
  int32_t slot;            // cross-KV slot (greedy: the row, beam: the group)
  int32_t len;
  const int32_t* tokens;   // [len]
  const int32_t* pages;    // [(len + 15) / 16]
};
struct PrefillCounts { int rows, seqs, items; };

inline int prefill_items_of(int len) { return (len + kPrefillBlock - 1) / kPrefillBlock; }
// words of the four tables of a pass over these sequences, in the order rows | slots | seqs | items
inline size_t prefill_table_words(int rows, int seqs, int items, int pps) {
  return (size_t)rows * 4 + (size_t)seqs * (3 + pps) + (size_t)items * 3;
}

// Fills the four tables of ONE pass (sq[0 .. n)); the arrays hold at least the counts returned.
inline PrefillCounts prefill_build_tables(const PrefillSeq* sq, int n, int pps, int32_t* rows, int32_t* slots, int32_t* seqs,
                                          int32_t* items) {
  PrefillCounts c{0, n, 0};
  for (int s = 0; s < n; ++s) {
    int32_t* e = seqs + (size_t)s * (3 + pps);
    e[0] = sq[s].slot; e[1] = c.rows; e[2] = sq[s].len;
    const int npg = (sq[s].len + kPrefillPageTokens - 1) / kPrefillPageTokens;
    for (int j = 0; j < pps; ++j) e[3 + j] = j < npg ? sq[s].pages[j] : 0;
    for (int q0 = 0; q0 < sq[s].len; q0 += kPrefillBlock) {
      int32_t* it = items + (size_t)c.items++ * 3;
      it[0] = s; it[1] = c.rows + q0; it[2] = std::min(kPrefillBlock, sq[s].len - q0);
    }
    for (int t = 0; t < sq[s].len; ++t) {
      int32_t* r = rows + (size_t)c.rows * 3;
      r[0] = s; r[1] = t; r[2] = sq[s].tokens[t];
      slots[c.rows++] = sq[s].slot;
    }
  }
  return c;
}

}  // namespace ttasr_detail
