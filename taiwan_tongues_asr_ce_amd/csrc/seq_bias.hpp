// libttasr: the sequence-bias table (ttasr_set_sequence_bias, kernels_bias.hip).  Plain C++, no HIP: the
// caps, the device layout and the host-side builder that groups the caller's sequences by their last token.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace ttasr_detail {

constexpr int kSeqBiasMaxLen = 16;                    // tokens of one sequence
constexpr int kSeqBiasW = kSeqBiasMaxLen - 1;         // history tokens a match can look at
constexpr int kSeqBiasMaxGroups = 4096;               // distinct last tokens
constexpr int kSeqBiasMaxEntries = 8192;              // sequences longer than one token

// a group's len1 when the table has no length-1 sequence for its token: biases are finite, so NaN is free to mean "none"
struct SeqBiasGroup { int32_t token; float len1; int32_t first, n; };
struct SeqBiasEntry { float bias; int32_t prefix_len, prefix_off; };

// The device block, in 32-bit words: header {n_groups, n_entries, 0, 0} | groups | entries | prefix tokens | the beam search's row
// windows [max_batch][kSeqBiasW] and history lengths [max_batch].  Fixed capacity: no install moves a pointer a graph holds.
constexpr size_t kSeqBiasGroupsAt = 4;
constexpr size_t kSeqBiasEntriesAt = kSeqBiasGroupsAt + (size_t)kSeqBiasMaxGroups * 4;
constexpr size_t kSeqBiasPrefixAt = kSeqBiasEntriesAt + (size_t)kSeqBiasMaxEntries * 3;
constexpr size_t kSeqBiasWinAt = kSeqBiasPrefixAt + (size_t)kSeqBiasMaxEntries * kSeqBiasW;
inline size_t seq_bias_block_words(int max_batch) { return kSeqBiasWinAt + (size_t)max_batch * (kSeqBiasW + 1); }

struct SeqBiasHostTable {
  std::vector<SeqBiasGroup> groups;
  std::vector<SeqBiasEntry> entries;
  std::vector<int32_t> prefix;
};

// n_seq sequences, sequence i = tokens[offsets[i] .. offsets[i + 1]) with bias[i], in table order -> the grouped layout.  Groups
// stand in the order their tokens first appear, entries keep table order inside a group.  Empty string, or what is refused.
inline std::string seq_bias_build(int n_seq, const int32_t* tokens, const int32_t* offsets, const float* bias, int vocab,
                                  SeqBiasHostTable& out) {
  char msg[160];
  auto refuse = [&](const char* fmt, int a, int b, int c) { snprintf(msg, sizeof msg, fmt, a, b, c); return std::string(msg); };
  out = SeqBiasHostTable{};
  std::map<int32_t, int> group_of;
  std::map<std::vector<int32_t>, int> seen;
  std::vector<std::vector<int>> members;   // per group: the sequences longer than one token, in table order
  for (int i = 0; i < n_seq; ++i) {
    const int L = offsets[i + 1] - offsets[i];
    if (offsets[i] < 0 || L < 1 || L > kSeqBiasMaxLen) return refuse("sequence %d: length %d outside [1, %d]", i, L, kSeqBiasMaxLen);
    if (!std::isfinite(bias[i])) return refuse("sequence %d: bias is not finite", i, 0, 0);
    const int32_t* t = tokens + offsets[i];
    for (int j = 0; j < L; ++j)
      if (t[j] < 0 || t[j] >= vocab) return refuse("sequence %d: token %d outside the %d-id vocabulary", i, t[j], vocab);
    if (!seen.emplace(std::vector<int32_t>(t, t + L), i).second) return refuse("sequence %d repeats an earlier sequence", i, 0, 0);
    auto it = group_of.find(t[L - 1]);
    if (it == group_of.end()) {
      if ((int)out.groups.size() >= kSeqBiasMaxGroups) return refuse("more than %d distinct last tokens", kSeqBiasMaxGroups, 0, 0);
      it = group_of.emplace(t[L - 1], (int)out.groups.size()).first;
      out.groups.push_back(SeqBiasGroup{t[L - 1], NAN, 0, 0});
      members.emplace_back();
    }
    if (L == 1) out.groups[it->second].len1 = bias[i];
    else members[it->second].push_back(i);
  }
  for (size_t g = 0; g < out.groups.size(); ++g) {
    out.groups[g].first = (int32_t)out.entries.size();
    out.groups[g].n = (int32_t)members[g].size();
    for (int i : members[g]) {
      const int L = offsets[i + 1] - offsets[i];
      out.entries.push_back(SeqBiasEntry{bias[i], L - 1, (int32_t)out.prefix.size()});
      out.prefix.insert(out.prefix.end(), tokens + offsets[i], tokens + offsets[i] + L - 1);
    }
  }
  if ((int)out.entries.size() > kSeqBiasMaxEntries) return refuse("%d sequences longer than one token, at most %d", (int)out.entries.size(), kSeqBiasMaxEntries, 0);
  return std::string();
}

}  // namespace ttasr_detail
