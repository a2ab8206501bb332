// Sequence-bias logits processor (HF generation/logits_process.py SequenceBiasLogitsProcessor, restated): a table maps token
// sequences to float biases; a sequence of length 1 always applies to its token, a longer one applies to its LAST token when the
// row's history holds at least as many tokens as the sequence and ends in the sequence's first L - 1 tokens.  Per vocabulary id the
// sum is 0, + the length-1 bias, + the matching longer sequences in table order, in float32, added to the raw logit once.
//
// The host groups the table by last token (seq_bias.hpp), so one thread owns one logit: it sums its group serially, in table
// order, and does one read-modify-write.  No atomics, no reduction across lanes: the result is the definition's, bit for bit.
// The kernel runs in front of the selection kernels, which apply the Whisper rules to what it leaves (a suppressed id stays -inf).
#include "common.hpp"
#include "seq_bias.hpp"

using namespace ttasr_detail;

// STATE: the device-resident search state of the greedy / sampled loops - the k-th token back is out_tokens[n_sampled - k], and
// beyond the sampled tokens prompt[prompt_len - ..]; only rows that choose a token at this step are touched (not finished, not
// forced through their prompt).  Otherwise: the window the beam search uploads, win[r][kSeqBiasW - k] = the k-th token back, with
// win_len[r] = min(history length, kSeqBiasMaxLen), or -1 for a row that does not search at this position.
template <bool STATE>
__global__ __launch_bounds__(256) void seq_bias_kernel(float* __restrict__ logits, int ldv, const int32_t* __restrict__ tab, SeqBiasHist h) {
  const int b = blockIdx.x;
  int total, n = 0, plen = 0;
  const int32_t *outp = nullptr, *pr = nullptr, *win = nullptr;
  if constexpr (STATE) {
    if (h.done[b]) return;
    const RuleDyn dyn = *h.dyn;   // the strides of the call, not of the capture (common.hpp RuleDyn)
    if (h.prompt) {
      plen = h.prompt_len[b];
      if (*h.step + 1 < plen) return;   // the select launch feeds this row its next prompt token
      pr = h.prompt + (int64_t)b * dyn.max_prompt;
    }
    n = min(h.n_sampled[b], dyn.max_new);
    outp = h.out_tokens + (int64_t)b * dyn.max_new;
    total = plen + n;
  } else {
    total = h.win_len[b];
    if (total < 0) return;
    win = h.win + (int64_t)b * kSeqBiasW;
  }
  auto back = [&](int k) -> int {   // the k-th history token from the end, 1 <= k <= min(total, kSeqBiasW)
    if constexpr (STATE) return k <= n ? outp[n - k] : pr[plen - (k - n)];
    else return win[kSeqBiasW - k];
  };
  const int n_groups = min(tab[0], kSeqBiasMaxGroups);
  const SeqBiasGroup* groups = (const SeqBiasGroup*)(tab + kSeqBiasGroupsAt);
  const SeqBiasEntry* entries = (const SeqBiasEntry*)(tab + kSeqBiasEntriesAt);
  const int32_t* prefix = tab + kSeqBiasPrefixAt;
  float* row = logits + (int64_t)b * ldv;
  for (int g = threadIdx.x; g < n_groups; g += 256) {
    const SeqBiasGroup G = groups[g];
    float sum = 0.f;
    bool applies = G.len1 == G.len1;   // NaN: no length-1 sequence for this token
    if (applies) sum += G.len1;
    for (int e = G.first; e < G.first + G.n; ++e) {
      const SeqBiasEntry E = entries[e];
      if (total < E.prefix_len + 1) continue;   // the reference skips a sequence longer than the history
      const int32_t* p = prefix + E.prefix_off;
      bool match = true;
      for (int k = 1; k <= E.prefix_len && match; ++k) match = back(k) == p[E.prefix_len - k];
      if (match) { sum += E.bias; applies = true; }
    }
    if (applies) row[G.token] = row[G.token] + sum;
  }
}

void launch_seq_bias(float* logits, int ldv, const int32_t* tab, const SeqBiasHist& h, bool state_form, int rows, hipStream_t s) {
  if (rows < 1) return;
  if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "seq_bias_kernel<%s> grid %d", state_form ? "true" : "false", rows * 256);
  if (state_form) hipLaunchKernelGGL(seq_bias_kernel<true>, dim3(rows), dim3(256), 0, s, logits, ldv, tab, h);
  else hipLaunchKernelGGL(seq_bias_kernel<false>, dim3(rows), dim3(256), 0, s, logits, ldv, tab, h);
}
