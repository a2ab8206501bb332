// libttasr: batched word alignment (one of the engine translation units, see engine_ctx.hpp): the teacher-forced pass over n
// sequences, the post-processing and DTW kernels of kernels_align.hip behind it, and ttasr_align_batch.  The session's
// ttasr_session_align (engine_refill.hip) runs the same align_batch_run on its held clips.
#include "engine_ctx.hpp"

namespace ttasr_detail {

// Everything that can be refused is refused here, before anything is enqueued (the slots are the caller's to check).
int align_batch_validate(ttasr_ctx* c, const AlignBatch& a) {
  if (a.n < 1 || a.n > c->maxB) return fail(c, TTASR_E_INVALID, "n %d outside [1, max_batch = %d]", a.n, c->maxB);
  if (!a.tokens || !a.n_tokens || !a.first_row || !a.num_frames || !a.pairs || !a.out_start)
    return fail(c, TTASR_E_INVALID, "NULL argument");
  if (a.medfilt < 1 || a.medfilt > kAlignMaxMedfilt || !(a.medfilt & 1))
    return fail(c, TTASR_E_INVALID, "medfilt_width %d must be odd and in [1, %d]", a.medfilt, kAlignMaxMedfilt);
  const int tok_max = std::min(c->cfg.n_text_ctx, c->cfg.n_audio_ctx);
  if (a.max_tokens < 2 || a.max_tokens > tok_max) return fail(c, TTASR_E_INVALID, "max_tokens %d outside [2, %d]", a.max_tokens, tok_max);
  if ((int64_t)a.n * a.max_tokens > (int64_t)c->maxB * c->cfg.n_audio_ctx)
    return fail(c, TTASR_E_INVALID, "%d x %d rows exceed the prefill workspaces (%lld rows)", a.n, a.max_tokens,
                (long long)c->maxB * c->cfg.n_audio_ctx);
  if (c->T > 6 * 256) return fail(c, TTASR_E_INVALID, "audio window %d > 1536 frames", c->T);
  for (int i = 0; i < a.n; ++i) {
    const int nt = a.n_tokens[i];
    if (nt < 2 || nt > a.max_tokens) return fail(c, TTASR_E_INVALID, "sequence %d: n_tokens %d outside [2, max_tokens = %d]", i, nt, a.max_tokens);
    if (a.first_row[i] < 0 || a.first_row[i] > nt - 2) return fail(c, TTASR_E_INVALID, "sequence %d: first_row %d outside [0, %d]", i, a.first_row[i], nt - 2);
    if (a.num_frames[i] < 0) return fail(c, TTASR_E_INVALID, "sequence %d: num_frames %d < 0", i, a.num_frames[i]);
    for (int t = 0; t < nt; ++t) {
      const int tok = a.tokens[(size_t)i * a.max_tokens + t];
      if (tok < 0 || tok >= c->V) return fail(c, TTASR_E_INVALID, "sequence %d: token outside vocabulary", i);
    }
  }
  if (a.n_pairs < 1 || a.n_pairs > c->cfg.dec_layers * c->H) return fail(c, TTASR_E_INVALID, "n_pairs %d", a.n_pairs);
  std::vector<char> seen((size_t)c->cfg.dec_layers * c->H, 0);
  for (int i = 0; i < a.n_pairs; ++i) {
    const int l = a.pairs[2 * i], h = a.pairs[2 * i + 1];
    if (l < 0 || l >= c->cfg.dec_layers || h < 0 || h >= c->H) return fail(c, TTASR_E_INVALID, "alignment head (%d, %d)", l, h);
    if (seen[(size_t)l * c->H + h]) return fail(c, TTASR_E_INVALID, "alignment head (%d, %d) listed twice", l, h);
    seen[(size_t)l * c->H + h] = 1;
  }
  return 0;
}

// validated arguments -> pass, post-processing, DTW, results on the host.  slot [n]: cross-KV slot of every sequence; pages
// [n][pages_per_seq]: the self-attention pages the sequence's K/V may use.
int align_batch_run(ttasr_ctx* c, const AlignBatch& a, const int32_t* slot, const int32_t* pages) {
  const int n = a.n, npos = a.max_tokens, T_ = c->T, pps = c->pages_per_seq, LH = c->cfg.dec_layers * c->H, R = n * npos;
  hipStream_t s = c->stream;
  // host image of the inputs: tokens [n][npos] | AlignSeq [n] | slots [n] | pages [n][pps] | sel [LH]
  const size_t in_words = (size_t)R + 4 * (size_t)n + n + (size_t)n * pps + LH;
  std::vector<int32_t> in(in_words, 0);
  int32_t* h_tok = in.data();
  AlignSeq* h_seq = (AlignSeq*)(h_tok + R);
  int32_t* h_slot = (int32_t*)(h_seq + n);
  int32_t* h_pages = h_slot + n;
  int32_t* h_sel = h_pages + (size_t)n * pps;
  int max_rows = 0;
  size_t lds_words = 0, spill_words = 0;
  for (int i = 0; i < n; ++i) {
    memcpy(h_tok + (size_t)i * npos, a.tokens + (size_t)i * npos, (size_t)a.n_tokens[i] * 4);   // padding positions feed token 0
    AlignSeq& q = h_seq[i];
    q.first_row = a.first_row[i]; q.n_tokens = a.n_tokens[i]; q.rows = q.n_tokens - 1 - q.first_row;
    q.frames = std::min(T_, std::max(1, a.num_frames[i] / 2));
    max_rows = std::max(max_rows, q.rows);
    const size_t w = dtw_trace_words(q.rows, q.frames);
    if (w * 4 <= kDtwLdsTraceBytes) lds_words = std::max(lds_words, w); else spill_words = std::max(spill_words, w);
    h_slot[i] = slot[i];
  }
  memcpy(h_pages, pages, (size_t)n * pps * 4);
  for (int i = 0; i < LH; ++i) h_sel[i] = -1;
  for (int i = 0; i < a.n_pairs; ++i) h_sel[(size_t)a.pairs[2 * i] * c->H + a.pairs[2 * i + 1]] = i;
  // device block: inputs | lp [R] | start [R] | stats [n][pairs][2][T] | cost [R][T] | probs [pairs][R][T] | spilled traces
  Carve cv;
  cv.take(in_words * 4);
  const size_t o_lp = cv.take((size_t)R * 4), o_start = cv.take((size_t)R * 4), o_stats = cv.take((size_t)n * a.n_pairs * 2 * T_ * 4),
               o_cost = cv.take((size_t)R * T_ * 4), o_probs = cv.take((size_t)a.n_pairs * R * T_ * 4),
               o_spill = cv.take((size_t)n * spill_words * 4);
  TRY(c->align_dev.ensure(c, cv.used, "alignment scratch"));   // the context's block, grown to the largest request
  char* base = c->align_dev;
  const int32_t* d_tok = (const int32_t*)base;
  const AlignSeq* d_seq = (const AlignSeq*)(d_tok + R);
  const int32_t* d_slot = (const int32_t*)(d_seq + n);
  const int32_t* d_pages = d_slot + n;
  const int32_t* d_sel = d_pages + (size_t)n * pps;
  float* d_lp = (float*)(base + o_lp);
  int32_t* d_start = (int32_t*)(base + o_start);
  float *d_stats = (float*)(base + o_stats), *d_cost = (float*)(base + o_cost), *d_probs = (float*)(base + o_probs);
  HIPCHK(c, hipMemcpyAsync(base, in.data(), in_words * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(base + o_lp, 0, o_stats - o_lp, s));
  if (a.out_cost) HIPCHK(c, hipMemsetAsync(d_cost, 0, (size_t)R * T_ * 4, s));
  // (a) the teacher-forced pass; the residual rows stay in c->x
  AlignOut al{0, d_sel, d_probs, d_slot, d_tok, d_pages};
  sched_prefill(c, n, npos, 1, npos, &al);
  if (a.out_lp) {
    // raw log p(tokens[t + 1] | tokens[0..t]) of every real row: final LayerNorm + vocabulary projection, max_batch rows at a time
    for (int i = 0; i < n; ++i)
      for (int r0 = 0; r0 < a.n_tokens[i] - 1; r0 += c->maxB) {
        const int m = std::min(c->maxB, a.n_tokens[i] - 1 - r0);
        const size_t row = (size_t)i * npos + r0;
        c->cur = s;
        TT_DISPATCH(c, {
          launch_layernorm<T>(c->x + row * c->d, c->dlnf_g, c->dlnf_b, (T*)c->dh, m, c->d, s);
          GemmArgs g = lin_args<T>(c->dh, c->emb, m, c->V, c->d); g.epi.out_f32 = c->logits; g.epi.ldc = c->ldv;
          sched_dec_gemm(c, g, c->emb_sh);
        });
        launch_token_logprob(c->logits, c->ldv, c->V, d_tok + row + 1, d_lp + row, m, s);
      }
  }
  // (b) cost matrices, (c) DTW
  launch_align_stats(d_probs, d_seq, n, npos, a.n_pairs, T_, d_stats, s);
  launch_align_cost(d_probs, d_stats, d_seq, n, npos, max_rows, a.n_pairs, T_, a.medfilt, d_cost, s);
  launch_align_dtw(d_cost, d_seq, n, npos, max_rows, T_, lds_words, (uint32_t*)(base + o_spill), spill_words, d_start, s, c->device);
  HIPCHK(c, hipMemcpyAsync(a.out_start, d_start, (size_t)R * 4, hipMemcpyDeviceToHost, s));
  if (a.out_lp) HIPCHK(c, hipMemcpyAsync(a.out_lp, d_lp, (size_t)R * 4, hipMemcpyDeviceToHost, s));
  if (a.out_cost) HIPCHK(c, hipMemcpyAsync(a.out_cost, d_cost, (size_t)R * T_ * 4, hipMemcpyDeviceToHost, s));
  if (a.out_weights)   // [n][pairs][npos][T] on the host, [pairs][n][npos][T] on the device
    for (int i = 0; i < n; ++i)
      HIPCHK(c, hipMemcpy2DAsync(a.out_weights + (size_t)i * a.n_pairs * npos * T_, (size_t)npos * T_ * 4, d_probs + (size_t)i * npos * T_,
                                 (size_t)R * T_ * 4, (size_t)npos * T_ * 4, a.n_pairs, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // `in` is a stack temporary; the results are on the host
  HIPCHK(c, hipGetLastError());
  return TTASR_OK;
}

// The same call through the PACKED pass (option align_packed): the sequences' real positions are the
// packed rows of admission passes (prefill_tables.hpp; more than kPrefillRowCap rows: several passes by whole sequences), every
// pass runs sched_admit_prefill with the alignment extras out of the context's pf_* workspace and is finished - log-probs, cost
// matrices, DTW, results on the host - before the next one starts, so the scratch block holds one pass.  Every kernel of a pass
// works on a row or on a sequence of its own and takes its form from context constants: a sequence's outputs are the same bits
// whatever else the call or the pass holds.  Outputs keep the [n][max_tokens] layout; positions past a sequence's end are 0.
int align_packed_run(ttasr_ctx* c, const AlignBatch& a, const int32_t* slot, const int32_t* pages) {
  const int n = a.n, npos = a.max_tokens, T_ = c->T, pps = c->pages_per_seq, LH = c->cfg.dec_layers * c->H, np = a.n_pairs;
  hipStream_t s = c->stream;
  TRY(prefill_workspace(c));
  std::vector<PrefillSeq> sq(n);
  std::vector<int> len(n);
  for (int i = 0; i < n; ++i) {
    sq[i] = PrefillSeq{slot[i], a.n_tokens[i], a.tokens + (size_t)i * npos, pages + (size_t)i * pps};
    len[i] = a.n_tokens[i];
  }
  const std::vector<int> cut = prefill_pass_split(len, kPrefillRowCap);
  // one pass: host image rows [R][3] | slots [R] | seqs [ns][3 + pps] | items [ni][3] | target [R] | AlignSeq [ns] | seq_row [ns] |
  // sel [LH]; device block: image | lp [R] | start [R] | stats [ns][pairs][2][T] | cost [R][T] | maps [pairs][R][T] | stat [pairs][R][2]
  // | spilled traces
  struct Lay { int R, ns, ni, max_rows; size_t w_slots, w_seqs, w_items, w_target, w_aseq, w_row, w_sel, in_words, lds_words, spill_words,
               o_lp, o_start, o_stats, o_cost, o_maps, o_stat, o_spill, total; };
  auto layout = [&](int k) {
    Lay L{};
    L.ns = cut[k + 1] - cut[k];
    for (int i = cut[k]; i < cut[k + 1]; ++i) {
      L.R += len[i]; L.ni += prefill_items_of(len[i]);
      const int rows = a.n_tokens[i] - 1 - a.first_row[i], frames = std::min(T_, std::max(1, a.num_frames[i] / 2));
      L.max_rows = std::max(L.max_rows, rows);
      const size_t w = dtw_trace_words(rows, frames);
      if (w * 4 <= kDtwLdsTraceBytes) L.lds_words = std::max(L.lds_words, w); else L.spill_words = std::max(L.spill_words, w);
    }
    L.w_slots = (size_t)L.R * 3; L.w_seqs = L.w_slots + L.R; L.w_items = L.w_seqs + (size_t)L.ns * (3 + pps);
    L.w_target = L.w_items + (size_t)L.ni * 3; L.w_aseq = L.w_target + L.R; L.w_row = L.w_aseq + (size_t)L.ns * 4;
    L.w_sel = L.w_row + L.ns; L.in_words = L.w_sel + LH;
    Carve cv;
    cv.take(L.in_words * 4);
    L.o_lp = cv.take((size_t)L.R * 4); L.o_start = cv.take((size_t)L.R * 4); L.o_stats = cv.take((size_t)L.ns * np * 2 * T_ * 4);
    L.o_cost = cv.take((size_t)L.R * T_ * 4); L.o_maps = cv.take((size_t)np * L.R * T_ * 4);
    L.o_stat = cv.take((size_t)np * L.R * 2 * 4); L.o_spill = cv.take((size_t)L.ns * L.spill_words * 4);
    L.total = cv.used;
    return L;
  };
  size_t total = 0;
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const Lay L = layout((int)k);
    if (L.R > kPrefillRowCap) return fail(c, TTASR_E_INVALID, "packed alignment: a pass of %d rows exceeds the workspace", L.R);
    total = std::max(total, L.total);
  }
  TRY(c->align_dev.ensure(c, total, "alignment scratch"));
  char* base = c->align_dev;
  memset(a.out_start, 0, (size_t)n * npos * 4);
  if (a.out_lp) memset(a.out_lp, 0, (size_t)n * npos * 4);
  if (a.out_cost) memset(a.out_cost, 0, (size_t)n * npos * T_ * 4);
  if (a.out_weights) memset(a.out_weights, 0, (size_t)n * np * npos * T_ * 4);
  std::vector<int32_t> in, h_start;
  std::vector<float> h_lp, h_cost, h_maps;
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    const Lay L = layout((int)k);
    const int R = L.R, ns = L.ns, i0 = cut[k];
    in.assign(L.in_words, 0);
    prefill_build_tables(&sq[i0], ns, pps, in.data(), in.data() + L.w_slots, in.data() + L.w_seqs, in.data() + L.w_items);
    int32_t* h_target = in.data() + L.w_target;
    AlignSeq* h_seq = (AlignSeq*)(in.data() + L.w_aseq);
    int32_t* h_row = in.data() + L.w_row;
    int32_t* h_sel = in.data() + L.w_sel;
    for (int j = 0; j < ns; ++j) {
      const int i = i0 + j, row0 = in[L.w_seqs + (size_t)j * (3 + pps) + 1];
      h_row[j] = row0;
      for (int t = 0; t + 1 < a.n_tokens[i]; ++t) h_target[row0 + t] = a.tokens[(size_t)i * npos + t + 1];   // the last row predicts nothing
      AlignSeq& q = h_seq[j];
      q.first_row = a.first_row[i]; q.n_tokens = a.n_tokens[i]; q.rows = q.n_tokens - 1 - q.first_row;
      q.frames = std::min(T_, std::max(1, a.num_frames[i] / 2));
    }
    for (int i = 0; i < LH; ++i) h_sel[i] = -1;
    for (int i = 0; i < np; ++i) h_sel[(size_t)a.pairs[2 * i] * c->H + a.pairs[2 * i + 1]] = i;
    const int32_t* dw = (const int32_t*)base;
    const PrefillPass P{dw, dw + L.w_slots, dw + L.w_seqs, dw + L.w_items, R, ns, L.ni, 3 + pps};
    float* d_lp = (float*)(base + L.o_lp);
    int32_t* d_start = (int32_t*)(base + L.o_start);
    float *d_stats = (float*)(base + L.o_stats), *d_cost = (float*)(base + L.o_cost), *d_maps = (float*)(base + L.o_maps);
    const AlignSeq* d_seq = (const AlignSeq*)(dw + L.w_aseq);
    const int32_t* d_row = dw + L.w_row;
    HIPCHK(c, hipMemcpyAsync(base, in.data(), L.in_words * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(base + L.o_lp, 0, L.o_stats - L.o_lp, s));
    if (a.out_cost) HIPCHK(c, hipMemsetAsync(d_cost, 0, (size_t)R * T_ * 4, s));
    const PackedAlign al{dw + L.w_sel, h_sel, d_maps, (float*)(base + L.o_stat), np};
    sched_admit_prefill(c, P, &al);
    if (a.out_lp) sched_packed_logprob(c, R, dw + L.w_target, d_lp);
    launch_align_stats(d_maps, d_seq, ns, npos, np, T_, d_stats, s, d_row, R);
    launch_align_cost(d_maps, d_stats, d_seq, ns, npos, L.max_rows, np, T_, a.medfilt, d_cost, s, d_row, R);
    launch_align_dtw(d_cost, d_seq, ns, npos, L.max_rows, T_, L.lds_words, (uint32_t*)(base + L.o_spill), L.spill_words, d_start, s, c->device,
                     d_row);
    h_start.resize(R);
    HIPCHK(c, hipMemcpyAsync(h_start.data(), d_start, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    if (a.out_lp) { h_lp.resize(R); HIPCHK(c, hipMemcpyAsync(h_lp.data(), d_lp, (size_t)R * 4, hipMemcpyDeviceToHost, s)); }
    if (a.out_cost) { h_cost.resize((size_t)R * T_); HIPCHK(c, hipMemcpyAsync(h_cost.data(), d_cost, (size_t)R * T_ * 4, hipMemcpyDeviceToHost, s)); }
    if (a.out_weights) { h_maps.resize((size_t)np * R * T_); HIPCHK(c, hipMemcpyAsync(h_maps.data(), d_maps, (size_t)np * R * T_ * 4, hipMemcpyDeviceToHost, s)); }
    HIPCHK(c, hipStreamSynchronize(s));   // the pass is on the host; the block and the workspace are free for the next one
    HIPCHK(c, hipGetLastError());
    for (int j = 0; j < ns; ++j) {
      const int i = i0 + j, row0 = h_row[j], nt = a.n_tokens[i], rows = nt - 1 - a.first_row[i];
      memcpy(a.out_start + (size_t)i * npos, h_start.data() + row0, (size_t)rows * 4);
      if (a.out_lp) memcpy(a.out_lp + (size_t)i * npos, h_lp.data() + row0, (size_t)(nt - 1) * 4);
      if (a.out_cost) memcpy(a.out_cost + (size_t)i * npos * T_, h_cost.data() + (size_t)row0 * T_, (size_t)rows * T_ * 4);
      if (a.out_weights)
        for (int p = 0; p < np; ++p)
          memcpy(a.out_weights + ((size_t)i * np + p) * npos * T_, h_maps.data() + ((size_t)p * R + row0) * T_, (size_t)nt * T_ * 4);
    }
  }
  return TTASR_OK;
}

}  // namespace ttasr_detail

extern "C" {

int ttasr_align_batch(ttasr_ctx* c, int32_t n, const int32_t* clip, const int32_t* tokens, const int32_t* n_tokens, int32_t max_tokens,
                      const int32_t* first_row, const int32_t* num_frames, const int32_t* pairs, int32_t n_pairs, int32_t medfilt_width,
                      int32_t* out_start_frame, float* out_logprob, float* out_cost, float* out_weights) {
  return guarded(c, [&]() -> int {
  TRY(check_ready(c, 1));
  const AlignBatch a{n, tokens, n_tokens, max_tokens, first_row, num_frames, pairs, n_pairs, medfilt_width,
                     out_start_frame, out_logprob, out_cost, out_weights};
  TRY(align_batch_validate(c, a));
  if (!clip) return fail(c, TTASR_E_INVALID, "NULL argument");
  for (int i = 0; i < n; ++i)
    if (clip[i] < 0 || clip[i] >= c->B_enc) return fail(c, TTASR_E_INVALID, "sequence %d: clip %d but the encoder state holds %d", i, clip[i], c->B_enc);
  // sequence i borrows the self-attention pages of row i: any step-level decode state is gone
  std::vector<int32_t> pages((size_t)n * c->pages_per_seq);
  for (size_t i = 0; i < pages.size(); ++i) pages[i] = (int32_t)i;
  c->B_dec = 0;
  return align_batch_run(c, a, clip, pages.data());
  });
}

}  // extern "C"
