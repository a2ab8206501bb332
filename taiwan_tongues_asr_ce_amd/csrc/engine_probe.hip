// libttasr: the known-answer hook of the token-selection kernels, ttasr_select_probe (one of the engine translation units, see
// engine_ctx.hpp).  It stages the caller's rows, histories and state in the buffers the searches use, calls ONE launcher of
// kernels_decode.hip with the arguments the engine passes it, and copies the results back.  No decision of its own: what is
// chosen, summed or finished is what the kernel did.  Behind it: the sequence-bias table's install (ttasr_set_sequence_bias) and the
// hook of its kernel (ttasr_seq_bias_probe), built the same way; and the hook of the encoder attention kernels (ttasr_enc_attn_probe).
#include "engine_ctx.hpp"

namespace ttasr_detail {

// the per-row history state the searches keep: length, last, penultimate, last timestamp (the kernel records a timestamp only
// in timestamp mode, so a history decoded without timestamps has none)
struct HistState { std::vector<int32_t> n, last, pen, lts; };
static HistState hist_state(const int32_t* hist, int stride, int rows, const ttasr_gen_opts* o) {
  HistState h{std::vector<int32_t>(rows, 0), std::vector<int32_t>(rows, -1), std::vector<int32_t>(rows, -1), std::vector<int32_t>(rows, -1)};
  if (!hist) return h;
  for (int r = 0; r < rows; ++r) {
    int k = 0;
    for (; k < stride && hist[(size_t)r * stride + k] >= 0; ++k) {
      const int t = hist[(size_t)r * stride + k];
      h.pen[r] = h.last[r]; h.last[r] = t;
      if (o->timestamps && t >= o->timestamp_begin) h.lts[r] = t;
    }
    h.n[r] = k;
  }
  return h;
}

static int select_probe(ttasr_ctx* c, int form, const ttasr_select_io& io, char* sig_buf, int sig_len) {
  const int n = io.n, V = c->V;
  if (form < TTASR_SELECT_STEP || form > TTASR_SELECT_PROB) return fail(c, TTASR_E_INVALID, "select probe: form %d", form);
  if (!io.rows_host || n < 1 || n > c->maxB) return fail(c, TTASR_E_INVALID, "select probe: rows NULL or n %d outside [1, max_batch=%d]", n, c->maxB);
  const bool ruled = form <= TTASR_SELECT_TOPK, stateful = form == TTASR_SELECT_STEP || form == TTASR_SELECT_ROWS;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const ttasr_gen_opts* o = io.opts;
  HistState h;
  std::vector<int32_t> ent, pos;
  int max_new = 1;
  if (ruled) {
    if (!o) return fail(c, TTASR_E_INVALID, "select probe: opts is NULL");
    if (io.hist_host && io.hist_stride < 1) return fail(c, TTASR_E_INVALID, "select probe: hist_stride %d", io.hist_stride);
    if (o->no_speech < -1 || o->no_speech >= V) return fail(c, TTASR_E_INVALID, "select probe: no_speech id %d outside the vocabulary", o->no_speech);
    if (!(io.temperature >= 0.f) || !(io.temperature < INFINITY)) return fail(c, TTASR_E_INVALID, "select probe: temperature");
    const bool prompted = stateful && io.prompt_host;
    const int max_prompt = prompted ? io.max_prompt : 1;
    if (prompted) {
      if (!io.prompt_len_host || max_prompt < 1 || max_prompt > c->max_prompt_alloc) return fail(c, TTASR_E_INVALID, "select probe: max_prompt %d", max_prompt);
      for (int r = 0; r < n; ++r) {
        const int len = io.prompt_len_host[r];
        if (len < 1 || len > max_prompt) return fail(c, TTASR_E_INVALID, "select probe: prompt %d: length %d outside [1, %d]", r, len, max_prompt);
        for (int j = 0; j < max_prompt; ++j) {
          const int t = io.prompt_host[(size_t)r * max_prompt + j];
          if (t < 0 || t >= V) return fail(c, TTASR_E_INVALID, "select probe: prompt %d: token %d outside the vocabulary", r, t);
        }
      }
    }
    if (stateful) {
      const int np = form == TTASR_SELECT_STEP ? 1 : n;
      if (!io.positions_host) return fail(c, TTASR_E_INVALID, "select probe: positions is NULL");
      for (int r = 0; r < np; ++r)
        if (io.positions_host[r] < 0 || io.positions_host[r] >= c->cfg.n_text_ctx)
          return fail(c, TTASR_E_INVALID, "select probe: position %d outside [0, %d)", io.positions_host[r], c->cfg.n_text_ctx);
      if (io.n_done < 0 || io.n_done > c->maxB) return fail(c, TTASR_E_INVALID, "select probe: n_done %d", io.n_done);
    }
    if (form == TTASR_SELECT_SESSION) {
      const int ne = io.n_entries;
      if (ne < 1 || ne > c->maxB || !io.entries_host || !io.entry_temp_host || !io.entry_seed_host)
        return fail(c, TTASR_E_INVALID, "select probe: 1 .. max_batch entries with temperatures and seeds expected");
      for (int e = 0; e < ne; ++e) {
        const int32_t* q = io.entries_host + 4 * e;
        if (q[0] < 0 || q[0] >= n || q[1] < 0 || q[1] >= c->cfg.n_text_ctx || q[2] < 0 || q[3] < 0 || q[3] > 3)
          return fail(c, TTASR_E_INVALID, "select probe: entry %d {%d, %d, %d, %d}", e, q[0], q[1], q[2], q[3]);
        if (!(io.entry_temp_host[e] >= 0.f) || !(io.entry_temp_host[e] < INFINITY)) return fail(c, TTASR_E_INVALID, "select probe: entry %d: temperature", e);
      }
    }
    if (form == TTASR_SELECT_TOPK && (io.k < 1 || io.k > 8)) return fail(c, TTASR_E_INVALID, "select probe: k %d outside [1, 8]", io.k);
    RuleParams old = c->rp;
    TRY(upload_rules(c, o, max_prompt));   // validates max_new_tokens and the token ids; synchronises the stream
    c->rp.temperature = stateful ? io.temperature : 0.f; c->rp.seed = io.seed;
    TRY(commit_rules(c, old));
    TRY(reset_search(c, n));
    max_new = c->rp.max_new;
    h = hist_state(io.hist_host, io.hist_stride, n, o);
  } else if (form == TTASR_SELECT_LOGPROB) {
    if (!io.targets_host) return fail(c, TTASR_E_INVALID, "select probe: targets is NULL");
    for (int r = 0; r < n; ++r)
      if (io.targets_host[r] < 0 || io.targets_host[r] >= V) return fail(c, TTASR_E_INVALID, "select probe: target %d outside the vocabulary", io.targets_host[r]);
  } else if (io.token < 0 || io.token >= V) {
    return fail(c, TTASR_E_INVALID, "select probe: token %d outside the vocabulary", io.token);
  }
  HIPCHK(c, hipMemcpy2DAsync(c->logits, (size_t)c->ldv * 4, io.rows_host, (size_t)V * 4, (size_t)V * 4, n, hipMemcpyHostToDevice, s));
  auto up = [&](void* dst, const void* src, size_t bytes) -> int { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); return 0; };
  auto down = [&](void* dst, const void* src, size_t bytes) -> int { if (dst) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s)); return 0; };
  const size_t n4 = (size_t)n * 4;
  g_kernel_sig[0] = 0;
  if (stateful) {
    TRY(up(c->st.n_sampled, h.n.data(), n4)); TRY(up(c->st.last_tok, h.last.data(), n4));
    TRY(up(c->st.pen_tok, h.pen.data(), n4)); TRY(up(c->st.last_ts, h.lts.data(), n4));
    if (io.done_host) TRY(up(c->st.done, io.done_host, n4));
    if (io.row_cap_host) TRY(up(c->row_cap_dev, io.row_cap_host, n4));
    if (io.sum_logprob_host) TRY(up(c->st.sum_logprob, io.sum_logprob_host, n4));
    TRY(up(c->st.n_done, &io.n_done, 4));
    HIPCHK(c, hipMemsetAsync(c->st.cur_tok, 0xff, n4, s));
    HIPCHK(c, hipMemsetAsync(c->st.out_tokens, 0xff, n4 * max_new, s));
    DecState st = c->st; st.prompt = nullptr; st.prompt_len = nullptr;
    if (io.prompt_host) {
      TRY(up(c->prompt_dev, io.prompt_host, n4 * io.max_prompt)); TRY(up(c->plen_dev, io.prompt_len_host, n4));
      st.prompt = c->prompt_dev; st.prompt_len = c->plen_dev;
    }
    if (form == TTASR_SELECT_STEP) {
      TRY(up(c->st.step, io.positions_host, 4));   // reset_search cleared the ticket word behind it
      g_kernel_sig_on = true;
      launch_select(c->logits, st, c->rp, n, nullptr, s, c->st.step + 1, n);
      g_kernel_sig_on = false;
      TRY(down(io.out_positions, c->st.step, 8));
    } else {
      if (!c->row_pos) TRY(dalloc(c, &c->row_pos, (size_t)c->maxB * 4));
      TRY(up(c->row_pos, io.positions_host, n4));
      st.step = c->row_pos;
      g_kernel_sig_on = true;
      launch_select_rows(c->logits, st, c->rp, n, s);
      g_kernel_sig_on = false;
      TRY(down(io.out_positions, c->row_pos, n4));
    }
    TRY(down(io.out_cur_tok, c->st.cur_tok, n4)); TRY(down(io.out_n_sampled, c->st.n_sampled, n4));
    TRY(down(io.out_last_tok, c->st.last_tok, n4)); TRY(down(io.out_pen_tok, c->st.pen_tok, n4));
    TRY(down(io.out_last_ts, c->st.last_ts, n4)); TRY(down(io.out_done, c->st.done, n4));
    TRY(down(io.out_n_done, c->st.n_done, 4)); TRY(down(io.out_sum_logprob, c->st.sum_logprob, n4));
    TRY(down(io.out_no_speech, c->st.no_speech, n4)); TRY(down(io.out_tokens, c->st.out_tokens, n4 * max_new));
  } else if (ruled) {
    // the host-owned row histories of the beam searches: [4][n] in the row-state block (engine_ctx.hpp beam_row_state)
    TRY(up(c->row_state, h.n.data(), n4)); TRY(up(c->row_state + n, h.last.data(), n4));
    TRY(up(c->row_state + 2 * n, h.pen.data(), n4)); TRY(up(c->row_state + 3 * n, h.lts.data(), n4));
    if (form == TTASR_SELECT_SESSION) {
      const int ne = io.n_entries;
      if (!c->sess_sel) TRY(dalloc(c, &c->sess_sel, (size_t)c->maxB * 9 * 4));
      // device layout as the session's: entries [4 ne] | temperatures [ne] | seeds [ne], results behind the input block
      int32_t* const d_ent = c->sess_sel;
      float* const d_out = (float*)(d_ent + 6 * c->maxB);
      TRY(up(d_ent, io.entries_host, (size_t)ne * 16)); TRY(up(d_ent + 4 * ne, io.entry_temp_host, (size_t)ne * 4));
      TRY(up(d_ent + 5 * ne, io.entry_seed_host, (size_t)ne * 4));
      const SessRowsArgs sa{d_ent, (const float*)(d_ent + 4 * ne), (const uint32_t*)(d_ent + 5 * ne), d_out};
      g_kernel_sig_on = true;
      launch_session_rows_select(c->logits, beam_row_state(c, n), c->rp, sa, ne, s);
      g_kernel_sig_on = false;
      TRY(down(io.out_f32, d_out, (size_t)ne * 12));
    } else {
      g_kernel_sig_on = true;
      launch_beam_topk(c->logits, beam_row_state(c, n), c->rp, n, io.k, c->topk_lp, c->topk_id, io.want_no_speech ? c->st.no_speech : nullptr, s);
      g_kernel_sig_on = false;
      TRY(down(io.out_f32, c->topk_lp, n4 * io.k)); TRY(down(io.out_i32, c->topk_id, n4 * io.k));
      if (io.want_no_speech) TRY(down(io.out_no_speech, c->st.no_speech, n4));
    }
  } else {
    g_kernel_sig_on = true;
    if (form == TTASR_SELECT_LOGPROB) {
      TRY(up(c->prompt_dev, io.targets_host, n4));
      launch_token_logprob(c->logits, c->ldv, V, c->prompt_dev, c->topk_lp, n, s);
    } else {
      launch_token_prob(c->logits, c->ldv, V, io.token, c->topk_lp, n, s);
    }
    g_kernel_sig_on = false;
    TRY(down(io.out_f32, c->topk_lp, n4));
  }
  HIPCHK(c, hipStreamSynchronize(s));   // the staged vectors are stack temporaries
  HIPCHK(c, hipGetLastError());
  c->B_dec = 0;   // the search state no longer belongs to a step-level decode
  if (sig_buf && sig_len > 0) snprintf(sig_buf, (size_t)sig_len, "%s", g_kernel_sig);
  return TTASR_OK;
}

// ---- sequence bias: the table's install and the known-answer hook of its kernel (kernels_bias.hip) ----
static int set_sequence_bias(ttasr_ctx* c, int n_seq, const int32_t* tokens, const int32_t* offsets, const float* bias) {
  if (n_seq < 0) return fail(c, TTASR_E_INVALID, "sequence bias: n_seq %d", n_seq);
  if (n_seq > 0 && (!tokens || !offsets || !bias)) return fail(c, TTASR_E_INVALID, "sequence bias: NULL argument");
  SeqBiasHostTable t;
  if (n_seq > 0) {
    const std::string why = seq_bias_build(n_seq, tokens, offsets, bias, c->V, t);
    if (!why.empty()) return fail(c, TTASR_E_INVALID, "sequence bias: %s", why.c_str());
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // nothing enqueued reads the old table any more
  if (n_seq == 0) { c->seq_bias_n = 0; return TTASR_OK; }
  TRY(c->seq_bias_dev.ensure(c, seq_bias_block_words(c->maxB) * 4, "sequence-bias block"));
  int32_t* const d = c->seq_bias_dev.get();
  const int32_t head[4] = {(int32_t)t.groups.size(), (int32_t)t.entries.size(), 0, 0};
  c->seq_bias_n = 0;   // a failed copy leaves no half-written table in service
  HIPCHK(c, hipMemcpyAsync(d, head, sizeof head, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + kSeqBiasGroupsAt, t.groups.data(), t.groups.size() * sizeof(SeqBiasGroup), hipMemcpyHostToDevice, c->stream));
  if (!t.entries.empty()) {
    HIPCHK(c, hipMemcpyAsync(d + kSeqBiasEntriesAt, t.entries.data(), t.entries.size() * sizeof(SeqBiasEntry), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + kSeqBiasPrefixAt, t.prefix.data(), t.prefix.size() * 4, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the sources are stack temporaries
  c->seq_bias_n = n_seq;
  return TTASR_OK;
}

static int seq_bias_probe(ttasr_ctx* c, int form, const ttasr_seq_bias_io& io, char* sig_buf, int sig_len) {
  const int n = io.n, V = c->V;
  if (form != TTASR_SEQ_BIAS_WINDOW && form != TTASR_SEQ_BIAS_STATE) return fail(c, TTASR_E_INVALID, "sequence-bias probe: form %d", form);
  if (c->seq_bias_n <= 0) return fail(c, TTASR_E_INVALID, "sequence-bias probe: no table installed");
  if (!io.rows_host || !io.out_rows_host || n < 1 || n > c->maxB)
    return fail(c, TTASR_E_INVALID, "sequence-bias probe: rows NULL or n %d outside [1, max_batch=%d]", n, c->maxB);
  const bool state = form == TTASR_SEQ_BIAS_STATE;
  if (state) {
    if (!io.out_tokens_host || !io.n_sampled_host) return fail(c, TTASR_E_INVALID, "sequence-bias probe: out_tokens / n_sampled is NULL");
    if (io.max_new < 1 || io.max_new > c->max_new_alloc) return fail(c, TTASR_E_INVALID, "sequence-bias probe: max_new %d outside [1, %d]", io.max_new, c->max_new_alloc);
    if (io.position < 0 || io.position >= c->cfg.n_text_ctx) return fail(c, TTASR_E_INVALID, "sequence-bias probe: position %d", io.position);
    if (io.prompt_host && (!io.prompt_len_host || io.max_prompt < 1 || io.max_prompt > c->max_prompt_alloc))
      return fail(c, TTASR_E_INVALID, "sequence-bias probe: max_prompt %d", io.max_prompt);
    for (int r = 0; r < n; ++r) {
      if (io.n_sampled_host[r] < 0 || io.n_sampled_host[r] > io.max_new)
        return fail(c, TTASR_E_INVALID, "sequence-bias probe: row %d: n_sampled %d outside [0, %d]", r, io.n_sampled_host[r], io.max_new);
      if (io.prompt_host && (io.prompt_len_host[r] < 1 || io.prompt_len_host[r] > io.max_prompt))
        return fail(c, TTASR_E_INVALID, "sequence-bias probe: row %d: prompt length %d outside [1, %d]", r, io.prompt_len_host[r], io.max_prompt);
    }
  } else {
    if (!io.hist_host || !io.hist_len_host) return fail(c, TTASR_E_INVALID, "sequence-bias probe: hist / hist_len is NULL");
    for (int r = 0; r < n; ++r)
      if (io.hist_len_host[r] < -1 || io.hist_len_host[r] > kSeqBiasMaxLen)
        return fail(c, TTASR_E_INVALID, "sequence-bias probe: row %d: history length %d outside [-1, %d]", r, io.hist_len_host[r], kSeqBiasMaxLen);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  auto up = [&](void* dst, const void* src, size_t bytes) -> int { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s)); return 0; };
  const size_t n4 = (size_t)n * 4;
  HIPCHK(c, hipMemcpy2DAsync(c->logits, (size_t)c->ldv * 4, io.rows_host, (size_t)V * 4, (size_t)V * 4, n, hipMemcpyHostToDevice, s));
  SeqBiasHist h{};
  const int32_t pos = io.position;
  if (state) {
    // the strides the kernel reads; the next search's commit_rules uploads its own
    c->rule_dyn_host.max_prompt = io.prompt_host ? io.max_prompt : 1;
    c->rule_dyn_host.max_new = io.max_new;
    TRY(up(c->rule_dyn_dev, &c->rule_dyn_host, sizeof(RuleDyn)));
    TRY(up(c->st.out_tokens, io.out_tokens_host, n4 * io.max_new)); TRY(up(c->st.n_sampled, io.n_sampled_host, n4));
    if (io.done_host) TRY(up(c->st.done, io.done_host, n4)); else HIPCHK(c, hipMemsetAsync(c->st.done, 0, n4, s));
    TRY(up(c->st.step, &pos, 4));
    h = SeqBiasHist{c->st.out_tokens, c->st.n_sampled, nullptr, nullptr, c->st.done, c->st.step, c->rule_dyn_dev, nullptr, nullptr};
    if (io.prompt_host) {
      TRY(up(c->prompt_dev, io.prompt_host, n4 * io.max_prompt)); TRY(up(c->plen_dev, io.prompt_len_host, n4));
      h.prompt = c->prompt_dev; h.prompt_len = c->plen_dev;
    }
  } else {
    int32_t* const win = (int32_t*)seq_bias_win(c);
    TRY(up(win, io.hist_host, n4 * kSeqBiasW)); TRY(up(win + (size_t)n * kSeqBiasW, io.hist_len_host, n4));
    h.win = win; h.win_len = win + (size_t)n * kSeqBiasW;
  }
  g_kernel_sig[0] = 0;
  g_kernel_sig_on = true;
  launch_seq_bias(c->logits, c->ldv, c->seq_bias_dev.get(), h, state, n, s);
  g_kernel_sig_on = false;
  HIPCHK(c, hipMemcpy2DAsync(io.out_rows_host, (size_t)V * 4, c->logits, (size_t)c->ldv * 4, (size_t)V * 4, n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the staged scalars are stack temporaries
  HIPCHK(c, hipGetLastError());
  if (state) HIPCHK(c, hipMemsetAsync(c->st.done, 0, n4, s));   // finished flags belong to a search: later step-level calls see live rows
  c->B_dec = 0;   // the search state no longer belongs to a step-level decode
  if (sig_buf && sig_len > 0) snprintf(sig_buf, (size_t)sig_len, "%s", g_kernel_sig);
  return TTASR_OK;
}

// ---- encoder attention: the known-answer hook of enc_attn_flash_kernel (both instantiation families) and enc_attn_simple_kernel ----
// Stages the caller's operands in a block of the hook's own (c->enc_probe_dev), fills the output and one guard row behind it with a
// NaN pattern, launches ONCE through the function the engine calls (sched_enc_attn | launch_cross_attn_decode) and copies the rows
// back.  Nothing resident - mel, encoder state, cross-KV, search state, graphs - is read or written.
static int enc_attn_probe(ttasr_ctx* c, int form, int B, int T_, const float* a, const float* k, const float* v, int Tk, float* out,
                          char* sig_buf, int sig_len) {
  const bool cross = form == TTASR_ENC_CROSS;
  if (form != TTASR_ENC_SELF && !cross) return fail(c, TTASR_E_INVALID, "encoder attention probe: form %d", form);
  if (!a || !out || (sig_buf && sig_len < 1)) return fail(c, TTASR_E_INVALID, "encoder attention probe: NULL argument");
  const int d = c->d, H = c->H;
  const size_t e = c->esz;
  if (cross) {
    if (!c->lowp) return fail(c, TTASR_E_INVALID, "encoder attention probe: the cross form needs a 16-bit engine");
    if (!k || !v) return fail(c, TTASR_E_INVALID, "encoder attention probe: k / v is NULL");
    if (T_ < 1 || T_ > c->cfg.n_text_ctx) return fail(c, TTASR_E_INVALID, "encoder attention probe: %d rows per clip outside [1, n_text_ctx=%d]", T_, c->cfg.n_text_ctx);
    if (Tk < 1 || Tk > c->cfg.n_audio_ctx) return fail(c, TTASR_E_INVALID, "encoder attention probe: %d frames outside [1, n_audio_ctx=%d]", Tk, c->cfg.n_audio_ctx);
  } else if (T_ < 1 || T_ > c->cfg.n_audio_ctx) {
    return fail(c, TTASR_E_INVALID, "encoder attention probe: T %d outside [1, n_audio_ctx=%d]", T_, c->cfg.n_audio_ctx);
  }
  const int64_t rows = (int64_t)B * T_, n_in = rows * (cross ? d : 3 * d), n_kv = cross ? (int64_t)B * H * Tk * 64 : 0, n_out = rows * d;
  Carve cv;
  const size_t o_f32 = cv.take((size_t)std::max(std::max(n_in, n_kv), n_out) * 4), o_a = cv.take((size_t)n_in * e), o_k = cv.take((size_t)n_kv * e),
               o_v = cv.take((size_t)n_kv * e), o_out = cv.take((size_t)(n_out + d) * e), o_ws = cv.take(cross ? (size_t)rows * H * 8 * 66 * 4 : 0);
  TRY(c->enc_probe_dev.ensure(c, cv.used, "encoder attention probe scratch"));
  hipStream_t s = c->stream;
  char* base = c->enc_probe_dev;
  float* f32 = (float*)(base + o_f32);
  auto stage = [&](const float* src, size_t at, int64_t n) -> int {   // f32 from the host, cast to the engine type
    if (c->lowp) {
      HIPCHK(c, hipMemcpyAsync(f32, src, (size_t)n * 4, hipMemcpyHostToDevice, s));
      TT_DISPATCH(c, launch_cast<T>(f32, (T*)(base + at), n, s));
    } else {
      HIPCHK(c, hipMemcpyAsync(base + at, src, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    return 0;
  };
  TRY(stage(a, o_a, n_in));
  if (cross) { TRY(stage(k, o_k, n_kv)); TRY(stage(v, o_v, n_kv)); }
  // a NaN in either 16-bit type / in f32: a row the kernel does not write and a write behind the last row are both visible
  constexpr unsigned short kFill16 = 0x7fc0; constexpr int kFill32 = 0x7fc00000;
  if (c->lowp) HIPCHK(c, hipMemsetD16Async((hipDeviceptr_t)(base + o_out), kFill16, (size_t)(n_out + d), s));
  else HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(base + o_out), kFill32, (size_t)(n_out + d), s));
  g_kernel_sig[0] = 0; g_kernel_sig_on = true;
  if (cross) {
    // kv_div = rows per clip and a workspace for every row: the launcher's own rule decides (flash from 32 rows per clip upward)
    TT_DISPATCH(c, launch_cross_attn_decode<T>((const T*)(base + o_a), (const T*)(base + o_k), (const T*)(base + o_v), (T*)(base + o_out), (int)rows,
                                               H, Tk, T_, c->ko, s, (float*)(base + o_ws), SlabIn{}, (int)rows));
  } else {
    sched_enc_attn(c, base + o_a, base + o_out, B, T_, s);
  }
  g_kernel_sig_on = false;
  if (sig_buf) snprintf(sig_buf, (size_t)sig_len, "%s", g_kernel_sig);
  std::vector<char> guard((size_t)d * e);
  HIPCHK(c, hipMemcpyAsync(guard.data(), base + o_out + (size_t)n_out * e, guard.size(), hipMemcpyDeviceToHost, s));
  if (c->lowp) { TT_DISPATCH(c, launch_uncast<T>((const T*)(base + o_out), f32, n_out, s));
                 HIPCHK(c, hipMemcpyAsync(out, f32, (size_t)n_out * 4, hipMemcpyDeviceToHost, s)); }
  else HIPCHK(c, hipMemcpyAsync(out, base + o_out, (size_t)n_out * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  bool intact = true;
  for (int i = 0; i < d && intact; ++i)
    intact = c->lowp ? ((const unsigned short*)guard.data())[i] == kFill16 : ((const int*)guard.data())[i] == kFill32;
  return intact ? TTASR_OK : TTASR_ENC_GUARD_TOUCHED;
}

}  // namespace ttasr_detail

extern "C" {

int ttasr_enc_attn_probe(ttasr_ctx* c, int32_t form, int32_t B, int32_t T, const float* a_host, const float* k_host, const float* v_host,
                         int32_t Tk, float* out_host, char* sig_buf, int32_t sig_len) {
  return guarded(c, [&]() -> int {
  TRY(check_ready(c, B));   // refused in an open session
  return enc_attn_probe(c, form, B, T, a_host, k_host, v_host, Tk, out_host, sig_buf, sig_len);
  });
}

int ttasr_set_sequence_bias(ttasr_ctx* c, int32_t n_seq, const int32_t* tokens_host, const int32_t* offsets_host, const float* bias_host) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  return set_sequence_bias(c, n_seq, tokens_host, offsets_host, bias_host);
  });
}

int ttasr_seq_bias_probe(ttasr_ctx* c, int32_t form, const ttasr_seq_bias_io* io, char* sig_buf, int32_t sig_len) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  if (!io) return fail(c, TTASR_E_INVALID, "sequence-bias probe: io is NULL");
  return seq_bias_probe(c, form, *io, sig_buf, sig_len);
  });
}

int ttasr_select_probe(ttasr_ctx* c, int32_t form, const ttasr_select_io* io, char* sig_buf, int32_t sig_len) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  if (!io) return fail(c, TTASR_E_INVALID, "select probe: io is NULL");
  return select_probe(c, form, *io, sig_buf, sig_len);
  });
}

}  // extern "C"
