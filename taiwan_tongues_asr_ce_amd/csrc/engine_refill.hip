// libttasr: the continuous-batching session for greedy, single-window decoding (one of the engine translation units, see
// engine_ctx.hpp; the life cycle is described in DESIGN.md "Continuous batching").
//
// The decode batch is always max_batch rows, so every step runs the same full-width kernel forms whatever the occupancy and a
// clip's bits do not depend on its neighbours.  Each row carries its own position (ttasr_ctx::row_pos, read by the MODE 3
// self-attention, the per-row embed LayerNorm and select_rows_kernel); a free row has done = 1 and leaves the attention
// kernels.  Submitted clips wait in a host queue; a batch of k of them is log-mel'd and encoded (batch k) into a STAGING
// cross-KV buffer, and at a poll its clips are admitted into finished rows: their cross-KV blocks are copied into the rows'
// slots and one admit_rows_kernel launch resets the rows' search state.  With option refill_overlap = 1 the encode runs on a
// second stream of the context while the step graphs replay on the main one: it shares no buffer with the decode step (the
// encoder's activations, mel and PCM buffers are its own; the decode step uses the d* rows, the K-split slabs, the logits and
// the KV pool), and the staging buffer is only rewritten after the copies of its previous batch (event ev_copy).
#include "engine_ctx.hpp"
#include <chrono>
#include <deque>

namespace ttasr_detail {

struct Session {
  struct Clip { int64_t id; std::vector<float> pcm; std::vector<int32_t> prompt; int32_t cap; };
  struct Done { int64_t id; std::vector<int32_t> tok; float lp, ns; };
  ttasr_gen_opts o{};
  int max_prompt = 0;
  int64_t next_id = 0;
  std::deque<Clip> queue;          // submitted, not yet encoded
  std::vector<Clip> staged;        // encoded into staging slots 0..k-1 (slot = index); admitted in order
  size_t staged_next = 0;          // first staged clip not admitted yet
  std::vector<int64_t> stage_ns;   // n_samples of the staged batch (source of an asynchronous copy: kept alive with it)
  bool enc_pending = false;        // overlapped encode enqueued and not yet seen complete
  std::vector<int64_t> row_clip;   // [maxB] clip id in the row, or -1 (free)
  std::vector<int32_t> row_plen;   // [maxB] prompt length of the row's clip
  std::deque<Done> finished;       // finished clips not yet returned by a poll
  int32_t* pin = nullptr;          // pinned: done | n_sampled | sum_logprob | no_speech [maxB] each, tokens [maxB][max_new], admit table
  size_t pin_words = 0;
  hipStream_t es = nullptr;        // encode stream (== the context's stream when refill_overlap = 0)
  hipEvent_t ev_enc0 = nullptr, ev_enc = nullptr, ev_copy = nullptr, ev_dec0 = nullptr, ev_dec1 = nullptr;
  bool overlap = true;
  // statistics (ttasr_session_stats)
  int64_t steps = 0, polls = 0, encodes = 0, clips_encoded = 0, live_row_steps = 0;
  double enc_ms = 0, dec_ms = 0;
};

int session_refusal(ttasr_ctx* c) {
  if (c && c->sess) return fail(c, TTASR_E_INVALID, "a continuous-batching session is open on this context (ttasr_session_end first)");
  return 0;
}

void session_free(ttasr_ctx* c) {
  Session* S = c->sess;
  if (!S) return;
  if (S->es && S->es != c->stream) { hipStreamSynchronize(S->es); hipStreamDestroy(S->es); }
  for (hipEvent_t e : {S->ev_enc0, S->ev_enc, S->ev_copy, S->ev_dec0, S->ev_dec1}) if (e) hipEventDestroy(e);
  if (S->pin) hipHostFree(S->pin);
  delete S;
  c->sess = nullptr;
  c->session_rows = false;
}

static int n_free_rows(const Session* S) {
  int n = 0;
  for (int64_t id : S->row_clip) n += id < 0;
  return n;
}

// mel + encoder of the next k queued clips into the staging cross-KV (slots 0..k-1), on S->es
static int start_encode(ttasr_ctx* c, Session* S, int k) {
  hipStream_t es = S->es;
  S->staged.clear(); S->staged_next = 0;
  S->stage_ns.assign(k, 0);
  if (es != c->stream) HIPCHK(c, hipStreamWaitEvent(es, S->ev_copy, 0));   // the previous batch's cross-KV has left the staging buffer
  HIPCHK(c, hipEventRecord(S->ev_enc0, es));
  for (int j = 0; j < k; ++j) {
    S->staged.push_back(std::move(S->queue.front()));
    S->queue.pop_front();
    const Session::Clip& cl = S->staged.back();
    S->stage_ns[j] = (int64_t)cl.pcm.size();
    if (!cl.pcm.empty())
      HIPCHK(c, hipMemcpyAsync(c->pcm_dev + (int64_t)j * c->n_samples, cl.pcm.data(), cl.pcm.size() * 4, hipMemcpyHostToDevice, es));
  }
  HIPCHK(c, hipMemcpyAsync(c->nsamp_dev, S->stage_ns.data(), (size_t)k * 8, hipMemcpyHostToDevice, es));
  launch_mel(c->pcm_dev, c->n_samples, c->nsamp_dev, k, c->M, c->F, c->filters, c->dcos, c->dsin, c->window, c->mel, c->clip_max, es);
  TT_DISPATCH(c, launch_mel_finish<T>(c->mel, c->clip_max, (T*)c->mel_t, k, c->M, c->F, es));
  // Every session pass runs the 256 x 256 GEMM family (gemm_bf16_v3; bit-identical to the persistent v4 / v5 forms that a 32-clip
  // encode picks).  The automatic choice goes by tile count, i.e. by k, and for a few clips it takes the 256 x 128 gemm_bf16_v2,
  // which rounds differently: a clip's bits would then depend on how many clips shared its pass - in overlap mode a matter of
  // GPU timing.  With the fixed family a clip's encoder output is the same in every pass (tests/test_gpu_session.py).
  void* const xkv = c->xkv;
  const int gemm_force = c->gemm_force;
  if (gemm_force == 0) c->gemm_force = 3;
  c->xkv = c->xkv_stage; c->cur = es;
  sched_encoder(c, k);
  c->xkv = xkv; c->cur = c->stream; c->gemm_force = gemm_force;
  HIPCHK(c, hipEventRecord(S->ev_enc, es));
  S->enc_pending = es != c->stream;
  S->encodes++; S->clips_encoded += k;
  return 0;
}

// staged clips -> free rows: cross-KV copies and one admit launch on the decode stream
static int admit(ttasr_ctx* c, Session* S) {
  const int avail = (int)(S->staged.size() - S->staged_next);
  if (avail == 0 || S->enc_pending) return 0;
  hipStream_t s = c->stream;
  if (S->es != s) {
    HIPCHK(c, hipStreamWaitEvent(s, S->ev_enc, 0));   // complete already (polled); orders the copies after the encode
    float ms = 0.f;
    if (S->staged_next == 0 && hipEventElapsedTime(&ms, S->ev_enc0, S->ev_enc) == hipSuccess) S->enc_ms += ms;
  }
  const int W = 3 + S->max_prompt;
  int32_t* tab = S->pin + (size_t)c->maxB * (4 + c->rp.max_new);
  const size_t blk = (size_t)c->H * c->T * 64 * c->esz, pitch = (size_t)c->xkv_which_elems * c->esz;
  int n = 0;
  for (int r = 0; r < c->maxB && (int)S->staged_next < (int)S->staged.size(); ++r) {
    if (S->row_clip[r] >= 0) continue;
    const int j = (int)S->staged_next++;
    Session::Clip& cl = S->staged[j];
    HIPCHK(c, hipMemcpy2DAsync((char*)c->xkv + (size_t)r * blk, pitch, (const char*)c->xkv_stage + (size_t)j * blk, pitch, blk,
                               2 * (size_t)c->cfg.dec_layers, hipMemcpyDeviceToDevice, s));
    int32_t* e = tab + (size_t)n * W;
    const int plen = (int)cl.prompt.size();
    // a row never samples past the text context: the static loop's last sampled position is n_text_ctx - 2
    e[0] = r; e[1] = plen; e[2] = std::min(cl.cap, c->cfg.n_text_ctx - plen);
    for (int q = 0; q < S->max_prompt; ++q) e[3 + q] = q < plen ? cl.prompt[q] : 0;
    S->row_clip[r] = cl.id; S->row_plen[r] = plen;
    ++n;
  }
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(c->admit_dev, tab, (size_t)n * W * 4, hipMemcpyHostToDevice, s));
    launch_admit_rows(c->admit_dev, n, c->maxB, S->max_prompt, c->st, c->prompt_dev, c->plen_dev, c->row_cap_dev, c->row_pos, s);
  }
  if (S->staged_next == S->staged.size()) {
    S->staged.clear(); S->staged_next = 0;
    HIPCHK(c, hipEventRecord(S->ev_copy, s));
  }
  return 0;
}

// admissions and encodes that can happen now (host side; never blocks on the GPU in overlap mode)
static int pump(ttasr_ctx* c, Session* S) {
  if (S->enc_pending) {
    const hipError_t q = hipEventQuery(S->ev_enc);
    if (q == hipSuccess) S->enc_pending = false;
    else if (q != hipErrorNotReady) return fail(c, TTASR_E_HIP, "encode event: %s", hipGetErrorString(q));
  }
  TRY(admit(c, S));
  if (S->staged.empty() && !S->queue.empty()) {
    const int free_now = n_free_rows(S);
    if (!S->overlap) {
      if (free_now == 0) return 0;
      // synchronous mode: the encode sits on the decode stream between two steps, and the host waits for it (the staged clips'
      // host buffers, sources of its copies, are released by the admission)
      TRY(start_encode(c, S, std::min<int>(free_now, (int)S->queue.size())));
      HIPCHK(c, hipEventSynchronize(S->ev_enc));
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, S->ev_enc0, S->ev_enc) == hipSuccess) S->enc_ms += ms;
      TRY(admit(c, S));
    } else {
      // encode ahead: at least an eighth of the batch per encode (small-k encoder passes are inefficient), more when rows are free now
      const int k = std::min<int>((int)S->queue.size(), std::max(free_now, std::max(1, c->maxB / 8)));
      TRY(start_encode(c, S, std::min(k, c->maxB)));
    }
  }
  return 0;
}

static int session_begin(ttasr_ctx* c, const ttasr_gen_opts* o, int max_prompt, float temperature) {
  if (!c) return TTASR_E_INVALID;
  if (!c->finalized) return fail(c, TTASR_E_INVALID, "weights not finalized (call ttasr_finalize_weights first)");
  TRY(session_refusal(c));
  if (!o) return fail(c, TTASR_E_INVALID, "opts is NULL");
  if (!(temperature == 0.f)) return fail(c, TTASR_E_INVALID, "a session decodes greedily (temperature %g: only 0)", temperature);
  if (c->xkv_fp8) return fail(c, TTASR_E_INVALID, "the e4m3 cross-KV mode (option xkv_fp8) is not supported in a session");
  if (max_prompt < 1 || max_prompt > c->max_prompt_alloc || max_prompt >= c->cfg.n_text_ctx)
    return fail(c, TTASR_E_INVALID, "max_prompt %d outside [1, %d]", max_prompt, std::min(c->max_prompt_alloc, c->cfg.n_text_ctx - 1));
  if (o->n_suppress < 0 || o->n_begin_suppress < 0 || (o->n_suppress && !o->suppress) || (o->n_begin_suppress && !o->begin_suppress))
    return fail(c, TTASR_E_INVALID, "suppress lists");
  HIPCHK(c, hipSetDevice(c->device));
  const RuleParams old = c->rp;
  TRY(upload_rules(c, o, max_prompt));   // validates max_new_tokens and the token ids; synchronises the stream
  c->rp.temperature = 0.f; c->rp.seed = 0;
  TRY(commit_rules(c, old));
  const int B = c->maxB;
  // first session of this context: its device buffers (kept for the context's lifetime)
  if (!c->row_pos) TRY(dalloc(c, &c->row_pos, (size_t)B * 4));
  if (!c->admit_dev) TRY(dalloc(c, &c->admit_dev, (size_t)B * (3 + c->max_prompt_alloc) * 4));
  if (!c->xkv_stage) TRY(dalloc(c, &c->xkv_stage, (size_t)c->xkv_layer_elems * c->cfg.dec_layers * c->esz, false));
  std::unique_ptr<Session> S(new Session());
  S->o = *o; S->o.suppress = nullptr; S->o.begin_suppress = nullptr;   // the rules are uploaded; the caller's arrays are not kept
  S->max_prompt = max_prompt;
  S->overlap = c->refill_overlap;
  S->row_clip.assign(B, -1); S->row_plen.assign(B, 1);
  S->pin_words = (size_t)B * (4 + c->rp.max_new) + (size_t)B * (3 + max_prompt);
  struct Undo { ttasr_ctx* c; Session* s; ~Undo() { if (s) { c->sess = s; session_free(c); } } } undo{c, nullptr};
  HIPCHK(c, hipHostMalloc((void**)&S->pin, S->pin_words * 4));
  for (hipEvent_t* e : {&S->ev_enc0, &S->ev_enc, &S->ev_copy, &S->ev_dec0, &S->ev_dec1}) {
    const hipError_t r = hipEventCreate(e);
    if (r != hipSuccess) { undo.s = S.release(); return fail(c, TTASR_E_HIP, "hipEventCreate: %s", hipGetErrorString(r)); }
  }
  if (S->overlap) {
    const hipError_t r = hipStreamCreateWithFlags(&S->es, hipStreamNonBlocking);
    if (r != hipSuccess) { S->es = nullptr; undo.s = S.release(); return fail(c, TTASR_E_HIP, "hipStreamCreate: %s", hipGetErrorString(r)); }
  } else {
    S->es = c->stream;
  }
  // every row free: finished (done = 1, n_done = max_batch), position 0, a valid token, a one-token prompt
  hipStream_t s = c->stream;
  int32_t* p = S->pin;
  for (int r = 0; r < B; ++r) { p[r] = 1; p[B + r] = 0; p[2 * B + r] = 1; p[3 * B + r] = B; }
  HIPCHK(c, hipMemcpyAsync(c->st.done, p, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->st.n_done, p + 3 * B, 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->plen_dev, p + 2 * B, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(c->row_pos, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.cur_tok, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.n_sampled, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.last_tok, 0xff, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.pen_tok, 0xff, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.last_ts, 0xff, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.sum_logprob, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.no_speech, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->row_cap_dev, 0x7f, (size_t)B * 4, s));
  HIPCHK(c, hipEventRecord(S->ev_copy, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->st.prompt = c->prompt_dev; c->st.prompt_len = c->plen_dev;
  c->kv_div = 1; c->identity_pages = 1;
  c->B_mel = c->B_enc = c->B_dec = 0;   // the session rewrites the encoder state and the cross-KV of every row
  c->session_rows = true;
  c->sess = S.release();
  return TTASR_OK;
}

static int session_submit(ttasr_ctx* c, int n, const float* const* pcm, const int64_t* n_samples, const int32_t* prompt,
                          const int32_t* prompt_len, const int32_t* max_new, int64_t* out_ids) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  if (n < 1) return fail(c, TTASR_E_INVALID, "n %d < 1", n);
  if (!pcm || !n_samples || !prompt || !prompt_len || !max_new) return fail(c, TTASR_E_INVALID, "NULL argument");
  const int P = S->max_prompt;
  // everything is validated before a clip is queued: a refused call leaves the session as it was
  for (int i = 0; i < n; ++i) {
    if (n_samples[i] < 0 || n_samples[i] > c->n_samples)
      return fail(c, TTASR_E_INVALID, "clip %d: %lld samples outside [0, %d] (one window)", i, (long long)n_samples[i], c->n_samples);
    if (n_samples[i] > 0 && !pcm[i]) return fail(c, TTASR_E_INVALID, "clip %d: pcm is NULL", i);
    if (prompt_len[i] < 1 || prompt_len[i] > P) return fail(c, TTASR_E_INVALID, "clip %d: prompt_len %d outside [1, %d]", i, prompt_len[i], P);
    if (prompt_len[i] >= c->cfg.n_text_ctx)
      return fail(c, TTASR_E_INVALID, "clip %d: prompt_len %d leaves no room in the %d-token context", i, prompt_len[i], c->cfg.n_text_ctx);
    for (int j = 0; j < prompt_len[i]; ++j)
      if (prompt[(size_t)i * P + j] < 0 || prompt[(size_t)i * P + j] >= c->V) return fail(c, TTASR_E_INVALID, "clip %d: prompt token outside vocabulary", i);
    if (max_new[i] < 1 || max_new[i] > S->o.max_new_tokens)
      return fail(c, TTASR_E_INVALID, "clip %d: max_new %d outside [1, max_new_tokens=%d]", i, max_new[i], S->o.max_new_tokens);
  }
  for (int i = 0; i < n; ++i) {
    Session::Clip cl;
    cl.id = S->next_id++;
    cl.pcm.assign(pcm[i], pcm[i] + n_samples[i]);
    cl.prompt.assign(prompt + (size_t)i * P, prompt + (size_t)i * P + prompt_len[i]);
    cl.cap = max_new[i];
    if (out_ids) out_ids[i] = cl.id;
    S->queue.push_back(std::move(cl));
  }
  return TTASR_OK;
}

static int run_steps(ttasr_ctx* c, Session* S, int n) {
  HIPCHK(c, hipEventRecord(S->ev_dec0, c->stream));
  for (int done = 0; done < n;) {
    const int left = n - done, run = (c->multi_step && left >= 8) ? 8 : ((c->multi_step && left >= 4) ? 4 : 1);
    TRY(step_graph(c, c->maxB, 0, run));
    done += run;
  }
  HIPCHK(c, hipEventRecord(S->ev_dec1, c->stream));
  return 0;
}

static int session_poll(ttasr_ctx* c, int max_steps, int cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp,
                        float* no_speech, int32_t* n_out) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  if (max_steps < 1 || cap < 1) return fail(c, TTASR_E_INVALID, "max_steps %d and cap %d must be >= 1", max_steps, cap);
  if (!ids || !tokens || !lens || !n_out) return fail(c, TTASR_E_INVALID, "NULL argument");
  HIPCHK(c, hipSetDevice(c->device));
  *n_out = 0;
  const int B = c->maxB, max_new = c->rp.max_new;
  const int interval = std::max(1, S->o.check_interval);
  int steps = 0;
  while (S->finished.empty()) {
    TRY(pump(c, S));
    int live = B - n_free_rows(S);
    if (live == 0) {
      if (S->enc_pending) {   // nothing to decode until the encode is done
        HIPCHK(c, hipEventSynchronize(S->ev_enc));
        S->enc_pending = false;
        continue;
      }
      if (S->staged.empty() && S->queue.empty()) break;   // nothing left
      continue;
    }
    if (steps >= max_steps) break;
    const int n = std::min(interval, max_steps - steps);
    TRY(run_steps(c, S, n));
    steps += n; S->steps += n; S->polls++;
    // one exchange per poll: the finished flags, lengths, scores and token rows of the batch
    int32_t* p = S->pin;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(p, c->st.done, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(p + B, c->st.n_sampled, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(p + 2 * B, c->st.sum_logprob, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(p + 3 * B, c->st.no_speech, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(p + 4 * B, c->st.out_tokens, (size_t)B * max_new * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, S->ev_dec0, S->ev_dec1) == hipSuccess) S->dec_ms += ms;
    for (int r = 0; r < B; ++r) {
      if (S->row_clip[r] < 0 || !p[r]) continue;
      Session::Done d;
      d.id = S->row_clip[r];
      const int len = std::min(p[B + r], max_new);
      d.tok.assign(p + 4 * B + (size_t)r * max_new, p + 4 * B + (size_t)r * max_new + len);
      memcpy(&d.lp, &p[2 * B + r], 4); memcpy(&d.ns, &p[3 * B + r], 4);
      S->live_row_steps += S->row_plen[r] - 1 + len;
      S->finished.push_back(std::move(d));
      S->row_clip[r] = -1;
    }
  }
  int k = 0;
  while (k < cap && !S->finished.empty()) {
    const Session::Done& d = S->finished.front();
    ids[k] = d.id; lens[k] = (int32_t)d.tok.size();
    memcpy(tokens + (size_t)k * max_new, d.tok.data(), d.tok.size() * 4);
    if (sum_lp) sum_lp[k] = d.lp;
    if (no_speech) no_speech[k] = d.ns;
    S->finished.pop_front();
    ++k;
  }
  *n_out = k;
  return TTASR_OK;
}

static int session_end(ttasr_ctx* c) {
  if (!c) return TTASR_E_INVALID;
  if (!c->sess) return fail(c, TTASR_E_INVALID, "no session is open");
  Session* S = c->sess;
  if (S->es && S->es != c->stream) hipStreamSynchronize(S->es);
  // the flags belong to the session: later step-level calls see live rows (as after every search)
  hipMemsetAsync(c->st.done, 0, (size_t)c->maxB * 4, c->stream);
  hipMemsetAsync(c->st.n_done, 0, 16, c->stream);
  const hipError_t e = hipStreamSynchronize(c->stream);
  session_free(c);
  c->st.prompt = nullptr; c->st.prompt_len = nullptr;
  c->B_mel = c->B_enc = c->B_dec = 0;
  if (e != hipSuccess) return fail(c, TTASR_E_HIP, "session end: %s", hipGetErrorString(e));
  return TTASR_OK;
}

}  // namespace ttasr_detail

// ---- C ABI (include/ttasr.h) ----
extern "C" {

int ttasr_session_begin(ttasr_ctx* c, const ttasr_gen_opts* o, int32_t max_prompt, float temperature) {
  return guarded(c, [&]() -> int { return session_begin(c, o, max_prompt, temperature); });
}

int ttasr_session_submit(ttasr_ctx* c, int32_t n, const float* const* pcm_host, const int64_t* n_samples, const int32_t* prompt,
                         const int32_t* prompt_len, const int32_t* max_new, int64_t* out_ids) {
  return guarded(c, [&]() -> int { return session_submit(c, n, pcm_host, n_samples, prompt, prompt_len, max_new, out_ids); });
}

int ttasr_session_poll(ttasr_ctx* c, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp,
                       float* no_speech, int32_t* n_out) {
  return guarded(c, [&]() -> int { return session_poll(c, max_steps, cap, ids, tokens, lens, sum_lp, no_speech, n_out); });
}

int ttasr_session_stats(ttasr_ctx* c, double out[8]) {
  return guarded(c, [&]() -> int {
    if (!c) return TTASR_E_INVALID;
    if (!out) return fail(c, TTASR_E_INVALID, "out is NULL");
    const Session* S = c->sess;
    if (!S) return fail(c, TTASR_E_INVALID, "no session is open");
    const double v[8] = {(double)S->steps, (double)S->polls, (double)S->encodes, (double)S->clips_encoded, (double)S->live_row_steps,
                         S->enc_ms, S->dec_ms, (double)(S->queue.size() + S->staged.size() - S->staged_next)};
    memcpy(out, v, sizeof v);
    return TTASR_OK;
  });
}

int ttasr_session_rows(ttasr_ctx* c, int32_t* row_pos, int32_t* done, int64_t* row_clip) {
  return guarded(c, [&]() -> int {
    if (!c) return TTASR_E_INVALID;
    const Session* S = c->sess;
    if (!S) return fail(c, TTASR_E_INVALID, "no session is open");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (row_pos) HIPCHK(c, hipMemcpy(row_pos, c->row_pos, (size_t)c->maxB * 4, hipMemcpyDeviceToHost));
    if (done) HIPCHK(c, hipMemcpy(done, c->st.done, (size_t)c->maxB * 4, hipMemcpyDeviceToHost));
    if (row_clip) memcpy(row_clip, S->row_clip.data(), (size_t)c->maxB * 8);
    return TTASR_OK;
  });
}

int ttasr_session_end(ttasr_ctx* c) {
  return guarded(c, [&]() -> int { return session_end(c); });
}

}  // extern "C"
