// libttasr: the continuous-batching session: greedy single-window clips, and beam groups that also take windows of long files and
// sampled attempts (one of the engine translation units, see engine_ctx.hpp; DESIGN.md "Continuous batching" and §4.13-4.15).
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
//
// Beam mode (ttasr_session_begin_beam, DESIGN.md "Beam search in a session"): the unit of admission is a GROUP of `beam` rows
// (group g = rows g*beam .. g*beam + beam - 1, cross-KV slot g read with kv_div = beam), the batch is R = G*beam rows.  The
// search runs on the host as in beam_search_impl: every step is the logits-only decode step (mode 1, per-row positions, loaded
// page tables) plus the candidate kernel, with ONE host exchange: page tables, fed tokens, positions, finished flags, history and
// copy-on-write pairs go out from one pinned block, the top-k candidates come back, and the shared selection code
// (beam_select / beam_pick) advances every searching group.  The page book (BeamPages), the pinned block (BeamExchange) and the
// history / candidate enqueues are beam_search_impl's own; only the loop around them differs.  Positions belong to the host;
// nothing on the device advances them.
//
// A group has a MODE, fixed when a clip is admitted: BEAM (temperature 0, rows > 1, and every clip of ttasr_session_submit) is
// the search above; ROWS (ttasr_session_submit_windows with temperature 0 and one row: greedy; temperature > 0: `rows`
// Gumbel-max samples) decodes independent rows, chosen on the device by session_rows_select_kernel in the same step as the
// candidate kernel, with the same one synchronisation.  A ROWS row ends at EOT or at its budget and its group when all its
// rows have ended; the pick is ttasr_generate_sample's (sample_pick).  Window clips (ttasr_session_submit_windows) carry the
// samples their window's STFT reads and the geometry of ttasr_log_mel_windows; a pass that holds one runs the mel in window form.
//
// Language detection inside the session (ttasr_session_detect_language): an ARMED session takes prompts
// that hold the placeholder TTASR_TOKEN_DETECT directly behind a <|startoftranscript|> token.  Such a clip's first step after
// admission is a detect step - <|startoftranscript|> at position 0 against the clip's own cross-KV, an ordinary step of the
// batch - and behind it lang_head_rows_kernel (kernels_lang.hip) computes the language of the rows whose pending flag is up.
// Greedy: the flag, the placeholder's slot and the fed token are set on the device at admission, the kernel patches the device
// prompt and restarts the row itself, and the launch is part of the armed session's step graphs (StepShape::lang_rows).  Beam: the
// kernel runs behind the logits-only step for the first row of each detecting group, its results come back in the step's one
// synchronisation, and the host patches the group's prompt and leaves its position at 0.  Either way the clip then decodes as if
// the language had been given: position 0 of its self-attention pages is simply written again.
//
// Prompt prefill at admission (option session_prefill = N > 0): a clip whose own prompt has p >= N
// prefillable positions (session_prefill_positions, prefill_tables.hpp) gets positions 0 .. p - 1 from an ADMISSION PASS - the
// decoder layers over the packed prompt rows of the clips admitted together (sched_admit_prefill), enqueued on the decode stream
// behind their cross-KV copies, between two steps - and its row (group) starts stepping at position p with prompt[p].  Greedy: the
// row's identity pages; beam: prefix pages taken once per group and shared by its rows (BeamPages::share_fresh), the partially
// filled last one split by the copy-on-write of the first private write.  The pass has its own workspace, so it runs with
// refill_overlap 0 and 1; a clip's bits do not depend on its pass-mates.  With the option at 0 nothing of this is enqueued.
//
// A new search on a held clip (ttasr_session_retry; beam sessions): in hold mode a finished clip keeps
// its group and cross-KV slot, and a retry starts the group over under a new clip id with its own prompt, budget, temperature,
// rows and seed.  admit() and the retry set the group up through the same start_group(); the retry enqueues no mel, encoder,
// copy or quantiser work - the slot (and its e4m3 block) is the one the clip's only encoder pass filled - so a retried clip
// equals the same audio submitted afresh with those parameters.
#include "engine_ctx.hpp"
#include <chrono>
#include <cmath>
#include <deque>

namespace ttasr_detail {

struct Session {
  struct Clip { int64_t id; std::vector<float> pcm; std::vector<int32_t> prompt; int32_t cap;
                // window clips: pcm = the samples the window's frames read, geom = ttasr_log_mel_windows' geometry, floor = the
                // ordered dynamic-range maximum (has_floor) ; search: mode (0 BEAM, 1 ROWS), rows, temperature, seed, sot index
                bool win = false, has_floor = false; int64_t geom[3] = {0, 0, 0}; unsigned floor = 0;
                int mode = 0, rows = 0; float temp = 0.f; uint32_t seed = 0; int32_t sot = 0;
                int det = -1; };   // armed session: the prompt index of the language placeholder, or -1
  // the language found for a clip inside the session: index into the span (-1: the clip carried no placeholder), softmax, span logits
  struct Lang { int idx = -1; std::vector<float> probs, logits; };
  struct Done { int64_t id; std::vector<int32_t> tok; float lp, ns; Lang lang; };
  ttasr_gen_opts o{};
  int max_prompt = 0;
  int64_t next_id = 0;
  std::deque<Clip> queue;          // submitted, not yet encoded
  std::vector<Clip> staged;        // encoded into staging slots 0..k-1 (slot = index); admitted in order
  size_t staged_next = 0;          // first staged clip not admitted yet
  std::vector<int64_t> stage_ns;   // n_samples of the staged batch (source of an asynchronous copy: kept alive with it)
  std::vector<int64_t> stage_geom; // [k][3] mel geometry of a pass that holds a window clip (idem)
  std::vector<unsigned> stage_floor;   // [k] ordered dynamic-range maxima of its window clips (idem)
  bool enc_pending = false;        // overlapped encode enqueued and not yet seen complete
  std::vector<int64_t> row_clip;   // [maxB] clip id in the row, or -1 (free)
  std::vector<int32_t> row_plen;   // [maxB] prompt length of the row's clip
  // language detection (ttasr_session_detect_language): the span, and per row (greedy) whether its clip's result is still on the
  // device (row_det 1) and the result once it is here; pinned block: admission table [maxB][2] | pending flags [maxB] (beam
  // upload) | winners [maxB] | probs [maxB][128] | logits [maxB][128] (the device block's result part, one copy)
  bool armed = false; int lang_sot = 0, lang_begin = 0, lang_n = 0;
  std::vector<char> row_det;
  std::vector<Lang> row_lang;
  PinBlock<int32_t> lang_pin;
  std::deque<Done> finished;       // finished clips not yet returned by a poll
  // hold mode (ttasr_session_hold): a finished clip keeps its unit - row (greedy) or group (beam) - and its cross-KV slot until
  // ttasr_session_align or ttasr_session_release; its rows are finished rows (done = 1), out of the attention kernels
  bool hold = false;
  std::vector<char> held;          // [maxB] greedy: the row's clip has finished and is held (row_clip keeps its id)
  PinBlock<int32_t> pin;           // pinned: done | n_sampled | sum_logprob | no_speech [maxB] each, tokens [maxB][max_new], admit table
  size_t pin_words = 0;
  hipStream_t es = nullptr;        // encode stream: es_own's, or the context's stream when refill_overlap = 0 (not the session's to destroy)
  OwnStream es_own;
  Event ev_enc0, ev_enc, ev_copy, ev_dec0, ev_dec1;
  bool overlap = true;
  // statistics (ttasr_session_stats)
  int64_t steps = 0, polls = 0, encodes = 0, clips_encoded = 0, live_row_steps = 0;
  double enc_ms = 0, dec_ms = 0;
  // beam mode (beam > 0): G groups of `beam` rows; per group the clip, its prompt, budget, position, no-speech value and finished
  // hypotheses; per row the hypothesis and its double-precision sum; one page book for all groups
  struct Group { int64_t clip = -1; std::vector<int32_t> prompt; int32_t cap = 0; int pos = 0; float ns = 0.f;
                 std::map<std::vector<int>, double> finished;
                 int mode = 0, rows = 0, sot = 0, max_cand = 1; float temp = 0.f; uint32_t seed = 0;
                 int det = -1; Lang lang;   // det >= 0: the group's next step is its detect step (placeholder at prompt[det])
                 int64_t held = -1; };   // hold mode: the finished clip that still owns the group (clip is -1 then)
  enum { BEAM = 0, ROWS = 1 };
  int beam = 0, G = 0, max_cand = 0;
  float patience = 1.f;
  std::vector<float> fsums;        // [R] f32 sum_logprob of the rows of ROWS groups (the device's order of additions)
  std::vector<Group> grp;
  std::vector<std::vector<int>> seqs;
  std::vector<double> sums;
  BeamPages pages;
  std::vector<int32_t> cur_tok, done_rows, pairs;
  std::unique_ptr<SearchScope> scope;   // the session's decode shape, from session_begin to session_end / session_free
  // prompt prefill at admission: the threshold (0: off); per greedy row the position its clip started stepping at; the pinned
  // tables of the last admission's passes, alive until ev_pf has completed (pf_busy); (start, stop) events of passes whose time
  // has not been collected yet; statistics (ttasr_session_prefill_stats)
  int prefill = 0;
  std::vector<int32_t> row_start;
  PinBlock<int32_t> pf_pin;
  Event ev_pf; bool pf_busy = false;
  std::vector<Event> pf_ev; size_t pf_ev_used = 0;
  int64_t pf_passes = 0, pf_clips = 0, pf_positions = 0; double pf_ms = 0;
  // before the members go: the encode stream is idle when it is destroyed, and the last pass no longer reads its pinned tables
  ~Session() {
    if (es_own) hipStreamSynchronize(es_own);
    if (pf_busy) hipEventSynchronize(ev_pf);
  }
};

// words of the table block of one admission (pinned and device): every unit admitted at once with the longest prompt
static size_t prefill_tab_cap(const ttasr_ctx* c) {
  return prefill_table_words(c->maxB * c->cfg.n_text_ctx, c->maxB, c->maxB * prefill_items_of(c->cfg.n_text_ctx), c->pages_per_seq);
}

int session_refusal(ttasr_ctx* c) {
  if (c && c->sess) return fail(c, TTASR_E_INVALID, "a continuous-batching session is open on this context (ttasr_session_end first)");
  return 0;
}

void session_free(ttasr_ctx* c) {
  delete c->sess;   // with its scope: the context is back to the defaults of a static search
  c->sess = nullptr;
}

static int n_free_rows(const Session* S) {
  int n = 0;
  for (int64_t id : S->row_clip) n += id < 0;
  return n;
}

// units of admission: rows (greedy) or groups of `beam` rows (beam mode)
static int n_units(const ttasr_ctx* c, const Session* S) { return S->beam ? S->G : c->maxB; }
static int n_free_units(const Session* S) {
  if (!S->beam) return n_free_rows(S);
  int n = 0;
  for (const Session::Group& g : S->grp) n += g.clip < 0 && g.held < 0;
  return n;
}
static int n_held_units(const Session* S) {
  int n = 0;
  if (S->beam) { for (const Session::Group& g : S->grp) n += g.held >= 0; }
  else for (char h : S->held) n += h != 0;
  return n;
}

// mel + encoder of the next k queued clips into the staging cross-KV (slots 0..k-1), on S->es
static int start_encode(ttasr_ctx* c, Session* S, int k) {
  hipStream_t es = S->es;
  S->staged.clear(); S->staged_next = 0;
  S->stage_ns.assign(k, 0);
  if (es != c->stream) HIPCHK(c, hipStreamWaitEvent(es, S->ev_copy, 0));   // the previous batch's cross-KV has left the staging buffer
  HIPCHK(c, hipEventRecord(S->ev_enc0, es));
  bool any_win = false;
  for (int j = 0; j < k; ++j) {
    S->staged.push_back(std::move(S->queue.front()));
    S->queue.pop_front();
    any_win |= S->staged.back().win;
  }
  // a pass that holds a window clip runs the mel in window form (ttasr_log_mel_windows: PCM stride n_samples + 512, per-clip
  // geometry); its plain clips get the geometry that reproduces the single-clip form exactly (lead 0, reflection at the window
  // end, every frame valid).  A pass of plain clips only runs the single-clip form, as before.
  const int64_t stride = any_win ? c->n_samples + 512 : c->n_samples;
  S->stage_geom.assign(any_win ? 3 * (size_t)k : 0, 0);
  S->stage_floor.assign(k, 0);
  for (int j = 0; j < k; ++j) {
    const Session::Clip& cl = S->staged[j];
    S->stage_ns[j] = (int64_t)cl.pcm.size();
    if (any_win) {
      const int64_t plain[3] = {0, (int64_t)c->F * 160, c->F};
      memcpy(&S->stage_geom[3 * (size_t)j], cl.win ? cl.geom : plain, 24);
      if (!cl.win) S->stage_ns[j] = std::min<int64_t>(S->stage_ns[j], (int64_t)c->F * 160);
    }
    if (!cl.pcm.empty())
      HIPCHK(c, hipMemcpyAsync(c->pcm_dev + (int64_t)j * stride, cl.pcm.data(), cl.pcm.size() * 4, hipMemcpyHostToDevice, es));
  }
  HIPCHK(c, hipMemcpyAsync(c->nsamp_dev, S->stage_ns.data(), (size_t)k * 8, hipMemcpyHostToDevice, es));
  const int64_t* geom = nullptr;
  if (any_win) {
    HIPCHK(c, hipMemcpyAsync(c->mel_geom, S->stage_geom.data(), (size_t)k * 24, hipMemcpyHostToDevice, es));
    geom = c->mel_geom;
  }
  launch_mel(c->pcm_dev, stride, c->nsamp_dev, k, c->M, c->F, c->filters, c->dcos, c->dsin, c->window, c->mel, c->clip_max, es, geom);
  for (int j = 0; j < k; ++j) {   // the file's maximum decides a window's dynamic-range floor (ttasr_log_mel_windows floor_max)
    const Session::Clip& cl = S->staged[j];
    if (!cl.has_floor) continue;
    S->stage_floor[j] = cl.floor;
    HIPCHK(c, hipMemcpyAsync(c->clip_max + j, &S->stage_floor[j], 4, hipMemcpyHostToDevice, es));
  }
  TT_DISPATCH(c, launch_mel_finish<T>(c->mel, c->clip_max, (T*)c->mel_t, k, c->M, c->F, es, geom));
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

// one xkv_quant_slots_kernel launch for the n (staging slot, live slot) pairs collected by an admission (n = 0: nothing to do)
static int flush_quant_pairs(ttasr_ctx* c, const XkvSlotPairs& qp, int& n) {
  if (n == 0) return 0;
  TT_DISPATCH(c, launch_xkv_quant_slots<T>((const T*)c->xkv_stage, c->xkv8, c->xkv8_scale, c->cfg.dec_layers, c->H, c->T, c->maxB,
                                           c->xkv_which_elems, qp, n, c->stream));
  n = 0;
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The times of the passes enqueued so far -> pf_ms.  Waits for the last pass; behind a poll's synchronisation it has completed.
static int prefill_collect(ttasr_ctx* c, Session* S) {
  if (!S->pf_busy) return 0;
  HIPCHK(c, hipEventSynchronize(S->ev_pf));
  for (size_t i = 0; i + 1 < S->pf_ev_used; i += 2) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, S->pf_ev[i], S->pf_ev[i + 1]) == hipSuccess) S->pf_ms += ms;
  }
  S->pf_ev_used = 0; S->pf_busy = false;
  return 0;
}

// The admission passes over the sequences collected by admit(): cut by whole sequences at the workspace's rows, the tables of all
// passes built in the session's pinned block (it outlives the copy: released by ev_pf) and uploaded in ONE copy, then one
// sched_admit_prefill per pass on the decode stream, behind the clips' cross-KV copies.
// The ONE place where an admission may wait for the GPU: the table blocks (pinned and device) are single, so a second admission
// with prefilled clips first waits for the previous admission's last pass (prefill_collect).  Every poll synchronises the decode
// stream behind its steps, so the event has completed whenever a poll lies between the two admissions - the usual case; with
// refill_overlap = 1 two admissions inside one poll (a pass of clips admitted, then the next encode found complete) can make
// pump() wait for a pass of a few ms.  Results do not depend on it.
static int run_prefill_passes(ttasr_ctx* c, Session* S, const std::vector<PrefillSeq>& sq) {
  if (sq.empty()) return 0;
  TRY(prefill_collect(c, S));   // the previous admission's tables are free
  hipStream_t s = c->stream;
  const int pps = c->pages_per_seq;
  std::vector<int> len(sq.size());
  for (size_t i = 0; i < sq.size(); ++i) len[i] = sq[i].len;
  const std::vector<int> cut = prefill_pass_split(len, kPrefillRowCap);
  std::vector<PrefillPass> passes;
  size_t w = 0;
  for (size_t k = 0; k + 1 < cut.size(); ++k) {
    int rows = 0, items = 0;
    const int n = cut[k + 1] - cut[k];
    for (int i = cut[k]; i < cut[k + 1]; ++i) { rows += len[i]; items += prefill_items_of(len[i]); }
    const size_t o_slots = w + (size_t)rows * 3, o_seqs = o_slots + rows, o_items = o_seqs + (size_t)n * (3 + pps);
    if (rows > kPrefillRowCap || o_items + (size_t)items * 3 > c->pf_tab_words)
      return fail(c, TTASR_E_INVALID, "session prefill: pass of %d rows / table of %zu words exceeds the workspace", rows, o_items + (size_t)items * 3);
    int32_t* const hp = S->pf_pin;
    prefill_build_tables(&sq[cut[k]], n, pps, hp + w, hp + o_slots, hp + o_seqs, hp + o_items);
    const int32_t* const dp = c->pf_tab;
    passes.push_back(PrefillPass{dp + w, dp + o_slots, dp + o_seqs, dp + o_items, rows, n, items, 3 + pps});
    w = o_items + (size_t)items * 3;
  }
  while (S->pf_ev.size() < 2 * passes.size()) {
    S->pf_ev.emplace_back();
    TRY(event_create(c, S->pf_ev.back()));
  }
  HIPCHK(c, hipMemcpyAsync(c->pf_tab, S->pf_pin, w * 4, hipMemcpyHostToDevice, s));
  for (size_t k = 0; k < passes.size(); ++k) {
    HIPCHK(c, hipEventRecord(S->pf_ev[2 * k], s));
    sched_admit_prefill(c, passes[k]);
    HIPCHK(c, hipEventRecord(S->pf_ev[2 * k + 1], s));
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S->ev_pf, s));
  S->pf_ev_used = 2 * passes.size(); S->pf_busy = true;
  S->pf_passes += (int64_t)passes.size(); S->pf_clips += (int64_t)sq.size();
  for (int l : len) S->pf_positions += l;
  return 0;
}

// Group g takes clip cl for a new search (admit, and ttasr_session_retry on a held group): mode, candidate count, page lists and
// host search state; the prefix of a prefilled prompt is collected in pf_seq / pf_pages for the caller's admission pass.  The
// group's cross-KV slot is the caller's business: admit has just enqueued the copy into it, a retry leaves it as it is.
static void start_group(ttasr_ctx* c, Session* S, int g, Session::Clip& cl, std::vector<PrefillSeq>& pf_seq,
                        std::vector<std::vector<int32_t>>& pf_pages) {
  Session::Group& gr = S->grp[g];
  const int plen = (int)cl.prompt.size();
  gr.clip = cl.id; gr.prompt = std::move(cl.prompt); gr.pos = 0; gr.ns = 0.f; gr.finished.clear();
  // the static search's last sampled position is n_text_ctx - 2: a clip never holds more than n_text_ctx - plen tokens
  gr.cap = std::min(cl.cap, c->cfg.n_text_ctx - plen);
  gr.mode = cl.mode; gr.rows = cl.rows; gr.temp = cl.temp; gr.seed = cl.seed; gr.sot = cl.sot;
  gr.det = cl.det; gr.lang = Session::Lang{};
  gr.max_cand = std::max(1, (int)std::lround(cl.rows * S->patience));
  // prompt prefill: the prefix pages are taken ONCE for the group and shared by its rows, as the static search's batched
  // prefill does; a pool that cannot supply them leaves the clip forced (a per-clip decision from pool state)
  int start = session_prefill_positions(plen, S->o.no_speech >= 0 ? gr.sot : -1, S->prefill, gr.det >= 0);
  const int n_pg = (start + kPrefillPageTokens - 1) / kPrefillPageTokens;
  if (start > 0 && (size_t)n_pg > S->pages.free_pages.size()) start = 0;
  if (start > 0) {
    pf_pages.emplace_back(n_pg);
    for (int q = 0; q < n_pg; ++q) pf_pages.back()[q] = S->pages.share_fresh(g * S->beam, S->beam, q);
    pf_seq.push_back(PrefillSeq{g, start, gr.prompt.data(), nullptr});
    gr.pos = start;
  }
  for (int b = 0; b < S->beam; ++b) {   // rows beyond the clip's `rows` stay finished
    const int r = g * S->beam + b;
    S->seqs[r].clear(); S->sums[r] = 0.0; S->fsums[r] = 0.f;
    S->row_clip[r] = cl.id; S->cur_tok[r] = gr.det >= 0 ? S->lang_sot : gr.prompt[start]; S->done_rows[r] = b < cl.rows ? 0 : 1;
  }
}

// staged clips -> free rows: cross-KV copies, the admission pass of the clips whose prompts are prefilled, and one admit launch
// on the decode stream
static int admit(ttasr_ctx* c, Session* S) {
  const int avail = (int)(S->staged.size() - S->staged_next);
  if (avail == 0 || S->enc_pending) return 0;
  hipStream_t s = c->stream;
  if (S->es != s) {
    HIPCHK(c, hipStreamWaitEvent(s, S->ev_enc, 0));   // complete already (polled); orders the copies after the encode
    float ms = 0.f;
    if (S->staged_next == 0 && hipEventElapsedTime(&ms, S->ev_enc0, S->ev_enc) == hipSuccess) S->enc_ms += ms;
  }
  const size_t blk = (size_t)c->H * c->T * 64 * c->esz, pitch = (size_t)c->xkv_which_elems * c->esz;
  // mode 2 of option xkv_fp8: the admitted clips' e4m3 blocks and scales, quantised from staging slot j straight into live slot r
  // (or group slot g) on the decode stream, behind the same event as the 16-bit copies; pairs by value, no copy to wait for
  XkvSlotPairs qp; int nq = 0;
  auto quant_pair = [&](int from, int to) -> int {
    if (!c->xkv8_valid) return 0;
    qp.src[nq] = (uint16_t)from; qp.dst[nq] = (uint16_t)to;
    if (++nq == XkvSlotPairs::N) return flush_quant_pairs(c, qp, nq);
    return 0;
  };
  // the clips of this admission whose prompt positions 0 .. len - 1 come from a pass; tokens and pages stay alive until the call returns
  std::vector<PrefillSeq> pf_seq;
  std::vector<std::vector<int32_t>> pf_pages;
  if (S->beam) {
    // a free group takes the clip: its cross-KV goes to slot g; the search state is host-side and goes out with the next step
    for (int g = 0; g < S->G && (int)S->staged_next < (int)S->staged.size(); ++g) {
      Session::Group& gr = S->grp[g];
      if (gr.clip >= 0 || gr.held >= 0) continue;
      const int j = (int)S->staged_next++;
      Session::Clip& cl = S->staged[j];
      HIPCHK(c, hipMemcpy2DAsync((char*)c->xkv + (size_t)g * blk, pitch, (const char*)c->xkv_stage + (size_t)j * blk, pitch, blk,
                                 2 * (size_t)c->cfg.dec_layers, hipMemcpyDeviceToDevice, s));
      TRY(quant_pair(j, g));
      start_group(c, S, g, cl, pf_seq, pf_pages);
    }
    TRY(flush_quant_pairs(c, qp, nq));
    for (size_t i = 0; i < pf_seq.size(); ++i) pf_seq[i].pages = pf_pages[i].data();   // (pf_pages no longer grows)
    TRY(run_prefill_passes(c, S, pf_seq));
    if (S->staged_next == S->staged.size()) {
      S->staged.clear(); S->staged_next = 0;
      HIPCHK(c, hipEventRecord(S->ev_copy, s));
    }
    return 0;
  }
  const int W = 4 + S->max_prompt;
  int32_t* tab = S->pin + (size_t)c->maxB * (4 + c->rp.max_new);
  int n = 0, n_det = 0;
  for (int r = 0; r < c->maxB && (int)S->staged_next < (int)S->staged.size(); ++r) {
    if (S->row_clip[r] >= 0) continue;
    const int j = (int)S->staged_next++;
    Session::Clip& cl = S->staged[j];
    HIPCHK(c, hipMemcpy2DAsync((char*)c->xkv + (size_t)r * blk, pitch, (const char*)c->xkv_stage + (size_t)j * blk, pitch, blk,
                               2 * (size_t)c->cfg.dec_layers, hipMemcpyDeviceToDevice, s));
    TRY(quant_pair(j, r));
    int32_t* e = tab + (size_t)n * W;
    const int plen = (int)cl.prompt.size();
    // a row never samples past the text context: the static loop's last sampled position is n_text_ctx - 2
    // prompt prefill: positions 0 .. start - 1 come from the admission pass (the row's identity pages), the row steps from `start`
    const int start = session_prefill_positions(plen, S->o.no_speech >= 0 ? S->o.sot_index : -1, S->prefill, cl.det >= 0);
    if (start > 0) {
      pf_pages.emplace_back((start + kPrefillPageTokens - 1) / kPrefillPageTokens);
      for (size_t q = 0; q < pf_pages.back().size(); ++q) pf_pages.back()[q] = r * c->pages_per_seq + (int)q;
      pf_seq.push_back(PrefillSeq{r, start, cl.prompt.data(), nullptr});
    }
    e[0] = r; e[1] = plen; e[2] = std::min(cl.cap, c->cfg.n_text_ctx - plen); e[3] = start;
    for (int q = 0; q < S->max_prompt; ++q) e[4 + q] = q < plen ? cl.prompt[q] : 0;
    S->row_clip[r] = cl.id; S->row_plen[r] = plen; S->row_start[r] = start;
    if (S->armed) {
      S->row_det[r] = cl.det >= 0; S->row_lang[r] = Session::Lang{};
      if (cl.det >= 0) { S->lang_pin[2 * n_det] = r; S->lang_pin[2 * n_det + 1] = cl.det; ++n_det; }
    }
    ++n;
  }
  TRY(flush_quant_pairs(c, qp, nq));
  for (size_t i = 0; i < pf_seq.size(); ++i) pf_seq[i].pages = pf_pages[i].data();   // (pf_pages no longer grows)
  TRY(run_prefill_passes(c, S, pf_seq));
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(c->admit_dev, tab, (size_t)n * W * 4, hipMemcpyHostToDevice, s));
    launch_admit_rows(c->admit_dev, n, c->maxB, S->max_prompt, c->st, c->prompt_dev, c->plen_dev, c->row_cap_dev, c->row_pos, s);
  }
  if (n_det > 0) {   // detecting rows: fed <|startoftranscript|> instead of prompt[0], flag and slot for lang_head_rows_kernel
    int32_t* const ls = c->lang_sess;
    HIPCHK(c, hipMemcpyAsync(ls + 2 * c->maxB, S->lang_pin, (size_t)n_det * 8, hipMemcpyHostToDevice, s));
    launch_lang_admit_rows(ls + 2 * c->maxB, n_det, c->maxB, S->lang_sot, ls, ls + c->maxB, c->st.cur_tok, s);
  }
  if (S->staged_next == S->staged.size()) {
    S->staged.clear(); S->staged_next = 0;
    HIPCHK(c, hipEventRecord(S->ev_copy, s));
  }
  return 0;
}

// admissions and encodes that can happen now (host side; never blocks on the GPU in overlap mode - but for the table wait of
// run_prefill_passes with option session_prefill)
static int pump(ttasr_ctx* c, Session* S) {
  if (S->enc_pending) {
    const hipError_t q = hipEventQuery(S->ev_enc);
    if (q == hipSuccess) S->enc_pending = false;
    else if (q != hipErrorNotReady) return fail(c, TTASR_E_HIP, "encode event: %s", hipGetErrorString(q));
  }
  TRY(admit(c, S));
  if (S->staged.empty() && !S->queue.empty()) {
    const int free_now = n_free_units(S), units = n_units(c, S);
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
      const int k = std::min<int>((int)S->queue.size(), std::max(free_now, std::max(1, units / 8)));
      TRY(start_encode(c, S, std::min(k, units)));
    }
  }
  return 0;
}

// The packed pass's own workspace (admission passes of option session_prefill, the alignment pass of option align_packed and its
// probe): kPrefillRowCap rows of activations, the device tables and the all -1 head selection.  Kept for the context's lifetime.
int prefill_workspace(ttasr_ctx* c) {
  const size_t R = kPrefillRowCap, e = c->esz;
  if (!c->pf_x) TRY(dalloc(c, &c->pf_x, R * c->d * 4));
  if (!c->pf_h) TRY(dalloc(c, &c->pf_h, R * c->d * e));
  if (!c->pf_qkv) TRY(dalloc(c, &c->pf_qkv, R * 3 * c->d * e));
  if (!c->pf_att) TRY(dalloc(c, &c->pf_att, R * c->d * e));
  if (!c->pf_mid) TRY(dalloc(c, &c->pf_mid, R * c->ffn * e));
  if (!c->pf_tab) { c->pf_tab_words = prefill_tab_cap(c); TRY(dalloc(c, &c->pf_tab, c->pf_tab_words * 4)); }
  if (!c->pf_sel) {
    TRY(dalloc(c, &c->pf_sel, (size_t)c->H * 4, false));
    HIPCHK(c, hipMemsetAsync(c->pf_sel, 0xff, (size_t)c->H * 4, c->stream));   // no head writes a softmax map
  }
  return 0;
}

static int session_begin(ttasr_ctx* c, const ttasr_gen_opts* o, int max_prompt, float temperature, StepShape shape) {
  if (!c) return TTASR_E_INVALID;
  if (!c->finalized) return fail(c, TTASR_E_INVALID, "weights not finalized (call ttasr_finalize_weights first)");
  TRY(session_refusal(c));
  TRY(seq_bias_refusal(c));
  if (!o) return fail(c, TTASR_E_INVALID, "opts is NULL");
  if (!(temperature == 0.f)) return fail(c, TTASR_E_INVALID, "a session decodes greedily (temperature %g: only 0)", temperature);
  // value 2 of the option is the session-capable mode: admitted clips are quantised from the staging buffer into their live slots
  if (c->xkv_fp8 == 1) return fail(c, TTASR_E_INVALID, "the e4m3 cross-KV mode (option xkv_fp8) is not supported in a session");
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
  if (!c->admit_dev) TRY(dalloc(c, &c->admit_dev, (size_t)B * (4 + c->max_prompt_alloc) * 4));
  if (!c->xkv_stage) TRY(dalloc(c, &c->xkv_stage, (size_t)c->xkv_layer_elems * c->cfg.dec_layers * c->esz, false));
  if (c->session_prefill > 0) TRY(prefill_workspace(c));   // first session with prompt prefill: the pass's own workspace and tables
  std::unique_ptr<Session> S(new Session());
  S->prefill = c->session_prefill;
  S->o = *o; S->o.suppress = nullptr; S->o.begin_suppress = nullptr;   // the rules are uploaded; the caller's arrays are not kept
  S->max_prompt = max_prompt;
  S->overlap = c->refill_overlap;
  S->row_clip.assign(B, -1); S->row_plen.assign(B, 1); S->held.assign(B, 0); S->row_start.assign(B, 0);
  S->pin_words = (size_t)B * (4 + c->rp.max_new) + (size_t)B * (4 + max_prompt);
  // every return from here to the end deletes the session with what it owns so far
  TRY(S->pin.ensure(c, S->pin_words * 4, "session pinned block"));
  if (S->prefill > 0) {
    TRY(S->pf_pin.ensure(c, prefill_tab_cap(c) * 4, "session prefill tables"));
    TRY(event_create(c, S->ev_pf));
  }
  for (Event* e : {&S->ev_enc0, &S->ev_enc, &S->ev_copy, &S->ev_dec0, &S->ev_dec1}) TRY(event_create(c, *e));
  if (S->overlap) TRY(stream_create(c, S->es_own));
  S->es = S->overlap ? S->es_own.h : c->stream;
  // the search state of a static search, except: every row free - finished (done = 1, n_done = max_batch) - at position 0 with a
  // valid token and a one-token prompt
  hipStream_t s = c->stream;
  TRY(reset_search(c, B));
  int32_t* p = S->pin;
  for (int r = 0; r < B; ++r) { p[r] = 1; p[B + r] = 0; p[2 * B + r] = 1; p[3 * B + r] = B; }
  HIPCHK(c, hipMemcpyAsync(c->st.done, p, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->st.n_done, p + 3 * B, 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->plen_dev, p + 2 * B, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(c->row_pos, 0, (size_t)B * 4, s));
  HIPCHK(c, hipMemsetAsync(c->st.cur_tok, 0, (size_t)B * 4, s));
  HIPCHK(c, hipEventRecord(S->ev_copy, s));
  HIPCHK(c, hipStreamSynchronize(s));
  S->scope.reset(new SearchScope(c, shape, c->prompt_dev, c->plen_dev, B));
  c->B_mel = c->B_enc = c->B_dec = 0;   // the session rewrites the encoder state and the cross-KV of every row
  // mode 2: the e4m3 copy is live for the whole session.  A free slot's stale block is never read: its rows are finished rows
  c->xkv8_valid = c->xkv_fp8 == 2 && c->xkv8 && c->xkv8_scale && c->lowp;
  c->sess = S.release();
  return TTASR_OK;
}

// ---- beam mode ----

static int session_begin_beam(ttasr_ctx* c, const ttasr_gen_opts* o, int max_prompt, int beam, float patience) {
  if (!c) return TTASR_E_INVALID;
  if (!c->finalized) return fail(c, TTASR_E_INVALID, "weights not finalized (call ttasr_finalize_weights first)");
  TRY(session_refusal(c));
  if (beam < 1 || beam > 7) return fail(c, TTASR_E_INVALID, "beam %d outside [1, 7]", beam);
  if (c->maxB < beam) return fail(c, TTASR_E_INVALID, "max_batch %d holds no group of %d rows", c->maxB, beam);
  if (!(patience > 0.f)) return fail(c, TTASR_E_INVALID, "patience %g must be > 0", patience);
  // rules, buffers, streams; every row free (done = 1).  Group g reads cross-KV slot g; rows read their own (shared) page lists
  TRY(session_begin(c, o, max_prompt, 0.f, StepShape{beam, 0, true}));
  Session* S = c->sess;
  const int G = c->maxB / beam, R = G * beam;
  S->beam = beam; S->G = G; S->max_cand = std::max(1, (int)std::lround(beam * patience)); S->patience = patience;
  S->grp.assign(G, Session::Group{});
  S->seqs.assign(R, {}); S->sums.assign(R, 0.0); S->fsums.assign(R, 0.f);
  S->pages.reset(R, c->pages_per_seq, c->maxB * c->pages_per_seq);
  S->cur_tok.assign(R, 0); S->done_rows.assign(R, 1);
  BeamExchange x;
  if (beam_exchange(c, R, beam + 1, x) != 0) { session_free(c); c->xkv8_valid = false; return TTASR_E_HIP; }   // the steps' pinned block exists from here on
  if (!c->sess_sel && dalloc(c, &c->sess_sel, (size_t)c->maxB * 9 * 4) != 0) { session_free(c); c->xkv8_valid = false; return TTASR_E_HIP; }
  return TTASR_OK;
}

// the language result of row r from the pinned copy of the device block's result part (winners | probs | logits, rows at n_lang)
static void session_lang_result(const Session* S, int B, int r, Session::Lang& out) {
  const int32_t* best = S->lang_pin + 3 * B;
  const float* probs = (const float*)(best + B) + (size_t)r * S->lang_n;
  const float* logits = (const float*)(best + B) + (size_t)B * 128 + (size_t)r * S->lang_n;
  out.idx = std::min(std::max(best[r], 0), S->lang_n - 1);
  out.probs.assign(probs, probs + S->lang_n);
  out.logits.assign(logits, logits + S->lang_n);
}

// One decode position of every live group: copy-on-write, one staged upload, the logits-only step over R rows, the candidate
// kernel (BEAM groups) and the independent-row kernel (ROWS groups), ONE synchronisation, then selection, re-indexing and the
// finished groups' results on the host.
static int beam_step(ttasr_ctx* c, Session* S) {
  const int beam = S->beam, G = S->G, R = G * beam, pps = c->pages_per_seq, K = beam + 1;
  const ttasr_gen_opts& o = S->o;
  hipStream_t s = c->stream;
  // 1. the page each live row writes must exist and be private to the row.  The pool should never run dry: a row holds at most
  // pps pages (positions < n_text_ctx), at most maxB rows hold pages, the pool has maxB * pps, and a page is back on the free
  // list as soon as no row references it (a finished group drops its rows' lists).
  S->pairs.clear();
  bool any_sampling = false, any_ns = false;
  int n_detect = 0;   // groups whose step this is the detect step
  for (int g = 0; g < G; ++g) {
    const Session::Group& gr = S->grp[g];
    if (gr.clip < 0) continue;
    for (int b = 0; b < beam; ++b)
      if (!S->pages.make_private(g * beam + b, gr.pos, S->pairs)) return fail(c, TTASR_E_NOMEM, "KV page pool exhausted");
    n_detect += gr.det >= 0;
    if (gr.mode != Session::BEAM || gr.det >= 0) continue;   // a detecting group takes no part in the candidate or no-speech work
    any_sampling |= gr.pos + 1 >= (int)gr.prompt.size();
    any_ns |= o.no_speech >= 0 && gr.pos == gr.sot;
  }
  // 2. the step's input, staged in the pinned block
  BeamExchange x;
  TRY(beam_exchange(c, R, K, x));
  // the rows of ROWS groups that need the independent-row kernel: past their prompt and not finished (choose), or the first row
  // at the group's <|startoftranscript|> position (no-speech)
  int n_ent = 0;
  for (int g = 0; g < G; ++g) {
    const Session::Group& gr = S->grp[g];
    if (gr.clip < 0 || gr.mode != Session::ROWS || gr.det >= 0) continue;
    const bool past = gr.pos + 1 >= (int)gr.prompt.size(), ns_here = o.no_speech >= 0 && gr.pos == gr.sot;
    for (int b = 0; b < gr.rows; ++b) {
      const int r = g * beam + b;
      const int flags = (past && !S->done_rows[r] ? 1 : 0) | (ns_here && b == 0 ? 2 : 0);
      if (!flags) continue;
      int32_t* e = x.ent + 4 * n_ent;
      e[0] = r; e[1] = gr.pos; e[2] = b; e[3] = flags;
      x.temp[n_ent] = gr.temp; x.seed[n_ent] = gr.seed;
      ++n_ent;
    }
  }
  S->pages.write_upload(x.tbl);
  for (int r = 0; r < R; ++r) {
    const Session::Group& gr = S->grp[r / beam];
    x.tok[r] = S->cur_tok[r]; x.pos[r] = gr.clip < 0 ? 0 : gr.pos; x.done[r] = S->done_rows[r];
  }
  HIPCHK(c, hipMemcpyAsync(c->page_table, x.tbl, (size_t)R * pps * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->st.cur_tok, x.tok, (size_t)R * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->row_pos, x.pos, (size_t)R * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->st.done, x.done, (size_t)R * 4, hipMemcpyHostToDevice, s));
  TRY(enqueue_page_copies(c, S->pairs, x));
  const bool topk = any_sampling || any_ns;
  if (topk || n_ent > 0) TRY(enqueue_row_histories(c, S->seqs, R, o.timestamp_begin, x));
  // device layout of the independent-row block (c->sess_sel): entries [4 R] | temperatures [R] | seeds [R] | results [3 R]
  int32_t* const d_ent = c->sess_sel;
  float* const d_out = (float*)(d_ent + 6 * R);
  if (n_ent > 0) {   // entries, temperatures and seeds are contiguous in both blocks: one copy
    memmove(x.ent + 4 * n_ent, x.temp, (size_t)n_ent * 4);
    memmove(x.ent + 5 * n_ent, x.seed, (size_t)n_ent * 4);
    HIPCHK(c, hipMemcpyAsync(d_ent, x.ent, (size_t)6 * n_ent * 4, hipMemcpyHostToDevice, s));
  }
  // 3. the decoder step (logits only) and, behind it, the candidates of every row and the choices of the independent rows
  HIPCHK(c, hipEventRecord(S->ev_dec0, s));
  TRY(step_graph(c, R, 1));
  if (topk) TRY(enqueue_candidates(c, R, K, any_ns, x));
  if (n_ent > 0) {
    const SessRowsArgs sa{d_ent, (const float*)(d_ent + 4 * n_ent), (const uint32_t*)(d_ent + 5 * n_ent), d_out};
    launch_session_rows_select(c->logits, beam_row_state(c, R), c->rp, sa, n_ent, s);
    HIPCHK(c, hipMemcpyAsync(x.sel, d_out, (size_t)3 * n_ent * 4, hipMemcpyDeviceToHost, s));
  }
  if (n_detect > 0) {   // the language head for the first row of every detecting group; results back with the step's synchronisation
    const int B = c->maxB;
    int32_t* const ls = c->lang_sess;
    int32_t* const flags = S->lang_pin + 2 * B;
    for (int r = 0; r < R; ++r) flags[r] = r % beam == 0 && S->grp[r / beam].clip >= 0 && S->grp[r / beam].det >= 0;
    HIPCHK(c, hipMemcpyAsync(ls, flags, (size_t)R * 4, hipMemcpyHostToDevice, s));
    const LangRows a{ls, nullptr, nullptr, 0, nullptr, nullptr, ls + 4 * B, (float*)(ls + 5 * B), (float*)(ls + 5 * B) + (size_t)B * 128};
    TT_DISPATCH(c, launch_lang_head_rows<T>((const T*)c->dh, (const T*)c->emb, R, c->d, c->V, S->lang_begin, S->lang_n, a, s));
    HIPCHK(c, hipMemcpyAsync(S->lang_pin + 3 * B, ls + 4 * B, (size_t)B * 257 * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipEventRecord(S->ev_dec1, s));
  HIPCHK(c, hipStreamSynchronize(s));   // the one synchronisation of the step
  HIPCHK(c, hipGetLastError());
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, S->ev_dec0, S->ev_dec1) == hipSuccess) S->dec_ms += ms;
  // 4. selection per searching BEAM group (the code beam_search_impl runs), re-index; ROWS groups keep their rows
  std::vector<std::vector<int>> nseq; std::vector<double> nsum; std::vector<int> src;
  std::vector<char> searching(G, 0);
  for (int g = 0; g < G; ++g) {
    Session::Group& gr = S->grp[g];
    searching[g] = gr.clip >= 0 && gr.det < 0 && gr.pos + 1 >= (int)gr.prompt.size();
    const bool beam_search = searching[g] && gr.mode == Session::BEAM;
    if (gr.clip >= 0 && gr.det < 0 && gr.mode == Session::BEAM && any_ns && gr.pos == gr.sot) gr.ns = x.ns[g * beam];
    int b0 = 0;
    if (beam_search) {
      if (!beam_select(S->seqs, S->sums, g * beam, gr.rows, gr.rows + 1, x.lp, x.id, o.eot, gr.max_cand, gr.finished, nseq, nsum, src, K))
        return fail(c, TTASR_E_INVALID, "beam search: no live candidate (every token masked)");
      b0 = gr.rows;
    }
    for (int b = b0; b < beam; ++b) { const int r = g * beam + b; nseq.push_back(S->seqs[r]); nsum.push_back(S->sums[r]); src.push_back(r); }
  }
  S->pages.reindex(src);
  S->seqs.swap(nseq); S->sums.swap(nsum);
  // the independent rows' choices: the token, the f32 sum in the order select_body adds, EOT or the budget end the row
  std::vector<int> live_rows(G, 0);
  for (int g = 0; g < G; ++g)
    for (int b = 0; b < beam; ++b) live_rows[g] += !S->done_rows[g * beam + b];
  for (int e = 0; e < n_ent; ++e) {
    const int32_t* en = x.ent + 4 * e;   // (the temperatures and seeds moved behind the entries; the entries stayed)
    const int r = en[0];
    Session::Group& gr = S->grp[r / beam];
    if (en[3] & 2) gr.ns = x.sel[3 * e + 2];
    if (!(en[3] & 1)) continue;
    int choice;
    memcpy(&choice, &x.sel[3 * e], 4);
    // a range guard only: the kernel answers a row with nothing selectable itself (EOT, increment -inf), so no id outside the
    // vocabulary is expected here any more
    if (choice < 0 || choice >= c->V) return fail(c, TTASR_E_INVALID, "session row %d: token %d outside the vocabulary", r, choice);
    S->seqs[r].push_back(choice);
    S->fsums[r] += x.sel[3 * e + 1];
    if (choice == o.eot || (int)S->seqs[r].size() >= gr.cap) S->done_rows[r] = 1;
  }
  for (int g = 0; g < G; ++g) {
    Session::Group& gr = S->grp[g];
    if (gr.clip < 0) continue;
    S->live_row_steps += live_rows[g];
    const int r0 = g * beam;
    if (gr.det >= 0) {   // the detect step: the winner's token replaces the placeholder, the group starts over at position 0
      session_lang_result(S, c->maxB, r0, gr.lang);
      gr.prompt[gr.det] = S->lang_begin + gr.lang.idx;
      gr.det = -1;
      for (int b = 0; b < beam; ++b) S->cur_tok[r0 + b] = S->done_rows[r0 + b] ? o.eot : gr.prompt[0];
      continue;
    }
    gr.pos++;
    bool ended = false;
    if (searching[g] && gr.mode == Session::BEAM) ended = (int)gr.finished.size() >= gr.max_cand || (int)S->seqs[r0].size() >= gr.cap;
    if (searching[g] && gr.mode == Session::ROWS) {
      ended = true;
      for (int b = 0; b < gr.rows; ++b) ended &= S->done_rows[r0 + b] != 0;
    }
    if (ended) {
      Session::Done d;
      d.id = gr.clip;
      if (gr.mode == Session::BEAM) {
        d.tok.resize(c->rp.max_new);
        double best = 0;
        d.tok.resize(beam_pick(gr.finished, S->seqs, S->sums, r0, gr.rows, o.eot, c->rp.max_new, d.tok.data(), &best));
        d.lp = (float)best;
      } else {   // ttasr_generate_sample's pick and tokens (EOT kept)
        std::vector<int32_t> lens(gr.rows);
        for (int b = 0; b < gr.rows; ++b) lens[b] = (int32_t)S->seqs[r0 + b].size();
        const int best = sample_pick(&S->fsums[r0], lens.data(), gr.rows);
        const std::vector<int>& w = S->seqs[r0 + best];
        d.tok.assign(w.begin(), w.begin() + std::min<size_t>(w.size(), (size_t)c->rp.max_new));
        d.lp = S->fsums[r0 + best];
      }
      d.ns = gr.ns;
      d.lang = std::move(gr.lang);
      S->finished.push_back(std::move(d));
      // the group is free: its page lists go back to the pool, its rows leave the attention kernels
      // (hold mode: the pages go back, the group and its cross-KV slot stay with the clip until it is aligned or released)
      if (S->hold) gr.held = gr.clip;
      gr.clip = -1; gr.finished.clear();
      for (int b = 0; b < beam; ++b) {
        const int r = r0 + b;
        S->pages.drop_row(r);
        S->done_rows[r] = 1; S->row_clip[r] = S->hold ? gr.held : -1; S->cur_tok[r] = 0;
      }
      continue;
    }
    for (int b = 0; b < beam; ++b) {
      const int r = r0 + b;
      S->cur_tok[r] = S->done_rows[r] ? o.eot : (searching[g] ? S->seqs[r].back() : gr.prompt[gr.pos]);
    }
  }
  return 0;
}

// What both submit calls build alike of clip i: its prompt (checked, with the sot index where no-speech is wanted) and its budget.
// A call validates and builds ALL its clips before queue_clips gives them ids: a refused call leaves the session as it was.
static int init_clip(ttasr_ctx* c, const Session* S, int i, const int32_t* prompt, const int32_t* prompt_len, const int32_t* sot,
                     const int32_t* max_new, Session::Clip& cl) {
  const int32_t* row = prompt + (size_t)i * S->max_prompt;
  const int len = prompt_len[i];
  std::vector<int32_t> checked;   // armed session: the prompt with a valid token in the placeholder's place
  if (S->armed && len >= 1 && len <= S->max_prompt) {
    for (int j = 0; j < len; ++j) {
      if (row[j] != TTASR_TOKEN_DETECT) continue;
      if (cl.det >= 0) return fail(c, TTASR_E_INVALID, "clip %d: two language placeholders (at %d and %d)", i, cl.det, j);
      if (j == 0 || row[j - 1] != S->lang_sot)
        return fail(c, TTASR_E_INVALID, "clip %d: the language placeholder at %d is not directly behind token %d (sot)", i, j, S->lang_sot);
      cl.det = j;
    }
    if (cl.det >= 0) { checked.assign(row, row + len); checked[cl.det] = S->lang_begin; }
  }
  TRY(check_prompt(c, i, cl.det >= 0 ? checked.data() : row, len, S->max_prompt, sot));
  if (max_new[i] < 1 || max_new[i] > S->o.max_new_tokens)
    return fail(c, TTASR_E_INVALID, "clip %d: max_new %d outside [1, max_new_tokens=%d]", i, max_new[i], S->o.max_new_tokens);
  cl.prompt.assign(row, row + prompt_len[i]);
  cl.cap = max_new[i];
  return 0;
}

static void queue_clips(Session* S, std::vector<Session::Clip>& cls, int64_t* out_ids) {
  for (size_t i = 0; i < cls.size(); ++i) {
    cls[i].id = S->next_id++;
    if (out_ids) out_ids[i] = cls[i].id;
    S->queue.push_back(std::move(cls[i]));
  }
}

static int session_submit(ttasr_ctx* c, int n, const float* const* pcm, const int64_t* n_samples, const int32_t* prompt,
                          const int32_t* prompt_len, const int32_t* max_new, int64_t* out_ids) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  if (n < 1) return fail(c, TTASR_E_INVALID, "n %d < 1", n);
  if (!pcm || !n_samples || !prompt || !prompt_len || !max_new) return fail(c, TTASR_E_INVALID, "NULL argument");
  std::vector<Session::Clip> cls(n);
  for (int i = 0; i < n; ++i) {
    if (n_samples[i] < 0 || n_samples[i] > c->n_samples)
      return fail(c, TTASR_E_INVALID, "clip %d: %lld samples outside [0, %d] (one window)", i, (long long)n_samples[i], c->n_samples);
    if (n_samples[i] > 0 && !pcm[i]) return fail(c, TTASR_E_INVALID, "clip %d: pcm is NULL", i);
    Session::Clip& cl = cls[i];
    TRY(init_clip(c, S, i, prompt, prompt_len, S->beam && S->o.no_speech >= 0 ? &S->o.sot_index : nullptr, max_new, cl));
    cl.pcm.assign(pcm[i], pcm[i] + n_samples[i]);
    cl.mode = Session::BEAM; cl.rows = S->beam; cl.sot = S->o.sot_index;
  }
  queue_clips(S, cls, out_ids);
  return TTASR_OK;
}

// Window clips (beam session only): window i = 30 s of file_pcm[i] from frame seek_frames[i], with its own prompt, sot index,
// budget, temperature, rows and seed.  Only the samples the window's STFT reads are copied (ttasr_log_mel_windows' span).
static int session_submit_windows(ttasr_ctx* c, int n, const float* const* file_pcm, const int64_t* file_samples, const int64_t* seek_frames,
                                  const float* floor_max, const int32_t* prompt, const int32_t* prompt_len, const int32_t* sot_index,
                                  const int32_t* max_new, const float* temperature, const int32_t* rows, const uint32_t* seed,
                                  int64_t* out_ids) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin_beam first)");
  if (!S->beam) return fail(c, TTASR_E_INVALID, "window clips need a session opened with ttasr_session_begin_beam");
  if (n < 1) return fail(c, TTASR_E_INVALID, "n %d < 1", n);
  if (!file_pcm || !file_samples || !seek_frames || !prompt || !prompt_len || !sot_index || !max_new || !rows || !seed)
    return fail(c, TTASR_E_INVALID, "NULL argument");
  std::vector<Session::Clip> cls(n);
  for (int i = 0; i < n; ++i) {
    if (file_samples[i] < 0) return fail(c, TTASR_E_INVALID, "window %d: negative file length", i);
    if (file_samples[i] > 0 && !file_pcm[i]) return fail(c, TTASR_E_INVALID, "window %d: pcm is NULL", i);
    if (seek_frames[i] < 0 || seek_frames[i] >= (file_samples[i] + 159) / 160)
      return fail(c, TTASR_E_INVALID, "window %d: seek %lld at or beyond the file (%lld samples)", i, (long long)seek_frames[i],
                  (long long)file_samples[i]);
    if (floor_max && !std::isfinite(floor_max[i])) return fail(c, TTASR_E_INVALID, "window %d: floor_max is not finite", i);
    if (rows[i] < 1 || rows[i] > S->beam) return fail(c, TTASR_E_INVALID, "window %d: rows %d outside [1, %d]", i, rows[i], S->beam);
    if (temperature && !(std::isfinite(temperature[i]) && temperature[i] >= 0.f))
      return fail(c, TTASR_E_INVALID, "window %d: temperature %g must be finite and >= 0", i, temperature[i]);
    Session::Clip& cl = cls[i];
    TRY(init_clip(c, S, i, prompt, prompt_len, S->o.no_speech >= 0 ? &sot_index[i] : nullptr, max_new, cl));
    const WindowSpan w = window_span(c, file_samples[i], seek_frames[i]);   // the span and geometry of ttasr_log_mel_windows
    cl.pcm.assign(file_pcm[i] + w.first, file_pcm[i] + w.first + w.n);
    cl.win = true;
    memcpy(cl.geom, w.geom, sizeof w.geom);
    if (floor_max) { cl.has_floor = true; cl.floor = mel_max_to_ordered(floor_max[i]); }
    cl.sot = sot_index[i];
    cl.temp = temperature ? temperature[i] : 0.f;
    cl.rows = rows[i];
    cl.seed = seed[i];
    cl.mode = (cl.temp == 0.f && cl.rows > 1) ? Session::BEAM : Session::ROWS;
  }
  queue_clips(S, cls, out_ids);
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

// ttasr_session_poll and ttasr_session_poll_lang: the plain poll passes no language outputs and drops what was detected
static int session_poll(ttasr_ctx* c, int max_steps, int cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp,
                        float* no_speech, int32_t* n_out, int32_t* lang = nullptr, float* lang_probs = nullptr,
                        float* lang_logits = nullptr) {
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
    const int live = n_units(c, S) - n_free_units(S) - n_held_units(S);
    if (live == 0) {
      if (S->enc_pending) {   // nothing to decode until the encode is done
        HIPCHK(c, hipEventSynchronize(S->ev_enc));
        S->enc_pending = false;
        continue;
      }
      if (S->staged.empty() && S->queue.empty()) break;   // nothing left
      if (n_free_units(S) == 0) break;   // every unit is held: the host has to align or release before a queued clip can start
      continue;
    }
    if (steps >= max_steps) break;
    if (S->beam) {   // selection is on the host: one step per exchange
      TRY(beam_step(c, S));
      steps++; S->steps++; S->polls++;
      continue;
    }
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
    bool lang_back = false;   // rows whose detect step has run since the last exchange: their results ride along
    for (int r = 0; r < B && S->armed; ++r) lang_back |= S->row_clip[r] >= 0 && S->row_det[r] == 1;
    if (lang_back) HIPCHK(c, hipMemcpyAsync(S->lang_pin + 3 * B, c->lang_sess + 4 * B, (size_t)B * 257 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, S->ev_dec0, S->ev_dec1) == hipSuccess) S->dec_ms += ms;
    for (int r = 0; r < B && lang_back; ++r)
      if (S->row_clip[r] >= 0 && S->row_det[r] == 1) { session_lang_result(S, B, r, S->row_lang[r]); S->row_det[r] = 2; }
    for (int r = 0; r < B; ++r) {
      if (S->row_clip[r] < 0 || !p[r] || S->held[r]) continue;
      Session::Done d;
      d.id = S->row_clip[r];
      const int len = std::min(p[B + r], max_new);
      d.tok.assign(p + 4 * B + (size_t)r * max_new, p + 4 * B + (size_t)r * max_new + len);
      memcpy(&d.lp, &p[2 * B + r], 4); memcpy(&d.ns, &p[3 * B + r], 4);
      S->live_row_steps += S->row_plen[r] - 1 - S->row_start[r] + len;   // prefilled positions ran no step
      if (S->armed) {   // a detected clip ran one more live row-step
        S->live_row_steps += S->row_det[r] != 0;
        d.lang = std::move(S->row_lang[r]); S->row_det[r] = 0; S->row_lang[r] = Session::Lang{};
      }
      S->finished.push_back(std::move(d));
      if (S->hold) S->held[r] = 1; else S->row_clip[r] = -1;
    }
  }
  int k = 0;
  while (k < cap && !S->finished.empty()) {
    const Session::Done& d = S->finished.front();
    ids[k] = d.id; lens[k] = (int32_t)d.tok.size();
    memcpy(tokens + (size_t)k * max_new, d.tok.data(), d.tok.size() * 4);
    if (sum_lp) sum_lp[k] = d.lp;
    if (no_speech) no_speech[k] = d.ns;
    if (lang) lang[k] = d.lang.idx;
    if (d.lang.idx >= 0 && lang_probs) memcpy(lang_probs + (size_t)k * S->lang_n, d.lang.probs.data(), (size_t)S->lang_n * 4);
    if (d.lang.idx >= 0 && lang_logits) memcpy(lang_logits + (size_t)k * S->lang_n, d.lang.logits.data(), (size_t)S->lang_n * 4);
    S->finished.pop_front();
    ++k;
  }
  *n_out = k;
  return TTASR_OK;
}

// ---- language detection inside the session ----

static int session_detect_language(ttasr_ctx* c, int sot, int lang_begin, int n_lang) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  if (S->armed) return fail(c, TTASR_E_INVALID, "the session is armed for language detection already");
  if (S->next_id > 0) return fail(c, TTASR_E_INVALID, "language detection is armed before the first submit of a session");
  if (sot < 0 || sot >= c->V) return fail(c, TTASR_E_INVALID, "sot %d outside the vocabulary (%d)", sot, c->V);
  if (n_lang < 1 || n_lang > 128) return fail(c, TTASR_E_INVALID, "n_lang %d outside [1, 128]", n_lang);
  if (lang_begin < 0 || lang_begin > c->V - n_lang)
    return fail(c, TTASR_E_INVALID, "language span [%d, %d) outside the vocabulary (%d)", lang_begin, lang_begin + n_lang, c->V);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->maxB;
  if (!c->lang_sess) TRY(dalloc(c, &c->lang_sess, (size_t)B * 261 * 4));
  TRY(S->lang_pin.ensure(c, (size_t)B * 260 * 4, "session language block"));
  // a session that ended between a clip's admission and its detect step left a flag up
  HIPCHK(c, hipMemsetAsync(c->lang_sess, 0, (size_t)B * 4, c->stream));
  if (c->sess_lang_begin != lang_begin || c->sess_lang_n != n_lang || c->sess_lang_stride != S->max_prompt) drop_lang_graphs(c);
  c->sess_lang_begin = lang_begin; c->sess_lang_n = n_lang; c->sess_lang_stride = S->max_prompt;
  S->lang_sot = sot; S->lang_begin = lang_begin; S->lang_n = n_lang;
  S->row_det.assign(B, 0); S->row_lang.assign(B, Session::Lang{});
  // greedy: the head is part of every step from here on (its graphs are keyed on the flag); beam: launched by beam_step
  if (!S->beam) S->scope->set_lang_rows(true);
  S->armed = true;
  return TTASR_OK;
}

// ---- hold mode: finished clips keep their unit until the host has aligned or released them ----

// unit (greedy: row, beam: group) that holds clip `id`, or -1
static int held_unit(const Session* S, int64_t id) {
  if (S->beam) { for (int g = 0; g < S->G; ++g) if (S->grp[g].held == id) return g; }
  else for (size_t r = 0; r < S->held.size(); ++r) if (S->held[r] && S->row_clip[r] == id) return (int)r;
  return -1;
}

static void release_unit(Session* S, int u) {
  if (S->beam) {
    S->grp[u].held = -1;
    for (int b = 0; b < S->beam; ++b) S->row_clip[(size_t)u * S->beam + b] = -1;
  } else {
    S->held[u] = 0; S->row_clip[u] = -1;
  }
}

static int session_hold(ttasr_ctx* c, int on) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  // the alignment pass borrows the encoder's activation workspaces, which an overlapped encode writes from the second stream
  if (on && S->overlap) return fail(c, TTASR_E_INVALID, "hold mode is not available with option refill_overlap = 1");
  S->hold = on != 0;
  if (!S->hold) {   // nothing stays held that could no longer be released
    for (int u = 0; u < (S->beam ? S->G : c->maxB); ++u)
      if (S->beam ? S->grp[u].held >= 0 : S->held[u] != 0) release_unit(S, u);
  }
  return TTASR_OK;
}

// ids -> units; every id must be a held clip and appear once.  Nothing is changed.
static int held_units(ttasr_ctx* c, Session* S, int n, const int64_t* ids, std::vector<int>& units) {
  if (!S->hold) return fail(c, TTASR_E_INVALID, "hold mode is off (ttasr_session_hold first)");
  if (n < 1 || n > c->maxB || !ids) return fail(c, TTASR_E_INVALID, "n %d outside [1, max_batch = %d] or ids NULL", n, c->maxB);
  units.assign(n, -1);
  for (int i = 0; i < n; ++i) {
    units[i] = held_unit(S, ids[i]);
    if (units[i] < 0) return fail(c, TTASR_E_INVALID, "clip %lld is not held", (long long)ids[i]);
    for (int j = 0; j < i; ++j) if (ids[j] == ids[i]) return fail(c, TTASR_E_INVALID, "clip %lld listed twice", (long long)ids[i]);
  }
  return 0;
}

static int session_release(ttasr_ctx* c, int n, const int64_t* ids) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  std::vector<int> units;
  TRY(held_units(c, S, n, ids, units));
  for (int u : units) release_unit(S, u);
  return TTASR_OK;
}

// A new search on held clips (beam session): clip ids[i]'s group starts over at the next step under a new clip id, with its own
// prompt, budget, temperature, rows and seed, exactly as admit() starts a staged clip - but the group's cross-KV slot (and its
// e4m3 block and scales) is the one the held clip's encoder pass filled, so no mel, encoder, copy or quantiser work is enqueued.
// Only the admission pass of option session_prefill runs, for the retried clips whose prompts qualify, as at admission.
// Everything is validated before anything changes.
static int session_retry(ttasr_ctx* c, int n, const int64_t* ids, const int32_t* prompt, const int32_t* prompt_len,
                         const int32_t* sot_index, const int32_t* max_new, const float* temperature, const int32_t* rows,
                         const uint32_t* seed, int64_t* out_ids) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin_beam first)");
  if (!S->beam) return fail(c, TTASR_E_INVALID, "a retry needs a session opened with ttasr_session_begin_beam");
  std::vector<int> units;
  TRY(held_units(c, S, n, ids, units));
  if (!prompt || !prompt_len || !sot_index || !max_new || !rows || !seed) return fail(c, TTASR_E_INVALID, "NULL argument");
  std::vector<Session::Clip> cls(n);
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 1 || rows[i] > S->beam) return fail(c, TTASR_E_INVALID, "retry %d: rows %d outside [1, %d]", i, rows[i], S->beam);
    if (temperature && !(std::isfinite(temperature[i]) && temperature[i] >= 0.f))
      return fail(c, TTASR_E_INVALID, "retry %d: temperature %g must be finite and >= 0", i, temperature[i]);
    Session::Clip& cl = cls[i];
    TRY(init_clip(c, S, i, prompt, prompt_len, S->o.no_speech >= 0 ? &sot_index[i] : nullptr, max_new, cl));
    if (cl.det >= 0) return fail(c, TTASR_E_INVALID, "retry %d: a retried clip's language is known (placeholder at %d)", i, cl.det);
    cl.sot = sot_index[i];
    cl.temp = temperature ? temperature[i] : 0.f;
    cl.rows = rows[i];
    cl.seed = seed[i];
    cl.mode = (cl.temp == 0.f && cl.rows > 1) ? Session::BEAM : Session::ROWS;
  }
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<PrefillSeq> pf_seq;
  std::vector<std::vector<int32_t>> pf_pages;
  for (int i = 0; i < n; ++i) {
    cls[i].id = S->next_id++;
    if (out_ids) out_ids[i] = cls[i].id;
    S->grp[units[i]].held = -1;
    start_group(c, S, units[i], cls[i], pf_seq, pf_pages);
  }
  for (size_t i = 0; i < pf_seq.size(); ++i) pf_seq[i].pages = pf_pages[i].data();   // (pf_pages no longer grows)
  TRY(run_prefill_passes(c, S, pf_seq));
  return TTASR_OK;
}

// The batched alignment pass (engine_align.hip) over held clips: sequence i reads the cross-KV slot of clip ids[i]'s unit and
// keeps its self-attention K/V in pages no live row uses - the held row's own (greedy: a row owns its pages for good) or free
// pool pages (beam: a finished group's page lists are back in the pool, and a held group accounts for beam x pages_per_seq of
// them).  The pass runs between two decode steps on the decode stream; the clips are released when it has succeeded.
static int session_align(ttasr_ctx* c, int n, const int64_t* ids, const AlignBatch& a) {
  if (!c) return TTASR_E_INVALID;
  Session* S = c->sess;
  if (!S) return fail(c, TTASR_E_INVALID, "no session is open (ttasr_session_begin first)");
  std::vector<int> units;
  TRY(held_units(c, S, n, ids, units));
  TRY(align_batch_validate(c, a));
  HIPCHK(c, hipSetDevice(c->device));
  const int pps = c->pages_per_seq;
  std::vector<int32_t> slot(units.begin(), units.end()), pages((size_t)n * pps);
  if (S->beam) {
    const int32_t* spare = S->pages.peek_free(pages.size());
    if (!spare) return fail(c, TTASR_E_INVALID, "session align: %zu free pages, %zu needed", S->pages.free_pages.size(), pages.size());
    std::copy_n(spare, pages.size(), pages.begin());
  } else {
    for (int i = 0; i < n; ++i)
      for (int p = 0; p < pps; ++p) pages[(size_t)i * pps + p] = units[i] * pps + p;
  }
  // option align_packed, read here: the packed pass, whose bits for a clip do not depend on the other clips of the call
  TRY(c->align_packed ? align_packed_run(c, a, slot.data(), pages.data()) : align_batch_run(c, a, slot.data(), pages.data()));
  for (int u : units) release_unit(S, u);
  return TTASR_OK;
}

static int session_end(ttasr_ctx* c) {
  if (!c) return TTASR_E_INVALID;
  if (!c->sess) return fail(c, TTASR_E_INVALID, "no session is open");
  session_free(c);   // the session's scope ends: default decode shape, the rows' finished flags cleared (as after every search)
  hipMemsetAsync(c->st.n_done, 0, 16, c->stream);
  const hipError_t e = hipStreamSynchronize(c->stream);
  c->B_mel = c->B_enc = c->B_dec = 0;
  c->xkv8_valid = false;   // like the rest of the resident encoder state: rebuilt by the next encode
  if (e != hipSuccess) return fail(c, TTASR_E_HIP, "session end: %s", hipGetErrorString(e));
  return TTASR_OK;
}

}  // namespace ttasr_detail

// ---- C ABI (include/ttasr.h) ----
extern "C" {

int ttasr_session_begin(ttasr_ctx* c, const ttasr_gen_opts* o, int32_t max_prompt, float temperature) {
  return guarded(c, [&]() -> int { return session_begin(c, o, max_prompt, temperature, StepShape{1, 1, true}); });
}

int ttasr_session_begin_beam(ttasr_ctx* c, const ttasr_gen_opts* o, int32_t max_prompt, int32_t beam, float patience) {
  return guarded(c, [&]() -> int { return session_begin_beam(c, o, max_prompt, beam, patience); });
}

int ttasr_session_submit(ttasr_ctx* c, int32_t n, const float* const* pcm_host, const int64_t* n_samples, const int32_t* prompt,
                         const int32_t* prompt_len, const int32_t* max_new, int64_t* out_ids) {
  return guarded(c, [&]() -> int { return session_submit(c, n, pcm_host, n_samples, prompt, prompt_len, max_new, out_ids); });
}

int ttasr_session_submit_windows(ttasr_ctx* c, int32_t n, const float* const* file_pcm, const int64_t* file_samples,
                                 const int64_t* seek_frames, const float* floor_max, const int32_t* prompt, const int32_t* prompt_len,
                                 const int32_t* sot_index, const int32_t* max_new, const float* temperature, const int32_t* rows,
                                 const uint32_t* seed, int64_t* out_ids) {
  return guarded(c, [&]() -> int {
    return session_submit_windows(c, n, file_pcm, file_samples, seek_frames, floor_max, prompt, prompt_len, sot_index, max_new,
                                  temperature, rows, seed, out_ids);
  });
}

int ttasr_session_poll(ttasr_ctx* c, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp,
                       float* no_speech, int32_t* n_out) {
  return guarded(c, [&]() -> int { return session_poll(c, max_steps, cap, ids, tokens, lens, sum_lp, no_speech, n_out); });
}

int ttasr_session_poll_lang(ttasr_ctx* c, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp,
                            float* no_speech, int32_t* lang, float* lang_probs, float* lang_logits, int32_t* n_out) {
  return guarded(c, [&]() -> int {
    if (c && c->sess && !lang) return fail(c, TTASR_E_INVALID, "lang is NULL");
    return session_poll(c, max_steps, cap, ids, tokens, lens, sum_lp, no_speech, n_out, lang, lang_probs, lang_logits);
  });
}

int ttasr_session_detect_language(ttasr_ctx* c, int32_t sot, int32_t lang_begin, int32_t n_lang) {
  return guarded(c, [&]() -> int { return session_detect_language(c, sot, lang_begin, n_lang); });
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

int ttasr_session_prefill_stats(ttasr_ctx* c, double out[4]) {
  return guarded(c, [&]() -> int {
    if (!c) return TTASR_E_INVALID;
    if (!out) return fail(c, TTASR_E_INVALID, "out is NULL");
    Session* S = c->sess;
    if (!S) return fail(c, TTASR_E_INVALID, "no session is open");
    HIPCHK(c, hipSetDevice(c->device));
    TRY(prefill_collect(c, S));
    const double v[4] = {(double)S->pf_passes, (double)S->pf_clips, (double)S->pf_positions, S->pf_ms};
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
    if (S->beam) {   // positions and flags are the host's: every row of a group reports the group's position
      for (int r = 0; r < c->maxB; ++r) {
        const bool in = r < S->G * S->beam;
        const Session::Group* g = in ? &S->grp[r / S->beam] : nullptr;
        if (row_pos) row_pos[r] = g && g->clip >= 0 ? g->pos : 0;
        if (done) done[r] = in ? S->done_rows[r] : 1;
      }
      if (row_clip) memcpy(row_clip, S->row_clip.data(), (size_t)c->maxB * 8);
      return TTASR_OK;
    }
    if (row_pos) HIPCHK(c, hipMemcpy(row_pos, c->row_pos, (size_t)c->maxB * 4, hipMemcpyDeviceToHost));
    if (done) HIPCHK(c, hipMemcpy(done, c->st.done, (size_t)c->maxB * 4, hipMemcpyDeviceToHost));
    if (row_clip) memcpy(row_clip, S->row_clip.data(), (size_t)c->maxB * 8);
    return TTASR_OK;
  });
}

int ttasr_session_hold(ttasr_ctx* c, int32_t on) {
  return guarded(c, [&]() -> int { return session_hold(c, on); });
}

int ttasr_session_align(ttasr_ctx* c, int32_t n, const int64_t* ids, const int32_t* tokens, const int32_t* n_tokens, int32_t max_tokens,
                        const int32_t* first_row, const int32_t* num_frames, const int32_t* pairs, int32_t n_pairs, int32_t medfilt_width,
                        int32_t* out_start_frame, float* out_logprob, float* out_cost, float* out_weights) {
  return guarded(c, [&]() -> int {
    const AlignBatch a{n, tokens, n_tokens, max_tokens, first_row, num_frames, pairs, n_pairs, medfilt_width,
                       out_start_frame, out_logprob, out_cost, out_weights};
    return session_align(c, n, ids, a);
  });
}

int ttasr_session_release(ttasr_ctx* c, int32_t n, const int64_t* ids) {
  return guarded(c, [&]() -> int { return session_release(c, n, ids); });
}

int ttasr_session_retry(ttasr_ctx* c, int32_t n, const int64_t* ids, const int32_t* prompt, const int32_t* prompt_len,
                        const int32_t* sot_index, const int32_t* max_new, const float* temperature, const int32_t* rows,
                        const uint32_t* seed, int64_t* out_ids) {
  return guarded(c, [&]() -> int {
    return session_retry(c, n, ids, prompt, prompt_len, sot_index, max_new, temperature, rows, seed, out_ids);
  });
}

int ttasr_session_end(ttasr_ctx* c) {
  return guarded(c, [&]() -> int { return session_end(c); });
}

}  // extern "C"
