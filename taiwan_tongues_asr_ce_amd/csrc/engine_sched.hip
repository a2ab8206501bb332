// libttasr: the typed launch schedules - encoder, cross-KV, decode step, prompt prefill - and the captured decode-step graphs
// (one of the engine translation units, see engine_ctx.hpp).
#include "engine_ctx.hpp"

namespace ttasr_detail {

// ---- typed schedules ------------------------------------------------------------------------------
// 256 x 256 tiles of a 16-bit GEMM (all its batches and groups)
static int64_t gemm_tiles_256(const GemmArgs& g) {
  return ((int64_t)(g.M + 255) / 256) * (g.N / 256) * std::max(1, g.batch) * std::max(1, g.groups);
}
// THE place that decides whether a 16-bit GEMM runs as persistent 256 x 256 workgroups (round 4): it pays once a workgroup has
// several tiles to walk (>= 2 per CU).  Shared by gemm() and the grouped cross-KV launch of run_cross_kv, which used to carry
// its own copy of this predicate.
static bool gemm_takes_persistent(const ttasr_ctx* c, const GemmArgs& g) {
  if (c->force_basic || g.M < 256) return false;
  const int v = c->gemm_force;  // option enc_gemm: force 1 = 128x128 two-stage, 2 = 256x128 three-stage, 3 = 256x256 four-stage, 4 = 3 as persistent workgroups
  return (v ? v == 4 : (c->gemm_persistent && gemm_tiles_256(g) >= 512)) && gemm_bf16_v4_ok(g);
}

template <typename T>
void gemm(ttasr_ctx* c, const GemmArgs& g) {
  if constexpr (sizeof(T) == 2) {
    if (!c->force_basic && g.M >= 256) {
      const int v = c->gemm_force;
      // 256x256 tiles need >= ~half the CUs' worth of tiles to pay; below that (one or two clips, short audio windows,
      // prefill) the 256x128 kernel's twice-as-many workgroups win (B = 1 encoder: 9.45 -> 6.6 ms)
      const int64_t tiles_v3 = gemm_tiles_256(g);
      if (gemm_takes_persistent(c, g)) {
        // round 5: the same persistent kernel with the last partial round of workgroups re-tiled into shorter tiles where that pays
        if (c->gemm_tail && v != 4 && launch_gemm_bf16_v5<T>(g, c->cur)) return;
        launch_gemm_bf16_v4<T>(g, c->cur);
        return;
      }
      if ((v ? v == 3 || v == 4 : tiles_v3 >= 128) && gemm_bf16_v3_ok(g)) { launch_gemm_bf16_v3<T>(g, c->cur); return; }
      if (v != 1 && gemm_bf16_v2_ok(g)) { launch_gemm_bf16_v2<T>(g, c->cur); return; }
      if (gemm_bf16_fast_ok(g)) { launch_gemm_bf16_fast<T>(g, c->cur); return; }
    }
  }
  launch_gemm_basic<T>(g, c->cur);
}

// decode-step GEMM: B rows against a streamed weight; bf16 uses the fragment-packed skinny kernel
template <typename T>
void dec_gemm(ttasr_ctx* c, const GemmArgs& g, const void* Wsh) {
  if (c->skip_mask & 2) return;
  if constexpr (sizeof(T) == 2) {
    if (!c->force_basic && Wsh) {
      // the vocabulary projection (f32 logits, nothing else in the epilogue): persistent workgroups, activation rows in registers
      const GemmEpi& e = g.epi;
      if (c->vocab_persistent && e.out_f32 && !e.out_t && !e.bias && !e.residual && e.act == 0 &&
          launch_gemm_vocab<T>((const T*)Wsh, (const T*)g.A, g.M, g.N, g.K, e.out_f32, e.ldc, c->ko, c->cur, c->device)) return;
      if (launch_gemm_skinny<T>((const T*)Wsh, (const T*)g.A, g.M, g.N, g.K, g.epi, c->ko, c->cur)) return;
    }
  }
  launch_gemm_basic<T>(g, c->cur);
}




void enc_mark(ttasr_ctx* c, int cls) {   // cls < 0: the start mark
  if (!c->enc_timing) return;
  const size_t i = c->enc_ev_class.size();
  if (i >= c->enc_ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; c->enc_ev.push_back(e); }
  hipEventRecord(c->enc_ev[i], c->cur);
  c->enc_ev_class.push_back(cls);
}

template <typename T>
int run_cross_kv(ttasr_ctx* c, int B) {
  const int d = c->d, T_ = c->T, L = c->cfg.dec_layers;
  auto layer_args = [&](int l) {
    GemmArgs g = lin_args<T>(c->enc_out, c->dec[l].wkvx, B * T_, 2 * d, d);
    g.epi.bias = c->dec[l].bkvx;
    g.epi.out_t = (char*)c->xkv + (size_t)l * c->xkv_layer_elems * c->esz;
    g.epi.headsplit = 1; g.epi.hs_T = T_; g.epi.hs_H = c->H; g.epi.hs_d = d; g.epi.hs_which = c->xkv_which_elems;
    return g;
  };
  // Round 5: the L projections share A (the encoder output) and their weights / biases / outputs are a fixed stride apart
  // (build_weights), so the persistent 256 x 256 kernel walks all L x tiles as ONE launch: at large-v3, B = 32 that is 60 160
  // tiles = 235.0 rounds of 256 workgroups instead of 32 launches x 8 rounds (7.34 rounded up).  Same tiles, same arithmetic
  // per tile: bit-identical to the per-layer launches (option xkv_grouped = 0).
  bool grouped = false;
  if constexpr (sizeof(T) == 2) {
    GemmArgs g = layer_args(0);
    g.groups = L; g.group_stride_w = (int64_t)2 * d * d; g.group_stride_out = c->xkv_layer_elems;
    if (c->xkv_grouped && L > 1 && gemm_takes_persistent(c, g)) {
      launch_gemm_bf16_v4<T>(g, c->cur);
      grouped = true;
      enc_mark(c, EC_XKV);
    }
  }
  // a session encodes into its staging buffer (c->xkv is swapped): slot j there is not slot j of the live e4m3 copy, whose rows
  // are decoding - the session quantises at admission instead (engine_refill.hip admit), and the copy's validity is the session's
  const bool staging = c->xkv_stage && c->xkv == c->xkv_stage;
  const bool quant = c->xkv_fp8 && c->xkv8 && !staging;
  for (int l = 0; l < L; ++l) {
    if (!grouped) gemm<T>(c, layer_args(l));
    if constexpr (sizeof(T) == 2) {
      if (quant) {   // quantise this layer's K and V blocks of the B clips (one workgroup per (clip, head) block)
        for (int which = 0; which < 2; ++which) {
          const int64_t off = (int64_t)l * c->xkv_layer_elems + which * c->xkv_which_elems;
          launch_xkv_quant<T>((const T*)c->xkv + off, c->xkv8 + off, c->xkv8_scale + ((size_t)l * 2 + which) * c->maxB * c->H,
                              (int64_t)B * c->H, T_, c->cur);
        }
      }
    }
    if (!grouped || quant) enc_mark(c, EC_XKV);
  }
  if (!staging) c->xkv8_valid = quant && sizeof(T) == 2;
  return 0;
}

// The encoder's self-attention over qkv [B][T_][3 d] -> att [B][T_][d]: THE place that chooses between the MFMA flash kernel
// (kernels_flash.hip; 16-bit engines, options generic_kernels = 0 and flash = 1; flash_qw picks 64 or 32 queries per wave) and the
// plain f32 kernel (kernels_attn.hip).  Called by run_encoder, by ttasr_bench_kernel "enc_attn" and, on caller-supplied rows, by the
// known-answer hook ttasr_enc_attn_probe - which therefore has no decision logic of its own.
template <typename T>
void run_enc_attn(ttasr_ctx* c, const void* qkv, void* att, int B, int T_, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (!c->force_basic && !c->no_flash) {
      const int qw = c->ko.flash_qw >= 2 ? 2 : 1;
      if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "enc_attn_flash_kernel<%s, false, %d> grid %d", sig_type<T>(), qw,
                                    (T_ + 128 * qw - 1) / (128 * qw) * c->H * B * 256);
      launch_enc_attn_flash_bf16<T>((const T*)qkv, (T*)att, B, T_, c->H, c->ko, s);
      return;
    }
  }
  if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "enc_attn_simple_kernel<%s> grid %d", sig_type<T>(), (T_ + 15) / 16 * c->H * B * 256);
  launch_enc_attn_simple<T>((const T*)qkv, (T*)att, B, T_, c->H, s);
}
void sched_enc_attn(ttasr_ctx* c, const void* qkv, void* att, int B, int T_, hipStream_t s) { TT_DISPATCH(c, run_enc_attn<T>(c, qkv, att, B, T_, s)); }

template <typename T>
int run_encoder(ttasr_ctx* c, int B) {
  const int d = c->d, T_ = c->T, F = c->F, M = c->M, ffn = c->ffn;
  hipStream_t s = c->cur;
  hipEventRecord(c->ev[2], s);
  c->enc_ev_class.clear();
  enc_mark(c, -1);
  {  // conv1 as GEMM over the zero-padded time-major mel image: row t of A = rows t..t+2 of the image
    GemmArgs g; g.A = c->mel_t; g.W = c->conv1_w; g.M = F; g.N = d; g.K = 3 * M; g.lda = M; g.ldw = 3 * M;
    g.batch = B; g.batch_stride_a = (int64_t)(F + 2) * M;
    g.epi.bias = c->conv1_b; g.epi.act = 1; g.epi.out_t = (char*)c->c1 + (size_t)d * c->esz; g.epi.ldc = d;
    g.epi.batch_stride_c = (int64_t)(F + 2) * d;
    gemm<T>(c, g);
  }
  {  // conv2 (stride 2): row t of A starts at padded row 2t; epilogue adds the sinusoid positions
    GemmArgs g; g.A = c->c1; g.W = c->conv2_w; g.M = T_; g.N = d; g.K = 3 * d; g.lda = 2 * d; g.ldw = 3 * d;
    g.batch = B; g.batch_stride_a = (int64_t)(F + 2) * d;
    g.epi.bias = c->conv2_b; g.epi.act = 1; g.epi.rowtab = c->epos; g.epi.rowmod = T_; g.epi.out_f32 = c->x;
    g.epi.ldc = d; g.epi.batch_stride_c = (int64_t)T_ * d;
    gemm<T>(c, g);
    enc_mark(c, EC_CONV);
  }
  const int R = B * T_;
  // bf16 mode: the out-proj / fc2 GEMMs write their result (bias added) as a T "delta" into the h buffer (dead at that
  // point: its consumer GEMM has run) with the plain wide-store epilogue, and the LayerNorm that follows adds it to the
  // f32 residual stream while normalising (kernels_misc.hip layernorm_kernel ADD).  The f32 residual read-modify-write in
  // those GEMMs' epilogues - exposed at one workgroup per CU - was what held out-proj at 0.66 PF/s.
  // f32 parity mode keeps the residual epilogue.
  const bool delta = sizeof(T) == 2 && !c->force_basic && !c->enc_res_epilogue;
  // Round 5 (option enc_ln_defer): the out-projection's delta goes to the (dead) qkv buffer and is NOT folded into x by the
  // LayerNorm that follows it (which only "peeks": normalises x + delta); the next LayerNorm - after fc2, whose delta sits in h -
  // folds both in, x = (x + delta_attn) + delta_ffn: one f32 read-modify-write of the residual stream per layer instead of two
  // (LayerNorm traffic per layer and element 22 B instead of 24), bit-identical.
  const bool defer = delta && c->enc_ln_defer;
  bool pending = false;       // a delta sits in h and has not been added to x yet
  bool pending_attn = false;  // defer: the out-projection's delta sits in the qkv buffer and has not been added to x yet
  auto ln = [&](const float* g_, const float* b_, void* out, bool after_attn = false) {
    if (pending_attn && after_attn) launch_layernorm_peek<T>(c->x, (const T*)c->qkv, g_, b_, (T*)out, R, d, s);
    else if (pending_attn && pending) { launch_layernorm_add2<T>(c->x, (const T*)c->qkv, (const T*)c->h, g_, b_, (T*)out, R, d, s); pending_attn = false; }
    else if (pending) launch_layernorm_add<T>(c->x, (const T*)c->h, g_, b_, (T*)out, R, d, s);
    else launch_layernorm<T>(c->x, g_, b_, (T*)out, R, d, s);
    if (!after_attn || !pending_attn) pending = false;
    enc_mark(c, EC_LN);
  };
  auto residual_gemm = [&](const void* A, const void* W, const float* bias, int K, int cls) {
    GemmArgs g = lin_args<T>(A, W, R, d, K); g.epi.bias = bias;
    if (delta && defer && cls == EC_OUT) { g.epi.out_t = c->qkv; pending_attn = true; }   // q / k / v are dead once attention has run
    else if (delta) { g.epi.out_t = c->h; pending = true; }
    else { g.epi.residual = c->x; g.epi.out_f32 = c->x; }
    gemm<T>(c, g);
    enc_mark(c, cls);
  };
  for (int l = 0; l < c->cfg.enc_layers; ++l) {
    const EncLayerW& L = c->enc[l];
    ln(L.ln1g, L.ln1b, c->h);
    { GemmArgs g = lin_args<T>(c->h, L.wqkv, R, 3 * d, d); g.epi.bias = L.bqkv; g.epi.out_t = c->qkv; gemm<T>(c, g); }
    enc_mark(c, EC_QKV);
    run_enc_attn<T>(c, c->qkv, c->att, B, T_, s);
    enc_mark(c, EC_ATTN);
    residual_gemm(c->att, L.wo, L.bo, d, EC_OUT);
    ln(L.ln2g, L.ln2b, c->h, true);
    { GemmArgs g = lin_args<T>(c->h, L.w1, R, ffn, d); g.epi.bias = L.b1; g.epi.act = 1; g.epi.out_t = c->mid; gemm<T>(c, g); }
    enc_mark(c, EC_FC1);
    residual_gemm(c->mid, L.w2, L.b2, ffn, EC_FC2);
  }
  ln(c->elnf_g, c->elnf_b, c->enc_out);
  hipEventRecord(c->ev[3], s);
  run_cross_kv<T>(c, B);
  hipEventRecord(c->ev[4], s);
  return 0;
}

// The decode step's cross-attention of layer l for rows [row0, row0 + n): THE place that chooses between the e4m3 forms
// (kernels_fp8.hip) and the 16-bit / f32 forms behind launch_cross_attn_decode.  Called by run_decode_rows and, with row0 = 0 and
// caller-supplied queries, by the known-answer hook ttasr_cross_attn_probe - which therefore has no decision logic of its own.
// dq: T [n][d] queries (unused where sq.n > 0: the query is summed from the K-split partial tiles); datt: T [n][d] output.
template <typename T>
void run_cross_attn(ttasr_ctx* c, int l, int row0, int n, int kv_div, const void* dq, void* datt, const SlabIn& sq, const int32_t* done) {
  hipStream_t s = c->cur;
  const bool skinny = sizeof(T) == 2 && !c->force_basic;
  // cross-KV of clip (row / kv_div); a half-batch offset is only used with kv_div == 1
  const T* Kx = (const T*)c->xkv + (int64_t)l * c->xkv_layer_elems + (int64_t)(row0 / kv_div) * c->H * c->T * 64;
  bool fp8_done = false;
  if constexpr (sizeof(T) == 2) {   // opt-in: the e4m3 copy of the cache, unshared rows that fill the chip (the single-pass kernel's case)
    if (c->xkv_fp8 && c->xkv8_valid && kv_div == 1 && n * c->H >= 256 && skinny && !(c->skip_mask & 8)) {
      const int64_t off = (int64_t)l * c->xkv_layer_elems + (int64_t)row0 * c->H * c->T * 64;
      const float* ksc = c->xkv8_scale + ((size_t)l * 2) * c->maxB * c->H + (size_t)row0 * c->H;
      fp8_done = launch_cross_attn_fp8<T>((const T*)dq, c->xkv8 + off, c->xkv8 + off + c->xkv_which_elems, ksc, ksc + (size_t)c->maxB * c->H,
                                          (T*)datt, n, c->H, c->T, s, sq, done);
    } else if (c->xkv_fp8 == 2 && c->xattn_mq_fp8 && c->xkv8_valid && kv_div >= 2 && skinny && !c->no_xsplit && !(c->skip_mask & 8)) {
      // mode 2: rows that share a clip (beam hypotheses, sampled attempts) - wherever the 16-bit path would take
      // cross_attn_mq_kernel with kv_div = 2..7, its e4m3 form; every other shape falls through to the 16-bit kernels
      const int clip0 = row0 / kv_div;
      const int64_t off = (int64_t)l * c->xkv_layer_elems + (int64_t)clip0 * c->H * c->T * 64;
      const float* ksc = c->xkv8_scale + ((size_t)l * 2) * c->maxB * c->H + (size_t)clip0 * c->H;
      fp8_done = launch_cross_attn_mq_fp8<T>((const T*)dq, c->xkv8 + off, c->xkv8 + off + c->xkv_which_elems, ksc, ksc + (size_t)c->maxB * c->H,
                                             (T*)datt, n, c->H, c->T, kv_div, c->ko, s, c->xsplit_ws + (size_t)row0 * c->H * 8 * 66, sq,
                                             c->maxB - row0, done);
    }
  }
  if (!fp8_done && !(c->skip_mask & 8))
    launch_cross_attn_decode<T>((const T*)dq, Kx, Kx + c->xkv_which_elems, (T*)datt, n, c->H, c->T, kv_div, c->ko, s,
                                c->no_xsplit ? nullptr : c->xsplit_ws + (size_t)row0 * c->H * 8 * 66, sq, c->maxB - row0, QProj{}, done);
}

// One decoder step for rows [row0, row0 + n) at position *st.step, enqueued on c->cur.
// mode 0: through logits + select; 1: logits only (test API / beam search); 2: no logits (all rows forced by
// the prompt), select just advances the forced token; 3: the language head (kernels_lang.hip) over the span c->lang_begin /
// c->lang_n instead of the vocabulary projection, no select (ttasr_detect_language).  `total_rows` = rows of the whole step (both half-batch chains):
// the select launch that finishes last advances the position counter.
//
// bf16 launch plan per layer (the measured mode; no float atomics anywhere, every launch bit-reproducible):
//   LN1 -> qkv GEMM (K-split, f32 slabs) -> self-attention (sums the q, k, v slabs) -> out-proj (K-split slabs) ->
//   LN2 (x += bias + slabs, then normalise) -> q GEMM (K-split slabs) -> cross-attention (sums the q slabs) ->
//   out-proj (slabs) -> LN3 (sums) -> fc1 + GELU (unsplit: the activation needs the full sum) -> fc2 (slabs) -> next LN1 (sums)
// Splitting K spreads every weight matrix over >= 160 workgroups in pieces of <= 20-40 KB (a CU takes in only ~25 GB/s
// of HBM-cold bytes).  LN1 of layer 0 creates the row from the token + position embedding itself.
// The f32 parity mode runs the generic kernels: LayerNorm, gemm_basic with the residual epilogue in place.
template <typename T>
void run_decode_rows(ttasr_ctx* c, int row0, int n, int mode, int total_rows) {
  const int d = c->d, ffn = c->ffn;
  hipStream_t s = c->cur;
  const size_t e = c->esz;
  auto tp = [&](void* base, int64_t width) { return (void*)((char*)base + (size_t)row0 * width * e); };  // T rows
  float* dx = c->dx + (size_t)row0 * d;
  void *dh = tp(c->dh, d), *dqkv = tp(c->dqkv, 3 * d), *dq = tp(c->dq, d), *datt = tp(c->datt, d), *dmid = tp(c->dmid, ffn);
  float* logits = c->logits + (size_t)row0 * c->ldv;
  const bool skinny = sizeof(T) == 2 && !c->force_basic;
  // round 6: rows whose search has FINISHED (st.done, set by select_kernel / uploaded by the beam search) leave the attention
  // kernels of the step - the per-row cross-KV and self-KV streams are the bytes of a decode step that scale with the rows
  // the continuous-batching session (engine_refill.hip) runs the per-row-position forms of the three kernels that read the position;
  // its idle and finished rows always leave the attention kernels (their slots may be refilled by a concurrent encode)
  const StepShape& sh = c->shape;
  const bool rows_pos = sh.rows_pos;
  const int32_t* done = (c->ragged_exit || rows_pos) ? c->st.done + row0 : nullptr;
  float* slab_base = c->slab;
  // K slices per GEMM kind (0 out-proj, 1 q, 2 qkv, 3 fc2); attention consumers sum at most 4 slabs
  auto slices = [&](int kind, int N, int K) {
    if (!skinny) return 1;
    int want = c->ks_want[kind];
    // Round 6: with the activation tile staged through LDS (kernels_skinny.hip) the K-split optimum of two GEMMs moved - re-swept
    // with `tools/decode_variants.py` (large-v3, 32 rows, decode of 128 tokens, two interleaved rounds): qkv UNSPLIT (120 n-blocks x
    // 8 waves, the self-attention reads q, k, v directly) 354.7-355.5 ms against 356.9-357.7 with the 2 slices that rounds 3-5
    // used; out-proj at the automatic 4 slices 355.4-356.1 against the 5 of round 5; both 352.7-352.9.  Wider batches (beam
    // search, streaming: 33-128 rows) keep the automatic choice, whose k-steps per wave fit the straight-line form.
    // (A different K split is a different summation order: the 16-bit token CRC of the benchmark was re-recorded with this change.)
    if (kind == 2 && want == 0 && n <= 32 && (N + 31) / 32 >= 96) want = 1;
    int ks = gemm_skinny_ksplit(n, N, K, want, c->ko);
    if ((kind == 1 || kind == 2) && ks > 4) ks = gemm_skinny_ksplit(n, N, K, 4, c->ko);
    return ks;
  };
  // what the next LayerNorm still has to add to the residual rows (K-split residual GEMM) or to create (embedding)
  struct { const float* bias = nullptr; int n_slab = 0; bool embed = true; } pend;

  // K-split GEMM into slabs [ks][maxB rows][N]; returns the slab descriptor for the consumer (n == 0: not split, `g` ran whole)
  auto split_gemm = [&](const GemmArgs& g, const void* Wsh, const float* bias, int ks) -> SlabIn {
    SlabIn si;
    if constexpr (sizeof(T) == 2) {
      if (ks > 1 && Wsh) {
        GemmEpi ep; ep.ldc = g.N;
        float* slab = slab_base;  // rows are local to this chain's region: [ks][maxB][N]
        const int64_t stride = (int64_t)c->maxB * g.N;
        if (launch_gemm_skinny<T>((const T*)Wsh, (const T*)g.A, n, g.N, g.K, ep, c->ko, s, ks, slab, stride)) {
          si.slab = slab; si.bias = bias; si.n = ks; si.stride = stride; si.ld = g.N;
        }
      }
    }
    return si;
  };
  // x += W a + b
  auto residual_gemm = [&](const void* A, const void* W, const void* Wsh, const float* bias, int K, int kind) {
    if (c->skip_mask & 2) return;
    GemmArgs g = lin_args<T>(A, W, n, d, K);
    const SlabIn si = split_gemm(g, Wsh, bias, slices(kind, d, K));
    if (si.n) { pend.bias = bias; pend.n_slab = si.n; return; }
    g.epi.bias = bias; g.epi.residual = dx; g.epi.out_f32 = dx;
    dec_gemm<T>(c, g, Wsh);
  };
  auto ln = [&](const float* g_, const float* b_) {
    if (c->skip_mask & 1) return;
    LnPre pre;
    pre.x_out = dx;
    if (pend.embed) { pre.tok = c->st.cur_tok + row0; pre.step = rows_pos ? c->row_pos + row0 : c->st.step; pre.emb = c->emb; pre.pos = c->dpos; }
    else if (pend.n_slab) { pre.bias = pend.bias; pre.slab = slab_base; pre.n_slab = pend.n_slab; pre.slab_stride = (int64_t)c->maxB * d; }
    if (pend.embed && rows_pos) launch_layernorm_rows_embed_pos<T>(g_, b_, (T*)dh, n, d, pre, s);
    else launch_layernorm_rows<T>(dx, g_, b_, (T*)dh, n, d, pre, s);
    pend.bias = nullptr; pend.n_slab = 0; pend.embed = false;
  };
  for (int l = 0; l < c->cfg.dec_layers; ++l) {
    const DecLayerW& L = c->dec[l];
    ln(L.ln1g, L.ln1b);
    SlabIn sqkv;
    { GemmArgs g = lin_args<T>(dh, L.wqkv, n, 3 * d, d);
      sqkv = split_gemm(g, L.wqkv_sh, L.bqkv, slices(2, 3 * d, d));
      if (!sqkv.n) { g.epi.bias = L.bqkv; g.epi.out_t = dqkv; dec_gemm<T>(c, g, L.wqkv_sh); } }
    if (!(c->skip_mask & 4) && rows_pos)
      launch_self_attn_decode_rows<T>((const T*)dqkv, (T*)c->pool, c->page_table, c->pages_per_seq, (int64_t)l * c->pool_layer_elems,
                                      sh.identity_pages, row0, c->row_pos, (T*)datt, n, c->H, s, sqkv, done);
    else if (!(c->skip_mask & 4))
      launch_self_attn_decode<T>((const T*)dqkv, (T*)c->pool, c->page_table, c->pages_per_seq, (int64_t)l * c->pool_layer_elems,
                                 sh.identity_pages, row0, c->st.step, (T*)datt, n, c->H, s, sqkv, done);
    residual_gemm(datt, L.wo, L.wo_sh, L.bo, d, 0);
    ln(L.ln2g, L.ln2b);
    SlabIn sq;
    { GemmArgs g = lin_args<T>(dh, L.wqx, n, d, d);
      sq = split_gemm(g, L.wqx_sh, L.bqx, slices(1, d, d));
      if (!sq.n) { g.epi.bias = L.bqx; g.epi.out_t = dq; dec_gemm<T>(c, g, L.wqx_sh); } }
    run_cross_attn<T>(c, l, row0, n, sh.kv_div, dq, datt, sq, done);
    residual_gemm(datt, L.wox, L.wox_sh, L.box, d, 0);
    ln(L.ln3g, L.ln3b);
    { GemmArgs g = lin_args<T>(dh, L.w1, n, ffn, d); g.epi.bias = L.b1; g.epi.act = 1; g.epi.out_t = dmid; dec_gemm<T>(c, g, L.w1_sh); }
    residual_gemm(dmid, L.w2, L.w2_sh, L.b2, ffn, 3);
  }
  if (mode != 2) {
    ln(c->dlnf_g, c->dlnf_b);
    if (mode == 3) {   // the rows of the plain tied embedding (not the packed copy): n_lang dot products per row, softmax, winner
      float* probs = c->lang_out + (size_t)row0 * c->lang_n;
      float* span = c->lang_out + (size_t)c->maxB * 128 + (size_t)row0 * c->lang_n;
      launch_lang_head<T>((const T*)dh, (const T*)c->emb, n, d, c->V, c->lang_begin, c->lang_n, probs,
                          (int32_t*)(c->lang_out + (size_t)c->maxB * 256) + row0, c->lang_want_logits ? span : nullptr, s);
      return;
    }
    GemmArgs g = lin_args<T>(dh, c->emb, n, c->V, d);  // proj_out tied to embed_tokens (modeling_whisper.py:965)
    g.epi.out_f32 = logits; g.epi.ldc = c->ldv;
    dec_gemm<T>(c, g, c->emb_sh);
  }
  if (mode != 1 && !(c->skip_mask & 16)) {
    DecState st = c->st;  // row-offset view of the search state
    st.cur_tok += row0; st.n_sampled += row0; st.last_tok += row0; st.pen_tok += row0; st.last_ts += row0; st.done += row0;
    st.sum_logprob += row0; st.no_speech += row0; st.out_tokens += (size_t)row0 * c->rp.max_new; st.row_cap += row0;
    if (st.prompt) { st.prompt += (size_t)row0 * c->rp.max_prompt; st.prompt_len += row0; }
    // a table is installed (static searches only): the bias lands on the raw logits of the rows that choose at this step, in
    // front of the rules (mode 2 computes no logits: every row is forced)
    if (sh.seq_bias && !rows_pos && mode == 0)
      launch_seq_bias(logits, c->ldv, c->seq_bias_dev.get(),
                      SeqBiasHist{st.out_tokens, st.n_sampled, st.prompt, st.prompt_len, st.done, c->st.step, st.dyn, nullptr, nullptr}, true, n, s);
    if (rows_pos) { st.step = c->row_pos + row0; launch_select_rows(logits, st, c->rp, n, s); }
    else launch_select(logits, st, c->rp, n, nullptr, s, c->st.step + 1, total_rows);
    if (rows_pos && sh.lang_rows && mode == 0) {
      // armed session: the rows that were admitted with the language placeholder have just run <|startoftranscript|> at position
      // 0; the head overwrites what select did to them (forced prompt rows: fed token and position) and restarts them
      int32_t* const ls = c->lang_sess + row0;
      const int B = c->maxB;
      const LangRows a{ls, ls + B, c->prompt_dev + (size_t)row0 * c->sess_lang_stride, c->sess_lang_stride, c->st.cur_tok + row0, c->row_pos + row0,
                       ls + 4 * B, (float*)(c->lang_sess + 5 * B) + (size_t)row0 * c->sess_lang_n,
                       (float*)(c->lang_sess + 5 * B) + (size_t)B * 128 + (size_t)row0 * c->sess_lang_n};
      launch_lang_head_rows<T>((const T*)dh, (const T*)c->emb, n, d, c->V, c->sess_lang_begin, c->sess_lang_n, a, s);
    }
  }
}


template <typename T>
void run_prefill(ttasr_ctx* c, int n_seq, int npos, int seq_per_clip, int max_prompt, const AlignOut* al) {
  const int d = c->d, ffn = c->ffn, n = n_seq * npos;
  hipStream_t s = c->cur = c->stream;
  float* x = c->x;
  void *h = c->h, *qkv = c->qkv, *att = c->att, *mid = c->mid;
  launch_embed_prefill<T>(al && al->tokens ? al->tokens : c->prompt_dev, max_prompt, 1, n_seq, npos, (const T*)c->emb, (const T*)c->dpos, x, d, s);
  // up to 128 rows (short prompts: a handful of positions x the clips of a pass) the fragment-packed decode GEMM streams each
  // weight once for all rows; beyond that the rows are a real M dimension for the tiled encoder GEMMs
  const bool small = n <= 128 && !c->force_basic && !c->prefill_tiled;
  // Round 3: the small pass runs the DECODE-STEP launch plan - every GEMM whose consumer can add partial results is cut into K
  // slices (160-320 workgroups instead of 40 of them pulling 164-656 KB each: a CU takes in ~25 GB/s of cold bytes), the
  // partial tiles go to the f32 slabs, and the per-row LayerNorm / the cross-attention kernel sum them in slab order (no
  // atomics: bit-reproducible).  A 3-position prompt of 32 clips then costs about 1.3 decode steps instead of 3.
  const bool slabbed = small && sizeof(T) == 2;
  const bool own_pages = al && al->page_table;   // batched alignment: the sequences' own page lists, not the rows' of the search
  const int64_t slab_cap = (int64_t)16 * c->maxB * 3 * d;   // floats in c->slab
  struct { const float* bias = nullptr; int n_slab = 0; int64_t stride = 0; } pend;
  auto pgemm = [&](const GemmArgs& g, const void* Wsh) {
    if constexpr (sizeof(T) == 2) {
      if (small && Wsh && launch_gemm_skinny<T>((const T*)Wsh, (const T*)g.A, g.M, g.N, g.K, g.epi, c->ko, s)) return;
    }
    gemm<T>(c, g);
  };
  // K-split GEMM into slabs [ks][n][N]; returns the slab descriptor (n == 0: not split, the caller runs the GEMM whole)
  auto split_gemm = [&](const GemmArgs& g, const void* Wsh, const float* bias, int max_ks) -> SlabIn {
    SlabIn si;
    if constexpr (sizeof(T) == 2) {
      if (slabbed && Wsh) {
        int ks = gemm_skinny_ksplit(n, g.N, g.K, 0, c->ko);
        if (ks > max_ks) ks = gemm_skinny_ksplit(n, g.N, g.K, max_ks, c->ko);
        const int64_t stride = (int64_t)n * g.N;
        GemmEpi ep; ep.ldc = g.N;
        if (ks > 1 && ks * stride <= slab_cap &&
            launch_gemm_skinny<T>((const T*)Wsh, (const T*)g.A, n, g.N, g.K, ep, c->ko, s, ks, c->slab, stride)) {
          si.slab = c->slab; si.bias = bias; si.n = ks; si.stride = stride; si.ld = g.N;
        }
      }
    }
    return si;
  };
  auto ln = [&](const float* g_, const float* b_) {
    if (slabbed) {
      LnPre pre; pre.x_out = x;
      if (pend.n_slab) { pre.bias = pend.bias; pre.slab = c->slab; pre.n_slab = pend.n_slab; pre.slab_stride = pend.stride; }
      launch_layernorm_rows<T>(x, g_, b_, (T*)h, n, d, pre, s);
      pend.bias = nullptr; pend.n_slab = 0;
    } else {
      launch_layernorm<T>(x, g_, b_, (T*)h, n, d, s);
    }
  };
  auto residual_gemm = [&](const void* A, const void* W, const void* Wsh, const float* bias, int K) {   // x += W a + b
    GemmArgs g = lin_args<T>(A, W, n, d, K);
    const SlabIn si = split_gemm(g, Wsh, bias, 16);
    if (si.n) { pend.bias = bias; pend.n_slab = si.n; pend.stride = si.stride; return; }
    g.epi.bias = bias; g.epi.residual = x; g.epi.out_f32 = x;
    pgemm(g, Wsh);
  };
  for (int l = 0; l < c->cfg.dec_layers; ++l) {
    const DecLayerW& L = c->dec[l];
    ln(L.ln1g, L.ln1b);
    { GemmArgs g = lin_args<T>(h, L.wqkv, n, 3 * d, d); g.epi.bias = L.bqkv; g.epi.out_t = qkv; pgemm(g, L.wqkv_sh); }
    launch_self_attn_prefill<T>((const T*)qkv, (T*)c->pool, own_pages ? al->page_table : c->page_table, c->pages_per_seq,
                                (int64_t)l * c->pool_layer_elems, own_pages ? 0 : c->shape.identity_pages, (T*)att, n_seq, npos, c->H, s);
    residual_gemm(att, L.wo, L.wo_sh, L.bo, d);
    ln(L.ln2g, L.ln2b);
    SlabIn sq;   // the query of the cross-attention: K-split too when its consumer can sum slabs (not the alignment pass)
    { GemmArgs g = lin_args<T>(h, L.wqx, n, d, d);
      if (!al && npos * seq_per_clip < 32) sq = split_gemm(g, L.wqx_sh, L.bqx, 4);   // >= 32 rows per clip: the MFMA flash pass reads T rows
      if (!sq.n) { g.epi.bias = L.bqx; g.epi.out_t = qkv; pgemm(g, L.wqx_sh); } }  // q reuses the qkv buffer
    const T* Kx = (const T*)c->xkv + (int64_t)l * c->xkv_layer_elems;
    if (al && al->seq_clip) {
      launch_cross_attn_probs_batch<T>((const T*)qkv, Kx, Kx + c->xkv_which_elems, (T*)att, n_seq, npos, c->H, c->T,
                                       al->sel + (size_t)l * c->H, al->seq_clip, al->probs, s);
    } else if (al) {
      const T* Kc = Kx + (int64_t)al->clip * c->H * c->T * 64;
      launch_cross_attn_probs<T>((const T*)qkv, Kc, Kc + c->xkv_which_elems, (T*)att, n, c->H, c->T, al->sel + (size_t)l * c->H,
                                 al->probs, s);
    } else {
      launch_cross_attn_decode<T>((const T*)qkv, Kx, Kx + c->xkv_which_elems, (T*)att, n, c->H, c->T, npos * seq_per_clip, c->ko, s,
                                  c->no_xsplit ? nullptr : c->xsplit_ws, sq, c->maxB);
    }
    residual_gemm(att, L.wox, L.wox_sh, L.box, d);
    ln(L.ln3g, L.ln3b);
    { GemmArgs g = lin_args<T>(h, L.w1, n, ffn, d); g.epi.bias = L.b1; g.epi.act = 1; g.epi.out_t = mid; pgemm(g, L.w1_sh); }
    residual_gemm(mid, L.w2, L.w2_sh, L.b2, ffn);
  }
  // callers read the finished residual rows from c->x (no-speech probability, token log-probs of the alignment pass): fold the
  // last fc2's partial tiles in (the final decoder LayerNorm does it; its normalised output lands in h and is not used here)
  if (pend.n_slab) ln(c->dlnf_g, c->dlnf_b);
}

// The admission pass of a session (option session_prefill; engine_refill.hip): the decoder layers over the PACKED prompt rows of
// the admitted clips, on the decode stream, out of the pass's own workspace (c->pf_*).  Only the self-attention K / V of these
// positions has to survive: no final LayerNorm, no vocabulary GEMM, nothing reads the residual afterwards.
// A prefilled clip's bits must not depend on its pass-mates, so every kernel form is a function of context constants: the GEMMs
// run in ONE family whatever the row count - 16-bit: the first of the 256 x 256, 256 x 128 and 128 x 128 tiled kernels that takes
// the context's widths (a row of a tile depends on its own A row only, and rows past M are loaded clamped and never stored);
// f32 or option generic_kernels: the generic kernel - the attention work items are cut from each sequence's own length, and the
// K-split skinny path of run_prefill, whose split follows the pass's row count, is not used.
// al != nullptr: the packed alignment pass (option align_packed, engine_align.hip).  The same launches; in a layer that holds a
// selected head the 16-bit cross-attention is the MAPS = true instantiation of the same kernel, the per-row form gets the
// layer's selection and the map buffer, and the stored score rows are finished into softmax maps behind the last layer.
template <typename T>
void align_cross_attn(ttasr_ctx* c, int l, const PrefillPass& P, const void* q, void* att, const PackedAlign* al) {
  hipStream_t s = c->stream;
  const T* Kx = (const T*)c->xkv + (int64_t)l * c->xkv_layer_elems;   // the 16-bit live slots, also under xkv_fp8 = 2
  bool any = false;
  if (al) for (int h = 0; h < c->H; ++h) any |= al->sel_host[(size_t)l * c->H + h] >= 0;
  if constexpr (sizeof(T) == 2) {
    if (!c->force_basic) {
      if (any) launch_prefill_cross_attn_maps<T>(P, (const T*)q, Kx, Kx + c->xkv_which_elems, (T*)att, c->H, c->T,
                                                 PrefillMaps{al->sel + (size_t)l * c->H, al->maps, al->stat, P.n_rows}, s);
      else launch_prefill_cross_attn<T>(P, (const T*)q, Kx, Kx + c->xkv_which_elems, (T*)att, c->H, c->T, s);
      return;
    }
  }
  // per-row form: "sequence" = one packed row, its slot from the table; without a selected head no softmax map is written
  launch_cross_attn_probs_batch<T>((const T*)q, Kx, Kx + c->xkv_which_elems, (T*)att, P.n_rows, 1, c->H, c->T,
                                   any ? al->sel + (size_t)l * c->H : c->pf_sel, P.slots, any ? al->maps : nullptr, s);
}
template <typename T>
void run_admit_prefill(ttasr_ctx* c, const PrefillPass& P, const PackedAlign* al) {
  const int d = c->d, ffn = c->ffn, n = P.n_rows;
  hipStream_t s = c->cur = c->stream;
  float* x = c->pf_x;
  void *h = c->pf_h, *qkv = c->pf_qkv, *att = c->pf_att, *mid = c->pf_mid;
  auto pgemm = [&](const GemmArgs& g) {
    if constexpr (sizeof(T) == 2) {
      if (!c->force_basic) {
        if (gemm_bf16_v3_ok(g)) { launch_gemm_bf16_v3<T>(g, s); return; }
        if (gemm_bf16_v2_ok(g)) { launch_gemm_bf16_v2<T>(g, s); return; }
        if (gemm_bf16_fast_ok(g)) { launch_gemm_bf16_fast<T>(g, s); return; }
      }
    }
    launch_gemm_basic<T>(g, s);
  };
  auto residual_gemm = [&](const void* A, const void* W, const float* bias, int K) {   // x += W a + b
    GemmArgs g = lin_args<T>(A, W, n, d, K);
    g.epi.bias = bias; g.epi.residual = x; g.epi.out_f32 = x;
    pgemm(g);
  };
  launch_prefill_embed<T>(P, (const T*)c->emb, (const T*)c->dpos, x, d, s);
  for (int l = 0; l < c->cfg.dec_layers; ++l) {
    const DecLayerW& L = c->dec[l];
    launch_layernorm<T>(x, L.ln1g, L.ln1b, (T*)h, n, d, s);
    { GemmArgs g = lin_args<T>(h, L.wqkv, n, 3 * d, d); g.epi.bias = L.bqkv; g.epi.out_t = qkv; pgemm(g); }
    launch_prefill_self_attn<T>(P, (const T*)qkv, (T*)c->pool + (int64_t)l * c->pool_layer_elems, (T*)att, c->H, s);
    residual_gemm(att, L.wo, L.bo, d);
    launch_layernorm<T>(x, L.ln2g, L.ln2b, (T*)h, n, d, s);
    { GemmArgs g = lin_args<T>(h, L.wqx, n, d, d); g.epi.bias = L.bqx; g.epi.out_t = qkv; pgemm(g); }   // q reuses the qkv buffer
    align_cross_attn<T>(c, l, P, qkv, att, al);
    residual_gemm(att, L.wox, L.box, d);
    launch_layernorm<T>(x, L.ln3g, L.ln3b, (T*)h, n, d, s);
    { GemmArgs g = lin_args<T>(h, L.w1, n, ffn, d); g.epi.bias = L.b1; g.epi.act = 1; g.epi.out_t = mid; pgemm(g); }
    residual_gemm(mid, L.w2, L.b2, ffn);
  }
  if (al && sizeof(T) == 2 && !c->force_basic) launch_prefill_maps_finish(al->maps, al->stat, al->n_pairs, n, c->T, s);
}

// log p(target[r] | row r) of the packed residual rows the alignment pass left in c->pf_x: final LayerNorm, the vocabulary
// projection in the admission pass's fixed GEMM family (a row's logits depend on its own row only), max_batch rows at a time
// through the step's logits buffer.
template <typename T>
void run_packed_logprob(ttasr_ctx* c, int n_rows, const int32_t* target, float* out) {
  hipStream_t s = c->cur = c->stream;
  const int d = c->d;
  launch_layernorm<T>(c->pf_x, c->dlnf_g, c->dlnf_b, (T*)c->pf_h, n_rows, d, s);
  for (int r0 = 0; r0 < n_rows; r0 += c->maxB) {
    const int m = std::min(c->maxB, n_rows - r0);
    GemmArgs g = lin_args<T>((const T*)c->pf_h + (size_t)r0 * d, c->emb, m, c->V, d);
    g.epi.out_f32 = c->logits; g.epi.ldc = c->ldv;
    bool done = false;
    if constexpr (sizeof(T) == 2) {
      if (!c->force_basic) {
        if (gemm_bf16_v3_ok(g)) { launch_gemm_bf16_v3<T>(g, s); done = true; }
        else if (gemm_bf16_v2_ok(g)) { launch_gemm_bf16_v2<T>(g, s); done = true; }
        else if (gemm_bf16_fast_ok(g)) { launch_gemm_bf16_fast<T>(g, s); done = true; }
      }
    }
    if (!done) launch_gemm_basic<T>(g, s);
    launch_token_logprob(c->logits, c->ldv, c->V, target + r0, out + r0, m, s);
  }
}

// How many leading prompt positions can be prefilled: every row must still have a forced token after them and the rows
// must fit the borrowed encoder workspaces.  Below 2 positions the pass does not pay.  `ns_from_prefill` = the caller can
// take the no-speech probability from the prefilled <|startoftranscript|> position (prefill_no_speech); otherwise that
// position needs a real decode step and bounds the prefill.
int prefill_positions(const ttasr_ctx* c, int min_plen, const ttasr_gen_opts* o, bool ns_from_prefill) {
  if (c->no_prefill) return 0;
  int p = min_plen - 1;
  if (o->no_speech >= 0 && !ns_from_prefill) p = std::min(p, o->sot_index);
  p = std::min(p, c->cfg.n_audio_ctx);
  return p >= 2 ? p : 0;
}

// No-speech probability from a prefill pass: the residual rows of position `sot` of every sequence (left in c->x by
// run_prefill, rows [sequence][position]) -> final LayerNorm -> vocabulary projection -> softmax(raw logits)[no_speech].
template <typename T>
int prefill_no_speech(ttasr_ctx* c, int n_seq, int npos, int sot, int no_speech_tok) {
  hipStream_t s = c->stream;
  const int d = c->d;
  c->cur = s;
  HIPCHK(c, hipMemcpy2DAsync(c->dx, (size_t)d * 4, c->x + (size_t)sot * d, (size_t)npos * d * 4, (size_t)d * 4, n_seq,
                             hipMemcpyDeviceToDevice, s));
  launch_layernorm_rows<T>(c->dx, c->dlnf_g, c->dlnf_b, (T*)c->dh, n_seq, d, LnPre{}, s);
  GemmArgs g = lin_args<T>(c->dh, c->emb, n_seq, c->V, d);
  g.epi.out_f32 = c->logits; g.epi.ldc = c->ldv;
  dec_gemm<T>(c, g, c->emb_sh);
  launch_token_prob(c->logits, c->ldv, c->V, no_speech_tok, c->st.no_speech, n_seq, s);
  return 0;
}

// One decode step = one dependent chain of ~355 launches on the context's stream, captured as a hipGraph.  Splitting the
// batch into two half-batch chains on two streams inside the graph (round 1's dual-chain experiment: +4 % then) doubles the
// launch count and, with the round-2 kernels, measures 3 % SLOWER (3.15 vs 3.05 ms per step): removed.
template <typename T>
void run_decode_step(ttasr_ctx* c, int B, int mode) {
  c->cur = c->stream;
  run_decode_rows<T>(c, 0, B, mode, B);
  // modes 0 and 2 end with select_kernel, whose last workgroup advances the position; mode 1 has no select
  if (mode == 1 || (c->skip_mask & 16)) launch_advance(c->st.step, c->stream);
}

// `nsteps` consecutive steps of the same mode as ONE graph (round 4): the search state is device-resident, so a run of greedy
// steps between two host polls needs no host involvement at all; one replay instead of nsteps saves the graph-launch gap
// (~8 us on the device, 10-16 us of host time per replay) per step.
int step_graph(ttasr_ctx* c, int B, int mode, int nsteps) {
  if (!c->use_graph) {
    for (int i = 0; i < nsteps; ++i) TT_DISPATCH(c, run_decode_step<T>(c, B, mode));
    return 0;
  }
  // everything that decides WHICH kernels a captured step holds is part of the key: whether the e4m3 cross-KV copy is live
  // changes with encode (run_cross_kv builds it), not only with set_option (a graph captured between
  // set_option(xkv_fp8) and the next encode held the 16-bit kernel and kept replaying after the copy existed)
  // ... and WHICH mode it is read in: 1 and 2 pick different kernels for shared rows, and so does option xattn_mq_fp8 under mode 2
  const int fp8_live = (c->xkv_fp8 && c->xkv8_valid) ? (c->xkv_fp8 == 2 ? (c->xattn_mq_fp8 ? 3 : 2) : 1) : 0;
  const ttasr_ctx::GraphKey key{B, mode, nsteps, c->shape, fp8_live};
  for (size_t i = 0; i < c->graphs.size(); ++i) {
    if (c->graphs[i].key == key) {
      // most recently used at the back: the cache is bounded (the streaming micro-batcher varies B from 1 to max_batch rows)
      if (i + 1 != c->graphs.size()) std::rotate(c->graphs.begin() + i, c->graphs.begin() + i + 1, c->graphs.end());
      HIPCHK(c, hipGraphLaunch(c->graphs.back().exec, c->stream));
      return 0;
    }
  }
  hipGraph_t graph = nullptr;
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < nsteps; ++i) TT_DISPATCH(c, run_decode_step<T>(c, B, mode));
  HIPCHK(c, hipStreamEndCapture(c->stream, &graph));
  hipGraphExec_t exec = nullptr;
  const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);   // on the failure path too
  if (ie != hipSuccess) return fail(c, TTASR_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
  if (c->graphs.size() >= ttasr_ctx::kMaxGraphs) {   // evict the least recently used executable
    hipGraphExecDestroy(c->graphs.front().exec);
    c->graphs.erase(c->graphs.begin());
  }
  c->graphs.push_back({key, exec});
  HIPCHK(c, hipGraphLaunch(exec, c->stream));
  return 0;
}

void drop_graphs(ttasr_ctx* c) {
  for (auto& g : c->graphs) hipGraphExecDestroy(g.exec);
  c->graphs.clear();
}

// The rule scalars (RuleParams) are baked into the select launch of the mode 0 / 2 graphs only; the logits-only graphs
// (mode 1: step API, beam search) never launch select_kernel and survive a change of rules - with
// condition_on_previous_text the prompt geometry changes on nearly every window of a file.
void drop_rule_graphs(ttasr_ctx* c) {
  size_t k = 0;
  for (auto& g : c->graphs) {
    if (g.key.mode == 1) c->graphs[k++] = g; else hipGraphExecDestroy(g.exec);
  }
  c->graphs.resize(k);
}

// The span and the prompt stride are baked into the language-head launch of an armed session's graphs: a session armed with
// other values captures its own.
void drop_lang_graphs(ttasr_ctx* c) {
  size_t k = 0;
  for (auto& g : c->graphs) {
    if (!g.key.shape.lang_rows) c->graphs[k++] = g; else hipGraphExecDestroy(g.exec);
  }
  c->graphs.resize(k);
}

// ---- entry points for the other translation units: T is dispatched here ----
void sched_encoder(ttasr_ctx* c, int B) { TT_DISPATCH(c, run_encoder<T>(c, B)); }
void sched_cross_kv(ttasr_ctx* c, int B) { TT_DISPATCH(c, run_cross_kv<T>(c, B)); }
void sched_prefill(ttasr_ctx* c, int n_seq, int npos, int seq_per_clip, int max_prompt, const AlignOut* al) {
  TT_DISPATCH(c, run_prefill<T>(c, n_seq, npos, seq_per_clip, max_prompt, al));
}
void sched_admit_prefill(ttasr_ctx* c, const PrefillPass& P, const PackedAlign* al) { TT_DISPATCH(c, run_admit_prefill<T>(c, P, al)); }
void sched_align_attn(ttasr_ctx* c, int layer, const PrefillPass& P, const void* dq, void* datt, const PackedAlign& al) {
  c->cur = c->stream;
  TT_DISPATCH(c, align_cross_attn<T>(c, layer, P, dq, datt, &al));
  if (c->lowp && !c->force_basic && al.n_pairs > 0) launch_prefill_maps_finish(al.maps, al.stat, al.n_pairs, P.n_rows, c->T, c->stream);
}
void sched_packed_logprob(ttasr_ctx* c, int n_rows, const int32_t* target, float* out) {
  TT_DISPATCH(c, run_packed_logprob<T>(c, n_rows, target, out));
}
int sched_prefill_no_speech(ttasr_ctx* c, int n_seq, int npos, int sot, int no_speech_tok) {
  TT_DISPATCH(c, return prefill_no_speech<T>(c, n_seq, npos, sot, no_speech_tok));
  return 0;
}
void sched_cross_attn(ttasr_ctx* c, int layer, int n, int kv_div, const void* dq, void* datt, const SlabIn& sq, const int32_t* done) {
  c->cur = c->stream;
  TT_DISPATCH(c, run_cross_attn<T>(c, layer, 0, n, kv_div, dq, datt, sq, done));
}
void sched_detect_rows(ttasr_ctx* c, int B) { c->cur = c->stream; TT_DISPATCH(c, run_decode_rows<T>(c, 0, B, 3, B)); }
void sched_gemm(ttasr_ctx* c, const GemmArgs& g) { TT_DISPATCH(c, gemm<T>(c, g)); }
void sched_dec_gemm(ttasr_ctx* c, const GemmArgs& g, const void* Wsh) { TT_DISPATCH(c, dec_gemm<T>(c, g, Wsh)); }

}  // namespace ttasr_detail
