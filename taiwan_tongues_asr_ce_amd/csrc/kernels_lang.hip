// Language head: the language-identification tail of a decoder pass at the <|startoftranscript|> position.  Instead of the
// full vocabulary projection (51 866 columns) followed by a host softmax over ~100 of them, one workgroup per row computes
// only the dot products of the row with the language rows of the tied embedding, the softmax over that span and its winner.
//   logits[r][i] = < dh[r], emb[lang_begin + i] >   (f32 accumulation),  probs[r] = softmax(logits[r]),  best[r] = first argmax
// No atomics; the lane -> element mapping and every reduction order are fixed: bit-reproducible, and independent of the
// other rows of the launch.
#include "common.hpp"

constexpr int LANG_MAX = 128;      // widest span (the C ABI refuses more)
constexpr int LANG_THREADS = 1024; // 16 waves: wave w takes languages w, w + 16, ...

struct OpMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };

// NCH = 16-byte chunks per lane that cover the widest row (d <= 1280): lane l owns chunks l, l + 64, ...; chunk c holds the
// elements [c * VEC, (c + 1) * VEC).  d is a multiple of 64, so a row is a whole number of chunks, but not of 64 chunks:
// large-v3 (1280) is 2.5 chunks per lane in 16-bit storage, micro (128) leaves 48 lanes without one - the chunks past the
// row are never loaded and count as zero.
// The head of ONE row, shared by the static and the session kernel (same arithmetic, same order): the span logits of activation
// row `xrow` go through s_logit; wave 0 writes the softmax to prow (and the logits to lrow, unless NULL) and returns the first
// maximum in all its lanes; the other waves return -1 behind the barrier.
template <typename T>
__device__ __forceinline__ int lang_head_row(const T* __restrict__ xrow, const T* __restrict__ emb, int d, int lang_begin, int n_lang,
                                             float* __restrict__ prow, float* __restrict__ lrow, float* s_logit) {
  constexpr int VEC = RowVec<T>::VEC, NCH = (1280 / VEC + 63) / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_chunk = d / VEC;
  // the activation row and this wave's first language row, one batch of loads
  float x[NCH][VEC], w[NCH][VEC];
  const T* wrow = emb + (int64_t)(lang_begin + min(wave, n_lang - 1)) * d;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int c = lane + 64 * j;
    if (c < n_chunk) { RowVec<T>::load(xrow + c * VEC, x[j]); RowVec<T>::load(wrow + c * VEC, w[j]); }
    else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) { x[j][e] = 0.f; w[j][e] = 0.f; }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  for (int l = wave; l < n_lang; l += LANG_THREADS / 64) {
    // the next language row of this wave is requested before this one is reduced (the last iteration re-reads its own row)
    float wn[NCH][VEC];
    const T* nrow = emb + (int64_t)(lang_begin + min(l + LANG_THREADS / 64, n_lang - 1)) * d;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int c = lane + 64 * j;
      if (c < n_chunk) RowVec<T>::load(nrow + c * VEC, wn[j]);
      else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) wn[j][e] = 0.f;
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc = fmaf(x[j][e], w[j][e], acc);
    acc = wave_sum(acc);
    if (lane == 0) s_logit[l] = acc;
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) w[j][e] = wn[j][e];
  }
  __syncthreads();
  if (wave != 0) return -1;
  // softmax over the span and its first maximum: lane i holds entries i and i + 64
  const int i0 = lane, i1 = lane + 64;
  const float v0 = i0 < n_lang ? s_logit[i0] : -INFINITY, v1 = i1 < n_lang ? s_logit[i1] : -INFINITY;
  const float m = wave_max(fmaxf(v0, v1));
  const float e0 = i0 < n_lang ? expf(v0 - m) : 0.f, e1 = i1 < n_lang ? expf(v1 - m) : 0.f;
  const float inv = 1.f / wave_sum(e0 + e1);
  const float first = group_reduce<64>(v0 == m ? (float)i0 : (v1 == m ? (float)i1 : (float)LANG_MAX), OpMin{});
  if (i0 < n_lang) prow[i0] = e0 * inv;
  if (i1 < n_lang) prow[i1] = e1 * inv;
  if (lrow) {
    if (i0 < n_lang) lrow[i0] = v0;
    if (i1 < n_lang) lrow[i1] = v1;
  }
  return (int)first;
}

template <typename T>
__global__ __launch_bounds__(LANG_THREADS) void lang_head_kernel(const T* __restrict__ dh_, const T* __restrict__ emb_, int d_,
                                                                 int lang_begin_, int n_lang_, float* __restrict__ probs_,
                                                                 int32_t* __restrict__ best_, float* __restrict__ logits_) {
  __shared__ float s_logit[LANG_MAX];
  const T* dh = sgpr_pin_ptr(dh_); const T* emb = sgpr_pin_ptr(emb_);
  float* probs = sgpr_pin_ptr(probs_); int32_t* best = sgpr_pin_ptr(best_); float* logits = sgpr_pin_ptr(logits_);
  const int d = sgpr_pin(d_), lang_begin = sgpr_pin(lang_begin_), n_lang = sgpr_pin(n_lang_);
  const int r = blockIdx.x;
  const int first = lang_head_row<T>(dh + (int64_t)r * d, emb, d, lang_begin, n_lang, probs + (int64_t)r * n_lang,
                                     logits ? logits + (int64_t)r * n_lang : nullptr, s_logit);
  if (threadIdx.x == 0) best[r] = first;
}

// The session form (engine_refill.hip): one workgroup per row of the step, behind the step's last kernel.
// A row whose pending flag is 0 leaves before anything else is loaded.  A pending row has just run position 0 with
// <|startoftranscript|>: its final LayerNorm row is in dh.  Results go to the row's own slots of best / probs / logits (rows packed
// at n_lang).  Greedy session (a.prompt != NULL): thread 0 also writes the winner's token over the placeholder in the row's
// device prompt and restarts the row - fed token prompt[0], position 0, flag cleared - so the next step (of the same graph,
// possibly) decodes the clip as if the language had been given.  Beam session (a.prompt == NULL): flags and positions are the
// host's; only the results are written.
template <typename T>
__global__ __launch_bounds__(LANG_THREADS) void lang_head_rows_kernel(const T* __restrict__ dh_, const T* __restrict__ emb_, int d_,
                                                                      int lang_begin_, int n_lang_, LangRows a) {
  const int r = blockIdx.x;
  if (a.pending[r] == 0) return;   // uniform; nothing is loaded before it
  __shared__ float s_logit[LANG_MAX];
  const T* dh = sgpr_pin_ptr(dh_); const T* emb = sgpr_pin_ptr(emb_);
  const int d = sgpr_pin(d_), lang_begin = sgpr_pin(lang_begin_), n_lang = sgpr_pin(n_lang_);
  const int first = lang_head_row<T>(dh + (int64_t)r * d, emb, d, lang_begin, n_lang, a.probs + (int64_t)r * n_lang,
                                     a.logits + (int64_t)r * n_lang, s_logit);
  if (threadIdx.x != 0) return;
  a.best[r] = first;
  if (!a.prompt) return;
  int32_t* prow = a.prompt + (int64_t)r * a.max_prompt;
  const int slot = a.slot[r];
  if (slot > 0 && slot < a.max_prompt) prow[slot] = lang_begin + first;   // (the host validated the slot; never write outside the row)
  a.cur_tok[r] = prow[0];
  a.row_pos[r] = 0;
  a.pending[r] = 0;
}

// Admission of detecting rows (greedy session): entry e of tab = {row, slot}; the row is fed `sot` at position 0 and its flag raised.
// Runs behind admit_rows_kernel on the decode stream.
__global__ __launch_bounds__(64) void lang_admit_rows_kernel(const int32_t* __restrict__ tab, int n, int B, int sot, int32_t* __restrict__ pending,
                                                             int32_t* __restrict__ slot, int32_t* __restrict__ cur_tok) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  const int row = tab[2 * e];
  if (row < 0 || row >= B) return;
  slot[row] = tab[2 * e + 1];
  cur_tok[row] = sot;
  pending[row] = 1;
}
void launch_lang_admit_rows(const int32_t* tab, int n, int B, int sot, int32_t* pending, int32_t* slot, int32_t* cur_tok, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(lang_admit_rows_kernel, dim3((n + 63) / 64), dim3(64), 0, s, tab, n, B, sot, pending, slot, cur_tok);
}

template <typename T>
void launch_lang_head_rows(const T* dh, const T* emb, int rows, int d, int V, int lang_begin, int n_lang, const LangRows& a, hipStream_t s) {
  if (rows < 1 || d < 64 || d % 64 || d > 1280 || n_lang < 1 || n_lang > LANG_MAX || lang_begin < 0 || lang_begin > V - n_lang ||
      !a.pending || !a.best || !a.probs || !a.logits || (a.prompt && (!a.slot || !a.cur_tok || !a.row_pos || a.max_prompt < 2))) {
    launch_fault("lang_head_rows: rows %d, d %d, span [%d, %d + %d) of %d", rows, d, lang_begin, lang_begin, n_lang, V);
    return;
  }
  hipLaunchKernelGGL(lang_head_rows_kernel<T>, dim3(rows), dim3(LANG_THREADS), 0, s, dh, emb, d, lang_begin, n_lang, a);
}
template void launch_lang_head_rows<float>(const float*, const float*, int, int, int, int, int, const LangRows&, hipStream_t);
template void launch_lang_head_rows<bf16_t>(const bf16_t*, const bf16_t*, int, int, int, int, int, const LangRows&, hipStream_t);
template void launch_lang_head_rows<f16_t>(const f16_t*, const f16_t*, int, int, int, int, int, const LangRows&, hipStream_t);

template <typename T>
void launch_lang_head(const T* dh, const T* emb, int rows, int d, int V, int lang_begin, int n_lang, float* probs, int32_t* best,
                      float* logits, hipStream_t s) {
  if (rows < 1 || d < 64 || d % 64 || d > 1280 || n_lang < 1 || n_lang > LANG_MAX || lang_begin < 0 || lang_begin > V - n_lang) {
    launch_fault("lang_head: rows %d, d %d, span [%d, %d + %d) of %d", rows, d, lang_begin, lang_begin, n_lang, V);
    return;
  }
  hipLaunchKernelGGL(lang_head_kernel<T>, dim3(rows), dim3(LANG_THREADS), 0, s, dh, emb, d, lang_begin, n_lang, probs, best, logits);
}
template void launch_lang_head<float>(const float*, const float*, int, int, int, int, int, float*, int32_t*, float*, hipStream_t);
template void launch_lang_head<bf16_t>(const bf16_t*, const bf16_t*, int, int, int, int, int, float*, int32_t*, float*, hipStream_t);
template void launch_lang_head<f16_t>(const f16_t*, const f16_t*, int, int, int, int, int, float*, int32_t*, float*, hipStream_t);
