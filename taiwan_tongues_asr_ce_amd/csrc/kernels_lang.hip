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
template <typename T>
__global__ __launch_bounds__(LANG_THREADS) void lang_head_kernel(const T* __restrict__ dh_, const T* __restrict__ emb_, int d_,
                                                                 int lang_begin_, int n_lang_, float* __restrict__ probs_,
                                                                 int32_t* __restrict__ best_, float* __restrict__ logits_) {
  constexpr int VEC = RowVec<T>::VEC, NCH = (1280 / VEC + 63) / 64;
  __shared__ float s_logit[LANG_MAX];
  const T* dh = sgpr_pin_ptr(dh_); const T* emb = sgpr_pin_ptr(emb_);
  float* probs = sgpr_pin_ptr(probs_); int32_t* best = sgpr_pin_ptr(best_); float* logits = sgpr_pin_ptr(logits_);
  const int d = sgpr_pin(d_), lang_begin = sgpr_pin(lang_begin_), n_lang = sgpr_pin(n_lang_);
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_chunk = d / VEC;
  // the activation row and this wave's first language row, one batch of loads
  float x[NCH][VEC], w[NCH][VEC];
  const T* xrow = dh + (int64_t)r * d;
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
  if (wave != 0) return;
  // softmax over the span and its first maximum: lane i holds entries i and i + 64
  const int i0 = lane, i1 = lane + 64;
  const float v0 = i0 < n_lang ? s_logit[i0] : -INFINITY, v1 = i1 < n_lang ? s_logit[i1] : -INFINITY;
  const float m = wave_max(fmaxf(v0, v1));
  const float e0 = i0 < n_lang ? expf(v0 - m) : 0.f, e1 = i1 < n_lang ? expf(v1 - m) : 0.f;
  const float inv = 1.f / wave_sum(e0 + e1);
  const float first = group_reduce<64>(v0 == m ? (float)i0 : (v1 == m ? (float)i1 : (float)LANG_MAX), OpMin{});
  float* prow = probs + (int64_t)r * n_lang;
  if (i0 < n_lang) prow[i0] = e0 * inv;
  if (i1 < n_lang) prow[i1] = e1 * inv;
  if (logits) {
    float* lrow = logits + (int64_t)r * n_lang;
    if (i0 < n_lang) lrow[i0] = v0;
    if (i1 < n_lang) lrow[i1] = v1;
  }
  if (lane == 0) best[r] = (int)first;
}

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
