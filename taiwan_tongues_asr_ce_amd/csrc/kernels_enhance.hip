// Audio enhancement (include/ttasr.h ttasr_enhance): denoise, high-pass and level one float32 mono 16 kHz recording, length kept.
//
// The definition (restated from the header; tests/enhance_cases.py pins it in float64).  N = 512, hop 128, bins k = 0..256, window
// w[n] = sin(pi (n + 0.5) / N) for analysis and synthesis (its shifted squares sum to 2).  L < N: out = x.  Otherwise
//   1. T = ceil(L / 128) + 3 frames; frame t reads samples t 128 - 384 + n, reflected without repeating the edge (s < 0 -> -s,
//      s >= L -> 2 (L - 1) - s): every sample lies in exactly four frames
//   2. X[t,k] = sum_n w[n] x_t[n] e^{-2 pi i k n / N}, P = |X|^2
//   3. S = box mean of P along t, radius 2; Q = box mean, radius 16; both clipped to [0, T - 1], divided by the frames summed
//   4. M[b,k] = min of Q over the 32 frames of block b; Nf[t,k] = oversubtract * min of M[b',k] over the blocks within 6 of t's
//   5. DENOISE: G = max(1 - Nf / S, 0) where S > 0, else 0; then G = max(G, 10^(-strength_db / 20)).  Without the flag G = 1
//   6. HIGHPASS: G[t,0] = G[t,1] = 0
//   7. y_t[n] = w[n] Re IDFT(G X)[n]; out[s] = 0.5 * the sum over the four frames that hold s, ascending t
//   8. LEVEL: p = max |out|, g = 1 if p == 0 else min(peak_target / p, max_gain), z = g out
//
// Both transforms are direct DFTs with table twiddles, the log-mel kernel's pattern: samples staged coalesced into LDS once per
// workgroup, thread k owns bin k for all frames of the workgroup, twiddle index k n mod 512 into a 512-entry (cos, sin) table in LDS.
// At N = 512 an LDS FFT would need 9 passes with a barrier each over 11 to 16 frames; the direct form has one barrier per stage and
// keeps a bin's whole time line - P of the neighbouring frames for S and Q - in the registers of one thread.  Bin 256 is the
// 257th of 256 threads: it is real, sum_n (-1)^n w[n] x[n], and is taken by a workgroup reduction in a fixed order.
//
//   enh_noise_kernel   one workgroup per block of 32 frames: the 64 frames Q of the block reads, in four batches of 16 -> P in LDS
//                      -> Q -> the block's minima M[b][257].  80 KiB of LDS: two workgroups per CU.
//   enh_gain_kernel    one workgroup per tile of 8 hops (1024 consecutive output samples, tile t covers [1024 t, 1024 t + 1024)
//                      whatever range a launch asks for): the 15 frames S reads -> S, Nf from M, G -> G X of the tile's 11 frames
//                      in LDS -> inverse DFT, thread n takes samples n and n + 256 from the even and the odd bins' sums -> windowed
//                      frames in LDS -> overlap-add of the four frames of every sample, ascending t.  The three halo frames are
//                      recomputed, no atomics: an output's operands and their order depend on its index alone, so neither the range
//                      of a launch (the host's chunks) nor the other recordings of a call can change a bit of it.  50 KiB of LDS.
//   enh_absmax_kernel / enh_level_kernel / enh_scale_kernel   the level stage: partial maxima, the gain, the scaling.
#include "common.hpp"
#include "enhance.hpp"

#include <mutex>

namespace {

constexpr int kNoiseNF = 16;                                         // frames of one batch of the noise pass
constexpr int kNoiseSpan = (kNoiseNF - 1) * kEnhHop + kEnhN;         // 2432 staged samples
constexpr int kNoiseRows = kEnhBlock + 2 * kEnhRQ;                   // 64 frames of P
constexpr int kNoiseLds = 1024 + 512 + kNoiseSpan + 4 * kNoiseNF + kNoiseRows * kEnhBins;   // floats: 80 KiB
constexpr int kGainNF = kEnhTileHops + 3 + 2 * kEnhRS;               // 15 frames analysed
constexpr int kSynNF = kEnhTileHops + 3;                             // 11 frames synthesised
constexpr int kGainSpan = (kGainNF - 1) * kEnhHop + kEnhN;           // 2304 staged samples
constexpr int kYStride = 258;                                        // float2 per frame of G X: even, so that a bin pair is one 16-byte read
static_assert(kGainSpan <= kSynNF * kEnhN, "the staged samples share the windowed frames' buffer");

// xs[i] = x[s_lo + i] with the reflection of the definition; what one reflection does not bring inside the recording reads as zero
// (frames outside [0, T), whose spectra nobody uses)
__device__ __forceinline__ void enh_stage(const float* __restrict__ x, int64_t L, float* xs, int64_t s_lo, int span, int tid) {
  for (int i = tid; i < span; i += kEnhThreads) {
    int64_t s = s_lo + i;
    if (s < 0) s = -s;
    if (s >= L) s = 2 * (L - 1) - s;
    xs[i] = (s >= 0 && s < L) ? x[s] : 0.0f;
  }
}

// Bin `tid` of NF frames, frame f at xs + 128 f: re = sum a cos, im = sum a sin (a = w x; the spectrum is re - i im), n ascending,
// 32 terms at a time into a partial sum that is then added to the total
template <int NF>
__device__ __forceinline__ void enh_dft(const float* xs, const float2* tw, const float* win, int tid, float (&re)[NF], float (&im)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) { re[f] = 0.0f; im[f] = 0.0f; }
  int idx = 0;
  for (int n0 = 0; n0 < kEnhN; n0 += 32) {
    float pr[NF], pi[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { pr[f] = 0.0f; pi[f] = 0.0f; }
    for (int n = n0; n < n0 + 32; n += 4) {
      const float4 w = *(const float4*)(win + n);
      const float2 t0 = tw[idx]; idx = (idx + tid) & 511;
      const float2 t1 = tw[idx]; idx = (idx + tid) & 511;
      const float2 t2 = tw[idx]; idx = (idx + tid) & 511;
      const float2 t3 = tw[idx]; idx = (idx + tid) & 511;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const float4 v = *(const float4*)(xs + f * kEnhHop + n);
        const float a0 = v.x * w.x, a1 = v.y * w.y, a2 = v.z * w.z, a3 = v.w * w.w;
        pr[f] = fmaf(a0, t0.x, pr[f]); pi[f] = fmaf(a0, t0.y, pi[f]);
        pr[f] = fmaf(a1, t1.x, pr[f]); pi[f] = fmaf(a1, t1.y, pi[f]);
        pr[f] = fmaf(a2, t2.x, pr[f]); pi[f] = fmaf(a2, t2.y, pi[f]);
        pr[f] = fmaf(a3, t3.x, pr[f]); pi[f] = fmaf(a3, t3.y, pi[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) { re[f] += pr[f]; im[f] += pi[f]; }
  }
}

// Bin 256: every wave's part of sum_n (-1)^n a[n] to red[wave][f]; after a barrier the value of frame f is
// (red[0][f] + red[1][f]) + (red[2][f] + red[3][f]) (enh_nyquist)
template <int NF>
__device__ __forceinline__ void enh_nyquist_parts(const float* xs, const float* win, int tid, float* red) {
  const float sg = (tid & 1) ? -1.0f : 1.0f, w0 = win[tid], w1 = win[tid + 256];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const float p = wave_sum(sg * (xs[f * kEnhHop + tid] * w0 + xs[f * kEnhHop + tid + 256] * w1));
    if ((tid & 63) == 0) red[(tid >> 6) * NF + f] = p;
  }
}
template <int NF>
__device__ __forceinline__ float enh_nyquist(const float* red, int f) {
  return (red[f] + red[NF + f]) + (red[2 * NF + f] + red[3 * NF + f]);
}

__global__ __launch_bounds__(kEnhThreads) void enh_noise_kernel(const EnhRec r, const int64_t b0) {
  extern __shared__ __align__(16) float lds[];
  float2* tw = (float2*)lds;
  float* win = lds + 1024;
  float* xs = win + 512;
  float* red = xs + kNoiseSpan;
  float* P = red + 4 * kNoiseNF;   // [64][257]: row i is frame base + i
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.x, T = enh_frames(r.L), base = b * kEnhBlock - kEnhRQ;
  for (int i = tid; i < 512; i += kEnhThreads) { tw[i] = r.tw[i]; win[i] = r.win[i]; }
  for (int q = 0; q < kNoiseRows / kNoiseNF; ++q) {
    const int64_t u0 = base + q * kNoiseNF;
    if (u0 + kNoiseNF - 1 < 0 || u0 >= T) continue;   // no frame of the batch exists (the same in every thread)
    __syncthreads();   // the batch before has read xs and red
    enh_stage(r.x, r.L, xs, u0 * kEnhHop - 384, kNoiseSpan, tid);
    __syncthreads();
    float re[kNoiseNF], im[kNoiseNF];
    enh_dft<kNoiseNF>(xs, tw, win, tid, re, im);
    enh_nyquist_parts<kNoiseNF>(xs, win, tid, red);
#pragma unroll
    for (int f = 0; f < kNoiseNF; ++f) P[(q * kNoiseNF + f) * kEnhBins + tid] = re[f] * re[f] + im[f] * im[f];
    __syncthreads();
    if (tid < kNoiseNF) {
      const float v = enh_nyquist<kNoiseNF>(red, tid);
      P[(q * kNoiseNF + tid) * kEnhBins + 256] = v * v;
    }
  }
  __syncthreads();
  for (int k = tid; k < kEnhBins; k += kEnhThreads) {   // thread 0 takes bin 256 too
    float m = INFINITY;
    for (int j = 0; j < kEnhBlock; ++j) {
      const int64_t t = b * kEnhBlock + j;
      if (t >= T) break;
      const int64_t lo = max(t - kEnhRQ, (int64_t)0), hi = min(t + kEnhRQ, T - 1);
      float acc = 0.0f;
      for (int64_t u = lo; u <= hi; ++u) acc += P[(int)(u - base) * kEnhBins + k];
      m = fminf(m, acc / (float)(hi - lo + 1));
    }
    r.M[b * kEnhBins + k] = m;
  }
}

// Bin k of the tile's frames: S from the P of the 15 analysed frames (P[i], xr[i], xi[i] belong to frame h0 - 2 + i), Nf from the
// block minima, G, and G X - scaled by 1 / N, twice that for the bins the Hermitian extension doubles - into Y
__device__ __forceinline__ void enh_bin(const EnhRec& r, const EnhGain& g, const EnhTaps& taps, int64_t h0, int64_t T, int64_t NB, int k,
                                        const float (&P)[kGainNF], const float (&xr)[kGainNF], const float (&xi)[kGainNF], float2* Y) {
  const float scale = (k == 0 || k == 256) ? 1.0f / kEnhN : 2.0f / kEnhN;
  const bool denoise = (g.flags & TTASR_DSP_DENOISE) != 0;
  int64_t b_have = -1;
  float mn = 0.0f;
#pragma unroll
  for (int j = 0; j < kSynNF; ++j) {
    const int64_t t = h0 + j;
    float2 y = make_float2(0.0f, 0.0f);
    if (t < T) {
      float acc = 0.0f;
      int cnt = 0;
#pragma unroll
      for (int d = -kEnhRS; d <= kEnhRS; ++d)
        if (t + d >= 0 && t + d < T) { acc += P[j + kEnhRS + d]; ++cnt; }
      const float S = acc / (float)cnt;
      float Nf = 0.0f, G = 1.0f;
      if (denoise || taps.Nf) {
        const int64_t b = t / kEnhBlock;
        if (b != b_have) {
          const int64_t lo = max(b - kEnhBlockWin, (int64_t)0), hi = min(b + kEnhBlockWin, NB - 1);
          mn = r.M[lo * kEnhBins + k];
          for (int64_t bb = lo + 1; bb <= hi; ++bb) mn = fminf(mn, r.M[bb * kEnhBins + k]);
          b_have = b;
        }
        Nf = g.oversubtract * mn;
      }
      if (denoise) G = fmaxf(S > 0.0f ? fmaxf(1.0f - Nf / S, 0.0f) : 0.0f, g.floor_gain);
      if ((g.flags & TTASR_DSP_HIGHPASS) && k < 2) G = 0.0f;
      y = make_float2(G * xr[j + kEnhRS] * scale, G * xi[j + kEnhRS] * scale);
      if (j >= 3 || h0 == 0) {   // every frame is written by one tile: the tile whose last eight frames hold it, the first three by tile 0
        if (taps.S) taps.S[t * kEnhBins + k] = S;
        if (taps.Nf) taps.Nf[t * kEnhBins + k] = Nf;
        if (taps.G) taps.G[t * kEnhBins + k] = G;
      }
    }
    Y[j * kYStride + k] = y;
  }
}

__global__ __launch_bounds__(kEnhThreads) void enh_gain_kernel(const EnhRec r, const EnhGain g, const EnhTaps taps, float* __restrict__ out,
                                                               const int64_t tile_lo, const int64_t s0, const int64_t s1) {
  __shared__ __align__(16) float2 tw[512];
  __shared__ __align__(16) float win[512];
  __shared__ __align__(16) float2 Y[kSynNF * kYStride];
  __shared__ __align__(16) float buf[kSynNF * kEnhN];   // the staged samples, later the windowed frames [11][512]
  __shared__ float red[4 * kGainNF];
  const int tid = threadIdx.x;
  const int64_t tile = tile_lo + blockIdx.x, h0 = tile * kEnhTileHops, T = enh_frames(r.L), NB = enh_blocks(T);
  for (int i = tid; i < 512; i += kEnhThreads) { tw[i] = r.tw[i]; win[i] = r.win[i]; }
  enh_stage(r.x, r.L, buf, (h0 - kEnhRS) * kEnhHop - 384, kGainSpan, tid);
  __syncthreads();
  {
    float re[kGainNF], im[kGainNF], P[kGainNF];
    enh_dft<kGainNF>(buf, tw, win, tid, re, im);
    enh_nyquist_parts<kGainNF>(buf, win, tid, red);
#pragma unroll
    for (int f = 0; f < kGainNF; ++f) P[f] = re[f] * re[f] + im[f] * im[f];
    enh_bin(r, g, taps, h0, T, NB, tid, P, re, im, Y);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int f = 0; f < kGainNF; ++f) { re[f] = enh_nyquist<kGainNF>(red, f); im[f] = 0.0f; P[f] = re[f] * re[f]; }
      enh_bin(r, g, taps, h0, T, NB, 256, P, re, im, Y);
    }
  }
  __syncthreads();
  {
    // samples n = tid and n + 256 of every frame: cos and sin of 2 pi k (n + 256) / N are (-1)^k times those of n, so the even
    // bins' sum E and the odd bins' sum O give E + O and E - O; k ascending in each
    float ev[kSynNF], od[kSynNF];
#pragma unroll
    for (int j = 0; j < kSynNF; ++j) { ev[j] = 0.0f; od[j] = 0.0f; }
    int idx = 0;
    for (int k = 0; k < 256; k += 2) {
      const float2 te = tw[idx]; idx = (idx + tid) & 511;
      const float2 to = tw[idx]; idx = (idx + tid) & 511;
#pragma unroll
      for (int j = 0; j < kSynNF; ++j) {
        const float4 y = *(const float4*)(Y + j * kYStride + k);
        ev[j] = fmaf(y.x, te.x, fmaf(y.y, te.y, ev[j]));
        od[j] = fmaf(y.z, to.x, fmaf(y.w, to.y, od[j]));
      }
    }
    const float c256 = tw[idx].x;   // idx = 256 n mod 512: (-1)^n
    const float w0 = win[tid], w1 = win[tid + 256];
#pragma unroll
    for (int j = 0; j < kSynNF; ++j) {
      const float e = fmaf(Y[j * kYStride + 256].x, c256, ev[j]);
      buf[j * kEnhN + tid] = (e + od[j]) * w0;
      buf[j * kEnhN + tid + 256] = (e - od[j]) * w1;
    }
  }
  __syncthreads();
  const int64_t tile0 = tile * kEnhTile;
  for (int p = tid; p < kEnhTile; p += kEnhThreads) {
    const int64_t s = tile0 + p;
    if (s < s0 || s >= s1) continue;
    const int f = p >> 7, q = p & 127;   // frames h0 + f .. h0 + f + 3 hold s, at n = 384 + q, 256 + q, 128 + q, q
    out[s] = 0.5f * (((buf[f * kEnhN + 384 + q] + buf[(f + 1) * kEnhN + 256 + q]) + buf[(f + 2) * kEnhN + 128 + q]) + buf[(f + 3) * kEnhN + q]);
  }
}

__global__ __launch_bounds__(kEnhThreads) void enh_absmax_kernel(const float* __restrict__ v, const int64_t s0, const int64_t s1,
                                                                 float* __restrict__ partial) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int64_t a = s0 + (int64_t)blockIdx.x * kEnhMaxSpan, e = min(a + kEnhMaxSpan, s1);
  float m = 0.0f;
  for (int64_t s = a + tid; s < e; s += kEnhThreads) m = fmaxf(m, fabsf(v[s]));
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(kEnhThreads) void enh_level_kernel(const float* __restrict__ partial, const int64_t n, const float peak_target,
                                                                const float max_gain, float* __restrict__ gain) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float m = 0.0f;
  for (int64_t i = tid; i < n; i += kEnhThreads) m = fmaxf(m, partial[i]);
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    const float p = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    *gain = p == 0.0f ? 1.0f : fminf(peak_target / p, max_gain);
  }
}

__global__ __launch_bounds__(kEnhThreads) void enh_scale_kernel(float* __restrict__ v, const int64_t s0, const int64_t s1,
                                                                const float* __restrict__ gain) {
  const float g = *gain;
  const int64_t s = s0 + (int64_t)blockIdx.x * kEnhThreads + threadIdx.x;
  if (s < s1) v[s] = g * v[s];
}

}  // namespace

void launch_enh_noise(const EnhRec& r, int64_t b0, int64_t b1, hipStream_t s) {
  if (b1 <= b0) return;
  const int64_t NB = enh_blocks(enh_frames(r.L));
  if (r.L < kEnhN || r.L > kEnhMaxSamples || b0 < 0 || b1 > NB || !r.x || !r.M || !r.tw || !r.win) {
    launch_fault("enh_noise: blocks [%lld, %lld) of %lld, %lld samples", (long long)b0, (long long)b1, (long long)NB, (long long)r.L);
    return;
  }
  // more than 64 KiB of dynamic LDS needs the opt-in, once per device
  static std::once_flag once[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::call_once(once[dev & 63], []() {
    (void)hipFuncSetAttribute((const void*)enh_noise_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kNoiseLds * 4);
  });
  enh_noise_kernel<<<(unsigned)(b1 - b0), kEnhThreads, (size_t)kNoiseLds * 4, s>>>(r, b0);
}

void launch_enh_gain(const EnhRec& r, const EnhGain& g, const EnhTaps& taps, float* out, int64_t s0, int64_t s1, hipStream_t s) {
  if (s1 <= s0) return;
  if (r.L < kEnhN || r.L > kEnhMaxSamples || s0 < 0 || s1 > r.L || !r.x || !r.tw || !r.win || !out ||
      (((g.flags & TTASR_DSP_DENOISE) || taps.Nf) && !r.M)) {
    launch_fault("enh_gain: samples [%lld, %lld) of %lld, flags %d", (long long)s0, (long long)s1, (long long)r.L, g.flags);
    return;
  }
  const int64_t tile_lo = s0 / kEnhTile, tile_hi = (s1 + kEnhTile - 1) / kEnhTile;
  enh_gain_kernel<<<(unsigned)(tile_hi - tile_lo), kEnhThreads, 0, s>>>(r, g, taps, out, tile_lo, s0, s1);
}

int64_t launch_enh_absmax(const float* v, int64_t s0, int64_t s1, float* partial, hipStream_t s) {
  if (s1 <= s0) return 0;
  const int64_t n = (s1 - s0 + kEnhMaxSpan - 1) / kEnhMaxSpan;
  enh_absmax_kernel<<<(unsigned)n, kEnhThreads, 0, s>>>(v, s0, s1, partial);
  return n;
}

void launch_enh_level(const float* partial, int64_t n_partial, float peak_target, float max_gain, float* gain, hipStream_t s) {
  enh_level_kernel<<<1, kEnhThreads, 0, s>>>(partial, n_partial, peak_target, max_gain, gain);
}

void launch_enh_scale(float* v, int64_t s0, int64_t s1, const float* gain, hipStream_t s) {
  if (s1 <= s0) return;
  enh_scale_kernel<<<(unsigned)((s1 - s0 + kEnhThreads - 1) / kEnhThreads), kEnhThreads, 0, s>>>(v, s0, s1, gain);
}
