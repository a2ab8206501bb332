// Segmentation VAD network (PyanNet shape; include/ttasr.h ttasr_seg_*), all f32, over a group of chunks of 80 000 samples:
//
//   seg_stats_kernel    mean and 1 / sqrt(var + eps) of a row (the chunk's waveform, or one channel of a stage), two passes, every
//                       sum in a fixed order: a thread's strided partial sum, then a fixed LDS tree.  No atomics anywhere.
//   seg_sinc_kernel     waveform norm -> sinc convolution (251 taps, stride 10) -> abs -> MaxPool(3): a workgroup owns 64 pooled
//                       outputs of all 80 channels; the 7 975 x 80 convolution output is never written.
//   seg_conv_kernel     previous stage's InstanceNorm + leaky_relu on load -> Conv1d(k 5) -> MaxPool(3), 64 pooled outputs x 60
//                       channels per workgroup.
//   seg_proj_kernel     a layer's input projection for all 293 frames and both directions: gx = (b_ih + b_hh) + W_ih x, k ascending.
//   seg_lstm_kernel<R>  the recurrence: one workgroup of 512 threads per (R chunks, direction); thread r keeps row r of W_hh in
//                       registers for the whole launch and uses it for R hidden vectors between the same two barriers.  A gate
//                       row's sum has the same order for every R.
//   seg_head_kernel     Linear 256 -> 128 -> 128 -> C, sigmoid, and the maximum over classes, 8 frames per workgroup.
//   seg_agg_kernel      the overlap-add of chunk scores into recording frames, gather form: one thread per output frame, chunks
//                       ascending.
//
// Every kernel's form is a function of the chunk only: the tiles never straddle two chunks, and the number of chunks in the group
// decides grid sizes alone.  Every multiply-add is written as fmaf and the file is compiled with -ffp-contract=off (Makefile), so
// that no instantiation of a template contracts an expression another one leaves alone: the recurrence forms agree bit for bit.
#include "common.hpp"
#include "seg.hpp"

namespace {

constexpr float kEps = 1e-5f;
__device__ __forceinline__ float seg_lrelu(float v) { return v > 0.f ? v : 0.01f * v; }
__device__ __forceinline__ float seg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the sum of one value per thread of a 256-thread workgroup, in a fixed tree; every thread receives it
__device__ __forceinline__ float block_sum_256(float v, float* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();   // the previous use of s_red is over
  s_red[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s_red[tid] += s_red[tid + w];
    __syncthreads();
  }
  return s_red[0];
}

// One row per workgroup.  desc != nullptr: row i is the chunk's waveform x + desc[i].off, desc[i].nvalid samples and zeros up to L;
// else row i is x + i * L.  out[i] = {mean, 1 / sqrt(biased variance + eps)}.
__global__ __launch_bounds__(256) void seg_stats_kernel(const float* __restrict__ x, const SegDesc* __restrict__ desc, int L,
                                                        float* __restrict__ out) {
  __shared__ float s_red[256];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* p = desc ? x + desc[row].off : x + (size_t)row * L;
  const int nv = desc ? desc[row].nvalid : L;
  float a = 0.f;
  for (int i = tid; i < nv; i += 256) a += p[i];
  const float mean = block_sum_256(a, s_red) / (float)L;
  float q = 0.f;
  for (int i = tid; i < L; i += 256) {
    const float d = (i < nv ? p[i] : 0.f) - mean;
    q = fmaf(d, d, q);
  }
  const float var = block_sum_256(q, s_red) / (float)L;
  if (tid == 0) { out[2 * row] = mean; out[2 * row + 1] = 1.f / sqrtf(var + kEps); }
}

constexpr int SP = 64;                                              // pooled outputs per workgroup
constexpr int SINC_X = 30 * (SP - 1) + 2 * kSegStride + kSegTaps;   // 2161 samples under them
constexpr int SINC_CG = kSegC1 / 4;                                 // 20 channels per wave

__global__ __launch_bounds__(256) void seg_sinc_kernel(SegWeights w, SegBuffers b) {
  __shared__ float s_x[SINC_X];
  const int chunk = blockIdx.y, p0 = blockIdx.x * SP, tid = threadIdx.x;
  const SegDesc d = b.desc[chunk];
  const float* pcm = b.pcm + d.off;
  const float mean = b.st0[2 * chunk], scale = b.st0[2 * chunk + 1] * w.wav_w[0], shift = w.wav_b[0];
  for (int i = tid; i < SINC_X; i += 256) {
    const int g = 30 * p0 + i;
    const float v = g < d.nvalid ? pcm[g] : 0.f;
    s_x[i] = g < kSegChunk ? fmaf(v - mean, scale, shift) : 0.f;   // past the chunk: read by no output that is stored
  }
  __syncthreads();
  const int p = tid & 63, cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  float acc[3][SINC_CG];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int c = 0; c < SINC_CG; ++c) acc[t][c] = 0.f;
  const float* wt = w.sinc_t + cg * SINC_CG;
  const float* xs = s_x + 30 * p;
  for (int k = 0; k < kSegTaps; ++k) {   // y[c][u] = sum_k filt[c][k] x[10 u + k], k ascending
    const float x0 = xs[k], x1 = xs[k + 10], x2 = xs[k + 20];
#pragma unroll
    for (int c = 0; c < SINC_CG; ++c) {
      const float wv = wt[k * kSegC1 + c];   // uniform over the wave
      acc[0][c] = fmaf(wv, x0, acc[0][c]);
      acc[1][c] = fmaf(wv, x1, acc[1][c]);
      acc[2][c] = fmaf(wv, x2, acc[2][c]);
    }
  }
  if (p0 + p < kSegL1) {
#pragma unroll
    for (int c = 0; c < SINC_CG; ++c)
      b.a1[((size_t)chunk * kSegC1 + cg * SINC_CG + c) * kSegL1 + p0 + p] = fmaxf(fmaxf(fabsf(acc[0][c]), fabsf(acc[1][c])), fabsf(acc[2][c]));
  }
}

constexpr int CONV_X = 3 * SP + 4;    // 196 inputs of a channel under 64 pooled outputs
constexpr int CONV_CG = kSegC2 / 4;   // 15 output channels per wave

// in [n][CIN][LIN] with its stats and norm -> out [n][60][LP], LP = (LIN - 4) / 3
template <int CIN, int LIN, int LP>
__global__ __launch_bounds__(256) void seg_conv_kernel(const float* __restrict__ in, const float* __restrict__ st,
                                                       const float* __restrict__ nw, const float* __restrict__ nb,
                                                       const float* __restrict__ wt, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
  __shared__ float s_x[CIN * CONV_X];
  const int chunk = blockIdx.y, p0 = blockIdx.x * SP, tid = threadIdx.x;
  for (int i = tid; i < CIN * CONV_X; i += 256) {
    const int c = i / CONV_X, g = 3 * p0 + i % CONV_X;
    float v = 0.f;
    if (g < LIN) {
      const float mean = st[2 * (chunk * CIN + c)], rstd = st[2 * (chunk * CIN + c) + 1];
      v = seg_lrelu(fmaf((in[((size_t)chunk * CIN + c) * LIN + g] - mean) * rstd, nw[c], nb[c]));
    }
    s_x[i] = v;
  }
  __syncthreads();
  const int p = tid & 63, cg = __builtin_amdgcn_readfirstlane(tid >> 6);
  float acc[3][CONV_CG];
#pragma unroll
  for (int o = 0; o < CONV_CG; ++o) { const float bv = bias[cg * CONV_CG + o]; acc[0][o] = bv; acc[1][o] = bv; acc[2][o] = bv; }
  for (int c = 0; c < CIN; ++c) {   // y[o][u] = bias[o] + sum_c sum_j w[o][c][j] x[c][u + j], c ascending, j ascending
    float v[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] = s_x[c * CONV_X + 3 * p + i];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const float* wj = wt + (size_t)(c * 5 + j) * kSegC2 + cg * CONV_CG;
#pragma unroll
      for (int o = 0; o < CONV_CG; ++o) {
        const float wv = wj[o];   // uniform over the wave
        acc[0][o] = fmaf(wv, v[j], acc[0][o]);
        acc[1][o] = fmaf(wv, v[j + 1], acc[1][o]);
        acc[2][o] = fmaf(wv, v[j + 2], acc[2][o]);
      }
    }
  }
  if (p0 + p < LP) {
#pragma unroll
    for (int o = 0; o < CONV_CG; ++o)
      out[((size_t)chunk * kSegC2 + cg * CONV_CG + o) * LP + p0 + p] = fmaxf(fmaxf(acc[0][o], acc[1][o]), acc[2][o]);
  }
}

constexpr int PT = 32;   // frames per workgroup of the projection

// FIRST: x[t][k] = leaky_relu(norm(a3[chunk][k][t])), K = 60; else x = y_in[chunk][t][0 .. 256)
template <bool FIRST>
__global__ __launch_bounds__(256) void seg_proj_kernel(const float* __restrict__ wih_t, const float* __restrict__ gate_b,
                                                       const float* __restrict__ in, const float* __restrict__ st,
                                                       const float* __restrict__ nw, const float* __restrict__ nb,
                                                       float* __restrict__ gx) {
  constexpr int K = FIRST ? kSegC2 : 2 * kSegHid;
  __shared__ __attribute__((aligned(16))) float s_x[PT * K];
  const int chunk = blockIdx.z, t0 = blockIdx.x * PT, tid = threadIdx.x;
  for (int i = tid; i < PT * K; i += 256) {
    float v = 0.f;
    if (FIRST) {
      const int r = i % PT, k = i / PT;
      if (t0 + r < kSegT) {
        const float mean = st[2 * (chunk * K + k)], rstd = st[2 * (chunk * K + k) + 1];
        v = seg_lrelu(fmaf((in[((size_t)chunk * K + k) * kSegT + t0 + r] - mean) * rstd, nw[k], nb[k]));
      }
      s_x[r * K + k] = v;
    } else {
      const int r = i / K, k = i % K;
      if (t0 + r < kSegT) v = in[((size_t)chunk * kSegT + t0 + r) * K + k];
      s_x[i] = v;
    }
  }
  __syncthreads();
  const int n = blockIdx.y * 256 + tid;   // gate row of direction n / 512
  float acc[PT];
  const float bv = gate_b[n];
#pragma unroll
  for (int r = 0; r < PT; ++r) acc[r] = bv;
  for (int k = 0; k < K; k += 4) {
    const float w0 = wih_t[(size_t)(k + 0) * 1024 + n], w1 = wih_t[(size_t)(k + 1) * 1024 + n],
                w2 = wih_t[(size_t)(k + 2) * 1024 + n], w3 = wih_t[(size_t)(k + 3) * 1024 + n];
#pragma unroll
    for (int r = 0; r < PT; ++r) {
      const f32x4 xv = *(const f32x4*)(s_x + r * K + k);
      acc[r] = fmaf(w0, xv[0], acc[r]);
      acc[r] = fmaf(w1, xv[1], acc[r]);
      acc[r] = fmaf(w2, xv[2], acc[r]);
      acc[r] = fmaf(w3, xv[3], acc[r]);
    }
  }
  float* g = gx + (((size_t)chunk * 2 + (n >> 9)) * kSegT + t0) * 512 + (n & 511);
#pragma unroll
  for (int r = 0; r < PT; ++r)
    if (t0 + r < kSegT) g[(size_t)r * 512] = acc[r];
}

// 512 threads = 8 waves, 2 per SIMD: a wave may hold 256 VGPRs, 128 of them row r of W_hh.  Direction 1 walks frames 292 -> 0.
template <int R>
__global__ __launch_bounds__(512) void seg_lstm_kernel(const float* __restrict__ whh_f, const float* __restrict__ whh_b,
                                                       const float* __restrict__ gx, float* __restrict__ y, int n) {
  __shared__ __attribute__((aligned(16))) float s_h[R][kSegHid];
  __shared__ float s_g[R][512];
  const int dir = blockIdx.y, base = blockIdx.x * R, r = threadIdx.x;
  const float* whh = dir ? whh_b : whh_f;
  float wr[128];
#pragma unroll
  for (int k = 0; k < 128; k += 4) {
    const f32x4 v = *(const f32x4*)(whh + (size_t)r * 128 + k);
    wr[k] = v[0]; wr[k + 1] = v[1]; wr[k + 2] = v[2]; wr[k + 3] = v[3];
  }
  // a slot past the group's last chunk computes on that last chunk's gates and stores nothing
  const float* g[R];
  float cell[R], g_cur[R];
  const int t_first = dir ? kSegT - 1 : 0, t_step = dir ? -1 : 1;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    g[q] = gx + ((size_t)min(base + q, n - 1) * 2 + dir) * kSegT * 512 + r;
    cell[q] = 0.f;
    g_cur[q] = g[q][(size_t)t_first * 512];
    if (r < kSegHid) s_h[q][r] = 0.f;
  }
  __syncthreads();
  for (int s = 0; s < kSegT; ++s) {
    const int t = t_first + s * t_step;
    float g_next[R];
#pragma unroll
    for (int q = 0; q < R; ++q) g_next[q] = s + 1 < kSegT ? g[q][(size_t)(t + t_step) * 512] : 0.f;   // requested a frame ahead
    // gate row r of chunk q: gx + W_hh[r] . h, four interleaved partial sums (k mod 4), each k ascending, joined as (a0 + a1) + (a2 + a3)
    float a[R][4];
#pragma unroll
    for (int q = 0; q < R; ++q) { a[q][0] = 0.f; a[q][1] = 0.f; a[q][2] = 0.f; a[q][3] = 0.f; }
#pragma unroll
    for (int k = 0; k < 128; k += 4) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const f32x4 hv = *(const f32x4*)(&s_h[q][k]);
        a[q][0] = fmaf(wr[k], hv[0], a[q][0]);
        a[q][1] = fmaf(wr[k + 1], hv[1], a[q][1]);
        a[q][2] = fmaf(wr[k + 2], hv[2], a[q][2]);
        a[q][3] = fmaf(wr[k + 3], hv[3], a[q][3]);
      }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) s_g[q][r] = g_cur[q] + ((a[q][0] + a[q][1]) + (a[q][2] + a[q][3]));
    __syncthreads();   // gates complete; every read of h is done
    if (r < kSegHid) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const float gi = seg_sigmoid(s_g[q][r]), gf = seg_sigmoid(s_g[q][128 + r]), gg = tanhf(s_g[q][256 + r]),
                    go = seg_sigmoid(s_g[q][384 + r]);
        cell[q] = fmaf(gf, cell[q], gi * gg);
        const float h = go * tanhf(cell[q]);
        s_h[q][r] = h;
        if (base + q < n) y[((size_t)(base + q) * kSegT + t) * 256 + dir * kSegHid + r] = h;
      }
    }
    __syncthreads();   // h complete; every read of the gates is done
#pragma unroll
    for (int q = 0; q < R; ++q) g_cur[q] = g_next[q];
  }
}

constexpr int HF = 8;   // frames per workgroup of the head

__global__ __launch_bounds__(128) void seg_head_kernel(SegWeights w, const float* __restrict__ y, float* __restrict__ probs,
                                                       float* __restrict__ logits, float* __restrict__ score) {
  __shared__ float s_x[HF][256];
  __shared__ float s_1[HF][128];
  __shared__ float s_2[HF][128];
  __shared__ float s_p[HF][kSegMaxC];
  const int chunk = blockIdx.y, t0 = blockIdx.x * HF, j = threadIdx.x, C = w.classes;
  for (int i = j; i < HF * 256; i += 128) {
    const int f = i >> 8;
    s_x[f][i & 255] = t0 + f < kSegT ? y[((size_t)chunk * kSegT + t0 + f) * 256 + (i & 255)] : 0.f;
  }
  __syncthreads();
  float acc[HF];
#pragma unroll
  for (int f = 0; f < HF; ++f) acc[f] = w.lin_b[0][j];
  for (int k = 0; k < 256; ++k) {   // k ascending
    const float wv = w.lin_t[0][k * 128 + j];
#pragma unroll
    for (int f = 0; f < HF; ++f) acc[f] = fmaf(wv, s_x[f][k], acc[f]);
  }
#pragma unroll
  for (int f = 0; f < HF; ++f) { s_1[f][j] = seg_lrelu(acc[f]); acc[f] = w.lin_b[1][j]; }
  __syncthreads();
  for (int k = 0; k < 128; ++k) {
    const float wv = w.lin_t[1][k * 128 + j];
#pragma unroll
    for (int f = 0; f < HF; ++f) acc[f] = fmaf(wv, s_1[f][k], acc[f]);
  }
#pragma unroll
  for (int f = 0; f < HF; ++f) s_2[f][j] = seg_lrelu(acc[f]);
  __syncthreads();
  if (j < HF * C) {   // one (frame, class) per thread
    const int f = j / C, c = j % C;
    float l = w.cls_b[c];
    for (int k = 0; k < 128; ++k) l = fmaf(w.cls_w[c * 128 + k], s_2[f][k], l);
    const float p = seg_sigmoid(l);
    s_p[f][c] = p;
    if (t0 + f < kSegT) {
      const size_t o = ((size_t)chunk * kSegT + t0 + f) * C + c;
      logits[o] = l;
      probs[o] = p;
    }
  }
  __syncthreads();
  if (j < HF && t0 + j < kSegT) {
    float m = s_p[j][0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, s_p[j][c]);
    score[(size_t)chunk * kSegT + t0 + j] = m;
  }
}

// frame j of a recording: sum_k w[f] p_k[f] / sum_k w[f] over the chunks k with f = j - s(k) in [0, 293), k ascending
__global__ __launch_bounds__(256) void seg_agg_kernel(const SegAggJob* __restrict__ jobs, const float* __restrict__ score,
                                                      const float* __restrict__ window, float* __restrict__ out) {
  const SegAggJob job = jobs[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, j = job.j0 + i;
  if (j >= job.j1) return;
  float num = 0.f, den = 0.f;
  for (int64_t k = job.kmin; k < job.kmax; ++k) {
    const int64_t f = j - (kSegStep * k + 135) / 270;
    if (f < 0 || f >= kSegT) continue;
    const float wv = window[f];
    num = fmaf(wv, score[(size_t)(job.row0 + (k - job.kmin)) * kSegT + f], num);
    den += wv;
  }
  out[job.out_off + i] = num / den;
}

}  // namespace

void launch_seg_frontend(const SegWeights& w, const SegBuffers& b, int n, hipStream_t s) {
  if (n < 1 || n > kSegGroup || !b.pcm || !b.desc || !b.st0 || !b.a1 || !b.st1 || !b.a2 || !b.st2 || !b.a3 || !b.st3) {
    launch_fault("seg_frontend: %d chunks", n);
    return;
  }
  hipLaunchKernelGGL(seg_stats_kernel, dim3(n), dim3(256), 0, s, b.pcm, b.desc, kSegChunk, b.st0);
  hipLaunchKernelGGL(seg_sinc_kernel, dim3((kSegL1 + SP - 1) / SP, n), dim3(256), 0, s, w, b);
  hipLaunchKernelGGL(seg_stats_kernel, dim3(n * kSegC1), dim3(256), 0, s, (const float*)b.a1, (const SegDesc*)nullptr, kSegL1, b.st1);
  hipLaunchKernelGGL((seg_conv_kernel<kSegC1, kSegL1, kSegL2>), dim3((kSegL2 + SP - 1) / SP, n), dim3(256), 0, s, (const float*)b.a1,
                     (const float*)b.st1, w.norm_w[0], w.norm_b[0], w.conv_t[0], w.conv_b[0], b.a2);
  hipLaunchKernelGGL(seg_stats_kernel, dim3(n * kSegC2), dim3(256), 0, s, (const float*)b.a2, (const SegDesc*)nullptr, kSegL2, b.st2);
  hipLaunchKernelGGL((seg_conv_kernel<kSegC2, kSegL2, kSegT>), dim3((kSegT + SP - 1) / SP, n), dim3(256), 0, s, (const float*)b.a2,
                     (const float*)b.st2, w.norm_w[1], w.norm_b[1], w.conv_t[1], w.conv_b[1], b.a3);
  hipLaunchKernelGGL(seg_stats_kernel, dim3(n * kSegC2), dim3(256), 0, s, (const float*)b.a3, (const SegDesc*)nullptr, kSegT, b.st3);
}

void launch_seg_network(const SegWeights& w, const SegBuffers& b, int n, int rows, hipStream_t s) {
  if (n < 1 || n > kSegGroup || (rows != 1 && rows != 2 && rows != 4) || !b.pcm || !b.desc || !b.gx || w.classes < 1 || w.classes > kSegMaxC) {
    launch_fault("seg_network: %d chunks, %d rows per recurrence workgroup", n, rows);
    return;
  }
  launch_seg_frontend(w, b, n, s);
  const dim3 pgrid((kSegT + PT - 1) / PT, 4, n), lgrid((n + rows - 1) / rows, 2);
  for (int l = 0; l < kSegLayers; ++l) {
    float* out = b.y[l & 1];
    if (l == 0)
      hipLaunchKernelGGL(seg_proj_kernel<true>, pgrid, dim3(256), 0, s, w.wih_t[0], w.gate_b[0], (const float*)b.a3,
                         (const float*)b.st3, w.norm_w[2], w.norm_b[2], b.gx);
    else
      hipLaunchKernelGGL(seg_proj_kernel<false>, pgrid, dim3(256), 0, s, w.wih_t[l], w.gate_b[l], (const float*)b.y[(l - 1) & 1],
                         (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, b.gx);
    if (rows == 1) hipLaunchKernelGGL(seg_lstm_kernel<1>, lgrid, dim3(512), 0, s, w.whh[l][0], w.whh[l][1], (const float*)b.gx, out, n);
    else if (rows == 2) hipLaunchKernelGGL(seg_lstm_kernel<2>, lgrid, dim3(512), 0, s, w.whh[l][0], w.whh[l][1], (const float*)b.gx, out, n);
    else hipLaunchKernelGGL(seg_lstm_kernel<4>, lgrid, dim3(512), 0, s, w.whh[l][0], w.whh[l][1], (const float*)b.gx, out, n);
  }
  hipLaunchKernelGGL(seg_head_kernel, dim3((kSegT + HF - 1) / HF, n), dim3(128), 0, s, w, (const float*)b.y[(kSegLayers - 1) & 1],
                     b.probs, b.logits, b.score + (size_t)kSegCarry * kSegT);
}

void launch_seg_aggregate(const SegBuffers& b, int n_jobs, int64_t max_frames, hipStream_t s) {
  if (n_jobs < 1 || n_jobs > kSegGroup || max_frames < 1 || max_frames > (int64_t)kSegGroup * kSegAggRow || !b.jobs || !b.agg_out) {
    launch_fault("seg_aggregate: %d jobs, %lld frames", n_jobs, (long long)max_frames);
    return;
  }
  hipLaunchKernelGGL(seg_agg_kernel, dim3((unsigned)((max_frames + 255) / 256), n_jobs), dim3(256), 0, s, b.jobs, (const float*)b.score,
                     b.window, b.agg_out);
}
