// Speaker-embedding network (XVectorSincNet shape; include/ttasr.h ttasr_spk_*), all f32, over a group of chunks of 80 000 samples.
// The front end is kernels_seg.hip's (launch_seg_frontend) with this network's weights; what is new here:
//
//   spk_gemm_kernel<MODE>  ONE GEMM body on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, exact f32):
//                          64 rows x 128 columns per workgroup of four waves, each wave two 32 x 32 accumulators, K in steps of 16
//                          through LDS, the next step's operands in registers while this one multiplies.
//                            MODE 0  TDNN block 1: rows = frames of a chunk, K = 5 taps x 60 channels, read from the third stage's
//                                    [60][293] output with its InstanceNorm and leaky_relu applied on load;
//                            MODE 1  TDNN blocks 2-5: K = taps x 512 channels, tap j of frame t reads row t + j * dilation of the
//                                    previous block's [frames][512] output - the dilated window is gathered while the tile is
//                                    loaded, no im2col buffer exists;
//                            MODE 2  the embedding Linear over the pooled rows, K = 3 000.
//                          Epilogue of modes 0 and 1: + bias, leaky_relu(0.01), BatchNorm (running statistics); of mode 2: + bias,
//                          and a row of a zero-sum mask reads zeros and is written as quiet NaN.
//                          An output row is a function of its own operand row, the weights and k ascending - not of the tile it
//                          sits in - and a tile of modes 0 and 1 lies inside one chunk.  Edge tiles (289 / 285 / 279 rows, K = 300,
//                          N = 1 500, any D) load zeros past the edge and store nothing there.
//   spk_pool_kernel        weighted statistics pooling, one thread per channel and (chunk, mask), two passes (the mean, then the
//                          squared differences: the one-pass form cancels, as in seg_stats_kernel), frames ascending.
//
// No atomics.  Every multiply-add is written as fmaf and the file is compiled with -ffp-contract=off (Makefile).
#include "common.hpp"
#include "spk.hpp"

namespace {

constexpr int BM = 64, BN = 128, BK = 16;
constexpr int AP = BM + 4;   // s_a row pitch: the four rows a wave's float4 pieces write spread over the banks

__device__ __forceinline__ float spk_lrelu(float v) { return v > 0.f ? v : 0.01f * v; }

struct SpkGemmArgs {
  const float* a;                 // mode 0: a3 [n][60][293]; mode 1: [n][..][512], chunks a_stride floats apart; mode 2: [rows][K]
  const float* st; const float* nw; const float* nb;   // mode 0: the third stage's statistics [n][60][2] and norm [60]
  const float* wt;                // [K][ldb]
  const float* bias; const float* bn_mean; const float* bn_scale; const float* bn_beta;   // [N]
  const int32_t* valid;           // mode 2: [rows]
  float* out;                     // [..][rows_out][N], chunks out_stride floats apart
  int rows_out, taps, dil, K, N, ldb;
  long a_stride, out_stride;
};

template <int MODE>
__global__ __launch_bounds__(256) void spk_gemm_kernel(SpkGemmArgs g) {
  __shared__ float s_a[BK * AP];
  __shared__ float s_b[BK * BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int chunk = blockIdx.z, m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int wr = wave >> 1, wc = wave & 1;
  constexpr int CIN = MODE == 0 ? kSegC2 : kSpkHid;

  float ra[4];
  float4 rb[2];
  // the operands of K step k0 into registers; zeros past every edge
  auto load = [&](int k0) {
    if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = m0 + lane, k = k0 + wave + 4 * i;   // k is uniform over the wave
        float v = 0.f;
        if (row < g.rows_out && k < g.K) {
          const int j = k / CIN, c = k - j * CIN, ch = chunk * CIN + c;
          const float mean = g.st[2 * ch], rstd = g.st[2 * ch + 1];
          v = spk_lrelu(fmaf((g.a[(size_t)ch * kSegT + row + j] - mean) * rstd, g.nw[c], g.nb[c]));
        }
        ra[i] = v;
      }
    } else {
      const int row = m0 + (tid >> 2), k = k0 + 4 * (tid & 3);   // K is a multiple of 4: a piece is inside or outside
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < g.rows_out && k < g.K) {
        if (MODE == 1) {
          const int j = k / CIN, c = k - j * CIN;
          v = *(const float4*)(g.a + (size_t)chunk * g.a_stride + (size_t)(row + j * g.dil) * CIN + c);
        } else if (g.valid[row]) {
          v = *(const float4*)(g.a + (size_t)row * g.K + k);
        }
      }
      ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int k = k0 + (tid >> 5) + 8 * i, col = n0 + 4 * (tid & 31);   // ldb is a multiple of 4
      rb[i] = k < g.K && col < g.ldb ? *(const float4*)(g.wt + (size_t)k * g.ldb + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
    if (MODE == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_a[(wave + 4 * i) * AP + lane] = ra[i];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s_a[(4 * (tid & 3) + e) * AP + (tid >> 2)] = ra[e];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *(float4*)(s_b + ((tid >> 5) + 8 * i) * BN + 4 * (tid & 31)) = rb[i];
  };

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  load(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
    __syncthreads();   // the previous step's reads are over
    stash();
    __syncthreads();
    if (k0 + BK < g.K) load(k0 + BK);
    const float* pa = s_a + (lane >> 5) * AP + wr * 32 + (lane & 31);
    const float* pb = s_b + (lane >> 5) * BN + wc * 64 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {   // lane l brings A[row l & 31][k = kk + (l >> 5)] and B[k][column l & 31]
      const float av = pa[kk * AP], b0 = pb[kk * BN], b1 = pb[kk * BN + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);
    }
  }

  // C/D of the 32 x 32 forms: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int col = n0 + wc * 64 + half * 32 + (lane & 31);
    if (col >= g.N) continue;
    const float bias = g.bias[col];
    float mean = 0.f, scale = 1.f, beta = 0.f;
    if (MODE != 2) { mean = g.bn_mean[col]; scale = g.bn_scale[col]; beta = g.bn_beta[col]; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= g.rows_out) continue;
      float v = (half ? acc1[r] : acc0[r]) + bias;
      if (MODE != 2) v = fmaf(spk_lrelu(v) - mean, scale, beta);
      else if (!g.valid[row]) v = __int_as_float(0x7FC00000);
      g.out[(size_t)chunk * g.out_stride + (size_t)row * g.N + col] = v;
    }
  }
}

// grid (ceil(1500 / 256), S, n): channel c of (chunk, mask).  w'[j] = w[(293 j) / 279]; v1 = sum w', v2 = sum w'^2;
// mean = sum w' x / v1; std = sqrt(sum w' (x - mean)^2 / (v1 - v2 / v1 + 1e-8)); every sum over j ascending.
__global__ __launch_bounds__(256) void spk_pool_kernel(const float* __restrict__ h5, const float* __restrict__ masks, int S,
                                                       int32_t* __restrict__ valid, float* __restrict__ stats) {
  __shared__ float s_w[kSpkT];
  const int chunk = blockIdx.z, tid = threadIdx.x, c = blockIdx.x * 256 + tid;
  const size_t row = (size_t)chunk * S + blockIdx.y;
  const float* m = masks + row * kSegT;
  for (int j = tid; j < kSpkT; j += 256) s_w[j] = m[(j * kSegT) / kSpkT];
  __syncthreads();
  float v1 = 0.f, v2 = 0.f;
  for (int j = 0; j < kSpkT; ++j) { v1 += s_w[j]; v2 = fmaf(s_w[j], s_w[j], v2); }
  const bool ok = v1 > 0.f;
  if (blockIdx.x == 0 && tid == 0) valid[row] = ok;
  if (c >= kSpkOut) return;
  float* out = stats + row * kSpkStats;
  if (!ok) {   // a zero-sum mask: nothing is computed from it
    out[c] = __int_as_float(0x7FC00000); out[kSpkOut + c] = __int_as_float(0x7FC00000);
    return;
  }
  const float* x = h5 + (size_t)chunk * kSpkT * kSpkOut + c;
  float a = 0.f;
  for (int j = 0; j < kSpkT; ++j) a = fmaf(s_w[j], x[(size_t)j * kSpkOut], a);
  const float mean = a / v1;
  float q = 0.f;
  for (int j = 0; j < kSpkT; ++j) {
    const float d = x[(size_t)j * kSpkOut] - mean;
    q = fmaf(s_w[j] * d, d, q);
  }
  out[c] = mean;
  out[kSpkOut + c] = sqrtf(q / (v1 - v2 / v1 + 1e-8f));
}

}  // namespace

void launch_spk_network(const SpkWeights& w, const SpkBuffers& b, int n, int S, hipStream_t s) {
  bool ok = n >= 1 && n <= kSpkGroup && S >= 1 && S <= kSpkMaxMasks && w.dim >= 1 && w.dim <= kSpkMaxDim && w.ldd == ((w.dim + 3) & ~3) &&
            b.h[0] && b.h[1] && b.h5 && b.masks && b.valid && b.stats && b.emb && w.emb_t && w.emb_b;
  for (int l = 0; l < kSpkLayers; ++l)
    ok = ok && w.wt[l] && w.bias[l] && w.bn_mean[l] && w.bn_scale[l] && w.bn_beta[l] &&
         kSpkFrames[l + 1] + (kSpkTaps[l] - 1) * kSpkDil[l] <= kSpkFrames[l] && kSpkFrames[l + 1] <= kSpkRows && kSpkCout[l] % 4 == 0;
  if (!ok) {
    launch_fault("spk_network: %d chunks, %d masks, dimension %d", n, S, w.dim);
    return;
  }
  launch_seg_frontend(w.front, b.front, n, s);
  for (int l = 0; l < kSpkLayers; ++l) {
    SpkGemmArgs g{};
    g.wt = w.wt[l]; g.bias = w.bias[l]; g.bn_mean = w.bn_mean[l]; g.bn_scale = w.bn_scale[l]; g.bn_beta = w.bn_beta[l];
    g.rows_out = kSpkFrames[l + 1]; g.taps = kSpkTaps[l]; g.dil = kSpkDil[l]; g.K = kSpkTaps[l] * kSpkCin[l];
    g.N = g.ldb = kSpkCout[l];
    g.a_stride = (long)kSpkRows * kSpkHid;
    g.out = l == kSpkLayers - 1 ? b.h5 : b.h[l & 1];
    g.out_stride = l == kSpkLayers - 1 ? (long)kSpkT * kSpkOut : (long)kSpkRows * kSpkHid;
    const dim3 grid((g.rows_out + BM - 1) / BM, (g.N + BN - 1) / BN, n);
    if (l == 0) {
      g.a = b.front.a3; g.st = b.front.st3; g.nw = w.front.norm_w[2]; g.nb = w.front.norm_b[2];
      hipLaunchKernelGGL(spk_gemm_kernel<0>, grid, dim3(256), 0, s, g);
    } else {
      g.a = b.h[(l - 1) & 1];
      hipLaunchKernelGGL(spk_gemm_kernel<1>, grid, dim3(256), 0, s, g);
    }
  }
  hipLaunchKernelGGL(spk_pool_kernel, dim3((kSpkOut + 255) / 256, S, n), dim3(256), 0, s, (const float*)b.h5, b.masks, S, b.valid, b.stats);
  SpkGemmArgs g{};
  g.a = b.stats; g.valid = b.valid; g.wt = w.emb_t; g.bias = w.emb_b; g.out = b.emb;
  g.rows_out = n * S; g.taps = 1; g.dil = 1; g.K = kSpkStats; g.N = w.dim; g.ldb = w.ldd;
  hipLaunchKernelGGL(spk_gemm_kernel<2>, dim3((g.rows_out + BM - 1) / BM, (g.N + BN - 1) / BN, 1), dim3(256), 0, s, g);
}
