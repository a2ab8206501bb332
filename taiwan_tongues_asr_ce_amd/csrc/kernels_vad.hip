// Voice-activity network (Silero-v5 shape, 16 kHz branch; include/ttasr.h ttasr_vad_*), all f32, in two kernels per time chunk:
//
//   vad_frames_kernel   frame-parallel: one workgroup per tile of kVadTile consecutive frames of one recording.  Gathers the
//                       frames from the staged PCM, then STFT -> magnitude -> four Conv1d + ReLU -> input projection
//                       gx = W_ih e + (b_ih + b_hh), everything between the PCM and gx in LDS.  A thread owns an output channel
//                       and carries one accumulator per frame of the tile, so a weight is loaded once per kVadTile frames; every
//                       frame's sums run in the same fixed order (input index ascending), whichever slot of the tile it has.
//   vad_lstm_kernel     recurrent: one workgroup of 512 threads per recording walks its frames in order.  Thread r keeps row r of
//                       W_hh (128 f32) in registers for the whole launch, h lives in LDS and is read as a broadcast; two barriers
//                       per frame; the output head is a fixed-order wave reduction.  No atomics anywhere.  Its (h, c) lives at
//                       state[slot[row]] (slot == nullptr: state[row]): the offline call keeps one state row per recording of
//                       the call, a stream push names the rows of the context's stream table.  ONE per-frame body for both.
//
// The form of both kernels is a function of the frame only: nothing depends on a recording's length, on the number of recordings
// or on a recording's place in the call (those decide grid sizes and early exits of whole workgroups, never an operand order).
#include "common.hpp"
#include "vad.hpp"

namespace {

constexpr int FT = kVadTile;
constexpr int VAD_THREADS = 256;
constexpr int X_LEN = kVadContext + kVadWindow + 64;   // 640: context | frame | right reflect pad
constexpr int N_BIN = 129, N_COL = 4, N_ROW = 2 * N_BIN;   // STFT: 129 bins (re rows 0..128, im rows 129..257), 4 columns
// two LDS regions, alternately source and destination of a stage
constexpr int REGION_A = FT * N_BIN * (N_COL + 2);    // 6192 floats: x [FT][640] | mag [FT][129][6] | a2 | a4
constexpr int REGION_B = N_ROW * N_COL * FT;          // 8256 floats: S [258][4][FT] | a1 [FT][128][6] | a3
static_assert(REGION_A >= FT * X_LEN && REGION_B >= FT * 128 * 6, "LDS regions hold every stage");

// Conv1d (k = 3, zero pad 1, stride STRIDE) + ReLU over the tile.  in [FT][CIN][TIN + 2], out [FT][COUT][TOUT + 2]: rows carry
// their zero padding (index 0 and the last), so y[o][t] = bias[o] + sum_c sum_j w[o][c][j] in[c][STRIDE t + j], c ascending, j ascending.
template <int CIN, int COUT, int TIN, int STRIDE>
__device__ __forceinline__ void vad_conv(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ wt,
                                         const float* __restrict__ bias) {
  constexpr int TOUT = (TIN - 1) / STRIDE + 1, PI = TIN + 2, PO = TOUT + 2;
  for (int it = threadIdx.x; it < COUT * TOUT; it += VAD_THREADS) {
    const int o = it % COUT, t = it / COUT;   // a wave's lanes: consecutive o, one t
    float acc[FT];
    const float b = bias[o];
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[f] = b;
    for (int c = 0; c < CIN; ++c) {
      const float w0 = wt[(c * 3 + 0) * COUT + o], w1 = wt[(c * 3 + 1) * COUT + o], w2 = wt[(c * 3 + 2) * COUT + o];
#pragma unroll
      for (int f = 0; f < FT; ++f) {
        const float* p = in + (f * CIN + c) * PI + STRIDE * t;
        acc[f] = fmaf(w0, p[0], acc[f]);
        acc[f] = fmaf(w1, p[1], acc[f]);
        acc[f] = fmaf(w2, p[2], acc[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) out[(f * COUT + o) * PO + 1 + t] = fmaxf(acc[f], 0.f);
  }
  for (int it = threadIdx.x; it < FT * COUT; it += VAD_THREADS) { out[it * PO] = 0.f; out[it * PO + PO - 1] = 0.f; }
}

__global__ __launch_bounds__(VAD_THREADS) void vad_frames_kernel(VadWeights w, const float* __restrict__ pcm,
                                                                 const int32_t* __restrict__ nf, float* __restrict__ gx) {
  const int file = blockIdx.y, f0 = blockIdx.x * FT;
  const int n = min(nf[file], kVadChunk);
  if (f0 >= n) return;   // uniform; nothing is loaded before it
  __shared__ __attribute__((aligned(16))) float s_a[REGION_A];
  __shared__ __attribute__((aligned(16))) float s_b[REGION_B];
  const int tid = threadIdx.x;
  // (0) gather: frame g of the chunk is pcm[512 g .. 512 g + 576) of the recording's slot (its first 64 floats are the context in
  // front of the chunk); x[576 + j] = x[574 - j].  Slots of the tile past the recording's last frame compute on zeros.
  const float* row = pcm + (size_t)file * kVadSlot;
  for (int i = tid; i < FT * X_LEN; i += VAD_THREADS) {
    const int f = i / X_LEN, j = i % X_LEN;
    const int src = j < 576 ? j : 1150 - j;   // 574 - (j - 576)
    s_a[i] = f0 + f < n ? row[(size_t)(f0 + f) * kVadWindow + src] : 0.f;
  }
  __syncthreads();
  // (1) STFT as a strided correlation: S[k][t] = sum_m basis[k][m] x[128 t + m], m ascending.  Thread k < 256 owns row k for
  // all 4 columns and all frames (32 accumulators per weight load); rows 256 and 257 are dealt to the 64 threads of the last
  // wave, one (row, column, frame) each, in the same order of m.
  {
    float acc[N_COL][FT];
#pragma unroll
    for (int t = 0; t < N_COL; ++t)
#pragma unroll
      for (int f = 0; f < FT; ++f) acc[t][f] = 0.f;
    for (int m = 0; m < 256; m += 4) {
      const float w0 = w.basis_t[(m + 0) * N_ROW + tid], w1 = w.basis_t[(m + 1) * N_ROW + tid],
                  w2 = w.basis_t[(m + 2) * N_ROW + tid], w3 = w.basis_t[(m + 3) * N_ROW + tid];
#pragma unroll
      for (int t = 0; t < N_COL; ++t)
#pragma unroll
        for (int f = 0; f < FT; ++f) {
          const f32x4 xv = *(const f32x4*)(s_a + f * X_LEN + 128 * t + m);
          acc[t][f] = fmaf(w0, xv[0], acc[t][f]);
          acc[t][f] = fmaf(w1, xv[1], acc[t][f]);
          acc[t][f] = fmaf(w2, xv[2], acc[t][f]);
          acc[t][f] = fmaf(w3, xv[3], acc[t][f]);
        }
    }
#pragma unroll
    for (int t = 0; t < N_COL; ++t)
#pragma unroll
      for (int f = 0; f < FT; ++f) s_b[(tid * N_COL + t) * FT + f] = acc[t][f];
    if (tid >= VAD_THREADS - 2 * N_COL * FT) {
      const int e = tid - (VAD_THREADS - 2 * N_COL * FT);   // 0 .. 63
      const int k = 256 + e / (N_COL * FT), t = (e / FT) % N_COL, f = e % FT;
      float a = 0.f;
      for (int m = 0; m < 256; ++m) a = fmaf(w.basis_t[m * N_ROW + k], s_a[f * X_LEN + 128 * t + m], a);
      s_b[(k * N_COL + t) * FT + f] = a;
    }
  }
  __syncthreads();
  // (2) magnitude -> mag [FT][129][6] with zero padding at 0 and 5
  for (int i = tid; i < N_BIN * N_COL * FT; i += VAD_THREADS) {
    const int f = i % FT, t = (i / FT) % N_COL, b = i / (FT * N_COL);
    const float re = s_b[i], im = s_b[i + N_BIN * N_COL * FT];
    s_a[(f * N_BIN + b) * (N_COL + 2) + 1 + t] = sqrtf(re * re + im * im);
  }
  for (int i = tid; i < FT * N_BIN; i += VAD_THREADS) { s_a[i * (N_COL + 2)] = 0.f; s_a[i * (N_COL + 2) + N_COL + 1] = 0.f; }
  __syncthreads();
  // (3) the encoder: time steps 4 -> 4 -> 2 -> 1 -> 1
  vad_conv<129, 128, 4, 1>(s_a, s_b, w.conv_t[0], w.conv_b[0]);
  __syncthreads();
  vad_conv<128, 64, 4, 2>(s_b, s_a, w.conv_t[1], w.conv_b[1]);
  __syncthreads();
  vad_conv<64, 64, 2, 2>(s_a, s_b, w.conv_t[2], w.conv_b[2]);
  __syncthreads();
  vad_conv<64, 128, 1, 1>(s_b, s_a, w.conv_t[3], w.conv_b[3]);
  __syncthreads();
  // (4) the LSTM's input projection, hoisted out of the recurrence: gx[r] = (b_ih + b_hh)[r] + sum_k W_ih[r][k] e[k], k ascending
  float* gout = gx + ((size_t)file * kVadChunk + f0) * 512;
  for (int r = tid; r < 512; r += VAD_THREADS) {
    float acc[FT];
    const float b = w.gate_b[r];
#pragma unroll
    for (int f = 0; f < FT; ++f) acc[f] = b;
    for (int k = 0; k < 128; ++k) {
      const float wv = w.wih_t[k * 512 + r];
#pragma unroll
      for (int f = 0; f < FT; ++f) acc[f] = fmaf(wv, s_a[(f * 128 + k) * 3 + 1], acc[f]);
    }
#pragma unroll
    for (int f = 0; f < FT; ++f)
      if (f0 + f < n) gout[(size_t)f * 512 + r] = acc[f];
  }
}

__device__ __forceinline__ float vad_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// 512 threads = 8 waves, 2 per SIMD: a wave may hold 256 VGPRs, 128 of them row r of W_hh.
__global__ __launch_bounds__(512) void vad_lstm_kernel(VadWeights w, const float* __restrict__ gx, const int32_t* __restrict__ nf,
                                                       float* __restrict__ state, const int32_t* __restrict__ slot,
                                                       float* __restrict__ out) {
  const int file = blockIdx.x;
  const int n = min(nf[file], kVadChunk);
  if (n <= 0) return;   // uniform
  __shared__ __attribute__((aligned(16))) float s_h[128];
  __shared__ float s_g[512];
  __shared__ float s_part[2];
  const int r = threadIdx.x;
  float wr[128];
#pragma unroll
  for (int k = 0; k < 128; k += 4) {
    const f32x4 v = *(const f32x4*)(w.whh + (size_t)r * 128 + k);
    wr[k] = v[0]; wr[k + 1] = v[1]; wr[k + 2] = v[2]; wr[k + 3] = v[3];
  }
  float* st = state + (size_t)(slot ? slot[file] : file) * 256;   // uniform; the host checked the index and that no two rows share one
  float cell = 0.f, wo = 0.f;
  if (r < 128) { s_h[r] = st[r]; cell = st[128 + r]; wo = w.w_out[r]; }
  const float b_out = w.b_out[0];
  const float* g = gx + (size_t)file * kVadChunk * 512;
  float* logits = out + (size_t)file * 2 * kVadChunk;
  float* probs = logits + kVadChunk;
  float g_cur = g[r];
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    const float g_next = t + 1 < n ? g[(size_t)(t + 1) * 512 + r] : 0.f;   // requested a frame ahead
    // gate row r: gx + W_hh[r] . h, four interleaved partial sums (k mod 4), each k ascending, joined as (a0 + a1) + (a2 + a3)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int k = 0; k < 128; k += 4) {
      const f32x4 hv = *(const f32x4*)(s_h + k);
      a0 = fmaf(wr[k], hv[0], a0);
      a1 = fmaf(wr[k + 1], hv[1], a1);
      a2 = fmaf(wr[k + 2], hv[2], a2);
      a3 = fmaf(wr[k + 3], hv[3], a3);
    }
    s_g[r] = g_cur + ((a0 + a1) + (a2 + a3));
    if (r == 0 && t > 0) {   // the previous frame's head: its two wave sums were written before the last barrier
      const float l = b_out + (s_part[0] + s_part[1]);
      logits[t - 1] = l;
      probs[t - 1] = vad_sigmoid(l);
    }
    __syncthreads();   // gates complete; every read of h and of s_part is done
    if (r < 128) {
      const float gi = vad_sigmoid(s_g[r]), gf = vad_sigmoid(s_g[128 + r]), gg = tanhf(s_g[256 + r]), go = vad_sigmoid(s_g[384 + r]);
      cell = gf * cell + gi * gg;
      const float h = go * tanhf(cell);
      s_h[r] = h;
      const float p = wave_sum(wo * fmaxf(h, 0.f));   // fixed butterfly over the wave's 64 channels
      if ((r & 63) == 0) s_part[r >> 6] = p;
    }
    __syncthreads();   // h and the head's partial sums complete; every read of the gates is done
    g_cur = g_next;
  }
  if (r == 0) {
    const float l = b_out + (s_part[0] + s_part[1]);
    logits[n - 1] = l;
    probs[n - 1] = vad_sigmoid(l);
  }
  if (r < 128) { st[r] = s_h[r]; st[128 + r] = cell; }
}

}  // namespace

void launch_vad_frames(const VadWeights& w, const float* pcm, const int32_t* nf, float* gx, int n, int max_nf, hipStream_t s) {
  if (n < 1 || max_nf < 1 || max_nf > kVadChunk || !pcm || !nf || !gx) {
    launch_fault("vad_frames: %d recordings, %d frames", n, max_nf);
    return;
  }
  hipLaunchKernelGGL(vad_frames_kernel, dim3((max_nf + FT - 1) / FT, n), dim3(VAD_THREADS), 0, s, w, pcm, nf, gx);
}

void launch_vad_lstm(const VadWeights& w, const float* gx, const int32_t* nf, float* state, const int32_t* slot, float* out, int n,
                     hipStream_t s) {
  if (n < 1 || !gx || !nf || !state || !out) {
    launch_fault("vad_lstm: %d recordings", n);
    return;
  }
  hipLaunchKernelGGL(vad_lstm_kernel, dim3(n), dim3(512), 0, s, w, gx, nf, state, slot, out);
}
