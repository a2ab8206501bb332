// Opt-in serving mode (option "xkv_fp8", never the headline configuration): the decoder's cross-attention K / V cache in
// OCP fp8 e4m3 with one f32 scale per (layer, K | V, clip, head) block.  SURVEY.md section 7 names it as the lever on the 7.87 GB
// a decode step streams: the cache is written once per clip and read once per (token, layer), so halving its bytes halves the
// HBM time of the dominant kernel.  The 16-bit cache stays the source of truth (every other path - beam search, prefill,
// alignment, the split-frame small-batch kernels - keeps reading it); this file adds
//   xkv_quant_kernel       one workgroup per (layer, K | V, clip, head) block of Tk x 64 stored values: pass 1 the block's |max|,
//                          pass 2 (the block is L2 / Infinity-Cache resident) value * 448 / |max| -> e4m3, scale = |max| / 448
//   cross_attn_fp8_kernel  the software-pipelined decode-step kernel of kernels_attn.hip on 64-byte rows: 16 values per lane, 4 lanes
//                          per frame, 16 frames per wave-instruction; the K scale is folded into the query, the V scale into the
//                          normalisation; scores, softmax and accumulation in f32 exactly as in the 16-bit kernel.
// Option value 2 ("read the copy wherever a kernel for it exists") adds
//   cross_attn_mq_fp8_kernel  the shared-clip kernel of kernels_attn.hip (cross_attn_mq_kernel: beam hypotheses, sampled rows) on
//                          the e4m3 copy: 8 values per lane, 8 lanes per frame, 8-byte loads - the 16-bit kernel's register shape
//   xkv_quant_slots_kernel the quantiser with (source slot, destination slot) pairs: a session quantises an admitted clip from
//                          its STAGING 16-bit block straight into the live slot of the e4m3 copy
// Accuracy is reported, not assumed: bench.py --xkv-fp8 (token agreement with the bf16 engine and the f32 parity engine on the
// headline workload); tests/test_gpu_fp8*.py hold the whole engine to the bf16 engine's (liveness, bit-reproducibility, step logits
// within 0.12, at least half the rows with equal tokens); tests/test_gpu_xattn_kernels.py holds THESE kernels to a float64 reference
// through the known-answer hooks ttasr_get_cross_kv_fp8 / ttasr_cross_attn_probe: quantiser codes and scales bit for bit
// (oracle/whisper_ref.py xkv_quant_ref), attention output over codes x scale within a derived f32 bound.
#include "common.hpp"

namespace {
using u32x4q = __attribute__((ext_vector_type(4))) unsigned;
using u32x2q = __attribute__((ext_vector_type(2))) unsigned;
typedef float f32x2q __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void unpack16_fp8(const u32x4q& r, float (&v)[16]) {
  const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2q lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2q hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    v[4 * i] = lo[0]; v[4 * i + 1] = lo[1]; v[4 * i + 2] = hi[0]; v[4 * i + 3] = hi[1];
  }
}
__device__ __forceinline__ void unpack8_fp8(const u32x2q& r, float (&v)[8]) {
  const unsigned w[2] = {r.x, r.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x2q lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2q hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    v[4 * i] = lo[0]; v[4 * i + 1] = lo[1]; v[4 * i + 2] = hi[0]; v[4 * i + 3] = hi[1];
  }
}
constexpr int DPP_ROR4 = 0x124;   // row_ror:4 - lane i <- lane (i + 4) % 16 of its row
// sum over the lanes that share (lane % 4): 4, 8, 12 lanes apart inside a row of 16, then the other rows and the other half
__device__ __forceinline__ float stride4_sum(float v) {
  v += dpp_f<DPP_ROR4>(v);
  v += dpp_f<DPP_ROR8>(v);
  v = xor16_reduce(v, OpSum{});
  v = xor32_reduce(v, OpSum{});
  return v;
}
}  // namespace

// One block of rows x 64 stored values: pass 1 the block's |max|, pass 2 value * 448 / |max| -> e4m3, *scale = |max| / 448.
// Shared by both quantisers: a block quantised at a session's admission is bit-identical to the static encode's.
template <typename T>
__device__ __forceinline__ void xkv_quant_block(const T* __restrict__ src, uint8_t* __restrict__ dst, float* __restrict__ scale, int rows) {
  static_assert(sizeof(T) == 2, "16-bit cache only");
  __shared__ float red[4];
  const int n16 = rows * 64 / 8;   // 16-byte chunks of 8 stored values
  const uint4* s = (const uint4*)src;
  float amax = 0.f;
  for (int i = threadIdx.x; i < n16; i += 256) {
    float v[8];
    up8<T>(s[i], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
  amax = wave_max(amax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;   // e4m3 finite maximum 448
  const float inv = 1.0f / sc;
  if (threadIdx.x == 0) *scale = sc;
  uint2* d = (uint2*)dst;
  for (int i = threadIdx.x; i < n16; i += 256) {
    float v[8];
    up8<T>(s[i], v);
    int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
    int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
    d[i] = make_uint2((unsigned)lo, (unsigned)hi);
  }
}
// src: T [n_blocks][rows * 64]; dst: fp8 [n_blocks][rows * 64]; scale: f32 [n_blocks] (dequantised value = fp8 * scale)
template <typename T>
__global__ __launch_bounds__(256) void xkv_quant_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, float* __restrict__ scale,
                                                        int rows) {
  const int64_t blk = blockIdx.x;
  xkv_quant_block<T>(src + blk * rows * 64, dst + blk * rows * 64, scale + blk, rows);
}
// Session admission: workgroup (h, l * 2 + which, i) quantises the block of clip slot p.src[i] of the 16-bit buffer `src`
// (the session's staging cross-KV) into slot p.dst[i] of the e4m3 copy and writes that slot's scale.  The pairs travel in the
// kernel arguments: no copy, nothing to keep alive.
template <typename T>
__global__ __launch_bounds__(256) void xkv_quant_slots_kernel(const T* __restrict__ src, uint8_t* __restrict__ dst, float* __restrict__ scale,
                                                              int rows, int H, int maxB, int64_t which_elems, XkvSlotPairs p) {
  const int h = blockIdx.x, lw = blockIdx.y, i = blockIdx.z;   // lw = layer * 2 + which: consecutive `which_elems` apart in both buffers
  const int from = p.src[i], to = p.dst[i];
  const int64_t blk = (int64_t)rows * 64;
  xkv_quant_block<T>(src + lw * which_elems + ((int64_t)from * H + h) * blk, dst + lw * which_elems + ((int64_t)to * H + h) * blk,
                     scale + ((int64_t)lw * maxB + to) * H + h, rows);
}
template <typename T>
void launch_xkv_quant(const T* src, uint8_t* dst, float* scale, int64_t n_blocks, int rows, hipStream_t s) {
  if constexpr (sizeof(T) == 2) hipLaunchKernelGGL(xkv_quant_kernel<T>, dim3((unsigned)n_blocks), dim3(256), 0, s, src, dst, scale, rows);
}
template void launch_xkv_quant<bf16_t>(const bf16_t*, uint8_t*, float*, int64_t, int, hipStream_t);
template void launch_xkv_quant<f16_t>(const f16_t*, uint8_t*, float*, int64_t, int, hipStream_t);
template void launch_xkv_quant<float>(const float*, uint8_t*, float*, int64_t, int, hipStream_t);
template <typename T>
void launch_xkv_quant_slots(const T* src, uint8_t* dst, float* scale, int n_layers, int H, int rows, int maxB, int64_t which_elems,
                            const XkvSlotPairs& p, int n, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (n < 1 || n > XkvSlotPairs::N) { launch_fault("xkv_quant_slots: %d pairs outside [1, %d]", n, XkvSlotPairs::N); return; }
    hipLaunchKernelGGL(xkv_quant_slots_kernel<T>, dim3(H, 2 * n_layers, n), dim3(256), 0, s, src, dst, scale, rows, H, maxB, which_elems, p);
  }
}
template void launch_xkv_quant_slots<bf16_t>(const bf16_t*, uint8_t*, float*, int, int, int, int, int64_t, const XkvSlotPairs&, int, hipStream_t);
template void launch_xkv_quant_slots<f16_t>(const f16_t*, uint8_t*, float*, int, int, int, int, int64_t, const XkvSlotPairs&, int, hipStream_t);
template void launch_xkv_quant_slots<float>(const float*, uint8_t*, float*, int, int, int, int, int64_t, const XkvSlotPairs&, int, hipStream_t);

// One workgroup (4 waves) per (row b, head h); K8 / V8: fp8 [B][H][Tk][64]; kscale / vscale: f32 [B][H].
template <typename T, bool QSLAB, int U>
__global__ __launch_bounds__(256) void cross_attn_fp8_kernel(const T* q, const uint8_t* K8, const uint8_t* V8, const float* kscale,
                                                             const float* vscale, T* out, const int32_t* done, int H, int Tk,
                                                             SlabIn sq) {
  static_assert(sizeof(T) == 2, "16-bit activations only");
  constexpr int NWV = 4, LPR = 4, RPI = 16, TSTEP = NWV * RPI;   // 64 frames per iteration of the workgroup
  extern __shared__ float sc[];  // [Tk] scores, then [NWV][64] partial outputs, [2 * NWV] reductions
  q = sgpr_pin_ptr(q); K8 = sgpr_pin_ptr(K8); V8 = sgpr_pin_ptr(V8); kscale = sgpr_pin_ptr(kscale); vscale = sgpr_pin_ptr(vscale);
  out = sgpr_pin_ptr(out); done = sgpr_pin_ptr(done); H = sgpr_pin(H); Tk = sgpr_pin(Tk);
  sq.slab = sgpr_pin_ptr(sq.slab); sq.bias = sgpr_pin_ptr(sq.bias); sq.n = sgpr_pin(sq.n); sq.stride = sgpr_pin(sq.stride);
  const int b = blockIdx.y, h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int done_raw = row_done_issue(done, b, K8);   // finished row of the batch (round 6; kernels_attn.hip cross_attn_pipe_kernel row_done_exit)
  const int d = H * 64;
  const int sub = lane % LPR, rin = lane / LPR;
  float* part = sc + Tk;
  float* red = part + NWV * 64;
  const uint8_t* Kp = K8 + ((int64_t)b * H + h) * Tk * 64 + sub * 16;
  const uint8_t* Vp = V8 + ((int64_t)b * H + h) * Tk * 64 + sub * 16;
  const int n_it = (Tk + TSTEP - 1) / TSTEP;
  const int trow = wave * RPI + rin;
  auto issue = [&](const uint8_t* base, int it0, u32x4q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = min((it0 + u) * TSTEP + trow, Tk - 1);   // clamped, unconditional
      r[u] = __builtin_nontemporal_load((const u32x4q*)(base + (int64_t)t * 64));
    }
  };
  u32x4q ra[U], rb[U];
  issue(Kp, 0, ra);
  const float ks = kscale[b * H + h], vs = vscale[b * H + h];
  float qv[16];
  {
    float q0[8], q1[8];
    const int64_t off = (int64_t)b * d + h * 64 + sub * 16;
    if constexpr (QSLAB) {
      // the two 8-value chunks of this lane's 16 query values, each summed from the q GEMM's K-split partial tiles
      float4 t[4][4], bs[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) bs[c] = *(const float4*)(sq.bias + h * 64 + sub * 16 + 4 * c);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* p = sq.slab + (int64_t)min(s, sq.n - 1) * sq.stride + off;
#pragma unroll
        for (int c = 0; c < 4; ++c) t[s][c] = *(const float4*)(p + 4 * c);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float4 a = bs[c];
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s == 0 || s < sq.n) { a.x += t[s][c].x; a.y += t[s][c].y; a.z += t[s][c].z; a.w += t[s][c].w; }
        float* dst = c < 2 ? q0 + 4 * c : q1 + 4 * (c - 2);
        dst[0] = to_f<T>(from_f<T>(a.x)); dst[1] = to_f<T>(from_f<T>(a.y)); dst[2] = to_f<T>(from_f<T>(a.z)); dst[3] = to_f<T>(from_f<T>(a.w));
      }
    } else {
      const uint4 a = *(const uint4*)(q + off), c = *(const uint4*)(q + off + 8);
      up8<T>(a, q0); up8<T>(c, q1);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { qv[j] = q0[j] * ks; qv[8 + j] = q1[j] * ks; }   // K scale folded into the query
  }
  if (done && done_raw) { if (Tk < 0) sc[0] = __uint_as_float(ra[0].x ^ ra[U - 1].x) + qv[0] + vs; return; }   // row_done_exit
  float mloc = -1e30f;
  auto score = [&](int it0, const u32x4q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = (it0 + u) * TSTEP + trow;
      float kf[16];
      unpack16_fp8(r[u], kf);
      float s = 0.f;
      if (t < Tk) {
#pragma unroll
        for (int j = 0; j < 16; ++j) s = fmaf(qv[j], kf[j], s);
      }
      s = group_reduce<LPR>(s, OpSum{});
      if (t < Tk) {
        if (sub == 0) sc[t] = s;
        mloc = fmaxf(mloc, s);
      }
    }
  };
  for (int it0 = 0; it0 < n_it; it0 += 2 * U) {
    if (it0 + U < n_it) issue(Kp, it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
    score(it0, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + 2 * U < n_it) issue(Kp, it0 + 2 * U, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + U < n_it) score(it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
  }
  issue(Vp, 0, ra);
  __builtin_amdgcn_sched_barrier(0);
  mloc = wave_max(mloc);
  if (lane == 0) red[wave] = mloc;
  __syncthreads();
  const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float lsum = 0.f;
  for (int t = tid; t < Tk; t += NWV * 64) {
    float p = __expf(sc[t] - mx);
    sc[t] = p;
    lsum += p;
  }
  lsum = wave_sum(lsum);
  if (lane == 0) red[NWV + wave] = lsum;
  __syncthreads();
  const float denom = (red[4] + red[5]) + (red[6] + red[7]);
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  auto accum = [&](int it0, const u32x4q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = (it0 + u) * TSTEP + trow;
      if (t < Tk) {
        float vf[16];
        unpack16_fp8(r[u], vf);
        const float p = sc[t];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
      }
    }
  };
  for (int it0 = 0; it0 < n_it; it0 += 2 * U) {
    if (it0 + U < n_it) issue(Vp, it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
    accum(it0, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + 2 * U < n_it) issue(Vp, it0 + 2 * U, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + U < n_it) accum(it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = stride4_sum(acc[j]);
  if (rin == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) part[wave * 64 + sub * 16 + j] = acc[j];
  }
  __syncthreads();
  if (tid < 64) {
    const float v = (part[tid] + part[64 + tid]) + (part[128 + tid] + part[192 + tid]);
    out[(int64_t)b * d + h * 64 + tid] = from_f<T>(v * vs / denom);   // V scale folded into the normalisation
  }
}

// false: shape unsupported (the caller takes the 16-bit kernel)
template <typename T>
bool launch_cross_attn_fp8(const T* q, const uint8_t* K8, const uint8_t* V8, const float* kscale, const float* vscale, T* out, int B, int H,
                           int Tk, hipStream_t s, SlabIn sq, const int32_t* done) {
  if constexpr (sizeof(T) != 2) return false;
  else {
    if (sq.n > 4 || Tk < 1) return false;
    const size_t lds = sizeof(float) * (Tk + 4 * 64 + 2 * 4);
    if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "cross_attn_fp8_kernel<%s, %s, 4> grid %d", sig_type<T>(), sq.n > 0 ? "true" : "false",
                                  H * B * 256);
    if (sq.n > 0) hipLaunchKernelGGL((cross_attn_fp8_kernel<T, true, 4>), dim3(H, B), dim3(256), lds, s, q, K8, V8, kscale, vscale, out, done, H, Tk, sq);
    else hipLaunchKernelGGL((cross_attn_fp8_kernel<T, false, 4>), dim3(H, B), dim3(256), lds, s, q, K8, V8, kscale, vscale, out, done, H, Tk, sq);
    return true;
  }
}
template bool launch_cross_attn_fp8<bf16_t>(const bf16_t*, const uint8_t*, const uint8_t*, const float*, const float*, bf16_t*, int, int, int,
                                            hipStream_t, SlabIn, const int32_t*);
template bool launch_cross_attn_fp8<f16_t>(const f16_t*, const uint8_t*, const uint8_t*, const float*, const float*, f16_t*, int, int, int,
                                           hipStream_t, SlabIn, const int32_t*);
template bool launch_cross_attn_fp8<float>(const float*, const uint8_t*, const uint8_t*, const float*, const float*, float*, int, int, int,
                                           hipStream_t, SlabIn, const int32_t*);

// The e4m3 form of cross_attn_mq_kernel (kernels_attn.hip): the NQ rows that share a clip's cross-KV (beam hypotheses, the rows of a
// sampled attempt) in ONE workgroup per (clip, head, frame slice); K and V are streamed once for all NQ queries.  Same slice
// protocol: every (row, slice) leaves {max, sum, unnormalised out[64]} for cross_attn_merge_kernel; a single slice is normalised
// and stored directly.  The K scale of (layer, clip, head) is folded into the queries, the V scale into what LEAVES the kernel
// (the merge kernel knows no scales); scores, softmax and accumulation in f32, no atomics.
// Register shape: 8 values per lane, 8 lanes per 64-byte row, 8-byte loads - NQ x 8 query values and
// NQ x 8 accumulators per lane as in the 16-bit kernel, and a load set of U x 2 registers instead of U x 4.  (16 values per lane,
// the per-row kernel's shape, would hold NQ x 16 + NQ x 16 = 224 registers at NQ = 7 before the two load sets.)
// NQ = kv_div = 2..7 only: one group per clip, every query row valid.
template <typename T, int NQ>
__global__ __launch_bounds__(256) void cross_attn_mq_fp8_kernel(const T* __restrict__ q, const uint8_t* __restrict__ K8,
                                                                const uint8_t* __restrict__ V8, const float* __restrict__ kscale,
                                                                const float* __restrict__ vscale, int H, int Tk, int chunk,
                                                                float* __restrict__ ws, SlabIn sq, T* __restrict__ out,
                                                                const int32_t* __restrict__ done) {
  static_assert(sizeof(T) == 2, "16-bit activations only");
  constexpr int VEC = 8, LPR = 8, RPI = 8;
  constexpr int U = NQ <= 5 ? 6 : 4;   // rows per lane and batch (two batches in flight), as in the 16-bit kernel
  extern __shared__ float sc[];  // [NQ][chunk] scores, then [4][NQ][64] partial outputs, [2][NQ][4] reductions
  const int h = blockIdx.x, clip = blockIdx.y, z = blockIdx.z, S = gridDim.z;
  const int row0 = clip * NQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = H * 64;
  const int sub = lane % LPR, rin = lane / LPR;
  float* part = sc + NQ * chunk;
  float* red = part + 4 * NQ * 64;
  if (done) {   // a group whose rows are ALL finished streams nothing; a partly finished group is computed whole
    int all = 1;
    for (int qi = 0; qi < NQ; ++qi) all &= sload_i32(done + row0 + qi) != 0;
    if (all) return;
  }
  const int t0 = z * chunk, n = min(chunk, Tk - t0);  // this slice: frames t0 .. t0+n-1 (n >= 1 by construction)
  const uint8_t* Kp = K8 + (((int64_t)clip * H + h) * Tk + t0) * 64 + sub * VEC;
  const uint8_t* Vp = V8 + (((int64_t)clip * H + h) * Tk + t0) * 64 + sub * VEC;
  const int n_it = (n + 4 * RPI - 1) / (4 * RPI);
  auto issue = [&](const uint8_t* base, int it0, u32x2q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = ((it0 + u) * 4 + wave) * RPI + rin;
      r[u] = __builtin_nontemporal_load((const u32x2q*)(base + (int64_t)min(t, n - 1) * 64));   // clamped, unconditional
    }
  };
  u32x2q ra[U], rb[U];
  issue(Kp, 0, ra);  // the stream starts before the queries are fetched
  const float ks = kscale[clip * H + h], vs = vscale[clip * H + h];
  float qv[NQ][VEC];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int64_t off = (int64_t)(row0 + qi) * d + h * 64 + sub * VEC;
    if (sq.n > 0) load_row_slabs<T>(sq, off, h * 64 + sub * VEC, qv[qi]);   // summed from the q GEMM's K-split partial tiles
    else RowVec<T>::load(q + off, qv[qi]);
#pragma unroll
    for (int j = 0; j < VEC; ++j) qv[qi][j] *= ks;   // K scale folded into the query
  }
  float mloc[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) mloc[qi] = -1e30f;
  auto score = [&](int it0, const u32x2q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = ((it0 + u) * 4 + wave) * RPI + rin;
      float kf[VEC];
      unpack8_fp8(r[u], kf);
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) s = fmaf(qv[qi][j], kf[j], s);
        s = group_reduce<LPR>(s, OpSum{});
        if (t < n) {
          if (sub == 0) sc[qi * chunk + t] = s;
          mloc[qi] = fmaxf(mloc[qi], s);
        }
      }
    }
  };
  for (int it0 = 0; it0 < n_it; it0 += 2 * U) {
    if (it0 + U < n_it) issue(Kp, it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);   // the next batch is requested before this one is scored
    score(it0, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + 2 * U < n_it) issue(Kp, it0 + 2 * U, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + U < n_it) score(it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
  }
  issue(Vp, 0, ra);  // V rows do not depend on the softmax: requested before it
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float m = wave_max(mloc[qi]);
    if (lane == 0) red[qi * 4 + wave] = m;
  }
  __syncthreads();
  float mx[NQ], lsum[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    mx[qi] = fmaxf(fmaxf(red[qi * 4], red[qi * 4 + 1]), fmaxf(red[qi * 4 + 2], red[qi * 4 + 3]));
    lsum[qi] = 0.f;
  }
  for (int t = tid; t < n; t += 256) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      const float p = __expf(sc[qi * chunk + t] - mx[qi]);
      sc[qi * chunk + t] = p;
      lsum[qi] += p;
    }
  }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float l = wave_sum(lsum[qi]);
    if (lane == 0) red[NQ * 4 + qi * 4 + wave] = l;
  }
  __syncthreads();
  float acc[NQ][VEC];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[qi][j] = 0.f;
  auto accum = [&](int it0, const u32x2q (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = ((it0 + u) * 4 + wave) * RPI + rin;
      if (t < n) {
        float vf[VEC];
        unpack8_fp8(r[u], vf);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          const float p = sc[qi * chunk + t];
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[qi][j] = fmaf(p, vf[j], acc[qi][j]);
        }
      }
    }
  };
  for (int it0 = 0; it0 < n_it; it0 += 2 * U) {
    if (it0 + U < n_it) issue(Vp, it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
    accum(it0, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + 2 * U < n_it) issue(Vp, it0 + 2 * U, ra);
    __builtin_amdgcn_sched_barrier(0);
    if (it0 + U < n_it) accum(it0 + U, rb);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[qi][j] = stride_reduce<LPR>(acc[qi][j], OpSum{});
    if (rin == 0) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) part[(wave * NQ + qi) * 64 + sub * VEC + j] = acc[qi][j];
    }
  }
  __syncthreads();
  for (int i = tid; i < NQ * 64; i += 256) {
    const int qi = i >> 6, c = i & 63;
    const float acc_c = ((part[(0 * NQ + qi) * 64 + c] + part[(1 * NQ + qi) * 64 + c]) + (part[(2 * NQ + qi) * 64 + c] + part[(3 * NQ + qi) * 64 + c])) * vs;   // V scale folded into the value that leaves the kernel
    const float lsl = (red[NQ * 4 + qi * 4] + red[NQ * 4 + qi * 4 + 1]) + (red[NQ * 4 + qi * 4 + 2] + red[NQ * 4 + qi * 4 + 3]);
    if (S == 1) {  // the only slice: finished here
      out[(int64_t)(row0 + qi) * d + h * 64 + c] = from_f<T>(acc_c / lsl);
      continue;
    }
    float* mine = ws + ((int64_t)((row0 + qi) * H + h) * S + z) * 66;
    mine[2 + c] = acc_c;
    if (c == 0) { mine[0] = mx[qi]; mine[1] = lsl; }  // every thread holds every query's maximum
  }
}

// The shapes launch_cross_attn_decode gives to cross_attn_mq_kernel, restricted to kv_div = 2..7, with the same slice rule and the
// same workspace check; false: not taken (the caller runs the 16-bit path, which then decides by its own rule).
template <typename T>
bool launch_cross_attn_mq_fp8(const T* q, const uint8_t* K8, const uint8_t* V8, const float* kscale, const float* vscale, T* out, int B,
                              int H, int Tk, int kv_div, const KernelOpts& ko, hipStream_t s, float* split_ws, SlabIn sq, int ws_rows, const int32_t* done) {
  if constexpr (sizeof(T) != 2) return false;
  else {
    if (ws_rows <= 0) ws_rows = B;
    if (!split_ws || kv_div < 2 || kv_div > 7 || B % kv_div != 0 || B * H < 256 || sq.n > 4 || Tk < 1) return false;
    const int A = B / kv_div;
    int Sq = cross_attn_splits(A, H, Tk);
    if (ko.xattn_mq_slices > 0) Sq = ko.xattn_mq_slices > 8 ? 8 : ko.xattn_mq_slices;
    const int chunk = ((Tk + Sq - 1) / Sq + 31) / 32 * 32;
    const int S2 = (Tk + chunk - 1) / chunk;  // every slice non-empty; S2 <= 8
    const size_t lds = sizeof(float) * ((size_t)kv_div * chunk + 4 * kv_div * 64 + 8 * kv_div);
    const bool ws_ok = S2 == 1 || (int64_t)B * S2 <= (int64_t)ws_rows * 8;  // one slice: stored directly, no workspace
    if (lds > 64 * 1024 || !ws_ok) return false;
    const dim3 grid(H, A, S2);
    if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "cross_attn_mq_fp8_kernel<%s, %d> grid %d slices %d%s", sig_type<T>(), kv_div,
                                  H * A * S2 * 256, S2, S2 > 1 ? " + cross_attn_merge_kernel" : "");
#define TTASR_MQ8(NQ_) \
  hipLaunchKernelGGL((cross_attn_mq_fp8_kernel<T, NQ_>), grid, dim3(256), lds, s, q, K8, V8, kscale, vscale, H, Tk, chunk, split_ws, sq, out, done)
    switch (kv_div) {
      case 2: TTASR_MQ8(2); break; case 3: TTASR_MQ8(3); break; case 4: TTASR_MQ8(4); break; case 5: TTASR_MQ8(5); break;
      case 6: TTASR_MQ8(6); break; default: TTASR_MQ8(7); break;
    }
#undef TTASR_MQ8
    if (S2 > 1) launch_cross_attn_merge<T>(split_ws, out, B, H, S2, done, s);
    return true;
  }
}
#define TTASR_MQ8_INST(T_) \
  template bool launch_cross_attn_mq_fp8<T_>(const T_*, const uint8_t*, const uint8_t*, const float*, const float*, T_*, int, int, int, int, \
                                             const KernelOpts&, hipStream_t, float*, SlabIn, int, const int32_t*)
TTASR_MQ8_INST(bf16_t); TTASR_MQ8_INST(f16_t); TTASR_MQ8_INST(float);
#undef TTASR_MQ8_INST
