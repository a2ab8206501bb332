// Prototype (timing + correctness probe, NOT in the product): LayerNorm folded into the launch of the decode GEMM
// that consumes it, with an in-launch hand-off instead of a kernel boundary.
//
//   separate : [residual GEMM, split-K atomics -> x]  ->  [LayerNorm x -> h]  ->  [GEMM h x W -> out]
//   fused    : [residual GEMM, split-K atomics -> x]  ->  [ LN producers (4 workgroups) || GEMM consumers (n_blocks) ]
//
// In the fused launch every consumer issues its weight loads first (they depend on nothing), then one lane polls an
// arrival counter the producers bump after their write-through (sc1) stores of h have drained, then the workgroup
// loads its slice of h with sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility: "every store sc1 + drained,
// every load sc1" form) and runs the MFMAs.  The counter is monotonic: target = producers * (*step + 1), with *step
// advanced by a one-thread kernel per replay exactly like the engine's decode step counter, so nothing is re-zeroed.
// Spins are bounded (a timeout word is set and the kernel proceeds) so that a mistake cannot hang the box.
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_misc.hip"
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_skinny.hip"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#pragma clang diagnostic ignored "-Wunused-value"

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;

template <int NW>
__global__ __launch_bounds__(NW * 64) void ln_gemm_fused_kernel(const bf16_t* __restrict__ Wsh, const float* __restrict__ x,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                bf16_t* h, unsigned* counter, const int* __restrict__ step,
                                                                unsigned* timeout, int B, int N, int K, int n_prod, GemmEpi e) {
  constexpr int U = 10;
  __shared__ __attribute__((aligned(16))) float red[NW][32 * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x < n_prod) {
    // ---- LN producer: one wave per row (d = K <= 1280), rows blockIdx.x * NW + wave ----
    const int row = blockIdx.x * NW + wave;
    if (row < B) {
      const float4* xr = (const float4*)(x + (int64_t)row * K);
      const int nv = K >> 2;
      float4 v[5], gm[5], bt[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int i = min(lane + 64 * j, nv - 1);
        v[j] = xr[i]; gm[j] = ((const float4*)gamma)[i]; bt[j] = ((const float4*)beta)[i];
      }
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) if (lane + 64 * j < nv) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
      const float mean = wave_sum(s) / K;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j)
        if (lane + 64 * j < nv) {
          float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d2 = v[j].w - mean;
          q += (a * a + b * b) + (c * c + d2 * d2);
        }
      const float rstd = rsqrtf(wave_sum(q) / K + 1e-5f);
      gu64* o = (gu64*)(h + (int64_t)row * K);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) {
          typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
          bf2 lo = {(__bf16)((v[j].x - mean) * rstd * gm[j].x + bt[j].x), (__bf16)((v[j].y - mean) * rstd * gm[j].y + bt[j].y)};
          bf2 hi = {(__bf16)((v[j].z - mean) * rstd * gm[j].z + bt[j].z), (__bf16)((v[j].w - mean) * rstd * gm[j].w + bt[j].w)};
          const unsigned long long pk = (unsigned long long)__builtin_bit_cast(uint32_t, lo) |
                                        ((unsigned long long)__builtin_bit_cast(uint32_t, hi) << 32);
          __hip_atomic_store(o + i, pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // 8-byte write-through (sc1) store
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add((gu32*)counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // ---- GEMM consumer (gemm_skinny_kernel<NW, 1> with the hand-off in front of the h loads) ----
  const int nb = blockIdx.x - n_prod;
  const int ks_per = K / 16, steps = ks_per / NW, k0 = wave * steps;
  const u32x4* wp = (const u32x4*)Wsh + ((int64_t)nb * ks_per + k0) * 64 + lane;
  const gu64* xp = (const gu64*)(h + (int64_t)min(lane & 31, B - 1) * K + k0 * 16 + 8 * (lane >> 5));
  const int eb = min(tid >> 3, B - 1), en = nb * 32 + 4 * (tid & 7);
  float4 ebias = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 256 && en + 3 < N && e.bias) ebias = *(const float4*)(e.bias + en);
  u32x4 w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = wp[(int64_t)min(u, steps - 1) * 64];      // weights first: they depend on nothing
  __shared__ int s_ok;
  if (tid == 0) {
    const unsigned target = (unsigned)n_prod * (unsigned)(*step + 1);
    unsigned spins = 0;
    int ok = 1;
    while (__hip_atomic_load((gu32*)counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (++spins > (1u << 20)) { *timeout = 1; ok = 0; break; }
      __builtin_amdgcn_s_sleep(1);
    }
    s_ok = ok;
  }
  __syncthreads();
  u32x4 xv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {   // every load of the handed-off bytes is an sc1 load (two 8-byte halves)
    const gu64* p = xp + (int64_t)min(u, steps - 1) * 4;
    const unsigned long long lo = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    xv[u] = u32x4{(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
  }
  f32x16 acc;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < steps) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(s16x8*)&w[u], *(s16x8*)&xv[u], acc, 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *(float4*)&red[wave][(lane & 31) * 32 + 8 * g + 4 * (lane >> 5)] = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  __syncthreads();
  if (tid >= 256) return;
  float4 v = *(const float4*)&red[0][(tid >> 3) * 32 + 4 * (tid & 7)];
#pragma unroll
  for (int ww = 1; ww < NW; ++ww) {
    const float4 t = *(const float4*)&red[ww][(tid >> 3) * 32 + 4 * (tid & 7)];
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  v.x += ebias.x; v.y += ebias.y; v.z += ebias.z; v.w += ebias.w;
  if ((tid >> 3) >= B || en + 3 >= N) return;
  uint2 pk;
  pk.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
  pk.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
  *(uint2*)((bf16_t*)e.out_t + (int64_t)eb * e.ldc + en) = pk;
}

__global__ void bump(int* step) { *step += 1; }

template <class F> double timeit(hipStream_t s, F f, int reps) {
  f(); hipStreamSynchronize(s);
  auto t0 = std::chrono::high_resolution_clock::now();
  for (int i = 0; i < reps; ++i) f();
  hipStreamSynchronize(s);
  return std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count() / reps;
}
static void* dmal(size_t bytes, int mode) {
  void* p; hipMalloc(&p, bytes);
  if (mode == 1) { std::vector<uint16_t> h(bytes / 2); for (auto& v : h) v = 0x3c00 + (rand() & 0x1ff) - ((rand() & 1) << 15); hipMemcpy(p, h.data(), bytes, hipMemcpyHostToDevice); }
  else if (mode == 2) { std::vector<float> h(bytes / 4); for (auto& v : h) v = (rand() % 2001 - 1000) * 1e-3f; hipMemcpy(p, h.data(), bytes, hipMemcpyHostToDevice); }
  else hipMemset(p, 0, bytes);
  return p;
}

int main() {
  KernelOpts ko;   // the kernel-variant options the launchers are handed (common.hpp)
  const int B = 32, d = 1280, L = 16;   // L independent (counter, weights) instances per replay, like layers
  hipStream_t s; hipStreamCreate(&s);
  struct Shape { const char* name; int N; } shapes[] = {{"q (N=1280)", 1280}, {"qkv (N=3840)", 3840}, {"fc1 (N=5120)", 5120}};
  float* x = (float*)dmal((size_t)B * d * 4, 2);
  float* gamma = (float*)dmal(d * 4, 2); float* beta = (float*)dmal(d * 4, 2); float* bias = (float*)dmal(5120 * 4, 2);
  bf16_t* att = (bf16_t*)dmal((size_t)B * d * 2, 1);
  bf16_t* h_sep = (bf16_t*)dmal((size_t)B * d * 2, 0); bf16_t* h_fus = (bf16_t*)dmal((size_t)B * d * 2, 0);
  bf16_t* out_sep = (bf16_t*)dmal((size_t)B * 5120 * 2, 0); bf16_t* out_fus = (bf16_t*)dmal((size_t)B * 5120 * 2, 0);
  unsigned* counters = (unsigned*)dmal(4096, 0); unsigned* timeout = (unsigned*)dmal(16, 0); int* step = (int*)dmal(16, 0);
  std::vector<bf16_t*> wo(L), wg(L);
  for (int l = 0; l < L; ++l) { wo[l] = (bf16_t*)dmal((size_t)d * d * 2, 1); wg[l] = (bf16_t*)dmal((size_t)5120 * d * 2, 1); }
  const int NW = 8, n_prod = (B + NW - 1) / NW;
  for (auto& sh : shapes) {
    const int N = sh.N;
    auto residual = [&](int l) { GemmEpi e; e.bias = bias; e.residual = x; e.out_f32 = x; e.ldc = d; launch_gemm_skinny(wo[l], att, B, d, d, e, ko, s); };
    auto sep = [&](int l) {
      residual(l);
      launch_layernorm<bf16_t>(x, gamma, beta, h_sep, B, d, s);
      GemmEpi e; e.bias = bias; e.out_t = out_sep; e.ldc = N; launch_gemm_skinny(wg[l], h_sep, B, N, d, e, ko, s);
    };
    auto fus = [&](int l) {
      residual(l);
      GemmEpi e; e.bias = bias; e.out_t = out_fus; e.ldc = N;
      hipLaunchKernelGGL((ln_gemm_fused_kernel<NW>), dim3(n_prod + N / 32), dim3(NW * 64), 0, s, wg[l], x, gamma, beta, h_fus,
                         counters + 16 * l, step, timeout, B, N, d, n_prod, e);
    };
    double t[2];
    for (int variant = 0; variant < 2; ++variant) {
      hipMemsetAsync(x, 0, (size_t)B * d * 4, s); hipMemsetAsync(counters, 0, 4096, s); hipMemsetAsync(step, 0, 16, s);
      hipGraph_t gr; hipGraphExec_t ex;
      hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
      for (int rep = 0; rep < 4; ++rep) {
        for (int l = 0; l < L; ++l) { if (variant == 0) sep(l); else fus(l); }
        hipLaunchKernelGGL(bump, dim3(1), dim3(1), 0, s, step);
      }
      // the counters advance once per (instance, rep): give every rep its own epoch by bumping *step after each sweep
      hipStreamEndCapture(s, &gr); hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
      t[variant] = timeit(s, [&] { hipGraphLaunch(ex, s); }, 20) / (4 * L);
      hipGraphExecDestroy(ex); hipGraphDestroy(gr);
    }
    // correctness probe: same x -> same h and out from both forms (one instance, outside the graph)
    hipMemsetAsync(counters, 0, 4096, s); hipMemsetAsync(step, 0, 16, s);
    { std::vector<float> hx((size_t)B * d); for (auto& v : hx) v = (rand() % 4001 - 2000) * 1e-3f; hipMemcpyAsync(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice, s); hipStreamSynchronize(s); }
    launch_layernorm<bf16_t>(x, gamma, beta, h_sep, B, d, s);
    { GemmEpi e; e.bias = bias; e.out_t = out_sep; e.ldc = N; launch_gemm_skinny(wg[0], h_sep, B, N, d, e, ko, s); }
    { GemmEpi e; e.bias = bias; e.out_t = out_fus; e.ldc = N;
      hipLaunchKernelGGL((ln_gemm_fused_kernel<NW>), dim3(n_prod + N / 32), dim3(NW * 64), 0, s, wg[0], x, gamma, beta, h_fus, counters, step, timeout, B, N, d, n_prod, e); }
    hipStreamSynchronize(s);
    std::vector<uint16_t> a((size_t)B * N), b((size_t)B * N), ha((size_t)B * d), hb((size_t)B * d);
    hipMemcpy(a.data(), out_sep, a.size() * 2, hipMemcpyDeviceToHost); hipMemcpy(b.data(), out_fus, b.size() * 2, hipMemcpyDeviceToHost);
    hipMemcpy(ha.data(), h_sep, ha.size() * 2, hipMemcpyDeviceToHost); hipMemcpy(hb.data(), h_fus, hb.size() * 2, hipMemcpyDeviceToHost);
    size_t bad = 0, badh = 0;
    for (size_t i = 0; i < a.size(); ++i) bad += a[i] != b[i];
    for (size_t i = 0; i < ha.size(); ++i) badh += ha[i] != hb[i];
    unsigned tmo; hipMemcpy(&tmo, timeout, 4, hipMemcpyDeviceToHost);
    printf("%-14s residual+LN+GEMM %.2f us   residual+fused %.2f us   (saves %.2f us per pair)  mismatches h %zu out %zu  timeout %u\n",
           sh.name, t[0], t[1], t[0] - t[1], badh, bad, tmo);
  }
  return 0;
}
