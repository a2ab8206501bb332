// The real decode GEMM per Whisper-large shape in the round-2 form (K slices -> f32 slabs), un-profiled wall time per
// launch in a graph-replayed chain over 40 distinct (cold: 40 x 3..13 MB > Infinity Cache for the big ones) weight
// matrices, next to a synthetic kernel that only moves the same bytes (k_traffic: W once, x per workgroup).
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_skinny.hip"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#pragma clang diagnostic ignored "-Wunused-value"
template <class F> double timeit(hipStream_t s, F f, int reps) {
  f(); hipStreamSynchronize(s);
  auto t0 = std::chrono::high_resolution_clock::now();
  for (int i = 0; i < reps; ++i) f();
  hipStreamSynchronize(s);
  return std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count() / reps;
}
static void* dmal(size_t bytes, int fill_rand) {
  void* p; hipMalloc(&p, bytes);
  if (fill_rand) { std::vector<uint16_t> h(1 << 20); for (auto& v : h) v = 0x3c00 + (rand() & 0x1ff);
    for (size_t o = 0; o < bytes; o += h.size() * 2) hipMemcpy((char*)p + o, h.data(), std::min(bytes - o, h.size() * 2), hipMemcpyHostToDevice); }
  else hipMemset(p, 0, bytes);
  return p;
}
// same loads as gemm_skinny_kernel<NW, 1, U> (weights: steps x 1 KiB per wave; x: steps x 1 KiB per wave), no MFMA, one small store
template <int U>
__global__ void k_traffic(const u32x4* __restrict__ W, const bf16_t* __restrict__ x, float* __restrict__ out, int K, int ksplit, int nw) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nb = blockIdx.x, ks = blockIdx.y;
  const int ks_per = K / 16, steps = ks_per / (nw * ksplit), k0 = (ks * nw + wave) * steps;
  const u32x4* wp = W + ((int64_t)nb * ks_per + k0) * 64 + lane;
  const bf16_t* xp = x + (int64_t)(lane & 31) * K + k0 * 16 + 8 * (lane >> 5);
  u32x4 w[U], xv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { const int i = min(u, steps - 1); w[u] = wp[(int64_t)i * 64]; xv[u] = *(const u32x4*)(xp + i * 16); }
  unsigned a = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) a += w[u].x ^ xv[u].y;
  if (a == 0x12345u) out[threadIdx.x] = 1.f;
}
int main() {
  KernelOpts ko;   // the kernel-variant options the launchers are handed (common.hpp)
  const int B = 32, L = 40;
  hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  struct Shape { const char* name; int N, K, ks, act; } shapes[] = {
    {"qkv  N3840 K1280 ks4", 3840, 1280, 4, 0}, {"qkv  N3840 K1280 ks2", 3840, 1280, 2, 0}, {"qkv  N3840 K1280 ks1", 3840, 1280, 1, 0},
    {"out  N1280 K1280 ks4", 1280, 1280, 4, 0}, {"out  N1280 K1280 ks5", 1280, 1280, 5, 0}, {"out  N1280 K1280 ks10", 1280, 1280, 10, 0},
    {"fc1  N5120 K1280 gelu", 5120, 1280, 1, 1},
    {"fc2  N1280 K5120 ks8", 1280, 5120, 8, 0}, {"fc2  N1280 K5120 ks16", 1280, 5120, 16, 0}, {"fc2  N1280 K5120 ks4", 1280, 5120, 4, 0}};
  float* bias = (float*)dmal(5120 * 4, 0); float* slab = (float*)dmal((size_t)16 * B * 3840 * 4, 0);
  bf16_t* in = (bf16_t*)dmal(B * 5120 * 2, 1); bf16_t* out = (bf16_t*)dmal(B * 5120 * 2, 1);
  for (auto& sh : shapes) {
    std::vector<bf16_t*> w(L);
    for (auto& p : w) p = (bf16_t*)dmal((size_t)sh.N * sh.K * 2, 1);
    auto chain = [&](auto launch) {
      hipGraph_t gr; hipGraphExec_t ex;
      hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
      for (int i = 0; i < 80; ++i) launch(w[i % L]);
      hipStreamEndCapture(s, &gr); hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
      const double us = timeit(s, [&] { hipGraphLaunch(ex, s); }, 10) / 80;
      hipGraphExecDestroy(ex); hipGraphDestroy(gr);
      return us;
    };
    const double real = chain([&](bf16_t* W) {
      GemmEpi e; e.ldc = sh.N; e.act = sh.act;
      if (sh.ks > 1) launch_gemm_skinny(W, in, B, sh.N, sh.K, e, ko, s, sh.ks, slab, (int64_t)B * sh.N);
      else { e.bias = bias; e.out_t = out; launch_gemm_skinny(W, in, B, sh.N, sh.K, e, ko, s); } });
    const int ks_per = sh.K / 16;
    int nw = 4; if (sh.ks == 1) { while (nw < 16 && ks_per % (nw * 2) == 0 && ks_per / nw > 10) nw *= 2; if (nw < 8) nw = 8; }
    const int steps = ks_per / (nw * sh.ks);
    const double traffic = chain([&](bf16_t* W) {
      dim3 grid(sh.N / 32, sh.ks);
      if (steps <= 5) hipLaunchKernelGGL(k_traffic<5>, grid, dim3(nw * 64), 0, s, (const u32x4*)W, in, (float*)out, sh.K, sh.ks, nw);
      else hipLaunchKernelGGL(k_traffic<10>, grid, dim3(nw * 64), 0, s, (const u32x4*)W, in, (float*)out, sh.K, sh.ks, nw); });
    const double mb = (double)sh.N * sh.K * 2 / 1e6;
    printf("%-24s grid %4d x %2d, %2d waves, %2d steps: real %6.2f us  traffic-only %6.2f us  (%.1f MB, %.2f TB/s real)\n", sh.name,
           sh.N / 32, sh.ks, nw, steps, real, traffic, mb, mb / real);
    for (auto& p : w) hipFree(p);
  }
  return 0;
}
