// Round 3: does a weight PREFETCH into the Infinity Cache pay in the decode chain?  Same chain as layer_bench2 (real kernels,
// 32 layers of distinct cold weights and cross-KV, B = 32, position 64, graph replays, wall clock) plus a forked graph branch
// per layer that touches layer l+1's 46 MB of fragment-packed weights while layer l's post-cross-attention kernels run
// (HBM is nearly idle there), joined before cross-attention l+1 (so the prefetch never competes with the HBM-bound stream).
//   layer_bench3 <mode> <prefetch_wgs> <nt>     mode 0 baseline; 1 fork after xattn(l), join before xattn(l+1);
//                                               2 fork after xattn(l), join at the end of layer l (before LN1 of l+1);
//                                               3 fork at the start of layer l (prefetch l+1 under the WHOLE layer l, incl. xattn)
//                                               4 no fork: the prefetch of layer l+1 runs IN the chain right after xattn(l)
//                                               5 upper bound: every layer uses layer 0's weights (46 MB that can stay in the
//                                                 Infinity Cache between layers, against the 246 MB each cross-attention streams)
//                                               6 as 5 and every layer also re-reads layer 0's cross-KV (everything cache-resident)
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_misc.hip"
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_skinny.hip"
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_attn.hip"
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
  void* p;
  if (hipMalloc(&p, bytes) != hipSuccess) { printf("alloc of %zu failed\n", bytes); exit(1); }
  if (fill_rand) { std::vector<uint16_t> h(1 << 20); for (auto& v : h) v = 0x3c00 + (rand() & 0x1ff);
    for (size_t o = 0; o < bytes; o += h.size() * 2) hipMemcpy((char*)p + o, h.data(), std::min(bytes - o, h.size() * 2), hipMemcpyHostToDevice); }
  else hipMemset(p, 0, bytes);
  return p;
}
struct PfArgs { const uint4* p[6]; unsigned n16[6]; };   // six matrices, sizes in 16-byte chunks
// stream every byte once with coalesced 16-byte loads (1 KiB per wave-instruction), 8 loads in flight per lane
__global__ __launch_bounds__(256) void prefetch_kernel(PfArgs a) {
  const unsigned tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    const unsigned nl = a.n16[m];
    for (unsigned i = tid; i < nl; i += nth * 8) {
      uint4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const unsigned j = min(i + u * nth, nl - 1); v[u] = a.p[m][j]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { acc.x ^= v[u].x; acc.y ^= v[u].y; }
    }
  }
  if (acc.x == 0x12345678u && acc.y == 0x9abcdef0u) ((uint4*)a.p[0])[0] = acc;   // never true: keeps the loads alive
}
int main(int argc, char** argv) {
  const int B = 32, d = 1280, F = 5120, H = 20, T = 1500, L = 32;
  const int mode = argc > 1 ? atoi(argv[1]) : 0, pf_wgs = argc > 2 ? atoi(argv[2]) : 128, nt = argc > 3 ? atoi(argv[3]) : 1;
  const int ks_d = 4, ks_q = 4, ks_qkv = 2, ks_f = 8;
  KernelOpts ko;
  ko.xattn_variant = 1;
  ko.skinny_nt = nt;
  hipStream_t s, s2; hipStreamCreateWithFlags(&s, hipStreamNonBlocking); hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
  float* x = (float*)dmal(B * d * 4, 0); float* g = (float*)dmal(d * 4, 0); float* bt = (float*)dmal(d * 4, 0);
  float* bias = (float*)dmal(F * 4, 0); float* slab = (float*)dmal((size_t)16 * B * 3 * d * 4, 0);
  bf16_t *h = (bf16_t*)dmal(B * d * 2, 1), *qkv = (bf16_t*)dmal(B * 3 * d * 2, 1), *att = (bf16_t*)dmal(B * d * 2, 1),
         *q = (bf16_t*)dmal(B * d * 2, 1), *mid = (bf16_t*)dmal(B * F * 2, 1);
  std::vector<bf16_t*> wqkv(L), wo(L), wq(L), wox(L), w1(L), w2(L), xk(L), xv(L);
  for (int l = 0; l < L; ++l) {
    wqkv[l] = (bf16_t*)dmal((size_t)3 * d * d * 2, 1); wo[l] = (bf16_t*)dmal((size_t)d * d * 2, 1); wq[l] = (bf16_t*)dmal((size_t)d * d * 2, 1);
    wox[l] = (bf16_t*)dmal((size_t)d * d * 2, 1); w1[l] = (bf16_t*)dmal((size_t)F * d * 2, 1); w2[l] = (bf16_t*)dmal((size_t)F * d * 2, 1);
    xk[l] = (bf16_t*)dmal((size_t)B * H * T * 64 * 2, 1); xv[l] = (bf16_t*)dmal((size_t)B * H * T * 64 * 2, 1);
  }
  const int pps = 28; bf16_t* pool = (bf16_t*)dmal((size_t)B * pps * 2 * H * 16 * 64 * 2, 1);
  int32_t* pt = (int32_t*)dmal(B * pps * 4, 0); int32_t* step = (int32_t*)dmal(16, 0);
  { int v = 64; hipMemcpy(step, &v, 4, hipMemcpyHostToDevice); }
  std::vector<hipEvent_t> evf(L), evj(L);
  for (int l = 0; l < L; ++l) { hipEventCreateWithFlags(&evf[l], hipEventDisableTiming); hipEventCreateWithFlags(&evj[l], hipEventDisableTiming); }
  auto pf = [&](int l) {   // prefetch layer l's matrices on s2
    PfArgs a;
    const bf16_t* ps[6] = {wqkv[l], wo[l], wq[l], wox[l], w1[l], w2[l]};
    const size_t nb[6] = {(size_t)3 * d * d * 2, (size_t)d * d * 2, (size_t)d * d * 2, (size_t)d * d * 2, (size_t)F * d * 2, (size_t)F * d * 2};
    for (int m = 0; m < 6; ++m) { a.p[m] = (const uint4*)ps[m]; a.n16[m] = (unsigned)(nb[m] / 16); }
    hipLaunchKernelGGL(prefetch_kernel, dim3(pf_wgs), dim3(256), 0, s2, a);
  };
  auto split = [&](const bf16_t* W, const bf16_t* A, int N, int K, int ks, const float* b) {
    SlabIn si;
    GemmEpi e; e.ldc = N;
    if (ks > 1) { launch_gemm_skinny(W, A, B, N, K, e, ko, s, ks, slab, (int64_t)B * N); si.slab = slab; si.bias = b; si.n = ks; si.stride = (int64_t)B * N; si.ld = N; }
    return si;
  };
  int pend = 0;
  auto ln = [&]() {
    LnPre pre; pre.x_out = x;
    if (pend) { pre.bias = bias; pre.slab = slab; pre.n_slab = pend; pre.slab_stride = (int64_t)B * d; }
    launch_layernorm_rows<bf16_t>(x, g, bt, h, B, d, pre, s);
    pend = 0;
  };
  bool pending_join[64] = {false};
  auto layer = [&](int l0) {
    const int l = l0;
    const int lw = (mode == 5 || mode == 6) ? 0 : l0, lk = mode == 6 ? 0 : l0;
    if (mode == 3 && l + 1 < L) { hipEventRecord(evf[l], s); hipStreamWaitEvent(s2, evf[l], 0); pf(l + 1); hipEventRecord(evj[l], s2); pending_join[l + 1] = true; }
    if (mode == 3 && pending_join[l]) { hipStreamWaitEvent(s, evj[l - 1], 0); pending_join[l] = false; }
    ln();
    SlabIn sqkv = split(wqkv[lw], h, 3 * d, d, ks_qkv, bias);
    launch_self_attn_decode<bf16_t>(qkv, pool, pt, pps, 0, 1, 0, step, att, B, H, s, sqkv);
    pend = split(wo[lw], att, d, d, ks_d, bias).n;
    ln();
    SlabIn sq = split(wq[lw], h, d, d, ks_q, bias);
    if (mode == 1 && pending_join[l]) { hipStreamWaitEvent(s, evj[l - 1], 0); pending_join[l] = false; }
    launch_cross_attn_decode<bf16_t>(q, xk[lk], xv[lk], att, B, H, T, 1, ko, s, nullptr, sq);
    if (mode == 4 && l + 1 < L) { hipStream_t keep = s2; s2 = s; pf(l + 1); s2 = keep; }
    if ((mode == 1 || mode == 2) && l + 1 < L) { hipEventRecord(evf[l], s); hipStreamWaitEvent(s2, evf[l], 0); pf(l + 1); hipEventRecord(evj[l], s2); pending_join[l + 1] = true; }
    pend = split(wox[lw], att, d, d, ks_d, bias).n;
    ln();
    { GemmEpi e; e.bias = bias; e.act = 1; e.out_t = mid; e.ldc = F; launch_gemm_skinny(w1[lw], h, B, F, d, e, ko, s); }
    pend = split(w2[lw], mid, d, F, ks_f, bias).n;
    if (mode == 2 && l + 1 < L) { hipStreamWaitEvent(s, evj[l], 0); pending_join[l + 1] = false; }
  };
  // the prefetch kernel alone (a chain of 32, cold weights), for scale
  { hipGraph_t g2; hipGraphExec_t x2;
    hipStreamBeginCapture(s2, hipStreamCaptureModeThreadLocal);
    for (int l = 0; l < L; ++l) pf(l);
    hipStreamEndCapture(s2, &g2); hipGraphInstantiate(&x2, g2, nullptr, nullptr, 0);
    printf("prefetch alone: %.2f us per layer (46 MB, %d workgroups)\n", timeit(s2, [&] { hipGraphLaunch(x2, s2); }, 5) / L, pf_wgs); }
  hipGraph_t gr; hipGraphExec_t ex;
  hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
  for (int l = 0; l < L; ++l) layer(l);
  hipError_t e1 = hipStreamEndCapture(s, &gr);
  hipError_t e2 = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
  if (e1 != hipSuccess || e2 != hipSuccess) { printf("capture failed: %s %s\n", hipGetErrorString(e1), hipGetErrorString(e2)); return 1; }
  double best = 1e30;
  for (int r = 0; r < 3; ++r) best = std::min(best, timeit(s, [&] { hipGraphLaunch(ex, s); }, 10) / L);
  printf("mode=%d prefetch_wgs=%d weights_nt=%d: %.2f us per layer (%.3f ms per 32-layer step)\n", mode, pf_wgs, nt, best, best * L / 1000);
  return 0;
}
