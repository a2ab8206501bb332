#define TTASR_EXPERIMENTS 1   // QMODE 2 of the cross-attention kernel is compiled in lab builds only
// Round 4: decoder-layer chain with projections folded INTO the attention kernels, against the shipped
// 11-launch plan.  Real kernels, 32 layers of distinct cold weights and cross-KV, B = 32, position 64, graph replays, wall clock.
//   variant 0  shipped plan (LN, qkv, self-attn, out-proj, LN, q, cross-attn, out-proj, LN, fc1, fc2)
//   variant 1  cross-attention computes its own query (QMODE 2): no q GEMM                               (10 launches)
//   variant 2  self-attention + out-projection in one launch, G = 4 rows per workgroup, per-head slabs  (10 launches)
//   variant 3  as 2 with G = 8
//   variant 4  1 + 2                                                                                     (9 launches)
// Each variant is first CHECKED against variant 0 on one layer (same inputs: the residual rows after LN2 / the cross-attention
// output), then timed.  hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-kernarg-preload-count=16 tools/microbench/layer_bench4.hip -o ...
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_misc.hip"
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_skinny.hip"
#include "../../taiwan_tongues_asr_ce_amd/csrc/kernels_attn.hip"
#include "fused_attn_oproj.hip"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cmath>
#pragma clang diagnostic ignored "-Wunused-value"
// the flash kernel lives in another translation unit of the library; the decode path at kv_div == 1 never calls it
template <typename T16> void launch_cross_attn_flash_bf16(const T16*, const T16*, const T16*, T16*, int, int, int, int, hipStream_t) {}
template void launch_cross_attn_flash_bf16<bf16_t>(const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, int, int, hipStream_t);
template void launch_cross_attn_flash_bf16<f16_t>(const f16_t*, const f16_t*, const f16_t*, f16_t*, int, int, int, int, hipStream_t);
template <class F> double timeit(hipStream_t s, F f, int reps) {
  f(); hipStreamSynchronize(s);
  auto t0 = std::chrono::high_resolution_clock::now();
  for (int i = 0; i < reps; ++i) f();
  hipStreamSynchronize(s);
  return std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count() / reps;
}
static uint16_t f2b(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }
static float b2f(uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static void* dmal(size_t bytes, int fill, float scale = 1.f) {   // fill 0: zeros, 1: random bf16 in [-scale, scale), 2: random f32
  void* p;
  if (hipMalloc(&p, bytes) != hipSuccess) { printf("alloc of %zu failed\n", bytes); exit(1); }
  if (fill == 1) { std::vector<uint16_t> h(1 << 20); for (auto& v : h) v = f2b(scale * ((rand() & 0xffff) / 32768.f - 1.f));
    for (size_t o = 0; o < bytes; o += h.size() * 2) hipMemcpy((char*)p + o, h.data(), std::min(bytes - o, h.size() * 2), hipMemcpyHostToDevice); }
  else if (fill == 2) { std::vector<float> h(1 << 18); for (auto& v : h) v = scale * ((rand() & 0xffff) / 32768.f - 1.f);
    for (size_t o = 0; o < bytes; o += h.size() * 4) hipMemcpy((char*)p + o, h.data(), std::min(bytes - o, h.size() * 4), hipMemcpyHostToDevice); }
  else hipMemset(p, 0, bytes);
  return p;
}
int main(int argc, char** argv) {
  const int B = 32, d = 1280, F = 5120, H = 20, T = 1500, L = 32;
  const int only = argc > 1 ? atoi(argv[1]) : -1;
  const int reps = argc > 2 ? atoi(argv[2]) : 10;
  KernelOpts ko;   // the defaults are what ships: nontemporal, software-pipelined cross-attention
  hipStream_t s; hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  float* x = (float*)dmal(B * d * 4, 2); float* x0 = (float*)dmal(B * d * 4, 2); float* g = (float*)dmal(d * 4, 2); float* bt = (float*)dmal(d * 4, 2);
  float* bias = (float*)dmal(F * 4, 2, 0.1f);
  float* slab = (float*)dmal((size_t)20 * B * 3 * d * 4, 0);
  bf16_t *h = (bf16_t*)dmal(B * d * 2, 1), *qkv = (bf16_t*)dmal(B * 3 * d * 2, 1), *att = (bf16_t*)dmal(B * d * 2, 1),
         *q = (bf16_t*)dmal(B * d * 2, 1), *mid = (bf16_t*)dmal(B * F * 2, 1);
  // row-major Wq (the fused cross-attention reads rows) beside the fragment-packed copies (here: independent random bits for
  // timing; for the CHECK layer 0's packed Wq / Wo are built from the row-major matrices)
  std::vector<bf16_t*> wqkv(L), wo(L), wq(L), wq_rm(L), wox(L), w1(L), w2(L), xk(L), xv(L);
  const float ws = 0.03f;
  for (int l = 0; l < L; ++l) {
    wqkv[l] = (bf16_t*)dmal((size_t)3 * d * d * 2, 1, ws); wo[l] = (bf16_t*)dmal((size_t)d * d * 2, 1, ws); wq[l] = (bf16_t*)dmal((size_t)d * d * 2, 1, ws);
    wq_rm[l] = (bf16_t*)dmal((size_t)d * d * 2, 1, ws);
    wox[l] = (bf16_t*)dmal((size_t)d * d * 2, 1, ws); w1[l] = (bf16_t*)dmal((size_t)F * d * 2, 1, ws); w2[l] = (bf16_t*)dmal((size_t)F * d * 2, 1, ws);
    xk[l] = (bf16_t*)dmal((size_t)B * H * T * 64 * 2, 1); xv[l] = (bf16_t*)dmal((size_t)B * H * T * 64 * 2, 1);
  }
  {  // layer 0: packed Wq = shuffle(row-major Wq) so that variant 1 can be checked against variant 0
    float* tmp = (float*)dmal((size_t)d * d * 4, 0);
    launch_uncast<bf16_t>(wq_rm[0], tmp, (int64_t)d * d, s);
    launch_shuffle_cast<bf16_t>(tmp, wq[0], d, d, 0, ko, s);
    hipStreamSynchronize(s); hipFree(tmp);
  }
  const int pps = 28; bf16_t* pool = (bf16_t*)dmal((size_t)B * pps * 2 * H * 16 * 64 * 2, 1);
  int32_t* pt = (int32_t*)dmal(B * pps * 4, 0); int32_t* step = (int32_t*)dmal(16, 0);
  { int v = argc > 3 ? atoi(argv[3]) : 64; hipMemcpy(step, &v, 4, hipMemcpyHostToDevice); printf("position %d\n", v); }
  float* x_ln2 = (float*)dmal(B * d * 4, 0);   // check only: the residual rows right after LN2's sum (before the cross-attention)
  bool snap = false;
  auto run_layer = [&](int l, int variant, int& pend, int64_t& pend_stride) {
    auto ln = [&]() {
      LnPre pre; pre.x_out = x;
      if (pend) { pre.bias = bias; pre.slab = slab; pre.n_slab = pend; pre.slab_stride = pend_stride; }
      launch_layernorm_rows<bf16_t>(x, g, bt, h, B, d, pre, s);
      pend = 0;
    };
    auto split = [&](const bf16_t* W, const bf16_t* A, int N, int K, int ks, const float* b) {
      SlabIn si; GemmEpi e; e.ldc = N;
      launch_gemm_skinny(W, A, B, N, K, e, ko, s, ks, slab, (int64_t)B * N);
      si.slab = slab; si.bias = b; si.n = ks; si.stride = (int64_t)B * N; si.ld = N;
      return si;
    };
    const bool fuse_q = variant == 1 || variant == 4, fuse_o = variant == 2 || variant == 3 || variant == 4;
    ln();
    SlabIn sqkv = split(wqkv[l], h, 3 * d, d, 2, bias);
    if (variant == 5) {   // one wave per (row, head) self-attention (no workgroup barriers), standard out-proj GEMM
      launch_self_attn_wave<bf16_t>(pool, pt, pps, 0, 1, 0, step, B, H, sqkv, qkv, att, s);
      pend = split(wo[l], att, d, d, 4, bias).n; pend_stride = (int64_t)B * d;
      ln();
    } else if (fuse_o) {
      // the qkv slabs occupy slab[0 .. 2*B*3d); the per-head out-proj slabs go behind them
      float* oslab = slab + (size_t)2 * B * 3 * d;
      launch_self_attn_oproj<bf16_t>(pool, pt, pps, 0, 1, 0, step, B, H, sqkv, qkv, wo[l], oslab, (int64_t)B * d, variant == 3 ? 8 : 4, s);
      // LN2 sums the H per-head slabs
      LnPre pre; pre.x_out = x; pre.bias = bias; pre.slab = oslab; pre.n_slab = H; pre.slab_stride = (int64_t)B * d;
      launch_layernorm_rows<bf16_t>(x, g, bt, h, B, d, pre, s);
    } else {
      launch_self_attn_decode<bf16_t>(qkv, pool, pt, pps, 0, 1, 0, step, att, B, H, s, sqkv);
      pend = split(wo[l], att, d, d, 4, bias).n; pend_stride = (int64_t)B * d;
      ln();
    }
    if (snap) hipMemcpyAsync(x_ln2, x, (size_t)B * d * 4, hipMemcpyDeviceToDevice, s);
    if (fuse_q) {
      QProj qp; qp.x = h; qp.W = wq_rm[l]; qp.bias = bias;
      launch_cross_attn_decode<bf16_t>(q, xk[l], xv[l], att, B, H, T, 1, ko, s, nullptr, SlabIn{}, 0, qp);
    } else {
      SlabIn sq = split(wq[l], h, d, d, 4, bias);
      launch_cross_attn_decode<bf16_t>(q, xk[l], xv[l], att, B, H, T, 1, ko, s, nullptr, sq);
    }
    pend = split(wox[l], att, d, d, 4, bias).n; pend_stride = (int64_t)B * d;
    ln();
    { GemmEpi e; e.bias = bias; e.act = 1; e.out_t = mid; e.ldc = F; launch_gemm_skinny(w1[l], h, B, F, d, e, ko, s); }
    pend = split(w2[l], mid, d, F, 8, bias).n; pend_stride = (int64_t)B * d;
  };
  // ---- checks on layer 0: x after the layer's LN3 input sums (residual rows) and the cross-attention output
  std::vector<float> xr((size_t)B * d), xt((size_t)B * d);
  std::vector<uint16_t> ar((size_t)B * d), at_((size_t)B * d);
  auto run_check = [&](int variant, std::vector<float>& xo, std::vector<uint16_t>& ao) {
    hipMemcpy(x, x0, (size_t)B * d * 4, hipMemcpyDeviceToDevice);
    int pend = 0; int64_t ps = 0;
    snap = true;
    run_layer(0, variant, pend, ps);
    snap = false;
    hipStreamSynchronize(s);
    // variants 2-4: the rows after LN2's sum (the self-attention + out-projection result; what follows amplifies last-bit
    // differences through a peaked softmax over random data); variant 1: the rows after LN3's sum (cross-attention + out-proj)
    hipMemcpy(xo.data(), variant == 1 || variant == 0 ? x : x_ln2, xo.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(ao.data(), att, ao.size() * 2, hipMemcpyDeviceToHost);
  };
  std::vector<float> xr2((size_t)B * d);
  run_check(0, xr, ar);
  hipMemcpy(xr2.data(), x_ln2, xr2.size() * 4, hipMemcpyDeviceToHost);
  for (int v : {1, 2, 3, 4, 5}) {
    run_check(v, xt, at_);
    if (v != 1) { xr = xr2; at_ = ar; }   // compare after LN2 (the cross-attention output is only compared for variant 1)
    double ex = 0, ea = 0, mx = 0, ma = 0;
    for (size_t i = 0; i < xr.size(); ++i) { ex = std::max(ex, (double)fabsf(xr[i] - xt[i])); mx = std::max(mx, (double)fabsf(xr[i]));
      ea = std::max(ea, (double)fabsf(b2f(ar[i]) - b2f(at_[i]))); ma = std::max(ma, (double)fabsf(b2f(ar[i]))); }
    printf("check variant %d vs 0: residual rows max|diff| %.3g (max|x| %.3g), cross-attention out max|diff| %.3g (max %.3g)%s\n", v, ex, mx, ea, ma,
           (ex > 0.02 * mx + 1e-3 || ea > 0.02 * ma + 1e-4) ? "   <-- MISMATCH" : "");
  }
  // ---- timing: interleaved rounds in one process
  const char* names[6] = {"shipped 11-launch plan", "q projection inside cross-attention", "self-attn + out-proj G=4 (per-head slabs)",
                          "self-attn + out-proj G=8", "both (variants 1 + 2)", "self-attn as one wave per (row, head), 11 launches"};
  hipGraphExec_t ex[6];
  for (int v = 0; v < 6; ++v) {
    hipGraph_t gr;
    hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    int pend = 0; int64_t ps = 0;
    for (int l = 0; l < L; ++l) run_layer(l, v, pend, ps);
    hipStreamEndCapture(s, &gr); hipGraphInstantiate(&ex[v], gr, nullptr, nullptr, 0); hipGraphDestroy(gr);
  }
  for (int round = 0; round < 3; ++round)
    for (int v = 0; v < 6; ++v) {
      if (only >= 0 && v != only && v != 0) continue;
      double us = timeit(s, [&] { hipGraphLaunch(ex[v], s); }, reps) / L;
      printf("round %d variant %d (%s): %.2f us per layer\n", round, v, names[v], us);
    }
  return 0;
}
