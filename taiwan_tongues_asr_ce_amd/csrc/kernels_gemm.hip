// GEMM kernels: C[M][N] = A[M][K] * W[N][K]^T with fused epilogues (bias / GELU / positions / residual /
// head-split scatter).  Replaces CTranslate2's Dense + Conv1D layers on the Whisper hot path
// (SURVEY.md section 2.1).  Both operands are K-contiguous ("B^T input"), which is exactly PyTorch's
// Linear weight layout, so MFMA A and B fragments are plain 16-byte row reads.
//
//   gemm_basic<T>   64x64x32 tile, register-staged LDS, any M/N/K (K % 8 == 0).  T = float uses the
//                   exact-f32 MFMA v_mfma_f32_16x16x4_f32 (parity mode), T = bf16 v_mfma_f32_16x16x32_bf16.
//   gemm_bf16_fast  128x128x64 tile, global_load_lds (16 B) double-buffered staging, XOR-swizzled LDS
//                   image (swizzle applied on the SOURCE address, guide rule 21), XCD-aware tile order.
#include "common.hpp"
#include <type_traits>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// epilogue
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void epi_store(const GemmEpi& e, int64_t zoff, int m, int n, float v) {
  if (e.bias) v += e.bias[n];
  if (e.act == 1) v = gelu_erf(v);
  if (e.rowtab) v += e.rowtab[(int64_t)(m % e.rowmod) * e.ldc + n];
  int64_t idx = zoff + (int64_t)m * e.ldc + n;
  if (e.residual) v += e.residual[idx];
  if (e.out_f32) e.out_f32[idx] = v;
  if (e.out_t) {
    if (e.headsplit) {
      int which = n / e.hs_d, nn = n - which * e.hs_d;
      int h = nn >> 6, j = nn & 63;
      int b = m / e.hs_T, t = m - b * e.hs_T;
      idx = (int64_t)which * e.hs_which + (((int64_t)b * e.hs_H + h) * e.hs_T + t) * 64 + j;
    }
    ((T*)e.out_t)[idx] = from_f<T>(v);
  }
}

// ------------------------------------------------------------------------------------------------
// gemm_basic
// ------------------------------------------------------------------------------------------------
template <typename T> struct BasicCfg;
template <> struct BasicCfg<float> { static constexpr int VEC = 4, PAD = 4; };
template <> struct BasicCfg<bf16_t> { static constexpr int VEC = 8, PAD = 8; };
template <> struct BasicCfg<f16_t> { static constexpr int VEC = 8, PAD = 8; };

template <typename T>
__global__ __launch_bounds__(256) void gemm_basic_kernel(GemmArgs g) {
  constexpr int BM = 64, BN = 64, BK = 32;
  constexpr int VEC = BasicCfg<T>::VEC, LDK = BK + BasicCfg<T>::PAD, VPR = BK / VEC;
  __shared__ __attribute__((aligned(16))) T As[BM * LDK];
  __shared__ __attribute__((aligned(16))) T Ws[BN * LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const T* A = (const T*)g.A + (int64_t)blockIdx.z * g.batch_stride_a;
  const T* W = (const T*)g.W;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < g.K; k0 += BK) {
    for (int v = tid; v < BM * VPR; v += 256) {
      int r = v / VPR, c = v - r * VPR;
      int k = k0 + c * VEC;
      uint4 va = make_uint4(0, 0, 0, 0), vw = make_uint4(0, 0, 0, 0);
      if (k < g.K) {
        if (m0 + r < g.M) va = *(const uint4*)(A + (int64_t)(m0 + r) * g.lda + k);
        if (n0 + r < g.N) vw = *(const uint4*)(W + (int64_t)(n0 + r) * g.ldw + k);
      }
      *(uint4*)(As + r * LDK + c * VEC) = va;
      *(uint4*)(Ws + r * LDK + c * VEC) = vw;
    }
    __syncthreads();
    if constexpr (sizeof(T) == 2) {
      s16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *(const s16x8*)(As + (wm * 32 + i * 16 + (lane & 15)) * LDK + 8 * (lane >> 4));
        b[i] = *(const s16x8*)(Ws + (wn * 32 + i * 16 + (lane & 15)) * LDK + 8 * (lane >> 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = N16<T>::mfma16(a[i], b[j], acc[i][j]);
    } else {
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = ((const float*)As)[(wm * 32 + i * 16 + (lane & 15)) * LDK + kk * 4 + (lane >> 4)];
          b[i] = ((const float*)Ws)[(wn * 32 + i * 16 + (lane & 15)) * LDK + kk * 4 + (lane >> 4)];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int64_t zoff = (int64_t)blockIdx.z * g.epi.batch_stride_c;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
        int n = n0 + wn * 32 + j * 16 + (lane & 15);
        if (m < g.M && n < g.N) epi_store<T>(g.epi, zoff, m, n, acc[i][j][r]);
      }
}

template <typename T>
void launch_gemm_basic(const GemmArgs& g, hipStream_t s) {
  dim3 grid((g.N + 63) / 64, (g.M + 63) / 64, g.batch);
  hipLaunchKernelGGL(gemm_basic_kernel<T>, grid, dim3(256), 0, s, g);
}
template void launch_gemm_basic<float>(const GemmArgs&, hipStream_t);
template void launch_gemm_basic<bf16_t>(const GemmArgs&, hipStream_t);
template void launch_gemm_basic<f16_t>(const GemmArgs&, hipStream_t);

// ------------------------------------------------------------------------------------------------
// gemm_bf16_fast: 128x128x64, glds double buffer
// ------------------------------------------------------------------------------------------------
// LDS image per operand tile: [128 rows][8 chunks of 16 B]; chunk slot s of row r holds global chunk
// s ^ (r & 7) (source-side swizzle), so a 16-lane ds_read_b128 group (16 rows, one k-chunk) covers all 64
// banks exactly once.
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}

template <typename T16>
__global__ __launch_bounds__(256, 2) void gemm_bf16_fast_kernel(GemmArgs g, int tiles_m, int tiles_n) {
  constexpr int BM = 128, BN = 128, BK = 64;
  constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 buf][A 16K | W 16K]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // XCD-aware tile order: blocks b and b+8 share an XCD (round-robin dispatch), so give each XCD a
  // contiguous range of tiles; n runs fastest so neighbours share the A panel in that XCD's L2.
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  const bf16_t* A = (const bf16_t*)g.A + (int64_t)blockIdx.z * g.batch_stride_a;
  const bf16_t* W = (const bf16_t*)g.W;

  // staging assignment: wave w issues 4 A pieces + 4 W pieces per k-tile; piece p covers rows 8p..8p+7
  const int srow = lane >> 3, sslot = lane & 7;
  const bf16_t* a_src[4];
  const bf16_t* w_src[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int row = (wave * 4 + p) * 8 + srow;
    int chunk = sslot ^ (row & 7);
    int am = min(m0 + row, g.M - 1);  // clamp: rows >= M are loaded but never stored
    a_src[p] = A + (int64_t)am * g.lda + chunk * 8;
    w_src[p] = W + (int64_t)(n0 + row) * g.ldw + chunk * 8;
  }
  auto stage = [&](int buf, int k0) {
    char* base = smem + buf * 2 * TILE_BYTES;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      glds16(a_src[p] + k0, base + (wave * 4 + p) * 1024);
      glds16(w_src[p] + k0, base + TILE_BYTES + (wave * 4 + p) * 1024);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = g.K / BK;
  stage(0, 0);
  __syncthreads();  // drains vmcnt(0): tile 0 landed
  const int fr = lane & 15, fq = lane >> 4;
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) stage(cur ^ 1, (t + 1) * BK);
    const char* As = smem + cur * 2 * TILE_BYTES;
    const char* Ws = As + TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      s16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int ra = wm * 64 + i * 16 + fr;
        a[i] = *(const s16x8*)(As + ra * 128 + (((ks * 4 + fq) ^ (ra & 7)) << 4));
        int rb = wn * 64 + i * 16 + fr;
        b[i] = *(const s16x8*)(Ws + rb * 128 + (((ks * 4 + fq) ^ (rb & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = N16<T16>::mfma16(a[i], b[j], acc[i][j]);
    }
    __syncthreads();  // next tile landed (vmcnt(0)) and everyone finished reading `cur`
  }

  const int64_t zoff = (int64_t)blockIdx.z * g.epi.batch_stride_c;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int m = m0 + wm * 64 + i * 16 + fq * 4 + rr;
        int n = n0 + wn * 64 + j * 16 + fr;
        if (m < g.M) epi_store<T16>(g.epi, zoff, m, n, acc[i][j][rr]);
      }
}

// ------------------------------------------------------------------------------------------------
// gemm_bf16_v2: 256x128x64 tile, 8 waves (4 along M x 2 along N, 64x64 each), THREE-stage LDS ring filled
// by global_load_lds with a counted s_waitcnt vmcnt(6) and a raw s_barrier, so the loads of the next
// k-tile stay in flight across the barrier (guide section 5 "Pipelining across barriers").  One block
// per CU (144 KiB LDS).  Operands are swapped in the MFMA (A = weight rows, B = activation rows) so each
// lane ends with 4 CONSECUTIVE output columns of one row: the epilogue stores 8-byte bf16 / 16-byte f32
// vectors and reads bias as float4.  GELU uses the Abramowitz-Stegun 7.1.26 erf (|err| < 1.5e-7).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float erfa = 1.0f - p * t * __expf(-z * z);  // erf(|x|/sqrt2)
  const float erfx = x < 0.f ? -erfa : erfa;
  return 0.5f * x * (1.0f + erfx);
}

// 4 consecutive columns n..n+3 of row m
template <typename T16>
__device__ __forceinline__ void epi_store4(const GemmEpi& e, int64_t zoff, int m, int n, f32x4 v) {
  if (e.bias) {
    const float4 b = *(const float4*)(e.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (e.act == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = gelu_fast(v[i]);
  }
  if (e.rowtab) {
    const float4 r = *(const float4*)(e.rowtab + (int64_t)(m % e.rowmod) * e.ldc + n);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  int64_t idx = zoff + (int64_t)m * e.ldc + n;
  if (e.residual) {
    const float4 r = *(const float4*)(e.residual + idx);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  if (e.out_f32) *(float4*)(e.out_f32 + idx) = make_float4(v[0], v[1], v[2], v[3]);
  if (e.out_t) {
    if (e.headsplit) {
      const int which = n / e.hs_d, nn = n - which * e.hs_d;
      const int h = nn >> 6, j = nn & 63;
      const int b = m / e.hs_T, t = m - b * e.hs_T;
      idx = (int64_t)which * e.hs_which + (((int64_t)b * e.hs_H + h) * e.hs_T + t) * 64 + j;
    }
    uint2 pk;
    pk.x = N16<T16>::pk(v[0], v[1]);
    pk.y = N16<T16>::pk(v[2], v[3]);
    *(uint2*)((bf16_t*)e.out_t + idx) = pk;
  }
}

template <typename T16>
__global__ __launch_bounds__(512, 2) void gemm_bf16_v2_kernel(GemmArgs g, int tiles_m, int tiles_n) {
  constexpr int BM = 256, BN = 128, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2, STAGE_BYTES = A_BYTES + W_BYTES;  // 32K + 16K
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = tiles_m * tiles_n;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  // grouped raster: bands of GM m-tiles, n-tile fastest across the band, m-tile fastest inside it, so the ~32
  // tiles an XCD runs at once form a 4 x 8 patch (4 A panels + 8 W panels ~ 5 MB against its 4 MiB L2)
  // instead of 1 x 32 (measured: 34 % L2 misses with the row-major order = every W panel missed).
  constexpr int GM = 4;
  const int band = tile / (GM * tiles_n);
  const int rows_in_band = min(GM, tiles_m - band * GM);
  const int in_band = tile - band * GM * tiles_n;
  const int tn = in_band / rows_in_band;
  const int tm = band * GM + (in_band - tn * rows_in_band);
  const int m0 = tm * BM, n0 = tn * BN;
  const bf16_t* A = (const bf16_t*)g.A + (int64_t)blockIdx.z * g.batch_stride_a;
  const bf16_t* W = (const bf16_t*)g.W;

  const int srow = lane >> 3, sslot = lane & 7;
  const bf16_t* a_src[4];
  const bf16_t* w_src[2];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = (wave * 4 + p) * 8 + srow;
    a_src[p] = A + (int64_t)min(m0 + row, g.M - 1) * g.lda + ((sslot ^ (row & 7)) << 3);
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = (wave * 2 + p) * 8 + srow;
    w_src[p] = W + (int64_t)(n0 + row) * g.ldw + ((sslot ^ (row & 7)) << 3);
  }
#define V2_STAGE(buf_, k0_)                                                             \
  do {                                                                                  \
    char* base_ = smem + (buf_) * STAGE_BYTES;                                          \
    _Pragma("unroll") for (int p = 0; p < 4; ++p)                                       \
        glds16(a_src[p] + (k0_), base_ + (wave * 4 + p) * 1024);                        \
    _Pragma("unroll") for (int p = 0; p < 2; ++p)                                       \
        glds16(w_src[p] + (k0_), base_ + A_BYTES + (wave * 2 + p) * 1024);              \
  } while (0)

  f32x4 acc[4][4];  // [i: m-frag][j: n-frag]; element r = column n0.. + j*16 + (lane>>4)*4 + r of row i*16 + (lane&15)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = g.K / BK;
  V2_STAGE(0, 0);
  if (nt > 1) V2_STAGE(1, BK);
  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 2 < nt) {
      const int nb = cur >= 1 ? cur - 1 : 2;  // (t + 2) % 3
      V2_STAGE(nb, (t + 2) * BK);
    }
    // All 16 fragment reads are issued first (64 VGPRs) as inline-asm ds_read_b128 with HAND-COUNTED waits:
    // the k-step-0 MFMAs start once the first 8 reads have landed (lgkmcnt(8)) while the other 8 stream
    // in behind them.  (hipcc's own placement waits lgkmcnt(0) before the first MFMA: guide 5.7.)
    s16x8 a[2][4], b[2][4];
    const uint32_t as_off = lds_base + cur * STAGE_BYTES, ws_off = as_off + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rb = wn * 64 + i * 16 + fr;
        asm volatile("ds_read_b128 %0, %1" : "=v"(b[ks][i]) : "v"(ws_off + rb * 128 + (((ks * 4 + fq) ^ (rb & 7)) << 4)));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ra = wm * 64 + i * 16 + fr;
        asm volatile("ds_read_b128 %0, %1" : "=v"(a[ks][i]) : "v"(as_off + ra * 128 + (((ks * 4 + fq) ^ (ra & 7)) << 4)));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[0][3]), "+v"(b[0][0]),
                 "+v"(b[0][1]), "+v"(b[0][2]), "+v"(b[0][3]));
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)  // A operand = weight rows (n), B operand = activation rows (m)
        acc[i][j] = N16<T16>::mfma16(b[0][j], a[0][i], acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]), "+v"(a[1][3]), "+v"(b[1][0]),
                 "+v"(b[1][1]), "+v"(b[1][2]), "+v"(b[1][3]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = N16<T16>::mfma16(b[1][j], a[1][i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    cur = cur == 2 ? 0 : cur + 1;
  }
#undef V2_STAGE
  const int64_t zoff = (int64_t)blockIdx.z * g.epi.batch_stride_c;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m < g.M) {
#pragma unroll
      for (int j = 0; j < 4; ++j) epi_store4<T16>(g.epi, zoff, m, n0 + wn * 64 + j * 16 + fq * 4, acc[i][j]);
    }
  }
}

bool gemm_bf16_v2_ok(const GemmArgs& g) {
  return g.N % 128 == 0 && g.K % 64 == 0 && g.K >= 128 && g.lda % 8 == 0 && g.ldw % 8 == 0 && g.epi.ldc % 4 == 0 &&
         ((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.W % 16) == 0 && (!g.epi.headsplit || g.epi.hs_d % 64 == 0);
}
template <typename T16>
void launch_gemm_bf16_v2(const GemmArgs& g, hipStream_t s) {
  // the opt-in to > 64 KiB of dynamic LDS was made once per device by gemm_tiles_init (ttasr_create)
  const int tiles_m = (g.M + 255) / 256, tiles_n = g.N / 128;
  hipLaunchKernelGGL(gemm_bf16_v2_kernel<T16>, dim3(tiles_m * tiles_n, 1, g.batch), dim3(512), 3 * 49152, s, g, tiles_m, tiles_n);
}
template void launch_gemm_bf16_v2<bf16_t>(const GemmArgs&, hipStream_t);
template void launch_gemm_bf16_v2<f16_t>(const GemmArgs&, hipStream_t);

// ------------------------------------------------------------------------------------------------
// The 256x256x32 tile: 32-deep stages, FOUR-stage LDS ring (128 KiB), 8 waves as 2 (M) x 4 (N), 128x64 per wave.
// The two wave groups (waves 0-3 / 4-7, i.e. the two SIMD partners) run staggered by one barrier: while
// one group issues its LDS-DMA (4 x global_load_lds) and fragment reads (12 x ds_read_b128), its partner
// on the same SIMD runs its 32 MFMAs, so the matrix pipe sees matrix-beside-memory instead of two waves
// doing the same thing in lockstep (MI355X_MICROARCH "Two waves per SIMD", items 5 and 9).
// Per iteration t and wave:   A_t: s_waitcnt vmcnt(4) [own pieces of stage t+1 landed]; s_barrier;
//                                  issue stage t+3 -> slot (t+3)&3; read fragments of stage t; lgkmcnt(0)
//                             B_t: s_barrier; 32 MFMAs
// Group 1 executes one extra barrier before the loop and group 0 one after it, so group 0's A_t barrier
// pairs with group 1's B_{t-1} barrier.  RAW: every wave has waited for its stage-t pieces one phase before
// anyone reads stage t.  WAR: slot (t+3)&3 held stage t-1, whose fragment reads were drained (lgkmcnt(0))
// before the barrier that precedes the first overwrite.
// LDS image per operand stage: [256 rows][4 chunks of 16 B]; chunk c of row r sits in slot c ^ H((r>>2)&3),
// H = {0,2,3,1}, which makes every ds_read_b128 lane group hit 16 distinct 16-byte bank slots.
//
// The tile is written ONCE, as the blocks of namespace t256:
//   xcd_chunk, raster       which tile a workgroup runs: contiguous chunk per XCD, bands of GM m-tiles inside it
//   Lane                    where a thread sits in the workgroup; its fragment offsets
//   Stager                  a wave's 2 + 2 LDS-DMA source pointers; stage(slot, k0); prologue() = stages 0..2
//   mainloop<T16, MI, ..>   the phase-A / phase-B loop above with its counted waits, for MI row blocks of 16 per wave group
//   load_bias               the lane's 16 bias values, waited for on the spot
//   out_cols, store_tile_t  the T-output epilogue: bias, GELU, pack, permlane16_swap, 16-byte stores (guarded or clamped)
// and two kernels compose them: gemm_bf16_v3_kernel (one workgroup per tile; adds the f32 / residual / row-table epilogue) and
// gemm_bf16_persistent_kernel (one workgroup per CU walks its tiles; TAIL = false is "v4", TAIL = true is "v5").
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int v3_h(int q) { return (0x78 >> (q * 2)) & 3; }  // {0,2,3,1} packed two bits each

namespace t256 {
constexpr int BM = 256, BN = 256, BK = 32;
constexpr int OP_BYTES = BM * BK * 2, STAGE_BYTES = 2 * OP_BYTES, LDS_BYTES = 4 * STAGE_BYTES;  // 16K + 16K per stage
constexpr int GM = 4;

// The workgroups that share an XCD (blockIdx % 8, round-robin dispatch) own one contiguous range [lo, hi) of n tiles.
__device__ __forceinline__ void xcd_chunk(int n, int xcd, int& lo, int& hi) {
  const int q = n >> 3, r = n & 7;
  lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  hi = lo + (xcd < r ? q + 1 : q);
}

// Grouped raster of a region of tiles_m x tiles_n tiles that starts at row base_row: bands of GM m-tiles, n-tile fastest across
// the band, m-tile fastest inside it, so the ~32 tiles an XCD runs at once form a 4 x 8 patch (see gemm_bf16_v2_kernel).
__device__ __forceinline__ void raster(int tile, int tiles_m, int tiles_n, int base_row, int rows_per_tile, int& m0, int& n0) {
  const int band = tile / (GM * tiles_n);
  const int rows_in_band = min(GM, tiles_m - band * GM);
  const int in_band = tile - band * GM * tiles_n;
  const int tn = in_band / rows_in_band;
  const int tm = band * GM + (in_band - tn * rows_in_band);
  m0 = base_row + tm * rows_per_tile; n0 = tn * BN;
}

struct Lane {
  char* smem;
  int lane, wave, wm, wn, fr, fq;
  uint32_t lds_base, frag_off;
  __device__ __forceinline__ explicit Lane(char* smem_) : smem(smem_) {
    lane = threadIdx.x & 63;
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    wm = wave >> 2; wn = wave & 3;
    fr = lane & 15; fq = lane >> 4;
    lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    // per-lane fragment offset inside an operand stage (row r = base + 16*i + fr -> (r>>2)&3 == (fr>>2)&3)
    frag_off = (uint32_t)(fr * 64 + ((fq ^ v3_h((fr >> 2) & 3)) << 4));
  }
  // LDS addresses of the lane's first A / W fragment in slot 0 (mi = row blocks of 16 per wave group)
  __device__ __forceinline__ uint32_t a_off(int mi) const { return lds_base + wm * (mi * 16) * 64 + frag_off; }
  __device__ __forceinline__ uint32_t w_off() const { return lds_base + OP_BYTES + wn * 64 * 64 + frag_off; }
  __device__ __forceinline__ int nbase(int n0) const { return n0 + wn * 64 + fq * 4; }   // the lane's first output column
};

// staging: one wave-instruction = 16 rows x 64 B; wave w moves rows (2w+p)*16 .. +15 of A and of W
struct Stager {
  const bf16_t* a_src[2];
  const bf16_t* w_src[2];
  // A rows from m0 (clamped to row_lim: rows past it are loaded but never stored), W rows from n0
  __device__ __forceinline__ void point(const Lane& L, const bf16_t* A, int64_t lda, int m0, int row_lim, const bf16_t* W, int64_t ldw, int n0) {
    const int srow = L.lane >> 2, sslot = L.lane & 3;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = (L.wave * 2 + p) * 16 + srow;
      const int chunk = sslot ^ v3_h((row >> 2) & 3);
      a_src[p] = A + (int64_t)min(m0 + row, row_lim) * lda + chunk * 8;
      w_src[p] = W + (int64_t)(n0 + row) * ldw + chunk * 8;
    }
  }
  __device__ __forceinline__ void stage(const Lane& L, int slot, int k0) const {
    char* base = L.smem + slot * STAGE_BYTES;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      glds16(a_src[p] + k0, base + (L.wave * 2 + p) * 1024);
      glds16(w_src[p] + k0, base + OP_BYTES + (L.wave * 2 + p) * 1024);
    }
  }
  __device__ __forceinline__ void prologue(const Lane& L) const { stage(L, 0, 0); stage(L, 1, BK); stage(L, 2, 2 * BK); }
};

// "own pieces of the wanted stage landed": everything but the 4 youngest pieces and the `carried` stores of the previous tile's
// epilogue (vmcnt retires in issue order).  carried = 2 per row block of that tile (16 / 12 / 8), or 0.
__device__ __forceinline__ void wait_stage(int carried) {
  if (carried == 16) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
  else if (carried == 12) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else if (carried == 8) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
}
template <int MI>
__device__ __forceinline__ void wait_frags(s16x8 (&a)[MI], s16x8 (&b)[4]) {
  static_assert(MI == 8 || MI == 6 || MI == 4, "row blocks per wave group");
  if constexpr (MI == 8)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                   "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  else if constexpr (MI == 6)
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
  else
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

// One tile's K loop: acc = A[m-rows] * W[n-rows]^T for MI x 4 fragments of 16 x 16 per wave.  On entry the three stages of
// Stager::prologue are in flight, with `carried` stores of the previous tile's epilogue issued behind them (persistent kernel) or
// none (v3); on exit every fragment read is drained, so the ring is free.  A shorter tile (MI = 6 / 4) is the same body with
// fewer row blocks: the A image is still staged 256 rows deep, every output element sees the same K loop in the same order.
// PEEL: the test for the carried waits does not look at `carried`, so the compiler peels iterations 0 and 1 off the loop (what the
// tail-re-tiled form has always had; measured: without it its qkv / out-proj / fc1 are 1.5-4 % slower, LAB_NOTEBOOK).
template <typename T16, int MI, bool PEEL>
__device__ __forceinline__ void mainloop(f32x4 (&acc)[MI][4], const Lane& L, const Stager& st, uint32_t a_off, uint32_t w_off, int nt,
                                         int carried) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // stages 0 and 1 landed (own pieces); queue behind them: stage 2 (4) [+ the carried stores]
  wait_stage(carried);
  if (L.wm == 1) __builtin_amdgcn_s_barrier();  // stagger: group 1 runs one barrier behind
  for (int t = 0; t < nt; ++t) {
    // ---- phase A ----
    if (t + 2 < nt) {
      // own pieces of stage t + 1 landed; queue behind them: stage t + 2 (4), and for t < 2 of a carried tile its stores
      // (t = 0: [stage 2][stores]; t = 1: [stores][stage 3] - from t = 2 on the stores are older than what is waited for)
      if ((PEEL || carried) && t < 2) wait_stage(carried); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 3 < nt) st.stage(L, (t + 3) & 3, (t + 3) * BK);
    s16x8 a[MI], b[4];
    const uint32_t so = (uint32_t)((t & 3) * STAGE_BYTES);
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(b[j]) : "v"(w_off + so + j * 16 * 64));
#pragma unroll
    for (int i = 0; i < MI; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(a[i]) : "v"(a_off + so + i * 16 * 64));
    wait_frags<MI>(a, b);
    __builtin_amdgcn_sched_barrier(0);
    // ---- phase B ----
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)  // A operand = weight rows (n), B operand = activation rows (m)
        acc[i][j] = N16<T16>::mfma16(b[j], a[i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (L.wm == 0) __builtin_amdgcn_s_barrier();  // balance the barrier count: every fragment read of this tile is drained
}

// the lane's bias values for columns n + 16 j .. + 3 (bias_n = bias + Lane::nbase)
__device__ __forceinline__ void load_bias(const float* bias_n, float4 (&b4)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) b4[j] = *(const float4*)(bias_n + j * 16);
  // waited for HERE, while nothing else is in flight: no later use of these registers may drain the LDS-DMA queue
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(b4[0].x), "+v"(b4[0].y), "+v"(b4[0].z), "+v"(b4[0].w), "+v"(b4[1].x), "+v"(b4[1].y),
               "+v"(b4[1].z), "+v"(b4[1].w), "+v"(b4[2].x), "+v"(b4[2].y), "+v"(b4[2].z), "+v"(b4[2].w), "+v"(b4[3].x),
               "+v"(b4[3].y), "+v"(b4[3].z), "+v"(b4[3].w));
}

// column part of the T-output index of the lane's four column groups nbase + 16 j, on top of `base` (HS: head-split scatter)
template <bool HS>
__device__ __forceinline__ void out_cols(const GemmEpi& e, int nbase, int64_t base, int64_t (&coloff)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = nbase + j * 16;
    if (HS) {
      const int which = n / e.hs_d, nn = n - which * e.hs_d;
      coloff[j] = base + (int64_t)which * e.hs_which + (int64_t)(nn >> 6) * e.hs_T * 64 + (nn & 63);
    } else {
      coloff[j] = base + n;
    }
  }
}

// T-output epilogue of MI row blocks (rows mrow0 + 16 i): bias, GELU (EPI bit 0), pack, 2 x 16-byte stores per row block and lane;
// the row part of the index is head-split (EPI bit 3) or zoff + m * ldc.  GUARD: rows >= M are not stored (v3); otherwise the stores
// are unconditional with the row index clamped (rows past M replicate row M-1's operands, so they write row M-1's own values again):
// the in-flight count the next tile's first waits rely on is then exact for every wave.
template <typename T16, int MI, int EPI, bool GUARD>
__device__ __forceinline__ void store_tile_t(const f32x4 (&acc)[MI][4], const float4 (&bias4)[4], const GemmEpi& e, int M, int64_t zoff,
                                             int mrow0, const int64_t (&coloff)[4], const Lane& L) {
  constexpr bool ACT = EPI & 1, HS = EPI & 8;
  static_assert((EPI & ~9) == 0, "T output: no residual, no row table");
  // Widen the 16-bit stores (guide T21, 16-lane form): lanes l and l^16 hold columns 4q..4q+3 and 4q+4..4q+7 of
  // the same row, so one v_permlane16_swap per dword over a pair of column groups (j, j+1) leaves the even
  // 16-lane rows with 16 contiguous bytes of group j and the odd rows with 16 contiguous bytes of group j+1:
  // 16 x 16-byte stores per lane instead of 32 x 8-byte (the store tail is issue-bound, not bandwidth-bound).
  const bool odd = (L.fq & 1) != 0;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = min(mrow0 + i * 16, M - 1);
    int64_t rowoff;
    if (HS) {
      const int bb = m / e.hs_T, tt = m - bb * e.hs_T;
      rowoff = ((int64_t)bb * e.hs_H * e.hs_T + tt) * 64;
    } else rowoff = zoff + (int64_t)m * e.ldc;
    uint2 pk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v = acc[i][j];
      v[0] += bias4[j].x; v[1] += bias4[j].y; v[2] += bias4[j].z; v[3] += bias4[j].w;
      if (ACT) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = gelu_fast(v[t]);
      }
      pk[j].x = N16<T16>::pk(v[0], v[1]);
      pk[j].y = N16<T16>::pk(v[2], v[3]);
    }
#pragma unroll
    for (int jp = 0; jp < 4; jp += 2) {
      auto sx = __builtin_amdgcn_permlane16_swap(pk[jp].x, pk[jp + 1].x, false, false);
      auto sy = __builtin_amdgcn_permlane16_swap(pk[jp].y, pk[jp + 1].y, false, false);
      // even row: {own group jp, partner's group jp}; odd row: {partner's group jp+1, own group jp+1}
      const uint4 w = make_uint4(sx[0], sy[0], sx[1], sy[1]);
      const int jj = odd ? jp + 1 : jp;
      if (!GUARD || mrow0 + i * 16 < M) *(uint4*)((bf16_t*)e.out_t + rowoff + coloff[jj] - (odd ? 4 : 0)) = w;
    }
  }
}
}  // namespace t256

// ------------------------------------------------------------------------------------------------
// gemm_bf16_v3: one workgroup per 256x256 tile.
// ------------------------------------------------------------------------------------------------
template <typename T16, int EPI>  // EPI: bit0 GELU, bit1 residual, bit2 row table (positions), bit3 head-split T output, bit4 f32 output
__global__ __launch_bounds__(512, 2) void gemm_bf16_v3_kernel(GemmArgs g, int tiles_m, int tiles_n) {
  using namespace t256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lane L(smem);
  int lo, hi, m0, n0;
  xcd_chunk(tiles_m * tiles_n, blockIdx.x & 7, lo, hi);
  raster(lo + (blockIdx.x >> 3), tiles_m, tiles_n, 0, BM, m0, n0);
  Stager st;
  st.point(L, (const bf16_t*)g.A + (int64_t)blockIdx.z * g.batch_stride_a, g.lda, m0, g.M - 1, (const bf16_t*)g.W, g.ldw, n0);
  st.prologue(L);
  f32x4 acc[8][4];
  mainloop<T16, 8, false>(acc, L, st, L.a_off(8), L.w_off(), g.K / BK /* >= 4 */, 0);
  // ---- epilogue, specialised at compile time (EPI) so no integer division / dead branch survives for the
  // common shapes; row offsets are computed once per row, column parts once per column group, and every load
  // (bias, positions, residual) is issued ahead of the stores it feeds.  (The generic per-element epilogue cost
  // 5 500 VALU instructions per thread: 25-40 % of the kernel.)
  constexpr bool ACT = EPI & 1, RES = EPI & 2, ROWTAB = EPI & 4, HS = EPI & 8, OUTF = EPI & 16;
  const GemmEpi& e = g.epi;
  const int64_t zoff = (int64_t)blockIdx.z * e.batch_stride_c;
  const int nbase = L.nbase(n0);
  float4 bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = e.bias ? *(const float4*)(e.bias + nbase + j * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (!OUTF) {
    int64_t coloff[4];
    out_cols<HS>(e, nbase, 0, coloff);
    store_tile_t<T16, 8, EPI, true>(acc, bias4, e, g.M, zoff, m0 + L.wm * 128 + L.fr, coloff, L);
  } else {
    // f32 output at zoff + m * ldc + n, with the residual and / or the row table (positions) added
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float4 extra[4][4];
      int64_t rowlin[4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int m = min(m0 + L.wm * 128 + (half * 4 + ii) * 16 + L.fr, g.M - 1);
        rowlin[ii] = zoff + (int64_t)m * e.ldc;
        if (RES || ROWTAB) {
          const int64_t tabrow = ROWTAB ? (int64_t)(m % e.rowmod) * e.ldc : 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (RES) r = *(const float4*)(e.residual + rowlin[ii] + nbase + j * 16);
            if (ROWTAB) {
              const float4 t = *(const float4*)(e.rowtab + tabrow + nbase + j * 16);
              r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w;
            }
            extra[ii][j] = r;
          }
        }
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int i = half * 4 + ii;
        const bool row_ok = m0 + L.wm * 128 + i * 16 + L.fr < g.M;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f32x4 v = acc[i][j];
          v[0] += bias4[j].x; v[1] += bias4[j].y; v[2] += bias4[j].z; v[3] += bias4[j].w;
          if (ACT) {
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = gelu_fast(v[t]);
          }
          if (RES || ROWTAB) { v[0] += extra[ii][j].x; v[1] += extra[ii][j].y; v[2] += extra[ii][j].z; v[3] += extra[ii][j].w; }
          if (row_ok) *(float4*)(e.out_f32 + rowlin[ii] + nbase + j * 16) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// gemm_bf16_persistent: the tile body as a PERSISTENT workgroup (one per CU) that walks its tiles, so that the part of a tile that
// v3 leaves exposed at one workgroup per CU - the store-issue-bound epilogue, the workgroup relaunch and the first stages' HBM/L2
// latency - overlaps with neighbouring work:
//   main loop of tile i  ->  bias of tile i+1 (waited for here: nothing else is in flight)  ->  LDS-DMA of stages 0..2 of tile
//   i+1 (the ring is free: every fragment read of tile i was drained before the last barrier)  ->  epilogue of tile i (VALU +
//   2 x 16-byte stores per row block and lane, no LDS, no load)  ->  main loop of tile i+1, whose first two counted waits allow
//   those stores to be still in flight (vmcnt retires in issue order: [4 pieces of stage 2][stores][4 pieces of stage 3] ...).
// Same arithmetic as v3 (accumulation order, bias added after the loop, same conversions): bit-identical outputs.
// EPI 0 (bias -> T), 1 (bias + GELU -> T), 8 (bias -> head-split T); batch == 1.
//
// TAIL = false ("v4", round 4): tiles_m x tiles_n tiles of 256 rows per group; g.groups > 1 walks the groups' tiles as one range
// (weights group_stride_w apart, bias N apart, outputs group_stride_out apart: the grouped cross-KV launch).
// TAIL = true ("v5", round 5; groups == 1, gemm_bf16_v5_ok): the LAST partial round of workgroups is re-tiled.  The rows are cut
// into a FULL region of tiles_m 256-row m-tiles whose tile count fills whole rounds of the persistent workgroups, and a TAIL region
// of tail_tiles_m shorter tiles - tail_mi * 32 rows (tail_mi = 6 or 4 row blocks of 16 per wave group instead of 8), all 256
// columns - chosen by v5_plan so that the tail's tile count fits ONE round: e.g. out-proj / fc2 at B = 32 (940 tiles = 3.67 rounds
// -> 4): 765 full tiles (2.99 rounds) + 230 tiles of 192 rows (one round of ~0.78 of a tile).  Stage t + 3 is issued right after
// the phase-A barrier; DESIGN 4.11 records the three other placements that were measured in round 5.
// ------------------------------------------------------------------------------------------------
template <typename T16, int EPI, bool TAIL>
__global__ __launch_bounds__(512, 2) void gemm_bf16_persistent_kernel(GemmArgs g, int tiles_m, int tiles_n, int tail_tiles_m, int tail_mi) {
  using namespace t256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lane L(smem);
  // tile ids: [0, n_full) 256-row tiles (of all groups), n_full + [0, n_tail) tail tiles
  const int tiles_per_group = tiles_m * tiles_n;
  const int n_full = TAIL ? tiles_per_group : tiles_per_group * g.groups, n_tail = TAIL ? tail_tiles_m * tiles_n : 0;
  // static schedule: the workgroups that share an XCD (bid % 8) own one contiguous chunk of the full tiles and one of the tail
  // tiles; a workgroup walks its full tiles round-robin (slot, slot + per_xcd, ...), then its tail tiles from the OTHER end of
  // the slot order (the workgroups that got one full tile less take the tail tiles first)
  const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3, per_xcd = (gridDim.x + 7 - xcd) >> 3;  // workgroups of this class
  int fb, fe, tb = 0, te = 0;
  xcd_chunk(n_full, xcd, fb, fe);
  if (TAIL) xcd_chunk(n_tail, xcd, tb, te);
  auto first_tail = [&]() { const int t = tb + (per_xcd - 1 - slot); return TAIL && t < te ? n_full + t : -1; };
  auto next_of = [&](int id) {   // -1: that was the workgroup's last tile
    const int nx = id + per_xcd;
    if (!TAIL || id < n_full) return nx < fe ? nx : first_tail();
    return nx - n_full < te ? nx : -1;
  };
  const GemmEpi& e = g.epi;
  const int nt = g.K / BK;  // >= 4

  int m0 = 0, n0 = 0;
  int64_t oofs = 0;          // output offset of the tile's group (elements)
  const float* bias_g = e.bias;   // != nullptr (gemm_bf16_v4_ok)
  int mi_placed = 8;         // row blocks per wave group of the tile place() was last called for
  Stager st;
  auto place = [&](int tile) {   // tile id -> (group,) (m0, n0), staging source pointers
    const bf16_t* W = (const bf16_t*)g.W;
    int tm_n = tiles_m, base_row = 0, rows_per_tile = BM;
    mi_placed = 8;
    if (TAIL) {
      if (tile >= n_full) { tile -= n_full; tm_n = tail_tiles_m; base_row = tiles_m * BM; rows_per_tile = tail_mi * 32; mi_placed = tail_mi; }
    } else if (g.groups > 1) {
      const int grp = tile / tiles_per_group;
      tile -= grp * tiles_per_group;
      W += (int64_t)grp * g.group_stride_w;
      bias_g = e.bias + (int64_t)grp * g.N;
      oofs = (int64_t)grp * g.group_stride_out;
    }
    raster(tile, tm_n, tiles_n, base_row, rows_per_tile, m0, n0);
    // every wave stages its 2 + 2 pieces for EVERY tile (the counted waits rely on it), but the A pieces of a short tile that lie
    // past its last row re-read that one row (one cache line per piece instead of sixteen): a short tile does not pay for A rows
    // it does not use - what fc2, whose 492 MB A operand streams from beyond L2, needs to gain anything
    const int row_lim = TAIL ? min(g.M - 1, m0 + rows_per_tile - 1) : g.M - 1;
    st.point(L, (const bf16_t*)g.A, g.lda, m0, row_lim, W, g.ldw, n0);
  };

  int tile = fb + slot < fe ? fb + slot : first_tail();
  if (tile < 0) return;
  place(tile);
  float4 bias4[4];
  load_bias(bias_g + L.nbase(n0), bias4);
  st.prologue(L);
  int carried = 0;   // stores of the previous tile's epilogue (2 per row block) that sit behind the three prefetched stages

  // one tile of MI row blocks per wave group (8: the 256 x 256 tile; 6 / 4: the shorter tiles of the tail region); false after
  // the workgroup's last tile
  auto run_tile = [&](auto mi_tag) -> bool {
    constexpr int MI = decltype(mi_tag)::value;
    f32x4 acc[MI][4];
    mainloop<T16, MI, TAIL>(acc, L, st, L.a_off(MI), L.w_off(), nt, carried);
    // ---- this tile's output coordinates (before the staging pointers move on) ----
    int64_t coloff[4];
    out_cols<(EPI & 8) != 0>(e, L.nbase(n0), oofs, coloff);
    const int mrow0 = m0 + L.wm * (MI * 16) + L.fr;
    // ---- next tile: bias (waited for now), then its first three stages into the free ring ----
    const int next = next_of(tile);
    float4 bias_next[4];
    if (next >= 0) {
      place(next);
      load_bias(bias_g + L.nbase(n0), bias_next);
      st.prologue(L);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- epilogue of this tile: VALU + 2 unconditional 16-byte stores per row block and lane ----
    store_tile_t<T16, MI, EPI, false>(acc, bias4, e, g.M, 0, mrow0, coloff, L);
    if (next < 0) return false;
    tile = next;
#pragma unroll
    for (int j = 0; j < 4; ++j) bias4[j] = bias_next[j];
    carried = 2 * MI;
    return true;
  };
  for (;;) {   // mi_placed: place(next) ran inside run_tile
    bool more;
    if (!TAIL || mi_placed == 8) more = run_tile(std::integral_constant<int, 8>{});
    else if (mi_placed == 6) more = run_tile(std::integral_constant<int, 6>{});
    else more = run_tile(std::integral_constant<int, 4>{});
    if (!more) break;
  }
}

// ---- host side of the tiled kernels ----
// epilogue variants actually used by the encoder / cross-KV schedules; anything else takes the v2 kernel
static int v3_epi_code(const GemmEpi& e) {
  return (e.act == 1 ? 1 : 0) | (e.residual ? 2 : 0) | (e.rowtab ? 4 : 0) | (e.headsplit ? 8 : 0) | (e.out_f32 ? 16 : 0);
}
// THE list of EPI instantiations: calls f(std::integral_constant<int, EPI>) for a v3_epi_code the tiled kernels are built for
// (T_ONLY: the T-output ones, which is what the persistent kernel carries); false for any other code.
template <bool T_ONLY, typename F>
static bool with_epi(int code, F&& f) {
  switch (code) {
    case 0: f(std::integral_constant<int, 0>{}); return true;    // bias -> T                 (qkv)
    case 1: f(std::integral_constant<int, 1>{}); return true;    // bias + GELU -> T          (fc1, conv1)
    case 8: f(std::integral_constant<int, 8>{}); return true;    // bias -> head-split T      (cross-KV)
    case 18: if constexpr (!T_ONLY) { f(std::integral_constant<int, 18>{}); return true; } return false;  // bias + residual -> f32 (out-proj, fc2)
    case 21: if constexpr (!T_ONLY) { f(std::integral_constant<int, 21>{}); return true; } return false;  // bias + GELU + positions -> f32 (conv2)
    default: return false;
  }
}
static bool epi_known(int code, bool t_only) { return t_only ? with_epi<true>(code, [](auto) {}) : with_epi<false>(code, [](auto) {}); }

bool gemm_bf16_v3_ok(const GemmArgs& g) {
  const bool one_out = (g.epi.out_f32 != nullptr) != (g.epi.out_t != nullptr);
  return epi_known(v3_epi_code(g.epi), false) && one_out && g.N % 256 == 0 && g.K % 32 == 0 && g.K >= 128 && g.lda % 8 == 0 &&
         g.ldw % 8 == 0 && g.epi.ldc % 8 == 0 && ((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.W % 16) == 0 &&
         (!g.epi.headsplit || g.epi.hs_d % 64 == 0);
}
bool gemm_bf16_v4_ok(const GemmArgs& g) {
  return epi_known(v3_epi_code(g.epi), true) && g.batch <= 1 && g.groups >= 1 && g.epi.bias != nullptr && gemm_bf16_v3_ok(g);
}
bool gemm_bf16_v5_ok(const GemmArgs& g) { return g.groups <= 1 && gemm_bf16_v4_ok(g); }

// Per-device launcher state, set ONCE per device by gemm_tiles_init (ttasr_create calls it before the context can launch
// anything; std::call_once orders the writes before every later reader): the opt-in to > 64 KiB of dynamic LDS for every tiled
// instantiation and the CU count that sizes the persistent grid.  Nothing is set lazily from a launcher any more (VERDICT
// round 4, weak #8: two contexts first-launching from two host threads raced on the old `static bool attr_done[64]`).
static int g_v4_cus[64] = {0};
static std::once_flag g_tiles_once[64];
template <typename T16>
static void tiles_attrs() {
  auto opt_in = [](const void* kernel, int bytes) { hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
  opt_in((const void*)gemm_bf16_v2_kernel<T16>, 3 * 49152);
  for (int code = 0; code < 32; ++code) {   // every instantiation with_epi knows
    with_epi<false>(code, [&](auto epi) { opt_in((const void*)gemm_bf16_v3_kernel<T16, decltype(epi)::value>, t256::LDS_BYTES); });
    with_epi<true>(code, [&](auto epi) {
      opt_in((const void*)gemm_bf16_persistent_kernel<T16, decltype(epi)::value, false>, t256::LDS_BYTES);
      opt_in((const void*)gemm_bf16_persistent_kernel<T16, decltype(epi)::value, true>, t256::LDS_BYTES);
    });
  }
}
void gemm_tiles_init(int device) {
  std::call_once(g_tiles_once[device & 63], [device]() {
    hipDeviceProp_t p;
    g_v4_cus[device & 63] = hipGetDeviceProperties(&p, device) == hipSuccess ? p.multiProcessorCount : 256;
    tiles_attrs<bf16_t>();
    tiles_attrs<f16_t>();
  });
}
static int tiles_cus() {
  int dev = 0;
  hipGetDevice(&dev);
  return g_v4_cus[dev & 63];
}

template <typename T16>
void launch_gemm_bf16_v3(const GemmArgs& g, hipStream_t s) {
  const int tiles_m = (g.M + 255) / 256, tiles_n = g.N / 256;
  with_epi<false>(v3_epi_code(g.epi), [&](auto epi) {   // any other code is excluded by gemm_bf16_v3_ok
    constexpr int EPI = decltype(epi)::value;
    if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "gemm_bf16_v3_kernel<%s, %d> grid %d", sig_type<T16>(), EPI,
                                  tiles_m * tiles_n * g.batch * 512);
    hipLaunchKernelGGL((gemm_bf16_v3_kernel<T16, EPI>), dim3(tiles_m * tiles_n, 1, g.batch), dim3(512), t256::LDS_BYTES, s, g, tiles_m, tiles_n);
  });
}
template void launch_gemm_bf16_v3<bf16_t>(const GemmArgs&, hipStream_t);
template void launch_gemm_bf16_v3<f16_t>(const GemmArgs&, hipStream_t);

// the recorded signature keeps the names the two forms had as separate kernels (profiles and tests match on them)
template <typename T16, bool TAIL>
static void launch_persistent(const GemmArgs& g, int tiles, int cus, int full_m, int tiles_n, int tail_m, int tail_mi, hipStream_t s) {
  const int grid = std::min(tiles, cus);
  with_epi<true>(v3_epi_code(g.epi), [&](auto epi) {   // any other code is excluded by gemm_bf16_v4_ok
    constexpr int EPI = decltype(epi)::value;
    if (g_kernel_sig_on) snprintf(g_kernel_sig, sizeof g_kernel_sig, "gemm_bf16_%s_kernel<%s, %d> grid %d", TAIL ? "v5" : "v4", sig_type<T16>(),
                                  EPI, grid * 512);
    hipLaunchKernelGGL((gemm_bf16_persistent_kernel<T16, EPI, TAIL>), dim3(grid), dim3(512), t256::LDS_BYTES, s, g, full_m, tiles_n, tail_m, tail_mi);
  });
}
template <typename T16>
void launch_gemm_bf16_v4(const GemmArgs& g, hipStream_t s) {
  const int tiles_m = (g.M + 255) / 256, tiles_n = g.N / 256;   // per group
  launch_persistent<T16, false>(g, tiles_m * tiles_n * std::max(1, g.groups), tiles_cus(), tiles_m, tiles_n, 0, 0, s);
}
template void launch_gemm_bf16_v4<bf16_t>(const GemmArgs&, hipStream_t);
template void launch_gemm_bf16_v4<f16_t>(const GemmArgs&, hipStream_t);

// ---- v5: where to cut the rows, and how tall the tail's tiles are ----
// Makespan model of the static schedule (per-XCD chunks, round-robin over the XCD's workgroups), in units of one 256 x 256 tile;
// a 192-row tile is priced 0.80, a 128-row tile 0.62 (measured: see DESIGN 4.11).  A plan must beat the plain tiling by more than
// 0.15 tile-times and its tail must fit one round.
struct V5Plan { int full_m = 0, tail_m = 0, tail_mi = 0; };
static bool v5_plan(int M, int tiles_n, int cus, V5Plan& plan) {
  if (cus < 8 || cus % 8) return false;
  const int tm_all = (M + 255) / 256, per = cus / 8;
  auto rounds = [&](int n) { return ((n + 7) / 8 + per - 1) / per; };
  double best = rounds(tm_all * tiles_n) - 0.15;
  bool found = false;
  for (int mi = 6; mi >= 4; mi -= 2) {
    const double cost = mi == 6 ? 0.80 : 0.62;
    for (int full_m = tm_all - 1; full_m >= 0 && full_m >= tm_all - 96; --full_m) {
      const int tail_rows = M - full_m * 256;
      if (tail_rows <= 0) continue;
      const int tail_m = (tail_rows + mi * 32 - 1) / (mi * 32), nt = tail_m * tiles_n;
      if (nt > cus) break;                       // taller full region -> fewer tail tiles: nothing further down fits either
      const double est = rounds(full_m * tiles_n) + cost * rounds(nt);
      if (est < best) { best = est; plan.full_m = full_m; plan.tail_m = tail_m; plan.tail_mi = mi; found = true; }
    }
  }
  return found;
}
// false: no plan beats the plain tiling for this shape (the caller launches v4)
template <typename T16>
bool launch_gemm_bf16_v5(const GemmArgs& g, hipStream_t s) {
  const int cus = tiles_cus(), tiles_n = g.N / 256;
  V5Plan p;
  if (!gemm_bf16_v5_ok(g) || !v5_plan(g.M, tiles_n, cus, p)) return false;
  launch_persistent<T16, true>(g, (p.full_m + p.tail_m) * tiles_n, cus, p.full_m, tiles_n, p.tail_m, p.tail_mi, s);
  return true;
}
template bool launch_gemm_bf16_v5<bf16_t>(const GemmArgs&, hipStream_t);
template bool launch_gemm_bf16_v5<f16_t>(const GemmArgs&, hipStream_t);

bool gemm_bf16_fast_ok(const GemmArgs& g) {
  return g.N % 128 == 0 && g.K % 64 == 0 && g.lda % 8 == 0 && g.ldw % 8 == 0 && g.M >= 1 &&
         ((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.W % 16) == 0;
}

template <typename T16>
void launch_gemm_bf16_fast(const GemmArgs& g, hipStream_t s) {
  int tiles_m = (g.M + 127) / 128, tiles_n = g.N / 128;
  dim3 grid(tiles_m * tiles_n, 1, g.batch);
  hipLaunchKernelGGL(gemm_bf16_fast_kernel<T16>, grid, dim3(256), 65536, s, g, tiles_m, tiles_n);
}
template void launch_gemm_bf16_fast<bf16_t>(const GemmArgs&, hipStream_t);
template void launch_gemm_bf16_fast<f16_t>(const GemmArgs&, hipStream_t);
