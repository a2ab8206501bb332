// Prompt prefill at a session's admission (option "session_prefill"): the kernels of a pass over PACKED
// rows - sequence after sequence, every sequence with its own cross-KV slot and its own page list (tables: prefill_tables.hpp).
//   prefill_embed          x[row] = emb[token] + pos[position] into the f32 residual
//   prefill_self_attn      append launch + attend launch (a position reads keys that other workgroups of the first launch
//                          write): row (s, t) writes K / V of position t into sequence s's pages and attends to 0 .. t
//   prefill_cross_attn     16-bit engines: ragged MFMA flash cross-attention, one workgroup per (head, work item); MAPS = true
//                          (the packed alignment pass, option align_packed) also leaves the selected heads' score rows, which
//                          prefill_maps_finish turns into softmax maps
// The f32 engine's cross-attention is the per-row kernel of the alignment pass with row -> slot from the table
// (launch_cross_attn_probs_batch).  Every row's result depends on the row's own sequence only: nothing here reads the pass's size.
#include "common.hpp"
#include <cstdio>
#include <type_traits>

constexpr int PF_PAGE = 16;   // positions per KV page (pool layout per layer: [page][2 (K, V)][H][16][64])

template <typename T>
__global__ __launch_bounds__(256) void prefill_embed_kernel(const int32_t* __restrict__ rows, const T* __restrict__ emb,
                                                            const T* __restrict__ pos, float* __restrict__ x, int d) {
  const int b = blockIdx.x, p = rows[3 * b + 1], tok = rows[3 * b + 2];
  for (int i = threadIdx.x; i < d; i += 256) x[(int64_t)b * d + i] = to_f<T>(emb[(int64_t)tok * d + i]) + to_f<T>(pos[(int64_t)p * d + i]);
}
template <typename T>
void launch_prefill_embed(const PrefillPass& P, const T* emb, const T* pos, float* x, int d, hipStream_t s) {
  hipLaunchKernelGGL(prefill_embed_kernel<T>, dim3(P.n_rows), dim3(256), 0, s, P.rows, emb, pos, x, d);
}

// append: packed row b = (sequence, position) stores its k, v (columns d .. 3d of its qkv row) at the position's place in the
// sequence's page.  The page comes from the sequence's own list: no other page is ever touched.
template <typename T>
__global__ __launch_bounds__(256) void prefill_append_kernel(const T* __restrict__ qkv, T* __restrict__ pool, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ seqs, int seq_stride, int H) {
  const int b = blockIdx.x, seq = rows[3 * b], pos = rows[3 * b + 1], d = H * 64;
  const int page = seqs[(int64_t)seq * seq_stride + 3 + pos / PF_PAGE];
  const T* src = qkv + (int64_t)b * 3 * d + d;
  for (int i = threadIdx.x; i < 2 * d; i += 256) {
    const int which = i / d, c = i - which * d, h = c >> 6, j = c & 63;
    pool[((((int64_t)page * 2 + which) * H + h) * PF_PAGE + (pos % PF_PAGE)) * 64 + j] = src[i];
  }
}

// attend: one workgroup (4 waves) per (head, packed row); the keys 0 .. position of the row's sequence from its pages.  A lane
// owns one 16-byte chunk of a key row and keeps an online-softmax state for its row slot; the slots are merged once at the end
// (the structure of self_attn_decode_kernel; all keys come from the pool here).
template <typename T>
__global__ __launch_bounds__(256) void prefill_attend_kernel(const T* __restrict__ qkv, const T* __restrict__ pool, const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ seqs, int seq_stride, T* __restrict__ out, int H) {
  constexpr int VEC = RowVec<T>::VEC, LPR = 64 / VEC, RPI = 64 / LPR;
  __shared__ float part[4][64];
  __shared__ float red[4][2];
  const int b = blockIdx.y, h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = H * 64, seq = rows[3 * b], nk = rows[3 * b + 1] + 1;
  const int32_t* pt = seqs + (int64_t)seq * seq_stride + 3;
  const int sub = lane % LPR, rin = lane / LPR;
  float q[VEC];
  RowVec<T>::load(qkv + (int64_t)b * 3 * d + h * 64 + sub * VEC, q);
  float m_run = -1e30f, l_run = 0.f, acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  const int n_it = (nk + 4 * RPI - 1) / (4 * RPI);
  for (int it = 0; it < n_it; ++it) {
    const int t = (it * 4 + wave) * RPI + rin, tc = min(t, nk - 1);   // clamped, unconditional loads
    const int64_t base = ((int64_t)pt[tc / PF_PAGE] * 2 * H + h) * PF_PAGE + (tc % PF_PAGE);
    float kv[VEC], vv[VEC];
    RowVec<T>::load(pool + base * 64 + sub * VEC, kv);
    RowVec<T>::load(pool + (base + (int64_t)H * PF_PAGE) * 64 + sub * VEC, vv);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) s = fmaf(q[j], kv[j], s);
    s = group_reduce<LPR>(s, OpSum{});
    if (t < nk) {
      const float mn = fmaxf(m_run, s);
      const float sc = __expf(m_run - mn), p = __expf(s - mn);
      l_run = l_run * sc + p;
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] = fmaf(acc[j], sc, p * vv[j]);
      m_run = mn;
    }
  }
  // merge the slots: workgroup maximum, then weights exp(m - M); a slot that saw no key has l = 0 and acc = 0
  const float mw = wave_max(m_run);
  if (lane == 0) red[wave][0] = mw;
  __syncthreads();
  const float M = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
  const float wgt = __expf(m_run - M);
  float lw = (sub == 0) ? l_run * wgt : 0.f;   // l is replicated over the LPR lanes of a row slot: count it once
  lw = wave_sum(lw);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    acc[j] *= wgt;
    acc[j] = stride_reduce<LPR>(acc[j], OpSum{});
  }
  if (lane == 0) red[wave][1] = lw;
  if (rin == 0) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) part[wave][sub * VEC + j] = acc[j];
  }
  __syncthreads();
  if (tid < 64) {
    const float denom = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    const float v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    out[(int64_t)b * d + h * 64 + tid] = from_f<T>(v / denom);
  }
}
template <typename T>
void launch_prefill_self_attn(const PrefillPass& P, const T* qkv, T* pool_layer, T* out, int H, hipStream_t s) {
  hipLaunchKernelGGL(prefill_append_kernel<T>, dim3(P.n_rows), dim3(256), 0, s, qkv, pool_layer, P.rows, P.seqs, P.seq_stride, H);
  hipLaunchKernelGGL(prefill_attend_kernel<T>, dim3(H, P.n_rows), dim3(256), 0, s, qkv, (const T*)pool_layer, P.rows, P.seqs, P.seq_stride, out, H);
  if (g_self_attn_sig) snprintf(g_self_attn_sig, kSelfAttnSigLen, "prefill_append_kernel<%s> grid %d + prefill_attend_kernel<%s> grid %d", sig_type<T>(),
                                P.n_rows * 256, sig_type<T>(), H * P.n_rows * 256);
}

// ------------------------------------------------------------------------------------------------
// Ragged MFMA cross-attention.  One workgroup (4 waves) per (head, work item): the item's <= 128 query rows are the 32-column B
// operands of the four waves, K and V of the sequence's slot ([slot][head][Tk][64]) are streamed ONCE per item in 64-key tiles
// through the double-buffered LDS image by LDS-DMA.  The scheme is that of kernels_flash.hip (one 32-query block per wave):
// S^T = K Q^T with keys on the MFMA rows and the query on the lane, online softmax in f32 with the lazily moved reference inside
// the score MFMA, the accumulator converted in place into the B operand of O^T += V^T P^T, V fragments by ds_read_b64_tr_b16,
// the same K / V swizzles applied on the source side of the DMA.  Query rows past the item's count are loaded clamped and never
// stored; a wave without a live row stages its share of K / V and keeps the barriers, and runs no MFMA or softmax.  Tk is any
// even value >= 4: the last tile (the only one when Tk < 64) loads clamped key rows and masks them.  A query's result depends on
// its own q and on the key-tile order only - not on the item, the other items of the launch or their number.
// SOURCE: the body is enc_attn_flash_kernel<T16, CROSS = true, QW = 1> of kernels_flash.hip with (batch, Tn) replaced by the item
// table (that template is what the benchmark launches and takes no new modes).  A fix to the swizzles, the clamped tail DMA and
// its mask index, the first-tile alpha guard, the vmcnt / barrier order or the epilogue's LDS reuse belongs in BOTH places.
// MAPS = true (the alignment pass of option align_packed, ttasr_align_attn_probe) is the same body; a workgroup whose head is
// selected (mp.sel[h] = pair >= 0) additionally stores, for its live rows and the keys below n_k,
//   maps[pair][row][key] = the score in exp2 units, ABSOLUTE: what the MFMA delivered plus the reference it was taken against -
//                          the one coordinate that does not move with the lazily moved reference
//   stat[pair][row]      = {final reference, softmax sum against it}
// and prefill_maps_finish_kernel turns each stored row into exp2(score - reference) / sum in place.  Nothing else changes: the
// attention output is computed by the same instructions in the same order, and MAPS = false has no argument and no code of it.
// ------------------------------------------------------------------------------------------------
typedef short pf_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ pf_s16x4 pf_lds_tr16(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((pf_s16x4 __attribute__((address_space(3)))*)(p));
}
constexpr int PF_KB = 64;   // keys per tile

template <typename T16, bool MAPS, typename... MP>   // MP = PrefillMaps when MAPS, else empty: MAPS = false keeps its argument list
__global__ __launch_bounds__(256, 3) void prefill_cross_attn_kernel(const bf16_t* __restrict__ q, bf16_t* __restrict__ out,
                                                                    const int32_t* __restrict__ items, const int32_t* __restrict__ seqs,
                                                                    int seq_stride, int H, const bf16_t* __restrict__ kx,
                                                                    const bf16_t* __restrict__ vx, int n_k, MP... mp_) {
  static_assert(sizeof...(MP) == (MAPS ? 1 : 0), "MAPS = true takes one PrefillMaps");
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x (K 8 KiB | V 8 KiB); reused for the O transpose
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hf = lane >> 5;
  const int h = blockIdx.x;
  const int32_t* it = items + 3 * (int64_t)blockIdx.y;
  const int seq = __builtin_amdgcn_readfirstlane(it[0]), row0 = __builtin_amdgcn_readfirstlane(it[1]);
  const int n_q = __builtin_amdgcn_readfirstlane(it[2]);
  const int slot = __builtin_amdgcn_readfirstlane(seqs[(int64_t)seq * seq_stride]);
  const int d = H * 64, q0 = wave * 32;   // this wave's first query of the item
  const bf16_t* base = q + (int64_t)row0 * d + h * 64;                // query rows of the item, head h
  const bf16_t* kbase = kx + ((int64_t)slot * H + h) * n_k * 64;
  const bf16_t* vbase = vx + ((int64_t)slot * H + h) * n_k * 64;

  // Q fragments (B operand of S^T): lane holds Q[q0 + r][16*ks + 8*hf .. +8], multiplied by log2(e) once: the scores leave the
  // MFMA in exp2 units
  constexpr float LOG2E = 1.4426950408889634f;
  s16x8 qf[4];
  {
    const bf16_t* qp = base + (int64_t)min(q0 + r, n_q - 1) * d + 8 * hf;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      uint4 t = *(const uint4*)(qp + 16 * ks);
      float v[8];
      up8<T16>(t, v);
      t.x = N16<T16>::pk(v[0] * LOG2E, v[1] * LOG2E); t.y = N16<T16>::pk(v[2] * LOG2E, v[3] * LOG2E);
      t.z = N16<T16>::pk(v[4] * LOG2E, v[5] * LOG2E); t.w = N16<T16>::pk(v[6] * LOG2E, v[7] * LOG2E);
      qf[ks] = __builtin_bit_cast(s16x8, t);
    }
  }
  const bool live = q0 < n_q;
  // MAPS: this lane's row of the selected head's map (nullptr: head not selected, or a row past the item's count)
  [[maybe_unused]] float* map_row = nullptr;
  [[maybe_unused]] float* stat_row = nullptr;
  if constexpr (MAPS) {
    const PrefillMaps mp = (mp_, ...);
    const int pair = __builtin_amdgcn_readfirstlane(mp.sel[h]);
    if (pair >= 0 && q0 + r < n_q) {
      const int64_t row = (int64_t)pair * mp.n_rows + row0 + q0 + r;
      map_row = mp.maps + row * n_k;
      stat_row = mp.stat + row * 2;
    }
  }

  // K / V staging by LDS-DMA: a wave-instruction of global_load_lds moves 1 KiB = 8 rows x 128 B straight into the LDS image.  A
  // tile is 8 K pieces + 8 V pieces; wave w issues K pieces 2w, 2w+1 and V pieces 2w, 2w+1.  Lane l of piece p lands in row
  // 8p + l/8, 16-byte slot l%8, so it FETCHES the chunk that belongs in that slot under the image's swizzle (K: chunk c of row k
  // sits in slot c ^ ((k>>1)&7); V: slot c ^ (((k>>1)&1) << 2)).
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int prow = lane >> 3, pslot = lane & 7;
  uint32_t koff[2], voff[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = (2 * wave_u + p) * 8 + prow;
    koff[p] = (uint32_t)(row * 64 + ((pslot ^ ((row >> 1) & 7)) << 3)) * 2u;
    voff[p] = (uint32_t)(row * 64 + ((pslot ^ (((row >> 1) & 1) << 2)) << 3)) * 2u;
  }
  const int64_t tstep = (int64_t)PF_KB * 64 * 2;               // bytes per tile
  const int full_tiles = n_k / PF_KB;                          // tiles 0 .. full_tiles-1 need no clamp
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef void __attribute__((address_space(3)))* lptr_t;
#define PF_DMA(kt_, buf_)                                                                                          \
  do {                                                                                                             \
    char* Kb_ = smem + (buf_) * 16384 + (2 * wave_u) * 1024;                                                       \
    char* Vb_ = Kb_ + 8192;                                                                                        \
    if ((kt_) < full_tiles) {                                                                                      \
      const char* kt_base_ = (const char*)kbase + (int64_t)(kt_) * tstep;                                          \
      const char* vt_base_ = (const char*)vbase + (int64_t)(kt_) * tstep;                                          \
      _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                              \
        __builtin_amdgcn_global_load_lds((gptr_t)(kt_base_ + koff[p]), (lptr_t)(Kb_ + p * 1024), 16, 0, 0);        \
        __builtin_amdgcn_global_load_lds((gptr_t)(vt_base_ + voff[p]), (lptr_t)(Vb_ + p * 1024), 16, 0, 0);        \
      }                                                                                                            \
    } else {                                                                                                       \
      _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                              \
        const int row_ = (2 * wave_u + p) * 8 + prow;                                                              \
        const int key_ = min((kt_) * PF_KB + row_, n_k - 1);   /* never past the slot's last key row */            \
        const bf16_t* kp_ = kbase + (int64_t)key_ * 64 + ((pslot ^ ((row_ >> 1) & 7)) << 3);                       \
        const bf16_t* vp_ = vbase + (int64_t)key_ * 64 + ((pslot ^ (((row_ >> 1) & 1) << 2)) << 3);                \
        __builtin_amdgcn_global_load_lds((gptr_t)kp_, (lptr_t)(Kb_ + p * 1024), 16, 0, 0);                         \
        __builtin_amdgcn_global_load_lds((gptr_t)vp_, (lptr_t)(Vb_ + p * 1024), 16, 0, 0);                         \
      }                                                                                                            \
    }                                                                                                              \
  } while (0)

  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[i][j] = 0.f;
  // Online softmax with the reference maximum inside the score MFMA: the accumulator of S^T starts at -m_ref, so the MFMA delivers
  // s - m_ref and p = exp2(s - m_ref) is one v_exp_f32 per element.  m_ref moves only when a tile's maximum exceeds it by more
  // than PF_THR exp2 units (p <= 64: well inside bf16 / fp16), and the first tile always sets it; the decision is taken before
  // the tile's P is exponentiated and scales o, l and this tile's scores exactly once: the exact softmax whatever m_ref is.
  constexpr float PF_THR = 6.0f;
  float m_ref = 0.f, l_run = 0.f;

  const int n_tiles = (n_k + PF_KB - 1) / PF_KB;
  PF_DMA(0, 0);
  // explicit: a wave with no live query reads no LDS itself, so nothing else forces ITS pieces to have landed before the others
  // pass the barrier and read them
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int vq = (lane & 15) >> 2, vp4 = lane & 3, vg = (lane >> 4) & 1;

  auto tile = [&](const int kt, auto cur_tag, auto last_tag) {
    constexpr bool LAST = decltype(last_tag)::value;
    constexpr int cur = decltype(cur_tag)::value;
    // tile kt + 1 into the other image: its last readers (tile kt - 1) are behind the barrier every wave has passed
    if (!LAST) PF_DMA(kt + 1, cur ^ 1);
    const char* Kb = smem + cur * 16384;
    const char* Vb = Kb + 8192;
    if (live) {
      // ---- S^T - m_ref = K Q^T - m_ref : two 32-key blocks ----
      f32x16 s[2];
      {
        f32x16 si;
#pragma unroll
        for (int j = 0; j < 16; ++j) si[j] = -m_ref;
        s[0] = si; s[1] = si;
      }
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2) {
        const int krow = 32 * kb2 + r;
        const int ksw = (krow >> 1) & 7;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          s16x8 kf = *(const s16x8*)(Kb + krow * 128 + (((2 * ks + hf) ^ ksw) << 4));
          s[kb2] = N16<T16>::mfma32(kf, qf[ks], s[kb2]);
        }
      }
      if (LAST) {  // mask keys past the end of the window (only the peeled last tile carries this code)
#pragma unroll
        for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int key = kt * PF_KB + 32 * kb2 + (j & 3) + 8 * (j >> 2) + 4 * hf;
            if (key >= n_k) s[kb2][j] = -1e30f;
          }
      }
      if constexpr (MAPS) {
        // lane (r, hf) holds keys kt*64 + 32 kb2 + 8 g + 4 hf + 0..3 of query r: two 8-byte stores per group (n_k is even, so a
        // row starts 8-byte aligned and a pair of keys is inside the window or outside it together); a clamped key is never stored
        if (map_row) {
#pragma unroll
          for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
              for (int e = 0; e < 4; e += 2) {
                const int key = kt * PF_KB + 32 * kb2 + 8 * g4 + 4 * hf + e;
                if (!LAST || key < n_k)
                  *(float2*)(map_row + key) = make_float2(s[kb2][4 * g4 + e] + m_ref, s[kb2][4 * g4 + e + 1] + m_ref);
              }
        }
      }
      // ---- this lane's query column: how far above the reference is the tile's maximum? ----
      float tmax = s[0][0];
#pragma unroll
      for (int j = 1; j < 16; ++j) tmax = fmaxf(tmax, s[0][j]);
#pragma unroll
      for (int j = 0; j < 16; ++j) tmax = fmaxf(tmax, s[1][j]);
      tmax = xor32_reduce(tmax, OpMax{});
      const bool move = (kt == 0) | (tmax > PF_THR);
      if (__builtin_amdgcn_ballot_w64(move) != 0) {
        const float delta = move ? tmax : 0.f;       // exp2(0) = 1 exactly for the others
        // first tile: o and l are still 0, only the reference moves - the rescale factor must not be evaluated (a first-tile
        // maximum far below zero would make exp2(-tmax) = +inf and 0 * inf = NaN for the whole query row)
        const float alpha = kt == 0 ? 1.0f : __builtin_amdgcn_exp2f(-delta);
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 16; ++j) { o[i][j] *= alpha; s[i][j] -= delta; }
        m_ref += delta;
      }
      uint32_t pf[2][8];  // 16-bit-packed P^T: [kb2][2*s' + pair]
      float psum = 0.f;
#pragma unroll
      for (int kb2 = 0; kb2 < 2; ++kb2)
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
          const float p0 = __builtin_amdgcn_exp2f(s[kb2][j]);
          const float p1 = __builtin_amdgcn_exp2f(s[kb2][j + 1]);
          psum += p0 + p1;
          pf[kb2][j >> 1] = N16<T16>::pk(p0, p1);
        }
      l_run += psum;

      // ---- O^T += V^T P^T : 4 k-steps of 16 keys, 2 d-blocks ----
#pragma unroll
      for (int ss = 0; ss < 4; ++ss) {
        const int kb2 = ss >> 1, sp = ss & 1;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const int vrow0 = 16 * ss + 4 * hf + vq;
          const int vrow1 = vrow0 + 8;
          const pf_s16x4 lo = pf_lds_tr16(Vb + vrow0 * 128 + (((db ^ ((vrow0 >> 1) & 1)) << 6) | (vg << 5) | (vp4 << 3)));
          const pf_s16x4 hi = pf_lds_tr16(Vb + vrow1 * 128 + (((db ^ ((vrow1 >> 1) & 1)) << 6) | (vg << 5) | (vp4 << 3)));
          const s16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          const uint4 t = make_uint4(pf[kb2][4 * sp + 0], pf[kb2][4 * sp + 1], pf[kb2][4 * sp + 2], pf[kb2][4 * sp + 3]);
          o[db] = N16<T16>::mfma32(vf, __builtin_bit_cast(s16x8, t), o[db]);
        }
      }
    }  // live
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile kt + 1 landed
    __syncthreads();   // barrier: everybody's did
  };
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  int kt = 0;
  for (; kt + 2 < n_tiles; kt += 2) {
    tile(kt, B0{}, std::false_type{});
    tile(kt + 1, B1{}, std::false_type{});
  }
  if (kt + 2 == n_tiles) {
    tile(kt, B0{}, std::false_type{});
    tile(kt + 1, B1{}, std::true_type{});
  } else {
    tile(kt, B0{}, std::true_type{});
  }
#undef PF_DMA

  // ---- epilogue: O^T[d][q] / l  ->  out[row0 + q][h*64 + d], transposed through LDS so rows leave as 128 B ----
  char* ob = smem + wave * (32 * 144);  // [32 q][64 d] 16-bit, row stride 144 B (128 + 16 pad); wave-private
  const float l_tot = xor32_reduce(l_run, OpSum{});
  const float inv = 1.0f / l_tot;       // (a wave without a live row never stores what it computes here)
  if constexpr (MAPS) {
    if (stat_row && hf == 0) *(float2*)stat_row = make_float2(m_ref, l_tot);   // both halves of a query hold the same reference
  }
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      uint2 pk;
      pk.x = N16<T16>::pk(o[db][4 * rg + 0] * inv, o[db][4 * rg + 1] * inv);
      pk.y = N16<T16>::pk(o[db][4 * rg + 2] * inv, o[db][4 * rg + 3] * inv);
      const int dcol = 32 * db + 8 * rg + 4 * hf;
      *(uint2*)(ob + r * 144 + dcol * 2) = pk;
    }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
#pragma unroll
  for (int i4 = 0; i4 < 4; ++i4) {
    const int id = i4 * 64 + lane, row = id >> 3, c = id & 7;
    if (q0 + row < n_q) {
      const uint4 v = *(const uint4*)(ob + row * 144 + c * 16);
      *(uint4*)(out + ((int64_t)row0 + q0 + row) * d + h * 64 + c * 8) = v;
    }
  }
}
template <typename T16>
void launch_prefill_cross_attn(const PrefillPass& P, const T16* q, const T16* K, const T16* V, T16* out, int H, int Tk, hipStream_t s) {
  hipLaunchKernelGGL((prefill_cross_attn_kernel<T16, false>), dim3(H, P.n_items), dim3(256), 32768, s, (const bf16_t*)q, (bf16_t*)out, P.items,
                     P.seqs, P.seq_stride, H, (const bf16_t*)K, (const bf16_t*)V, Tk);
}
template <typename T16>
void launch_prefill_cross_attn_maps(const PrefillPass& P, const T16* q, const T16* K, const T16* V, T16* out, int H, int Tk,
                                    const PrefillMaps& mp, hipStream_t s) {
  hipLaunchKernelGGL((prefill_cross_attn_kernel<T16, true, PrefillMaps>), dim3(H, P.n_items), dim3(256), 32768, s, (const bf16_t*)q,
                     (bf16_t*)out, P.items, P.seqs, P.seq_stride, H, (const bf16_t*)K, (const bf16_t*)V, Tk, mp);
}

// The stored score rows of launch_prefill_cross_attn_maps -> softmax over the n_k frames, in place and in f32: one workgroup per
// (packed row, pair); p = exp2(score - reference) / sum with the row's own reference and sum (stat), nothing of any other row.
__global__ __launch_bounds__(256) void prefill_maps_finish_kernel(float* __restrict__ maps, const float* __restrict__ stat, int n_k) {
  const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const float m = stat[2 * row], inv = 1.0f / stat[2 * row + 1];
  float* p = maps + row * n_k;
  for (int f = threadIdx.x; f < n_k; f += 256) p[f] = __builtin_amdgcn_exp2f(p[f] - m) * inv;
}
void launch_prefill_maps_finish(float* maps, const float* stat, int n_pairs, int n_rows, int Tk, hipStream_t s) {
  hipLaunchKernelGGL(prefill_maps_finish_kernel, dim3(n_rows, n_pairs), dim3(256), 0, s, maps, stat, Tk);
}

#define TTASR_PF_ALL(T_)                                                                                          \
  template void launch_prefill_embed<T_>(const PrefillPass&, const T_*, const T_*, float*, int, hipStream_t);     \
  template void launch_prefill_self_attn<T_>(const PrefillPass&, const T_*, T_*, T_*, int, hipStream_t)
TTASR_PF_ALL(float); TTASR_PF_ALL(bf16_t); TTASR_PF_ALL(f16_t);
#undef TTASR_PF_ALL
template void launch_prefill_cross_attn<bf16_t>(const PrefillPass&, const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, hipStream_t);
template void launch_prefill_cross_attn<f16_t>(const PrefillPass&, const f16_t*, const f16_t*, const f16_t*, f16_t*, int, int, hipStream_t);
template void launch_prefill_cross_attn_maps<bf16_t>(const PrefillPass&, const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, const PrefillMaps&, hipStream_t);
template void launch_prefill_cross_attn_maps<f16_t>(const PrefillPass&, const f16_t*, const f16_t*, const f16_t*, f16_t*, int, int, const PrefillMaps&, hipStream_t);
