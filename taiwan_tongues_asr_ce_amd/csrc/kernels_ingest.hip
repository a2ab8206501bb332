// File ingest (include/ttasr.h ttasr_ingest_pcm): raw interleaved samples -> float32 mono 16 kHz in one kernel.
//
//   ingest_kernel   one 256-thread workgroup per tile of consecutive outputs of one recording.  The workgroup stages the input
//                   span of its tile into LDS - raw samples read with consecutive lanes on consecutive frames, converted to
//                   [-1, 1) and averaged over the channels on the way in, zeros outside the recording - and every thread then
//                   accumulates its outputs in f32 over the taps of its phase row, input index ascending.  No atomics; an output's
//                   operands and their order are a function of its index alone, so neither the tile length nor the chunk, the
//                   number of recordings or a recording's place in the call can change a bit of it.
//
// The taps are read from the phase-major table in global memory (at most 84 KiB per rate: it lives in L2 and the vector L1).  With
// up == 1 there is one row and the tap address is wave-uniform: the UP1 instance reads it through the scalar unit.  With up > 1
// neighbouring lanes sit on different rows and gather.  Output and tap indices are 64-bit: k * down passes 2^31 after about five
// minutes of 44.1 kHz audio.
#include "common.hpp"
#include "ingest.hpp"

namespace {

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// One sample as decode_audio converts it: the integer formats scaled by a power of two (exact), 32-bit integers and doubles rounded
// to float32 (nearest even) first.  Packed 24-bit samples are read byte by byte: they are not dword-aligned.
template <int FMT>
__device__ __forceinline__ float ingest_sample(const uint8_t* __restrict__ raw, int64_t idx) {
  if constexpr (FMT == TTASR_PCM_U8) return ((float)raw[idx] - 128.0f) * (1.0f / 128.0f);
  else if constexpr (FMT == TTASR_PCM_S16) return (float)((const int16_t*)raw)[idx] * (1.0f / 32768.0f);
  else if constexpr (FMT == TTASR_PCM_S24) {
    const uint8_t* b = raw + idx * 3;
    const int32_t v = (int32_t)((uint32_t)b[0] << 8 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 24) >> 8;
    return (float)v * (1.0f / 8388608.0f);
  } else if constexpr (FMT == TTASR_PCM_S32) return (float)((const int32_t*)raw)[idx] * (1.0f / 2147483648.0f);
  else if constexpr (FMT == TTASR_PCM_F32) return ((const float*)raw)[idx];
  else return (float)((const double*)raw)[idx];
}

// mono[i] of the staged range: the channels summed in order, then one division (what numpy's mean over the channel axis does)
template <int FMT>
__device__ __forceinline__ float ingest_frame(const uint8_t* __restrict__ raw, int64_t r, int channels) {
  float v = ingest_sample<FMT>(raw, r * channels);
  if (channels == 1) return v;
  for (int c = 1; c < channels; ++c) v += ingest_sample<FMT>(raw, r * channels + c);
  return v / (float)channels;
}

template <int FMT>
__device__ __forceinline__ void ingest_stage(const IngestJob& J, float* s, int64_t i_lo) {
  for (int q = threadIdx.x; q < J.span; q += kIngestThreads) {
    const int64_t i = i_lo + q, r = i - J.f0;
    float v = 0.0f;
    if (i >= 0 && i < J.n_frames && r >= 0 && r < J.nf) v = ingest_frame<FMT>(J.raw, r, J.channels);
    s[q] = v;
  }
}

template <bool UP1>
__global__ __launch_bounds__(kIngestThreads) void ingest_kernel(const IngestJob J) {
  extern __shared__ float s[];   // [span] mono samples from frame i_lo on
  const int64_t k0 = J.k_begin + (int64_t)blockIdx.x * J.tile;
  const int64_t left = J.k_begin + J.n_out - k0;
  const int nk = left < J.tile ? (int)left : J.tile;
  const int64_t i_lo = J.taps ? -floor_div((int64_t)J.half - k0 * J.down, J.up) : k0;   // ceil((k0 down - half) / up)
  switch (J.format) {
    case TTASR_PCM_U8: ingest_stage<TTASR_PCM_U8>(J, s, i_lo); break;
    case TTASR_PCM_S16: ingest_stage<TTASR_PCM_S16>(J, s, i_lo); break;
    case TTASR_PCM_S24: ingest_stage<TTASR_PCM_S24>(J, s, i_lo); break;
    case TTASR_PCM_S32: ingest_stage<TTASR_PCM_S32>(J, s, i_lo); break;
    case TTASR_PCM_F32: ingest_stage<TTASR_PCM_F32>(J, s, i_lo); break;
    default: ingest_stage<TTASR_PCM_F64>(J, s, i_lo); break;
  }
  __syncthreads();
  float* __restrict__ out = J.out + (k0 - J.k_begin);
  if (!J.taps) {
    for (int kk = threadIdx.x; kk < nk; kk += kIngestThreads) out[kk] = s[kk];
    return;
  }
  for (int kk = threadIdx.x; kk < nk; kk += kIngestThreads) {
    // y[k] = sum_i mono[i] h[a - i up], a = k down + half: with ih = a / up and p = a % up the taps are row p of the table,
    // h[p + j up] at i = ih - j, for the j whose tap index is at most 2 half
    const int64_t a = (k0 + kk) * J.down + J.half;
    int64_t ih; int p, jmax;
    if constexpr (UP1) { ih = a; p = 0; jmax = 2 * J.half; }
    else { ih = a / J.up; p = (int)(a - ih * J.up); jmax = (2 * J.half - p) / J.up; }
    const float* __restrict__ row = J.taps + (size_t)p * J.L;
    const float* __restrict__ x = s + (int)(ih - i_lo);
    float acc = 0.0f;
    for (int j = jmax; j >= 0; --j) acc = fmaf(x[-j], row[j], acc);   // i ascending
    out[kk] = acc;
  }
}

}  // namespace

void launch_ingest(const IngestJob& j, hipStream_t s) {
  if (j.n_out <= 0) return;
  const int64_t need = j.taps ? ingest_span(j.tile, j.up, j.down, j.half) : j.tile;
  if (j.tile < 1 || j.tile > kIngestMaxTile || j.span < need || j.span > kIngestSpanMax || j.channels < 1 || j.channels > 8 ||
      j.format < TTASR_PCM_U8 || j.format > TTASR_PCM_F64 || j.nf < 0 || (j.taps && (j.up < 1 || j.down < 1 || j.L < 1))) {
    launch_fault("ingest: tile %d span %d (needs %lld) channels %d format %d", j.tile, j.span, (long long)need, j.channels, j.format);
    return;
  }
  const size_t lds = (size_t)j.span * sizeof(float);
  if (lds > 64 * 1024) {   // the rare ratios only; per device, so asked for at every such launch
    (void)hipFuncSetAttribute((const void*)ingest_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kIngestSpanMax * 4);
    (void)hipFuncSetAttribute((const void*)ingest_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kIngestSpanMax * 4);
  }
  const unsigned grid = (unsigned)((j.n_out + j.tile - 1) / j.tile);
  if (j.taps && j.up == 1) ingest_kernel<true><<<grid, kIngestThreads, lds, s>>>(j);
  else ingest_kernel<false><<<grid, kIngestThreads, lds, s>>>(j);
}
