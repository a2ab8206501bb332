// File ingest (include/ttasr.h ttasr_ingest_pcm / ttasr_ingest_wave): raw interleaved samples -> float32 mono 16 kHz in one kernel.
//
//   ingest_kernel   one 256-thread workgroup per tile of consecutive outputs of one recording.  The workgroup stages the input
//                   span of its tile into LDS - raw samples read with consecutive lanes on consecutive frames, converted to
//                   [-1, 1) and averaged over the channels on the way in, zeros outside the recording - and every thread then
//                   accumulates its outputs in f32 over the taps of its phase row, input index ascending.  No atomics; an output's
//                   operands and their order are a function of its index alone, so neither the tile length nor the chunk, the
//                   number of recordings or a recording's place in the call can change a bit of it.
//
//   ima_decode_kernel  the pre-pass of IMA ADPCM recordings: one lane per (block, channel) walks its block - a serial chain of
//                   predictor and step index - and writes int16 [frames][channels]; ingest_kernel then reads that as s16.  Lane t
//                   takes block t % n_blocks of channel t / n_blocks: consecutive lanes read consecutive blocks of one channel.
//
//   flac_decode_kernel  the pre-pass of FLAC recordings: one lane per FLAC frame runs the decode body of flac.hpp - the one the
//                   host decoder runs - over its frame's bytes: header, subframes (Rice residual, predictor recurrence) into the
//                   lane's int32 work rows, then decorrelation and the left-justified interleaved store; ingest_kernel reads that
//                   as s16 or s32.  A frame is a serial bit stream, so the frame is the unit of parallelism; the lane's status
//                   word goes out with an ordinary store.  64-thread workgroups, so that a chunk's frames spread over the CUs.
//
//   wire_kernel     ingest_kernel for wire streams (ttasr_vad_stream_push_wire): ONE launch for all rows of
//                   a push chunk, the jobs in a device table, the span staged from the stream's history in a device table and
//                   then from the new frames, the same sum; one more workgroup per row writes the row's new history into the
//                   table half the tiles do not read.
//
// The taps are read from the phase-major table in global memory (at most 84 KiB per rate: it lives in L2 and the vector L1).  With
// up == 1 there is one row and the tap address is wave-uniform: the UP1 instance reads it through the scalar unit.  With up > 1
// neighbouring lanes sit on different rows and gather.  Output and tap indices are 64-bit: k * down passes 2^31 after about five
// minutes of 44.1 kHz audio.
#include "common.hpp"
#include "ingest.hpp"
#include "flac.hpp"

namespace {

__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// One sample as decode_audio converts it: the integer formats scaled by a power of two (exact), 32-bit integers and doubles rounded
// to float32 (nearest even) first.  Packed 24-bit samples are read byte by byte: they are not dword-aligned.  The two G.711 laws
// expand a byte to its int16 with shifts and adds (the header's formulas; no table), then scale as s16 does.
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
  else if constexpr (FMT == TTASR_PCM_ULAW) {
    const int u = ~(int)raw[idx] & 0xFF, e = (u >> 4) & 7, m = u & 15;
    const int v = (((m << 3) + 0x84) << e) - 0x84;
    return (float)((u & 0x80) ? -v : v) * (1.0f / 32768.0f);
  } else if constexpr (FMT == TTASR_PCM_ALAW) {
    const int a = (int)raw[idx] ^ 0x55, e = (a >> 4) & 7, m = a & 15;
    int v = (m << 4) + 8;
    if (e >= 1) v = (v + 0x100) << (e - 1);
    return (float)((a & 0x80) ? v : -v) * (1.0f / 32768.0f);
  } else return (float)((const double*)raw)[idx];
}

// mono[i] of the staged range: the channels summed in order, then one division (what numpy's mean over the channel axis does);
// with a pick, that channel's sample as it is
template <int FMT>
__device__ __forceinline__ float ingest_frame(const uint8_t* __restrict__ raw, int64_t r, int channels, int pick) {
  if (pick >= 0) return ingest_sample<FMT>(raw, r * channels + pick);
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
    if (i >= 0 && i < J.n_frames && r >= 0 && r < J.nf) v = ingest_frame<FMT>(J.raw, r, J.channels, J.pick);
    s[q] = v;
  }
}

// THE sum of both kernels: out[kk] = y[k0 + kk] for kk < nk from the staged span s (mono samples from frame i_lo on).  A file
// and a wire stream agree bit for bit because they both run this: the same operands in the same order, i ascending.
template <bool UP1>
__device__ __forceinline__ void ingest_sum(const float* __restrict__ taps, int L, int up, int down, int half, const float* s,
                                           float* __restrict__ out, int64_t k0, int64_t i_lo, int nk) {
  for (int kk = threadIdx.x; kk < nk; kk += kIngestThreads) {
    // y[k] = sum_i mono[i] h[a - i up], a = k down + half: with ih = a / up and p = a % up the taps are row p of the table,
    // h[p + j up] at i = ih - j, for the j whose tap index is at most 2 half
    const int64_t a = (k0 + kk) * down + half;
    int64_t ih; int p, jmax;
    if constexpr (UP1) { ih = a; p = 0; jmax = 2 * half; }
    else { ih = a / up; p = (int)(a - ih * up); jmax = (2 * half - p) / up; }
    const float* __restrict__ row = taps + (size_t)p * L;
    const float* __restrict__ x = s + (int)(ih - i_lo);
    float acc = 0.0f;
    for (int j = jmax; j >= 0; --j) acc = fmaf(x[-j], row[j], acc);   // i ascending
    out[kk] = acc;
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
    case TTASR_PCM_ALAW: ingest_stage<TTASR_PCM_ALAW>(J, s, i_lo); break;
    case TTASR_PCM_ULAW: ingest_stage<TTASR_PCM_ULAW>(J, s, i_lo); break;
    default: ingest_stage<TTASR_PCM_F64>(J, s, i_lo); break;
  }
  __syncthreads();
  float* __restrict__ out = J.out + (k0 - J.k_begin);
  if (!J.taps) {
    for (int kk = threadIdx.x; kk < nk; kk += kIngestThreads) out[kk] = s[kk];
    return;
  }
  ingest_sum<UP1>(J.taps, J.L, J.up, J.down, J.half, s, out, k0, i_lo, nk);
}

// mono[i] of a wire stream's row: below frame 0 and behind the chunk zeros, in front of the chunk the stream's history
template <int FMT>
__device__ __forceinline__ float wire_frame(const WireJob& J, const uint8_t* __restrict__ raw, const float* __restrict__ hist, int64_t i) {
  if (i < 0) return 0.0f;
  const int64_t r = i - J.f_old;
  if (r < 0) return r + J.H >= 0 ? hist[J.hist_in + (int)(r + J.H)] : 0.0f;
  return r < J.nf ? ingest_frame<FMT>(raw, r, J.channels, J.pick) : 0.0f;
}

// q-th of `count` mono values from frame i_lo on -> dst[q]
template <int FMT>
__device__ __forceinline__ void wire_stage(const WireJob& J, const uint8_t* __restrict__ raw, const float* __restrict__ hist,
                                           float* dst, int64_t i_lo, int count) {
  for (int q = threadIdx.x; q < count; q += kIngestThreads) dst[q] = wire_frame<FMT>(J, raw, hist, i_lo + q);
}

__device__ __forceinline__ void wire_stage_any(const WireJob& J, const uint8_t* __restrict__ raw, const float* __restrict__ hist,
                                               float* dst, int64_t i_lo, int count) {
  switch (J.format) {
    case TTASR_PCM_U8: wire_stage<TTASR_PCM_U8>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_S16: wire_stage<TTASR_PCM_S16>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_S24: wire_stage<TTASR_PCM_S24>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_S32: wire_stage<TTASR_PCM_S32>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_F32: wire_stage<TTASR_PCM_F32>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_ALAW: wire_stage<TTASR_PCM_ALAW>(J, raw, hist, dst, i_lo, count); break;
    case TTASR_PCM_ULAW: wire_stage<TTASR_PCM_ULAW>(J, raw, hist, dst, i_lo, count); break;
    default: wire_stage<TTASR_PCM_F64>(J, raw, hist, dst, i_lo, count); break;
  }
}

// Wire streams: blockIdx.y is the row of the job table, blockIdx.x a tile of the row's outputs, and the block behind the row's
// last tile writes the row's new history.  Tiles read the history half the row had before the push chunk (hist_in), the history
// block writes the other half (hist_out): no workgroup reads what another writes.  The job's fields are uniform over the
// workgroup: the compiler fetches them through the scalar unit.
__global__ __launch_bounds__(kIngestThreads) void wire_kernel(const WireJob* __restrict__ jobs, const uint8_t* __restrict__ raw_pool,
                                                              float* __restrict__ out_pool, float* __restrict__ hist) {
  extern __shared__ float s[];   // [span] mono samples from frame i_lo on
  const WireJob J = jobs[blockIdx.y];
  const int tiles = (J.n_out + J.tile - 1) / J.tile;
  const int t = (int)blockIdx.x;
  const uint8_t* __restrict__ raw = raw_pool + J.raw_off;
  if (t > tiles) return;
  if (t == tiles) {   // the last H mono values after the chunk
    if (J.hist_out >= 0) wire_stage_any(J, raw, hist, hist + J.hist_out, J.f_old + J.nf - J.H, J.H);
    return;
  }
  const int64_t k0 = J.k_begin + (int64_t)t * J.tile;
  const int left = J.n_out - t * J.tile;
  const int nk = left < J.tile ? left : J.tile;
  const int64_t i_lo = J.taps ? -floor_div((int64_t)J.half - k0 * J.down, J.up) : k0;   // ceil((k0 down - half) / up)
  const int span = J.taps ? (int)((int64_t)nk * J.down / J.up) + 2 * J.half / J.up + 2 : nk;
  wire_stage_any(J, raw, hist, s, i_lo, span);
  __syncthreads();
  float* __restrict__ out = out_pool + J.out_off + t * J.tile;
  if (!J.taps) {
    for (int kk = threadIdx.x; kk < nk; kk += kIngestThreads) out[kk] = s[kk];
    return;
  }
  if (J.up == 1) ingest_sum<true>(J.taps, J.L, J.up, J.down, J.half, s, out, k0, i_lo, nk);
  else ingest_sum<false>(J.taps, J.L, J.up, J.down, J.half, s, out, k0, i_lo, nk);
}

__constant__ int16_t kImaStep[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
    11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767};

__global__ __launch_bounds__(kIngestThreads) void ima_decode_kernel(const ImaJob J) {
  const int64_t t = (int64_t)blockIdx.x * kIngestThreads + threadIdx.x;
  if (t >= (int64_t)J.n_blocks * J.channels) return;
  const int c = (int)(t / J.n_blocks), b = (int)(t - (int64_t)c * J.n_blocks);
  const uint8_t* __restrict__ blk = J.raw + (size_t)b * J.block_align;
  const uint32_t head = *(const uint32_t*)(blk + 4 * c);        // block_align is a multiple of 4: every group is a dword
  int pred = (int16_t)(head & 0xFFFF);
  int index = (head >> 16) & 0xFF;
  if (index > 88) index = 88;
  int64_t fr = (int64_t)b * J.spb;
  int16_t* __restrict__ out = J.out + c;
  if (fr < J.n_frames) out[fr * J.channels] = (int16_t)pred;
  ++fr;
  const int groups = (J.block_align / J.channels - 4) / 4;
  const uint8_t* __restrict__ data = blk + 4 * J.channels + 4 * c;
  for (int g = 0; g < groups && fr < J.n_frames; ++g) {
    uint32_t w = *(const uint32_t*)(data + (size_t)g * 4 * J.channels);
    for (int j = 0; j < 8; ++j, w >>= 4, ++fr) {
      const int n = (int)(w & 15), step = kImaStep[index];
      int d = step >> 3;
      if (n & 4) d += step;
      if (n & 2) d += step >> 1;
      if (n & 1) d += step >> 2;
      pred = (n & 8) ? pred - d : pred + d;
      pred = pred > 32767 ? 32767 : (pred < -32768 ? -32768 : pred);
      index += (n & 4) ? 2 * (n & 3) + 2 : -1;                   // {-1, -1, -1, -1, 2, 4, 6, 8} at n & 7
      index = index < 0 ? 0 : (index > 88 ? 88 : index);
      if (fr < J.n_frames) out[fr * J.channels] = (int16_t)pred;
    }
  }
}

__global__ __launch_bounds__(kFlacThreads) void flac_decode_kernel(const FlacJob J) {
  const int t = (int)(blockIdx.x * kFlacThreads + threadIdx.x);
  if (t >= J.n_frames) return;
  const FlacRec r = J.table[t];
  int32_t e = flac::kHeader;
  if ((int64_t)r.off + r.len <= J.raw_bytes && (int64_t)r.s0 + r.bs <= J.cap_samples && r.bs >= 1) {
    const flac::Stream si{J.rate, J.channels, J.bits};
    const size_t at = (size_t)r.s0 * J.channels;
    if (J.bits <= 16) e = flac::decode_frame(J.raw + r.off, r.len, si, r.bs, J.work + at, (int16_t*)J.out + at, flac::kStoreS16);
    else e = flac::decode_frame(J.raw + r.off, r.len, si, r.bs, J.work + at, (int32_t*)J.out + at, flac::kStoreS32);
  }
  J.status[t] = e;
}

}  // namespace

void launch_ingest(const IngestJob& j, hipStream_t s) {
  if (j.n_out <= 0) return;
  const int64_t need = j.taps ? ingest_span(j.tile, j.up, j.down, j.half) : j.tile;
  if (j.tile < 1 || j.tile > kIngestMaxTile || j.span < need || j.span > kIngestSpanMax || j.channels < 1 || j.channels > 8 ||
      !((j.format >= TTASR_PCM_U8 && j.format <= TTASR_PCM_F64) || j.format == TTASR_PCM_ALAW || j.format == TTASR_PCM_ULAW) ||
      j.pick < -1 || j.pick >= j.channels || j.nf < 0 || (j.taps && (j.up < 1 || j.down < 1 || j.L < 1))) {
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

void launch_wire(const WireJob* jobs, int n, int max_tiles, int span, const uint8_t* raw, float* out, float* hist, hipStream_t s) {
  if (n <= 0) return;
  if (n > 65535 || max_tiles < 0 || span < 1 || span > kWireSpan || !jobs || !raw || !out || !hist) {
    launch_fault("wire: %d rows, %d tiles, span %d", n, max_tiles, span);
    return;
  }
  wire_kernel<<<dim3((unsigned)max_tiles + 1, (unsigned)n), kIngestThreads, (size_t)span * sizeof(float), s>>>(jobs, raw, out, hist);
}

void launch_ima_decode(const ImaJob& j, hipStream_t s) {
  if (j.n_blocks <= 0 || j.n_frames <= 0) return;
  if (j.channels < 1 || j.channels > 8 || j.block_align < 8 * j.channels || j.block_align % (4 * j.channels) ||
      j.spb != ima_spb(j.block_align, j.channels) || ((uintptr_t)j.raw & 3)) {
    launch_fault("ima decode: %d blocks of %d bytes, %d channels, %d samples per block", j.n_blocks, j.block_align, j.channels, j.spb);
    return;
  }
  const int64_t lanes = (int64_t)j.n_blocks * j.channels;
  ima_decode_kernel<<<(unsigned)((lanes + kIngestThreads - 1) / kIngestThreads), kIngestThreads, 0, s>>>(j);
}

void launch_flac_decode(const FlacJob& j, hipStream_t s) {
  if (j.n_frames <= 0) return;
  if (j.channels < 1 || j.channels > 8 || j.bits < 4 || j.bits > 24 || j.raw_bytes < 0 || j.cap_samples < 1 || !j.raw || !j.table ||
      !j.work || !j.out || !j.status || ((uintptr_t)j.table & 3)) {
    launch_fault("flac decode: %d frames, %d channels, %d bits, %lld bytes, %lld samples", j.n_frames, j.channels, j.bits,
                 (long long)j.raw_bytes, (long long)j.cap_samples);
    return;
  }
  flac_decode_kernel<<<(unsigned)((j.n_frames + kFlacThreads - 1) / kFlacThreads), kFlacThreads, 0, s>>>(j);
}
