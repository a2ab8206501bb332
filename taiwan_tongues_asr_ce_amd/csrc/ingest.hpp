// File ingest on the device (include/ttasr.h ttasr_ingest_*): what kernels_ingest.hip and engine_ingest.hip share.  The result is
// defined in the header; DESIGN.md section 4.21 has the kernel's shape and the measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ttasr.h"

constexpr int kIngestThreads = 256;
constexpr int kIngestMaxR = 1024;            // accepted ratios: max(up, down) <= 1024
constexpr int kIngestSpan = 8192;            // floats of LDS a workgroup stages at the usual ratios (32 KiB: four workgroups per CU)
constexpr int kIngestSpanMax = 36864;        // ... and at ratios whose 256-output tile needs more (144 KiB: one workgroup per CU)
constexpr int kIngestMaxTile = 4096;         // outputs per workgroup, at most

// One launch: the outputs [k_begin, k_begin + n_out) of one recording from the frames [f0, f0 + nf) of it that `raw` holds
// (interleaved, in the file's sample format).  Frames outside [0, n_frames) are zeros; a frame inside the recording but outside
// the staged range reads as zero as well (the host never asks for one: the guard keeps a wrong host off foreign memory).
// pick = -1: the mean of the channels; pick = c: channel c as it is.  The formats are the six TTASR_PCM_* sample formats and the
// two G.711 codes; an IMA recording arrives here as the TTASR_PCM_S16 its pre-pass wrote, a FLAC recording as the TTASR_PCM_S16 or
// TTASR_PCM_S32 of its pre-pass.
struct IngestJob {
  const uint8_t* raw;      // device, staged frames
  float* out;              // device, n_out floats
  const float* taps;       // device, phase-major [up][L]; nullptr: no filter (rate 16000), out[k] = mono[k]
  int64_t n_frames, f0, k_begin;
  int32_t nf, n_out, up, down, half, L, channels, format, tile, span;
  int32_t pick = -1;
};

// Staged floats a tile of `tile` outputs reads: floor(tile * down / up) + floor(2 * half / up) + 2.
inline int64_t ingest_span(int64_t tile, int up, int down, int half) { return tile * down / up + 2 * (int64_t)half / up + 2; }

void launch_ingest(const IngestJob& j, hipStream_t s);

// Wire streams (ttasr_vad_stream_push_wire): ONE launch for all rows of a push chunk.  Entry r of the job table, in device memory,
// is row r: the outputs [k_begin, k_begin + n_out) of a stream that had f_old frames before this chunk and brings nf new ones at
// raw + raw_off (whole frames, 8-byte aligned).  Frame i < f_old is hist_in[i - f_old + H] (the stream's last H mono values,
// converted and downmixed), frames below 0 and from f_old + nf on are zeros.  hist_out, when not negative, receives the last H
// mono values after the chunk; hist_in and hist_out are float offsets into the history table and never the same half of it.
struct WireJob {
  const float* taps;       // device, phase-major [up][L]; nullptr: no filter
  int64_t raw_off, f_old, k_begin;
  int32_t nf, n_out, out_off /*floats into the output pool*/, hist_in, hist_out;
  int32_t up, down, half, L, H, tile, channels, format, pick;
};
constexpr int kWireSpan = kIngestSpan;       // a stream rate's tile always fits the usual LDS budget (H <= 255)

// jobs / raw / out / hist: device.  max_tiles = the largest ceil(n_out / tile) of the table, span = the largest staged span of it.
void launch_wire(const WireJob* jobs, int n, int max_tiles, int span, const uint8_t* raw, float* out, float* hist, hipStream_t s);

// The IMA ADPCM pre-pass: `n_blocks` whole blocks of `block_align` bytes at `raw` -> int16 [frames][channels] at `out`, block b's
// sample s at frame b * spb + s; frames from `n_frames` on (the cut of the last block, the end of the scratch) are not written.
struct ImaJob {
  const uint8_t* raw;      // device, 4-byte aligned
  int16_t* out;            // device, n_frames * channels int16
  int64_t n_frames;
  int32_t n_blocks, channels, block_align, spb;
};

inline int ima_spb(int block_align, int channels) { return 1 + 2 * (block_align / channels - 4); }

void launch_ima_decode(const ImaJob& j, hipStream_t s);

// The FLAC pre-pass: one lane per FLAC frame runs flac.hpp's decode body.  Entry t of `table` (device) is frame t of the staged
// range: its bytes are raw[off .. off + len), its samples go to frame s0 .. s0 + bs of `out` - left-justified int16 (bits <= 16)
// or int32 [samples][channels] - through the lane's part of `work` (int32 [channels][bs] at work + s0 * channels), and its status
// word (flac.hpp; 0 = ok) to status[t], an ordinary store.  A table entry that leaves raw_bytes or cap_samples is not decoded.
struct FlacRec { uint32_t off, len, s0, bs; };
struct FlacJob {
  const uint8_t* raw;      // device, the staged frames' bytes
  const FlacRec* table;    // device, n_frames entries
  int32_t* work;           // device, cap_samples * channels int32
  void* out;               // device, cap_samples * channels int16 / int32
  int32_t* status;         // device, n_frames words
  int64_t raw_bytes, cap_samples;
  int32_t n_frames, rate, channels, bits;
};
constexpr int kFlacThreads = 64;             // one wave per workgroup: the frames of a chunk spread over the CUs

void launch_flac_decode(const FlacJob& j, hipStream_t s);
