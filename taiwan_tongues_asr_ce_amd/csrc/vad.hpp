// Voice-activity network (Silero-v5 shape, 16 kHz branch): what kernels_vad.hip and engine_vad.hip share.  The network is the
// text of include/ttasr.h (ttasr_vad_*); DESIGN.md section 4.20 has the launch geometry and the measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ttasr.h"

constexpr int kVadWindow = 512;                           // samples per frame
constexpr int kVadContext = 64;                           // samples of the previous frame in front of it
constexpr int kVadChunk = TTASR_VAD_CHUNK_FRAMES;         // frames of one recording per time chunk
constexpr int kVadSlot = kVadContext + kVadWindow * kVadChunk;   // staged floats of one recording's chunk: context | frames
constexpr int kVadTile = 8;                               // frames per workgroup of the frame-parallel kernel
static_assert(kVadChunk % kVadTile == 0, "a chunk is a whole number of frame tiles");

// Device weights, f32, in the layouts the kernels read (engine_vad.hip transposes at load time so that the lanes of a wave,
// which own consecutive output channels, read consecutive addresses).
struct VadWeights {
  const float* basis_t;     // [256][258]        basis_t[m][k]         = stft.forward_basis_buffer[k][0][m]
  const float* conv_t[4];   // [cin * 3][cout]   conv_t[c * 3 + j][o]  = encoder.l.reparam_conv.weight[o][c][j]
  const float* conv_b[4];   // [cout]
  const float* wih_t;       // [128][512]        wih_t[k][r]           = decoder.rnn.weight_ih[r][k]
  const float* gate_b;      // [512]             bias_ih + bias_hh (one f32 addition, at ttasr_vad_finalize)
  const float* whh;         // [512][128]        decoder.rnn.weight_hh as given: one row per thread, read once per launch
  const float* w_out;       // [128]             decoder.decoder.2.weight
  const float* b_out;       // [1]
};

// One time chunk of n recordings.  pcm [n][kVadSlot] staged samples; nf [n] frames of recording i in this chunk (0 ... kVadChunk);
// gx [n][kVadChunk][512] the hoisted input projection; state [...][256] h | c, carried from chunk to chunk (and, for a stream,
// from call to call); slot [n] (device memory) the state row of each row of the call - distinct, inside the state table - or
// nullptr for row i -> state row i; out [n][2][kVadChunk] logits | probabilities.  max_nf = the largest nf (host copy): sizes the
// frame kernel's grid only.
void launch_vad_frames(const VadWeights& w, const float* pcm, const int32_t* nf, float* gx, int n, int max_nf, hipStream_t s);
void launch_vad_lstm(const VadWeights& w, const float* gx, const int32_t* nf, float* state, const int32_t* slot, float* out, int n,
                     hipStream_t s);
