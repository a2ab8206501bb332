// Audio enhancement on the device (include/ttasr.h ttasr_enhance*): what kernels_enhance.hip and engine_enhance.hip share.  The
// result is defined in the header; DESIGN.md section 4.35 has the kernels' shape and the measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ttasr.h"

constexpr int kEnhN = 512;            // frame length
constexpr int kEnhHop = 128;          // hop: every sample lies in four frames
constexpr int kEnhBins = 257;
constexpr int kEnhRS = 2;             // radius of the box mean S (drives the gain)
constexpr int kEnhRQ = 16;            // radius of the box mean Q (drives the noise tracker)
constexpr int kEnhBlock = 32;         // frames of one block minimum
constexpr int kEnhBlockWin = 6;       // blocks on either side of a frame's block the floor looks at
constexpr int kEnhThreads = 256;
constexpr int kEnhTileHops = 8;       // hops of output one synthesis workgroup owns
constexpr int kEnhTile = kEnhTileHops * kEnhHop;
constexpr int kEnhMaxSpan = 4096;     // samples one workgroup of the maximum reduction reads
constexpr int64_t kEnhMaxSamples = (int64_t)1 << 36;

__host__ __device__ inline int64_t enh_frames(int64_t L) { return (L + kEnhHop - 1) / kEnhHop + 3; }
__host__ __device__ inline int64_t enh_blocks(int64_t T) { return (T + kEnhBlock - 1) / kEnhBlock; }
// samples of a recording that must be on the device before block b's minima can be taken: frame 32 b + 47 ends here
inline int64_t enh_block_need(int64_t b) { return (b * kEnhBlock + kEnhBlock - 1 + kEnhRQ) * kEnhHop - 384 + kEnhN; }

// One recording on the device.  x [L] f32 (L >= kEnhN), M [NB][257] block minima of Q, tw [512] (cos, sin)(2 pi m / 512) and
// win [512] the sine window, both rounded from double.
struct EnhRec {
  const float* x;
  float* M;
  const float2* tw;
  const float* win;
  int64_t L;
};
// flags: TTASR_DSP_*; floor_gain = 10^(-strength_db / 20) rounded from double
struct EnhGain { float oversubtract, floor_gain; int32_t flags; };
// optional outputs of the gain pass (ttasr_enhance_probe): [T][257] each, nullptr = not wanted
struct EnhTaps { float *S, *Nf, *G; };

// block minima M[b] for b in [b0, b1)
void launch_enh_noise(const EnhRec& r, int64_t b0, int64_t b1, hipStream_t s);
// out[s] for s in [s0, s1), 0 <= s0 < s1 <= L: gain and synthesis before the level stage
void launch_enh_gain(const EnhRec& r, const EnhGain& g, const EnhTaps& taps, float* out, int64_t s0, int64_t s1, hipStream_t s);
// partial[i] = max |v[s]| over the i-th span of kEnhMaxSpan samples of [s0, s1); returns the number of spans
int64_t launch_enh_absmax(const float* v, int64_t s0, int64_t s1, float* partial, hipStream_t s);
// *gain = 1 if the maximum of the partials is 0, else min(peak_target / maximum, max_gain)
void launch_enh_level(const float* partial, int64_t n_partial, float peak_target, float max_gain, float* gain, hipStream_t s);
// v[s] *= *gain for s in [s0, s1)
void launch_enh_scale(float* v, int64_t s0, int64_t s1, const float* gain, hipStream_t s);
