// Segmentation VAD network (PyanNet shape: SincNet front end, 4-layer bidirectional LSTM, linear head): what kernels_seg.hip and
// engine_seg.hip share.  The network is the text of include/ttasr.h (ttasr_seg_*); DESIGN.md section 4.30 has the launch
// geometry and the measurements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ttasr.h"

constexpr int kSegGroup = TTASR_SEG_GROUP;    // chunks of one pass through the kernels
constexpr int kSegChunk = 80000;              // samples of a chunk
constexpr int kSegStep = 8000;                // samples between two chunk starts
constexpr int kSegTaps = 251, kSegStride = 10, kSegC1 = 80, kSegC2 = 60;
constexpr int kSegL1 = 2658, kSegL2 = 884;    // pooled lengths of the first two stages
constexpr int kSegT = 293;                    // frames of a chunk (pooled length of the third stage)
constexpr int kSegHid = 128, kSegLayers = 4;
constexpr int kSegMaxC = 8;                   // classes
constexpr int kSegCarry = 10;                 // chunks in front of a group whose frames can still overlap the group's (293 * 270 < 10 * 8000)
constexpr int kSegAggRow = kSegT + 33;        // output frames one chunk of a group can complete at most: s(k + 1) - s(k) <= 30, + a recording's last 293

// A chunk of the group: its samples are pcm[off .. off + nvalid), zeros behind (nvalid in [1, 80000])
struct SegDesc { int32_t off, nvalid; };

// One recording's share of a group's aggregation: output frames [j0, j1) from the chunks [kmin, kmax), whose speech scores are the
// rows row0 ... of the score table (row0 counts from the first carry row); the frames go to agg_out[out_off ...]
struct SegAggJob { int64_t kmin, kmax, j0, j1; int32_t row0, out_off; };

// Device weights, f32, in the layouts the kernels read (engine_seg.hip transposes at load time so that a wave's lanes, or a
// thread's consecutive channels, read consecutive addresses).
struct SegWeights {
  const float* wav_w; const float* wav_b;     // [1]
  const float* sinc_t;                        // [251][80]          sinc_t[k][c]            = sincnet.conv1d.0.filters[c][0][k]
  const float* norm_w[3]; const float* norm_b[3];   // [80] [60] [60]
  const float* conv_t[2];                     // [cin * 5][60]      conv_t[c * 5 + j][o]    = sincnet.conv1d.{1,2}.weight[o][c][j]
  const float* conv_b[2];                     // [60]
  const float* wih_t[kSegLayers];             // [in][1024]         wih_t[k][d * 512 + r]   = lstm.weight_ih_l{l}[_reverse][r][k]
  const float* gate_b[kSegLayers];            // [1024]             bias_ih + bias_hh (one f32 addition, at ttasr_seg_finalize)
  const float* whh[kSegLayers][2];            // [512][128]         as given: one row per thread, read once per launch
  const float* lin_t[2]; const float* lin_b[2];     // [256][128], [128][128]: lin_t[k][j] = linear.{0,1}.weight[j][k]
  const float* cls_w; const float* cls_b;     // [C][128], [C]
  int classes;
};

// The scratch block of a group of n <= kSegGroup chunks (all device memory)
struct SegBuffers {
  const float* pcm; const SegDesc* desc;
  float* st0;            // [n][2]            mean, 1 / sqrt(var + eps) of the chunk
  float* a1; float* st1; // [n][80][2658]     pooled |sinc|, before its norm;   [n][80][2]
  float* a2; float* st2; // [n][60][884]                                         [n][60][2]
  float* a3; float* st3; // [n][60][293]                                         [n][60][2]
  float* gx;             // [n][2][293][512]  the hoisted input projection of the running layer, both directions
  float* y[2];           // [n][293][256]     a layer's output forward | backward (ping-pong)
  float* probs; float* logits;   // [n][293][C]
  float* score;          // [kSegCarry + n][293]  max over classes; the first kSegCarry rows: the chunks in front of the group
  const SegAggJob* jobs; const float* window; float* agg_out;
};

// n chunks through the front end alone (waveform norm, sinc stage, two conv stages and the statistics of the third): a3 and st3
// are its results; the third InstanceNorm and leaky_relu are applied by whoever reads them.  The first launches of
// launch_seg_network, and the front end of the speaker-embedding network (kernels_spk.hip) with that network's weights.
void launch_seg_frontend(const SegWeights& w, const SegBuffers& b, int n, hipStream_t s);
// n chunks through the front end, the LSTM (rows = chunks per recurrence workgroup: 1, 2 or 4) and the head
void launch_seg_network(const SegWeights& w, const SegBuffers& b, int n, int rows, hipStream_t s);
// n_jobs aggregation jobs, the longest of max_frames output frames
void launch_seg_aggregate(const SegBuffers& b, int n_jobs, int64_t max_frames, hipStream_t s);
