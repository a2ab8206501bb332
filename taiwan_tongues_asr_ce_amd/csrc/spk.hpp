// Speaker-embedding network (XVectorSincNet shape: SincNet front end, five TDNN blocks, weighted statistics pooling, one Linear):
// what kernels_spk.hip and engine_spk.hip share.  The network is the text of include/ttasr.h (ttasr_spk_*); DESIGN.md section
// 4.32 has the kernels and the measurements.  The front end is kernels_seg.hip's (seg.hpp launch_seg_frontend) with this
// network's weights.
#pragma once
#include "seg.hpp"

constexpr int kSpkGroup = TTASR_SPK_GROUP;     // chunks of one pass through the kernels
constexpr int kSpkMaxMasks = TTASR_SPK_MAX_MASKS;
constexpr int kSpkMaxDim = TTASR_SPK_MAX_DIM;
constexpr int kSpkLayers = 5;
constexpr int kSpkHid = 512, kSpkOut = 1500;   // channels of blocks 1-4 and of block 5
constexpr int kSpkStats = 2 * kSpkOut;         // [mean | std]
constexpr int kSpkCin[kSpkLayers] = {kSegC2, kSpkHid, kSpkHid, kSpkHid, kSpkHid};
constexpr int kSpkCout[kSpkLayers] = {kSpkHid, kSpkHid, kSpkHid, kSpkHid, kSpkOut};
constexpr int kSpkTaps[kSpkLayers] = {5, 3, 3, 1, 1};
constexpr int kSpkDil[kSpkLayers] = {1, 2, 3, 1, 1};
constexpr int kSpkFrames[kSpkLayers + 1] = {kSegT, 289, 285, 279, 279, 279};   // frames in front of block l and behind the last
constexpr int kSpkT = 279;                     // frames the pooling sees
constexpr int kSpkRows = 289;                  // rows of a ping-pong buffer: the most frames a 512-channel block writes

// Device weights, f32, in the layouts the kernels read
struct SpkWeights {
  SegWeights front;                            // the front end's share (only the sincnet.* members are set)
  const float* wt[kSpkLayers];                 // [taps * cin][cout]   wt[j * cin + c][o] = tdnns.{0,3,6,9,12}.weight[o][c][j]
  const float* bias[kSpkLayers];               // [cout]
  const float* bn_mean[kSpkLayers];            // [cout]               running_mean
  const float* bn_scale[kSpkLayers];           // [cout]               weight / sqrt(running_var + 1e-5), float64 rounded once
  const float* bn_beta[kSpkLayers];            // [cout]               bias of the BatchNorm
  const float* emb_t;                          // [3000][ldd]          emb_t[k][o] = embedding.weight[o][k], ldd = dim rounded up to 4
  const float* emb_b;                          // [dim]
  int dim, ldd;
};

// The scratch block of a group of n <= kSpkGroup chunks with S masks each (all device memory)
struct SpkBuffers {
  SegBuffers front;      // pcm, desc, st0, a1, st1, a2, st2, a3, st3 (the other members stay null)
  float* h[2];           // [n][289][512]     outputs of blocks 1-4, ping-pong (a chunk's rows are 289 * 512 floats apart)
  float* h5;             // [n][279][1500]    output of block 5
  const float* masks;    // [n][S][293]       the caller's frame weights
  int32_t* valid;        // [n * S]           1 where the resampled weights sum to more than 0
  float* stats;          // [n * S][3000]     mean | std; quiet NaN in the rows of a zero-sum mask
  float* emb;            // [n * S][dim]
};

// n chunks with S masks each through the front end, the TDNN blocks (once per chunk), the pooling (once per mask) and the Linear
void launch_spk_network(const SpkWeights& w, const SpkBuffers& b, int n, int S, hipStream_t s);
