// libttasr: batched on-device word alignment (ttasr_align_batch / ttasr_session_align): the recurrence step the host DTW
// (ttasr_dtw) and the device DTW (kernels_align.hip) share, the per-sequence geometry the kernels read, and their launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ttasr_detail {

// One cell of the DTW recurrence: the three predecessors in (c0 diagonal, c1 up = previous row, c2 left = previous frame), the
// best of them and the move out.  Ties go to "left", then to "up" - the rule of ttasr_dtw since it exists; host and device
// call THIS function, so for one cost matrix both walk the same path.
__host__ __device__ inline int dtw_step(float c0, float c1, float c2, float* best) {
  if (c0 < c1 && c0 < c2) { *best = c0; return 0; }
  if (c1 < c0 && c1 < c2) { *best = c1; return 1; }
  *best = c2; return 2;
}

// sequence i of a batched alignment pass (device array [n]); rows of the pass are [sequence][position], npos positions each
struct AlignSeq {
  int32_t first_row;   // first token row of the cost matrix
  int32_t rows;        // n_tokens - 1 - first_row rows
  int32_t frames;      // F = max(1, num_frames / 2), capped at the audio window
  int32_t n_tokens;
};

constexpr int kAlignMaxMedfilt = 15;
constexpr size_t kDtwLdsTraceBytes = 150 * 1024;   // the CU has 160 KiB; three diagonals and the launch overhead take the rest

// probs [n_pairs][n_seq * npos][Tk] -> mean and std (std 0 -> 1) over each sequence's token rows, per pair and frame:
// stats [n_seq][n_pairs][2][Tk]
// seq_row != nullptr (the packed pass, here and below): sequence i starts at packed row seq_row[i] of the n_rows rows instead of
// i * npos - in probs, in cost and in start
void launch_align_stats(const float* probs, const AlignSeq* seq, int n_seq, int npos, int n_pairs, int Tk, float* stats, hipStream_t s,
                        const int32_t* seq_row = nullptr, int n_rows = 0);
// normalise, median of `width` along time (reflected edges), mean over pairs, negate: cost [n_seq][npos][Tk], C_i = rows x frames
void launch_align_cost(const float* probs, const float* stats, const AlignSeq* seq, int n_seq, int npos, int max_rows, int n_pairs, int Tk,
                       int width, float* cost, hipStream_t s, const int32_t* seq_row = nullptr, int n_rows = 0);
// words of 2-bit trace one sequence needs
__host__ __device__ inline size_t dtw_trace_words(int rows, int frames) { return (size_t)rows * ((frames + 15) / 16); }
// one workgroup per sequence; start [n_seq][npos]: the frame at which the path first enters each row.  A trace beyond
// kDtwLdsTraceBytes goes to trace_spill [n_seq][spill_words]
void launch_align_dtw(const float* cost, const AlignSeq* seq, int n_seq, int npos, int max_rows, int Tk, size_t lds_trace_words,
                      uint32_t* trace_spill, size_t spill_words, int32_t* start, hipStream_t s, int device,
                      const int32_t* seq_row = nullptr);


}  // namespace ttasr_detail

// the alignment pass over several sequences: rows = n_seq * npos, [sequence][position]; sequence s reads the cross-KV of slot
// seq_clip[s] (device); probs [n_sel][rows][Tk] as launch_cross_attn_probs
template <typename T>
void launch_cross_attn_probs_batch(const T* q, const T* K, const T* V, T* out, int n_seq, int npos, int H, int Tk, const int* sel,
                                   const int* seq_clip, float* probs, hipStream_t s);
