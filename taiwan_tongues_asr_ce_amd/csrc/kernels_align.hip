// Batched word alignment on the device (ttasr_align_batch / ttasr_session_align), behind the teacher-forced pass: what
// alignment.token_start_times does on the host for one sequence - per-head normalisation over the token rows, median filter
// along time, mean over heads, negate, DTW, first frame of every row - for n sequences, so that only [n][max_tokens] start
// frames cross to the host instead of the n_pairs x n_tokens x 1500 softmax maps.
//   align_stats_kernel   mean and std (0 -> 1) over a sequence's token rows, per (pair, frame): threads along frames (coalesced)
//   align_cost_kernel    one workgroup per (sequence, row): per pair the normalised row is staged in LDS, every thread takes the
//                        median of its frame's window from there; the pairs' medians are averaged and negated
//   align_dtw_kernel     one workgroup per sequence, one thread per row, one barrier per anti-diagonal (below)
// Rows of a sequence: the padded pass has sequence i at rows i * npos ..; the packed pass (option align_packed) hands seq_row
// [n_seq], every sequence's first packed row, and the cost rows and start frames then sit at the packed rows too.  The
// arithmetic does not know which: equal maps give equal cost matrices and paths.
#include <mutex>

#include "align_batch.hpp"
#include "common.hpp"

namespace ttasr_detail {

// Sums run in double: a column holds up to 447 positive softmax values, and the sequential f32 sum of the host code is the
// largest term of ITS error against exact arithmetic; the loads, not the adds, bound this kernel.
__global__ __launch_bounds__(256) void align_stats_kernel(const float* __restrict__ probs, const AlignSeq* __restrict__ seq, int npos,
                                                          int n_pairs, int Tk, int64_t pair_stride, float* __restrict__ stats,
                                                          const int32_t* __restrict__ seq_row) {
  const int i = blockIdx.z, p = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
  const AlignSeq sq = seq[i];
  if (f >= sq.frames) return;
  const int64_t base = seq_row ? seq_row[i] : (int64_t)i * npos;
  const float* col = probs + (int64_t)p * pair_stride + (base + sq.first_row) * Tk + f;
  double sum = 0.0;
  for (int r = 0; r < sq.rows; ++r) sum += (double)col[(int64_t)r * Tk];
  const float mean = (float)(sum / sq.rows);
  double var = 0.0;
  for (int r = 0; r < sq.rows; ++r) {
    const float dv = col[(int64_t)r * Tk] - mean;   // the f32 deviation the normalisation uses too
    var += (double)dv * (double)dv;
  }
  const float sd = (float)sqrt(var / sq.rows);
  float* out = stats + ((int64_t)i * n_pairs + p) * 2 * Tk;
  out[f] = mean;
  out[Tk + f] = sd > 0.f ? sd : 1.f;
}

void launch_align_stats(const float* probs, const AlignSeq* seq, int n_seq, int npos, int n_pairs, int Tk, float* stats, hipStream_t s,
                        const int32_t* seq_row, int n_rows) {
  hipLaunchKernelGGL(align_stats_kernel, dim3((Tk + 255) / 256, n_pairs, n_seq), dim3(256), 0, s, probs, seq, npos, n_pairs, Tk,
                     (int64_t)(seq_row ? n_rows : n_seq * npos) * Tk, stats, seq_row);
}

__global__ __launch_bounds__(256) void align_cost_kernel(const float* __restrict__ probs, const float* __restrict__ stats,
                                                         const AlignSeq* __restrict__ seq, int npos, int n_pairs, int Tk,
                                                         int64_t pair_stride, int width, float* __restrict__ cost,
                                                         const int32_t* __restrict__ seq_row) {
  extern __shared__ float z[];   // [frames] one pair's normalised row
  const int i = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
  const AlignSeq sq = seq[i];
  if (r >= sq.rows) return;
  const int64_t base = seq_row ? seq_row[i] : (int64_t)i * npos;
  const int F = sq.frames, pad = width / 2;
  const bool filter = width > 1 && F > pad;   // numpy's median_filter is a no-op on an axis no longer than the padding
  constexpr int NF = 6;                       // frames per thread: 6 x 256 >= the 1500-frame window
  double acc[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) acc[k] = 0.0;
  for (int p = 0; p < n_pairs; ++p) {
    const float* row = probs + (int64_t)p * pair_stride + (base + sq.first_row + r) * Tk;
    const float* st = stats + ((int64_t)i * n_pairs + p) * 2 * Tk;
    for (int f = tid; f < F; f += 256) z[f] = (row[f] - st[f]) / st[Tk + f];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int f = tid + k * 256;
      if (f >= F) continue;
      float m = z[f];
      if (filter) {
        float v[kAlignMaxMedfilt];
#pragma unroll
        for (int w = 0; w < kAlignMaxMedfilt; ++w) {
          int g = f + w - pad;
          g = g < 0 ? -g : (g >= F ? 2 * (F - 1) - g : g);      // reflected, the edge sample not repeated
          v[w] = w < width ? z[g] : INFINITY;                    // unused slots sort to the end
        }
#pragma unroll
        for (int a = 1; a < kAlignMaxMedfilt; ++a)
#pragma unroll
          for (int b = a; b > 0; --b) {
            const float lo = fminf(v[b - 1], v[b]), hi = fmaxf(v[b - 1], v[b]);
            v[b - 1] = lo; v[b] = hi;
          }
        m = v[0];
#pragma unroll
        for (int w = 1; w < kAlignMaxMedfilt; ++w) m = w == pad ? v[w] : m;
      }
      acc[k] += (double)m;
    }
    __syncthreads();
  }
  float* out = cost + (base + r) * Tk;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int f = tid + k * 256;
    if (f < F) out[f] = -(float)(acc[k] / n_pairs);
  }
}

void launch_align_cost(const float* probs, const float* stats, const AlignSeq* seq, int n_seq, int npos, int max_rows, int n_pairs, int Tk,
                       int width, float* cost, hipStream_t s, const int32_t* seq_row, int n_rows) {
  if (Tk > 6 * 256) { launch_fault("align_cost: %d frames > 1536", Tk); return; }
  hipLaunchKernelGGL(align_cost_kernel, dim3(max_rows, n_seq), dim3(256), (size_t)Tk * 4, s, probs, stats, seq, npos, n_pairs, Tk,
                     (int64_t)(seq_row ? n_rows : n_seq * npos) * Tk, width, cost, seq_row);
}

// DTW over C [rows][F] of one sequence.  Thread i owns row i and walks it one frame per anti-diagonal k = i + j: the cells of a
// diagonal are independent, the left predecessor is the thread's own previous value (a register), the upper and the diagonal
// one are row i - 1's values of the diagonals k - 1 and k - 2, exchanged through three rotating LDS rows - so ONE barrier per
// diagonal orders everything (the row written at k + 1 is the one last read at k).  Arithmetic and tie rule are dtw_step's, the
// boundary is ttasr_dtw's (acc = +inf outside the matrix, 0 at the corner).  The move of every cell is kept as 2 bits, 16 frames
// of a row per word, words of one frame block adjacent over the rows (conflict-free stores); thread 0 walks the path back from
// (rows - 1, F - 1) and leaves in start[i] the last - that is the lowest - frame it sees in row i.  rows + F - 1 dependent
// barriers of <= 8 waves: the kernel is latency-bound by construction, and independent sequences run on other CUs.
__global__ __launch_bounds__(512) void align_dtw_kernel(const float* __restrict__ cost, const AlignSeq* __restrict__ seq, int npos, int Tk,
                                                        size_t lds_trace_words, uint32_t* __restrict__ trace_spill, size_t spill_words,
                                                        int32_t* __restrict__ start, const int32_t* __restrict__ seq_row) {
  extern __shared__ float lds[];   // [3][blockDim] diagonals, then the trace words
  const int s = blockIdx.x, i = threadIdx.x, nt = blockDim.x;
  const AlignSeq sq = seq[s];
  const int rows = sq.rows, F = sq.frames;
  const int64_t base = seq_row ? seq_row[s] : (int64_t)s * npos;
  uint32_t* trace = dtw_trace_words(rows, F) <= lds_trace_words ? (uint32_t*)(lds + 3 * nt) : trace_spill + (size_t)s * spill_words;
  const float* crow = cost + (base + min(i, rows - 1)) * Tk;
  const bool mine = i < rows;
  float left = INFINITY, cnext = crow[0];
  uint32_t tw = 0;
  const int n_diag = rows + F - 1;
  for (int k = 0; k < n_diag; ++k) {
    const int j = k - i;
    float* cur = lds + (k % 3) * nt;
    if (mine && j >= 0 && j < F) {
      const float* up_row = lds + ((k + 2) % 3) * nt;   // diagonal k - 1
      const float* dg_row = lds + ((k + 1) % 3) * nt;   // diagonal k - 2
      const float c = cnext;
      cnext = crow[min(j + 1, F - 1)];                  // the next cell's cost is in flight over the barrier
      const float c1 = i == 0 ? INFINITY : up_row[i - 1];
      const float c0 = i == 0 ? (j == 0 ? 0.f : INFINITY) : (j == 0 ? INFINITY : dg_row[i - 1]);
      float best;
      const int t = dtw_step(c0, c1, left, &best);
      left = c + best;
      cur[i] = left;
      tw |= (uint32_t)t << (2 * (j & 15));
      if ((j & 15) == 15 || j == F - 1) { trace[(size_t)(j >> 4) * rows + i] = tw; tw = 0; }
    }
    __syncthreads();
  }
  if (i != 0) return;
  int32_t* out = start + base;
  int r = rows - 1, j = F - 1;
  while (r >= 0 && j >= 0) {
    out[r] = j;
    const int t = (trace[(size_t)(j >> 4) * rows + r] >> (2 * (j & 15))) & 3;
    if (t == 0) { --r; --j; } else if (t == 1) --r; else --j;
  }
}

void launch_align_dtw(const float* cost, const AlignSeq* seq, int n_seq, int npos, int max_rows, int Tk, size_t lds_trace_words,
                      uint32_t* trace_spill, size_t spill_words, int32_t* start, hipStream_t s, int device, const int32_t* seq_row) {
  if (max_rows < 1 || max_rows > 512) { launch_fault("align_dtw: %d rows outside [1, 512]", max_rows); return; }
  static std::once_flag once[64];
  std::call_once(once[device & 63], []() {
    (void)hipFuncSetAttribute((const void*)align_dtw_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  const int nt = (max_rows + 63) / 64 * 64;
  const size_t lds = (size_t)3 * nt * 4 + lds_trace_words * 4;
  hipLaunchKernelGGL(align_dtw_kernel, dim3(n_seq), dim3(nt), lds, s, cost, seq, npos, Tk, lds_trace_words, trace_spill, spill_words,
                     start, seq_row);
}

}  // namespace ttasr_detail
