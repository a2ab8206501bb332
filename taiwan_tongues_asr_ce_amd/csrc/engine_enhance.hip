// libttasr: audio enhancement behind the C ABI (one of the engine translation units, see engine_ctx.hpp): the tables in double, the
// context's device block and the chunk loops of ttasr_enhance / ttasr_enhance_probe.  The kernels are kernels_enhance.hip; the
// result is the text of include/ttasr.h.  Nothing here touches mel, encoder, search or graph state, and no model weights are
// needed: the call's only shared resource is the context's stream.
#include "engine_ctx.hpp"
#include "enhance.hpp"

namespace ttasr_detail {

constexpr int64_t kEnhDefaultChunk = (int64_t)1 << 22;   // samples per chunk when option enhance_chunk is 0

struct EnhState {
  DevBlock<> dev;   // tables | gain | partial maxima | block minima | samples | result | the probe's S, Nf, G
};

void enhance_free(ttasr_ctx* c) {
  delete c->enhance;
  c->enhance = nullptr;
}

namespace {

// (cos, sin)(2 pi m / 512) and the sine window, rounded from double
struct EnhHostTables { float tw[2 * kEnhN]; float win[kEnhN]; };
const EnhHostTables& enh_host_tables() {
  static const EnhHostTables t = [] {
    EnhHostTables h;
    const double pi = 3.14159265358979323846;
    for (int m = 0; m < kEnhN; ++m) {
      h.tw[2 * m] = (float)std::cos(2 * pi * m / kEnhN);
      h.tw[2 * m + 1] = (float)std::sin(2 * pi * m / kEnhN);
      h.win[m] = (float)std::sin(pi * (m + 0.5) / kEnhN);
    }
    // the quarter points exactly: bin 0 has no sine part, bin 256's cosine is (-1)^n
    h.tw[1] = 0.0f; h.tw[2 * 256 + 1] = 0.0f; h.tw[2 * 128] = 0.0f; h.tw[2 * 384] = 0.0f;
    return h;
  }();
  return t;
}

int64_t enh_chunk(const ttasr_ctx* c) { return c->enhance_chunk > 0 ? c->enhance_chunk : kEnhDefaultChunk; }

// The block carved for recordings of at most Lmax samples in chunks of C; taps: room for the probe's three [T][257] outputs.
struct EnhLayout {
  size_t tw, win, gain, partial, M, x, out, S, Nf, G, bytes;
  EnhLayout(int64_t Lmax, int64_t C, bool taps) {
    const int64_t T = enh_frames(Lmax), NB = enh_blocks(T), chunks = (Lmax + C - 1) / C;
    Carve k;
    tw = k.take(sizeof(float) * 2 * kEnhN); win = k.take(sizeof(float) * kEnhN); gain = k.take(sizeof(float));
    partial = k.take(sizeof(float) * (size_t)(Lmax / kEnhMaxSpan + chunks + 1));
    M = k.take(sizeof(float) * (size_t)NB * kEnhBins);
    x = k.take(sizeof(float) * (size_t)Lmax); out = k.take(sizeof(float) * (size_t)Lmax);
    const size_t plane = taps ? sizeof(float) * (size_t)T * kEnhBins : 0;
    S = k.take(plane); Nf = k.take(plane); G = k.take(plane);
    bytes = k.used;
  }
};

int enh_check_params(ttasr_ctx* c, const ttasr_dsp_params* p) {
  if (!p) return fail(c, TTASR_E_INVALID, "params is NULL");
  const int32_t all = TTASR_DSP_DENOISE | TTASR_DSP_HIGHPASS | TTASR_DSP_LEVEL;
  if (p->flags == 0 || (p->flags & ~all)) return fail(c, TTASR_E_INVALID, "flags %d: at least one of DENOISE (1), HIGHPASS (2), LEVEL (4) and no other bit", p->flags);
  if (!std::isfinite(p->strength_db) || !std::isfinite(p->oversubtract) || !std::isfinite(p->peak_target) || !std::isfinite(p->max_gain))
    return fail(c, TTASR_E_INVALID, "a parameter is not finite");
  if (p->strength_db < 0.0f || p->strength_db > 40.0f) return fail(c, TTASR_E_INVALID, "strength_db %g outside [0, 40]", p->strength_db);
  if (!(p->oversubtract > 0.0f) || p->oversubtract > 16.0f) return fail(c, TTASR_E_INVALID, "oversubtract %g outside (0, 16]", p->oversubtract);
  if (!(p->peak_target > 0.0f) || p->peak_target > 1.0f) return fail(c, TTASR_E_INVALID, "peak_target %g outside (0, 1]", p->peak_target);
  if (p->max_gain < 1.0f) return fail(c, TTASR_E_INVALID, "max_gain %g is below 1", p->max_gain);
  return 0;
}

int enh_check_len(ttasr_ctx* c, int i, int64_t L) {
  if (L < 0 || L > kEnhMaxSamples) return fail(c, TTASR_E_INVALID, "recording %d: %lld samples outside [0, 2^36]", i, (long long)L);
  return 0;
}

// The block for this call and its tables
int enh_prepare(ttasr_ctx* c, const EnhLayout& lay) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->enhance) c->enhance = new EnhState();
  TRY(c->enhance->dev.ensure(c, lay.bytes, "enhancement block"));
  char* const d = c->enhance->dev;
  const EnhHostTables& h = enh_host_tables();
  HIPCHK(c, hipMemcpyAsync(d + lay.tw, h.tw, sizeof h.tw, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + lay.win, h.win, sizeof h.win, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// One recording of L > 0 samples through the launchers, everything enqueued on the context's stream: the samples go up chunk by
// chunk, the result before the level stage stands in the block's `out` region afterwards.  taps: device pointers or NULL.
int enh_run(ttasr_ctx* c, const EnhLayout& lay, const float* x_host, int64_t L, const ttasr_dsp_params& p, bool noise, const EnhTaps& taps) {
  hipStream_t s = c->stream;
  char* const d = c->enhance->dev;
  const int64_t C = enh_chunk(c);
  float* const d_x = (float*)(d + lay.x);
  float* const d_out = (float*)(d + lay.out);
  if (L < kEnhN) {   // no frame: out = x
    HIPCHK(c, hipMemcpyAsync(d_out, x_host, (size_t)L * 4, hipMemcpyHostToDevice, s));
    return 0;
  }
  EnhRec r;
  r.x = d_x; r.M = (float*)(d + lay.M); r.tw = (const float2*)(d + lay.tw); r.win = (const float*)(d + lay.win); r.L = L;
  const int64_t NB = enh_blocks(enh_frames(L));
  int64_t b_next = 0;
  for (int64_t a = 0; a < L; a += C) {
    const int64_t e = std::min(a + C, L);
    HIPCHK(c, hipMemcpyAsync(d_x + a, x_host + a, (size_t)(e - a) * 4, hipMemcpyHostToDevice, s));
    if (!noise) continue;
    int64_t b_hi = b_next;   // the blocks whose last sample has arrived; all that are left with the last chunk
    if (e == L) b_hi = NB;
    else while (b_hi < NB && enh_block_need(b_hi) <= e) ++b_hi;
    launch_enh_noise(r, b_next, b_hi, s);
    b_next = b_hi;
  }
  EnhGain g;
  g.oversubtract = p.oversubtract; g.floor_gain = (float)std::pow(10.0, -(double)p.strength_db / 20.0); g.flags = p.flags;
  for (int64_t a = 0; a < L; a += C) launch_enh_gain(r, g, taps, d_out, a, std::min(a + C, L), s);
  return 0;
}

}  // namespace

}  // namespace ttasr_detail

extern "C" {

int64_t ttasr_enhance_frames(int64_t n_samples) {
  if (n_samples < 0 || n_samples > kEnhMaxSamples) return TTASR_E_INVALID;
  return n_samples < kEnhN ? 0 : enh_frames(n_samples);
}

int ttasr_enhance(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* n_samples, const ttasr_dsp_params* params,
                  float* const* out_pcm, float* out_gain) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (n < 0) return fail(c, TTASR_E_INVALID, "n %d is negative", n);
  TRY(enh_check_params(c, params));
  if (n == 0) return TTASR_OK;
  if (!pcm || !n_samples || !out_pcm) return fail(c, TTASR_E_INVALID, "NULL argument");
  int64_t Lmax = 0;
  for (int i = 0; i < n; ++i) {
    TRY(enh_check_len(c, i, n_samples[i]));
    if (n_samples[i] > 0 && (!pcm[i] || !out_pcm[i])) return fail(c, TTASR_E_INVALID, "recording %d: NULL sample or output row with %lld samples", i, (long long)n_samples[i]);
    Lmax = std::max(Lmax, n_samples[i]);
  }
  TRY(session_refusal(c));
  if (out_gain) for (int i = 0; i < n; ++i) out_gain[i] = 1.0f;
  if (Lmax == 0) return TTASR_OK;
  const int64_t C = enh_chunk(c);
  const EnhLayout lay(Lmax, C, false);
  TRY(enh_prepare(c, lay));
  hipStream_t s = c->stream;
  char* const d = c->enhance->dev;
  float* const d_out = (float*)(d + lay.out);
  float* const d_gain = (float*)(d + lay.gain);
  float* const d_partial = (float*)(d + lay.partial);
  const bool level = (params->flags & TTASR_DSP_LEVEL) != 0, noise = (params->flags & TTASR_DSP_DENOISE) != 0;
  for (int i = 0; i < n; ++i) {
    const int64_t L = n_samples[i];
    if (L == 0) continue;
    TRY(enh_run(c, lay, pcm[i], L, *params, noise, EnhTaps{nullptr, nullptr, nullptr}));
    if (level) {
      int64_t np = 0;
      for (int64_t a = 0; a < L; a += C) np += launch_enh_absmax(d_out, a, std::min(a + C, L), d_partial + np, s);
      launch_enh_level(d_partial, np, params->peak_target, params->max_gain, d_gain, s);
    }
    for (int64_t a = 0; a < L; a += C) {
      const int64_t e = std::min(a + C, L);
      if (level) launch_enh_scale(d_out, a, e, d_gain, s);
      HIPCHK(c, hipMemcpyAsync(out_pcm[i] + a, d_out + a, (size_t)(e - a) * 4, hipMemcpyDeviceToHost, s));
    }
    if (level && out_gain) HIPCHK(c, hipMemcpyAsync(out_gain + i, d_gain, 4, hipMemcpyDeviceToHost, s));
    // the next recording's samples overwrite the block: the copies into the caller's pageable rows have to be over
    HIPCHK(c, hipStreamSynchronize(s));
  }
  HIPCHK(c, hipGetLastError());
  return TTASR_OK;
  });
}

int ttasr_enhance_probe(ttasr_ctx* c, const float* pcm, int64_t n_samples, const ttasr_dsp_params* params, float* out_S, float* out_Nf,
                        float* out_G, float* out_pcm) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(enh_check_params(c, params));
  TRY(enh_check_len(c, 0, n_samples));
  if (n_samples > 0 && !pcm) return fail(c, TTASR_E_INVALID, "NULL sample row with %lld samples", (long long)n_samples);
  TRY(session_refusal(c));
  if (n_samples == 0) return TTASR_OK;
  const int64_t L = n_samples, T = enh_frames(L);
  const bool frames = L >= kEnhN;
  const EnhLayout lay(L, enh_chunk(c), frames);
  TRY(enh_prepare(c, lay));
  hipStream_t s = c->stream;
  char* const d = c->enhance->dev;
  EnhTaps taps{nullptr, nullptr, nullptr};
  if (frames) taps = EnhTaps{(float*)(d + lay.S), (float*)(d + lay.Nf), (float*)(d + lay.G)};
  TRY(enh_run(c, lay, pcm, L, *params, frames, taps));
  const size_t plane = (size_t)T * kEnhBins * 4;
  if (frames && out_S) HIPCHK(c, hipMemcpyAsync(out_S, taps.S, plane, hipMemcpyDeviceToHost, s));
  if (frames && out_Nf) HIPCHK(c, hipMemcpyAsync(out_Nf, taps.Nf, plane, hipMemcpyDeviceToHost, s));
  if (frames && out_G) HIPCHK(c, hipMemcpyAsync(out_G, taps.G, plane, hipMemcpyDeviceToHost, s));
  if (out_pcm) HIPCHK(c, hipMemcpyAsync(out_pcm, d + lay.out, (size_t)L * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  return TTASR_OK;
  });
}

}  // extern "C"
