// libttasr: the speaker-embedding network behind the C ABI (one of the engine translation units, see engine_ctx.hpp): weight intake
// into the kernels' layouts, the context's scratch block and pinned staging, and the group loop of ttasr_spk_embed.  The kernels
// are kernels_spk.hip (and the front end of kernels_seg.hip); the network is the text of include/ttasr.h.  Nothing here touches
// mel, encoder, search, graph, session, Silero or segmentation state: the call's only shared resource is the context's stream.
#include "engine_ctx.hpp"
#include "spk.hpp"

#include <cfloat>

namespace ttasr_detail {

// kind: 0 as given, 1 filters [80][1][251] -> [251][80], 2 conv [60][cin][5] -> [cin * 5][60] (the front end's layouts, as in
// engine_seg.hip), 3 a TDNN weight [cout][cin][taps] -> [taps * cin][cout], 4 a BatchNorm vector (kept on the host until
// ttasr_spk_finalize forms the scale; part = 0 weight, 1 bias, 2 running_mean, 3 running_var), 5 embedding.weight [D][3000] ->
// [3000][D rounded up to 4], 6 embedding.bias [D]
struct SpkSpec { std::string name; int ndim; int64_t dims[3]; int kind, layer, part; };

static std::vector<SpkSpec> spk_specs() {
  std::vector<SpkSpec> v;
  auto add = [&](std::string name, int ndim, int64_t d0, int64_t d1, int64_t d2, int kind, int layer = 0, int part = 0) {
    v.push_back(SpkSpec{std::move(name), ndim, {d0, d1, d2}, kind, layer, part});
  };
  add("sincnet.wav_norm1d.weight", 1, 1, 1, 1, 0); add("sincnet.wav_norm1d.bias", 1, 1, 1, 1, 0);
  add("sincnet.conv1d.0.filters", 3, kSegC1, 1, kSegTaps, 1);
  const int64_t nch[3] = {kSegC1, kSegC2, kSegC2};
  for (int i = 0; i < 3; ++i) {
    add("sincnet.norm1d." + std::to_string(i) + ".weight", 1, nch[i], 1, 1, 0);
    add("sincnet.norm1d." + std::to_string(i) + ".bias", 1, nch[i], 1, 1, 0);
  }
  add("sincnet.conv1d.1.weight", 3, kSegC2, kSegC1, 5, 2); add("sincnet.conv1d.1.bias", 1, kSegC2, 1, 1, 0);
  add("sincnet.conv1d.2.weight", 3, kSegC2, kSegC2, 5, 2); add("sincnet.conv1d.2.bias", 1, kSegC2, 1, 1, 0);
  static const char* parts[4] = {"weight", "bias", "running_mean", "running_var"};
  for (int l = 0; l < kSpkLayers; ++l) {
    const std::string conv = "tdnns." + std::to_string(3 * l), bn = "tdnns." + std::to_string(3 * l + 2);
    add(conv + ".weight", 3, kSpkCout[l], kSpkCin[l], kSpkTaps[l], 3, l);
    add(conv + ".bias", 1, kSpkCout[l], 1, 1, 0, l);
    for (int p = 0; p < 4; ++p) add(bn + "." + parts[p], 1, kSpkCout[l], 1, 1, 4, l, p);
  }
  add("embedding.weight", 2, 0, kSpkStats, 1, 5); add("embedding.bias", 1, 0, 1, 1, 6);
  return v;
}

// The scratch block (device) and its pinned twin.  Device: every region of SpkBuffers for kSpkGroup chunks.  Pinned: the PCM of a
// group, its chunk descriptors, its masks and its results.
struct SpkLayout {
  size_t pcm, desc, st0, a1, st1, a2, st2, a3, st3, h0, h1, h5, masks, valid, stats, emb, total;
  size_t p_pcm, p_desc, p_masks, p_stats, p_emb, p_total;
};
static SpkLayout spk_layout() {
  SpkLayout l;
  const size_t G = kSpkGroup, R = G * kSpkMaxMasks;
  Carve d, p;
  l.pcm = d.take(G * kSegChunk * 4); l.desc = d.take(G * sizeof(SegDesc));
  l.st0 = d.take(G * 8);
  l.a1 = d.take(G * kSegC1 * kSegL1 * 4); l.st1 = d.take(G * kSegC1 * 8);
  l.a2 = d.take(G * kSegC2 * kSegL2 * 4); l.st2 = d.take(G * kSegC2 * 8);
  l.a3 = d.take(G * kSegC2 * kSegT * 4);  l.st3 = d.take(G * kSegC2 * 8);
  l.h0 = d.take(G * kSpkRows * kSpkHid * 4); l.h1 = d.take(G * kSpkRows * kSpkHid * 4);
  l.h5 = d.take(G * kSpkT * kSpkOut * 4);
  l.masks = d.take(R * kSegT * 4); l.valid = d.take(R * 4);
  l.stats = d.take(R * kSpkStats * 4); l.emb = d.take(R * kSpkMaxDim * 4);
  l.total = d.used;
  l.p_pcm = p.take(G * kSegChunk * 4); l.p_desc = p.take(G * sizeof(SegDesc)); l.p_masks = p.take(R * kSegT * 4);
  l.p_stats = p.take(R * kSpkStats * 4); l.p_emb = p.take(R * kSpkMaxDim * 4);
  l.p_total = p.used;
  return l;
}

struct SpkState {
  std::vector<SpkSpec> spec = spk_specs();
  std::vector<float*> dev = std::vector<float*>(spec.size(), nullptr);   // device tensors (arena memory of the context)
  std::vector<uint8_t> loaded = std::vector<uint8_t>(spec.size(), 0);
  std::vector<float> bn[kSpkLayers][4];        // host copies of a BatchNorm's vectors until ttasr_spk_finalize
  float* bn_dev[kSpkLayers] = {};              // [3][cout]: running_mean | scale | bias
  int d_weight = 0, d_bias = 0;                // D as embedding.weight and embedding.bias brought it
  bool finalized = false;
  SpkWeights w{};
  DevBlock<> scratch; PinBlock<> pinned;
};

void spk_free(ttasr_ctx* c) {
  delete c->spk;
  c->spk = nullptr;
}

static int spk_load(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  if (!c->spk) c->spk = new SpkState();
  SpkState* v = c->spk;
  if (v->finalized) return fail(c, TTASR_E_INVALID, "speaker-embedding weights are finalized: they are read-only");
  int id = -1;
  for (size_t i = 0; i < v->spec.size(); ++i)
    if (v->spec[i].name == name) id = (int)i;
  if (id < 0) return fail(c, TTASR_E_WEIGHTS, "unknown speaker-embedding tensor '%s'", name);
  const SpkSpec& sp = v->spec[id];
  bool ok = ndim == sp.ndim;
  size_t n = 1;
  for (int i = 0; ok && i < ndim; ++i) {
    ok = sp.dims[i] ? dims[i] == sp.dims[i] : (dims[i] >= 1 && dims[i] <= kSpkMaxDim);   // 0: the embedding's dimension
    n *= (size_t)dims[i];
  }
  if (!ok) return fail(c, TTASR_E_WEIGHTS, "speaker-embedding tensor '%s': wrong shape", name);
  HIPCHK(c, hipSetDevice(c->device));
  if (sp.kind == 4) {
    v->bn[sp.layer][sp.part].assign(data, data + n);
    v->loaded[id] = 1;
    return TTASR_OK;
  }
  std::vector<float> t(data, data + n);
  size_t cap = n;   // floats of the device tensor
  if (sp.kind == 1) {
    for (int ch = 0; ch < kSegC1; ++ch)
      for (int k = 0; k < kSegTaps; ++k) t[(size_t)k * kSegC1 + ch] = data[(size_t)ch * kSegTaps + k];
  } else if (sp.kind == 2 || sp.kind == 3) {
    const int O = (int)sp.dims[0], Cin = (int)sp.dims[1], J = (int)sp.dims[2];
    for (int o = 0; o < O; ++o)
      for (int ci = 0; ci < Cin; ++ci)
        for (int j = 0; j < J; ++j)
          t[(sp.kind == 2 ? (size_t)ci * J + j : (size_t)j * Cin + ci) * O + o] = data[((size_t)o * Cin + ci) * J + j];
  } else if (sp.kind == 5) {
    const int D = (int)dims[0], ldd = (D + 3) & ~3;
    t.assign((size_t)kSpkStats * ldd, 0.f);
    for (int o = 0; o < D; ++o)
      for (int k = 0; k < kSpkStats; ++k) t[(size_t)k * ldd + o] = data[(size_t)o * kSpkStats + k];
    v->d_weight = D;
    cap = (size_t)kSpkStats * kSpkMaxDim;   // sized for the largest D, so a reload with another D reuses it
  } else if (sp.kind == 6) {
    v->d_bias = (int)dims[0];
    cap = kSpkMaxDim;
  }
  if (!v->dev[id]) TRY(dalloc(c, &v->dev[id], cap * 4));
  HIPCHK(c, hipMemcpyAsync(v->dev[id], t.data(), t.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // `t` is a stack temporary
  v->loaded[id] = 1;
  return TTASR_OK;
}

static int spk_finalize(ttasr_ctx* c) {
  SpkState* v = c->spk;
  if (!v) return fail(c, TTASR_E_WEIGHTS, "no speaker-embedding tensor was loaded");
  if (v->finalized) return TTASR_OK;
  for (size_t i = 0; i < v->spec.size(); ++i)
    if (!v->loaded[i]) return fail(c, TTASR_E_WEIGHTS, "speaker-embedding tensor '%s' is missing", v->spec[i].name.c_str());
  if (v->d_weight != v->d_bias)
    return fail(c, TTASR_E_WEIGHTS, "embedding.weight has %d rows, embedding.bias %d", v->d_weight, v->d_bias);
  HIPCHK(c, hipSetDevice(c->device));
  auto dev = [&](const std::string& name) -> const float* {
    for (size_t i = 0; i < v->spec.size(); ++i)
      if (v->spec[i].name == name) return v->dev[i];
    return nullptr;
  };
  SpkWeights& w = v->w;
  for (int l = 0; l < kSpkLayers; ++l) {
    const int N = kSpkCout[l];
    std::vector<float> t(3 * (size_t)N);
    for (int o = 0; o < N; ++o) {
      t[o] = v->bn[l][2][o];
      t[N + o] = (float)((double)v->bn[l][0][o] / sqrt((double)v->bn[l][3][o] + 1e-5));
      t[2 * N + o] = v->bn[l][1][o];
    }
    if (!v->bn_dev[l]) TRY(dalloc(c, &v->bn_dev[l], t.size() * 4));
    HIPCHK(c, hipMemcpyAsync(v->bn_dev[l], t.data(), t.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    w.bn_mean[l] = v->bn_dev[l]; w.bn_scale[l] = v->bn_dev[l] + N; w.bn_beta[l] = v->bn_dev[l] + 2 * N;
    w.wt[l] = dev("tdnns." + std::to_string(3 * l) + ".weight");
    w.bias[l] = dev("tdnns." + std::to_string(3 * l) + ".bias");
  }
  SegWeights& f = w.front;
  f.wav_w = dev("sincnet.wav_norm1d.weight"); f.wav_b = dev("sincnet.wav_norm1d.bias");
  f.sinc_t = dev("sincnet.conv1d.0.filters");
  for (int i = 0; i < 3; ++i) {
    f.norm_w[i] = dev("sincnet.norm1d." + std::to_string(i) + ".weight");
    f.norm_b[i] = dev("sincnet.norm1d." + std::to_string(i) + ".bias");
  }
  for (int i = 0; i < 2; ++i) {
    f.conv_t[i] = dev("sincnet.conv1d." + std::to_string(i + 1) + ".weight");
    f.conv_b[i] = dev("sincnet.conv1d." + std::to_string(i + 1) + ".bias");
  }
  w.emb_t = dev("embedding.weight"); w.emb_b = dev("embedding.bias");
  w.dim = v->d_weight; w.ldd = (v->d_weight + 3) & ~3;
  v->finalized = true;
  return TTASR_OK;
}

static int64_t spk_chunks(int64_t n) { return n <= 0 ? 0 : n <= kSegChunk ? 1 : 1 + (n - kSegChunk + kSegStep - 1) / kSegStep; }

// a recording's chunks [k0, k1) inside one group, the first of them at row `row` of the group
struct SpkPiece { int rec; int64_t k0, k1; int row; };

static int spk_embed(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* ns, int32_t S, const float* const* weights,
                     float* const* out_emb, float* const* out_stats) {
  SpkState* v = c->spk;
  if (!v || !v->finalized)
    return fail(c, TTASR_E_INVALID, "speaker-embedding weights not finalized (ttasr_spk_load_tensor, ttasr_spk_finalize first)");
  if (n < 1 || n > c->maxB) return fail(c, TTASR_E_INVALID, "n %d outside [1, max_batch = %d]", n, c->maxB);
  if (S < 1 || S > kSpkMaxMasks) return fail(c, TTASR_E_INVALID, "n_masks %d outside [1, %d]", S, kSpkMaxMasks);
  if (!pcm || !ns || !weights || !out_emb) return fail(c, TTASR_E_INVALID, "NULL argument");
  int64_t total_chunks = 0;
  for (int i = 0; i < n; ++i) {
    if (ns[i] < 0 || ns[i] > ((int64_t)1 << 40)) return fail(c, TTASR_E_INVALID, "recording %d: length outside [0, 2^40]", i);
    if (ns[i] > 0 && (!pcm[i] || !weights[i] || !out_emb[i] || (out_stats && !out_stats[i])))
      return fail(c, TTASR_E_INVALID, "recording %d: NULL pcm, weights or output row with %lld samples", i, (long long)ns[i]);
    total_chunks += spk_chunks(ns[i]);
  }
  for (int i = 0; i < n; ++i) {
    const size_t cnt = (size_t)spk_chunks(ns[i]) * S * kSegT;
    for (size_t q = 0; q < cnt; ++q)
      if (!(weights[i][q] >= 0.f && weights[i][q] <= FLT_MAX))
        return fail(c, TTASR_E_INVALID, "recording %d: weight %zu is negative or not finite", i, q);
  }
  TRY(session_refusal(c));
  HIPCHK(c, hipSetDevice(c->device));
  if (total_chunks == 0) return TTASR_OK;
  const SpkLayout l = spk_layout();
  TRY(v->scratch.ensure(c, l.total, "speaker-embedding scratch"));
  TRY(v->pinned.ensure(c, l.p_total, "speaker-embedding pinned staging"));
  hipStream_t s = c->stream;
  const int D = v->w.dim;
  SpkBuffers b{};
  SegBuffers& f = b.front;
  f.pcm = (const float*)(v->scratch + l.pcm); f.desc = (const SegDesc*)(v->scratch + l.desc);
  f.st0 = (float*)(v->scratch + l.st0);
  f.a1 = (float*)(v->scratch + l.a1); f.st1 = (float*)(v->scratch + l.st1);
  f.a2 = (float*)(v->scratch + l.a2); f.st2 = (float*)(v->scratch + l.st2);
  f.a3 = (float*)(v->scratch + l.a3); f.st3 = (float*)(v->scratch + l.st3);
  b.h[0] = (float*)(v->scratch + l.h0); b.h[1] = (float*)(v->scratch + l.h1); b.h5 = (float*)(v->scratch + l.h5);
  b.masks = (const float*)(v->scratch + l.masks); b.valid = (int32_t*)(v->scratch + l.valid);
  b.stats = (float*)(v->scratch + l.stats); b.emb = (float*)(v->scratch + l.emb);
  float* p_pcm = (float*)(v->pinned + l.p_pcm);
  SegDesc* p_desc = (SegDesc*)(v->pinned + l.p_desc);
  float* p_masks = (float*)(v->pinned + l.p_masks);
  float* p_stats = (float*)(v->pinned + l.p_stats);
  float* p_emb = (float*)(v->pinned + l.p_emb);

  std::vector<SpkPiece> pieces;
  pieces.reserve(kSpkGroup);
  int rec = 0; int64_t k = 0;   // the next chunk to place
  while (rec < n) {
    // the group: recordings in call order, chunks ascending, at most kSpkGroup chunks
    pieces.clear();
    int m = 0; size_t pcm_used = 0;
    while (rec < n && m < kSpkGroup) {
      const int64_t K = spk_chunks(ns[rec]);
      if (k >= K) { ++rec; k = 0; continue; }
      const int64_t k1 = std::min(K, k + (kSpkGroup - m));
      // its samples [8000 k0, end) once, the chunks as windows into them
      const int64_t first = (int64_t)kSegStep * k, end = std::min<int64_t>(ns[rec], (int64_t)kSegStep * (k1 - 1) + kSegChunk);
      memcpy(p_pcm + pcm_used, pcm[rec] + first, (size_t)(end - first) * 4);
      for (int64_t q = k; q < k1; ++q)
        p_desc[m + (q - k)] = SegDesc{(int32_t)(pcm_used + (size_t)kSegStep * (q - k)),
                                      (int32_t)std::min<int64_t>(kSegChunk, ns[rec] - (int64_t)kSegStep * q)};
      pcm_used += (size_t)(end - first);
      memcpy(p_masks + (size_t)m * S * kSegT, weights[rec] + (size_t)k * S * kSegT, (size_t)(k1 - k) * S * kSegT * 4);
      pieces.push_back(SpkPiece{rec, k, k1, m});
      m += (int)(k1 - k);
      k = k1;
    }
    if (m == 0) break;
    HIPCHK(c, hipMemcpyAsync((void*)f.pcm, p_pcm, pcm_used * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)f.desc, p_desc, (size_t)m * sizeof(SegDesc), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)b.masks, p_masks, (size_t)m * S * kSegT * 4, hipMemcpyHostToDevice, s));
    launch_spk_network(v->w, b, m, S, s);
    HIPCHK(c, hipMemcpyAsync(p_emb, b.emb, (size_t)m * S * D * 4, hipMemcpyDeviceToHost, s));
    if (out_stats) HIPCHK(c, hipMemcpyAsync(p_stats, b.stats, (size_t)m * S * kSpkStats * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    for (const SpkPiece& pc : pieces) {
      const size_t rows = (size_t)(pc.k1 - pc.k0) * S, at = (size_t)pc.row * S, to = (size_t)pc.k0 * S;
      memcpy(out_emb[pc.rec] + to * D, p_emb + at * D, rows * D * 4);
      if (out_stats) memcpy(out_stats[pc.rec] + to * kSpkStats, p_stats + at * kSpkStats, rows * kSpkStats * 4);
    }
  }
  return TTASR_OK;
}

}  // namespace ttasr_detail

extern "C" {

int ttasr_spk_load_tensor(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (!name || !data || !dims || ndim < 1 || ndim > 3)
    return fail(c, name && data && dims ? TTASR_E_WEIGHTS : TTASR_E_INVALID, "speaker-embedding tensor: bad argument");
  TRY(session_refusal(c));
  return spk_load(c, name, data, dims, ndim);
  });
}

int ttasr_spk_finalize(ttasr_ctx* c) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  return spk_finalize(c);
  });
}

int ttasr_spk_dim(ttasr_ctx* c) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (!c->spk || !c->spk->finalized) return fail(c, TTASR_E_INVALID, "speaker-embedding weights not finalized");
  return c->spk->w.dim;
  });
}

int ttasr_spk_embed(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* n_samples, int32_t n_masks,
                    const float* const* weights, float* const* out_emb, float* const* out_stats) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return spk_embed(c, n, pcm, n_samples, n_masks, weights, out_emb, out_stats);
  });
}

}  // extern "C"
