// libttasr: the segmentation VAD network behind the C ABI (one of the engine translation units, see engine_ctx.hpp): weight intake
// into the kernels' layouts, the context's scratch block and pinned staging, and the group loop of ttasr_seg_scores.  The kernels
// are kernels_seg.hip; the network is the text of include/ttasr.h.  Nothing here touches mel, encoder, search, graph, session or
// Silero state: the call's only shared resource is the context's stream.
#include "engine_ctx.hpp"
#include "seg.hpp"

namespace ttasr_detail {

// kind: how a tensor is laid out on the device - 0 as given, 1 filters [80][1][251] -> [251][80], 2 conv [60][cin][5] -> [cin * 5][60],
// 3 weight_ih [512][in] -> columns dir * 512 ... of [in][1024], 4 linear [out][in] -> [in][out], 5 a gate bias (kept on the host
// until ttasr_seg_finalize adds the pair), 6 classifier.weight [C][128] and 7 classifier.bias [C] with C in [1, 8]
struct SegSpec { std::string name; int ndim; int64_t dims[3]; int kind, layer, dir; };

static std::vector<SegSpec> seg_specs() {
  std::vector<SegSpec> v;
  auto add = [&](std::string name, int ndim, int64_t d0, int64_t d1, int64_t d2, int kind, int layer = 0, int dir = 0) {
    v.push_back(SegSpec{std::move(name), ndim, {d0, d1, d2}, kind, layer, dir});
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
  for (int l = 0; l < kSegLayers; ++l)
    for (int d = 0; d < 2; ++d) {
      const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
      add("lstm.weight_ih" + sfx, 2, 512, l ? 2 * kSegHid : kSegC2, 1, 3, l, d);
      add("lstm.weight_hh" + sfx, 2, 512, kSegHid, 1, 0, l, d);
      add("lstm.bias_ih" + sfx, 1, 512, 1, 1, 5, l, d);
      add("lstm.bias_hh" + sfx, 1, 512, 1, 1, 5, l, d);
    }
  add("linear.0.weight", 2, kSegHid, 2 * kSegHid, 1, 4); add("linear.0.bias", 1, kSegHid, 1, 1, 0);
  add("linear.1.weight", 2, kSegHid, kSegHid, 1, 4);     add("linear.1.bias", 1, kSegHid, 1, 1, 0);
  add("classifier.weight", 2, 0, kSegHid, 1, 6);         add("classifier.bias", 1, 0, 1, 1, 7);
  return v;
}

// The scratch block (device) and its pinned twin.  Device: every region of SegBuffers for kSegGroup chunks, the tables a group
// brings (chunk descriptors, aggregation jobs) and the Hamming window.  Pinned: the PCM of a group, its tables and its results.
struct SegLayout {
  size_t pcm, desc, jobs, st0, a1, st1, a2, st2, a3, st3, gx, y0, y1, probs, logits, score, agg, window, total;
  size_t p_pcm, p_desc, p_jobs, p_probs, p_logits, p_agg, p_total;
};
static SegLayout seg_layout() {
  SegLayout l;
  const size_t G = kSegGroup;
  Carve d, p;
  l.pcm = d.take(G * kSegChunk * 4); l.desc = d.take(G * sizeof(SegDesc)); l.jobs = d.take(G * sizeof(SegAggJob));
  l.st0 = d.take(G * 8);
  l.a1 = d.take(G * kSegC1 * kSegL1 * 4); l.st1 = d.take(G * kSegC1 * 8);
  l.a2 = d.take(G * kSegC2 * kSegL2 * 4); l.st2 = d.take(G * kSegC2 * 8);
  l.a3 = d.take(G * kSegC2 * kSegT * 4);  l.st3 = d.take(G * kSegC2 * 8);
  l.gx = d.take(G * 2 * kSegT * 512 * 4);
  l.y0 = d.take(G * kSegT * 256 * 4); l.y1 = d.take(G * kSegT * 256 * 4);
  l.probs = d.take(G * kSegT * kSegMaxC * 4); l.logits = d.take(G * kSegT * kSegMaxC * 4);
  l.score = d.take((G + kSegCarry) * kSegT * 4);
  l.agg = d.take(G * kSegAggRow * 4);
  l.window = d.take(kSegT * 4);
  l.total = d.used;
  l.p_pcm = p.take(G * kSegChunk * 4); l.p_desc = p.take(G * sizeof(SegDesc)); l.p_jobs = p.take(G * sizeof(SegAggJob));
  l.p_probs = p.take(G * kSegT * kSegMaxC * 4); l.p_logits = p.take(G * kSegT * kSegMaxC * 4); l.p_agg = p.take(G * kSegAggRow * 4);
  l.p_total = p.used;
  return l;
}

struct SegState {
  std::vector<SegSpec> spec = seg_specs();
  std::vector<float*> dev = std::vector<float*>(spec.size(), nullptr);   // device tensors (arena memory of the context)
  std::vector<uint8_t> loaded = std::vector<uint8_t>(spec.size(), 0);
  std::vector<float> bias[kSegLayers][2][2];   // host copies of bias_ih | bias_hh until ttasr_seg_finalize adds them
  float* wih_t[kSegLayers] = {}; float* gate_b[kSegLayers] = {};
  int c_weight = 0, c_bias = 0;                // C as classifier.weight and classifier.bias brought it
  bool finalized = false;
  SegWeights w{};
  DevBlock<> scratch; PinBlock<> pinned;
};

void seg_free(ttasr_ctx* c) {
  delete c->seg;
  c->seg = nullptr;
}

// Both blocks, allocated by the first call; the device block's first allocation brings the Hamming window
static int seg_blocks(ttasr_ctx* c) {
  SegState* v = c->seg;
  const SegLayout l = seg_layout();
  if (!v->scratch) {
    TRY(v->scratch.ensure(c, l.total, "segmentation scratch"));
    // w = np.hamming(293) rounded to f32
    std::vector<float> win(kSegT);
    for (int i = 0; i < kSegT; ++i) win[i] = (float)(0.54 - 0.46 * cos(2.0 * 3.14159265358979323846 * i / (kSegT - 1)));
    HIPCHK(c, hipMemcpyAsync(v->scratch + l.window, win.data(), kSegT * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // `win` is a stack temporary
  }
  return v->pinned.ensure(c, l.p_total, "segmentation pinned staging");
}

static int seg_load(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  if (!c->seg) c->seg = new SegState();
  SegState* v = c->seg;
  if (v->finalized) return fail(c, TTASR_E_INVALID, "segmentation weights are finalized: they are read-only");
  int id = -1;
  for (size_t i = 0; i < v->spec.size(); ++i)
    if (v->spec[i].name == name) id = (int)i;
  if (id < 0) return fail(c, TTASR_E_WEIGHTS, "unknown segmentation tensor '%s'", name);
  const SegSpec& sp = v->spec[id];
  bool ok = ndim == sp.ndim;
  size_t n = 1;
  for (int i = 0; ok && i < ndim; ++i) {
    ok = sp.dims[i] ? dims[i] == sp.dims[i] : (dims[i] >= 1 && dims[i] <= kSegMaxC);   // 0: the number of classes
    n *= (size_t)dims[i];
  }
  if (!ok) return fail(c, TTASR_E_WEIGHTS, "segmentation tensor '%s': wrong shape", name);
  HIPCHK(c, hipSetDevice(c->device));
  if (sp.kind == 5) {
    v->bias[sp.layer][sp.dir][sp.name.compare(0, 12, "lstm.bias_hh") == 0].assign(data, data + n);
    v->loaded[id] = 1;
    return TTASR_OK;
  }
  std::vector<float> t(data, data + n);
  float* dst = nullptr;
  size_t dst_off = 0, rows = 1, row_len = n, pitch = n;   // the upload: `rows` pieces of row_len floats, `pitch` apart on the device
  if (sp.kind == 1) {
    for (int ch = 0; ch < kSegC1; ++ch)
      for (int k = 0; k < kSegTaps; ++k) t[(size_t)k * kSegC1 + ch] = data[(size_t)ch * kSegTaps + k];
  } else if (sp.kind == 2) {
    const int O = (int)sp.dims[0], Cin = (int)sp.dims[1];
    for (int o = 0; o < O; ++o)
      for (int ci = 0; ci < Cin; ++ci)
        for (int j = 0; j < 5; ++j) t[((size_t)ci * 5 + j) * O + o] = data[((size_t)o * Cin + ci) * 5 + j];
  } else if (sp.kind == 3 || sp.kind == 4) {
    const int O = (int)sp.dims[0], In = (int)sp.dims[1];
    for (int r = 0; r < O; ++r)
      for (int k = 0; k < In; ++k) t[(size_t)k * O + r] = data[(size_t)r * In + k];
    if (sp.kind == 3) {
      if (!v->wih_t[sp.layer]) TRY(dalloc(c, &v->wih_t[sp.layer], (size_t)In * 1024 * 4));
      dst = v->wih_t[sp.layer]; dst_off = (size_t)sp.dir * 512; rows = In; row_len = 512; pitch = 1024;
    }
  }
  if (sp.kind == 6) v->c_weight = (int)dims[0];
  if (sp.kind == 7) v->c_bias = (int)dims[0];
  if (!dst) {
    // the classifier's pieces are sized for kSegMaxC classes, so a reload with another C reuses them
    if (!v->dev[id]) TRY(dalloc(c, &v->dev[id], (sp.kind >= 6 ? n / (size_t)dims[0] * kSegMaxC : n) * 4));
    dst = v->dev[id];
  }
  HIPCHK(c, hipMemcpy2DAsync(dst + dst_off, pitch * 4, t.data(), row_len * 4, row_len * 4, rows, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // `t` is a stack temporary
  v->loaded[id] = 1;
  return TTASR_OK;
}

static int seg_finalize(ttasr_ctx* c) {
  SegState* v = c->seg;
  if (!v) return fail(c, TTASR_E_WEIGHTS, "no segmentation tensor was loaded");
  if (v->finalized) return TTASR_OK;
  for (size_t i = 0; i < v->spec.size(); ++i)
    if (!v->loaded[i]) return fail(c, TTASR_E_WEIGHTS, "segmentation tensor '%s' is missing", v->spec[i].name.c_str());
  if (v->c_weight != v->c_bias)
    return fail(c, TTASR_E_WEIGHTS, "classifier.weight has %d classes, classifier.bias %d", v->c_weight, v->c_bias);
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<float> gb(1024);
  for (int l = 0; l < kSegLayers; ++l) {
    for (int d = 0; d < 2; ++d)
      for (int r = 0; r < 512; ++r) gb[d * 512 + r] = v->bias[l][d][0][r] + v->bias[l][d][1][r];
    if (!v->gate_b[l]) TRY(dalloc(c, &v->gate_b[l], 1024 * 4));
    HIPCHK(c, hipMemcpyAsync(v->gate_b[l], gb.data(), 1024 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  auto dev = [&](const std::string& name) -> const float* {
    for (size_t i = 0; i < v->spec.size(); ++i)
      if (v->spec[i].name == name) return v->dev[i];
    return nullptr;
  };
  SegWeights& w = v->w;
  w.wav_w = dev("sincnet.wav_norm1d.weight"); w.wav_b = dev("sincnet.wav_norm1d.bias");
  w.sinc_t = dev("sincnet.conv1d.0.filters");
  for (int i = 0; i < 3; ++i) {
    w.norm_w[i] = dev("sincnet.norm1d." + std::to_string(i) + ".weight");
    w.norm_b[i] = dev("sincnet.norm1d." + std::to_string(i) + ".bias");
  }
  for (int i = 0; i < 2; ++i) {
    w.conv_t[i] = dev("sincnet.conv1d." + std::to_string(i + 1) + ".weight");
    w.conv_b[i] = dev("sincnet.conv1d." + std::to_string(i + 1) + ".bias");
    w.lin_t[i] = dev("linear." + std::to_string(i) + ".weight");
    w.lin_b[i] = dev("linear." + std::to_string(i) + ".bias");
  }
  for (int l = 0; l < kSegLayers; ++l) {
    w.wih_t[l] = v->wih_t[l]; w.gate_b[l] = v->gate_b[l];
    w.whh[l][0] = dev("lstm.weight_hh_l" + std::to_string(l));
    w.whh[l][1] = dev("lstm.weight_hh_l" + std::to_string(l) + "_reverse");
  }
  w.cls_w = dev("classifier.weight"); w.cls_b = dev("classifier.bias");
  w.classes = v->c_weight;
  v->finalized = true;
  return TTASR_OK;
}

static int64_t seg_chunks(int64_t n) { return n <= 0 ? 0 : n <= kSegChunk ? 1 : 1 + (n - kSegChunk + kSegStep - 1) / kSegStep; }
static int64_t seg_start(int64_t k) { return ((int64_t)kSegStep * k + 135) / 270; }   // s(k): the recording frame of chunk k's frame 0
static int64_t seg_frames(int64_t n) {
  const int64_t K = seg_chunks(n);
  return K == 0 ? 0 : std::min((n + 269) / 270, seg_start(K - 1) + kSegT);
}

// a recording's chunks [k0, k1) inside one group, the first of them at row `row` of the group
struct SegPiece { int rec; int64_t k0, k1; int row; int64_t j0, j1; int32_t out_off; };

static int seg_scores(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* ns, float* const* out_scores,
                      float* const* out_probs, float* const* out_logits) {
  SegState* v = c->seg;
  if (!v || !v->finalized)
    return fail(c, TTASR_E_INVALID, "segmentation weights not finalized (ttasr_seg_load_tensor, ttasr_seg_finalize first)");
  if (n < 1 || n > c->maxB) return fail(c, TTASR_E_INVALID, "n %d outside [1, max_batch = %d]", n, c->maxB);
  if (!pcm || !ns || !out_scores) return fail(c, TTASR_E_INVALID, "NULL argument");
  int64_t total_chunks = 0;
  for (int i = 0; i < n; ++i) {
    if (ns[i] < 0 || ns[i] > ((int64_t)1 << 40)) return fail(c, TTASR_E_INVALID, "recording %d: length outside [0, 2^40]", i);
    if (ns[i] > 0 && (!pcm[i] || !out_scores[i] || (out_probs && !out_probs[i]) || (out_logits && !out_logits[i])))
      return fail(c, TTASR_E_INVALID, "recording %d: NULL pcm or output row with %lld samples", i, (long long)ns[i]);
    total_chunks += seg_chunks(ns[i]);
  }
  TRY(session_refusal(c));
  HIPCHK(c, hipSetDevice(c->device));
  if (total_chunks == 0) return TTASR_OK;
  TRY(seg_blocks(c));
  hipStream_t s = c->stream;
  const SegLayout l = seg_layout();
  const int C = v->w.classes;
  SegBuffers b;
  b.pcm = (const float*)(v->scratch + l.pcm); b.desc = (const SegDesc*)(v->scratch + l.desc); b.jobs = (const SegAggJob*)(v->scratch + l.jobs);
  b.st0 = (float*)(v->scratch + l.st0);
  b.a1 = (float*)(v->scratch + l.a1); b.st1 = (float*)(v->scratch + l.st1);
  b.a2 = (float*)(v->scratch + l.a2); b.st2 = (float*)(v->scratch + l.st2);
  b.a3 = (float*)(v->scratch + l.a3); b.st3 = (float*)(v->scratch + l.st3);
  b.gx = (float*)(v->scratch + l.gx); b.y[0] = (float*)(v->scratch + l.y0); b.y[1] = (float*)(v->scratch + l.y1);
  b.probs = (float*)(v->scratch + l.probs); b.logits = (float*)(v->scratch + l.logits);
  b.score = (float*)(v->scratch + l.score); b.agg_out = (float*)(v->scratch + l.agg); b.window = (const float*)(v->scratch + l.window);
  float* p_pcm = (float*)(v->pinned + l.p_pcm);
  SegDesc* p_desc = (SegDesc*)(v->pinned + l.p_desc);
  SegAggJob* p_jobs = (SegAggJob*)(v->pinned + l.p_jobs);
  float* p_probs = (float*)(v->pinned + l.p_probs);
  float* p_logits = (float*)(v->pinned + l.p_logits);
  float* p_agg = (float*)(v->pinned + l.p_agg);
  // the recurrence form: one chunk per workgroup is the measured choice at every group size
  const int rows = c->seg_lstm_rows ? c->seg_lstm_rows : 1;

  std::vector<SegPiece> pieces;
  pieces.reserve(kSegGroup);
  int rec = 0; int64_t k = 0;   // the next chunk to place
  while (rec < n) {
    // (1) the group: recordings in call order, chunks ascending, at most kSegGroup chunks
    pieces.clear();
    int m = 0; size_t pcm_used = 0; int32_t agg_used = 0; int64_t max_frames = 0; int64_t carry = 0;
    while (rec < n && m < kSegGroup) {
      const int64_t K = seg_chunks(ns[rec]);
      if (k >= K) { ++rec; k = 0; continue; }
      const int64_t k1 = std::min(K, k + (kSegGroup - m));
      const int64_t F = seg_frames(ns[rec]);
      SegPiece pc{rec, k, k1, m, std::min(F, k ? seg_start(k) : 0), k1 == K ? F : std::min(F, seg_start(k1)), agg_used};
      // its samples [8000 k0, end) once, the chunks as windows into them
      const int64_t first = (int64_t)kSegStep * k, end = std::min<int64_t>(ns[rec], (int64_t)kSegStep * (k1 - 1) + kSegChunk);
      memcpy(p_pcm + pcm_used, pcm[rec] + first, (size_t)(end - first) * 4);
      for (int64_t q = k; q < k1; ++q) {
        p_desc[m + (q - k)] = SegDesc{(int32_t)(pcm_used + (size_t)kSegStep * (q - k)),
                                      (int32_t)std::min<int64_t>(kSegChunk, ns[rec] - (int64_t)kSegStep * q)};
      }
      pcm_used += (size_t)(end - first);
      if (k > 0 && m == 0) carry = std::min<int64_t>(kSegCarry, k);   // its earlier chunks closed the previous group
      p_jobs[pieces.size()] = SegAggJob{k - (m == 0 ? carry : 0), k1, pc.j0, pc.j1, (int32_t)(kSegCarry + m - (m == 0 ? carry : 0)), agg_used};
      agg_used += (int32_t)(pc.j1 - pc.j0);
      max_frames = std::max(max_frames, pc.j1 - pc.j0);
      pieces.push_back(pc);
      m += (int)(k1 - k);
      k = k1;
    }
    if (m == 0) break;
    // (2) the scores of the chunks in front of the group: the last rows of the previous group
    if (carry)
      HIPCHK(c, hipMemcpyAsync(b.score + (size_t)(kSegCarry - carry) * kSegT, b.score + (size_t)(kSegCarry + kSegGroup - carry) * kSegT,
                               (size_t)carry * kSegT * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)b.pcm, p_pcm, pcm_used * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)b.desc, p_desc, (size_t)m * sizeof(SegDesc), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync((void*)b.jobs, p_jobs, pieces.size() * sizeof(SegAggJob), hipMemcpyHostToDevice, s));
    launch_seg_network(v->w, b, m, rows, s);
    if (max_frames > 0) {
      launch_seg_aggregate(b, (int)pieces.size(), max_frames, s);
      HIPCHK(c, hipMemcpyAsync(p_agg, b.agg_out, (size_t)agg_used * 4, hipMemcpyDeviceToHost, s));
    }
    if (out_probs) HIPCHK(c, hipMemcpyAsync(p_probs, b.probs, (size_t)m * kSegT * C * 4, hipMemcpyDeviceToHost, s));
    if (out_logits) HIPCHK(c, hipMemcpyAsync(p_logits, b.logits, (size_t)m * kSegT * C * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    for (const SegPiece& pc : pieces) {
      if (pc.j1 > pc.j0) memcpy(out_scores[pc.rec] + pc.j0, p_agg + pc.out_off, (size_t)(pc.j1 - pc.j0) * 4);
      const size_t cnt = (size_t)(pc.k1 - pc.k0) * kSegT * C, at = (size_t)pc.row * kSegT * C, to = (size_t)pc.k0 * kSegT * C;
      if (out_probs) memcpy(out_probs[pc.rec] + to, p_probs + at, cnt * 4);
      if (out_logits) memcpy(out_logits[pc.rec] + to, p_logits + at, cnt * 4);
    }
  }
  return TTASR_OK;
}

}  // namespace ttasr_detail

extern "C" {

int ttasr_seg_load_tensor(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (!name || !data || !dims || ndim < 1 || ndim > 3)
    return fail(c, name && data && dims ? TTASR_E_WEIGHTS : TTASR_E_INVALID, "segmentation tensor: bad argument");
  TRY(session_refusal(c));
  return seg_load(c, name, data, dims, ndim);
  });
}

int ttasr_seg_finalize(ttasr_ctx* c) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  return seg_finalize(c);
  });
}

int ttasr_seg_classes(ttasr_ctx* c) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (!c->seg || !c->seg->finalized) return fail(c, TTASR_E_INVALID, "segmentation weights not finalized");
  return c->seg->w.classes;
  });
}

int64_t ttasr_seg_chunks(int64_t n_samples) {
  return n_samples < 0 || n_samples > ((int64_t)1 << 40) ? -1 : seg_chunks(n_samples);
}

int64_t ttasr_seg_frames(int64_t n_samples) {
  return n_samples < 0 || n_samples > ((int64_t)1 << 40) ? -1 : seg_frames(n_samples);
}

int ttasr_seg_scores(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* n_samples, float* const* out_scores,
                     float* const* out_chunk_probs, float* const* out_chunk_logits) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return seg_scores(c, n, pcm, n_samples, out_scores, out_chunk_probs, out_chunk_logits);
  });
}

}  // extern "C"
