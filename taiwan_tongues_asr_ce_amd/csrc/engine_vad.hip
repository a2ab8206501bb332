// libttasr: the voice-activity network behind the C ABI (one of the engine translation units, see engine_ctx.hpp): weight intake
// into the kernels' layouts, the context's scratch block and pinned staging, the chunk loop that ttasr_vad_probs and
// ttasr_vad_stream_push share, the streams' host state, and wire streams (ttasr_vad_stream_push_wire: bytes through the stream
// kernel of kernels_ingest.hip, then into that same push).  The kernels are kernels_vad.hip; the network is the text of
// include/ttasr.h.  Nothing here touches mel, encoder, search or graph state: the call's only shared resource is the context's stream.
#include "engine_ctx.hpp"
#include "ingest.hpp"
#include "vad.hpp"

namespace ttasr_detail {

// The tensor-name table of the C side (a leading "_model." is stripped before the lookup).  kind: how the tensor is laid out on
// the device - 0 as given, 1 [258][1][256] -> [256][258], 2 conv [out][in][3] -> [in * 3][out], 3 [512][128] -> [128][512].
struct VadSpec { const char* name; int ndim; int64_t dims[3]; int kind; };
enum { V_BASIS, V_W0, V_W1, V_W2, V_W3, V_B0, V_B1, V_B2, V_B3, V_WIH, V_WHH, V_BIH, V_BHH, V_WOUT, V_BOUT, V_COUNT };
static const VadSpec kVadSpec[V_COUNT] = {
    {"stft.forward_basis_buffer", 3, {258, 1, 256}, 1},
    {"encoder.0.reparam_conv.weight", 3, {128, 129, 3}, 2}, {"encoder.1.reparam_conv.weight", 3, {64, 128, 3}, 2},
    {"encoder.2.reparam_conv.weight", 3, {64, 64, 3}, 2},   {"encoder.3.reparam_conv.weight", 3, {128, 64, 3}, 2},
    {"encoder.0.reparam_conv.bias", 1, {128, 1, 1}, 0},     {"encoder.1.reparam_conv.bias", 1, {64, 1, 1}, 0},
    {"encoder.2.reparam_conv.bias", 1, {64, 1, 1}, 0},      {"encoder.3.reparam_conv.bias", 1, {128, 1, 1}, 0},
    {"decoder.rnn.weight_ih", 2, {512, 128, 1}, 3},         {"decoder.rnn.weight_hh", 2, {512, 128, 1}, 0},
    {"decoder.rnn.bias_ih", 1, {512, 1, 1}, 0},             {"decoder.rnn.bias_hh", 1, {512, 1, 1}, 0},
    {"decoder.decoder.2.weight", 3, {1, 128, 1}, 0},        {"decoder.decoder.2.bias", 1, {1, 1, 1}, 0},
};

constexpr int kVadPinSlots = 8;   // chunk slots of PCM in the pinned staging block (8 x 2 MiB)

struct VadStreams;
struct VadState {
  float* dev[V_COUNT] = {};       // device tensors (arena memory of the context)
  float* gate_b = nullptr;        // b_ih + b_hh
  bool loaded[V_COUNT] = {};
  std::vector<float> bih, bhh;    // host copies until ttasr_vad_finalize adds them
  bool finalized = false;
  VadWeights w{};
  // scratch: pcm [files][kVadSlot] | gx [files][C][512] | out [files][2][C] | state [files][256] | nf [files] | slot [files]
  DevBlock<> scratch; int scratch_files = 0;
  // pinned: pcm slots [kVadPinSlots][kVadSlot] | out [max_batch][2][C] | nf [max_batch] | slot [max_batch]
  PinBlock<> pinned;
  std::unique_ptr<VadStreams> streams;   // created by the first ttasr_vad_stream_open
  ~VadState();                           // where VadStreams is complete
};

// One row of a pass through the chunk loop, as ONE sequence of samples: positions [-64, 0) the context in front of the first frame
// (ctx; nullptr = zeros), [0, n_head) samples held from earlier (a stream's pending ones), [n_head, n_head + n_pcm) the caller's,
// zeros behind.  `frames` frames of 512 are evaluated from position 0.
struct VadRow {
  const float* ctx; const float* head; int64_t n_head; const float* pcm; int64_t n_pcm;
  int64_t frames; float* probs; float* logits;
};

// count samples of the row's sequence from position pos (>= -64) on: what a frame of the network reads is this and nothing else,
// for a whole recording and for a stream alike
static void vad_gather(float* dst, const VadRow& r, int64_t pos, int64_t count) {
  const int64_t end = pos + count, total = r.n_head + r.n_pcm;
  const struct { int64_t lo, hi; const float* p; } seg[3] = {
      {-(int64_t)kVadContext, 0, r.ctx}, {0, r.n_head, r.head}, {r.n_head, total, r.pcm}};
  for (const auto& g : seg) {
    const int64_t lo = std::max(pos, g.lo), hi = std::min(end, g.hi);
    if (lo >= hi) continue;
    if (g.p) memcpy(dst + (lo - pos), g.p + (lo - g.lo), (size_t)(hi - lo) * 4);
    else memset(dst + (lo - pos), 0, (size_t)(hi - lo) * 4);
  }
  const int64_t z = std::max(pos, total);
  if (z < end) memset(dst + (z - pos), 0, (size_t)(end - z) * 4);
}

// A stream (include/ttasr.h): its (h, c) is row `id` of the device table; here the last 64 evaluated samples and the samples that
// do not fill a frame yet.  fresh: the table row is to be zeroed before the stream's next frame (open, reset, finish and a failed
// push only set the flag, so none of them touches the device).
// A WIRE stream adds what stands in front of the network: the format it was opened with, the frames received (F) and the 16 kHz
// samples handed on (K) so far, the bytes that do not fill a frame yet, and which half of the device history table holds its
// last H mono values.  A stream with F == 0 reads no history: reset touches no device memory.
struct VadStream {
  bool open = false, fresh = true; int n_pend = 0; float ctx[kVadContext] = {}; float pend[kVadWindow] = {};
  bool wire = false; WirePlan plan; int channels = 1, format = TTASR_PCM_S16, pick = -1, fb = 2;
  int64_t F = 0, K = 0; int n_raw = 0, half = 0; uint8_t raw[64] = {};
};

constexpr size_t kWireRawBytes = (size_t)8 << 20;     // raw bytes of all rows of one push chunk
constexpr size_t kWireOutFloats = (size_t)2 << 20;    // their results
constexpr size_t kWireJobBytes = (sizeof(WireJob) * TTASR_VAD_MAX_STREAMS + 255) & ~(size_t)255;

// one row of a ttasr_vad_stream_push_wire while the call walks its chunks
struct WireRow {
  const uint8_t* src; int64_t n_src, pos /*bytes of [held | src] consumed*/, frames_left, pcm_done; int32_t vad_done;
  bool fin, done;
};

struct VadStreams {
  DevBlock<float> table;                        // [TTASR_VAD_MAX_STREAMS][256], device
  int n_open = 0;
  std::vector<VadStream> s = std::vector<VadStream>(TTASR_VAD_MAX_STREAMS);
  std::vector<VadRow> rows = std::vector<VadRow>(TTASR_VAD_MAX_STREAMS);   // a push's rows (n <= open streams): a push never allocates
  std::vector<uint8_t> seen = std::vector<uint8_t>(TTASR_VAD_MAX_STREAMS);
  // wire streams (the first ttasr_vad_stream_open_wire allocates): the history table [2][TTASR_VAD_MAX_STREAMS][256], the device
  // block job table | raw pool | result pool and its pinned twin, and a wire push's rows with the float push each chunk hands on
  DevBlock<float> hist; DevBlock<> wire_dev; PinBlock<> wire_pin;
  std::vector<WireRow> wrows;
  std::vector<int32_t> sub_ids, sub_fin, sub_frames, sub_row;
  std::vector<const float*> sub_pcm; std::vector<int64_t> sub_ns; std::vector<float*> sub_probs, sub_logits;
};
static void vad_stream_clear(VadStream& st) {
  st.fresh = true; st.n_pend = 0; memset(st.ctx, 0, sizeof st.ctx);
  st.F = st.K = 0; st.n_raw = 0;
}

VadState::~VadState() = default;
void vad_free(ttasr_ctx* c) {
  delete c->vad;
  c->vad = nullptr;
}

struct VadScratch { size_t pcm, gx, out, state, nf, slot, total; };
static VadScratch vad_scratch_layout(int files) {
  VadScratch l;
  Carve cv;
  l.pcm = cv.take((size_t)files * kVadSlot * 4);
  l.gx = cv.take((size_t)files * kVadChunk * 512 * 4);
  l.out = cv.take((size_t)files * 2 * kVadChunk * 4);
  l.state = cv.take((size_t)files * 256 * 4);
  l.nf = cv.take((size_t)files * 4);
  l.slot = cv.take((size_t)files * 4);
  l.total = cv.used;
  return l;
}

// One device block for `files` recordings, grown to the largest request (the layout is that of scratch_files recordings)
static int vad_scratch(ttasr_ctx* c, int files) {
  VadState* v = c->vad;
  if (files <= v->scratch_files) return 0;
  const int rc = v->scratch.ensure(c, vad_scratch_layout(files).total, "VAD scratch");
  if (!v->scratch) v->scratch_files = 0;   // could not be allocated: the next call allocates again
  else if (rc == 0) v->scratch_files = files;
  return rc;
}

static int vad_pinned(ttasr_ctx* c) {
  return c->vad->pinned.ensure(c, (size_t)kVadPinSlots * kVadSlot * 4 + (size_t)c->maxB * 2 * kVadChunk * 4 + (size_t)c->maxB * 8,
                               "VAD pinned staging");
}

static int vad_load(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  if (!c->vad) c->vad = new VadState();
  VadState* v = c->vad;
  if (v->finalized) return fail(c, TTASR_E_INVALID, "VAD weights are finalized: they are read-only");
  if (strncmp(name, "_model.", 7) == 0) name += 7;
  int id = -1;
  for (int i = 0; i < V_COUNT; ++i)
    if (strcmp(name, kVadSpec[i].name) == 0) id = i;
  if (id < 0) return fail(c, TTASR_E_WEIGHTS, "unknown VAD tensor '%s'", name);
  const VadSpec& sp = kVadSpec[id];
  bool ok = ndim == sp.ndim;
  size_t n = 1;
  for (int i = 0; ok && i < ndim; ++i) { ok = dims[i] == sp.dims[i]; n *= (size_t)sp.dims[i]; }
  if (!ok) return fail(c, TTASR_E_WEIGHTS, "VAD tensor '%s': wrong shape", name);
  std::vector<float> t(data, data + n);
  if (sp.kind == 1) {
    for (int k = 0; k < 258; ++k)
      for (int m = 0; m < 256; ++m) t[(size_t)m * 258 + k] = data[(size_t)k * 256 + m];
  } else if (sp.kind == 2) {
    const int O = (int)sp.dims[0], Cin = (int)sp.dims[1];
    for (int o = 0; o < O; ++o)
      for (int ci = 0; ci < Cin; ++ci)
        for (int j = 0; j < 3; ++j) t[((size_t)ci * 3 + j) * O + o] = data[((size_t)o * Cin + ci) * 3 + j];
  } else if (sp.kind == 3) {
    for (int r = 0; r < 512; ++r)
      for (int k = 0; k < 128; ++k) t[(size_t)k * 512 + r] = data[(size_t)r * 128 + k];
  }
  if (id == V_BIH) v->bih.assign(data, data + n);
  if (id == V_BHH) v->bhh.assign(data, data + n);
  HIPCHK(c, hipSetDevice(c->device));
  if (!v->dev[id]) TRY(dalloc(c, &v->dev[id], n * 4));
  HIPCHK(c, hipMemcpyAsync(v->dev[id], t.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // `t` is a stack temporary
  v->loaded[id] = true;
  return TTASR_OK;
}

static int vad_finalize(ttasr_ctx* c) {
  VadState* v = c->vad;
  if (!v) return fail(c, TTASR_E_WEIGHTS, "no VAD tensor was loaded");
  if (v->finalized) return TTASR_OK;
  for (int i = 0; i < V_COUNT; ++i)
    if (!v->loaded[i]) return fail(c, TTASR_E_WEIGHTS, "VAD tensor '%s' is missing", kVadSpec[i].name);
  std::vector<float> gb(512);
  for (int r = 0; r < 512; ++r) gb[r] = v->bih[r] + v->bhh[r];
  HIPCHK(c, hipSetDevice(c->device));
  if (!v->gate_b) TRY(dalloc(c, &v->gate_b, 512 * 4));
  HIPCHK(c, hipMemcpyAsync(v->gate_b, gb.data(), 512 * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  VadWeights& w = v->w;
  w.basis_t = v->dev[V_BASIS];
  for (int l = 0; l < 4; ++l) { w.conv_t[l] = v->dev[V_W0 + l]; w.conv_b[l] = v->dev[V_B0 + l]; }
  w.wih_t = v->dev[V_WIH]; w.gate_b = v->gate_b; w.whh = v->dev[V_WHH]; w.w_out = v->dev[V_WOUT]; w.b_out = v->dev[V_BOUT];
  v->finalized = true;
  return TTASR_OK;
}

// The chunk loop of both paths: n <= scratch_files rows, frames of row i in time chunks of kVadChunk, (h, c) of row i at
// state[slots[i]] (slots == nullptr: state[i]) carried from chunk to chunk.  Ends synchronised.
static int vad_run(ttasr_ctx* c, const VadRow* rows, int n, float* d_state, const int32_t* slots) {
  VadState* v = c->vad;
  hipStream_t s = c->stream;
  const VadScratch l = vad_scratch_layout(v->scratch_files);
  float* d_pcm = (float*)(v->scratch + l.pcm);
  float* d_gx = (float*)(v->scratch + l.gx);
  float* d_out = (float*)(v->scratch + l.out);
  int32_t* d_nf = (int32_t*)(v->scratch + l.nf);
  int32_t* d_slot = slots ? (int32_t*)(v->scratch + l.slot) : nullptr;
  float* p_pcm = (float*)v->pinned.get();
  float* p_out = p_pcm + (size_t)kVadPinSlots * kVadSlot;
  int32_t* p_nf = (int32_t*)(p_out + (size_t)c->maxB * 2 * kVadChunk);
  int32_t* p_slot = p_nf + c->maxB;
  int64_t max_frames = 0;
  for (int i = 0; i < n; ++i) max_frames = std::max(max_frames, rows[i].frames);
  if (max_frames == 0) return TTASR_OK;
  if (slots) {
    memcpy(p_slot, slots, (size_t)n * 4);
    HIPCHK(c, hipMemcpyAsync(d_slot, p_slot, (size_t)n * 4, hipMemcpyHostToDevice, s));
  }
  for (int64_t k0 = 0; k0 < max_frames; k0 += kVadChunk) {
    int max_nf = 0, staged = 0;
    for (int i = 0; i < n; ++i) {
      const int nf = (int)std::min<int64_t>(std::max<int64_t>(rows[i].frames - k0, 0), kVadChunk);
      p_nf[i] = nf;
      max_nf = std::max(max_nf, nf);
      if (nf == 0) continue;
      // the slot: 64 samples in front of the chunk (zeros in front of the recording) | nf frames, zeros behind the last sample
      if (staged && staged % kVadPinSlots == 0) HIPCHK(c, hipStreamSynchronize(s));   // the slots are free again
      float* slot = p_pcm + (size_t)(staged % kVadPinSlots) * kVadSlot;
      const int64_t count = kVadContext + (int64_t)nf * kVadWindow;
      vad_gather(slot, rows[i], k0 * kVadWindow - kVadContext, count);
      HIPCHK(c, hipMemcpyAsync(d_pcm + (size_t)i * kVadSlot, slot, (size_t)count * 4, hipMemcpyHostToDevice, s));
      ++staged;
    }
    HIPCHK(c, hipMemcpyAsync(d_nf, p_nf, (size_t)n * 4, hipMemcpyHostToDevice, s));
    launch_vad_frames(v->w, d_pcm, d_nf, d_gx, n, max_nf, s);
    launch_vad_lstm(v->w, d_gx, d_nf, d_state, d_slot, d_out, n, s);
    HIPCHK(c, hipMemcpyAsync(p_out, d_out, (size_t)n * 2 * kVadChunk * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < n; ++i) {
      if (p_nf[i] == 0) continue;
      const float* row = p_out + (size_t)i * 2 * kVadChunk;
      if (rows[i].logits) memcpy(rows[i].logits + k0, row, (size_t)p_nf[i] * 4);
      memcpy(rows[i].probs + k0, row + kVadChunk, (size_t)p_nf[i] * 4);
    }
  }
  return TTASR_OK;
}

static int vad_probs(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* ns, float* const* out_probs,
                     float* const* out_logits) {
  VadState* v = c->vad;
  if (!v || !v->finalized) return fail(c, TTASR_E_INVALID, "VAD weights not finalized (ttasr_vad_load_tensor, ttasr_vad_finalize first)");
  if (n < 1 || n > c->maxB) return fail(c, TTASR_E_INVALID, "n %d outside [1, max_batch = %d]", n, c->maxB);
  if (!pcm || !ns || !out_probs) return fail(c, TTASR_E_INVALID, "NULL argument");
  int64_t max_frames = 0;
  std::vector<VadRow> rows(n);
  for (int i = 0; i < n; ++i) {
    if (ns[i] < 0) return fail(c, TTASR_E_INVALID, "recording %d: negative length", i);
    if (ns[i] > 0 && (!pcm[i] || !out_probs[i] || (out_logits && !out_logits[i])))
      return fail(c, TTASR_E_INVALID, "recording %d: NULL pcm or output row with %lld samples", i, (long long)ns[i]);
    rows[i] = VadRow{nullptr, nullptr, 0, pcm[i], ns[i], (ns[i] + kVadWindow - 1) / kVadWindow, out_probs[i],
                     out_logits ? out_logits[i] : nullptr};
    max_frames = std::max(max_frames, rows[i].frames);
  }
  TRY(session_refusal(c));
  HIPCHK(c, hipSetDevice(c->device));
  if (max_frames == 0) return TTASR_OK;
  TRY(vad_pinned(c));
  TRY(vad_scratch(c, n));
  float* d_state = (float*)(v->scratch + vad_scratch_layout(v->scratch_files).state);
  HIPCHK(c, hipMemsetAsync(d_state, 0, (size_t)n * 256 * 4, c->stream));   // (h, c) = 0 at the start of every recording
  return vad_run(c, rows.data(), n, d_state, nullptr);
}

// ---- streams ----

// What wire streams need beside the float streams' blocks; a failed allocation leaves what exists in place for the next open.
static int vad_wire_blocks(ttasr_ctx* c, VadStreams* S) {
  TRY(S->hist.ensure(c, (size_t)2 * TTASR_VAD_MAX_STREAMS * 256 * 4, "wire stream history table"));
  TRY(S->wire_dev.ensure(c, kWireJobBytes + kWireRawBytes + kWireOutFloats * 4, "wire stream device pools"));
  TRY(S->wire_pin.ensure(c, kWireJobBytes + kWireRawBytes + kWireOutFloats * 4, "wire stream pinned pools"));
  if (S->wrows.empty()) {
    const size_t m = TTASR_VAD_MAX_STREAMS;
    S->wrows.resize(m); S->sub_ids.resize(m); S->sub_fin.resize(m); S->sub_frames.resize(m); S->sub_row.resize(m);
    S->sub_pcm.resize(m); S->sub_ns.resize(m); S->sub_probs.resize(m); S->sub_logits.resize(m);
  }
  return 0;
}

// wire == nullptr: a float stream.  Otherwise {rate, channels, format, pick} of a wire stream.
static int vad_stream_open(ttasr_ctx* c, const int32_t* wire, int32_t* out_id) {
  VadState* v = c->vad;
  if (!v || !v->finalized) return fail(c, TTASR_E_INVALID, "VAD weights not finalized (ttasr_vad_load_tensor, ttasr_vad_finalize first)");
  if (!out_id) return fail(c, TTASR_E_INVALID, "NULL argument");
  if (wire) {
    if (!sample_bytes(wire[2])) return fail(c, TTASR_E_INVALID, "format %d is no stream format (the six sample formats, A-law, mu-law)", wire[2]);
    if (wire[1] < 1 || wire[1] > 8) return fail(c, TTASR_E_INVALID, "%d channels outside [1, 8]", wire[1]);
    if (wire[3] < -1 || wire[3] >= wire[1]) return fail(c, TTASR_E_INVALID, "pick %d outside [-1, %d)", wire[3], wire[1]);
    if (!wire_plan(wire[0]).ok) return fail(c, TTASR_E_INVALID, "rate %d is no stream rate (ttasr_ingest_stream_len)", wire[0]);
  }
  TRY(session_refusal(c));   // the first open allocates
  HIPCHK(c, hipSetDevice(c->device));
  if (!v->streams) v->streams.reset(new VadStreams());
  VadStreams* S = v->streams.get();
  if (S->n_open >= TTASR_VAD_MAX_STREAMS) return fail(c, TTASR_E_INVALID, "all %d VAD streams of a context are open", S->n_open);
  WirePlan plan;
  if (wire) {
    TRY(vad_wire_blocks(c, S));
    TRY(wire_plan_dev(c, wire[0], &plan));
  }
  // everything a push ever needs: the table, the pinned staging, the scratch block for groups of max_batch rows
  TRY(S->table.ensure(c, (size_t)TTASR_VAD_MAX_STREAMS * 256 * 4, "VAD stream table"));
  TRY(vad_pinned(c));
  TRY(vad_scratch(c, c->maxB));
  int id = 0;
  while (S->s[id].open) ++id;   // n_open < TTASR_VAD_MAX_STREAMS: one is free
  VadStream& st = S->s[id];
  st.open = true;
  st.wire = wire != nullptr;
  if (wire) {
    st.plan = plan; st.channels = wire[1]; st.format = wire[2]; st.pick = wire[3]; st.fb = sample_bytes(wire[2]) * wire[1];
  }
  vad_stream_clear(st);
  ++S->n_open;
  *out_id = id;
  return TTASR_OK;
}

static VadStream* vad_stream_of(ttasr_ctx* c, int32_t id) {
  VadStreams* S = c->vad ? c->vad->streams.get() : nullptr;
  return S && id >= 0 && id < TTASR_VAD_MAX_STREAMS && S->s[id].open ? &S->s[id] : nullptr;
}

// wire: the kind of stream the caller may name - float streams for ttasr_vad_stream_push, wire streams for the chunks of
// ttasr_vad_stream_push_wire, whose 16 kHz samples enter here
static int vad_stream_push(ttasr_ctx* c, bool wire, int32_t n, const int32_t* ids, const float* const* pcm, const int64_t* ns,
                           const int32_t* finish, float* const* out_probs, float* const* out_logits, int32_t* out_frames) {
  VadState* v = c->vad;
  if (!v || !v->finalized) return fail(c, TTASR_E_INVALID, "VAD weights not finalized (ttasr_vad_load_tensor, ttasr_vad_finalize first)");
  VadStreams* S = v->streams.get();
  const int n_open = S ? S->n_open : 0;
  if (n < 1 || n > n_open) return fail(c, TTASR_E_INVALID, "n %d outside [1, open streams = %d]", n, n_open);
  if (!ids || !pcm || !ns || !out_probs || !out_frames) return fail(c, TTASR_E_INVALID, "NULL argument");
  VadRow* rows = S->rows.data();
  memset(S->seen.data(), 0, S->seen.size());
  for (int i = 0; i < n; ++i) {
    VadStream* st = vad_stream_of(c, ids[i]);
    if (!st) return fail(c, TTASR_E_INVALID, "row %d: stream %d is not open", i, ids[i]);
    if (st->wire != wire) return fail(c, TTASR_E_INVALID, "row %d: stream %d is a %s stream", i, ids[i], st->wire ? "wire" : "float");
    if (S->seen[ids[i]]) return fail(c, TTASR_E_INVALID, "row %d: stream %d appears twice in the call", i, ids[i]);
    S->seen[ids[i]] = 1;
    if (ns[i] < 0) return fail(c, TTASR_E_INVALID, "row %d: negative length", i);
    if (ns[i] > 0 && !pcm[i]) return fail(c, TTASR_E_INVALID, "row %d: NULL pcm with %lld samples", i, (long long)ns[i]);
    const int64_t total = st->n_pend + ns[i];
    int64_t frames = total / kVadWindow;
    if (finish && finish[i] && total % kVadWindow) ++frames;   // the zero-padded remainder
    if (frames > 0 && (!out_probs[i] || (out_logits && !out_logits[i])))
      return fail(c, TTASR_E_INVALID, "row %d: NULL output row for %lld values", i, (long long)frames);
    if (frames > INT32_MAX) return fail(c, TTASR_E_INVALID, "row %d: %lld frames in one push", i, (long long)frames);
    rows[i] = VadRow{st->ctx, st->pend, st->n_pend, pcm[i], ns[i], frames, out_probs[i], out_logits ? out_logits[i] : nullptr};
  }
  // from here on a failure leaves the streams of this call reset
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < n; ++i)
      if (rows[i].frames > 0 && S->s[ids[i]].fresh)
        HIPCHK(c, hipMemsetAsync(S->table + (size_t)ids[i] * 256, 0, 256 * 4, c->stream));
    for (int g0 = 0; g0 < n; g0 += c->maxB)
      TRY(vad_run(c, rows + g0, std::min(c->maxB, n - g0), S->table, ids + g0));
    return TTASR_OK;
  };
  const int rc = run();
  float ctx[kVadContext], pend[kVadWindow];
  for (int i = 0; i < n; ++i) {
    VadStream& st = S->s[ids[i]];
    const VadRow& r = rows[i];
    const int64_t total = r.n_head + r.n_pcm, done = r.frames * kVadWindow;
    out_frames[i] = rc == TTASR_OK ? (int32_t)r.frames : 0;
    if (rc != TTASR_OK || (finish && finish[i])) { vad_stream_clear(st); continue; }   // failed, or finished: as freshly opened
    // done <= total < done + 512: the last 64 evaluated samples and the new remainder, read before either is overwritten
    if (r.frames > 0) {
      vad_gather(ctx, r, done - kVadContext, kVadContext);
      vad_gather(pend, r, done, total - done);
      memcpy(st.ctx, ctx, sizeof ctx);
      memcpy(st.pend, pend, (size_t)(total - done) * 4);
      st.fresh = false;
    } else if (r.n_pcm > 0) {
      memcpy(st.pend + st.n_pend, r.pcm, (size_t)r.n_pcm * 4);
    }
    st.n_pend = (int)(total - done);
  }
  return rc;
}

// count bytes of a row's sequence [the stream's held bytes | the caller's] from byte pos on
static void wire_bytes(uint8_t* dst, const VadStream& st, const WireRow& r, int64_t pos, int64_t count) {
  const int64_t from_held = std::max<int64_t>(std::min<int64_t>(st.n_raw - pos, count), 0);
  if (from_held) memcpy(dst, st.raw + pos, (size_t)from_held);
  if (count > from_held) memcpy(dst + from_held, r.src + (pos + from_held - st.n_raw), (size_t)(count - from_held));
}

static int vad_stream_push_wire(ttasr_ctx* c, int32_t n, const int32_t* ids, const void* const* raw, const int64_t* n_bytes,
                                const int32_t* finish, float* const* out_pcm, const int64_t* out_cap, int64_t* out_len,
                                float* const* out_probs, float* const* out_logits, int32_t* out_frames) {
  VadState* v = c->vad;
  if (!v || !v->finalized) return fail(c, TTASR_E_INVALID, "VAD weights not finalized (ttasr_vad_load_tensor, ttasr_vad_finalize first)");
  VadStreams* S = v->streams.get();
  const int n_open = S ? S->n_open : 0;
  if (n < 1 || n > n_open) return fail(c, TTASR_E_INVALID, "n %d outside [1, open streams = %d]", n, n_open);
  if (!ids || !raw || !n_bytes || !out_len || !out_probs || !out_frames) return fail(c, TTASR_E_INVALID, "NULL argument");
  memset(S->seen.data(), 0, S->seen.size());
  for (int i = 0; i < n; ++i) {
    VadStream* st = vad_stream_of(c, ids[i]);
    if (!st) return fail(c, TTASR_E_INVALID, "row %d: stream %d is not open", i, ids[i]);
    if (!st->wire) return fail(c, TTASR_E_INVALID, "row %d: stream %d is a float stream", i, ids[i]);
    if (S->seen[ids[i]]) return fail(c, TTASR_E_INVALID, "row %d: stream %d appears twice in the call", i, ids[i]);
    S->seen[ids[i]] = 1;
    if (n_bytes[i] < 0) return fail(c, TTASR_E_INVALID, "row %d: negative length", i);
    if (n_bytes[i] > 0 && !raw[i]) return fail(c, TTASR_E_INVALID, "row %d: NULL raw with %lld bytes", i, (long long)n_bytes[i]);
    const bool fin = finish && finish[i];
    const int64_t frames = (st->n_raw + n_bytes[i]) / st->fb;
    if (st->F + frames > ((int64_t)1 << 40)) return fail(c, TTASR_E_INVALID, "row %d: more than 2^40 frames in a stream", i);
    const int64_t outs = wire_final(st->plan, st->F + frames, fin) - st->K;
    if (out_pcm && out_pcm[i] && (!out_cap || out_cap[i] < outs))
      return fail(c, TTASR_E_INVALID, "row %d: %lld samples become final, the row holds %lld", i, (long long)outs, (long long)(out_cap ? out_cap[i] : 0));
    const int64_t total = st->n_pend + outs;
    const int64_t vf = total / kVadWindow + (fin && total % kVadWindow ? 1 : 0);
    if (vf > 0 && (!out_probs[i] || (out_logits && !out_logits[i])))
      return fail(c, TTASR_E_INVALID, "row %d: NULL output row for %lld values", i, (long long)vf);
    if (vf > INT32_MAX) return fail(c, TTASR_E_INVALID, "row %d: %lld frames in one push", i, (long long)vf);
    S->wrows[i] = WireRow{(const uint8_t*)raw[i], n_bytes[i], 0, frames, 0, 0, fin, false};
  }
  // from here on a failure leaves the streams of this call reset
  hipStream_t s = c->stream;
  WireJob* const p_jobs = (WireJob*)S->wire_pin.get();
  uint8_t* const p_raw = (uint8_t*)S->wire_pin.get() + kWireJobBytes;
  float* const p_out = (float*)(S->wire_pin + kWireJobBytes + kWireRawBytes);
  const WireJob* const d_jobs = (const WireJob*)S->wire_dev.get();
  uint8_t* const d_raw = (uint8_t*)S->wire_dev.get() + kWireJobBytes;
  float* const d_out = (float*)(S->wire_dev + kWireJobBytes + kWireRawBytes);
  // every row's share of the pools: a chunk takes the frames whose bytes and whose results fit it (or option wire_chunk)
  const int64_t share_raw = (int64_t)(kWireRawBytes / n) & ~(int64_t)63, share_out = (int64_t)(kWireOutFloats / n);
  auto run = [&]() -> int {
    HIPCHK(c, hipSetDevice(c->device));
    for (int left = n; left > 0;) {
      int m = 0, sub = 0, max_tiles = 0, span = 1;
      int64_t raw_used = 0, out_used = 0;
      for (int i = 0; i < n; ++i) {
        WireRow& r = S->wrows[i];
        if (r.done) continue;
        VadStream& st = S->s[ids[i]];
        const WirePlan& P = st.plan;
        int64_t C = std::min<int64_t>(share_raw / st.fb, (share_out - 2) * P.down / P.up);
        if (c->wire_chunk > 0) C = std::min<int64_t>(C, c->wire_chunk);
        const int64_t cf = std::min(C, r.frames_left);
        const bool last = cf == r.frames_left;
        // without new frames (the tail a finish releases, walked in shares) the history stands and K moves alone
        const int64_t emit = std::min<int64_t>(wire_final(P, st.F + cf, last && r.fin) - st.K, share_out);
        if (cf > 0 || emit > 0) {
          wire_bytes(p_raw + raw_used, st, r, r.pos, cf * st.fb);
          WireJob& J = p_jobs[m++];
          J.taps = P.taps; J.raw_off = raw_used; J.f_old = st.F; J.k_begin = st.K;
          J.nf = (int32_t)cf; J.n_out = (int32_t)emit; J.out_off = (int32_t)out_used;
          J.hist_in = (st.half * TTASR_VAD_MAX_STREAMS + ids[i]) * 256;
          J.hist_out = cf > 0 ? ((st.half ^ 1) * TTASR_VAD_MAX_STREAMS + ids[i]) * 256 : -1;
          J.up = P.up; J.down = P.down; J.half = P.half; J.L = P.L; J.H = P.H; J.tile = P.tile;
          J.channels = st.channels; J.format = st.format; J.pick = st.pick;
          max_tiles = std::max<int>(max_tiles, (int)((emit + P.tile - 1) / P.tile));
          span = std::max<int>(span, P.taps ? (int)ingest_span(P.tile, P.up, P.down, P.half) : P.tile);
          raw_used += (cf * st.fb + 63) & ~(int64_t)63;
        }
        r.done = last && st.K + emit == wire_final(P, st.F + cf, r.fin);
        if (emit > 0 || (r.done && r.fin)) {
          S->sub_row[sub] = i; S->sub_ids[sub] = ids[i]; S->sub_fin[sub] = r.done && r.fin;
          S->sub_pcm[sub] = p_out + out_used; S->sub_ns[sub] = emit;
          S->sub_probs[sub] = out_probs[i] ? out_probs[i] + r.vad_done : nullptr;
          S->sub_logits[sub] = out_logits && out_logits[i] ? out_logits[i] + r.vad_done : nullptr;
          ++sub;
        }
        if (r.done) {   // the bytes behind the last whole frame stay with the stream (a finish drops them with everything else)
          const int64_t end = st.n_raw + r.n_src, keep = end - (r.pos + cf * st.fb);
          uint8_t held[64];
          wire_bytes(held, st, r, end - keep, keep);
          memcpy(st.raw, held, (size_t)keep);
          st.n_raw = (int)keep;
          --left;
        } else {
          r.pos += cf * st.fb;
        }
        r.frames_left -= cf;
        st.F += cf; st.K += emit;
        if (cf > 0) st.half ^= 1;
        out_used += emit;
      }
      if (m > 0) {
        HIPCHK(c, hipMemcpyAsync((void*)d_jobs, p_jobs, (size_t)m * sizeof(WireJob), hipMemcpyHostToDevice, s));
        if (raw_used) HIPCHK(c, hipMemcpyAsync(d_raw, p_raw, (size_t)raw_used, hipMemcpyHostToDevice, s));
        launch_wire(d_jobs, m, max_tiles, span, d_raw, d_out, S->hist, s);
        if (out_used) HIPCHK(c, hipMemcpyAsync(p_out, d_out, (size_t)out_used * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        HIPCHK(c, hipGetLastError());
      }
      if (sub == 0) continue;
      for (int k = 0; k < sub; ++k) {
        WireRow& r = S->wrows[S->sub_row[k]];
        float* const dst = out_pcm ? out_pcm[S->sub_row[k]] : nullptr;
        if (dst && S->sub_ns[k]) memcpy(dst + r.pcm_done, S->sub_pcm[k], (size_t)S->sub_ns[k] * 4);
        r.pcm_done += S->sub_ns[k];
      }
      TRY(vad_stream_push(c, true, sub, S->sub_ids.data(), S->sub_pcm.data(), S->sub_ns.data(), S->sub_fin.data(),
                          S->sub_probs.data(), out_logits ? S->sub_logits.data() : nullptr, S->sub_frames.data()));
      for (int k = 0; k < sub; ++k) S->wrows[S->sub_row[k]].vad_done += S->sub_frames[k];
    }
    return TTASR_OK;
  };
  const int rc = run();
  for (int i = 0; i < n; ++i) {
    out_len[i] = rc == TTASR_OK ? S->wrows[i].pcm_done : 0;
    out_frames[i] = rc == TTASR_OK ? S->wrows[i].vad_done : 0;
    if (rc != TTASR_OK) vad_stream_clear(S->s[ids[i]]);
  }
  return rc;
}

}  // namespace ttasr_detail

extern "C" {

int ttasr_vad_load_tensor(ttasr_ctx* c, const char* name, const float* data, const int64_t* dims, int32_t ndim) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  if (!name || !data || !dims || ndim < 1 || ndim > 3) return fail(c, name && data && dims ? TTASR_E_WEIGHTS : TTASR_E_INVALID, "VAD tensor: bad argument");
  TRY(session_refusal(c));
  return vad_load(c, name, data, dims, ndim);
  });
}

int ttasr_vad_finalize(ttasr_ctx* c) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  TRY(session_refusal(c));
  return vad_finalize(c);
  });
}

int ttasr_vad_probs(ttasr_ctx* c, int32_t n, const float* const* pcm, const int64_t* n_samples, float* const* out_probs,
                    float* const* out_logits) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return vad_probs(c, n, pcm, n_samples, out_probs, out_logits);
  });
}

int ttasr_vad_stream_open(ttasr_ctx* c, int32_t* out_id) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return vad_stream_open(c, nullptr, out_id);
  });
}

int ttasr_vad_stream_open_wire(ttasr_ctx* c, int32_t rate, int32_t channels, int32_t format, int32_t pick, int32_t* out_id) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  const int32_t wire[4] = {rate, channels, format, pick};
  return vad_stream_open(c, wire, out_id);
  });
}

int ttasr_vad_stream_push_wire(ttasr_ctx* c, int32_t n, const int32_t* ids, const void* const* raw, const int64_t* n_bytes,
                               const int32_t* finish, float* const* out_pcm, const int64_t* out_pcm_cap, int64_t* out_pcm_len,
                               float* const* out_probs, float* const* out_logits, int32_t* out_frames) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return vad_stream_push_wire(c, n, ids, raw, n_bytes, finish, out_pcm, out_pcm_cap, out_pcm_len, out_probs, out_logits, out_frames);
  });
}

int ttasr_vad_stream_reset(ttasr_ctx* c, int32_t id) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  VadStream* st = vad_stream_of(c, id);
  if (!st) return fail(c, TTASR_E_INVALID, "VAD stream %d is not open", id);
  vad_stream_clear(*st);
  return TTASR_OK;
  });
}

int ttasr_vad_stream_close(ttasr_ctx* c, int32_t id) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  VadStream* st = vad_stream_of(c, id);
  if (!st) return fail(c, TTASR_E_INVALID, "VAD stream %d is not open", id);
  st->open = false;
  --c->vad->streams->n_open;
  return TTASR_OK;
  });
}

int ttasr_vad_stream_push(ttasr_ctx* c, int32_t n, const int32_t* ids, const float* const* pcm, const int64_t* n_samples,
                          const int32_t* finish, float* const* out_probs, float* const* out_logits, int32_t* out_frames) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return vad_stream_push(c, false, n, ids, pcm, n_samples, finish, out_probs, out_logits, out_frames);
  });
}

}  // extern "C"
