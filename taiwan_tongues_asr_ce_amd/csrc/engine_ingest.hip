// libttasr: file ingest behind the C ABI (one of the engine translation units, see engine_ctx.hpp): the filter design in double,
// the per-rate tap tables of a context, its device and pinned chunk slots, the IMA scratch block, and the chunk loop of
// ttasr_ingest_pcm / ttasr_ingest_wave.  The kernels are kernels_ingest.hip; the result is the text of include/ttasr.h.  Nothing here touches mel, encoder, search or graph state, and
// no model weights are needed: the call's only shared resource is the context's stream.
#include "engine_ctx.hpp"
#include "ingest.hpp"
#include "flac.hpp"

#include <chrono>

namespace ttasr_detail {

constexpr int kIngestSlots = 4;                       // chunks in flight: staging copy, upload, kernel and download of neighbours overlap
constexpr size_t kIngestInBytes = (size_t)8 << 20;    // raw bytes of one chunk slot
constexpr size_t kIngestOutFloats = (size_t)1 << 20;  // results of one chunk slot
constexpr int64_t kIngestMaxFrames = (int64_t)1 << 40;
constexpr size_t kIngestScratchBytes = (size_t)8 << 20;   // decoded int16 of one IMA chunk (the stream runs chunk after chunk: one block)
constexpr int kImaMaxBlockAlign = 65536;
// FLAC: the decoded chunk (left-justified int16 / int32 [samples][channels]) and the lanes' int32 work rows of the same shape, each
// 32 MiB = 16 of the largest legal frames (65535 samples x 8 channels x 4 B): a frame, and the frames the filter's halo touches on
// both sides, always fit.  A chunk has at most kFlacMaxChunkFrames FLAC frames: one status word each, per slot.
constexpr size_t kFlacScratchBytes = (size_t)32 << 20;
constexpr int64_t kFlacMaxChunkFrames = 65536;

static bool is_pcm(int32_t f) { return f >= TTASR_PCM_U8 && f <= TTASR_PCM_F64; }
static bool is_g711(int32_t f) { return f == TTASR_PCM_ALAW || f == TTASR_PCM_ULAW; }

// What a rate decides: the ratio, the filter and the tile.  ok = false: the rate is not accepted.
struct IngestPlan {
  bool ok = false, filter = false;
  int up = 1, down = 1, half = 0, N = 0, L = 0, tile = kIngestMaxTile, span = kIngestMaxTile;
};

static int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

static IngestPlan ingest_plan(int32_t rate) {
  IngestPlan p;
  if (rate < 1) return p;
  const int g = gcd_i(rate, 16000);
  p.up = 16000 / g; p.down = rate / g;
  const int R = std::max(p.up, p.down);
  if (R > kIngestMaxR) return p;
  p.ok = true;
  if (rate == 16000) return p;   // convert and downmix only
  p.filter = true;
  p.half = 10 * R; p.N = 2 * p.half + 1; p.L = (p.N + p.up - 1) / p.up;
  // the longest tile (a multiple of the workgroup) whose span fits the usual LDS budget; ratios whose shortest such tile does not
  // fit take the large budget, with as many outputs as fit there
  p.tile = 0;
  for (int t = kIngestMaxTile; t >= kIngestThreads && !p.tile; t -= kIngestThreads)
    if (ingest_span(t, p.up, p.down, p.half) <= kIngestSpan) p.tile = t;
  if (!p.tile) {
    p.tile = kIngestThreads;
    while (p.tile > 1 && ingest_span(p.tile, p.up, p.down, p.half) > kIngestSpanMax) --p.tile;
  }
  p.span = (int)ingest_span(p.tile, p.up, p.down, p.half);
  return p;
}

static double bessel_i0(double x) {   // power series: sum_k ((x / 2)^k / k!)^2
  const double q = x * x / 4;
  double term = 1, sum = 1;
  for (int k = 1; k < 500 && term > 1e-20 * sum; ++k) { term *= q / ((double)k * k); sum += term; }
  return sum;
}

// h[m] = up w[m] / sum(w), w[m] = (1 / R) sinc((m - half) / R) kaiser_{N, 5}(m): scipy's firwin(N, 1 / R, window = ("kaiser", 5)) * up
static std::vector<double> ingest_design(const IngestPlan& p) {
  const int R = std::max(p.up, p.down);
  const double pi = 3.14159265358979323846, beta = 5.0, i0b = bessel_i0(beta);
  std::vector<double> w(p.N);
  double sum = 0;
  for (int m = 0; m < p.N; ++m) {
    const double x = (double)(m - p.half) / R, r = (double)(m - p.half) / p.half;
    const double sinc = x == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
    w[m] = sinc / R * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    sum += w[m];
  }
  for (double& v : w) v = v * p.up / sum;
  return w;
}

struct IngestFilter { IngestPlan plan; DevBlock<float> dev; };

struct IngestState {
  std::map<int32_t, IngestFilter> filters;   // per rate: the phase-major table [up][L] on the device (its own allocation)
  DevBlock<> dev;                            // [kIngestSlots] raw | [kIngestSlots] results
  PinBlock<> pinned;                         // the same layout in pinned host memory
  DevBlock<int16_t> scratch;                 // kIngestScratchBytes: the decoded chunk of an IMA recording (first IMA call)
  DevBlock<> flac_dev;                       // decoded chunk | work rows (kFlacScratchBytes each) | [kIngestSlots] status words (first FLAC call)
  PinBlock<int32_t> flac_status;             // pinned: [kIngestSlots][kFlacMaxChunkFrames] status words
  Event done[kIngestSlots];
};

void ingest_free(ttasr_ctx* c) {
  delete c->ingest;
  c->ingest = nullptr;
}

static int ingest_blocks(ttasr_ctx* c) {
  IngestState* g = c->ingest;
  const size_t bytes = kIngestSlots * (kIngestInBytes + kIngestOutFloats * 4);
  TRY(g->dev.ensure(c, bytes, "ingest device slots"));
  TRY(g->pinned.ensure(c, bytes, "ingest pinned staging"));
  for (auto& e : g->done) TRY(event_create(c, e, hipEventDisableTiming));
  return 0;
}

// The table of `rate` on the device, designed and uploaded by the first call that brings the rate.
static int ingest_filter_dev(ttasr_ctx* c, int32_t rate, const IngestFilter** out) {
  IngestState* g = c->ingest;
  auto it = g->filters.find(rate);
  if (it == g->filters.end()) {
    IngestFilter f; f.plan = ingest_plan(rate);
    if (f.plan.filter) {
      const std::vector<double> h = ingest_design(f.plan);
      std::vector<float> t((size_t)f.plan.up * f.plan.L, 0.0f);
      for (int m = 0; m < f.plan.N; ++m) t[(size_t)(m % f.plan.up) * f.plan.L + m / f.plan.up] = (float)h[m];
      TRY(f.dev.ensure(c, t.size() * 4, "ingest taps"));
      const hipError_t e2 = hipMemcpy(f.dev, t.data(), t.size() * 4, hipMemcpyHostToDevice);   // `t` is a stack temporary
      if (e2 != hipSuccess) return fail(c, TTASR_E_HIP, "ingest taps of rate %d: %s", rate, hipGetErrorString(e2));
    }
    it = g->filters.emplace(rate, std::move(f)).first;
  }
  *out = &it->second;
  return 0;
}

static int64_t ceil_div(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }   // b > 0
static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ---- wire streams: what engine_vad.hip needs of a rate ----

WirePlan wire_plan(int32_t rate) {
  WirePlan w;
  const IngestPlan p = ingest_plan(rate);
  if (!p.ok) return w;
  w.up = p.up; w.down = p.down; w.half = p.half; w.L = p.L; w.H = 2 * p.half / p.up;
  if (w.H > 255) return w;   // one row of the history table
  // the longest tile of at most 1024 outputs (a push is short: more, smaller workgroups) whose span fits the usual LDS budget
  w.tile = 1024;
  while (w.tile > kIngestThreads && (p.filter ? ingest_span(w.tile, p.up, p.down, p.half) : w.tile) > kWireSpan) w.tile -= kIngestThreads;
  w.ok = true;
  return w;
}

int wire_plan_dev(ttasr_ctx* c, int32_t rate, WirePlan* out) {
  WirePlan w = wire_plan(rate);
  if (!w.ok) return fail(c, TTASR_E_INVALID, "rate %d is no stream rate (ttasr_ingest_stream_len)", rate);
  if (!c->ingest) c->ingest = new IngestState();
  const IngestFilter* f = nullptr;
  TRY(ingest_filter_dev(c, rate, &f));
  w.taps = f->dev;
  *out = w;
  return 0;
}

int64_t wire_final(const WirePlan& p, int64_t n_frames, bool finished) {
  if (finished) return ceil_div(n_frames * p.up, p.down);
  return std::max<int64_t>(0, ceil_div(n_frames * p.up - p.half, p.down));
}

struct IngestPending {
  bool live = false; float* dst = nullptr; size_t n = 0;
  int rec = 0; int64_t frame0 = 0, n_status = 0;   // FLAC: the recording, the chunk's first FLAC frame and its number of status words
};

static int ingest_scratch(ttasr_ctx* c) { return c->ingest->scratch.ensure(c, kIngestScratchBytes, "ingest IMA scratch"); }

static int ingest_flac_scratch(ttasr_ctx* c) {
  IngestState* g = c->ingest;
  const size_t status = (size_t)kIngestSlots * kFlacMaxChunkFrames * 4;
  TRY(g->flac_dev.ensure(c, 2 * kFlacScratchBytes + status, "ingest FLAC scratch"));
  return g->flac_status.ensure(c, status, "ingest FLAC status words");
}

// A FLAC recording's chunks are whole FLAC frames.  Chunk [a, b) of the frame table owns the outputs whose index k satisfies
// first sample of a <= k down / up < first sample of b; what it stages is its own frames and those the filter's halo touches.
struct FlacCut { int64_t kb = 0, ke = 0, fa = 0, fb = -1, bytes = 0, samples = 0; bool ok = true; };

struct FlacCutter {
  const flac::Probe& B;
  const IngestPlan& P;
  int64_t nfr, ch;
  int64_t n_out() const { return ceil_div(nfr * P.up, P.down); }
  int64_t frame_of(int64_t smp) const {   // the frame that holds sample smp
    const std::vector<flac::FrameRec>& F = B.frames;
    int64_t lo = 0, hi = (int64_t)F.size() - 1;
    while (lo < hi) { const int64_t m = (lo + hi + 1) / 2; if (F[m].first <= smp) lo = m; else hi = m - 1; }
    return lo;
  }
  FlacCut cut(int64_t a, int64_t b) const {
    const std::vector<flac::FrameRec>& F = B.frames;
    FlacCut u;
    const int64_t sb = b < (int64_t)F.size() ? F[b].first : B.samples, no = n_out();
    u.kb = std::min(ceil_div(F[a].first * P.up, P.down), no);
    u.ke = sb >= nfr ? no : std::min(ceil_div(sb * P.up, P.down), no);
    if (u.ke <= u.kb) return u;
    const int64_t lo = std::max<int64_t>(ceil_div(u.kb * P.down - P.half, P.up), 0);
    const int64_t hi = std::min<int64_t>(floor_div((u.ke - 1) * P.down + P.half, P.up), nfr - 1);
    u.fa = frame_of(lo); u.fb = std::max(frame_of(hi), u.fa);
    u.samples = F[u.fb].first + F[u.fb].bs - F[u.fa].first;
    u.bytes = F[u.fb].off + F[u.fb].len - F[u.fa].off;
    const int64_t nt = u.fb - u.fa + 1;
    u.ok = nt <= kFlacMaxChunkFrames && nt * (int64_t)sizeof(FlacRec) + u.bytes <= (int64_t)kIngestInBytes &&
           u.samples * ch * 4 <= (int64_t)kFlacScratchBytes && u.ke - u.kb <= (int64_t)kIngestOutFloats;
    return u;
  }
  // the first frame that does not fit the staging slots even as a chunk of its own, or -1: the chunk loop relies on there being none
  int64_t misfit() const {
    const std::vector<flac::FrameRec>& F = B.frames;
    for (int64_t a = 0; a < (int64_t)F.size() && F[a].first < nfr; ++a)
      if (!cut(a, a + 1).ok) return a;
    return -1;
  }
};

// The call behind both entry points.  `wave` = ttasr_ingest_wave: the coded formats are legal, n_bytes is there and checked,
// block_align and pick may be NULL (no IMA recording / the mean everywhere).  ttasr_ingest_pcm: the three are NULL.
static int ingest_run(ttasr_ctx* c, bool wave, int32_t n, const void* const* raw, const int64_t* n_bytes, const int64_t* n_frames,
                      const int32_t* rate, const int32_t* channels, const int32_t* format, const int32_t* block_align,
                      const int32_t* pick, float* const* out) {
  if (n < 0) return fail(c, TTASR_E_INVALID, "n %d is negative", n);
  if (n == 0) return TTASR_OK;
  if (!raw || !n_frames || !rate || !channels || !format || !out || (wave && !n_bytes)) return fail(c, TTASR_E_INVALID, "NULL argument");
  bool any_ima = false, any_flac = false;
  std::vector<flac::Probe> probes;           // of the FLAC recordings, by recording: STREAMINFO and the frame table of the scan
  for (int i = 0; i < n; ++i) {
    if (n_frames[i] < 0 || n_frames[i] > kIngestMaxFrames) return fail(c, TTASR_E_INVALID, "recording %d: %lld frames outside [0, 2^40]", i, (long long)n_frames[i]);
    if (channels[i] < 1 || channels[i] > 8) return fail(c, TTASR_E_INVALID, "recording %d: %d channels outside [1, 8]", i, channels[i]);
    const bool ima = wave && format[i] == TTASR_PCM_IMA4;
    const bool fl = wave && format[i] == TTASR_PCM_FLAC;
    if (!is_pcm(format[i]) && !(wave && (is_g711(format[i]) || ima || fl))) return fail(c, TTASR_E_INVALID, "recording %d: unknown sample format %d", i, format[i]);
    if (wave) {
      const int32_t pk = pick ? pick[i] : -1;
      if (pk < -1 || pk >= channels[i]) return fail(c, TTASR_E_INVALID, "recording %d: pick %d outside [-1, %d)", i, pk, channels[i]);
      if (n_bytes[i] < 0) return fail(c, TTASR_E_INVALID, "recording %d: %lld bytes", i, (long long)n_bytes[i]);
      int64_t held;
      if (fl) {
        if (!raw[i]) return fail(c, TTASR_E_INVALID, "recording %d: NULL FLAC bytes", i);
        if (probes.empty()) probes.resize(n);
        char why[200];
        if (!flac::scan((const uint8_t*)raw[i], n_bytes[i], probes[i], why, (int32_t)sizeof why)) return fail(c, TTASR_E_INVALID, "recording %d: FLAC: %s", i, why);
        const flac::Stream& si = probes[i].si;
        if (rate[i] != si.rate || channels[i] != si.channels)
          return fail(c, TTASR_E_INVALID, "recording %d: FLAC stream of %d Hz and %d channels given as %d Hz and %d channels", i, si.rate, si.channels, rate[i], channels[i]);
        held = probes[i].samples;
        any_flac = true;
      } else if (ima) {
        if (!block_align) return fail(c, TTASR_E_INVALID, "recording %d: IMA ADPCM without block_align", i);
        const int32_t ba = block_align[i];
        if (ba < 8 * channels[i] || ba > kImaMaxBlockAlign || ba % (4 * channels[i]))
          return fail(c, TTASR_E_INVALID, "recording %d: IMA block_align %d is no multiple of %d in [%d, %d]", i, ba, 4 * channels[i], 8 * channels[i], kImaMaxBlockAlign);
        held = n_bytes[i] / ba * ima_spb(ba, channels[i]);
        any_ima = true;
      } else {
        held = n_bytes[i] / (sample_bytes(format[i]) * (int64_t)channels[i]);
      }
      if (n_frames[i] > held) return fail(c, TTASR_E_INVALID, "recording %d: %lld frames, but %lld bytes hold %lld", i, (long long)n_frames[i], (long long)n_bytes[i], (long long)held);
    }
    if (!ingest_plan(rate[i]).ok)
      return fail(c, TTASR_E_INVALID, "recording %d: rate %d is not accepted (max(up, down) of the ratio to 16000 must be at most %d)", i, rate[i], kIngestMaxR);
    if (fl && n_frames[i] > 0) {   // every chunk of the chunk loop is known to fit before anything is enqueued
      const IngestPlan plan = ingest_plan(rate[i]);
      const int64_t a = FlacCutter{probes[i], plan, n_frames[i], channels[i]}.misfit();
      if (a >= 0)
        return fail(c, TTASR_E_INVALID, "recording %d: FLAC frame %lld (%u samples at rate %d) does not fit the staging slots", i, (long long)a, probes[i].frames[a].bs, rate[i]);
    }
    if (n_frames[i] > 0 && (!raw[i] || !out[i])) return fail(c, TTASR_E_INVALID, "recording %d: NULL sample or output row with %lld frames", i, (long long)n_frames[i]);
  }
  TRY(session_refusal(c));
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->ingest) c->ingest = new IngestState();
  IngestState* g = c->ingest;
  TRY(ingest_blocks(c));
  if (any_ima) TRY(ingest_scratch(c));
  if (any_flac) TRY(ingest_flac_scratch(c));
  hipStream_t s = c->stream;
  char* const d_in = g->dev; char* const d_out = g->dev + kIngestSlots * kIngestInBytes;
  char* const p_in = g->pinned; char* const p_out = g->pinned + kIngestSlots * kIngestInBytes;
  IngestPending pend[kIngestSlots];
  const bool timing = c->ingest_timing;
  using clk = std::chrono::steady_clock;
  double ms[4] = {0, 0, 0, 0};   // staging copies (both directions, host) | upload | kernel | download
  auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  auto retire = [&](int slot) -> int {   // the slot's results to the caller's row
    if (!pend[slot].live) return 0;
    HIPCHK(c, hipEventSynchronize(g->done[slot]));
    pend[slot].live = false;
    const int32_t* st = g->flac_status ? g->flac_status + (size_t)slot * kFlacMaxChunkFrames : nullptr;
    for (int64_t k = 0; k < pend[slot].n_status; ++k)
      if (st[k]) {   // a frame whose content is illegal although its CRC holds: nothing of the call stays in flight
        (void)hipStreamSynchronize(s);
        return fail(c, TTASR_E_INVALID, "recording %d: FLAC frame %lld: %s", pend[slot].rec, (long long)(pend[slot].frame0 + k), flac::status_text(st[k]));
      }
    const auto t0 = clk::now();
    memcpy(pend[slot].dst, p_out + (size_t)slot * kIngestOutFloats * 4, pend[slot].n * 4);
    ms[0] += since(t0);
    pend[slot].live = false;
    return 0;
  };
  int64_t job = 0;
  // A FLAC recording, chunk after chunk (FlacCutter): the frames a chunk's outputs read go up as one byte range (frames lie back
  // to back in the file) behind their table, the pre-pass decodes them into the scratch block, and the filter kernel reads that
  // as s16 / s32.
  auto run_flac = [&](int i, const IngestFilter* f) -> int {
    const IngestPlan& P = f->plan;
    const flac::Probe& B = probes[i];
    const std::vector<flac::FrameRec>& F = B.frames;
    const int64_t NF = (int64_t)F.size(), nfr = n_frames[i];
    const int fmt = B.si.bits <= 16 ? TTASR_PCM_S16 : TTASR_PCM_S32;
    const FlacCutter cutter{B, P, nfr, channels[i]};
    const int64_t target = c->ingest_chunk > 0 ? c->ingest_chunk : INT64_MAX;   // rounded up to whole FLAC frames
    for (int64_t a = 0, b; a < NF && F[a].first < nfr; a = b) {
      b = a + 1;
      FlacCut u = cutter.cut(a, b);   // fits: the validation above saw to it
      while (b < NF && F[b].first < nfr && F[b].first - F[a].first < target) {
        const FlacCut v = cutter.cut(a, b + 1);
        if (!v.ok) break;
        u = v; ++b;
      }
      if (u.ke <= u.kb) continue;
      const int slot = (int)(job % kIngestSlots);
      ++job;
      TRY(retire(slot));
      const int64_t nt = u.fb - u.fa + 1, tbytes = nt * (int64_t)sizeof(FlacRec);
      char* const pin = p_in + (size_t)slot * kIngestInBytes;
      char* const din = d_in + (size_t)slot * kIngestInBytes;
      auto t0 = clk::now();
      FlacRec* recs = (FlacRec*)pin;
      for (int64_t k = 0; k < nt; ++k) {
        const flac::FrameRec& r = F[u.fa + k];
        recs[k] = FlacRec{(uint32_t)(r.off - F[u.fa].off), (uint32_t)r.len, (uint32_t)(r.first - F[u.fa].first), r.bs};
      }
      memcpy(pin + tbytes, (const char*)raw[i] + F[u.fa].off, (size_t)u.bytes);
      ms[0] += since(t0);
      t0 = clk::now();
      HIPCHK(c, hipMemcpyAsync(din, pin, (size_t)(tbytes + u.bytes), hipMemcpyHostToDevice, s));
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[1] += since(t0); t0 = clk::now(); }
      int32_t* const d_status = (int32_t*)(g->flac_dev + 2 * kFlacScratchBytes) + (size_t)slot * kFlacMaxChunkFrames;
      FlacJob D;
      D.raw = (const uint8_t*)(din + tbytes); D.table = (const FlacRec*)din;
      D.out = g->flac_dev; D.work = (int32_t*)(g->flac_dev + kFlacScratchBytes); D.status = d_status;
      D.raw_bytes = u.bytes; D.cap_samples = u.samples;
      D.n_frames = (int32_t)nt; D.rate = B.si.rate; D.channels = B.si.channels; D.bits = B.si.bits;
      launch_flac_decode(D, s);
      IngestJob J;
      J.raw = (const uint8_t*)g->flac_dev.get();
      J.out = (float*)(d_out + (size_t)slot * kIngestOutFloats * 4);
      J.taps = f->dev;
      J.n_frames = nfr; J.f0 = F[u.fa].first; J.k_begin = u.kb; J.nf = (int32_t)u.samples; J.n_out = (int32_t)(u.ke - u.kb);
      J.up = P.up; J.down = P.down; J.half = P.half; J.L = P.L; J.channels = channels[i]; J.format = fmt;
      J.tile = P.tile; J.span = P.span; J.pick = pick ? pick[i] : -1;
      launch_ingest(J, s);
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[2] += since(t0); t0 = clk::now(); }
      HIPCHK(c, hipMemcpyAsync(p_out + (size_t)slot * kIngestOutFloats * 4, J.out, (size_t)J.n_out * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(g->flac_status + (size_t)slot * kFlacMaxChunkFrames, d_status, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[3] += since(t0); }
      HIPCHK(c, hipEventRecord(g->done[slot], s));
      pend[slot].live = true; pend[slot].dst = out[i] + u.kb; pend[slot].n = (size_t)J.n_out;
      pend[slot].rec = i; pend[slot].frame0 = u.fa; pend[slot].n_status = nt;
    }
    return 0;
  };
  for (int i = 0; i < n; ++i) {
    if (n_frames[i] == 0) continue;
    const IngestFilter* f = nullptr;
    TRY(ingest_filter_dev(c, rate[i], &f));
    if (format[i] == TTASR_PCM_FLAC) { TRY(run_flac(i, f)); continue; }
    const IngestPlan& P = f->plan;
    const bool ima = format[i] == TTASR_PCM_IMA4;
    const int64_t ba = ima ? block_align[i] : 0, spb = ima ? ima_spb((int)ba, channels[i]) : 1;
    const int64_t nfr = n_frames[i], fb = ima ? 0 : (int64_t)sample_bytes(format[i]) * channels[i];
    const int64_t halo = 2 * (int64_t)P.half / P.up + 2;
    const int64_t n_out = ceil_div(nfr * P.up, P.down);
    // frames per chunk: what the raw slot holds beside the halo and what the result slot holds, or the option when it is smaller.
    // IMA: whole blocks - the raw slot holds blocks, the scratch block their int16, and the halo may reach into one more block on
    // either side; the option is rounded up to blocks
    int64_t C;
    if (ima) {
      const int64_t cap = std::min<int64_t>((int64_t)kIngestInBytes / ba * spb, (int64_t)kIngestScratchBytes / (2 * channels[i]));
      C = std::min<int64_t>(cap - halo - 2 * spb, ((int64_t)kIngestOutFloats - 2) * P.down / P.up) / spb * spb;
      if (c->ingest_chunk > 0) C = std::min<int64_t>(C, ceil_div(c->ingest_chunk, spb) * spb);
    } else {
      C = std::min<int64_t>((int64_t)kIngestInBytes / fb - halo, ((int64_t)kIngestOutFloats - 2) * P.down / P.up);
      if (c->ingest_chunk > 0) C = std::min<int64_t>(C, c->ingest_chunk);
    }
    if (C < 1) return fail(c, TTASR_E_INVALID, "recording %d: no chunk of rate %d fits the staging slots", i, rate[i]);
    const int64_t chunks = ceil_div(nfr, C);
    for (int64_t ch = 0; ch < chunks; ++ch, ++job) {
      const int64_t kb = std::min(ceil_div(ch * C * P.up, P.down), n_out);
      const int64_t ke = ch + 1 == chunks ? n_out : std::min(ceil_div((ch + 1) * C * P.up, P.down), n_out);
      if (ke <= kb) continue;
      // the frames these outputs read, cut at the ends of the recording
      const int64_t lo = std::max<int64_t>(ceil_div(kb * P.down - P.half, P.up), 0);
      const int64_t hi = std::min<int64_t>(floor_div((ke - 1) * P.down + P.half, P.up), nfr - 1);
      int64_t nf = std::max<int64_t>(hi - lo + 1, 0);
      // what goes up: the frames [lo, lo + nf), or for IMA the whole blocks that hold them - the staged range then begins with
      // block b_lo's first frame and ends with the recording or with block b_hi
      int64_t f0 = lo, src = lo * fb, bytes = nf * fb, n_blk = 0;
      if (ima) {
        const int64_t b_lo = lo / spb, b_hi = nf ? hi / spb : b_lo - 1;
        n_blk = b_hi - b_lo + 1;
        f0 = b_lo * spb; src = b_lo * ba; bytes = n_blk * ba;
        nf = n_blk ? std::min<int64_t>((b_hi + 1) * spb, nfr) - f0 : 0;
        if (nf * 2 * channels[i] > (int64_t)kIngestScratchBytes)
          return fail(c, TTASR_E_INVALID, "recording %d: chunk %lld exceeds the IMA scratch (%lld frames)", i, (long long)ch, (long long)nf);
      }
      if (bytes > (int64_t)kIngestInBytes || ke - kb > (int64_t)kIngestOutFloats || (wave && src + bytes > n_bytes[i]))
        return fail(c, TTASR_E_INVALID, "recording %d: chunk %lld exceeds its slot (%lld frames, %lld outputs)", i, (long long)ch, (long long)nf, (long long)(ke - kb));
      const int slot = (int)(job % kIngestSlots);
      TRY(retire(slot));
      auto t0 = clk::now();
      memcpy(p_in + (size_t)slot * kIngestInBytes, (const char*)raw[i] + src, (size_t)bytes);
      ms[0] += since(t0);
      t0 = clk::now();
      if (bytes) HIPCHK(c, hipMemcpyAsync(d_in + (size_t)slot * kIngestInBytes, p_in + (size_t)slot * kIngestInBytes, (size_t)bytes, hipMemcpyHostToDevice, s));
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[1] += since(t0); t0 = clk::now(); }
      IngestJob J;
      J.raw = (const uint8_t*)(d_in + (size_t)slot * kIngestInBytes);
      J.out = (float*)(d_out + (size_t)slot * kIngestOutFloats * 4);
      J.taps = f->dev;
      J.n_frames = nfr; J.f0 = f0; J.k_begin = kb; J.nf = (int32_t)nf; J.n_out = (int32_t)(ke - kb);
      J.up = P.up; J.down = P.down; J.half = P.half; J.L = P.L; J.channels = channels[i]; J.format = format[i];
      J.tile = P.tile; J.span = P.span; J.pick = pick ? pick[i] : -1;
      if (ima) {   // decode the staged blocks into the scratch block; the filter kernel reads that as s16
        ImaJob D;
        D.raw = J.raw; D.out = g->scratch; D.n_frames = nf;
        D.n_blocks = (int32_t)n_blk; D.channels = channels[i]; D.block_align = (int32_t)ba; D.spb = (int32_t)spb;
        launch_ima_decode(D, s);
        J.raw = (const uint8_t*)g->scratch.get(); J.format = TTASR_PCM_S16;
      }
      launch_ingest(J, s);
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[2] += since(t0); t0 = clk::now(); }
      HIPCHK(c, hipMemcpyAsync(p_out + (size_t)slot * kIngestOutFloats * 4, J.out, (size_t)J.n_out * 4, hipMemcpyDeviceToHost, s));
      if (timing) { HIPCHK(c, hipStreamSynchronize(s)); ms[3] += since(t0); }
      HIPCHK(c, hipEventRecord(g->done[slot], s));
      pend[slot].live = true; pend[slot].dst = out[i] + kb; pend[slot].n = (size_t)J.n_out; pend[slot].n_status = 0;
    }
  }
  for (int64_t k = 0; k < kIngestSlots; ++k) TRY(retire((int)((job + k) % kIngestSlots)));   // oldest first
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (timing) for (int k = 0; k < 4; ++k) c->phase_ms[k] = (float)ms[k];
  return TTASR_OK;
}

}  // namespace ttasr_detail

extern "C" {

int64_t ttasr_ingest_len(int32_t rate, int64_t n_frames) {
  const IngestPlan p = ingest_plan(rate);
  if (!p.ok || n_frames < 0 || n_frames > kIngestMaxFrames) return TTASR_E_INVALID;
  return (n_frames * p.up + p.down - 1) / p.down;
}

int64_t ttasr_ingest_stream_len(int32_t rate, int64_t n_frames, int32_t finished) {
  const WirePlan p = wire_plan(rate);
  if (!p.ok || n_frames < 0 || n_frames > kIngestMaxFrames) return TTASR_E_INVALID;
  return wire_final(p, n_frames, finished != 0);
}

int32_t ttasr_ingest_filter(int32_t rate, float* out, int32_t cap) {
  try {
    const IngestPlan p = ingest_plan(rate);
    if (!p.ok) return TTASR_E_INVALID;
    if (!p.filter) return 0;   // 16000: there is no filter
    if (out && cap > 0) {
      const std::vector<double> h = ingest_design(p);
      for (int m = 0; m < std::min(cap, p.N); ++m) out[m] = (float)h[m];
    }
    return p.N;
  } catch (...) {
    return TTASR_E_NOMEM;
  }
}

int ttasr_ingest_pcm(ttasr_ctx* c, int32_t n, const void* const* raw, const int64_t* n_frames, const int32_t* rate,
                     const int32_t* channels, const int32_t* format, float* const* out_pcm) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return ingest_run(c, false, n, raw, nullptr, n_frames, rate, channels, format, nullptr, nullptr, out_pcm);
  });
}

int ttasr_ingest_wave(ttasr_ctx* c, int32_t n, const void* const* raw, const int64_t* n_bytes, const int64_t* n_frames,
                      const int32_t* rate, const int32_t* channels, const int32_t* format, const int32_t* block_align,
                      const int32_t* pick, float* const* out_pcm) {
  return guarded(c, [&]() -> int {
  if (!c) return TTASR_E_INVALID;
  return ingest_run(c, true, n, raw, n_bytes, n_frames, rate, channels, format, block_align, pick, out_pcm);
  });
}

}  // extern "C"
