// libttasr host side, shared by the engine translation units (round 4: the 1 900-line engine.hip split into allocation /
// weight intake, schedules, search and the C ABI - no behaviour change): the context, the error / dispatch macros and the entry
// points the units call in each other.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ttasr.h"
#include "common.hpp"
#include "align_batch.hpp"
#include "beam_pages.hpp"
#include "prefill_tables.hpp"
#include "owned.hpp"
#include "seq_bias.hpp"

namespace ttasr_detail {

// The production policies of owned.hpp.  Memory: quiesce is the synchronisation of the context's stream, nomem is
// fail(c, TTASR_E_NOMEM, "<what> (<bytes> bytes): <error>") (both defined next to HIPCHK below); a failed allocation leaves no sticky error.
struct HipMem {
  static int quiesce(ttasr_ctx* c);
  static int nomem(ttasr_ctx* c, const char* what, size_t bytes, const char* err);
  static const char* text(hipError_t e) { if (e == hipSuccess) return nullptr; (void)hipGetLastError(); return hipGetErrorString(e); }
};
struct DeviceMem : HipMem {
  static const char* alloc(void** p, size_t bytes) { return text(hipMalloc(p, bytes)); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem : HipMem {
  static const char* alloc(void** p, size_t bytes) { return text(hipHostMalloc(p, bytes, hipHostMallocDefault)); }
  static void release(void* p) { (void)hipHostFree(p); }
};
struct EventKind { using type = hipEvent_t; static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); } };
struct StreamKind { using type = hipStream_t; static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); } };
template <class T = char> using DevBlock = Block<DeviceMem, T>;
template <class T = char> using PinBlock = Block<PinnedMem, T>;
using Event = Handle<EventKind>;         // created by event_create (below)
using OwnStream = Handle<StreamKind>;    // a stream its holder created: never an alias of the context's stream

extern thread_local std::string g_create_error;   // error text of a failed ttasr_create (engine_alloc.hip)

struct Slot {              // where one named tensor lands on the device
  void* dst = nullptr;     // T* (matrix kinds) or float* (vector kinds)
  int64_t rows = 0, cols = 0;
  int kind = 0;            // 0 matrix->T, 1 vector->f32, 2 conv [out][in][3] -> T [out][3][in], 3 f32 matrix
  float scale = 1.0f;
  bool loaded = false;
  void* sh_base = nullptr;  // bf16 mode, decoder matrices: fragment-packed copy for the skinny GEMM
  int sh_row_off = 0;
  int sh_rows_total = 0;    // rows of the whole packed matrix (a fused q/k/v matrix is packed as three parts): decides the block height
};

struct Session;            // continuous-batching session state (engine_refill.hip)
struct SegState;           // segmentation network: weights, scratch and staging of one context (engine_seg.hip)
struct SpkState;           // speaker-embedding network: weights, scratch and staging of one context (engine_spk.hip)
struct VadState;           // voice-activity network: weights, scratch, staging and streams of one context (engine_vad.hip)
struct EnhState;           // audio enhancement: the device block of one context (engine_enhance.hip)
struct IngestState;        // file ingest: tap tables per rate, the chunk slots and the IMA scratch of one context (engine_ingest.hip)
// What run_decode_rows reads about the rows of a step, and (with the batch, the mode and the e4m3 state) what a captured step
// graph is keyed on.  Installed and restored by SearchScope only.
struct StepShape {
  int kv_div = 1;            // rows per clip sharing one cross-KV (beam width); 1 for greedy
  int identity_pages = 1;    // page_table is the identity map (greedy): the self-attention kernel computes page ids
  bool rows_pos = false;     // per-row positions (continuous-batching session: row_pos instead of st.step)
  bool lang_rows = false;    // the language head runs behind the select of every step (greedy session armed by ttasr_session_detect_language)
  bool seq_bias = false;     // a sequence-bias table is installed: the bias kernel runs in front of the select of every step
  bool operator==(const StepShape& o) const {
    return kv_div == o.kv_div && identity_pages == o.identity_pages && rows_pos == o.rows_pos && lang_rows == o.lang_rows &&
           seq_bias == o.seq_bias;
  }
};
struct EncLayerW { float *ln1g, *ln1b, *bqkv, *bo, *ln2g, *ln2b, *b1, *b2; void *wqkv, *wo, *w1, *w2; };
struct DecLayerW {
  float *ln1g, *ln1b, *bqkv, *bo, *ln2g, *ln2b, *bqx, *bkvx, *box, *ln3g, *ln3b, *b1, *b2;
  void *wqkv, *wo, *wqx, *wkvx, *wox, *w1, *w2;
  void *wqkv_sh = nullptr, *wo_sh = nullptr, *wqx_sh = nullptr, *wox_sh = nullptr, *w1_sh = nullptr, *w2_sh = nullptr;
};

}  // namespace ttasr_detail
using namespace ttasr_detail;

struct ttasr_ctx {
  ttasr_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t cur = nullptr;      // stream the schedule helpers enqueue on
  std::string err;
  bool lowp = false;   // 16-bit storage mode (bf16 or fp16 weights / activations, f32 accumulate / LayerNorm / softmax)
  bool f16 = false;    // ... and the 16-bit format is IEEE fp16 (TTASR_COMPUTE_F16) instead of bf16
  bool finalized = false;
  bool force_basic = false;
  bool use_graph = true;
  size_t esz = 4;  // sizeof(T)
  int T = 0, F = 0, d = 0, H = 0, ffn = 0, V = 0, ldv = 0, M = 0, maxB = 0, n_samples = 0;
  int pages_per_seq = 0;
  std::vector<void*> allocs;
  struct Pool { char* base = nullptr; size_t cap = 0, used = 0; } small_pool, big_pool;  // bump arenas (see dalloc)
  size_t arena_hint = 0;   // rough device footprint of this context (bytes): picks the big-arena chunk size
  std::unordered_map<std::string, Slot> slots;

  // weights
  void *conv1_w = nullptr, *conv2_w = nullptr, *emb = nullptr, *dpos = nullptr, *emb_sh = nullptr;
  float *conv1_b = nullptr, *conv2_b = nullptr, *epos = nullptr, *elnf_g = nullptr, *elnf_b = nullptr, *dlnf_g = nullptr,
        *dlnf_b = nullptr;
  std::vector<EncLayerW> enc;
  std::vector<DecLayerW> dec;
  float* stage_f32 = nullptr;  // upload staging (destination layout, f32)
  float* stage_raw = nullptr;  // host uploads land here first (source layout)
  size_t stage_elems = 0;

  // mel constants
  float *filters = nullptr, *dcos = nullptr, *dsin = nullptr, *window = nullptr;

  // workspaces
  float* pcm_dev = nullptr; int64_t* nsamp_dev = nullptr; unsigned* clip_max = nullptr; int64_t* mel_geom = nullptr;
  float* mel = nullptr; void* mel_t = nullptr; void* c1 = nullptr;
  float* x = nullptr; void *h = nullptr, *qkv = nullptr, *att = nullptr, *mid = nullptr, *enc_out = nullptr;
  void* xkv = nullptr; int64_t xkv_layer_elems = 0, xkv_which_elems = 0;
  // option xkv_fp8 (opt-in serving mode, kernels_fp8.hip): an e4m3 copy of the cross-KV cache (same element strides, one byte per
  // value) + one f32 scale per (layer, K | V, clip, head); read by the decode step's cross-attention only
  // xkv_fp8: 0 off; 1 unshared greedy rows of a static pass only (sessions refused); 2 wherever a kernel for the copy exists -
  // shared rows (beam, sampled attempts) too, and in sessions, which quantise at admission
  int xkv_fp8 = 0; bool xkv8_valid = false; uint8_t* xkv8 = nullptr; float* xkv8_scale = nullptr;
  bool xattn_mq_fp8 = true;   // option xattn_mq_fp8 [1]: 0 = shared rows read the 16-bit cache under xkv_fp8 = 2 (A/B)
  void* pool = nullptr; int64_t pool_layer_elems = 0; int32_t* page_table = nullptr;
  float* xsplit_ws = nullptr;  // split-frame cross-attention (small batches)
  float* dx = nullptr; void *dh = nullptr, *dqkv = nullptr, *dq = nullptr, *datt = nullptr, *dmid = nullptr; float* logits = nullptr;
  float* rows_out = nullptr;
  // language detection (ttasr_detect_language): the span of the tied embedding the pass ends in and its device results -
  // probs [maxB][128] f32, span logits [maxB][128] f32, winners [maxB] i32 (rows packed at n_lang); allocated by the first call
  float* lang_out = nullptr; int lang_begin = 0, lang_n = 0; bool lang_want_logits = false;
  // ... inside a session (ttasr_session_detect_language): ONE block, allocated by the first armed session - pending flags [maxB],
  // placeholder slots [maxB], admission table [maxB][2], winners [maxB] (i32), probs [maxB][128], span logits [maxB][128] (f32; rows
  // packed at n_lang) - and the span and prompt stride the armed sessions' step graphs were captured with
  int32_t* lang_sess = nullptr; int sess_lang_begin = 0, sess_lang_n = 0, sess_lang_stride = 0;
  StepShape shape;           // the decode shape of the search that is running (SearchScope); the defaults between searches
  int32_t* pairs_dev = nullptr;  // beam search: copy-on-write page pairs
  float* topk_lp = nullptr; int32_t* topk_id = nullptr; int32_t* row_state = nullptr;  // beam search scratch
#ifdef TTASR_EXPERIMENTS
  int skip_mask = 0;  // TTASR_SKIP (experiment builds only): 1 LN, 2 decode GEMMs, 4 self-attn, 8 cross-attn, 16 select
#else
  static constexpr int skip_mask = 0;  // release builds cannot drop work from the decode step
#endif
  float* slab = nullptr;      // [16][maxB][3d] f32 partial tiles of the K-split decode GEMMs (bf16 mode)
  int ks_want[4] = {0, 0, 0, 0};  // option ksplit_out / _q / _qkv / _fc2: K slices of the out-proj / q / qkv / fc2 decode GEMMs (0 = automatic, 1 = unsplit)
  int gemm_force = 0;         // option enc_gemm = 1|2|3|4 (A/B testing of the encoder GEMM kernels)
  bool gemm_persistent = true;   // option enc_gemm_persistent [1]: the persistent 256x256 GEMM where a workgroup has >= 2 tiles (round 4: encoder + cross-KV 92.6 -> 89.1 ms, bit-identical)
  bool vocab_persistent = true;  // option vocab_persistent = 0: the one-workgroup-per-32-outputs kernel for the vocabulary projection (A/B)
  bool no_flash = false;      // option flash = 0
  int prefill_ns_min = 2;     // option prefill_ns_min: shortest prompt (positions before the last) whose <|startoftranscript|> position is taken
                              // from the prefill pass.  Round 3: 2 (was 16) - the small prefill pass now runs the decode-step launch plan
                              // (K-split GEMMs), so 3 prompt positions x 32 clips cost 6.4 ms against 8.8 ms as three steps
  bool enc_res_epilogue = false;  // option enc_residual_epilogue: keep the f32 residual add in the encoder GEMM epilogues (A/B testing)
  DecState st{}; int32_t* prompt_dev = nullptr; int32_t* plen_dev = nullptr; uint8_t* mask_dev = nullptr;
  // round 6: several contexts on one GPU may share ONE copy of the device weights (ttasr_create_shared: the pipelined folder
  // path runs pass i + 1's log-mel / encoder under pass i's decode from two contexts; a second private copy would double the
  // 5 GB of large-v3).  A sharer holds `weight_owner` and counts in the owner's `sharers`; an owner that is destroyed while
  // sharers live is only marked (`destroy_pending`) and freed by the last of them.  Weights are read-only once shared.
  ttasr_ctx* weight_owner = nullptr;
  std::atomic<int> sharers{0};
  bool destroy_pending = false;
  int32_t* row_cap_dev = nullptr;   // [maxB] per-row token budgets (st.row_cap; ttasr_generate_capped), "no budget" = 0x7f7f7f7f
  bool ragged_exit = true;          // option ragged_exit [1]: finished rows (st.done) leave the attention kernels of the decode step
                                    // (0: the static batch of rounds 1-5 - every row streams its cross-KV until the last one ends; A/B)
  RuleDyn* rule_dyn_dev = nullptr; RuleDyn rule_dyn_host{};  // per-window rule scalars read by select_kernel (common.hpp RuleDyn)
  PinBlock<int32_t> pinned_i32;  // host pinned scratch
  // beam search (round 6): every per-position host <-> device exchange goes through ONE pinned block - page tables, fed tokens,
  // row histories and copy-on-write pairs out, top-k candidates back - so the copies are truly asynchronous (a pageable source
  // makes hipMemcpyAsync stage and block: measured ~0.5 ms of host time per position in round 5's loop) and a searching position
  // costs ONE stream synchronisation instead of two.  The beam session's steps use the same block (BeamExchange below carves
  // it for either search): a context never runs a static search while a session is open (session_refusal).  Allocated by the
  // first search for the largest one this context can run; ttasr_destroy resets it before the stream goes.
  PinBlock<> pinned_beam;
  float beam_prof_ms[4]{0, 0, 0, 0};   // last beam search: host time enqueueing, waiting for the GPU, selecting candidates; positions
  int max_new_alloc = 0, max_prompt_alloc = 0;

  // continuous-batching session (engine_refill.hip): open between ttasr_session_begin[_beam] and ttasr_session_end
  ttasr_detail::Session* sess = nullptr;
  bool refill_overlap = false;    // option refill_overlap: encode the next clips on a second stream under the step graphs (opt-in:
                                  // a second stream = a second hardware queue, which makes processes sharing the GPU time-slice)
  int32_t* row_pos = nullptr;     // [maxB] per-row positions of the session (allocated by the first session)
  void* xkv_stage = nullptr;      // [dec_layers][2][maxB][H][T][64] T: the session's encoder writes the admitted clips' cross-KV here
  int32_t* admit_dev = nullptr;   // [maxB][3 + max_prompt_alloc] row-admission table (launch_admit_rows)
  int32_t* sess_sel = nullptr;    // [maxB][9] beam session: entries, temperatures, seeds and results of the independent-row kernel
  // prompt prefill at a session's admission (option session_prefill): 0 = off, N > 0 = clips with at least
  // N prefillable prompt positions get them from an admission pass.  The pass has its OWN activation workspace of kPrefillRowCap
  // rows (the encoder's is written by an overlapped encode from the second stream), its device tables and the all -1 head
  // selection of the f32 engine's per-row cross-attention: allocated by the first session that enables the option
  int session_prefill = 0;
  float* pf_x = nullptr; void *pf_h = nullptr, *pf_qkv = nullptr, *pf_att = nullptr, *pf_mid = nullptr;
  int32_t* pf_tab = nullptr; size_t pf_tab_words = 0; int* pf_sel = nullptr;
  // option align_packed: ttasr_session_align runs the PACKED pass of the admission (one fixed GEMM family,
  // work items cut from each sequence's own length) out of the pf_* workspace instead of the padded run_prefill; read at call time
  bool align_packed = false;

  // batched alignment (engine_align.hip): ONE device block for the pass's tables, softmax maps, cost matrices and spilled DTW
  // traces; allocated by the first call, grown to the largest request (ensure), reset by ttasr_destroy
  DevBlock<> align_dev;
  // sequence bias (ttasr_set_sequence_bias, seq_bias.hpp): ONE device block of fixed capacity - the table and the beam search's row
  // windows - allocated by the first install, reset by ttasr_destroy; seq_bias_n = sequences installed (0: no table, nothing of
  // the feature is launched)
  DevBlock<int32_t> seq_bias_dev;
  int seq_bias_n = 0;
  // ttasr_enc_attn_probe: ONE device block of its own - f32 staging, the operands in the engine type, the output with its guard
  // row, the frame-split workspace of the cross form - allocated by the first call, grown to the largest request, reset by
  // ttasr_destroy.  The encoder's and the decode step's own buffers are never touched.
  DevBlock<> enc_probe_dev;
  // voice-activity network (engine_vad.hip): created by the first ttasr_vad_load_tensor, freed by ttasr_destroy; per context,
  // outside the weight-share bookkeeping
  ttasr_detail::VadState* vad = nullptr;
  // file ingest (engine_ingest.hip): created by the first ttasr_ingest_pcm / ttasr_ingest_wave, freed by ttasr_destroy.  Options: ingest_chunk = input
  // frames per chunk (0: what the slots hold), ingest_timing = 1: the chunks run one after the other and the call leaves its
  // host-clock phase split in phase_ms
  ttasr_detail::IngestState* ingest = nullptr;
  int ingest_chunk = 0; bool ingest_timing = false;
  // segmentation network (engine_seg.hip): created by the first ttasr_seg_load_tensor, freed by ttasr_destroy.  Option seg_lstm_rows:
  // chunks per recurrence workgroup (0: the measured choice; 1, 2, 4 force one; results identical)
  ttasr_detail::SegState* seg = nullptr;
  int seg_lstm_rows = 0;
  // speaker-embedding network (engine_spk.hip): created by the first ttasr_spk_load_tensor, freed by ttasr_destroy
  ttasr_detail::SpkState* spk = nullptr;
  // audio enhancement (engine_enhance.hip): created by the first ttasr_enhance / ttasr_enhance_probe, freed by ttasr_destroy.  Option
  // enhance_chunk = samples per chunk (0: 2^22)
  ttasr_detail::EnhState* enhance = nullptr;
  int enhance_chunk = 0;
  int wire_chunk = 0;       // option wire_chunk: input frames of a row per internal chunk of ttasr_vad_stream_push_wire (0: what the pools hold)

  int B_mel = 0, B_enc = 0, B_dec = 0;
  std::atomic_flag busy = ATOMIC_FLAG_INIT;  // one call in flight per context: a second concurrent call is refused
  KernelOpts ko;            // the kernel-variant options of this context (common.hpp), handed to every launcher that picks a variant
  bool weights_packed = false;
  bool enc_ln_defer = true; // option enc_ln_defer = 0: every encoder LayerNorm folds its delta into the f32 residual stream (two read-modify-writes per layer; A/B testing, bit-identical)
  bool gemm_tail = true;    // option enc_gemm_tail = 0: plain 256-row tiling in the persistent encoder GEMM (A/B testing; bit-identical)
  bool xkv_grouped = true;  // option xkv_grouped = 0: one cross-KV GEMM launch per decoder layer instead of one grouped launch (A/B testing; bit-identical)
  bool multi_step = true;   // option multi_step_graph = 0: one graph replay per decode step (A/B testing)
  bool no_xsplit = false;   // option xsplit = 0: never split the cross-attention frames over workgroups (A/B testing)
  bool no_prefill = false;  // option prefill = 0: feed prompts token by token (A/B testing)
  bool prefill_tiled = false;  // option prefill_tiled: tiled encoder GEMMs in the prefill pass whatever the row count (A/B testing)
  Event ev[8];
  int32_t* probe_done = nullptr; float* probe_zero = nullptr;   // ttasr_cross_attn_probe: its own [maxB] finished flags and a [d] zero bias (allocated by the first call)
  // ttasr_self_attn_probe / ttasr_self_kv_*: an f32 and a T staging block of max(one pool layer, 512 x 3 d) elements, a T output
  // [512][d], [maxB] positions, a [3 d] zero bias and the packed pass's tables (allocated by the first call)
  float* sprobe_f32 = nullptr; void *sprobe_t = nullptr, *sprobe_out = nullptr; int32_t *sprobe_pos = nullptr, *sprobe_tab = nullptr;
  float* sprobe_zero = nullptr; int64_t sprobe_elems = 0;
  std::string bench_sig;    // signature of the kernel the last ttasr_bench_kernel call launched (ttasr_bench_kernel_signature)
  float phase_ms[4]{0, 0, 0, 0};
  // option enc_kernel_timing: one hipEvent after every launch of run_encoder / run_cross_kv, so the NEXT ttasr_encode also
  // reports where the phase went, in situ (class sums: ttasr_encoder_kernel_ms).  Off in the timed benchmark steps.
  bool enc_timing = false;
  std::vector<hipEvent_t> enc_ev;
  std::vector<int> enc_ev_class;
  float enc_class_ms[8]{0, 0, 0, 0, 0, 0, 0, 0};

  // decode-step graphs, keyed by everything that decides which kernels a captured step holds (engine_sched.hip step_graph)
  struct GraphKey {
    int B, mode, nsteps; StepShape shape; int fp8_live;
    bool operator==(const GraphKey& o) const { return B == o.B && mode == o.mode && nsteps == o.nsteps && shape == o.shape && fp8_live == o.fp8_live; }
  };
  struct Graph { GraphKey key; hipGraphExec_t exec; };
  std::vector<Graph> graphs;   // least recently used first
  static constexpr size_t kMaxGraphs = 32;   // per batch size up to four step graphs exist (1- / 4- / 8-step greedy, logits-only): 8 batch sizes stay resident
  RuleParams rp{};
};

namespace ttasr_detail {

int fail(ttasr_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, call)                                                                                       \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) return fail((c), TTASR_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                      __FILE__, __LINE__);                                                    \
  } while (0)

inline int HipMem::quiesce(ttasr_ctx* c) { HIPCHK(c, hipStreamSynchronize(c->stream)); return 0; }   // enqueued work may still read the block
inline int HipMem::nomem(ttasr_ctx* c, const char* what, size_t bytes, const char* err) {
  return fail(c, TTASR_E_NOMEM, "%s (%zu bytes): %s", what, bytes, err);
}
inline int event_create(ttasr_ctx* c, Event& e, unsigned flags = hipEventDefault) {
  if (!e) HIPCHK(c, hipEventCreateWithFlags(&e.h, flags));
  return 0;
}
inline int stream_create(ttasr_ctx* c, OwnStream& s) { HIPCHK(c, hipStreamCreateWithFlags(&s.h, hipStreamNonBlocking)); return 0; }
// bytes per sample of a format that arrives as samples - the six PCM formats in the order of their codes, A-law, mu-law - else 0
inline int sample_bytes(int32_t format) {
  static const int pcm[6] = {1, 2, 3, 4, 4, 8};
  if (format >= TTASR_PCM_U8 && format <= TTASR_PCM_F64) return pcm[format];
  return format == TTASR_PCM_ALAW || format == TTASR_PCM_ULAW ? 1 : 0;
}

// No C++ exception may cross the C ABI (std::bad_alloc from a host vector would otherwise terminate the caller's process)
template <class F>
inline int guarded(ttasr_ctx* c, F&& f) {
  // a context is not re-entrant (ttasr.h): a call that arrives while another is in flight on the same context is
  // refused instead of corrupting the search state (its error text is not stored: the other call owns c->err)
  struct Busy {
    ttasr_ctx* c; bool own;
    explicit Busy(ttasr_ctx* c_) : c(c_), own(c_ == nullptr || !c_->busy.test_and_set(std::memory_order_acquire)) {}
    ~Busy() { if (c && own) c->busy.clear(std::memory_order_release); }
  } busy(c);
  if (!busy.own) return TTASR_E_INVALID;
  g_launch_fault[0] = 0;
  try {
    const int rc = f();
    // a launcher that had no kernel for what it was asked (common.hpp launch_fault) launched nothing: the call's output is invalid
    if (g_launch_fault[0] && rc == TTASR_OK) return fail(c, TTASR_E_INVALID, "launcher refused: %s", g_launch_fault);
    return rc;
  } catch (const std::bad_alloc&) {
    return fail(c, TTASR_E_NOMEM, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(c, TTASR_E_INVALID, "C++ exception: %s", e.what());
  } catch (...) {
    return fail(c, TTASR_E_INVALID, "unknown C++ exception");
  }
}

// Device memory comes from a few large arenas, not one hipMalloc per tensor: the decode step is ~350 dependent launches
// whose first access is to a small, rarely touched buffer (LayerNorm gamma / beta, a bias, the residual rows).  With ~2500
// separate allocations every one of those sat on its own page, and after the ~10 GB a step streams (weights + cross-KV)
// each launch opened with an address-translation miss.  The small pool (< 1 MiB requests: every vector, every decode
// activation) is one 64 MiB block that stays translation- and cache-resident; matrices and KV pools come from 1 GiB+
// blocks that the driver can map with its largest page fragments.
template <typename P>
int dalloc(ttasr_ctx* c, P** p, size_t bytes, bool zero = true) {
  if (bytes == 0) bytes = 16;
  bytes = (bytes + 255) & ~(size_t)255;
  ttasr_ctx::Pool& pool = bytes < (1u << 20) ? c->small_pool : c->big_pool;
  // big chunks: 1 GiB for real models; small geometries (tests, streaming-size engines) open 64 MiB chunks instead of pinning a
  // gigabyte each - the hint is the footprint ttasr_create estimated for this context
  const size_t big_chunk = c->arena_hint >= ((size_t)1 << 30) ? (size_t)1 << 30 : (size_t)64 << 20;
  const size_t chunk = &pool == &c->small_pool ? (size_t)64 << 20 : big_chunk;
  if (bytes > chunk / 2) {
    // an oversize request gets its own allocation and leaves the active chunk (and its unused tail) in service
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(c, TTASR_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    c->allocs.push_back(q);
    if (zero) HIPCHK(c, hipMemsetAsync(q, 0, bytes, c->stream));
    *p = (P*)q;
    return 0;
  }
  if (pool.used + bytes > pool.cap) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, chunk);
    if (e != hipSuccess) return fail(c, TTASR_E_NOMEM, "hipMalloc(%zu) failed: %s", chunk, hipGetErrorString(e));
    c->allocs.push_back(q);
    pool.base = (char*)q; pool.cap = chunk; pool.used = 0;
  }
  void* q = pool.base + pool.used;
  pool.used += bytes;
  if (zero) HIPCHK(c, hipMemsetAsync(q, 0, bytes, c->stream));
  *p = (P*)q;
  return 0;
}
#define TRY(expr) do { int rc_ = (expr); if (rc_ != 0) return rc_; } while (0)
// Run CALL with T = the context's storage type (float | bf16_t | f16_t)
#define TT_DISPATCH(c_, CALL)                                   \
  do {                                                          \
    if (!(c_)->lowp) { using T = float; CALL; }                 \
    else if ((c_)->f16) { using T = f16_t; CALL; }              \
    else { using T = bf16_t; CALL; }                            \
  } while (0)

template <typename T>
GemmArgs lin_args(const void* A, const void* W, int M, int N, int K) {
  GemmArgs g; g.A = A; g.W = W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.epi.ldc = N;
  return g;
}

// in-situ kernel classes of the encoder phase (ttasr_encoder_kernel_ms)
enum EncClass { EC_CONV = 0, EC_LN = 1, EC_QKV = 2, EC_ATTN = 3, EC_OUT = 4, EC_FC1 = 5, EC_FC2 = 6, EC_XKV = 7 };
// Batched prompt prefill: positions 0..npos-1 of n_seq sequences in ONE pass (rows [sequence][position]) instead of
// npos token-by-token steps.  Only the self-attention K/V of those positions has to survive (no logits: every one of
// these positions is followed by another forced prompt token), so the pass borrows the encoder's activation
// workspaces, which are idle once the cross-KV is built.  Sequence s attends to the cross-KV of clip s / seq_per_clip.
// GEMMs go through the encoder dispatch (M = n_seq * npos rows; 256x256 MFMA tiles once M >= 256).
// Alignment variant (ttasr_align): one sequence of clip `al->clip`; the cross-attention rows of the selected
// (layer, head) pairs are written to al->probs, and the residual stream is left in c->x for the token log-probs.
// Batched form (ttasr_align_batch / ttasr_session_align): n_seq sequences padded to npos positions; sequence s reads the
// cross-KV slot seq_clip[s], its tokens come from `tokens` [n_seq][npos] and its self-attention K/V go to the pages
// page_table[s][..] (the pass never touches another row's pages); probs is [n_sel][n_seq * npos][T].
struct AlignOut {
  int clip;
  const int* sel;   // device [dec_layers][H]: index into probs or -1
  float* probs;     // device [n_sel][npos][T]
  const int* seq_clip = nullptr;          // device [n_seq], batched form only
  const int32_t* tokens = nullptr;        // device [n_seq][npos], batched form only
  const int32_t* page_table = nullptr;    // device [n_seq][pages_per_seq], batched form only
};

// ---- engine_alloc.hip: arenas, weight slots, workspaces, weight intake ----
int build_weights(ttasr_ctx* c);
int build_workspaces(ttasr_ctx* c);
int ingest_tensor(ttasr_ctx* c, const char* name, const void* src, int src_type, const int64_t* dims, int32_t ndim);

// ---- engine_sched.hip: the typed launch schedules (T = the context's storage type is dispatched inside) ----
void enc_mark(ttasr_ctx* c, int cls);
void sched_encoder(ttasr_ctx* c, int B);                       // conv stem, encoder layers, final LayerNorm, cross-KV
void sched_cross_kv(ttasr_ctx* c, int B);
void sched_prefill(ttasr_ctx* c, int n_seq, int npos, int seq_per_clip, int max_prompt, const AlignOut* al = nullptr);
// the packed alignment pass's extras on top of an admission pass: sel (device [dec_layers][H]: pair or -1) and sel_host (the same),
// maps (device [n_pairs][n_rows][T]) and stat (device [n_pairs][n_rows][2], 16-bit MFMA form only)
struct PackedAlign { const int32_t* sel; const int32_t* sel_host; float* maps; float* stat; int n_pairs; };
// the decoder layers over the packed rows of an admission pass, on the decode stream; al != nullptr: the alignment pass, whose
// selected heads leave finished softmax maps in al->maps and whose residual rows stay in c->pf_x
void sched_admit_prefill(ttasr_ctx* c, const PrefillPass& P, const PackedAlign* al = nullptr);
// one layer's cross-attention of that pass on caller-supplied query rows (ttasr_align_attn_probe): dq, datt [n_rows][d]
void sched_align_attn(ttasr_ctx* c, int layer, const PrefillPass& P, const void* dq, void* datt, const PackedAlign& al);
// final LayerNorm + vocabulary projection (the pass's GEMM family) + log p(target[r]) for packed rows [0, n_rows) of c->pf_x
void sched_packed_logprob(ttasr_ctx* c, int n_rows, const int32_t* target, float* out);
int prefill_workspace(ttasr_ctx* c);   // engine_refill.hip: the pf_* workspace, allocated by the first caller that needs it
int sched_prefill_no_speech(ttasr_ctx* c, int n_seq, int npos, int sot, int no_speech_tok);
void sched_gemm(ttasr_ctx* c, const GemmArgs& g);              // encoder-side GEMM dispatch (ttasr_bench_kernel)
void sched_dec_gemm(ttasr_ctx* c, const GemmArgs& g, const void* Wsh);
int prefill_positions(const ttasr_ctx* c, int min_plen, const ttasr_gen_opts* o, bool ns_from_prefill = false);
int step_graph(ttasr_ctx* c, int B, int mode, int nsteps = 1);
void sched_detect_rows(ttasr_ctx* c, int B);                  // decode pass of B rows that ends in the language head (mode 3), launched directly
// the decode step's cross-attention dispatch of `layer` for rows [0, n) on the context's stream (ttasr_cross_attn_probe)
void sched_cross_attn(ttasr_ctx* c, int layer, int n, int kv_div, const void* dq, void* datt, const SlabIn& sq, const int32_t* done);
// the encoder's self-attention dispatch on stream s: qkv T [B][T_][3 d] -> att T [B][T_][d] (run_encoder's choice; ttasr_enc_attn_probe)
void sched_enc_attn(ttasr_ctx* c, const void* qkv, void* att, int B, int T_, hipStream_t s);
void drop_graphs(ttasr_ctx* c);
void drop_rule_graphs(ttasr_ctx* c);
void drop_lang_graphs(ttasr_ctx* c);                          // the step graphs of armed sessions (StepShape::lang_rows)

// One 30-s window of a recording from frame `seek`: the samples its STFT reads - `lead` before the window (200, fewer at the file
// start), the window, 200 after, cut at the end of the file - and the geometry launch_mel takes: {lead, reflect_end, valid_frames}.
// The signal is reflected where the FILE ends if that is inside the span; the whole-file STFT drops its last frame (HF feature
// extractor :154).  Callers check seek against the recording first.
struct WindowSpan { int64_t first, n, geom[3]; };
inline WindowSpan window_span(const ttasr_ctx* c, int64_t file_samples, int64_t seek) {
  const int64_t start = seek * 160, lead = std::min<int64_t>(200, start);
  const int64_t left = file_samples - (start - lead), span = lead + c->n_samples + 200;
  return WindowSpan{start - lead, std::max<int64_t>(std::min(left, span), 0),
                    {lead, left < span ? left : ((int64_t)1 << 40), std::max<int64_t>(std::min<int64_t>(c->F, file_samples / 160 - seek), 0)}};
}

// ---- engine_refill.hip: the continuous-batching session (greedy and beam search) ----
int session_refusal(ttasr_ctx* c);   // TTASR_E_INVALID with a message while a session is open, else 0
void session_free(ttasr_ctx* c);     // ttasr_destroy: deletes the session, which owns its stream, events and pinned memory

// ---- engine_align.hip: the batched alignment pass (ttasr_align_batch, ttasr_session_align) ----
struct AlignBatch {   // the host arguments of ttasr_align_batch without the clips
  int n; const int32_t* tokens; const int32_t* n_tokens; int max_tokens; const int32_t* first_row; const int32_t* num_frames;
  const int32_t* pairs; int n_pairs; int medfilt; int32_t* out_start; float* out_lp; float* out_cost; float* out_weights;
};
int align_batch_validate(ttasr_ctx* c, const AlignBatch& a);
int align_batch_run(ttasr_ctx* c, const AlignBatch& a, const int32_t* slot /*[n]*/, const int32_t* pages /*[n][pages_per_seq]*/);
// the same call through the packed pass (option align_packed): every output of a sequence is a function of that sequence alone
int align_packed_run(ttasr_ctx* c, const AlignBatch& a, const int32_t* slot, const int32_t* pages);

// ---- engine_vad.hip: the voice-activity network (ttasr_vad_*) ----
void vad_free(ttasr_ctx* c);         // ttasr_destroy: deletes the state, which owns its side blocks (the weights live in the arenas)

// ---- engine_seg.hip: the segmentation network (ttasr_seg_*) ----
void seg_free(ttasr_ctx* c);         // ttasr_destroy: deletes the state, which owns its side blocks (the weights live in the arenas)

// ---- engine_spk.hip: the speaker-embedding network (ttasr_spk_*) ----
void spk_free(ttasr_ctx* c);         // ttasr_destroy: deletes the state, which owns its side blocks (the weights live in the arenas)

// ---- engine_enhance.hip: audio enhancement (ttasr_enhance*) ----
void enhance_free(ttasr_ctx* c);     // ttasr_destroy: deletes the state, which owns its device block

// ---- engine_ingest.hip: file ingest (ttasr_ingest_*) ----
void ingest_free(ttasr_ctx* c);      // ttasr_destroy: deletes the state, which owns its tap tables, chunk slots and events
// What a wire stream (engine_vad.hip) keeps of its rate: the ratio, the filter and its table on the device (taps == nullptr at
// 16000: no filter), H = floor(2 half / up) frames of history and the stream kernel's tile.  ok = false: not a stream rate.
struct WirePlan { bool ok = false; int up = 1, down = 1, half = 0, L = 0, H = 0, tile = 256; const float* taps = nullptr; };
WirePlan wire_plan(int32_t rate);                                // the arithmetic alone: no context, taps stay nullptr
int wire_plan_dev(ttasr_ctx* c, int32_t rate, WirePlan* out);    // ... with the table of the rate, built on first use (allocates)
int64_t wire_final(const WirePlan& p, int64_t n_frames, bool finished);   // K(F), or n_out(F) when finished

// ---- engine_search.hip: rules, options, greedy / sampled / beam search ----
// The decode shape of ONE search (a static search's call, or a session from begin to end / free): installs the StepShape and the
// prompt rows the select kernel forces; every exit - error returns included - restores the defaults (kv_div 1, identity pages,
// static positions, no prompt) and enqueues the clear of the rows' finished flags, which belong to the search: later step-level
// calls see live rows.
struct SearchScope {
  ttasr_ctx* c; int rows;
  SearchScope(ttasr_ctx* c_, StepShape shape, const int32_t* prompt, const int32_t* prompt_len, int rows_) : c(c_), rows(rows_) {
    c->shape = shape; c->st.prompt = prompt; c->st.prompt_len = prompt_len;
  }
  ~SearchScope() {
    c->shape = StepShape{}; c->st.prompt = nullptr; c->st.prompt_len = nullptr;
    (void)hipMemsetAsync(c->st.done, 0, (size_t)rows * 4, c->stream);
  }
  // arming a session for language detection changes which kernels its steps hold, not its rows: no other member moves
  void set_lang_rows(bool on) { c->shape.lang_rows = on; }
  SearchScope(const SearchScope&) = delete; SearchScope& operator=(const SearchScope&) = delete;
};
int check_ready(ttasr_ctx* c, int B);
int upload_rules(ttasr_ctx* c, const ttasr_gen_opts* o, int max_prompt);
int commit_rules(ttasr_ctx* c, const RuleParams& old);
int set_option(ttasr_ctx* c, const std::string& key, int v);
int reset_search(ttasr_ctx* c, int B);
// One prompt of a call: `len` tokens at `row`, 1 <= len <= max_prompt with room left in the text context, every id inside the
// vocabulary and, where the no-speech probability is wanted, *sot inside the prompt (sot = nullptr: not wanted).  i names the
// prompt in the error text.
int check_prompt(ttasr_ctx* c, int i, const int32_t* row, int len, int max_prompt, const int32_t* sot);
int generate_rows(ttasr_ctx* c, int R, int rows_per_clip, const int32_t* prompt, const int32_t* prompt_len, int max_prompt,
                  const ttasr_gen_opts* o, float temperature, uint32_t seed, int32_t* out_tokens, int32_t* out_len, float* out_lp,
                  float* out_ns, const int32_t* row_cap = nullptr /*host [R] per-row token budgets, each in [1, max_new_tokens]*/);
bool beam_select(const std::vector<std::vector<int>>& seqs, const std::vector<double>& sums, int r0, int beam, int K,
                 const float* lp, const int32_t* id, int eot, int max_cand, std::map<std::vector<int>, double>& finished,
                 std::vector<std::vector<int>>& nseq, std::vector<double>& nsum, std::vector<int>& src, int stride /*of the rows of lp / id*/);
int sample_pick(const float* lp, const int32_t* len, int n);
int beam_pick(const std::map<std::vector<int>, double>& finished, const std::vector<std::vector<int>>& seqs,
              const std::vector<double>& sums, int r0, int beam, int eot, int max_new, int32_t* out, double* out_sum);
// The pinned exchange block of one beam position (ttasr_ctx::pinned_beam) carved for R rows, K candidates per row: out go the
// page tables [R][pps], fed tokens, positions and finished flags [R], row histories [4][R] and copy-on-write pairs [2 R]; back
// come the candidates lp / id [R][K] and the no-speech values [R].  The session's independent-row kernel adds entries [4 R],
// temperatures [R] and seeds [R] out (contiguous in this order: they go out in one copy) and results [3 R] back.
struct BeamExchange {
  int32_t *tbl, *tok, *pos, *done, *state, *pairs; float* lp; int32_t* id; float* ns;
  int32_t* ent; float* temp; uint32_t* seed; float* sel;
  int32_t* win;   // sequence bias: the rows' last kSeqBiasW history tokens [R][kSeqBiasW], then their history lengths [R]
};
inline size_t beam_exchange_words(int R, int pps, int K) { return (size_t)R * (pps + 19 + 2 * K + kSeqBiasW + 1); }
int beam_exchange(ttasr_ctx* c, int R, int K, BeamExchange& x);   // allocates the block on first use
inline BeamRowState beam_row_state(const ttasr_ctx* c, int R) {
  return BeamRowState{c->row_state, c->row_state + R, c->row_state + 2 * R, c->row_state + 3 * R, c->mask_dev};
}
// the steps both searches enqueue alike around the decoder step: the copy-on-write page copies, the row histories the candidate
// kernels apply the rules from (length, last, penultimate, last timestamp), and the candidates of every row with their way back
int enqueue_page_copies(ttasr_ctx* c, const std::vector<int32_t>& pairs, const BeamExchange& x);
int enqueue_row_histories(ttasr_ctx* c, const std::vector<std::vector<int>>& seqs, int R, int timestamp_begin, const BeamExchange& x);
int enqueue_candidates(ttasr_ctx* c, int R, int K, bool no_speech, const BeamExchange& x);
// sequence bias: the window of every row from the newest tokens of its history (hist[r]: all of them, or at least the last
// kSeqBiasMaxLen; searching[r] == 0: the row is left alone), uploaded for the bias launch of enqueue_candidates.  Nothing happens
// without a table.
int enqueue_bias_windows(ttasr_ctx* c, const std::vector<std::vector<int>>& hist, const std::vector<char>& searching, int R, const BeamExchange& x);
// the table block's regions on the device
inline const int32_t* seq_bias_win(const ttasr_ctx* c) { return c->seq_bias_dev.get() + kSeqBiasWinAt; }
int seq_bias_refusal(ttasr_ctx* c);   // TTASR_E_INVALID with a message while a table is installed (sessions), else 0
int beam_search_impl(ttasr_ctx* c, int32_t A, int32_t beam, const int32_t* prompt, int32_t max_prompt, const int32_t* plens,
                     const int32_t* sots, const ttasr_gen_opts* o, float patience, int32_t* out_tokens, int32_t* out_len,
                     float* out_lp, float* out_ns);

}  // namespace ttasr_detail
