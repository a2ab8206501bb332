/*
 * ttasr.h - C ABI of the MI355X-native Whisper inference hot path (libttasr.so).
 *
 * Drop-in boundary.  The reference has no native FFI: its hot path is reached through the Python object
 * faster_whisper.WhisperModel (constructor asr_core.py:141, api/file_asr.py:188,
 * api/stt_streaming/src/asr/faster_whisper_asr.py:107-109; transcribe() asr_core.py:159-167,
 * api/file_asr.py:457-465, faster_whisper_asr.py:170-172), which internally binds the CTranslate2 C++
 * engine (ctranslate2.models.Whisper.encode / .generate).  The entry points below are what a binding
 * for that pair of calls needs: everything from float32 PCM to token ids.  Plain pointers and sizes only;
 * no torch / Python types.  INTEGRATION.md shows the ctypes stub on the reference side.
 *
 * Conventions: every function returns 0 on success, a negative TTASR_E_* otherwise, and never aborts the
 * process; ttasr_last_error() gives the message.  A context is bound to one GPU and one HIP stream and is
 * NOT re-entrant: one call in flight per context (the reference never issues concurrent transcribe()
 * calls on one model: file_asr.py:175, streaming_asr.py:85-86); a call arriving while another runs on the same context
 * returns TTASR_E_INVALID at once and leaves the running call untouched.  Different contexts are independent.
 * No C++ exception crosses this boundary.  All device memory (weights, paged KV
 * pools, workspaces) is owned by the context from ttasr_create to ttasr_destroy.
 * Pointers named *_host are caller-owned host buffers; `pcm` may be a host or device pointer as stated
 * by `pcm_on_device`.
 */
#ifndef TTASR_H_
#define TTASR_H_

#include <stdint.h>

/* The ONLY symbols libttasr.so exports: the library is built with -fvisibility=hidden (csrc/Makefile), so none of its internal
 * C++ names (kernel launchers, device stubs, helpers) can collide with anything else loaded into the host process
 * (torch, RCCL, other extensions). */
#define TTASR_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

#define TTASR_OK 0
#define TTASR_E_INVALID (-1)   /* bad argument / wrong call order */
#define TTASR_E_HIP (-2)       /* HIP runtime error (message holds hipGetErrorString) */
#define TTASR_E_NOMEM (-3)
#define TTASR_E_WEIGHTS (-4)   /* unknown / missing / mis-shaped tensor */

#define TTASR_COMPUTE_F32 0    /* f32 weights+activations, exact-f32 MFMA: the 1e-3 parity mode */
#define TTASR_COMPUTE_BF16 1   /* bf16 weights+activations, f32 accumulate/LN/softmax: throughput mode */
#define TTASR_COMPUTE_F16 2    /* fp16 weights+activations, f32 accumulate/LN/softmax/residual stream: the reference's GPU regime
                                * (compute_type="float16": asr_core.py:141, api/config.py:12, faster_whisper_asr.py:95); same
                                * kernels and schedules as bf16 with the f16 MFMA forms, 3 more mantissa bits */

typedef struct ttasr_ctx ttasr_ctx;

/* Model geometry (what CTranslate2 reads from config.json / model.bin of the `models/` directory,
 * faster_whisper_asr.py:38) plus engine sizing. */
typedef struct ttasr_config {
  int32_t n_mels;       /* 80 (tiny..large-v2) or 128 (large-v3) */
  int32_t n_audio_ctx;  /* encoder positions, 1500; mel frames per window = 2 * n_audio_ctx */
  int32_t d_model;
  int32_t n_heads;      /* head_dim = d_model / n_heads must be 64 */
  int32_t ffn_dim;
  int32_t enc_layers;
  int32_t dec_layers;
  int32_t vocab;
  int32_t n_text_ctx;   /* 448 */
  int32_t compute_type; /* TTASR_COMPUTE_* */
  int32_t max_batch;    /* largest B any call will use; sizes the KV pools and workspaces */
  int32_t reserved;
} ttasr_config;

/* Decoding rules: the logits-processor stack of the reference path (CTranslate2 generate() options
 * suppress_blank / suppress_tokens / max_initial_timestamp_index; same rules as HF
 * generation/logits_process.py:1816,1869,1909-2047). */
typedef struct ttasr_gen_opts {
  int32_t max_new_tokens;
  int32_t eot;
  int32_t no_timestamps;
  int32_t timestamp_begin;
  int32_t no_speech;                   /* token id, or -1: do not compute no-speech probability */
  int32_t sot_index;                   /* prompt position of <|startoftranscript|> */
  int32_t timestamps;                  /* 1: apply the timestamp rules */
  int32_t max_initial_timestamp_index; /* -1: none */
  int32_t suppress_eot;                /* 1: fixed-length decode (benchmark mode) */
  int32_t n_suppress;
  int32_t n_begin_suppress;
  int32_t check_interval;              /* host polls "all rows finished" every this many steps (>=1) */
  const int32_t* suppress;             /* host, n_suppress ids masked at every step */
  const int32_t* begin_suppress;       /* host, n_begin_suppress ids masked at the first sampled position */
} ttasr_gen_opts;

/* ---- lifetime ---------------------------------------------------------------------------------- */
/* Geometry limits (TTASR_E_INVALID otherwise): d_model <= 1280, vocab <= 53248 (every Whisper checkpoint: <= 1280, <= 51866),
 * n_mels % 8 == 0, ffn_dim % 64 == 0. */
TTASR_API int ttasr_create(const ttasr_config* cfg, int device_id, ttasr_ctx** out_ctx);
/* A further context on the SAME GPU that shares `owner`'s device weights instead of loading its own copy (round 6): own stream,
 * own KV pools / workspaces / search state / captured graphs / kernel options, sized for max_batch rows (<= 0: the owner's) -
 * and zero bytes of weights (3.1 GB + the 1.9 GB packed decoder copies of large-v3 stay resident once).  What a host needs to keep
 * two batches in flight on one GPU (pass i + 1's log-mel / encoder under pass i's latency-bound decode chain: +27 % audio-s/s,
 * DESIGN.md 4.11) - the reference's folder loop is strictly serial (asr_core.py:151).  The owner's weights must be finalized; from
 * then on they are read-only for every context that shares them (ttasr_load_tensor* return TTASR_E_INVALID).  Contexts may be
 * destroyed in any order: an owner that is destroyed first stays alive, unusable, until its last sharer is gone. */
TTASR_API int ttasr_create_shared(ttasr_ctx* owner, int32_t max_batch, ttasr_ctx** out_ctx);
TTASR_API void ttasr_destroy(ttasr_ctx* ctx);
/* Message of the last failing call on this context (ctx == NULL: last ttasr_create failure). */
TTASR_API const char* ttasr_last_error(const ttasr_ctx* ctx);
/* Version / build string, e.g. "ttasr 0.1 gfx950". */
TTASR_API const char* ttasr_version(void);

/* ---- weights (replaces WhisperModel.__init__'s model.bin load) ---------------------------------- */
/* One tensor, float32 host data, HF state-dict name (model.encoder.conv1.weight, ...).  The engine
 * converts to its device layout (bf16 cast, QKV fusion, conv tap re-ordering, q pre-scaling by 1/8). */
TTASR_API int ttasr_load_tensor(ttasr_ctx* ctx, const char* name, const float* data_host, const int64_t* dims, int32_t ndim);
/* The same for a tensor that is already in DEVICE memory of this context's GPU (e.g. the bucket an RCCL broadcast just
 * filled: multi-GPU start-up moves every weight GPU-to-GPU over xGMI, in bf16 where the engine stores bf16, and never
 * stages it through a host): data_dev holds float32 (TTASR_DTYPE_F32), raw bfloat16 bits (TTASR_DTYPE_BF16) or IEEE half bits
 * (TTASR_DTYPE_F16) in the
 * HF layout.  Must be complete (the caller's stream synchronised) when the call is made.  The reference's
 * WhisperModel(..., device="cuda") does this copy inside CTranslate2 (asr_core.py:141). */
#define TTASR_DTYPE_F32 0
#define TTASR_DTYPE_BF16 1
#define TTASR_DTYPE_F16 2
TTASR_API int ttasr_load_tensor_device(ttasr_ctx* ctx, const char* name, const void* data_dev, int32_t dtype, const int64_t* dims,
                             int32_t ndim);
/* Checks every tensor arrived; must precede any compute call. */
TTASR_API int ttasr_finalize_weights(ttasr_ctx* ctx);

/* ---- a5: log-mel front end ----------------------------------------------------------------------- */
/* pcm: B clips, clip b at pcm + b*pcm_stride, n_samples[b] valid samples (zero-padded / trimmed to one
 * window = 2*n_audio_ctx*160 samples).  Result stays resident for ttasr_encode; if out_mel_host != NULL
 * it also receives float32 [B][n_mels][2*n_audio_ctx]. */
TTASR_API int ttasr_log_mel(ttasr_ctx* ctx, const float* pcm, int64_t pcm_stride, const int64_t* n_samples_host, int32_t B,
                  int32_t pcm_on_device, float* out_mel_host);
/* File-level form (faster-whisper computes the features of the WHOLE recording once and the 30-s window loop slices
 * them: generate_segments, called from WhisperModel.transcribe at asr_core.py:159-167): B windows, window b belonging to
 * the recording file_pcm_of_host[b][0..file_samples_of_host[b]) (the same pointer for windows of one file; different files
 * when several files advance in lock step) and starting at its frame seek_frames_host[b] (10-ms frames).  Each window's
 * frames are those of the whole-file STFT (true neighbour samples across window boundaries, reflection only at the ends
 * of the file), frames beyond the end of the recording are 0 in feature space (pad_or_trim of the feature slice), and the
 * dynamic-range floor is max - 8 of floor_max_host[b] when given (the caller passes the whole-file maximum, obtained from
 * a first pass with out_window_max_host) instead of the window's own maximum.  out_window_max_host (optional) receives
 * each window's log10-mel maximum over its valid frames.  Result resident for ttasr_encode like ttasr_log_mel. */
TTASR_API int ttasr_log_mel_windows(ttasr_ctx* ctx, const float* const* file_pcm_of_host, const int64_t* file_samples_of_host,
                          const int64_t* seek_frames_host, int32_t B, const float* floor_max_host, float* out_window_max_host,
                          float* out_mel_host);
/* The same with windows that may END before the recording does (clip_timestamps of the window loop): window b keeps the
 * whole-file STFT's frames [seek, seek + min(n_frames_host[b], 2*n_audio_ctx, frames left in the file)).  The cut limits which
 * frames are valid, not which samples are read: the frames just before the cut see their true neighbour samples BEYOND it, so the
 * kept frames are bit for bit those of the uncut window.  Every later frame is 0 in feature space (pad_or_trim of the feature
 * slice features[:, seek:seek + n]) and out_window_max_host covers the kept frames only.  n_frames_host[b] < 1 (or NULL):
 * TTASR_E_INVALID.  ttasr_log_mel_windows is this call without a cut. */
TTASR_API int ttasr_log_mel_windows_cut(ttasr_ctx* ctx, const float* const* file_pcm_of_host, const int64_t* file_samples_of_host,
                          const int64_t* seek_frames_host, int32_t B, const float* floor_max_host, float* out_window_max_host,
                          float* out_mel_host, const int64_t* n_frames_host);
/* Test hook: place a caller-computed mel [B][n_mels][2*n_audio_ctx] as the encoder input. */
TTASR_API int ttasr_set_mel(ttasr_ctx* ctx, const float* mel_host, int32_t B);

/* ---- a6-a8: encoder + cross-attention K/V (ctranslate2 Whisper.encode) ------------------------- */
/* Runs the conv stem, the encoder stack and the per-decoder-layer cross K/V projection for the B clips
 * whose mel is resident.  out_enc_host (optional) receives float32 [B][n_audio_ctx][d_model]. */
TTASR_API int ttasr_encode(ttasr_ctx* ctx, int32_t B, float* out_enc_host);
/* Test hooks. */
TTASR_API int ttasr_set_encoder_output(ttasr_ctx* ctx, const float* enc_host, int32_t B); /* then builds cross K/V */
TTASR_API int ttasr_get_cross_kv(ttasr_ctx* ctx, int32_t layer, int32_t which /*0 K, 1 V*/, int32_t B, float* out_host /*[B][H][T][64]*/);
/* Known-answer hooks for the cross-attention kernels (tests/test_gpu_xattn_kernels.py).
 *
 * The e4m3 copy of the cross-KV cache (option "xkv_fp8") as it is resident: the raw OCP e4m3fn bytes of block (layer, which) of the
 * first B clips and the f32 scale of every (clip, head) block (value = code x scale).  TTASR_E_INVALID when no valid copy exists
 * (option off, f32 engine, no encode since the option was set); otherwise the argument checks of the 16-bit readback above.
 * Read-only, and therefore also allowed while a session is open: B then counts cross-KV slots (up to max_batch), and which clip
 * a slot holds is what the session's row report says (greedy: row = slot; beam: group = slot). */
TTASR_API int ttasr_get_cross_kv_fp8(ttasr_ctx* ctx, int32_t layer, int32_t which /*0 K, 1 V*/, int32_t B,
                                     uint8_t* out_codes_host /*[B][H][T][64]*/, float* out_scale_host /*[B][H]*/);
/* The decode step's cross-attention of `layer`, ONCE, on caller-supplied queries against the resident cache: n_rows rows, row r
 * reading clip r / kv_div (kv_div >= 1 divides n_rows; n_rows / kv_div clips must be resident).  n_slab = 0: q_host is f32
 * [n_rows][d_model], cast to the engine type.  n_slab = 1..4 (16-bit engines): q_host is n_slab f32 partial tiles
 * [n_slab][n_rows][d_model], summed by the kernel (with a zero bias) the way the step's kernels sum the K-split q GEMM.  The query
 * is used as given: the 1/8 of the attention lives in the q weights, not in the kernels.  done_host: optional int32 [n_rows],
 * nonzero = finished row (copied to a flag array of the hook's own).  out_host: f32 [n_rows][d_model]; the device output is
 * zero-filled before the launch, so rows a kernel does not write come back 0.  The launch goes through the very function the
 * step calls to choose its kernel, so every option that steers the step ("xkv_fp8", "xattn_mq_fp8", "xsplit", "xattn_pipeline",
 * "xattn_nontemporal", "xattn_deep_items", "xattn_mq_slices") steers this call; sig_buf (optional, sig_len bytes) receives the
 * signature of what ran, in the spelling of the bench signature call below plus the slice count of the frame-split forms.
 * Refused in an open session and without resident encoder state; search state and captured step graphs are not touched. */
TTASR_API int ttasr_cross_attn_probe(ttasr_ctx* ctx, int32_t layer, int32_t n_rows, int32_t kv_div, const float* q_host, int32_t n_slab,
                                     const int32_t* done_host, float* out_host, char* sig_buf, int32_t sig_len);
/* The cross-attention of the PACKED alignment pass (option "align_packed"; tests/test_gpu_align_packed.py)
 * of `layer`, once, on caller-supplied queries: n_seq sequences packed one after the other, sequence i with lens_host[i] >= 1 rows
 * (at most 512 rows in all) reading the resident cross-KV of clip slots_host[i].  q_host: f32 [rows][d_model], cast to the engine
 * type and used as given.  head_pair_host [n_heads]: -1, or the index in [0, n_pairs) of the map this head writes (every index
 * exactly once).  No weight of the layer is involved.  out_host: f32 [rows][d_model], the attention output;
 * out_maps_host: f32 [n_pairs][rows][T], every selected head's softmax over the T frames of the audio window, per packed row
 * (may be NULL when n_pairs = 0).  16-bit engines run the MFMA kernel of the admission pass - its map-writing instantiation when
 * a head is selected - and the finishing kernel; the f32 engine and option "generic_kernels" run the per-row kernel: what
 * ttasr_session_align launches under "align_packed" = 1.  Refused in an open session and without resident encoder state; search
 * state and captured step graphs are not touched. */
TTASR_API int ttasr_align_attn_probe(ttasr_ctx* ctx, int32_t layer, int32_t n_seq, const int32_t* lens_host, const int32_t* slots_host,
                                     const float* q_host, const int32_t* head_pair_host, int32_t n_pairs, float* out_host,
                                     float* out_maps_host);
/* Known-answer hooks for the decoder SELF-attention kernels over the paged KV pool (tests/test_gpu_self_attn_kernels.py; DESIGN.md
 * section 4.28).  The pool of one layer is [page][2 (K, V)][n_heads][16 positions][64] with max_batch x pages_per_seq pages,
 * pages_per_seq = ceil(n_text_ctx / 16); page images below have that layout, [n_pages][2][n_heads][16][64] f32.  All four calls are
 * refused in an open session.  They overwrite search state: after any of them the decode state (KV pool, positions, finished
 * flags) is UNDEFINED until ttasr_decode_reset, a generate call or a session start; the device page table is the identity again
 * when ttasr_self_attn_probe returns, captured step graphs are not touched.
 *
 * ttasr_self_kv_fill: every element of `layer` (-1: of every layer) becomes `pattern` - its 32 bits on an f32 engine, its low 16
 * bits on a 16-bit engine (a NaN pattern makes a read outside a row's history visible).
 * ttasr_self_kv_set: positions [0, n) (1 <= n <= 16) of the listed pages of `layer`, K and V of every head, from the page images
 * kv_host (cast to the engine type; positions >= n of the images are ignored and their pool elements keep their bits).
 * ttasr_self_kv_get: the listed pages (pages_host NULL and n_pages = all pages: the whole layer in pool order) as f32, exactly. */
TTASR_API int ttasr_self_kv_fill(ttasr_ctx* ctx, int32_t layer, uint32_t pattern);
TTASR_API int ttasr_self_kv_set(ttasr_ctx* ctx, int32_t layer, const int32_t* pages_host, int32_t n_pages, int32_t n, const float* kv_host);
TTASR_API int ttasr_self_kv_get(ttasr_ctx* ctx, int32_t layer, const int32_t* pages_host, int32_t n_pages, float* out_host);
/* ONE launch of a named form of the self-attention on caller-supplied rows, through the launcher the engine itself calls:
 *   TTASR_SELF_STEP     launch_self_attn_decode: n_rows rows at the one position geom_host[0] (n_geom = 1)
 *   TTASR_SELF_ROWS     launch_self_attn_decode_rows: row r at position geom_host[r] (n_geom = n_rows)
 *   TTASR_SELF_PREFILL  launch_self_attn_prefill (append launch + attend launch): geom_host = {n_seq, npos}, rows [sequence][position]
 *   TTASR_SELF_PACKED   launch_prefill_self_attn over the tables prefill_build_tables makes: geom_host = the n_geom sequences' lengths,
 *                       aux_host = their page lists one after the other (ceil(length / 16) pages each), n_rows = the lengths' sum
 *   TTASR_SELF_COPY     launch_copy_pages over every layer: aux_host = n_aux / 2 (source, destination) page pairs, at most max_batch
 *                       pairs; no pairs launch nothing; qkv_host, out_host, layer's rows and geom are not used
 * qkv_host: f32 [n_rows][3 d_model] (q | k | v), cast to the engine type and used as given (the 1/8 lives in the weights); step and
 * rows forms on a 16-bit engine also take n_slab = 1..4 f32 partial tiles [n_slab][n_rows][3 d_model], completed by the kernel with a
 * zero bias the way the step completes the K-split qkv GEMM.  Step and rows forms: the rows are rows [row0, row0 + n_rows) of the
 * batch (row0 offsets qkv, out and the finished flags, never the pages: row r uses the pages of batch row row0 + r); done_host:
 * optional int32 [n_rows], nonzero = finished.  Step, rows and prefill forms: aux_host = the device page table
 * [max_batch][pages_per_seq] for the launch (n_aux = 0: the identity), identity_pages != 0 = the instantiation that computes page ids
 * instead of loading them.  At most 512 rows in the two prefill forms, positions below n_text_ctx, page ids inside the pool.
 * out_host: f32 [n_rows][d_model]; the device output is zero-filled before the launch.  sig_buf (optional, sig_len bytes) receives
 * the instantiation(s) that ran, "name<template arguments> grid <threads>" joined by " + "; "" when nothing was launched. */
#define TTASR_SELF_STEP 0
#define TTASR_SELF_ROWS 1
#define TTASR_SELF_PREFILL 2
#define TTASR_SELF_PACKED 3
#define TTASR_SELF_COPY 4
TTASR_API int ttasr_self_attn_probe(ttasr_ctx* ctx, int32_t form, int32_t layer, int32_t n_rows, const float* qkv_host, int32_t n_slab,
                                    const int32_t* geom_host, int32_t n_geom, const int32_t* aux_host, int32_t n_aux, int32_t identity_pages,
                                    int32_t row0, const int32_t* done_host, float* out_host, char* sig_buf, int32_t sig_len);
/* Known-answer hook for the ENCODER attention kernels (tests/test_gpu_enc_attn_kernels.py): ONE launch on
 * caller-supplied operands, through the function the engine itself calls to choose its kernel.
 *   TTASR_ENC_SELF   the encoder layer's self-attention: a_host = qkv, f32 [B][T][3 d_model] (q | k | v per row), B <= max_batch,
 *                    1 <= T <= n_audio_ctx; k_host, v_host and Tk are not used.  Options "flash", "flash_qw" and "generic_kernels"
 *                    steer the launch exactly as they steer ttasr_encode (16-bit engines: the MFMA flash kernel with 64 or 32
 *                    queries per wave, or the plain kernel; the f32 engine: the plain kernel).
 *   TTASR_ENC_CROSS  (16-bit engines) the cross-attention launcher with T rows per clip: a_host = q, f32 [B clips][T][d_model],
 *                    1 <= T <= n_text_ctx; k_host / v_host = f32 [B][n_heads][Tk][64], 1 <= Tk <= n_audio_ctx.  The launcher gets
 *                    kv_div = T and a frame-split workspace, so its own rule applies: the flash kernel's many-row form from 32 rows
 *                    per clip upward, the decode step's kernels below.
 * Operands are cast to the engine type and used as given (the 1/8 of the attention lives in the q weights).  out_host: f32
 * [B][T][d_model].  The device output is filled with a NaN pattern (0x7fc0 in 16 bits, 0x7fc00000 in f32) before the launch and
 * has one guard row of the same pattern behind it: a row no kernel writes comes back NaN, and the call returns
 * TTASR_ENC_GUARD_TOUCHED (1; out_host is filled all the same) when the guard row did not keep its pattern - the one positive
 * return value of the library.  sig_buf (optional, sig_len bytes) receives the signature of what ran, "name<template arguments>
 * grid <threads>" (cross form: the launcher's own text).  Refused in an open session.  Operands, output and workspace live in a
 * block of the hook's own (allocated by the first call): resident mel / encoder / cross-KV state, search state and captured
 * graphs are not touched. */
#define TTASR_ENC_SELF 0
#define TTASR_ENC_CROSS 1
#define TTASR_ENC_GUARD_TOUCHED 1
TTASR_API int ttasr_enc_attn_probe(ttasr_ctx* ctx, int32_t form, int32_t B, int32_t T, const float* a_host, const float* k_host,
                                   const float* v_host, int32_t Tk, float* out_host, char* sig_buf, int32_t sig_len);

/* Short-window option (opt-in, a behavioural change versus Whisper's fixed 30-s training window, the
 * same trade whisper.cpp's `audio_ctx` makes): subsequent log_mel / encode / generate calls use only the first n_ctx
 * encoder positions (= 2*n_ctx mel frames = n_ctx*320 samples), n_ctx even, 4 <= n_ctx <= cfg.n_audio_ctx; 0 restores
 * the model's window.  A 3-s utterance (n_ctx 150) then costs a tenth of the encoder flops and cross-KV bytes.
 * Drops the resident mel / encoder state. */
TTASR_API int ttasr_set_audio_ctx(ttasr_ctx* ctx, int32_t n_ctx);

/* ---- a9-a10: decoder (ctranslate2 Whisper.generate) --------------------------------------------- */
/* Greedy search.  prompt_host: [B][max_prompt] ids, prompt_len_host[b] of them valid (>=1).
 * out_tokens_host: [B][max_new_tokens] sampled ids (EOT included when emitted), out_len_host[b] count.
 * out_sum_logprob_host / out_no_speech_host: optional [B].
 * A row whose logits leave NO selectable token at some step - every id masked by the rules, or every logit NaN (non-finite
 * weights, mel or encoder output reach this through the test hooks above) - ends there: the token is EOT, the step's
 * log-probability increment is -inf (so out_sum_logprob is -inf and the clip's average fails every log-prob threshold), the row is
 * finished.  The same holds for ttasr_generate_capped, ttasr_generate_sample, the rows of a continuous-batching session and the
 * independent rows of a beam session; beam search answers the case with TTASR_E_INVALID "no live candidate".  No token id outside
 * [0, vocab) is ever produced.  A row with SOME NaN logits never selects them, but its log-probabilities are NaN. */
TTASR_API int ttasr_generate(ttasr_ctx* ctx, int32_t B, const int32_t* prompt_host, const int32_t* prompt_len_host,
                   int32_t max_prompt, const ttasr_gen_opts* opts, int32_t* out_tokens_host, int32_t* out_len_host,
                   float* out_sum_logprob_host, float* out_no_speech_host);
/* Greedy search with a token budget PER ROW (round 6): row b is finished after min(row_max_new_host[b], opts->max_new_tokens)
 * sampled tokens or at EOT, whichever comes first; row_max_new_host[b] in [1, opts->max_new_tokens].  Everything else as
 * ttasr_generate - in particular every row's tokens are identical, bit for bit, to the same row of a ttasr_generate call cut at its
 * budget: rows are computed independently, and a FINISHED row (here or in ttasr_generate after EOT, or a finished clip of a beam
 * search) leaves the attention kernels of the decode step - it no longer streams its 2 x n_audio_ctx x 128 B of cross-KV per
 * (layer, head), the bytes that dominate a step - while the launch grid and the captured graphs stay those of the full batch.
 * What the reference's consumers do with natural stopping (segments are consumed until the generator ends: asr_core.py:159-172)
 * on a batch whose rows stop at different lengths; synthetic weights never emit a meaningful EOT, so benchmarks and tests
 * state the lengths here.  Option "ragged_exit" = 0 restores the static batch (A/B). */
TTASR_API int ttasr_generate_capped(ttasr_ctx* ctx, int32_t B, const int32_t* prompt_host, const int32_t* prompt_len_host,
                                    int32_t max_prompt, const ttasr_gen_opts* opts, const int32_t* row_max_new_host,
                                    int32_t* out_tokens_host, int32_t* out_len_host, float* out_sum_logprob_host,
                                    float* out_no_speech_host);
/* Beam search (the reference call sites pass beam_size=5: asr_core.py:164, file_asr.py:462,
 * faster_whisper_asr.py:144).  n_audio clips x `beam` hypotheses = rows of the decode batch (<= max_batch; the bf16
 * weight-streaming GEMM carries up to 128 rows); the `beam` rows of a clip share its cross-attention K/V, and a re-index of the
 * hypotheses permutes the self-attention page tables (copy-on-write of the one partially filled page) instead
 * of copying caches.  prompt_host: [n_audio][prompt_len] (same length for every clip).  Candidate selection
 * follows Whisper's published beam search (top beam+1 per hypothesis, EOT hypotheses go to a finished pool of
 * round(beam * patience), winner = max sum_logprob / length).  Outputs as ttasr_generate (EOT stripped). */
TTASR_API int ttasr_generate_beam(ttasr_ctx* ctx, int32_t n_audio, int32_t beam, const int32_t* prompt_host, int32_t prompt_len,
                        const ttasr_gen_opts* opts, float patience, int32_t* out_tokens_host, int32_t* out_len_host,
                        float* out_sum_logprob_host, float* out_no_speech_host);
/* The same search with one prompt per clip (prompt_host [n_audio][max_prompt], prompt_len_host[a] tokens valid,
 * sot_index_host[a] = position of <|startoftranscript|> in clip a's prompt, or NULL for opts->sot_index everywhere): what
 * a caller needs to run several FILES through one engine pass when each carries its own previous-text prompt
 * (condition_on_previous_text).  The step loop is position-synchronous: clips with longer prompts are still being forced
 * while the others already search. */
TTASR_API int ttasr_generate_beam_ragged(ttasr_ctx* ctx, int32_t n_audio, int32_t beam, const int32_t* prompt_host,
                               const int32_t* prompt_len_host, const int32_t* sot_index_host, int32_t max_prompt,
                               const ttasr_gen_opts* opts, float patience, int32_t* out_tokens_host, int32_t* out_len_host,
                               float* out_sum_logprob_host, float* out_no_speech_host);
/* Temperature sampling (the fallback ladder of faster-whisper's generate_with_fallback: temperatures 0.2 ... 1.0
 * with best_of hypotheses).  n_audio clips x best_of independently sampled rows that share the clip's cross-KV;
 * tokens are drawn from softmax(processed logits / temperature) with a counter-based generator keyed by
 * (seed, row, position, token), so a run is reproducible; per clip the hypothesis with the highest
 * sum_logprob / length is returned (EOT kept when emitted, as ttasr_generate). */
TTASR_API int ttasr_generate_sample(ttasr_ctx* ctx, int32_t n_audio, int32_t best_of, const int32_t* prompt_host, int32_t prompt_len,
                          const ttasr_gen_opts* opts, float temperature, uint32_t seed, int32_t* out_tokens_host,
                          int32_t* out_len_host, float* out_sum_logprob_host, float* out_no_speech_host);
/* Step-level access for parity tests: reset the self-attention cache, then feed one token per row per
 * call; logits_host (optional) receives raw float32 [B][vocab] for the position just fed. */
TTASR_API int ttasr_decode_reset(ttasr_ctx* ctx, int32_t B);
TTASR_API int ttasr_decode_step(ttasr_ctx* ctx, const int32_t* tokens_host, int32_t B, float* logits_host);
/* Known-answer hook for the rule kernel alone: rows [n][vocab] raw logits, hist [n][hist_stride]
 * sampled-token histories padded with -1 -> processed rows (masked entries = -inf) and the selected id. */
TTASR_API int ttasr_apply_rules(ttasr_ctx* ctx, const float* rows_host, const int32_t* hist_host, int32_t hist_stride,
                      int32_t n, const ttasr_gen_opts* opts, float* out_rows_host, int32_t* out_choice_host);
/* Known-answer hook for the token-selection kernels (kernels_decode.hip; tests/test_gpu_select_kernels.py):
 * ONE launch of a named form, through the launcher the engine itself calls, on caller-supplied raw logits rows_host f32 [n][vocab]
 * (1 <= n <= max_batch), which are copied into the engine's logits block at its row stride.  The hook has no decision logic:
 *   TTASR_SELECT_STEP     launch_select (no processed-row output, the step ticket, total_rows = n) at the position positions_host[0]
 *   TTASR_SELECT_ROWS     launch_select_rows: row r at its own position positions_host[r]
 *   TTASR_SELECT_SESSION  launch_session_rows_select over n_entries <= max_batch entries {row < n, position, key row, flags
 *                         (1 choose, 2 no-speech)} with a temperature and a seed per entry -> out_f32 [n_entries][3] = {choice (int
 *                         bits, -1: entry does not choose), log-probability increment, no-speech}
 *   TTASR_SELECT_TOPK     launch_beam_topk, 1 <= k <= 8 -> out_f32 [n][k] log-probabilities, out_i32 [n][k] ids (-1: fewer than k
 *                         allowed tokens, log-probability -inf), no_speech [n] when want_no_speech != 0
 *   TTASR_SELECT_LOGPROB  launch_token_logprob: out_f32 [n] = log softmax(row r)[targets_host[r]]
 *   TTASR_SELECT_PROB     launch_token_prob: out_f32 [n] = softmax(row r)[token]
 * opts, temperature, seed: the rules of the launch (STEP, ROWS, SESSION, TOPK; temperature > 0 = the sampling instantiation of STEP
 * and ROWS).  hist_host [n][hist_stride]: sampled-token histories padded with -1, as ttasr_apply_rules (NULL: empty histories).
 * STEP and ROWS: prompt_host [n][max_prompt] with prompt_len_host [n] (NULL: no forced tokens) and the initial done, row_cap,
 * sum_logprob [n] (NULL: live rows, no budget, 0) and n_done; they return the WHOLE search state after the launch - cur_tok,
 * n_sampled, last_tok, pen_tok, last_ts, done [n], positions (STEP: {*step, the ticket word}; ROWS: [n]), n_done [1], sum_logprob,
 * no_speech [n], out_tokens [n][opts->max_new_tokens] (-1 where nothing was stored; cur_tok starts at -1 too).  Any output pointer
 * may be NULL.  sig_buf (optional, sig_len bytes) receives the instantiation that ran.  Refused in an open session.  The call
 * overwrites search state: it is UNDEFINED afterwards until ttasr_decode_reset, a generate call or a session start. */
#define TTASR_SELECT_STEP 0
#define TTASR_SELECT_ROWS 1
#define TTASR_SELECT_SESSION 2
#define TTASR_SELECT_TOPK 3
#define TTASR_SELECT_LOGPROB 4
#define TTASR_SELECT_PROB 5
typedef struct ttasr_select_io {
  /* in */
  const float* rows_host;
  const ttasr_gen_opts* opts;
  const int32_t* hist_host;
  const int32_t* positions_host;
  const int32_t* prompt_host;
  const int32_t* prompt_len_host;
  const int32_t* done_host;
  const int32_t* row_cap_host;
  const float* sum_logprob_host;
  const int32_t* entries_host;       /* SESSION [n_entries][4] */
  const float* entry_temp_host;      /* SESSION [n_entries] */
  const uint32_t* entry_seed_host;   /* SESSION [n_entries] */
  const int32_t* targets_host;       /* LOGPROB [n] */
  /* out (each optional) */
  int32_t* out_cur_tok;
  int32_t* out_n_sampled;
  int32_t* out_last_tok;
  int32_t* out_pen_tok;
  int32_t* out_last_ts;
  int32_t* out_done;
  int32_t* out_positions;
  int32_t* out_n_done;
  float* out_sum_logprob;
  float* out_no_speech;
  int32_t* out_tokens;
  float* out_f32;
  int32_t* out_i32;
  /* scalars */
  int32_t n, hist_stride, max_prompt, n_done, n_entries, k, want_no_speech, token;
  float temperature;
  uint32_t seed;
} ttasr_select_io;
TTASR_API int ttasr_select_probe(ttasr_ctx* ctx, int32_t form, const ttasr_select_io* io, char* sig_buf, int32_t sig_len);

/* ---- sequence bias: a logits processor that rewards listed token sequences --------------------
 * The definition is HF Transformers' SequenceBiasLogitsProcessor.  The table maps token sequences to float biases.  A row's
 * history is its whole token sequence so far: the prompt, then every sampled token.  A sequence of length 1 always applies to its
 * token; a sequence of length L > 1 applies to its LAST token when the history holds at least L tokens and its last L - 1 tokens
 * equal the sequence's first L - 1.  Per vocabulary id the sum starts at 0, takes the length-1 bias, then the matching longer
 * sequences in table order, in float32, and is added to the raw logit once, in front of the Whisper rules (a suppressed id stays
 * -inf); log-probabilities are those of the processed distribution.
 *
 * ttasr_set_sequence_bias installs n_seq sequences - sequence i = tokens_host[offsets_host[i] .. offsets_host[i + 1]) with
 * bias_host[i], offsets_host [n_seq + 1] - replacing the table of THIS context (a context of ttasr_create_shared has its own);
 * n_seq = 0 clears it.  Refused with a message, the old table kept: a length outside 1 .. 16, more than 4096 distinct last tokens,
 * more than 8192 sequences longer than one token, a bias that is not finite, an id outside the vocabulary, a repeated sequence,
 * an open session.  The table lives in a device block of fixed capacity whose counts the kernel reads from the block: replacing
 * it invalidates no captured graph.  While a table is installed it applies to ttasr_generate, _capped, _sample and
 * ttasr_generate_beam[_ragged]; ttasr_decode_step, ttasr_align*, ttasr_detect_language and ttasr_apply_rules stay raw, and
 * ttasr_session_begin[_beam] is refused.  With no table every launch chain is what it is without this feature.
 *
 * ttasr_seq_bias_probe: the known-answer hook of the kernel (tests/test_gpu_seq_bias_kernels.py): ONE launch, through the
 * launcher the engine calls, with the installed table on rows_host f32 [n][vocab] -> out_rows_host [n][vocab].
 *   TTASR_SEQ_BIAS_WINDOW  the beam search's form: hist_host [n][15] with hist_host[r][15 - k] = the k-th token back,
 *                          hist_len_host [n] = min(history length, 16), or -1: the row is left alone
 *   TTASR_SEQ_BIAS_STATE   the greedy loop's form: out_tokens_host [n][max_new] with n_sampled_host [n], behind them prompt_host
 *                          [n][max_prompt] with prompt_len_host [n] (NULL: no prompt), done_host [n] (NULL: live rows) and
 *                          `position`, the position of the token being fed: a row with position + 1 < prompt length is forced
 *                          and, like a finished row, left alone
 * The call overwrites search state, as ttasr_select_probe does. */
TTASR_API int ttasr_set_sequence_bias(ttasr_ctx* ctx, int32_t n_seq, const int32_t* tokens_host, const int32_t* offsets_host,
                                      const float* bias_host);
#define TTASR_SEQ_BIAS_WINDOW 0
#define TTASR_SEQ_BIAS_STATE 1
typedef struct ttasr_seq_bias_io {
  const float* rows_host;
  const int32_t* hist_host;
  const int32_t* hist_len_host;
  const int32_t* prompt_host;
  const int32_t* prompt_len_host;
  const int32_t* out_tokens_host;
  const int32_t* n_sampled_host;
  const int32_t* done_host;
  float* out_rows_host;
  int32_t n, max_prompt, max_new, position;
} ttasr_seq_bias_io;
TTASR_API int ttasr_seq_bias_probe(ttasr_ctx* ctx, int32_t form, const ttasr_seq_bias_io* io, char* sig_buf, int32_t sig_len);

/* ---- continuous batching: greedy single-window decoding with slot refill ----------------------------------------------
 * Clips are submitted at any time; each takes a free row of the context's max_batch-row decode batch, decodes until EOT or its
 * own token budget, and its row is handed to the next queued clip.  The batch always runs at max_batch rows (the full-width
 * kernel forms), and every encoder pass of a session runs one GEMM family whatever the number of clips it encodes, so a clip's
 * result does not depend on its neighbours, on when it was submitted or on GPU timing: its tokens, sum_logprob and no_speech
 * are bit-identical to the same clip in a static batch of max_batch rows decoded by ttasr_generate_capped with option
 * "prefill" = 0, in every compute mode.  With option "xkv_fp8" = 2 the same holds against that static pass run with the option
 * at 2 as well: an admitted clip's e4m3 block and scales are those a static ttasr_encode builds for it.  Prompt tokens are forced through ordinary decode steps.  While a session is open
 * every other search, step, encoder, mel, rule-hook, audio-window and option call on the context is refused (TTASR_E_INVALID); ttasr_session_end closes it and leaves no resident encoder state (log-mel and encode
 * again before a static ttasr_generate).
 *
 * ttasr_session_begin: opts as for ttasr_generate (opts->check_interval = decode steps between two polls of the finished
 *   flags); max_prompt = the longest prompt a clip may bring; temperature must be 0 (greedy only).  Refused: the e4m3
 *   cross-KV mode at value 1 (option xkv_fp8; value 2 is the session-capable mode: the session quantises every admitted clip
 *   from its staging cross-KV into the clip's live slot).  The first session of a context allocates its staging cross-KV (the size of the
 *   context's cross-KV cache), the row positions and the admission table; later sessions reuse them.
 * ttasr_session_submit: n clips, clip i = pcm_host[i][0 .. n_samples[i]) (at most one window), prompt [n][max_prompt] with
 *   prompt_len[i] tokens valid, max_new[i] in [1, opts->max_new_tokens] = the clip's token budget; out_ids (optional)
 *   receives the ids the session gave the clips (0, 1, 2 ... in submission order).  Everything is validated before
 *   anything is queued; the PCM and prompts are copied.
 * ttasr_session_poll: admits ready clips into free rows, runs decode steps until at least one clip finished, nothing is
 *   left, or max_steps steps ran; returns up to `cap` finished clips: ids [cap], tokens [cap][opts->max_new_tokens]
 *   (lens[k] valid, EOT kept when sampled, as ttasr_generate), sum_lp / no_speech [cap] (optional), *n_out.  Clips that
 *   finished beyond `cap` are returned by the next poll.  *n_out == 0 means "idle" (nothing submitted is unfinished) only
 *   when the poll did not stop at max_steps: with a bounded max_steps, count the clips received against those submitted (or
 *   read ttasr_session_stats out[7] and ttasr_session_rows) before concluding that the session is idle.
 * ttasr_session_rows: the batch's rows now (after the work enqueued so far has run): row_pos [max_batch] positions, done
 *   [max_batch] finished flags (1 = finished or free), row_clip [max_batch] id of the clip holding the row or -1 (free);
 *   any of the three may be NULL.  For monitoring and tests.
 * ttasr_session_stats: out[0] decode steps, [1] polls, [2] encoder passes, [3] clips encoded, [4] live row-steps of the
 *   clips returned so far (prompt_len - 1 + tokens each), [5] encoder ms (GPU events: mel + encoder + cross-KV),
 *   [6] decode ms (GPU events around the step runs), [7] clips submitted and not yet admitted. */
TTASR_API int ttasr_session_begin(ttasr_ctx* ctx, const ttasr_gen_opts* opts, int32_t max_prompt, float temperature);
/* Beam-search mode of the session.  beam in 1..7; the batch is G = max_batch / beam groups of `beam` rows (rows G*beam ..
 * max_batch-1 stay free).  Submit, poll, stats, rows and end are the calls above, with these differences:
 *   - A clip occupies one group of `beam` rows and one cross-KV slot: group g uses slot g, read with kv_div = beam exactly as
 *     in ttasr_generate_beam.
 *   - max_new[i] of ttasr_session_submit is clip i's token budget: its search ends when round(beam * patience) hypotheses
 *     have finished, or when its best live hypothesis holds min(max_new[i], n_text_ctx - prompt_len) tokens.
 *   - The winner has the highest sum_logprob / length (as ttasr_generate_beam); tokens come back with EOT stripped (the
 *     greedy session keeps it), sum_lp is the winner's sum, no_speech is the group's first row at opts->sot_index, which must
 *     lie inside every clip's prompt when opts->no_speech >= 0 (checked by submit).
 *   - Candidate selection runs on the host, so a poll runs one step per host exchange; opts->check_interval is ignored.  A
 *     finished group is handed to the next clip at the following step.
 *   - ttasr_session_rows: every row of a group reports the group's clip and the group's position (the next one to compute).
 *   - ttasr_session_stats: the values keep their meaning; out[4] counts the live row-steps of all `beam` rows of a group.
 * A clip equals, bit for bit (tokens, sum_logprob, no_speech), the same clip in ttasr_generate_beam over a static pass of
 * exactly G clips on the same context with option prefill = 0 (and, in 16-bit, option enc_gemm = 3).  With option "xkv_fp8" = 2
 * on both sides the same holds - the groups' rows read the e4m3 copy through the shared-clip kernel in either form - and a
 * sampled window clip equals slot 0 of a static ttasr_generate_sample pass under that option.
 * Refused, leaving the context usable and no session open: beam outside 1..7, max_batch < beam, patience <= 0, option xkv_fp8
 * = 1, a session already open, and everything ttasr_session_begin refuses.  While a beam session is open, every call that the
 * greedy session refuses is refused too. */
TTASR_API int ttasr_session_begin_beam(ttasr_ctx* ctx, const ttasr_gen_opts* opts, int32_t max_prompt, int32_t beam,
                                       float patience);
TTASR_API int ttasr_session_submit(ttasr_ctx* ctx, int32_t n, const float* const* pcm_host, const int64_t* n_samples,
                                   const int32_t* prompt, const int32_t* prompt_len, const int32_t* max_new, int64_t* out_ids);
TTASR_API int ttasr_session_poll(ttasr_ctx* ctx, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens,
                                 float* sum_lp, float* no_speech, int32_t* n_out);
/* Window clips and independent rows in a beam session (ttasr_session_begin_beam; refused in a greedy session).  Window i is
 * the 30-s window of the recording file_pcm[i][0 .. file_samples[i]) that starts at 10-ms frame seek_frames[i], with its own
 * prompt (prompt [n][max_prompt], prompt_len[i] valid), <|startoftranscript|> position sot_index[i], budget max_new[i] in
 * [1, opts->max_new_tokens], temperature[i] >= 0 (temperature NULL: all 0), rows[i] in [1, beam] and seed[i].
 *   - Its log-mel is bit-identical to ttasr_log_mel_windows for the same (file, seek, floor_max[i]) (floor_max NULL: each
 *     window's own maximum decides its dynamic-range floor): true neighbour samples across the window seam, reflection only at
 *     the file ends, frames past the recording 0 in feature space.  Only the samples the window's frames read are copied.
 *     Plain clips (ttasr_session_submit) and window clips may share an encoder pass; plain clips keep their own mel.
 *   - temperature 0 and rows > 1: beam search of width rows[i], as for a plain clip (tokens without EOT).
 *   - temperature 0 and one row: greedy; temperature > 0: rows[i] independent Gumbel-max samples, row b keyed
 *     pcg_hash(seed ^ pcg_hash(b * 0x9E3779B9 + position)); a row ends at EOT or its budget, the clip when all its rows have
 *     ended, and the row with the highest sum_logprob / length wins.  Tokens come back as ttasr_generate_sample returns them
 *     (EOT kept when sampled), sum_lp is the winner's f32 sum, no_speech the group's first row at sot_index[i].  Such a clip
 *     equals, bit for bit, the same clip in slot 0 of a static ttasr_generate_sample pass of G clips with best_of = rows = beam
 *     and the same seed (prefill = 0; in 16-bit enc_gemm = 3), and with temperature 0 and beam = 1 the same clip of a static
 *     ttasr_generate_capped pass.
 * Everything is validated before anything is queued: rows outside [1, beam], a negative or non-finite temperature, a seek at
 * or beyond the end of the file, a NULL pcm with samples, a non-finite floor_max, a sot_index outside the prompt when
 * opts->no_speech >= 0, and what ttasr_session_submit refuses.  Results come back through ttasr_session_poll; out_ids as
 * there. */
TTASR_API int ttasr_session_submit_windows(ttasr_ctx* ctx, int32_t n, const float* const* file_pcm, const int64_t* file_samples,
                                           const int64_t* seek_frames, const float* floor_max, const int32_t* prompt,
                                           const int32_t* prompt_len, const int32_t* sot_index, const int32_t* max_new,
                                           const float* temperature, const int32_t* rows, const uint32_t* seed, int64_t* out_ids);

/* Language identification INSIDE a session (greedy or beam): no detection pass, and no second encoder pass, before the session.
 * ttasr_session_detect_language arms the open session for the span [lang_begin, lang_begin + n_lang) of the tied embedding and
 * the <|startoftranscript|> token `sot`.  From then on a prompt given to ttasr_session_submit / ttasr_session_submit_windows
 * may hold the placeholder TTASR_TOKEN_DETECT, at most once and only directly behind a token equal to `sot`.
 *   - When such a clip is admitted, its row (beam session: its group) first runs ONE detect step: `sot` at position 0 against
 *     the clip's own cross-KV, an ordinary step of the session's max_batch rows.  Behind it the language head of
 *     ttasr_detect_language - the same dot products, softmax and first maximum, in the same order - runs for that row on the
 *     device, the placeholder is replaced by lang_begin + winner, and the row starts over at position 0 with prompt[0]
 *     (position 0 of its self-attention pages is written again).  From there the clip decodes as if the language had been
 *     given: its tokens, sum_logprob and no_speech are bit-identical to the same clip submitted with that token written out,
 *     and winner, probabilities and span logits are those of ttasr_detect_language for the clip in a static pass of max_batch
 *     clips.  A detected clip costs one more decode step and no encoder work; clips without the placeholder, and their
 *     neighbours, are untouched.
 *   - Greedy session: the head is one more launch in every step of the armed session's step graphs (also inside a run of
 *     opts->check_interval steps); the device patches the prompt itself.  Beam session: the head runs behind the logits-only
 *     step for the first row of each detecting group, its results come back with the step's one synchronisation, and the group
 *     takes no part in that step's candidate, no-speech or independent-row work (BEAM and ROWS groups, plain and window clips).
 *   - An unarmed session enqueues exactly what it did before this call existed.
 *   - ttasr_session_stats: a detect step is a decode step (out[0]); out[4] counts one more live row-step per detected clip
 *     (beam session: one per live row of its group).  ttasr_session_rows shows position 0 during the detect step.
 * Refused with TTASR_E_INVALID, the context and the session stay usable: no session open; a clip was submitted already; the
 * session is armed already; sot outside the vocabulary; n_lang outside [1, 128]; a span past the vocabulary.  The device
 * buffers (flags, slots, results: max_batch * 261 words) belong to the context: allocated by the first armed session, freed by
 * ttasr_destroy.  The submit calls refuse, before anything is queued: the placeholder in an unarmed session (as before: it is no
 * token), not directly behind `sot`, or twice in a prompt.
 * ttasr_session_poll_lang: ttasr_session_poll (same arguments, same behaviour; both are one implementation) plus
 *   lang         int32 [cap]                   index into the span, -1 for a clip that carried no placeholder (required)
 *   lang_probs   optional float32 [cap][n_lang] softmax over the span (rows of clips without placeholder are not written)
 *   lang_logits  optional float32 [cap][n_lang] the raw span logits (idem)
 * In an unarmed session every lang[k] is -1.  ttasr_session_poll on an armed session works and drops the language. */
#define TTASR_TOKEN_DETECT (-1)
TTASR_API int ttasr_session_detect_language(ttasr_ctx* ctx, int32_t sot, int32_t lang_begin, int32_t n_lang);
TTASR_API int ttasr_session_poll_lang(ttasr_ctx* ctx, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens,
                                      float* sum_lp, float* no_speech, int32_t* lang, float* lang_probs, float* lang_logits,
                                      int32_t* n_out);

/* ---- prompt prefill at admission (option "session_prefill", default 0 = off) ------------------------------------------
 * By default a session forces every prompt token through an ordinary decode step of max_batch rows.  With
 * ttasr_set_option(ctx, "session_prefill", N), N in [1, n_text_ctx - 2], set BEFORE ttasr_session_begin[_beam] (which reads it,
 * like "refill_overlap"), a clip's leading prompt positions are computed in one ADMISSION PASS instead - the decoder layers over
 * the packed prompt rows of the clips admitted together, enqueued on the decode stream between two steps, behind the clips'
 * cross-KV copies.
 * The rule, per clip, decided at admission from the clip's own prompt only: let p = prompt_len - 1; if opts->no_speech >= 0,
 * p = min(p, sot index) - the clip's own sot_index in a beam session, opts->sot_index in a greedy one - so the
 * <|startoftranscript|> position stays a real step and no_speech is computed where it always was.  If p >= N, positions
 * 0 .. p - 1 come from the pass and the row (group) starts stepping at position p with prompt[p]; otherwise the clip is forced
 * as before.  A clip that carries TTASR_TOKEN_DETECT is NEVER prefilled: its detect step rewrites position 0 of its pages.
 * Beam session: the prefix pages are taken once per group and shared by its rows (BEAM and ROWS groups alike); a clip whose
 * prefix the page pool cannot supply at that moment is forced as before: a per-clip decision from pool state, taken before
 * anything is enqueued for the clip.  Such a clip is an unprefilled clip in every respect (bit-identical to the option at 0) and
 * is NOT counted by ttasr_session_prefill_stats, whose four values hold what the passes did: a host that applies the rule above
 * to the prompts it submitted finds these clips as the difference to out[1].  (The pool holds max_batch * pages_per_seq pages
 * and a live row at most pages_per_seq: the case needs hypotheses that have split nearly every page of every group.)
 * The contract:
 *   - A clip that is not prefilled is bit-identical (tokens, sum_logprob, no_speech, language results) to the same clip in a
 *     session with the option at 0, whatever its neighbours do.
 *   - A prefilled clip's results depend only on the clip, the options and the compute mode - not on which other clips shared
 *     its admission pass, not on how many passes the admission was cut into, not on "refill_overlap", not on timing.  Every
 *     kernel form inside the pass (GEMM family, attention block height) is a function of the clip's own prompt length and of
 *     context constants, never of the pass.
 *   - f32 engine: the tokens of the forced session, sum_logprob and no_speech up to f32 summation order.  16-bit engines: not
 *     bit-identical to the forced path (the pass runs the tiled GEMM family, the steps the K-split decode GEMMs), as with the
 *     static searches' "prefill".
 * The pass has its own activation workspace (512 rows of f32 residual, h, qkv, attention output and the FFN's hidden rows:
 * about 14 MB at large-v3), owned by the context: allocated by the first session that enables the option, freed by
 * ttasr_destroy.  It works with "refill_overlap" 0 and 1 and under "xkv_fp8" = 2 (it reads the 16-bit live slots).  An admission
 * that holds more than 512 prompt rows is cut into several passes by whole clips.  Hold mode and ttasr_session_align are
 * untouched.  With the option at 0 a session enqueues the launches and copies it did before the option existed; one thing
 * differs in form: a row's entry of the admission table is one word wider (its start position, 0), and the admission kernel reads
 * that word.
 * ttasr_session_prefill_stats (open session): out[0] passes, out[1] clips prefilled, out[2] positions prefilled (once per
 * clip, not per beam row), out[3] GPU ms of the passes (events; the call waits for the last pass).  ttasr_session_stats
 * out[0] and out[4] count only steps and row-steps that ran: prefilled positions are in neither. */
TTASR_API int ttasr_session_prefill_stats(ttasr_ctx* ctx, double out[4]);
TTASR_API int ttasr_session_stats(ttasr_ctx* ctx, double out[8]);
TTASR_API int ttasr_session_rows(ttasr_ctx* ctx, int32_t* row_pos, int32_t* done, int64_t* row_clip);
TTASR_API int ttasr_session_end(ttasr_ctx* ctx);

/* ---- word timestamps (faster-whisper find_alignment -> ctranslate2 Whisper.align; WhisperModel.transcribe(word_timestamps=True),
 * requested at faster_whisper_asr.py:289-294) -------------------------------------------------------------------------- */
/* Teacher-forces tokens_host[0..n_tokens) (sot sequence + text tokens + eot) against the resident encoder state of
 * clip `clip` in one batched pass and returns
 *   out_weights_host  float32 [n_pairs][n_tokens][n_ctx]  softmax cross-attention rows of the (layer, head) pairs
 *                     pairs_host[2*i], pairs_host[2*i+1]   (n_ctx = the current audio window, 1500 by default)
 *   out_logprob_host  optional float32 [n_tokens - 1]       log p(tokens[i+1] | tokens[0..i]) from the raw logits.
 * Invalidates any step-level decode state (it reuses row 0's self-attention pages). */
TTASR_API int ttasr_align(ttasr_ctx* ctx, int32_t clip, const int32_t* tokens_host, int32_t n_tokens, const int32_t* pairs_host,
                int32_t n_pairs, float* out_weights_host, float* out_logprob_host);
/* ---- language identification (faster-whisper detect_language / transcribe(language=None): info.language,
 * info.language_probability, all_language_probs) ------------------------------------------------------------------------ */
/* Detects the language of the B clips whose encoder state is resident (log_mel -> encode -> detect -> generate: no second
 * encoder pass).  One decoder pass of B rows at position 0 with the token `sot` - the attention and GEMM kernels a
 * ttasr_decode_step of B rows at position 0 takes, under every option - that ends in the language head instead of the
 * vocabulary projection: the dot products of each row's final LayerNorm output with the rows [lang_begin, lang_begin + n_lang)
 * of the tied embedding (f32 accumulation), their softmax and its first maximum, on the device.  Bit-reproducible, and a
 * clip's results do not depend on the other clips of the call.
 *   out_lang_host    int32 [B]            index into the span (language token = lang_begin + index)
 *   out_probs_host   optional float32 [B][n_lang]   softmax over the span
 *   out_logits_host  optional float32 [B][n_lang]   the raw span logits (tests)
 * Checked before anything is enqueued, TTASR_E_INVALID, the context stays usable: out_lang_host NULL; no resident encoder state;
 * B outside [1, clips of the encoder state]; sot outside the vocabulary; n_lang outside [1, 128]; a span past the vocabulary;
 * an open session.  Like ttasr_align the call invalidates any step-level decode state (row i uses position 0 of row i's
 * self-attention pages); a following ttasr_generate* is bit-identical to one without the detection in between. */
TTASR_API int ttasr_detect_language(ttasr_ctx* ctx, int32_t B, int32_t sot, int32_t lang_begin, int32_t n_lang,
                                    int32_t* out_lang_host, float* out_probs_host, float* out_logits_host);
/* The same alignment for n sequences in ONE pass, with the host part of the algorithm on the device as well.  Sequence i is
 * tokens_host[i][0 .. n_tokens_host[i]) (rows of max_tokens entries; the rest of a row is ignored) against the resident
 * encoder state of clip clip_host[i]; several sequences may name the same clip.  Shorter sequences are padded to max_tokens
 * positions behind their real ones (causal self-attention: the real positions do not see them).  Behind the pass, per sequence:
 *   rows [first_row_i, n_tokens_i - 1) and frames [0, F_i), F_i = max(1, num_frames_i / 2) capped at n_ctx, of every pair's
 *   map -> per pair and frame, mean and population standard deviation over the rows (a zero deviation divides by 1) ->
 *   median of medfilt_width along time, edges reflected (no filter when F_i <= medfilt_width / 2) -> mean over the pairs,
 *   negated = the cost matrix C_i [rows_i][F_i] -> the DTW of ttasr_dtw (same f32 operations, same tie rule: for one cost
 *   matrix the same path) -> per row the first frame of the path in it.
 * Out (host):
 *   out_start_frame_host  int32 [n][max_tokens]    rows_i = n_tokens_i - 1 - first_row_i entries valid per sequence
 *   out_logprob_host      optional float32 [n][max_tokens]   n_tokens_i - 1 valid: log p(tokens[t+1] | tokens[0..t])
 *   out_cost_host         optional float32 [n][max_tokens][n_ctx]   C_i in the top-left rows_i x F_i corner (tests)
 *   out_weights_host      optional float32 [n][n_pairs][max_tokens][n_ctx]   the raw maps of every position (tests)
 * (n_ctx = the current audio window.)  Checked before anything is enqueued, TTASR_E_INVALID: n outside [1, max_batch];
 * max_tokens outside [2, min(n_text_ctx, n_audio_ctx)] or n * max_tokens > max_batch * n_audio_ctx (the rows of the borrowed
 * workspaces); n_tokens_i outside [2, max_tokens]; first_row_i outside [0, n_tokens_i - 2]; num_frames_i < 0; medfilt_width
 * even or outside [1, 15]; a token outside the vocabulary; the heads as for ttasr_align; a clip the encoder state does not
 * hold; an open session.  The scratch (tables, maps [n_pairs][n * max_tokens][n_ctx] f32, cost matrices, DTW traces that do
 * not fit the CU's LDS) is one block owned by the context: allocated by the first call, grown when a call needs more, freed by
 * ttasr_destroy; a request that cannot be allocated returns TTASR_E_NOMEM and leaves the context usable.  Like ttasr_align the
 * call invalidates any step-level decode state (sequence i uses row i's self-attention pages). */
TTASR_API int ttasr_align_batch(ttasr_ctx* ctx, int32_t n, const int32_t* clip_host, const int32_t* tokens_host,
                                const int32_t* n_tokens_host, int32_t max_tokens, const int32_t* first_row_host,
                                const int32_t* num_frames_host, const int32_t* pairs_host, int32_t n_pairs, int32_t medfilt_width,
                                int32_t* out_start_frame_host, float* out_logprob_host, float* out_cost_host,
                                float* out_weights_host);
/* Alignment inside a continuous-batching session (greedy or beam).
 * ttasr_session_hold(ctx, 1): from now on a clip that finishes is returned by ttasr_session_poll as usual but KEEPS its row
 *   (beam: its group) and its cross-KV slot; its rows are finished rows, which have left the attention kernels, so no live
 *   row's result changes.  ttasr_session_rows shows the clip's id on its rows until it is aligned or released.  The host MUST
 *   align or release held clips: a poll that can start nothing because every free unit is held returns *n_out == 0 with
 *   ttasr_session_stats out[7] > 0.  Refused with option refill_overlap = 1 (the pass borrows the encoder workspaces, which the
 *   overlapped encode writes from its own stream).  ttasr_session_hold(ctx, 0) switches the mode off and releases every
 *   held clip.  A session that never calls it behaves as before.
 * ttasr_session_align: ttasr_align_batch (same arguments, checks, outputs and scratch) for n DISTINCT held clips ids[i],
 *   each with its own cross-KV slot, in self-attention pages no live row uses; on success the clips are released.
 *   With option "align_packed" = 1 (read by this call) the pass is the PACKED one: the sequences' real positions, no padding,
 *   in the admission pass's workspace (allocated by the first call that needs it; more than 512 rows: several passes by whole
 *   sequences) and its one fixed GEMM family.  Arguments, checks, refusals, the release and the output layout are the same
 *   (positions past a sequence's end are 0 in every output).  Contract: a held clip's start frames, log-probs, cost matrix
 *   and maps are the same bits whether it is aligned alone or with other clips, in any order, in one call or several, in one
 *   pass or cut over two (tests/test_gpu_align_packed.py; the padded pass chooses its GEMM family from the row count of the
 *   whole call and does not promise this).
 * ttasr_session_release: frees held clips without aligning them.
 * An unknown id, an id that is not held, an id listed twice and any of the two calls with hold mode off are TTASR_E_INVALID,
 * and nothing happens.  ttasr_session_end releases everything. */
TTASR_API int ttasr_session_hold(ttasr_ctx* ctx, int32_t on);
TTASR_API int ttasr_session_align(ttasr_ctx* ctx, int32_t n, const int64_t* ids, const int32_t* tokens_host,
                                  const int32_t* n_tokens_host, int32_t max_tokens, const int32_t* first_row_host,
                                  const int32_t* num_frames_host, const int32_t* pairs_host, int32_t n_pairs, int32_t medfilt_width,
                                  int32_t* out_start_frame_host, float* out_logprob_host, float* out_cost_host,
                                  float* out_weights_host);
TTASR_API int ttasr_session_release(ttasr_ctx* ctx, int32_t n, const int64_t* ids);
/* A new search on held clips, with no encoder work (beam sessions; a greedy session refuses it like
 * ttasr_session_submit_windows).  ids[i] are n DISTINCT held clips.  The group of clip ids[i] starts a new search at the next
 * step under a new clip id, taken from the session's counter and returned in out_ids[i] (optional); the old id stops being held.
 * prompt [n][max_prompt], prompt_len, sot_index, max_new, temperature (NULL: all 0), rows and seed mean what they mean in
 * ttasr_session_submit_windows; the group's mode (BEAM or ROWS), candidate count, page lists and host search state are set up as an
 * admission sets them, and the rule of option "session_prefill" is applied to the new prompt as at admission (its pass is the
 * only thing a retry may enqueue).
 *   - Not touched: the group's cross-KV slot and, under "xkv_fp8" = 2, its e4m3 block and scales.  No log-mel, encoder, cross-KV
 *     projection, slot copy or quantiser launch is enqueued; ttasr_session_stats out[2], out[3] and out[5] do not move.  Live
 *     groups and other held clips are untouched.
 *   - The contract: a retried clip's tokens, sum_logprob and no_speech are bit-identical to the same audio submitted afresh with
 *     those parameters - a clip that came through ttasr_session_submit against a fresh ttasr_session_submit (a plain clip keeps
 *     its own mel; rows = beam, temperature 0, sot_index = opts->sot_index are that call's parameters), a window clip against a
 *     fresh ttasr_session_submit_windows - in f32, bf16 and fp16, with "xkv_fp8" 0 and 2 and "session_prefill" 0 and N.  This
 *     follows from the session's independence contract above: a clip's cross-KV block does not depend on the pass that encoded
 *     it, and a search depends only on its group's slot, its parameters and the options.
 *   - Everything is validated before anything changes, TTASR_E_INVALID: an id that is unknown, not held or listed twice; hold
 *     mode off; a greedy session; whatever ttasr_session_submit_windows refuses for these arguments; TTASR_TOKEN_DETECT in a
 *     prompt (the language is known by then).  After a refusal the clips are still held and can be aligned or released.
 * A session that never calls it enqueues exactly what it did before the call existed. */
TTASR_API int ttasr_session_retry(ttasr_ctx* ctx, int32_t n, const int64_t* ids, const int32_t* prompt, const int32_t* prompt_len,
                                  const int32_t* sot_index, const int32_t* max_new, const float* temperature, const int32_t* rows,
                                  const uint32_t* seed, int64_t* out_ids);
/* Host-side dynamic time warping over a row-major cost matrix [n_rows][n_cols] (tokens x frames): the monotone path
 * of minimum total cost from (0,0) to (n_rows-1, n_cols-1); out_row / out_col need n_rows + n_cols entries.  Pure CPU
 * (no context): CTranslate2 does this step in C++ too. */
TTASR_API int ttasr_dtw(const float* cost, int32_t n_rows, int32_t n_cols, int32_t* out_row, int32_t* out_col, int32_t* out_len);

/* ---- voice activity detection: the Silero-v5-shaped network, 16 kHz branch (faster-whisper's vad_filter=True, requested at
 * asr_core.py:163, file_asr.py:284,461, faster_whisper_asr.py:144) ------------------------------------------------------ */
/* One speech probability per 512-sample frame (32 ms) of every recording of the call, all arithmetic f32 in every compute mode.
 * Framing: n_frames = ceil(n_samples / 512), the recording zero-padded to 512 * n_frames samples; frame i reads the 64 samples
 * before it (zeros before sample 0) and its own 512; the LSTM state (h, c) is zero at the start of a recording.  Per frame: right
 * reflect pad by 64 -> strided correlation with the [258][1][256] STFT basis (stride 128, 4 columns) -> magnitude [129][4] -> four
 * Conv1d (k = 3, zero pad 1) + ReLU, 129 -> 128 s1, 128 -> 64 s2, 64 -> 64 s2, 64 -> 128 s1 -> LSTM cell 128 -> 128 (gates i, f,
 * g, o) -> logit = b_out + < w_out, relu(h') >, p = sigmoid(logit).  DESIGN.md section 4.20 has the kernels; faithfulness to the
 * file Silero ships is NOT checked anywhere (no weights offline): the network is held to a float64 restatement of this text.
 *
 * ttasr_vad_load_tensor: one tensor, float32 host data, Silero state-dict name (a leading "_model." is stripped):
 *   stft.forward_basis_buffer [258,1,256]; encoder.{0..3}.reparam_conv.weight [128,129,3] [64,128,3] [64,64,3] [128,64,3] and
 *   .bias [128] [64] [64] [128]; decoder.rnn.weight_ih / weight_hh [512,128]; decoder.rnn.bias_ih / bias_hh [512];
 *   decoder.decoder.2.weight [1,128,1]; decoder.decoder.2.bias [1].
 *   Unknown name or wrong shape: TTASR_E_WEIGHTS.  After ttasr_vad_finalize, and in an open session: TTASR_E_INVALID.
 *   The weights (1.3 MB) belong to THIS context: a ttasr_create_shared context loads its own copy.
 * ttasr_vad_finalize: TTASR_E_WEIGHTS when a tensor is missing; afterwards the weights are read-only.
 * ttasr_vad_probs: n recordings, recording i = pcm_host[i][0 .. n_samples[i]); out_probs_host[i] (and out_logits_host[i] when
 *   out_logits_host != NULL: the pre-sigmoid values) receive ceil(n_samples[i] / 512) floats.  A recording of 0 samples is legal
 *   and writes nothing (its pointers may be NULL).  Refused with TTASR_E_INVALID before anything is enqueued, the context stays
 *   usable: VAD weights not finalized; n outside [1, max_batch]; a NULL array; a NULL pcm or output row with samples; a negative
 *   length; an open session; a call already in flight on the context.
 *   Work proceeds in time chunks of TTASR_VAD_CHUNK_FRAMES frames per recording (about 33 s): host PCM is staged through a
 *   bounded pinned buffer chunk by chunk, the LSTM state and the 64-sample context carry across chunks, and every kernel's form
 *   is a function of the frame only - a recording's values do not depend, bit for bit, on its length, on the other recordings of
 *   the call or on its place in it, and the first k values equal those of the recording cut to 512 k samples.
 *   Device scratch: n x (4 (64 + 512 C) + 2048 C + 8 C + 1032) bytes with C = TTASR_VAD_CHUNK_FRAMES (4.01 MiB per recording,
 *   at most max_batch of them; never a function of the recordings' lengths), ONE block owned by the context: allocated by the
 *   first call, grown when a call brings more recordings, freed by ttasr_destroy; a request that cannot be allocated returns
 *   TTASR_E_NOMEM and leaves the context usable.  The pinned staging block (8 chunk slots of PCM + max_batch rows of results) is
 *   allocated by the first call as well.
 *   The call touches no mel, encoder, search or graph state: a ttasr_generate* after it is bit-identical to one without it. */
#define TTASR_VAD_CHUNK_FRAMES 1024
TTASR_API int ttasr_vad_load_tensor(ttasr_ctx* ctx, const char* name, const float* data_host, const int64_t* dims, int32_t ndim);
TTASR_API int ttasr_vad_finalize(ttasr_ctx* ctx);
TTASR_API int ttasr_vad_probs(ttasr_ctx* ctx, int32_t n, const float* const* pcm_host, const int64_t* n_samples,
                              float* const* out_probs_host, float* const* out_logits_host);

/* ---- stateful streaming VAD: the same network over recordings that arrive in pieces (the streaming server's
 * vad_pipeline.detect_activity(client), buffering_strategies.py:104-126, asked again for every 1.5-s chunk) ------------------- */
/* A stream is ONE recording that arrives in pieces.  It owns its LSTM state (h, c) in a device table
 * [TTASR_VAD_MAX_STREAMS][256] of the context and, on the host inside the context, the last 64 evaluated samples and the pending
 * samples (at most 511) that do not fill a frame yet.
 *
 * ttasr_vad_stream_open: a new stream with zero state and nothing pending; *out_id receives its id (0 ... TTASR_VAD_MAX_STREAMS
 *   - 1; ids of closed streams are handed out again).  The FIRST open of a context allocates everything the stream path ever
 *   needs - the 1 MiB state table, the pinned staging, and the scratch block of ttasr_vad_probs sized for max_batch recordings (the
 *   two paths share that block) - so device memory is the offline block for max_batch recordings plus the table, never a function of
 *   the number of rows of a push or of their lengths.  Refused (TTASR_E_INVALID) in an open session, because it may allocate,
 *   without finalized VAD weights, and when TTASR_VAD_MAX_STREAMS streams are open.  TTASR_E_NOMEM leaves the context usable.
 * ttasr_vad_stream_reset: the stream is as freshly opened.  ttasr_vad_stream_close: its id is free again.  An id that is not open:
 *   TTASR_E_INVALID.
 * ttasr_vad_stream_push: n rows; row i appends pcm_host[i][0 .. n_samples[i]) to stream ids[i] (0 samples is legal, its pcm may be
 *   NULL).  Every complete 512-sample frame of pending + new samples is evaluated, in order; what is left stays pending.  With
 *   finish != NULL and finish[i] != 0, samples still pending are evaluated as one more frame, zero-padded, and the stream is then as
 *   reset.  out_frames[i] receives the number of values written to out_probs_host[i] (and out_logits_host[i] when out_logits_host
 *   != NULL); the caller provides n_samples[i] / 512 + 2 floats per row (a row that receives no value may be NULL).
 *   THE BIT CONTRACT: the form of every kernel is a function of the frame only, across calls as well as inside one.  However a
 *   recording x is cut into pushes (pieces of 0, 1, 511, 513 ... samples), however the pushes are interleaved with those of other
 *   streams, in whatever order the ids stand and however many rows a call has: the concatenated outputs of a stream whose last push
 *   has finish equal ttasr_vad_probs on x, probabilities and logits, bit for bit; without finish they equal its first
 *   floor(len / 512) values.  Compute modes do not change a bit either.
 *   A push walks its rows in groups of at most max_batch and long inputs in time chunks of TTASR_VAD_CHUNK_FRAMES frames, through
 *   the same chunk loop and per-frame kernels as ttasr_vad_probs; it never allocates.  The stream table is separate from the state
 *   region ttasr_vad_probs zeroes: an offline call between two pushes changes nothing in any stream.
 *   Sessions: push, reset and close are legal while a continuous-batching session is open, between session calls; they use the
 *   context's stream and touch no mel, encoder, search, graph or session state.  ttasr_vad_probs stays refused there.
 *   Refused with TTASR_E_INVALID before anything is enqueued, the context and every stream stay as they were: VAD weights not
 *   finalized (no stream can be open); n < 1 or n above the number of open streams; a NULL ids / pcm_host / n_samples /
 *   out_probs_host / out_frames array; an id that is not open; the same id twice in one call; a negative length; a NULL pcm with
 *   samples; a NULL output row that would receive values; a call already in flight on the context.
 *   A TTASR_E_HIP in the middle of a push leaves the streams of THAT call reset (zero state, nothing pending): the caller feeds
 *   them again from the start of their recordings, or closes them.
 * Streams belong to their context (a ttasr_create_shared context has its own) and everything is freed by ttasr_destroy.
 * The streams described here are FLOAT streams; WIRE streams ("wire streams" below) are fed bytes in a wire format instead.  The
 * two kinds share the ids and the limit of TTASR_VAD_MAX_STREAMS open streams, and each push call takes its own kind only. */
#define TTASR_VAD_MAX_STREAMS 1024
TTASR_API int ttasr_vad_stream_open(ttasr_ctx* ctx, int32_t* out_id);
TTASR_API int ttasr_vad_stream_reset(ttasr_ctx* ctx, int32_t id);
TTASR_API int ttasr_vad_stream_close(ttasr_ctx* ctx, int32_t id);
TTASR_API int ttasr_vad_stream_push(ttasr_ctx* ctx, int32_t n, const int32_t* ids, const float* const* pcm_host,
                                    const int64_t* n_samples, const int32_t* finish, float* const* out_probs_host,
                                    float* const* out_logits_host, int32_t* out_frames);

/* ---- file ingest: raw samples of a file -> float32 mono 16 kHz (what librosa.load(..., sr=16000) does in front of every file
 * entry point of the reference: asr_core.py:156, file_asr.py:271,455; faster-whisper's decode_audio) -------------------------- */
/* The resampler is scipy.signal.resample_poly with its defaults, written out.  For a recording of n_frames frames at `rate`:
 *   g = gcd(rate, 16000), up = 16000 / g, down = rate / g, R = max(up, down), half = 10 R, N = 2 half + 1;
 *   h[m] = up w[m] / sum(w), w[m] = (1 / R) sinc((m - half) / R) kaiser(N, beta = 5)(m), m = 0 .. N - 1, designed in double (the
 *     Kaiser window's I0 by its power series) and rounded to float32;
 *   mono[i] = the mean over the channels of frame i's samples scaled to [-1, 1): u8 (v - 128) / 128, s16 / 32768, packed s24
 *     / 8388608, s32 / 2147483648 (rounded to float32 first), f32 as is, f64 rounded to float32; channels summed in order, then
 *     one division;
 *   n_out = ceil(n_frames up / down);
 *   y[k] = sum_i mono[i] h[k down + half - i up] over the i in [0, n_frames) whose tap index lies in [0, 2 half] (zeros outside
 *     the recording), accumulated in float32 with i ascending.
 * Accepted rates: every rate with R <= 1024 (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000
 * among them).  At rate 16000 there is no filter: y = mono, bit for bit what the host conversion gives.
 *
 * ttasr_ingest_len: n_out of a recording; negative when the rate is not accepted (or n_frames is outside [0, 2^40]).  No context.
 * ttasr_ingest_filter: the float32 taps h[0 .. N) of `rate` - min(cap, N) of them are written when out != NULL - and returns N
 *   (0 at rate 16000: no filter; negative: rate not accepted).  No context, no GPU: the known-answer hook of the design.
 * ttasr_ingest_pcm: n recordings in one call, recording i = n_frames[i] interleaved frames of channels[i] (1 ... 8) samples in
 *   format[i] (TTASR_PCM_*, little endian) at raw_host[i] (any alignment); out_pcm_host[i] receives ttasr_ingest_len(rate[i],
 *   n_frames[i]) floats.  Rates and formats may differ inside a call, n is not limited by max_batch, and no model weights are
 *   needed.  A recording of 0 frames is legal and writes nothing (its pointers may be NULL).  Refused with TTASR_E_INVALID before
 *   anything is enqueued, the context stays usable: a rate that is not accepted; a channel count outside [1, 8]; an unknown
 *   format; a negative frame count; a NULL array; a NULL sample or output row with frames; an open session; a call already in
 *   flight on the context.
 *   One 256-thread workgroup computes a tile of consecutive outputs of one recording from an input span it stages in LDS (the
 *   samples are converted and downmixed on the way in); there are no atomics and an output's operands and their order depend on
 *   its index only.  Recordings go through the device in chunks of input frames - option "ingest_chunk", 0 = as many as the slots
 *   hold - each uploaded with the filter's halo on both sides through 4 pinned slots of 8 MiB (results: 4 x 4 MiB; the same again
 *   in device memory; allocated by the first call, freed by ttasr_destroy).  A recording's values do not depend, bit for bit, on
 *   the chunk size, on the other recordings of the call or on its place in it.  The tap table of a rate (at most 84 KiB) is built
 *   by the first call that brings the rate and kept by the context.
 *   The call touches no mel, encoder, search or graph state. */
#define TTASR_PCM_U8 0
#define TTASR_PCM_S16 1
#define TTASR_PCM_S24 2   /* packed: 3 bytes per sample */
#define TTASR_PCM_S32 3
#define TTASR_PCM_F32 4
#define TTASR_PCM_F64 5
TTASR_API int64_t ttasr_ingest_len(int32_t rate, int64_t n_frames);
TTASR_API int32_t ttasr_ingest_filter(int32_t rate, float* out, int32_t cap);
TTASR_API int ttasr_ingest_pcm(ttasr_ctx* ctx, int32_t n, const void* const* raw_host, const int64_t* n_frames, const int32_t* rate,
                               const int32_t* channels, const int32_t* format, float* const* out_pcm_host);

/* ---- coded WAVE files and the channel pick (G.711 A-law / mu-law, IMA ADPCM: what telephony and voice loggers write) ---------
 * All three codecs decode to int16, and the int16 becomes a float as TTASR_PCM_S16 does (/ 32768).  Everything is integer-exact.
 *   mu-law byte b (WAVE tag 7):  u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, v = (((m << 3) + 0x84) << e) - 0x84;
 *     the sample is -v if u & 0x80, else v (range +-32124).
 *   A-law byte b (WAVE tag 6):  a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, v = (m << 4) + 8, and v = (v + 0x100) << (e - 1)
 *     if e >= 1; the sample is v if a & 0x80, else -v (range +-32256).
 *   IMA ADPCM (WAVE tag 0x11, 4 bits per sample): the data are blocks of block_align bytes.  A block starts with one 4-byte header
 *     per channel, in channel order: int16 LE predictor, uint8 step index, one reserved byte; the header predictor is that
 *     channel's first sample of the block.  The data follow in groups of 4 bytes per channel, interleaved channel by channel; a
 *     group holds 8 samples of one channel, low nibble first.  Samples per block: spb = 1 + 2 (block_align / channels - 4).  Per
 *     nibble n, with the 89-entry step table (7, 8, 9, ... 32767) and the index steps {-1, -1, -1, -1, 2, 4, 6, 8} taken at n & 7:
 *     d = step >> 3, + step if n & 4, + step >> 1 if n & 2, + step >> 2 if n & 1; the predictor moves by -d if n & 8, else by +d,
 *     and is clamped to int16; the index is clamped to [0, 88].  A header step index above 88 is read as 88.  Bytes behind the
 *     last whole block are ignored; n_frames is at most blocks * spb (a `fact` chunk may make it shorter).
 *   Channel pick: pick = -1 is the mean of ttasr_ingest_pcm (channels summed in order, one division); pick = c in [0, channels)
 *     takes channel c's converted sample as is, with no division - the recording is then channel c as a mono recording.
 *
 * ttasr_ingest_wave: ttasr_ingest_pcm for the six TTASR_PCM_* codes above and the three below, with a pick per recording (pick =
 *   NULL: -1 everywhere).  n_bytes[i] is what raw_host[i] holds; block_align[i] is read for TTASR_PCM_IMA4 only (block_align = NULL
 *   is legal when no recording is IMA).  Refused like ttasr_ingest_pcm, before anything is enqueued and with the context left
 *   usable, and also: a pick outside [-1, channels); IMA with a block_align that is no multiple of 4 channels, below 8 channels or
 *   above 65536; n_frames beyond what n_bytes hold (IMA: beyond (n_bytes / block_align) spb); a NULL n_bytes.
 *   G.711 is decoded arithmetically inside the ingest kernel.  IMA recordings go through a pre-pass first: one lane per (block,
 *   channel), consecutive lanes on consecutive blocks of a channel, writes int16 [frames][channels] into a device scratch block of
 *   the context (8 MiB, allocated by the first call that needs it, freed by ttasr_destroy), which the ingest kernel then reads as
 *   TTASR_PCM_S16.  IMA chunks are cut on block boundaries: "ingest_chunk" counts frames and is rounded up to whole blocks.
 *   For every accepted recording the result equals, bit for bit, ttasr_ingest_pcm fed the decoded int16 (with a pick: fed that
 *   one channel as a mono recording), and depends neither on the chunk size nor on the other recordings of the call nor on its
 *   place in it. */
#define TTASR_PCM_ALAW 16
#define TTASR_PCM_ULAW 17
#define TTASR_PCM_IMA4 18
TTASR_API int ttasr_ingest_wave(ttasr_ctx* ctx, int32_t n, const void* const* raw_host, const int64_t* n_bytes, const int64_t* n_frames,
                                const int32_t* rate, const int32_t* channels, const int32_t* format, const int32_t* block_align,
                                const int32_t* pick, float* const* out_pcm_host);

/* ---- FLAC files (RFC 9639; the folder tool, the file service and the reference all list *.flac) ----------------------------------
 * The stream that is accepted: an optional ID3v2 tag, "fLaC", the metadata blocks with STREAMINFO (34 bytes) first and every other
 * type skipped (type 127 is invalid), then frames back to back up to the end of the data or to a 128-byte ID3v1 tag ("TAG").  1 to 8
 * channels, 4 to 24 bits per sample, every blocksize from 1 to 65535, both blocking strategies, constant / verbatim / fixed (order
 * 0 ... 4) / LPC (order 1 ... 32) subframes, both Rice methods with escape partitions, wasted bits, and the three stereo codes.  Ogg
 * FLAC is out of scope.  Refused, each with a message that says which: 25 to 32 bits; a frame whose rate, channel count or width
 * differs from STREAMINFO's; a reserved code; a broken CRC-8 or CRC-16; a coded number that does not continue the previous frame
 * (fixed blocking + 1, variable blocking + the previous blocksize; the first frame may start anywhere); bytes behind the last frame
 * that are no ID3v1 tag; more than 2^40 samples.
 *   Frame scan (host): a frame starts where a header is valid - its fields, its CRC-8, the stream's parameters, the continuity - and
 *     ends at the smallest q where the two bytes before q are the CRC-16 (0x8005, init 0, MSB first) of the frame up to them AND q is
 *     the end of the data or the start of a valid continuing header: one table-driven CRC pass over the file.  A q where the CRC-16
 *     holds and a sync code stands, but no valid continuing header, is passed over - such bytes occur inside valid frames - and only
 *     serves the message: when the frame found at last does not decode while the bytes up to that q do, the file is refused for
 *     the damaged header at q (its CRC-8, a reserved code, its parameters, its number).  STREAMINFO's frame sizes are not used.
 *     The samples HELD are the sum of the blocksizes found, whatever STREAMINFO's total says.
 *   Sample value: an integer v of a `bits`-wide stream is the float v / 2^(bits - 1).  The decoder left-justifies: v << (16 - bits)
 *     as int16 for bits <= 16, v << (32 - bits) as int32 otherwise, and the result is read as TTASR_PCM_S16 / TTASR_PCM_S32.  All
 *     decoder arithmetic is integer and wraps; a malformed stream has no undefined behaviour.
 *   Status word of a frame (the decode body, the same code on the host and on the device): 0 ok, 1 reserved subframe type or field,
 *     or a padding bit in front of the CRC-16 that is set,
 *     2 LPC precision 1111 or negative shift, 3 a partition order that does not divide the blocksize or leaves less than the order,
 *     4 the subframes run past the end of the frame, 5 the header disagrees with the frame table or the stream, 6 the subframes end
 *     before the frame does.
 *
 * The three functions below need no context and no GPU.  `why` (may be NULL), of `why_len` bytes, receives the reason of a refusal.
 * ttasr_flac_probe: out[0] rate, [1] channels, [2] bits per sample, [3] samples per channel held, [4] the number of FLAC frames,
 *   [5] the largest blocksize, [6] the byte offset of the first frame, [7] flags: 1 = STREAMINFO carries an MD5, 2 = STREAMINFO's
 *   total is set and disagrees with what is held.  TTASR_OK, or TTASR_E_INVALID for a refused stream.
 * ttasr_flac_frames: the scan's known-answer hook.  Returns the number of frames (negative: refused) and writes min(cap, frames)
 *   rows (byte offset, byte length, first sample) to `table` when it is not NULL.
 * ttasr_flac_decode: the host decoder.  out[sample][channel] receives the plain integers v (not left-justified); cap_samples is
 *   the number of samples per channel `out` takes.  Returns the samples per channel decoded, or TTASR_E_INVALID for a refused
 *   stream, a frame with a status word other than 0 (the message names the frame) or an output that is too small.  The frames are
 *   decoded one after the other on the calling thread.  The MD5 is the caller's to check (over the samples interleaved, each a
 *   little-endian signed number of ceil(bits / 8) bytes).
 *
 * TTASR_PCM_FLAC in ttasr_ingest_wave: raw_host[i] / n_bytes[i] are the whole file as read, ID3 tags and metadata included;
 *   rate[i] and channels[i] must equal what the stream says; n_frames[i] is at most the samples held; block_align[i] is ignored;
 *   pick works as for every other format.  Everything ttasr_flac_probe refuses is refused here too, before anything is enqueued and
 *   with the context left usable.  Wire streams refuse the format, as they refuse IMA.
 *   FLAC chunks are cut on FLAC frame boundaries ("ingest_chunk" is rounded up to whole FLAC frames).  A chunk uploads the bytes of
 *   its frames - and of the frames the filter's halo touches on both sides - behind a table with one entry per frame (offset in the
 *   slot, length, first sample, blocksize).  The pre-pass runs one lane per FLAC frame over that table: the decode body writes the
 *   left-justified int16 / int32 [samples][channels] into a device scratch block, which the ingest kernel then reads as
 *   TTASR_PCM_S16 / TTASR_PCM_S32, unchanged.  The scratch is 64 MiB + 1 MiB of device memory - 32 MiB for the decoded chunk, 32 MiB
 *   for the lanes' int32 work rows, each 16 of the largest legal frames (65535 samples x 8 channels x 4 B), so that a frame and its
 *   halo frames always fit, and one status word per frame and slot - with 1 MiB of pinned status words; allocated by the first FLAC
 *   call, freed by ttasr_destroy.  A chunk must also fit a result slot: a single FLAC frame that resamples to more than 2^20
 *   outputs (65535 samples at a rate below 1 kHz) is refused, like everything else before anything is enqueued.
 *   A frame whose content is illegal although its CRC-16 holds makes the call return TTASR_E_INVALID with a message naming the
 *   recording, the frame and the status word's meaning: every lane writes its status word with an ordinary store and the words
 *   return with the chunk.  The context stays usable; that call's outputs are unspecified.
 *   For every accepted recording the result equals, bit for bit, ttasr_ingest_pcm fed the left-justified integers as TTASR_PCM_S16
 *   / TTASR_PCM_S32 (with a pick: fed that one channel as a mono recording), and depends neither on the chunk size nor on the other
 *   recordings of the call nor on its place in it. */
#define TTASR_PCM_FLAC 32
TTASR_API int ttasr_flac_probe(const void* bytes, int64_t n_bytes, int64_t* out, char* why, int32_t why_len);
TTASR_API int64_t ttasr_flac_frames(const void* bytes, int64_t n_bytes, int64_t* table, int64_t cap, char* why, int32_t why_len);
TTASR_API int64_t ttasr_flac_decode(const void* bytes, int64_t n_bytes, int32_t* out, int64_t cap_samples, char* why, int32_t why_len);

/* ---- wire streams: a VAD stream fed the BYTES of a live connection (the streaming server's `rate` 8000 | 16000 and `channel`
 * 1 | 2 query parameters, the config message's sampleRate / channels; G.711 telephony with one party per channel) ----------------
 * A wire stream is a VAD stream (above) opened with a wire format: rate, channels (1 ... 8), format (the six TTASR_PCM_* sample
 * formats, TTASR_PCM_ALAW, TTASR_PCM_ULAW; TTASR_PCM_IMA4 is a block codec and is refused) and pick (-1 the mean of the channels,
 * c channel c, as in ttasr_ingest_wave).  It is ONE recording that arrives as bytes in pieces; a piece may end inside a sample.
 * The arithmetic is that of ttasr_ingest_pcm - up, down, half, h, mono, y[k], n_out as defined there - made stateful:
 *   final outputs: y[k] is final once every input it reads has arrived; its last input is floor((k down + half) / up).  After F
 *     whole frames the final outputs are k < K(F) = max(0, ceil((F up - half) / down)) (K(F) = F at 16000); with finish all
 *     n_out(F) = ceil(F up / down) are final, inputs past the end counting as absent, as they do offline;
 *   history: outputs from K(F) on read at most the last H = floor(2 half / up) frames.  The stream keeps those H mono values -
 *     converted and downmixed, f32 - in a device table [2][TTASR_VAD_MAX_STREAMS][256] of the context, which is never uploaded;
 *   pending bytes: bytes that do not fill a frame (channels x sample size, at most 63) wait on the host inside the context.
 * A stream rate is a rate ttasr_ingest_len accepts with H <= 255: every rate listed above up to 192000 (H = 240); 384000 is not.
 *
 * ttasr_ingest_stream_len: the number of final outputs after n_frames frames at `rate` - K(n_frames), or n_out(n_frames) when
 *   finished != 0; negative for a rate that is no stream rate (or n_frames outside [0, 2^40]).  No context.
 * ttasr_vad_stream_open_wire: ttasr_vad_stream_open for a wire stream.  The first one of a context also allocates what wire
 *   streams ever need: the 2 MiB history table, one device block and one pinned block of 8 MiB raw bytes + 8 MiB results + the
 *   job table; every open builds the tap table of its rate when the context has none yet.  Refused like ttasr_vad_stream_open
 *   (an open session included), and for TTASR_PCM_IMA4 or an unknown format, channels outside [1, 8], a pick outside
 *   [-1, channels), and a rate for which ttasr_ingest_stream_len is negative.  Both kinds share the ids and the limit of
 *   TTASR_VAD_MAX_STREAMS open streams; ttasr_vad_stream_reset (history, pending bytes and VAD state: as freshly opened, without
 *   touching the device) and ttasr_vad_stream_close serve both.
 * ttasr_vad_stream_push_wire: n rows; row i appends raw_host[i][0 .. n_bytes[i]) to wire stream ids[i] (0 bytes is legal).  The
 *   outputs that become final are written to out_pcm_host[i] (out_pcm_host, or a row of it, may be NULL: the samples are not
 *   returned) and counted in out_pcm_len[i]; out_pcm_cap[i] floats must hold them (ttasr_ingest_stream_len gives the number).  The
 *   same samples enter the stream's VAD framing exactly as ttasr_vad_stream_push would take them - 512-sample frames, 64-sample
 *   context, the same finish rule - and out_probs_host / out_logits_host / out_frames mean what they mean there (the caller
 *   provides final outputs / 512 + 2 floats per row).  With finish[i] the stream is afterwards as reset; bytes that fill no frame
 *   are dropped then.
 *   THE BIT CONTRACT.  Let the last push of a stream carry finish.  However the bytes of a recording are cut into pushes (pieces
 *   of 0 bytes, 1 byte, cuts inside a sample, H - 1 or H + 1 frames), however the pushes share calls with streams of other rates
 *   and formats, in whatever row order and under any "wire_chunk": the concatenated out_pcm of the stream equals ttasr_ingest_wave
 *   on the whole recording with the same pick, bit for bit, and the concatenated probabilities and logits equal ttasr_vad_probs on
 *   that result, bit for bit.  Without finish they equal its first K(F) samples and first floor(K(F) / 512) values.  An output's
 *   operands and their order depend on its index alone (i ascending, as offline); there are no atomics.
 *   ONE launch per push chunk serves all rows: a job table in device memory has one entry per row, a 256-thread workgroup takes a
 *   tile of outputs of one row and stages its span in LDS - the row's history from the table, then the new frames, converted and
 *   downmixed on the way in - and one more workgroup per row writes the row's new history into the OTHER half of the table (the
 *   halves flip per chunk and stream: no workgroup reads what another writes).  The results return through the pinned block and
 *   enter the chunk loop of ttasr_vad_stream_push, which enqueues what it always did.  A push of any size is legal: it is walked
 *   in chunks of as many frames per row as the row's share (1 / n) of the pools holds, or option "wire_chunk" when that is
 *   smaller.  The call never allocates and is legal while a session is open, like ttasr_vad_stream_push.
 *   Refused with TTASR_E_INVALID before anything is enqueued, the context and every stream stay as they were: everything
 *   ttasr_vad_stream_push refuses; a float stream's id here, or a wire stream's id in ttasr_vad_stream_push; a NULL n_bytes or
 *   out_pcm_len; an out_pcm_cap[i] (or a NULL out_pcm_cap) below the final outputs of a row whose samples are returned.
 *   A TTASR_E_HIP in the middle of a push leaves the streams of THAT call reset. */
TTASR_API int64_t ttasr_ingest_stream_len(int32_t rate, int64_t n_frames, int32_t finished);
TTASR_API int ttasr_vad_stream_open_wire(ttasr_ctx* ctx, int32_t rate, int32_t channels, int32_t format, int32_t pick, int32_t* out_id);
TTASR_API int ttasr_vad_stream_push_wire(ttasr_ctx* ctx, int32_t n, const int32_t* ids, const void* const* raw_host, const int64_t* n_bytes,
                                         const int32_t* finish, float* const* out_pcm_host, const int64_t* out_pcm_cap, int64_t* out_pcm_len,
                                         float* const* out_probs_host, float* const* out_logits_host, int32_t* out_frames);

/* ---- segmentation VAD: the PyanNet-shaped network (the streaming server's PyannoteVAD, pyannote_vad.py:12-62, which runs
 * pyannote/segmentation under VoiceActivityDetection(onset 0.5, offset 0.5, min_duration_on 0.3, min_duration_off 0.3)) ----------- */
/* UNPINNED against the published pyannote/segmentation checkpoint: neither pyannote.audio nor the checkpoint exists offline, so
 * the tensor names, the ParamSincFB filter formula, the Hamming aggregation window and the Binarize rules are restated from
 * memory, and the network is held to a float64 restatement of THIS text on synthetic weights.
 *
 * The network (PyanNet defaults; all arithmetic f32 on the device in every compute mode).  Input: 16 kHz mono float32, in chunks
 * of 80 000 samples; chunk k starts at sample 8 000 k; a recording of n samples has K(n) = 0 chunks for n = 0, 1 for n <= 80 000,
 * else 1 + ceil((n - 80 000) / 8 000); the last chunk is zero-padded.  Per chunk (every norm: biased variance, eps 1e-5):
 *   1. InstanceNorm1d(1, affine) over the chunk;
 *   2. sinc convolution 1 -> 80 channels, kernel 251, stride 10, no bias, with the materialised filters [80,1,251] (the host
 *      builds them in float64 from the checkpoint's 40 low_hz_ / band_hz_ pairs: min_low_hz = min_band_hz = 50, 125-point half
 *      Hamming window, 40 cosine then 40 sine filters, each divided by twice its band), then abs: 80 000 -> 7 975;
 *   3. MaxPool1d(3,3) -> 2 658, InstanceNorm1d(80, affine), leaky_relu(0.01);
 *   4. Conv1d(80 -> 60, k 5) -> 2 654, pool 3 -> 884, InstanceNorm1d(60, affine), leaky_relu;
 *   5. Conv1d(60 -> 60, k 5) -> 880, pool 3 -> 293 frames, InstanceNorm1d(60, affine), leaky_relu;
 *   6. LSTM, input 60, hidden 128, 4 layers, bidirectional, gates i, f, g, o with bias_ih + bias_hh, layers 1-3 on the 256-wide
 *      forward | backward concatenation, zero initial state per chunk;
 *   7. Linear(256 -> 128), leaky_relu, Linear(128 -> 128), leaky_relu, Linear(128 -> C), sigmoid; C in [1, 8] = classifier.weight's
 *      first dimension.
 * A frame's receptive field is 991 samples and its step 270: frame j is centred on sample 495 + 270 j.  The speech score of a
 * chunk frame is the maximum over its C classes.  Aggregation (deterministic overlap-add): chunk k's frame f lands on recording
 * frame s(k) + f, s(k) = (8 000 k + 135) / 270 in integer division; score[j] = sum_k w[f] p_k[f] / sum_k w[f] over the chunks
 * that cover j, k ascending, w = hamming(293) = 0.54 - 0.46 cos(2 pi f / 292) rounded to f32; a recording has
 * F(n) = min(ceil(n / 270), s(K - 1) + 293) frames.
 *
 * ttasr_seg_load_tensor: one tensor, float32 host data, PyanNet state-dict name: sincnet.wav_norm1d.weight | bias [1];
 *   sincnet.conv1d.0.filters [80,1,251] (derived, see 2.); sincnet.norm1d.{0,1,2}.weight | bias [80] [60] [60];
 *   sincnet.conv1d.1.weight [60,80,5], .bias [60]; sincnet.conv1d.2.weight [60,60,5], .bias [60];
 *   lstm.weight_ih_l{0..3}[_reverse] [512,60] (layer 0) / [512,256]; lstm.weight_hh_l*[_reverse] [512,128];
 *   lstm.bias_ih_l*[_reverse], lstm.bias_hh_l*[_reverse] [512]; linear.0.weight [128,256], linear.1.weight [128,128], their .bias
 *   [128]; classifier.weight [C,128], classifier.bias [C]: 51 tensors.  Unknown name or wrong shape: TTASR_E_WEIGHTS.  After
 *   ttasr_seg_finalize, and in an open session: TTASR_E_INVALID.  The weights (5.9 MB) belong to THIS context.
 * ttasr_seg_finalize: TTASR_E_WEIGHTS when a tensor is missing or the classifier's weight and bias disagree on C; afterwards the
 *   weights are read-only.  ttasr_seg_classes: C of the finalized network (TTASR_E_INVALID before).
 * ttasr_seg_chunks / ttasr_seg_frames: K(n) and F(n); no context; negative for n outside [0, 2^40].
 * ttasr_seg_scores: n recordings, recording i = pcm_host[i][0 .. n_samples[i]); out_scores_host[i] receives F(n_i) floats.  The
 *   two optional arrays are the known-answer hooks: row i of out_chunk_probs_host / out_chunk_logits_host, when the array is not
 *   NULL, receives [K_i][293][C] per-class probabilities / pre-sigmoid logits.  A recording of 0 samples is legal and writes
 *   nothing (its pointers may be NULL).  Refused with TTASR_E_INVALID before anything is enqueued, the context stays usable:
 *   weights not finalized; n outside [1, max_batch]; a NULL array; a NULL pcm or output row with samples; a length outside
 *   [0, 2^40]; an open session; a call already in flight on the context.
 *   Work proceeds in groups of at most TTASR_SEG_GROUP chunks - the recordings in call order, chunks ascending - and every
 *   kernel's form is a function of the chunk only: a chunk's 293 x C values depend on its 80 000 samples alone, bit for bit - not
 *   on the recording it is cut from, the other recordings of the call, its place in the call, the group it runs in, the compute
 *   mode or option "seg_lstm_rows" - and a frame's score on its covering chunks, summed in ascending order.
 *   Device scratch: ONE block owned by the context, allocated by the first call, never a function of the recordings' lengths,
 *   freed by ttasr_destroy: per chunk of a group 4 x (80 000 PCM + 80 x 2 658 + 60 x 884 + 60 x 293 stage outputs + 2 x 293 x 512
 *   gate inputs + 2 x 293 x 256 layer outputs + 2 x 293 x 8 head outputs + 293 scores + 326 aggregated frames) + 1 664 bytes of
 *   statistics and tables = 3 276 124 bytes, times TTASR_SEG_GROUP, + 10 x 293 x 4 (the scores of the chunks in front of a group)
 *   + 293 x 4 (the window), every region rounded up to 256 bytes: 200 MiB.  Host PCM goes through a pinned staging block of
 *   TTASR_SEG_GROUP x 320 000 bytes (+ the group's tables and results, 21 MiB in all), allocated by the first call as well.
 *   A block that cannot be allocated: TTASR_E_NOMEM, the context stays usable.
 *   The call touches no mel, encoder, search, graph, session or Silero state: a ttasr_generate* or ttasr_vad_probs after it is
 *   bit-identical to one without it. */
#define TTASR_SEG_GROUP 64
#define TTASR_SEG_CHUNK_FRAMES 293
TTASR_API int ttasr_seg_load_tensor(ttasr_ctx* ctx, const char* name, const float* data_host, const int64_t* dims, int32_t ndim);
TTASR_API int ttasr_seg_finalize(ttasr_ctx* ctx);
TTASR_API int ttasr_seg_classes(ttasr_ctx* ctx);
TTASR_API int64_t ttasr_seg_chunks(int64_t n_samples);
TTASR_API int64_t ttasr_seg_frames(int64_t n_samples);
TTASR_API int ttasr_seg_scores(ttasr_ctx* ctx, int32_t n, const float* const* pcm_host, const int64_t* n_samples,
                               float* const* out_scores_host, float* const* out_chunk_probs_host, float* const* out_chunk_logits_host);

/* ---- speaker embeddings: the XVectorSincNet-shaped network (the embedding model that pairs with pyannote/segmentation in a
 * pyannote-style diarization pipeline; the reference service's DIA subtitle type, api/file_asr.py:591-632, has no speaker
 * labelling behind it yet) ------------------------------------------------------------------------------------------------------- */
/* UNPINNED against the published pyannote/embedding checkpoint: neither pyannote.audio nor the checkpoint exists offline, so the
 * tensor names, the layer table, the pooling formula and the nearest-neighbour resampling of the weights are restated from
 * memory, and the network is held to a float64 restatement of THIS text on synthetic weights (tests/xvector_reference.py).
 *
 * The network (all arithmetic f32 on the device in every compute mode).  Input and chunking are ttasr_seg_scores': 16 kHz mono
 * float32, chunks of 80 000 samples, chunk k starts at sample 8 000 k, K(n) = ttasr_seg_chunks(n), the last chunk zero-padded.
 * Per chunk:
 *   1. the SincNet front end of the segmentation network with weights of its own (steps 1.-5. of that text: waveform
 *      InstanceNorm1d(1, affine); 80 sinc filters of 251 taps, stride 10, abs, MaxPool1d(3), InstanceNorm1d(80, affine),
 *      leaky_relu(0.01); Conv1d(80 -> 60, k 5), pool 3, norm, leaky_relu; Conv1d(60 -> 60, k 5), pool 3, norm, leaky_relu):
 *      [60][293];
 *   2. five TDNN blocks, each Conv1d (no padding, with bias) -> leaky_relu(0.01) -> BatchNorm1d in eval mode
 *      ((x - running_mean) / sqrt(running_var + 1e-5) * weight + bias):
 *        block   cin -> cout   kernel   dilation   frames out
 *          1      60 ->  512     5         1          289
 *          2     512 ->  512     3         2          285
 *          3     512 ->  512     3         3          279
 *          4     512 ->  512     1         1          279
 *          5     512 -> 1500     1         1          279
 *   3. weighted statistics pooling, once per mask w[293] >= 0 of the chunk: w'[j] = w[(293 j) / 279] in integer division for
 *      j < 279 (torch's interpolate(mode="nearest"); frames 20, 41, 62, ..., 292 of the 293 - fourteen of them, 146 and 292 among
 *      them - are read by no j), v1 = sum w', v2 = sum w'^2, mean_c = sum w' x_c / v1,
 *      var_c = sum w' (x_c - mean_c)^2 / (v1 - v2 / v1 + 1e-8), std_c = sqrt(var_c); the result is [mean | std], 3 000 values;
 *   4. embedding = Linear(3 000 -> D), D = embedding.weight's first dimension, 1 <= D <= TTASR_SPK_MAX_DIM.
 *
 * ttasr_spk_load_tensor: one tensor, float32 host data, state-dict name: the 13 sincnet.* names and shapes of
 *   ttasr_seg_load_tensor (sincnet.conv1d.0.filters derived from the checkpoint's cutoffs in the same way);
 *   tdnns.{0,3,6,9,12}.weight [cout,cin,kernel] and .bias [cout]; tdnns.{2,5,8,11,14}.weight | bias | running_mean | running_var
 *   [cout] (num_batches_tracked is not a tensor of the network); embedding.weight [D,3000], embedding.bias [D]: 45 tensors.
 *   Unknown name or wrong shape: TTASR_E_WEIGHTS.  After ttasr_spk_finalize, and in an open session: TTASR_E_INVALID.  The weights
 *   (up to 13.5 MB) belong to THIS context.
 * ttasr_spk_finalize: TTASR_E_WEIGHTS when a tensor is missing or embedding.weight and embedding.bias disagree on D; afterwards
 *   the weights are read-only.  ttasr_spk_dim: D of the finalized network (TTASR_E_INVALID before).
 * ttasr_spk_embed: n recordings, recording i = pcm_host[i][0 .. n_samples[i]) with K_i = ttasr_seg_chunks(n_samples[i]) chunks;
 *   weights_host[i] is float32 [K_i][S][293], S = n_masks in [1, TTASR_SPK_MAX_MASKS]: S frame-weight masks for every chunk, on the
 *   segmentation network's frame grid; out_emb_host[i] receives [K_i][S][D].  The optional array out_stats_host is the
 *   known-answer hook: row i, when the array is not NULL, receives the pooled [K_i][S][3000].  A one-hot mask on a frame that the
 *   resampling reads makes `mean` the block-5 output of ONE frame, so the hook shows single frames without reading the 1.6 MB of
 *   a chunk's block-5 output back.  A mask whose RESAMPLED weights sum to 0 (all zeros, or weight on unread frames only): its D
 *   and 3 000 values are written as quiet NaN, nothing is computed from them, and the other masks of the chunk are unaffected.  A
 *   recording of 0 samples is legal and writes nothing (its pointers may be NULL).  Refused with TTASR_E_INVALID before anything
 *   is enqueued, the context stays usable: weights not finalized; n outside [1, max_batch]; n_masks out of range; a NULL array; a
 *   NULL pcm, weights or output row with samples; a length outside [0, 2^40]; a weight that is negative or not finite; an open
 *   session; a call already in flight on the context.
 *   Work proceeds in groups of at most TTASR_SPK_GROUP chunks - the recordings in call order, chunks ascending.  The TDNN blocks
 *   do not read the masks: they run once per chunk and their output is pooled S times.  Every tile of the block kernels lies
 *   inside one chunk, an output row of the GEMM body is a function of its own operand row and the weights with k ascending, and
 *   the pooling's sums run over the frames in ascending order: the D and 3 000 values of (chunk, mask) depend on the chunk's
 *   80 000 samples and that mask alone, bit for bit - not on the recording, the call, the group, S, the other masks or the
 *   compute mode.
 *   Device scratch: ONE block owned by the context, allocated by the first call, never a function of the recordings' lengths,
 *   freed by ttasr_destroy: per chunk of a group 4 x (80 000 PCM + 80 x 2 658 + 60 x 884 + 60 x 293 stage outputs + 2 x 289 x 512
 *   ping-pong block outputs + 279 x 1 500 block-5 output + 8 x (293 weights + 1 flag + 3 000 pooled + 512 embedding)) + 1 616
 *   bytes of statistics and tables = 4 434 192 bytes, times TTASR_SPK_GROUP, every region rounded up to 256 bytes: 68 MiB.
 *   TTASR_SPK_GROUP = 16: block 2's grid is then 5 x 4 x 16 = 320 workgroups on 256 CUs, and a group's reference costs a test a
 *   few seconds.  Host data goes through a pinned staging block of TTASR_SPK_GROUP x 320 000 bytes of PCM + the group's tables,
 *   masks and results: 7 MiB, allocated by the first call as well.  A block that cannot be allocated: TTASR_E_NOMEM, the context
 *   stays usable.
 *   The call touches no mel, encoder, search, graph, session, Silero or segmentation state: a ttasr_generate*, ttasr_vad_probs
 *   or ttasr_seg_scores after it is bit-identical to one without it. */
#define TTASR_SPK_GROUP 16
#define TTASR_SPK_MAX_MASKS 8
#define TTASR_SPK_MAX_DIM 512
#define TTASR_SPK_STATS 3000
TTASR_API int ttasr_spk_load_tensor(ttasr_ctx* ctx, const char* name, const float* data_host, const int64_t* dims, int32_t ndim);
TTASR_API int ttasr_spk_finalize(ttasr_ctx* ctx);
TTASR_API int ttasr_spk_dim(ttasr_ctx* ctx);
TTASR_API int ttasr_spk_embed(ttasr_ctx* ctx, int32_t n, const float* const* pcm_host, const int64_t* n_samples, int32_t n_masks,
                              const float* const* weights_host, float* const* out_emb_host, float* const* out_stats_host);

/* ---- audio enhancement ("dspMode"): denoise, high-pass, level -------------------------------------- */
/* One length-preserving call over float32 mono 16 kHz recordings: out has the samples of the input, so times, VAD frames and
 * word timestamps keep their meaning.  The definition is THIS PROJECT'S OWN (the product publishes none); its effect on CER is
 * unmeasured.  tests/enhance_cases.py pins it as a float64 reference.
 *
 * Input x[0..L), output z[0..L).  N = 512, hop 128, bins k = 0..256, window w[n] = sin(pi (n + 0.5) / N) for analysis and
 * synthesis (its shifted squares sum to exactly 2).  L < N: out = x, bit for bit; only stage 8 may still apply.
 *   1. Frames: T = ceil(L / 128) + 3; frame t reads samples s = t 128 - 384 + n, n = 0..511; indices outside [0, L) are reflected
 *      without repeating the edge (s < 0 -> -s, s >= L -> 2 (L - 1) - s).  Every real sample lies in exactly four frames.
 *   2. Spectrum: X[t,k] = sum_n w[n] x_t[n] e^{-2 pi i k n / N}, P = |X|^2.
 *   3. Two box means of P along t, clipped to [0, T - 1] and divided by the number of frames summed: S (radius 2) drives the
 *      gain, Q (radius 16) the noise tracker.
 *   4. Noise floor: M[b,k] = min of Q over the 32 frames of block b, NB = ceil(T / 32);
 *      Nf[t,k] = oversubtract * min(M[b',k], b' in [max(0, b - 6), min(NB - 1, b + 6)]), b = floor(t / 32).
 *   5. Gain (TTASR_DSP_DENOISE): G = max(1 - Nf / S, 0) where S > 0, else 0; then G = max(G, 10^(-strength_db / 20)).  Without
 *      the flag G = 1.
 *   6. High-pass (TTASR_DSP_HIGHPASS): G[t,0] = G[t,1] = 0 (DC and the 31.25 Hz bin).
 *   7. Synthesis: y_t[n] = w[n] Re IDFT(G X)[n] (Hermitian extension, factor 1 / N); out[s] = 0.5 * the sum over the four frames
 *      that hold s, ascending t.
 *   8. Level (TTASR_DSP_LEVEL): p = max |out|, g = 1 if p == 0 else min(peak_target / p, max_gain), z = g out.
 * Every stage is continuous in x (max, min and clamps only; S = 0 has X = 0).
 *
 * ttasr_enhance_frames(n_samples) = T for n_samples >= 512, 0 for shorter recordings (no frame exists), TTASR_E_INVALID for a
 *   negative length.  No context.
 * ttasr_enhance: n recordings, recording i = pcm_host[i][0 .. n_samples[i]) -> out_pcm_host[i][0 .. n_samples[i]) (may be the
 *   input row itself); out_gain, when not NULL, receives the n level gains g (1 without TTASR_DSP_LEVEL).  n is not limited by
 *   max_batch, no model weights are needed, a recording of 0 samples is legal (its rows may be NULL, its gain is 1).
 *   Refused with TTASR_E_INVALID and a message before anything is enqueued, the context stays usable: n < 0; a NULL array;
 *   flags 0 or with unknown bits; a parameter that is not finite; strength_db outside [0, 40]; oversubtract outside (0, 16];
 *   peak_target outside (0, 1]; max_gain < 1; a length that is negative or above 2^36; a NULL row with samples; an open session; a
 *   call already in flight on the context.
 *   CONTRACT: a recording's result is a function of its samples and the parameters alone, bit for bit - not of the other
 *   recordings, their order, option "enhance_chunk" or the run.  No atomics; an output's operands and their order depend on its
 *   index alone.
 *   Device memory: ONE block owned by the context - the tables, the longest recording's samples and result (8 B per sample), its
 *   block minima [NB][257] and the partial maxima - allocated by the first call, grown on demand, freed by ttasr_destroy.  A block
 *   that cannot be allocated: TTASR_E_NOMEM, the context stays usable.  Recordings go through the stream one after the other,
 *   each cut into chunks of option "enhance_chunk" samples: per chunk one upload and the noise pass over the blocks whose samples
 *   have arrived, then per chunk the gain and synthesis pass and the partial maxima, then the gain, then per chunk the scaling and
 *   the download.  The call touches no mel, encoder, search, graph, session or network state.
 * ttasr_enhance_probe: the known-answer hook.  ONE recording through the launchers ttasr_enhance calls, every output optional
 *   (NULL = not wanted): out_S, out_Nf, out_G float32 [T][257] (S and Nf are computed whatever the flags say; G is what the
 *   flags make of it) and out_pcm [n_samples] BEFORE the level stage.  n_samples < 512: no frame exists, only out_pcm is
 *   written.  The refusals of ttasr_enhance. */
#define TTASR_DSP_DENOISE 1
#define TTASR_DSP_HIGHPASS 2
#define TTASR_DSP_LEVEL 4
typedef struct ttasr_dsp_params {
  float strength_db;    /* [0, 40]: the gain never falls below 10^(-strength_db / 20); default 12 */
  float oversubtract;   /* (0, 16]; default 3 */
  float peak_target;    /* (0, 1]; default 10^(-1 / 20) */
  float max_gain;       /* >= 1; default 10 */
  int32_t flags;        /* TTASR_DSP_*, at least one */
} ttasr_dsp_params;
TTASR_API int64_t ttasr_enhance_frames(int64_t n_samples);
TTASR_API int ttasr_enhance(ttasr_ctx* ctx, int32_t n, const float* const* pcm_host, const int64_t* n_samples,
                            const ttasr_dsp_params* params, float* const* out_pcm_host, float* out_gain);
TTASR_API int ttasr_enhance_probe(ttasr_ctx* ctx, const float* pcm_host, int64_t n_samples, const ttasr_dsp_params* params,
                                  float* out_S, float* out_Nf, float* out_G, float* out_pcm);

/* ---- kernel-selection overrides (tests, A/B measurements) ----------------------------------------- */
/* The release library reads NO environment variable; every deviation from the measured configuration is an explicit call.
 * Keys (value 0 / 1 unless stated; defaults in brackets): "flash" [1] MFMA flash attention in the encoder (0: the
 * one-query-per-wave f32 kernel); "prefill" [1] batched prompt prefill (0: prompts token by token); "vocab_persistent" [1] persistent vocabulary GEMM; "xsplit" [1] frame-split
 * cross-attention for small batches; "graph" [1] hipGraph replay of the decode step; "multi_step_graph" [1] runs of 8 / 4 greedy
 * steps between two host polls replay as one graph; "generic_kernels" [0] the 64x64 generic
 * GEMM / per-row kernels everywhere; "prefill_tiled" [0]; "prefill_ns_min" [2] (tokens); "enc_residual_epilogue" [0];
 * "enc_gemm" [0] = 1 | 2 | 3 | 4 forces one encoder GEMM kernel; "enc_gemm_persistent" [1] persistent 256x256 GEMM workgroups (bit-identical to the one-tile-per-workgroup form); "dec_narrow_blocks" [1] 20-row n-blocks in the packed decode matrix whose 20-row block count is a multiple of the 256 CUs (large-v3 family: fc1 = 256 workgroups instead of 160; a weight LAYOUT choice: set it before the first ttasr_load_tensor, later changes are refused); "enc_ln_defer" [1] one f32 read-modify-write of the encoder's residual stream per layer instead of two (bit-identical); "enc_gemm_tail" [1] the persistent GEMM's last partial round of workgroups re-tiled with 192- / 128-row tiles where the plan beats the plain tiling (bit-identical); "xkv_grouped" [1] the cross-KV projections of all decoder layers as ONE grouped launch of that kernel (bit-identical to one launch per layer); "ksplit_out" / "ksplit_q" / "ksplit_qkv" / "ksplit_fc2" [0 =
 * automatic] K slices of the decode GEMMs; "xattn_nontemporal" [1], "xattn_pipeline" [1] (software-pipelined cross-attention), "weights_nontemporal" [1], "dec_x_lds" [1] (the decode GEMMs stage their activation tile through LDS with coalesced loads; 0 = fragment loads straight from memory, bit-identical), "dec_red_swizzle" [1] (XOR-swizzled 16-byte chunk slots in the decode GEMMs' cross-wave LDS reduction buffer: conflict-free stores; 0 = linear rows, bit-identical) (all per context
 * since round 4); "ragged_exit" [1] finished rows of a decode batch leave its attention kernels (0: static batch, every row
 * streams its cross-KV until the last one ends; live rows are bit-identical either way); "xattn_deep_items" [512] live (row, head)
 * items at or below which the decode step's cross-attention workgroups keep 8 instead of 3 rows per lane in flight (0: never;
 * bit-identical); "xattn_mq_slices" [0 = automatic] frame slices of the shared-clip cross-attention (beam rows, prompt positions;
 * 1 ... 8, A/B); "flash_qw" [2] query blocks of 32 per wave in the encoder's MFMA flash attention (1: the round-5 form with 32
 * queries per wave; bit-identical);
 * "enc_kernel_timing" [0] per-launch events in ttasr_encode (see ttasr_encoder_kernel_ms); "xkv_fp8" [0] (16-bit engines; opt-in serving
 * mode, NOT the measured configuration) keeps an OCP e4m3 copy of the cross-KV cache with one scale per (layer, K | V, clip, head),
 * built by the next ttasr_encode and read by the decode step's cross-attention (half the bytes of the dominant kernel).  Values:
 * 0 off; 1 the copy is read by a static greedy batch of unshared rows with rows x heads >= 256 only - beam and sampled rows read
 * the 16-bit cache and sessions are refused; 2 the copy is read wherever a kernel for it exists: those greedy rows, the rows that
 * share a clip (ttasr_generate_beam, ttasr_generate_sample: 2..7 rows per clip and rows x heads >= 256), and continuous-batching
 * sessions of either kind, which quantise a clip when it is admitted.  Prefill, alignment and the frame-split kernels of small
 * batches read the 16-bit cache in every mode.  Other values: TTASR_E_INVALID; the f32 engine refuses 1 and 2;
 * "xattn_mq_fp8" [1] under "xkv_fp8" = 2, rows that share a clip read the e4m3 copy (0: the 16-bit cache; A/B);
 * "refill_overlap" [0] the continuous-batching session encodes the next clips on a second stream of the context while the
 * decode steps run (0: synchronously between two step runs on the context's one stream; results identical; read by
 * ttasr_session_begin).  Opt-in: the second stream is a second hardware queue, and several processes sharing a GPU are then
 * time-sliced;
 * "session_prefill" [0] (0 ... n_text_ctx - 2; read by ttasr_session_begin / ttasr_session_begin_beam) N > 0: a clip with at least
 * N prefillable prompt positions gets them from an admission pass instead of N forced decode steps (see "prompt prefill at
 * admission" above);
 * "align_packed" [0] (read by ttasr_session_align at call time) 1: the alignment pass over held clips runs packed and
 * pass-mate-independent (see ttasr_session_align); 0: the padded pass, unchanged;
 * "ingest_chunk" [0] (0 ... 2^30) input frames per chunk of ttasr_ingest_pcm / ttasr_ingest_wave (IMA: rounded up to whole blocks),
 * 0 = as many as the staging slots hold (results do not depend on it, bit for bit: tests put chunk boundaries inside small inputs
 * with it); "wire_chunk" [0] (0 ... 2^30) input frames of a row per chunk of ttasr_vad_stream_push_wire, 0 = as many as the row's
 * share of the pools holds (results do not depend on it either); "ingest_timing" [0] 1: ttasr_ingest_pcm
 * waits for every copy and kernel before it enqueues the next and leaves the host-clock split of the call in ttasr_phase_ms
 * (measurement only: the waits cost the overlap);
 * "seg_lstm_rows" [0] chunks per recurrence workgroup of ttasr_seg_scores: 0 = the measured choice, 1 | 2 | 4 force that form
 * (bit-identical: a gate row's summation order does not depend on it; A/B);
 * "enhance_chunk" [0] (0 ... 2^30) samples per chunk of ttasr_enhance / ttasr_enhance_probe, 0 = 2^22 (results do not depend on
 * it, bit for bit: tests put chunk boundaries inside frames, blocks and the floor's 13-block window with it);
 * Drops the captured decode graphs (except "enc_kernel_timing", "refill_overlap", "session_prefill", "align_packed", "ingest_chunk", "wire_chunk", "ingest_timing", "seg_lstm_rows" and "enhance_chunk").  Unknown key or value out of range: TTASR_E_INVALID. */
TTASR_API int ttasr_set_option(ttasr_ctx* ctx, const char* key, int32_t value);

/* ---- measurement --------------------------------------------------------------------------------- */
/* hipEvent times (ms) of the last log_mel / encode (stem+layers, cross-KV) / generate calls:
 * out[0]=mel out[1]=encoder out[2]=cross_kv out[3]=decode.  After a ttasr_ingest_pcm under option "ingest_timing" = 1 the four
 * values are that call's host-clock split instead: out[0]=staging copies on the host (into the pinned slots and out of them)
 * out[1]=uploads out[2]=kernels out[3]=downloads. */
TTASR_API int ttasr_phase_ms(ttasr_ctx* ctx, float out_ms[4]);
/* Host-side split of the LAST beam search on this context (ms): out[0] enqueueing (copies, launches), out[1] waiting for the GPU
 * (the one stream synchronisation per searching position), out[2] candidate selection + page bookkeeping on the host, out[3] =
 * number of positions stepped (a count, not ms).  The search is position-synchronous with the candidate rule on the host
 * (C++ inside the library); this is what that costs. */
TTASR_API int ttasr_beam_profile(ttasr_ctx* ctx, float out_ms[4]);
/* Where the encoder phase went, IN SITU: with option "enc_kernel_timing" = 1 the next ttasr_encode records one hipEvent after
 * every launch of its schedule (not an isolated relaunch loop: each kernel runs between its real neighbours) and this call
 * returns the per-class sums of that pass in ms: out[0] conv stem, [1] LayerNorms, [2] qkv GEMMs, [3] attention, [4] out-proj
 * GEMMs, [5] fc1 GEMMs, [6] fc2 GEMMs, [7] cross-KV GEMMs.  The extra events cost a few microseconds per launch; keep the
 * option off in timed runs. */
TTASR_API int ttasr_encoder_kernel_ms(ttasr_ctx* ctx, float out_ms[8]);
/* Re-launches one named hot kernel `iters` times on the context's stream with the state left by the
 * last encode/generate (B clips) and returns its average duration measured with hipEvents, plus the
 * algorithmic bytes and flops one launch moves/does.  Names: "xattn" (decoder cross-attention),
 * "enc_gemm_qkv", "enc_gemm_out", "enc_gemm_fc1", "enc_gemm_fc2", "enc_attn", "dec_gemm_fc1", "logits_gemm". */
TTASR_API int ttasr_bench_kernel(ttasr_ctx* ctx, const char* name, int32_t B, int32_t iters, float* out_avg_ms,
                       double* out_bytes_per_launch, double* out_flops_per_launch);
/* Signature of the kernel the LAST ttasr_bench_kernel call on this context launched, in the spelling rocprofv3 prints it
 * ("kernel_name<template arguments> grid <threads>"; "" when that kernel's launcher records none: names "xattn" and "enc_gemm_*"
 * do).  bench.py compares it with the signature stored in the committed counter profiles (profiles/xattn_pmc.json, *_pmc.json)
 * and reports their numbers only when they describe the kernel this build launches. */
TTASR_API int ttasr_bench_kernel_signature(ttasr_ctx* ctx, char* buf, int32_t len);
/* Device-wide synchronisation of the context's stream. */
TTASR_API int ttasr_sync(ttasr_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* TTASR_H_ */
