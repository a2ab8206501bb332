"""ctypes binding of libttasr.so (include/ttasr.h).  Loads the in-tree build only; there is no fallback:
a missing library or a missing GPU raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libttasr.so")

# every symbol include/ttasr.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    "ttasr_create", "ttasr_create_shared", "ttasr_destroy", "ttasr_last_error", "ttasr_version", "ttasr_load_tensor", "ttasr_load_tensor_device",
    "ttasr_finalize_weights", "ttasr_log_mel", "ttasr_log_mel_windows", "ttasr_log_mel_windows_cut", "ttasr_set_mel", "ttasr_encode", "ttasr_set_encoder_output",
    "ttasr_get_cross_kv", "ttasr_get_cross_kv_fp8", "ttasr_cross_attn_probe", "ttasr_align_attn_probe",
    "ttasr_self_kv_fill", "ttasr_self_kv_set", "ttasr_self_kv_get", "ttasr_self_attn_probe", "ttasr_enc_attn_probe", "ttasr_set_audio_ctx", "ttasr_generate", "ttasr_generate_capped", "ttasr_generate_beam", "ttasr_generate_beam_ragged", "ttasr_generate_sample", "ttasr_decode_reset", "ttasr_decode_step", "ttasr_apply_rules", "ttasr_select_probe", "ttasr_set_sequence_bias", "ttasr_seq_bias_probe", "ttasr_align", "ttasr_dtw",
    "ttasr_set_option", "ttasr_phase_ms", "ttasr_beam_profile", "ttasr_encoder_kernel_ms", "ttasr_bench_kernel", "ttasr_bench_kernel_signature", "ttasr_sync",
    "ttasr_session_begin", "ttasr_session_begin_beam", "ttasr_session_submit", "ttasr_session_submit_windows", "ttasr_session_poll", "ttasr_session_stats", "ttasr_session_rows", "ttasr_session_end",
    "ttasr_align_batch", "ttasr_session_hold", "ttasr_session_align", "ttasr_session_release", "ttasr_detect_language",
    "ttasr_session_detect_language", "ttasr_session_poll_lang", "ttasr_session_prefill_stats", "ttasr_session_retry",
    "ttasr_vad_load_tensor", "ttasr_vad_finalize", "ttasr_vad_probs",
    "ttasr_vad_stream_open", "ttasr_vad_stream_reset", "ttasr_vad_stream_close", "ttasr_vad_stream_push",
    "ttasr_ingest_len", "ttasr_ingest_filter", "ttasr_ingest_pcm", "ttasr_ingest_wave",
    "ttasr_ingest_stream_len", "ttasr_vad_stream_open_wire", "ttasr_vad_stream_push_wire",
    "ttasr_flac_probe", "ttasr_flac_frames", "ttasr_flac_decode",
    "ttasr_seg_load_tensor", "ttasr_seg_finalize", "ttasr_seg_classes", "ttasr_seg_chunks", "ttasr_seg_frames", "ttasr_seg_scores",
    "ttasr_spk_load_tensor", "ttasr_spk_finalize", "ttasr_spk_dim", "ttasr_spk_embed",
    "ttasr_enhance_frames", "ttasr_enhance", "ttasr_enhance_probe",
]

PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = range(6)   # TTASR_PCM_* of include/ttasr.h
PCM_BYTES = (1, 2, 3, 4, 4, 8)                                    # bytes per sample, by format code
PCM_ALAW, PCM_ULAW, PCM_IMA4 = 16, 17, 18                         # the coded formats of ttasr_ingest_wave
PCM_FLAC = 32                                                     # a whole FLAC file as read (ttasr_ingest_wave, ttasr_flac_*)
CODED_BYTES = {PCM_ALAW: 1, PCM_ULAW: 1}                          # bytes per sample of the G.711 codes (IMA: 4 bits, in blocks)
VAD_MAX_STREAMS = 1024    # TTASR_VAD_MAX_STREAMS of include/ttasr.h: open streams of one context (ttasr_vad_stream_*)
SEG_GROUP = 64            # TTASR_SEG_GROUP of include/ttasr.h: chunks of one pass of ttasr_seg_scores through its kernels
SEG_CHUNK_FRAMES = 293    # TTASR_SEG_CHUNK_FRAMES: frames of one 80 000-sample chunk of the segmentation network
SPK_GROUP = 16            # TTASR_SPK_GROUP of include/ttasr.h: chunks of one pass of ttasr_spk_embed through its kernels
SPK_MAX_MASKS, SPK_MAX_DIM, SPK_STATS = 8, 512, 3000   # TTASR_SPK_MAX_MASKS, TTASR_SPK_MAX_DIM, TTASR_SPK_STATS
VAD_CHUNK_FRAMES = 1024   # TTASR_VAD_CHUNK_FRAMES of include/ttasr.h: frames of one recording per time chunk of ttasr_vad_probs


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_mels", "n_audio_ctx", "d_model", "n_heads", "ffn_dim", "enc_layers", "dec_layers", "vocab",
        "n_text_ctx", "compute_type", "max_batch", "reserved")]


class GenOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "max_new_tokens", "eot", "no_timestamps", "timestamp_begin", "no_speech", "sot_index", "timestamps",
        "max_initial_timestamp_index", "suppress_eot", "n_suppress", "n_begin_suppress", "check_interval")] + [
        ("suppress", C.POINTER(C.c_int32)), ("begin_suppress", C.POINTER(C.c_int32))]


SELECT_FORMS = {"step": 0, "rows": 1, "session": 2, "topk": 3, "logprob": 4, "prob": 5}   # TTASR_SELECT_* of include/ttasr.h


class SelectIO(C.Structure):
    """ttasr_select_io: 13 input pointers, 13 output pointers, 8 int32 scalars, temperature, seed."""
    _fields_ = [(n, C.c_void_p) for n in (
        "rows_host", "opts", "hist_host", "positions_host", "prompt_host", "prompt_len_host", "done_host", "row_cap_host",
        "sum_logprob_host", "entries_host", "entry_temp_host", "entry_seed_host", "targets_host",
        "out_cur_tok", "out_n_sampled", "out_last_tok", "out_pen_tok", "out_last_ts", "out_done", "out_positions", "out_n_done",
        "out_sum_logprob", "out_no_speech", "out_tokens", "out_f32", "out_i32")] + [(n, C.c_int32) for n in (
        "n", "hist_stride", "max_prompt", "n_done", "n_entries", "k", "want_no_speech", "token")] + [
        ("temperature", C.c_float), ("seed", C.c_uint32)]


SEQ_BIAS_FORMS = {"window": 0, "state": 1}   # TTASR_SEQ_BIAS_* of include/ttasr.h


class DspParamsC(C.Structure):
    """ttasr_dsp_params: strength_db, oversubtract, peak_target, max_gain, flags (TTASR_DSP_DENOISE 1 | HIGHPASS 2 | LEVEL 4)."""
    _fields_ = [(n, C.c_float) for n in ("strength_db", "oversubtract", "peak_target", "max_gain")] + [("flags", C.c_int32)]


class SeqBiasIO(C.Structure):
    """ttasr_seq_bias_io: 8 input pointers, the output rows, 4 int32 scalars."""
    _fields_ = [(n, C.c_void_p) for n in (
        "rows_host", "hist_host", "hist_len_host", "prompt_host", "prompt_len_host", "out_tokens_host", "n_sampled_host", "done_host",
        "out_rows_host")] + [(n, C.c_int32) for n in ("n", "max_prompt", "max_new", "position")]


def build(verbose: bool = False) -> str:
    """Compile libttasr.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc"), "-j", str(min(8, os.cpu_count() or 1))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("libttasr build failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is the only implementation; there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32p = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    lib.ttasr_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(vp)]
    lib.ttasr_create_shared.argtypes = [vp, i32, C.POINTER(vp)]
    lib.ttasr_destroy.argtypes = [vp]
    lib.ttasr_destroy.restype = None
    lib.ttasr_last_error.argtypes = [vp]
    lib.ttasr_last_error.restype = C.c_char_p
    lib.ttasr_version.argtypes = []
    lib.ttasr_version.restype = C.c_char_p
    lib.ttasr_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    lib.ttasr_load_tensor_device.argtypes = [vp, C.c_char_p, vp, i32, i64p, i32]
    lib.ttasr_finalize_weights.argtypes = [vp]
    lib.ttasr_log_mel.argtypes = [vp, vp, i64, i64p, i32, i32, vp]
    lib.ttasr_log_mel_windows.argtypes = [vp, C.POINTER(vp), i64p, i64p, i32, vp, vp, vp]
    lib.ttasr_log_mel_windows_cut.argtypes = [vp, C.POINTER(vp), i64p, i64p, i32, vp, vp, vp, i64p]
    lib.ttasr_set_mel.argtypes = [vp, vp, i32]
    lib.ttasr_encode.argtypes = [vp, i32, vp]
    lib.ttasr_set_encoder_output.argtypes = [vp, vp, i32]
    lib.ttasr_get_cross_kv.argtypes = [vp, i32, i32, i32, vp]
    lib.ttasr_get_cross_kv_fp8.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.ttasr_cross_attn_probe.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, C.c_char_p, i32]
    lib.ttasr_align_attn_probe.argtypes = [vp, i32, i32, i32p, i32p, vp, i32p, i32, vp, vp]
    lib.ttasr_self_kv_fill.argtypes = [vp, i32, C.c_uint32]
    lib.ttasr_self_kv_set.argtypes = [vp, i32, vp, i32, i32, vp]
    lib.ttasr_self_kv_get.argtypes = [vp, i32, vp, i32, vp]
    lib.ttasr_self_attn_probe.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, C.c_char_p, i32]
    lib.ttasr_enc_attn_probe.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, C.c_char_p, i32]
    lib.ttasr_set_audio_ctx.argtypes = [vp, i32]
    lib.ttasr_generate.argtypes = [vp, i32, i32p, i32p, i32, C.POINTER(GenOpts), i32p, i32p, f32p, f32p]
    lib.ttasr_generate_capped.argtypes = [vp, i32, i32p, i32p, i32, C.POINTER(GenOpts), i32p, i32p, i32p, f32p, f32p]
    lib.ttasr_generate_beam.argtypes = [vp, i32, i32, i32p, i32, C.POINTER(GenOpts), C.c_float, i32p, i32p, f32p, f32p]
    lib.ttasr_generate_beam_ragged.argtypes = [vp, i32, i32, i32p, i32p, i32p, i32, C.POINTER(GenOpts), C.c_float, i32p, i32p, f32p, f32p]
    lib.ttasr_generate_sample.argtypes = [vp, i32, i32, i32p, i32, C.POINTER(GenOpts), C.c_float, C.c_uint32, i32p, i32p, f32p, f32p]
    lib.ttasr_decode_reset.argtypes = [vp, i32]
    lib.ttasr_decode_step.argtypes = [vp, i32p, i32, vp]
    lib.ttasr_apply_rules.argtypes = [vp, vp, i32p, i32, i32, C.POINTER(GenOpts), vp, i32p]
    lib.ttasr_select_probe.argtypes = [vp, i32, C.POINTER(SelectIO), C.c_char_p, i32]
    lib.ttasr_set_sequence_bias.argtypes = [vp, i32, i32p, i32p, f32p]
    lib.ttasr_seq_bias_probe.argtypes = [vp, i32, C.POINTER(SeqBiasIO), C.c_char_p, i32]
    lib.ttasr_align.argtypes = [vp, i32, i32p, i32, i32p, i32, f32p, f32p]
    lib.ttasr_detect_language.argtypes = [vp, i32, i32, i32, i32, i32p, f32p, f32p]
    lib.ttasr_align_batch.argtypes = [vp, i32, i32p, i32p, i32p, i32, i32p, i32p, i32p, i32, i32, i32p, f32p, f32p, f32p]
    lib.ttasr_session_hold.argtypes = [vp, i32]
    lib.ttasr_session_align.argtypes = [vp, i32, i64p, i32p, i32p, i32, i32p, i32p, i32p, i32, i32, i32p, f32p, f32p, f32p]
    lib.ttasr_session_release.argtypes = [vp, i32, i64p]
    lib.ttasr_session_retry.argtypes = [vp, i32, i64p, i32p, i32p, i32p, i32p, f32p, i32p, C.POINTER(C.c_uint32), i64p]
    lib.ttasr_dtw.argtypes = [f32p, i32, i32, i32p, i32p, i32p]
    lib.ttasr_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.ttasr_phase_ms.argtypes = [vp, f32p]
    lib.ttasr_beam_profile.argtypes = [vp, f32p]
    lib.ttasr_encoder_kernel_ms.argtypes = [vp, f32p]
    lib.ttasr_bench_kernel.argtypes = [vp, C.c_char_p, i32, i32, f32p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ttasr_sync.argtypes = [vp]
    lib.ttasr_session_begin.argtypes = [vp, C.POINTER(GenOpts), i32, C.c_float]
    lib.ttasr_session_begin_beam.argtypes = [vp, C.POINTER(GenOpts), i32, i32, C.c_float]
    lib.ttasr_session_submit.argtypes = [vp, i32, C.POINTER(vp), i64p, i32p, i32p, i32p, i64p]
    lib.ttasr_session_submit_windows.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p, f32p, i32p, i32p, i32p, i32p, f32p, i32p,
                                                 C.POINTER(C.c_uint32), i64p]
    lib.ttasr_session_poll.argtypes = [vp, i32, i32, i64p, i32p, i32p, f32p, f32p, i32p]
    lib.ttasr_session_detect_language.argtypes = [vp, i32, i32, i32]
    lib.ttasr_session_poll_lang.argtypes = [vp, i32, i32, i64p, i32p, i32p, f32p, f32p, i32p, f32p, f32p, i32p]
    lib.ttasr_session_stats.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ttasr_session_prefill_stats.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ttasr_session_rows.argtypes = [vp, i32p, i32p, i64p]
    lib.ttasr_session_end.argtypes = [vp]
    lib.ttasr_vad_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    lib.ttasr_vad_finalize.argtypes = [vp]
    lib.ttasr_vad_probs.argtypes = [vp, i32, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp)]
    lib.ttasr_vad_stream_open.argtypes = [vp, i32p]
    lib.ttasr_vad_stream_reset.argtypes = [vp, i32]
    lib.ttasr_vad_stream_close.argtypes = [vp, i32]
    lib.ttasr_vad_stream_push.argtypes = [vp, i32, i32p, C.POINTER(vp), i64p, i32p, C.POINTER(vp), C.POINTER(vp), i32p]
    lib.ttasr_ingest_len.argtypes = [i32, i64]
    lib.ttasr_ingest_len.restype = i64
    lib.ttasr_ingest_filter.argtypes = [i32, f32p, i32]
    lib.ttasr_ingest_filter.restype = i32
    lib.ttasr_ingest_pcm.argtypes = [vp, i32, C.POINTER(vp), i64p, i32p, i32p, i32p, C.POINTER(vp)]
    lib.ttasr_ingest_wave.argtypes = [vp, i32, C.POINTER(vp), i64p, i64p, i32p, i32p, i32p, i32p, i32p, C.POINTER(vp)]
    lib.ttasr_ingest_stream_len.argtypes = [i32, i64, i32]
    lib.ttasr_ingest_stream_len.restype = i64
    lib.ttasr_vad_stream_open_wire.argtypes = [vp, i32, i32, i32, i32, i32p]
    lib.ttasr_vad_stream_push_wire.argtypes = [vp, i32, i32p, C.POINTER(vp), i64p, i32p, C.POINTER(vp), i64p, i64p, C.POINTER(vp),
                                               C.POINTER(vp), i32p]
    lib.ttasr_flac_probe.argtypes = [vp, i64, i64p, C.c_char_p, i32]
    lib.ttasr_flac_frames.argtypes = [vp, i64, i64p, i64, C.c_char_p, i32]
    lib.ttasr_flac_frames.restype = i64
    lib.ttasr_flac_decode.argtypes = [vp, i64, i32p, i64, C.c_char_p, i32]
    lib.ttasr_flac_decode.restype = i64
    lib.ttasr_seg_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    lib.ttasr_seg_finalize.argtypes = [vp]
    lib.ttasr_seg_classes.argtypes = [vp]
    lib.ttasr_seg_chunks.argtypes = [i64]
    lib.ttasr_seg_chunks.restype = i64
    lib.ttasr_seg_frames.argtypes = [i64]
    lib.ttasr_seg_frames.restype = i64
    lib.ttasr_seg_scores.argtypes = [vp, i32, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.ttasr_spk_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    lib.ttasr_spk_finalize.argtypes = [vp]
    lib.ttasr_spk_dim.argtypes = [vp]
    lib.ttasr_spk_embed.argtypes = [vp, i32, C.POINTER(vp), i64p, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.ttasr_enhance_frames.argtypes = [i64]
    lib.ttasr_enhance_frames.restype = i64
    lib.ttasr_enhance.argtypes = [vp, i32, C.POINTER(vp), i64p, C.POINTER(DspParamsC), C.POINTER(vp), f32p]
    lib.ttasr_enhance_probe.argtypes = [vp, vp, i64, C.POINTER(DspParamsC), vp, vp, vp, vp]
    for s in SYMBOLS:
        f = getattr(lib, s)
        if s not in ("ttasr_destroy", "ttasr_last_error", "ttasr_version", "ttasr_ingest_len", "ttasr_ingest_filter",
                     "ttasr_ingest_stream_len", "ttasr_flac_frames", "ttasr_flac_decode", "ttasr_seg_chunks", "ttasr_seg_frames",
                     "ttasr_enhance_frames"):
            f.restype = C.c_int
    _lib = lib
    return lib


class FlacInfo(tuple):
    """ttasr_flac_probe's eight numbers with names."""
    rate = property(lambda s: s[0]); channels = property(lambda s: s[1]); bits = property(lambda s: s[2])    # noqa: E702
    samples = property(lambda s: s[3]); frames = property(lambda s: s[4]); max_blocksize = property(lambda s: s[5])   # noqa: E702
    first_frame = property(lambda s: s[6]); has_md5 = property(lambda s: bool(s[7] & 1))    # noqa: E702
    total_disagrees = property(lambda s: bool(s[7] & 2))


def _flac_buffer(data):
    import numpy as np
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def flac_probe(data) -> FlacInfo:
    """A whole FLAC file as read -> FlacInfo (ttasr_flac_probe: no GPU).  ValueError with the library's reason for a stream it refuses."""
    b, out, why = _flac_buffer(data), (C.c_int64 * 8)(), C.create_string_buffer(256)
    if load().ttasr_flac_probe(b.ctypes.data, len(b), out, why, len(why)) != 0:
        raise ValueError("FLAC: " + why.value.decode("utf-8", "replace"))
    return FlacInfo(int(v) for v in out)


def flac_frames(data):
    """The frame table of the scan: int64 [frames][3] = byte offset, byte length, first sample (ttasr_flac_frames)."""
    import numpy as np
    b, why = _flac_buffer(data), C.create_string_buffer(256)
    n = load().ttasr_flac_frames(b.ctypes.data, len(b), None, 0, why, len(why))
    if n < 0:
        raise ValueError("FLAC: " + why.value.decode("utf-8", "replace"))
    table = np.zeros((max(n, 1), 3), dtype=np.int64)
    load().ttasr_flac_frames(b.ctypes.data, len(b), table.ctypes.data_as(C.POINTER(C.c_int64)), n, why, len(why))
    return table[:n]


def flac_decode(data):
    """A whole FLAC file as read -> (int32 [samples][channels] plain integers, FlacInfo), decoded by the library on the host
    (ttasr_flac_decode).  ValueError with the library's reason for a stream it refuses or a frame with illegal content."""
    import numpy as np
    info = flac_probe(data)
    b, why = _flac_buffer(data), C.create_string_buffer(256)
    out = np.zeros((info.samples, info.channels), dtype=np.int32)
    n = load().ttasr_flac_decode(b.ctypes.data, len(b), out.ctypes.data_as(C.POINTER(C.c_int32)), info.samples, why, len(why))
    if n < 0:
        raise ValueError("FLAC: " + why.value.decode("utf-8", "replace"))
    return out, info
