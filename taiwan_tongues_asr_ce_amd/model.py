"""`WhisperModel` - the drop-in for `faster_whisper.WhisperModel` on the reference's hot path.

Same constructor and `transcribe()` surface the three reference call sites use
(asr_core.py:141,159-167; api/file_asr.py:188,457-465; api/stt_streaming/src/asr/faster_whisper_asr.py:107-109,
170-172): `WhisperModel(path, device=..., compute_type=...)`, `.transcribe(audio, language=, word_timestamps=,
vad_filter=, beam_size=, condition_on_previous_text=, initial_prompt=) -> (iterable of Segment, TranscriptionInfo)`.
Host Python does checkpoint reading, tokenisation and the 30-s window loop; everything from PCM to token ids
is libttasr (HIP).  There is no CPU path: `device="cpu"` raises, as a failed CUDA load does in the reference
(faster_whisper_asr.py:116-134 then retries on CPU - that retry is out of scope here).
"""
from __future__ import annotations

import contextlib
import functools
import inspect
import json
import os
import threading
import warnings
import zlib
from dataclasses import dataclass, field
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import alignment, audio_io, ct2, dsp, seq_bias, synth, vad
from .audio_io import CodedAudio, decode_audio, parse_audio_channel, read_audio_coded, read_audio_raw  # noqa: F401  (public here too)
from .config import (COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, HOP, N_FRAMES, N_SAMPLES, PRESETS, SAMPLE_RATE, SpecialTokens,
                     WhisperDims)
from .tokenizer import load_tokenizer


class Word(NamedTuple):
    start: float
    end: float
    word: str
    probability: float


class Segment(NamedTuple):
    id: int
    seek: int
    start: float
    end: float
    text: str
    tokens: List[int]
    temperature: float
    avg_logprob: float
    compression_ratio: float
    no_speech_prob: float
    words: Optional[List[Word]]


@dataclass
class TranscriptionInfo:
    language: str
    language_probability: float
    duration: float
    duration_after_vad: float
    all_language_probs: Optional[List[Tuple[str, float]]] = None
    transcription_options: Dict = field(default_factory=dict)
    vad_options: Optional[Dict] = None
    # transcribe_many(continuous=True, multilingual=True): the language found for every window that was decoded, in file order
    window_languages: Optional[List[str]] = None
    # BatchedInferencePipeline: one entry per group - start / end (samples of the recording), its speech pieces and its attempts
    # as (temperature, avg_logprob, no_speech_prob, compression_ratio); and Session.stats() of the run plus "retries"
    chunks: Optional[List[Dict]] = None
    session: Optional[Dict[str, float]] = None


_COMPUTE_ALIASES = {
    "float32": COMPUTE_F32, "fp32": COMPUTE_F32,
    # "float16" is the reference's GPU setting (asr_core.py:141, api/config.py:12, faster_whisper_asr.py:95) and means what it
    # says: fp16 weights / activations, f32 accumulation.  The int8 variants have no int8 weight path here: they run with
    # 16-bit weights of the named activation type (a superset in precision), with a warning.
    "bfloat16": COMPUTE_BF16, "bf16": COMPUTE_BF16, "float16": COMPUTE_F16, "fp16": COMPUTE_F16,
    "int8_float16": COMPUTE_F16, "int8_bfloat16": COMPUTE_BF16, "int8": COMPUTE_F16,
    # "default" / "auto" (CTranslate2: the type the model was converted with / the fastest supported one - float16 for the
    # reference's GPU deployments, asr_core.py:141) map to fp16 since round 4: on the headline workload the fp16 engine reproduces
    # the f32 parity engine's 32 x 128 greedy tokens exactly, the bf16 engine on 21 of 32 rows (its near-ties resolve differently:
    # bench.py output_check.vs_f32_parity_tokens), at 1 % lower throughput (2 023 vs 2 043 audio-s/s).  "bfloat16" stays one
    # keyword away and is BASELINE.json's measured configuration.
    "default": COMPUTE_F16, "auto": COMPUTE_F16,
}

# multilingual Whisper language order (tokens sot+1 ...); only the codes the reference can request matter
LANGUAGES = ("en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la "
             "mi ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be "
             "tg sd gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha ba jw su yue").split()


def select_language(tops: Sequence[Tuple[str, float]], threshold: Optional[float] = 0.5) -> Tuple[str, float, int]:
    """faster-whisper's language_detection_segments / language_detection_threshold rule over the top (language, probability) of
    the windows that were examined, in file order -> (language, probability, index of the window the answer is taken from).
    The first window whose top probability exceeds the threshold decides; when none does, the language that won the most
    windows (a tie goes to the one seen first), with the largest probability it reached, taken from that window."""
    if not tops:
        raise ValueError("select_language needs at least one window")
    votes: Dict[str, List[Tuple[float, int]]] = {}
    for i, (lang, prob) in enumerate(tops):
        if threshold is None or prob > threshold:
            return lang, float(prob), i
        votes.setdefault(lang, []).append((float(prob), i))
    lang = max(votes, key=lambda k: len(votes[k]))      # dicts keep insertion order: the first of equally frequent languages
    prob, i = max(votes[lang], key=lambda e: e[0])      # the first of equal probabilities
    return lang, prob, i


def parse_clip_timestamps(clip_timestamps, n_total: int) -> List[Tuple[int, int]]:
    """`clip_timestamps` of transcribe() -> the (start, end) pairs of 10-ms frames the window loop walks, as openai-whisper's
    transcribe() builds its seek_clips (restated from memory: unpinned): a comma-separated string of seconds ("0", the default; ""
    counts as "0") or a sequence of seconds; a seek point is round(t * 100); an odd count means the last clip runs to the end of the
    recording.  Here every point is clamped to the recording's n_total frames - a clip that starts past the end is empty - and a
    negative, non-finite or non-numeric value raises ValueError."""
    if isinstance(clip_timestamps, str):
        parts = [t.strip() for t in clip_timestamps.split(",")] if clip_timestamps.strip() else []
    elif isinstance(clip_timestamps, (list, tuple, np.ndarray)):
        parts = list(clip_timestamps)
    else:
        raise ValueError(f"clip_timestamps={clip_timestamps!r}: a comma-separated string of seconds or a list of seconds")
    points = []
    for t in parts:
        try:
            v = float(t)
        except (TypeError, ValueError):
            raise ValueError(f"clip_timestamps: {t!r} is not a number of seconds") from None
        if not np.isfinite(v) or v < 0:
            raise ValueError(f"clip_timestamps: {t!r} is not a finite, non-negative number of seconds")
        points.append(min(int(round(v * 100)), int(n_total)))
    if not points:
        points.append(0)
    if len(points) % 2:
        points.append(int(n_total))
    return list(zip(points[::2], points[1::2]))


def _clip_lists(clip_timestamps, n: int) -> list:
    """`clip_timestamps` of a many-file surface -> one entry per file: a string or a flat sequence of seconds holds for every file,
    a sequence of strings / sequences is one entry per file."""
    if not isinstance(clip_timestamps, str) and isinstance(clip_timestamps, (list, tuple)) and \
            any(isinstance(c, (str, list, tuple, np.ndarray)) for c in clip_timestamps):
        if len(clip_timestamps) != n:
            raise ValueError(f"clip_timestamps needs one entry per file ({n}), got {len(clip_timestamps)}")
        return list(clip_timestamps)
    return [clip_timestamps] * n


def _frames_of(n_samples: int) -> int:
    """Frames of the whole-file STFT: len // HOP (the feature extractor drops its last frame); a tail shorter than one hop still
    yields one (all-padding) window, as faster-whisper's 160 samples of end padding do."""
    return max(n_samples // HOP, 1) if n_samples else 0


LOCK_STEP_ONLY = ("{what}: clip_timestamps and hallucination_silence_threshold are not available in a continuous-batching session "
                  "(ttasr_session_submit_windows has no cut, and a session aligns a window after its file has moved on); use the "
                  "lock-step form, transcribe_many(..., continuous=False)")


def refuse_in_session(what: str, clip_timestamps="0", hallucination_silence_threshold=None) -> None:
    """The ValueError of every continuous surface for a non-neutral clip_timestamps / hallucination_silence_threshold; raised
    before any session opens.  The neutral clip values are those that parse to the whole recording whatever its length: "0", "",
    [0], [], None.  [0, duration] is refused here although the lock-step loop treats it as the default: a recording's length
    is not known where these surfaces check their arguments."""
    neutral_clip = clip_timestamps is None or (isinstance(clip_timestamps, str) and clip_timestamps.strip() in ("", "0")) or \
        (isinstance(clip_timestamps, (list, tuple)) and all(isinstance(c, (int, float)) for c in clip_timestamps)
         and [float(c) for c in clip_timestamps] in ([], [0.0]))
    if not neutral_clip or hallucination_silence_threshold is not None:
        raise ValueError(LOCK_STEP_ONLY.format(what=what))


def skip_hallucinations(kept: List[dict], single_timestamp_ending: bool, seek: int, win_frames: int, next_seek: int,
                        threshold: float, last_speech_end: float, n_total: int, n_window: int = N_FRAMES
                        ) -> Tuple[List[dict], int, bool]:
    """hallucination_silence_threshold for one window whose words are dealt to its kept segments (dicts with start, end, words),
    as openai-whisper's transcribe() applies it (restated from memory: unpinned).  seek / win_frames: the window's first frame
    and frame count; next_seek: where the segment rule would go on; last_speech_end: the last word end of the windows before;
    n_total: frames of the recording; n_window: frames of a full window - the rules measure the silence left in the window to
    seek + n_window, also when the window itself is shorter.  -> (segments to yield, next seek, True when the window yields
    nothing and leaves the previous text and the prompt reset alone).
    1. The window does not end in a single timestamp and its last word ends after the window's start: go on at that word's end
       when more than `threshold` of the window follows it, else behind the window.
    2. The first segment with words is anomalous (alignment.is_segment_anomaly) and starts more than `threshold` into the
       window: yield nothing and go on where it starts.
    3. The first anomalous segment with silence on both sides - before: more than `threshold` since the last kept segment's
       end, a start below `threshold`, or less than 2 s into the window; after: more than `threshold` to the next segment with
       words (the window's end without one), that segment anomalous too, or less than 2 s of the window left - is dropped with
       everything after it; go on at max(1 s into the window, its start), or at the end of the recording when less than
       `threshold` of audio follows its end."""
    time_offset = seek * HOP / SAMPLE_RATE
    window_end = (seek + n_window) * HOP / SAMPLE_RATE
    with_words = [seg for seg in kept if seg.get("words")]
    if not single_timestamp_ending and with_words:
        last_word_end = with_words[-1]["words"][-1].end
        if last_word_end > time_offset:
            next_seek = int(round(last_word_end * 100)) if window_end - last_word_end > threshold else seek + win_frames
    if with_words and alignment.is_segment_anomaly(with_words[0]):
        gap = with_words[0]["start"] - time_offset
        if gap > threshold:
            return [], seek + max(int(round(gap * 100)), 1), True
    last_end = last_speech_end
    for i, seg in enumerate(kept):
        if not seg.get("words"):
            continue
        if alignment.is_segment_anomaly(seg):
            nxt = next((n for n in kept[i + 1:] if n.get("words")), None)
            next_start = nxt["words"][0].start if nxt is not None else time_offset + win_frames * HOP / SAMPLE_RATE
            before = seg["start"] - last_end > threshold or seg["start"] < threshold or seg["start"] - time_offset < 2.0
            after = next_start - seg["end"] > threshold or alignment.is_segment_anomaly(nxt) or window_end - seg["end"] < 2.0
            if before and after:
                next_seek = int(round(max(time_offset + 1, seg["start"]) * 100))
                if n_total * HOP / SAMPLE_RATE - seg["end"] < threshold:
                    next_seek = n_total
                return kept[:i], next_seek, False
        last_end = seg["end"]
    return kept, next_seek, False


def _read_hf_dir(path: str) -> Tuple[WhisperDims, Iterable[Tuple[str, np.ndarray]]]:
    with open(os.path.join(path, "config.json"), "r", encoding="utf-8") as f:
        cfg = json.load(f)
    dims = WhisperDims(os.path.basename(os.path.normpath(path)), cfg["num_mel_bins"], cfg["max_source_positions"],
                       cfg["d_model"], cfg["encoder_attention_heads"], cfg["encoder_ffn_dim"], cfg["encoder_layers"],
                       cfg["decoder_layers"], cfg["vocab_size"], cfg.get("max_target_positions", 448))
    st_path = os.path.join(path, "model.safetensors")
    bin_path = os.path.join(path, "pytorch_model.bin")

    def tensors():
        if os.path.exists(st_path):
            from safetensors import safe_open
            with safe_open(st_path, framework="np") as f:
                for k in f.keys():
                    if k != "proj_out.weight":
                        yield k, np.asarray(f.get_tensor(k), dtype=np.float32)
        elif os.path.exists(bin_path):
            import torch
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
            for k, v in sd.items():
                if k != "proj_out.weight":
                    yield k, v.float().numpy()
        else:
            raise FileNotFoundError(f"{path}: no model.bin (CTranslate2), model.safetensors or pytorch_model.bin")
    return dims, tensors()


def _lock_step_bias(fn):
    """transcribe_many's keywords sequence_bias / prompt_words / prompt_word_boost: the table is resolved once (prompt_words is
    tokenised here), refused with continuous=True before any device work, installed on the calling thread's engine context for
    the call and cleared when it ends, on error paths too."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def call(self, *args, sequence_bias=None, prompt_words=None, prompt_word_boost=None, **kw):
        if sig.bind(self, *args, **kw).arguments.get("continuous"):
            seq_bias.refuse_in_session(f"{fn.__name__}(continuous=True)", sequence_bias, prompt_words)
        with self._sequence_bias(self._bias_table(sequence_bias, prompt_words, prompt_word_boost)):
            return fn(self, *args, **kw)
    return call


class WhisperModel:
    def __init__(self, model_size_or_path: str, device: str = "auto", device_index: int = 0,
                 compute_type: str = "default", max_batch: int = 8, pipeline_depth: int = 1, cross_kv_fp8: bool = False,
                 vad_model=None, _engine_factory=None, **_unused):
        """`vad_model` (MI355X extension): the Silero-v5 VAD network for vad_filter=True, run on the device - a path (`.npz`, or a
        TorchScript / state-dict file when torch imports) or a mapping of the tensors of vad.SILERO_V5_TENSORS (`load_vad`).
        Without it vad_filter=True behaves as before (operator callable, energy opt-in, or a warning).
        `cross_kv_fp8` (MI355X extension, opt-in serving mode, 16-bit compute types only): every engine context of the model
        reads the e4m3 copy of the decoder's cross-attention cache wherever a kernel for it exists (engine option xkv_fp8 = 2:
        greedy rows, the rows of a beam or a sampled attempt, continuous-batching sessions).  Outputs are no longer those of the
        16-bit cache.  The lock-step and the continuous form of transcribe_many agree bit for bit only under the session's
        contract (include/ttasr.h): prompts forced through decode steps (engine option prefill = 0) and G = max_batch / beam
        files per lock-step pass; with the default prefill the lock-step form reads the 16-bit cache for the prompt positions
        and the two forms may differ in the last bits.  Ignored by an engine without options (the oracle test seam).
        `pipeline_depth` (MI355X extension, default 1 = the reference's serial behaviour, asr_core.py:151): how many engine
        contexts `transcribe_groups` / the folder tool may keep in flight on this GPU.  The extra contexts SHARE the first one's
        device weights (ttasr_create_shared: workspaces only) and are created on first use; pass i + 1's log-mel / encoder then
        runs under pass i's latency-bound decode chain.  Results are identical, file by file, to pipeline_depth = 1.
        `_engine_factory` is a TEST seam only (tests/oracle_engine.py drives the host-side window loop with the CPU oracle
        to pin it against HF long-form goldens without a GPU); the product always builds the HIP Engine."""
        if device not in ("cuda", "auto", "gpu", "hip"):
            raise RuntimeError(f"device={device!r}: this build has only the MI355X HIP path (no CPU fallback)")
        if compute_type not in _COMPUTE_ALIASES:
            raise ValueError(f"unknown compute_type {compute_type!r}")
        if cross_kv_fp8 and _COMPUTE_ALIASES[compute_type] == COMPUTE_F32:
            raise ValueError("cross_kv_fp8=True needs a 16-bit compute_type (the float32 engine has no e4m3 cross-KV copy)")
        from .engine import Engine  # imports/loads libttasr; raises when the extension is missing
        self.model_size_or_path = model_size_or_path
        self.device = "cuda"
        self.compute_type = compute_type
        self.ct2_config: dict = {}
        self.vad_speech_prob_fn = None   # operator hook: audio f32[n] -> speech probability per 512-sample frame (e.g. Silero ONNX)
        if os.path.isdir(model_size_or_path) and ct2.is_ct2_dir(model_size_or_path):
            # the deployed format (CTranslate2 model.bin; faster_whisper_asr.py:38) -- reader is unpinned, see ct2.py
            dims, tensors, self.ct2_config = ct2.read_ct2_dir(model_size_or_path)
            self.tokenizer = load_tokenizer(model_size_or_path, dims.vocab)
        elif os.path.isdir(model_size_or_path):
            dims, tensors = _read_hf_dir(model_size_or_path)
            self.tokenizer = load_tokenizer(model_size_or_path, dims.vocab)
        elif model_size_or_path.startswith("synthetic:"):
            dims = PRESETS[model_size_or_path.split(":", 1)[1]]
            tensors = synth.iter_weights(dims)
            self.tokenizer = load_tokenizer(None, dims.vocab)
        else:
            raise FileNotFoundError(
                f"{model_size_or_path!r} is not a local HF Whisper directory (no network for hub ids); use a directory "
                "with model.bin (CTranslate2) or config.json + model.safetensors (HF), or 'synthetic:<preset>' for seeded "
                "random weights")
        self.dims = dims
        # word timestamps: curated (layer, head) pairs from the model directory when it has them (CTranslate2 config.json
        # / HF generation_config.json "alignment_heads"), else the capped last-half-of-the-decoder default
        heads = self.ct2_config.get("alignment_heads")
        if heads is None and os.path.isdir(model_size_or_path):
            gc_path = os.path.join(model_size_or_path, "generation_config.json")
            if os.path.exists(gc_path):
                with open(gc_path, "r", encoding="utf-8") as f:
                    heads = json.load(f).get("alignment_heads")
        self.alignment_heads = [tuple(h) for h in heads] if heads else alignment.default_alignment_heads(dims.dec_layers, dims.n_heads)
        if compute_type in ("int8_float16", "int8_bfloat16", "int8"):
            # the reference asks for int8 on CPU (api/file_asr.py:188); there is no int8 weight path on this engine - say so
            # instead of silently computing in another type
            warnings.warn(f"compute_type={compute_type!r}: int8 weights are not implemented by this engine; computing with "
                          f"{'bfloat16' if 'bfloat16' in compute_type else 'float16'} weights and activations "
                          "(f32 accumulation, LayerNorm and softmax)", stacklevel=2)
        if pipeline_depth < 1 or pipeline_depth > 4:
            raise ValueError(f"pipeline_depth={pipeline_depth}: 1 ... 4 contexts per GPU")
        self.pipeline_depth = int(pipeline_depth)
        self.cross_kv_fp8 = bool(cross_kv_fp8)
        # engine options of the MODEL: set on lane 0 before its first encode and replayed on every lane created later (_lane)
        self._lane_options: List[Tuple[str, int]] = [("xkv_fp8", 2)] if self.cross_kv_fp8 else []
        self._engine_ctor = (_engine_factory or Engine)
        self._engine_args = (dims, _COMPUTE_ALIASES[compute_type], max_batch, device_index)
        self._lanes = [self._engine_ctor(*self._engine_args)]     # lane 0 owns the device weights
        self._lanes[0].load_weights(tensors)
        self._apply_lane_options(self._lanes[0])
        self._tls = threading.local()                             # which lane the calling thread drives (default: 0)
        self._vad_state = None                                    # the device VAD's tensors, replayed into every lane (_lane)
        if vad_model is not None:
            self.load_vad(vad_model)
        self.special = self.engine.special
        self.max_batch = max_batch
        self.is_multilingual = dims.vocab >= 51865
        self.n_window = dims.n_frames * HOP

    # ------------------------------------------------------------------------------------------
    @property
    def engine(self):
        """The engine context of the calling thread: lane 0 unless the thread was bound to another lane by transcribe_groups."""
        tls = self.__dict__.get("_tls")
        return self.__dict__["_lanes"][getattr(tls, "lane", 0) if tls is not None else 0]

    @engine.setter
    def engine(self, e):
        """Replaces lane 0 (tests install engine doubles on a bare model)."""
        self.__dict__.setdefault("_tls", threading.local())
        lanes = self.__dict__.setdefault("_lanes", [])
        if lanes:
            lanes[0] = e
        else:
            lanes.append(e)

    def _apply_lane_options(self, engine) -> None:
        """The model-level engine options on one engine context (an engine without set_option - the oracle seam - has none)."""
        setter = getattr(engine, "set_option", None)
        if setter is None:
            return
        for key, value in getattr(self, "_lane_options", ()):   # a bare model (tests build one without __init__) has none
            setter(key, value)

    # -- keyword biasing (seq_bias.py) ------------------------------------------
    def _bias_table(self, sequence_bias, prompt_words, prompt_word_boost):
        """The sequence-bias table of one call from its three options, checked (None: the call has none)."""
        return seq_bias.resolve(sequence_bias, prompt_words, prompt_word_boost, self.tokenizer.encode, self.dims.vocab)

    @contextlib.contextmanager
    def _sequence_bias(self, table):
        """`table` installed on the calling thread's engine context (its lane) from here to the end of the block, whatever ends it."""
        if table is None:
            yield
            return
        setter = getattr(self.engine, "set_sequence_bias", None)
        if setter is None:
            raise ValueError("sequence_bias / prompt_words need an engine with Engine.set_sequence_bias")
        setter(table)
        try:
            yield
        finally:
            setter(None)

    def _biased_segments(self, segments, table):
        """The lazy segments of `transcribe` with the table installed while they are produced."""
        with self._sequence_bias(table):
            yield from segments

    def _lane(self, i: int):
        """Engine context `i` (created on first use, sharing lane 0's device weights and the model's engine options)."""
        while len(self._lanes) <= i:
            try:
                lane = self._engine_ctor(*self._engine_args, share_weights_with=self._lanes[0])
            except TypeError:       # the oracle test seam has no weight sharing: pipelining is a HIP-engine feature
                raise RuntimeError("pipeline_depth > 1 needs the HIP engine")
            self._lanes.append(lane)
            self._apply_lane_options(lane)
            if self.has_device_vad:   # VAD weights are per context: a sharer loads its own 1.3 MB copy
                lane.load_vad(self._vad_state)
        return self._lanes[i]

    # -- voice activity detection on the device ------------------------------------------------------
    @property
    def has_device_vad(self) -> bool:
        """True once load_vad() has put the VAD network on the model's engine contexts."""
        return self.__dict__.get("_vad_state") is not None

    def load_vad(self, path_or_mapping) -> None:
        """Loads the Silero-v5-shaped VAD network (vad.load_silero_state) into every engine context of the model; contexts created
        later get it too.  From then on vad_filter=True filters with it, unless a vad_speech_prob_fn is given."""
        state = vad.load_silero_state(path_or_mapping)
        for lane in self._lanes:
            lane.load_vad(state)
        self._vad_state = state

    def vad_speech_probs(self, audios: Sequence[np.ndarray]) -> List[np.ndarray]:
        """One speech probability per 512-sample frame of every recording, from the device network (Engine.vad_probs: all
        recordings in one call, max_batch at a time)."""
        if not self.has_device_vad:
            raise RuntimeError("no VAD network is loaded (WhisperModel(vad_model=...) or model.load_vad(...))")
        return self.engine.vad_probs(list(audios))

    def _vad_source(self, params: dict, prob_fn, stacklevel: int = 3):
        """The speech-probability source of a vad_filter=True call, in this order: an explicit vad_speech_prob_fn, the device
        network, the vad_parameters={"backend": "energy"} opt-in, none (a warning; the whole clip counts as speech).
        -> ("fn", callable) | ("device", None) | ("none", None); `backend` is removed from params."""
        backend = params.pop("backend", None)
        if prob_fn is not None:
            return "fn", prob_fn
        if self.has_device_vad:
            return "device", None
        if backend == "energy":
            warnings.warn("vad_filter=True with the short-time-energy stand-in (NOT equivalent to Silero VAD)", stacklevel=stacklevel)
            return "fn", None   # get_speech_timestamps' default
        warnings.warn("vad_filter=True: the Silero VAD network is not available in this build and no "
                      "vad_speech_prob_fn was given; the whole clip is treated as speech", stacklevel=stacklevel)
        return "none", None

    # -- speaker diarization ------------------------------------------------------------------------------
    @property
    def has_diarization(self) -> bool:
        """True once load_diarization() has put the segmentation and the speaker-embedding network on lane 0."""
        return bool(self.__dict__.get("_diarization"))

    def load_diarization(self, seg_weights, spk_weights) -> None:
        """Loads the PyanNet-shaped segmentation network (vad.load_pyannet_state) and the XVectorSincNet-shaped speaker-embedding
        network (diarization.load_xvector_state) into lane 0, the context diarize() runs on (a few hundred MB of scratch belong to
        a context that runs them, so the other lanes stay without).  A segmentation network lane 0 already holds is kept."""
        from . import diarization
        lane = self._lanes[0]
        if not getattr(lane, "has_segmentation", False):
            lane.load_segmentation(vad.load_pyannet_state(seg_weights))
        lane.load_speaker_embedding(diarization.load_xvector_state(spk_weights))
        self._diarization = True

    def diarize(self, audio: Union[str, np.ndarray], num_speakers: Optional[int] = None, audio_channel=None, dsp_mode=None,
                **kw) -> list:
        """Who spoke when: a list of diarization.Turn(start, end, speaker) in seconds, speakers "SPEAKER_00", "SPEAKER_01", ... in
        order of first appearance.  Two device calls - the segmentation network, then the speaker embeddings of every chunk's
        local speakers - with the masks on the host between them, then clustering and reconstruction on the host
        (diarization.diarize; its keywords - threshold, onset, min_duration_on, min_duration_off, ... - pass through).
        num_speakers forces the number of clusters.  dsp_mode (dsp.resolve; None = off): both networks read the enhanced
        recording (Engine.enhance, once)."""
        from . import diarization
        dsp_params = dsp.resolve(dsp_mode)
        if not self.has_diarization:
            raise RuntimeError("no diarization networks are loaded (model.load_diarization(seg_weights, spk_weights))")
        if isinstance(audio, str):
            audio = decode_audio(audio, channel=parse_audio_channel(audio_channel))
        audio = np.asarray(audio, dtype=np.float32)
        if dsp_params is not None:
            audio = self._lanes[0].enhance([audio], params=dsp_params)[0]
        return diarization.diarize(self._lanes[0], audio, num_speakers=num_speakers, **kw)

    def transcribe_diarized(self, audio: Union[str, np.ndarray], num_speakers: Optional[int] = None,
                            diarization_options: Optional[dict] = None, dsp_mode=None, **kw) -> Tuple[list, TranscriptionInfo]:
        """transcribe(audio, **kw) with every segment's speaker: ([(Segment, speaker or None), ...], info).  The speaker of a
        segment is the one whose turns overlap it longest (diarization.assign_speakers); Segment keeps its fields.
        dsp_mode (dsp.resolve; None = off): the recording is enhanced once (Engine.enhance) and both passes read the result."""
        from . import diarization
        dsp_params = dsp.resolve(dsp_mode)
        if isinstance(audio, str):   # read once, for both passes
            audio = decode_audio(audio, channel=parse_audio_channel(kw.pop("audio_channel", None)))
        if dsp_params is not None:
            audio = self.engine.enhance([np.asarray(audio, dtype=np.float32)], params=dsp_params)[0]
        turns = self.diarize(audio, num_speakers=num_speakers, **(diarization_options or {}))
        segments, info = self.transcribe(audio, **kw)
        segments = list(segments)
        return list(zip(segments, diarization.assign_speakers(segments, turns))), info

    # -- file ingest on the device --------------------------------------------------------------------
    def decode_audio_many(self, paths_or_arrays: Sequence[Union[str, np.ndarray]], audio_channel=None, dsp_mode=None
                          ) -> List[np.ndarray]:
        """Every path -> mono float32 @16 kHz with ONE device call for all the files the device takes (read_audio_coded +
        Engine.ingest on the calling thread's engine context: conversion or G.711 / IMA ADPCM / FLAC decoding, downmix and the
        polyphase resampler run on the device over the whole batch).  Every path is read once: a file the device does not take
        - a rate outside the accepted ratios, more than 8 channels, or any file on an engine without `ingest` - is decoded on
        the host from what was read, as decode_audio does it; a container read_audio_coded has no reader for goes through
        decode_audio.  Arrays pass through.
        audio_channel (None / "mix", "left", "right" or an index from 0: parse_audio_channel) picks one channel of every path
        instead of their mean; with an array among the inputs it is refused: an array is already mono.
        The device resampler is decode_audio's (scipy.signal.resample_poly) accumulated in float32 instead of float64.
        dsp_mode (dsp.resolve; None = off): every result - arrays that passed through included - goes through ONE
        Engine.enhance call once it is mono float32 at 16 kHz."""
        from . import _lib
        eng = self.engine
        dsp_params = dsp.resolve(dsp_mode)
        pick = parse_audio_channel(audio_channel)
        out: List[Optional[np.ndarray]] = [None] * len(paths_or_arrays)
        jobs = []
        for i, a in enumerate(paths_or_arrays):
            if not isinstance(a, str):
                if pick is not None:
                    raise ValueError("audio_channel picks a channel of a file: an array input is already mono")
                out[i] = np.asarray(a)
                continue
            raw = read_audio_coded(a)
            if raw is None:
                out[i] = decode_audio(a, channel=pick)
                continue
            c = audio_io._pick_channel(a, pick, raw.channels)
            if callable(getattr(eng, "ingest", None)) and raw.channels <= 8 and eng.ingest_accepts(raw.rate):
                jobs.append((i, raw))
            else:      # the host path over what was read
                out[i] = audio_io.resample(audio_io.decode_coded(raw, c), raw.rate)
        if jobs:
            args = [[getattr(r, k) for _, r in jobs] for k in ("samples", "rate", "channels", "format")]
            if pick is None and all(r.format < _lib.PCM_ALAW for _, r in jobs):
                got = eng.ingest(*args)
            else:
                got = eng.ingest(*args, block_aligns=[r.block_align for _, r in jobs], picks=[pick] * len(jobs),
                                 n_frames=[r.n_frames for _, r in jobs])
            for (i, _), y in zip(jobs, got):
                out[i] = y
        if dsp_params is not None:
            return eng.enhance([np.asarray(a, dtype=np.float32) for a in out], params=dsp_params)
        return out

    def transcribe_groups(self, groups: Sequence[Sequence[Union[str, np.ndarray]]], pipeline_depth: Optional[int] = None, **kw
                          ) -> List[List[Tuple[List[Segment], TranscriptionInfo]]]:
        """`transcribe_many(group, **kw)` for every group of files, with up to `pipeline_depth` groups in flight: each worker
        thread drives its own engine context (own HIP stream, KV pools, workspaces; ONE shared copy of the weights), so one
        group's log-mel / encoder pass runs under another's decode chain - on one batch the decode phase leaves most of the
        chip idle between its ~45 000 dependent launches (measured +27 % audio-s/s with two contexts).
        Every group is processed exactly as a serial transcribe_many call would process it (same grouping, same engine
        inputs): the results are identical, file by file, to pipeline_depth = 1; returned in group order.
        clip_timestamps, hallucination_silence_threshold, prompt_reset_on_temperature, suppress_tokens (among **kw): as in
        transcribe_many; a per-file clip list holds for the files of EVERY group, so it needs groups of one length.
        sequence_bias / prompt_words / prompt_word_boost (among **kw): one table, built once, installed by every worker on its own
        engine context for each of its groups.
        device_resample=True (one of **kw): each worker ingests its group's paths on its own engine context; audio_channel (one
        of **kw) picks a channel of every path, as in transcribe_many.
        dsp_mode (one of **kw): checked once here; each worker enhances its group's recordings on its own engine context."""
        if kw.get("dsp_mode") is not None:
            kw = dict(kw, dsp_mode=dsp.resolve(kw["dsp_mode"]))
        if any(kw.get(k) is not None for k in ("sequence_bias", "prompt_words")):
            # tokenised and checked once; every worker's transcribe_many installs the table on its own engine context
            if kw.get("continuous"):
                seq_bias.refuse_in_session("transcribe_groups(continuous=True)", kw.get("sequence_bias"), kw.get("prompt_words"))
            table = self._bias_table(kw.pop("sequence_bias", None), kw.pop("prompt_words", None), kw.pop("prompt_word_boost", None))
            kw = dict(kw, sequence_bias=dict(table) if table else None)
        depth = max(1, min(int(pipeline_depth or self.pipeline_depth), len(groups) or 1, 4))
        if depth == 1:
            return [self.transcribe_many(g, **kw) for g in groups]
        for i in range(depth):
            self._lane(i)
        out: List = [None] * len(groups)
        nxt = iter(range(len(groups)))
        lock, errs = threading.Lock(), []

        def worker(lane: int):
            self._tls.lane = lane
            try:
                while not errs:
                    with lock:
                        gi = next(nxt, None)
                    if gi is None:
                        return
                    out[gi] = self.transcribe_many(groups[gi], **kw)
            except BaseException as ex:      # re-raised on the caller's thread
                errs.append(ex)
            finally:
                self._tls.lane = 0
        th = [threading.Thread(target=worker, args=(i,), name=f"ttasr-lane{i}") for i in range(depth)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]
        return out

    def close(self):
        """Destroys every engine context of this model (the sharers first, then the owner of the weights)."""
        for e in reversed(getattr(self, "_lanes", [])):
            e.close()
        self._lanes = []

    def _lang_token(self, language: str) -> int:
        if not self.is_multilingual:
            return self.special.lang_zh
        if language not in LANGUAGES:
            raise ValueError(f"unknown language {language!r}")
        return self.special.sot + 1 + LANGUAGES.index(language)

    def detect_language(self, audio: np.ndarray) -> Tuple[str, float, List[Tuple[str, float]]]:
        """Language = argmax over the language tokens of the logits after <|startoftranscript|>."""
        return self.detect_language_batch([audio])[0]

    def _ranked(self, probs: np.ndarray) -> List[Tuple[str, float]]:
        """One row of language probabilities -> [(language, probability)] by falling probability (ties: vocabulary order)."""
        order = np.argsort(-probs, kind="stable")
        return [(LANGUAGES[i], float(probs[i])) for i in order]

    def _detect_resident(self, B: int) -> List[Tuple[str, float, List[Tuple[str, float]]]]:
        """(language, probability, all probabilities) of the B clips whose encoder state is resident (Engine.detect_language)."""
        idx, probs = self.engine.detect_language(B)
        return [(LANGUAGES[int(idx[b])], float(probs[b, int(idx[b])]), self._ranked(probs[b])) for b in range(B)]

    def detect_language_batch(self, audios_or_windows: Sequence[np.ndarray]) -> List[Tuple[str, float, List[Tuple[str, float]]]]:
        """detect_language for many clips: the first 30-s window of each, max_batch at a time - one log-mel, one encoder pass and
        one decoder pass that ends in the language head (ttasr_detect_language) per chunk; softmax and argmax run on the device."""
        eng = self.engine
        out: List[Tuple[str, float, List[Tuple[str, float]]]] = []
        for i in range(0, len(audios_or_windows), self.max_batch):
            chunk = [np.ascontiguousarray(np.asarray(a)[: self.n_window], dtype=np.float32) for a in audios_or_windows[i:i + self.max_batch]]
            eng.set_audio_ctx(0)
            eng.log_mel(chunk, want_output=False)
            eng.encode(len(chunk))
            out.extend(self._detect_resident(len(chunk)))
        return out

    def _check_languages(self, language, n: int, what: str) -> List[Optional[str]]:
        """`language` of a batched surface -> one entry per item: a string (every item), None (detect every item) or a sequence
        of n strings / None."""
        if language is None or isinstance(language, str):
            langs: List[Optional[str]] = [language] * n
        else:
            langs = list(language)
            if len(langs) != n:
                raise ValueError(f"language needs one entry per {what} ({n}), got {len(langs)}")
        for l in langs:
            if l is not None and not isinstance(l, str):
                raise ValueError(f"language entries must be a language code or None, got {l!r}")
            if l is not None:
                self._lang_token(l)   # raises on a code this build cannot name
        return langs

    def _resolve_languages(self, language, first_windows: Sequence[np.ndarray], what: str
                           ) -> List[Tuple[str, float, Optional[List[Tuple[str, float]]]]]:
        """(language, probability, all probabilities or None) per item: given languages count as certain, None entries are
        detected from `first_windows` in batched passes (detect_language_batch)."""
        langs = self._check_languages(language, len(first_windows), what)
        out: List = [(l, 1.0, None) for l in langs]
        todo = [i for i, l in enumerate(langs) if l is None]
        if todo and not self.is_multilingual:
            for i in todo:
                out[i] = ("en", 1.0, None)
        elif todo:
            for i, r in zip(todo, self.detect_language_batch([first_windows[i] for i in todo])):
                out[i] = r
        return out

    def _prompt(self, lang_tok: int, task: str, without_timestamps: bool, prev: Sequence[int],
                hotwords: Optional[Sequence[int]] = None, prefix: Optional[Sequence[int]] = None) -> Tuple[List[int], int]:
        """faster-whisper get_prompt: [<|startofprev|> hotwords… previous…] <|startoftranscript|> <|lang|> <|task|>
        [<|notimestamps|>] [<|0.00|> prefix…]; hotwords are dropped when a prefix is given, each part is capped at
        n_text_ctx // 2 - 1 tokens.  Returns (prompt, position of <|startoftranscript|>)."""
        st = self.special
        half = self.dims.n_text_ctx // 2 - 1
        p: List[int] = []
        use_hot = bool(hotwords) and not prefix
        hot = list(hotwords)[:half] if use_hot else []
        pre = list(prefix)[:half] if prefix else []
        # hotwords + previous text + prefix could exceed the 448-token context (faster-whisper does not guard this
        # corner): the oldest previous tokens give way so that at least 32 positions stay free for the transcript
        fixed = 1 + len(hot) + 3 + int(without_timestamps) + (len(pre) + (0 if without_timestamps else 1) if pre else 0)
        keep_prev = max(0, min(half, self.dims.n_text_ctx - 32 - fixed))
        prev = list(prev)[-keep_prev:] if keep_prev and prev else []
        if prev or use_hot:
            p.append(st.sot_prev)
            p.extend(hot)
            p.extend(prev)
        sot_index = len(p)
        p.append(st.sot)
        p.append(lang_tok)
        p.append(st.translate if task == "translate" else st.transcribe)
        if without_timestamps:
            p.append(st.no_timestamps)
        if pre:
            if not without_timestamps:
                p.append(st.timestamp_begin)
            p.extend(pre)
        return p, sot_index

    def _split_segments(self, tokens: List[int], seek: int, n_frames_window: int, time_offset: float,
                        without_timestamps: bool):
        """Split one window's tokens on timestamp pairs (openai-whisper / faster-whisper segment rule).
        Returns (list of (start, end, tokens), frames to advance)."""
        st = self.special
        tb = st.timestamp_begin
        prec = 0.02
        toks = [t for t in tokens if t != st.eot]
        is_ts = [t >= tb for t in toks]
        out = []
        single_end = len(is_ts) >= 2 and is_ts[-1] and not is_ts[-2]
        consec = [i for i in range(1, len(toks)) if is_ts[i] and is_ts[i - 1]]
        if consec and not without_timestamps:
            slices = list(consec)
            if single_end:
                slices.append(len(toks))
            last = 0
            for cur in slices:
                sl = toks[last:cur]
                if sl:
                    out.append((time_offset + (sl[0] - tb) * prec, time_offset + (sl[-1] - tb) * prec, sl))
                last = cur
            if single_end:
                advance = n_frames_window
            else:
                advance = (toks[last - 1] - tb) * 2  # timestamp units of 20 ms -> 10-ms frames
        else:
            dur = n_frames_window * HOP / SAMPLE_RATE
            ts = [t for t in toks if t >= tb]
            if ts and ts[-1] != tb and not without_timestamps:
                dur = (ts[-1] - tb) * prec
            if toks:
                out.append((time_offset, time_offset + dur, toks))
            advance = n_frames_window
        return out, max(int(advance), 1)

    # ------------------------------------------------------------------------------------------
    def transcribe(self, audio: Union[str, np.ndarray], language: Optional[str] = None, task: str = "transcribe",
                   beam_size: int = 5, word_timestamps: bool = False, vad_filter: bool = False,
                   condition_on_previous_text: bool = True, initial_prompt: Optional[str] = None,
                   without_timestamps: bool = False, max_new_tokens: Optional[int] = None,
                   no_speech_threshold: Optional[float] = 0.6, log_prob_threshold: Optional[float] = -1.0,
                   max_initial_timestamp: float = 1.0, suppress_blank: bool = True,
                   temperature: Union[float, Sequence[float]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0), best_of: int = 5,
                   compression_ratio_threshold: Optional[float] = 2.4, multilingual: bool = False,
                   language_detection_threshold: Optional[float] = 0.5, language_detection_segments: int = 1,
                   device_resample: bool = False, audio_channel=None, clip_timestamps: Union[str, Sequence[float]] = "0",
                   hallucination_silence_threshold: Optional[float] = None, prompt_reset_on_temperature: float = 0.5,
                   suppress_tokens: Optional[Sequence[int]] = (-1,), sequence_bias=None, prompt_words=None,
                   prompt_word_boost: Optional[float] = None, dsp_mode=None, **kwargs
                   ) -> Tuple[Iterator[Segment], TranscriptionInfo]:
        """dsp_mode (None; the reference service's dspMode): None / 0 / False = off, nothing new runs; 1 / True = denoise, high-pass
        and level (the product's 1); a dsp.DspParams or a dict of its fields = as given.  The recording is enhanced ONCE on the
        device (Engine.enhance: length-preserving, so every time keeps its meaning) as soon as it is mono float32 at 16 kHz;
        VAD, language detection, log-mel and alignment all read the enhanced samples.  The definition is this project's own and
        its effect on CER is unmeasured.
        sequence_bias ({tuple of token ids: bias}; None): HF Transformers' SequenceBiasLogitsProcessor on the device - a sequence
        of one token always adds its bias to that token's raw logit, a longer one adds it to its last token when the history
        (prompt, then everything sampled, timestamps included) ends in its first tokens; the Whisper rules run afterwards and
        avg_logprob is that of the biased distribution.  At most 16 tokens per sequence, 4096 distinct last tokens, 8192 sequences
        longer than one token, finite biases (Engine.set_sequence_bias).
        prompt_words (a comma-separated string or a list of names and proper nouns; None): expanded into such a table
        (seq_bias.expand_prompt_words: every prefix of two or more tokens of each phrase, with and without a leading space, gets
        prompt_word_boost, the first token alone half of it).  The prompt is not touched: combine with hotwords yourself.
        prompt_word_boost (None = 2.0): a starting value nobody has measured - no trained checkpoint is available offline.
        The table is installed while the segments are produced and cleared afterwards; detection and alignment passes stay raw.
        clip_timestamps ("0"; a comma-separated string or a list of seconds: start, end, start, end, ...; an odd count runs the
        last clip to the end; an end past the recording is clamped): only those spans are decoded (parse_clip_timestamps).  A
        window ends where its clip does (Engine.log_mel_windows(n_frames=...)), the dynamic-range floor stays the whole
        recording's, previous-text conditioning carries across clips as across windows, language=None detects from the windows
        that start at the first clip's start, and vad_filter=True with clips other than the whole recording skips the VAD with a
        warning.  "0", [0] and [0, duration] are today's run, bit for bit.
        hallucination_silence_threshold (seconds; None): with word_timestamps=True, silence longer than this around a segment
        whose words look invented (alignment.is_segment_anomaly) is skipped and the segment dropped (skip_hallucinations has the
        rules); without word_timestamps one warning says it has no effect.
        prompt_reset_on_temperature (0.5): a window decoded above this temperature is not carried into the next prompt.
        suppress_tokens ([-1]): -1 stands for the model's list, other ids are added to it; without -1 only the given ids and
        the task / start tokens no search may emit are suppressed; an id outside the vocabulary raises ValueError.
        These four restate openai-whisper's transcribe(), which faster-whisper copies, from memory: unpinned.
        device_resample=True (path input only): the file is converted, downmixed and resampled on the device
        (decode_audio_many) instead of on the host.
        audio_channel (path input only; None / "mix", "left", "right" or an index from 0): that channel of the file alone
        instead of the mean of its channels, on either path.  Refused with an array, which is already mono.
        language=None: the language is detected from the first `language_detection_segments` 30-s windows (select_language:
        the first window whose top probability exceeds `language_detection_threshold`, else the majority).  multilingual=True:
        every window is detected again between its encoder pass and its search, and its prompt carries that window's language
        token (code-switched speech); info.language stays the file-level answer."""
        # faster-whisper options this build does not implement are never silently ignored when they differ from
        # their defaults (the reference call sites pass none of them)
        neutral = {"patience": None, "vad_parameters": None, "vad_speech_prob_fn": None, "length_penalty": 1, "repetition_penalty": 1,
                   "no_repeat_ngram_size": 0,
                   "prepend_punctuations": alignment.PREPEND_PUNCTUATIONS, "append_punctuations": alignment.APPEND_PUNCTUATIONS,
                   "chunk_length": None, "log_progress": False}
        for k, v in kwargs.items():
            if k in ("patience", "vad_parameters", "vad_speech_prob_fn", "hotwords", "prefix"):
                continue
            if k not in neutral:
                raise TypeError(f"transcribe() got an unexpected keyword argument {k!r}")
            if v is not None and v != neutral[k]:
                warnings.warn(f"transcribe(): option {k}={v!r} is not implemented in this build and is ignored", stacklevel=2)
        suppress = self._user_suppress(suppress_tokens)
        threshold = self._silence_threshold(hallucination_silence_threshold, word_timestamps)
        bias_table = self._bias_table(sequence_bias, prompt_words, prompt_word_boost)
        dsp_params = dsp.resolve(dsp_mode)
        pick = parse_audio_channel(audio_channel)
        if isinstance(audio, str):
            audio = self.decode_audio_many([audio], audio_channel=pick)[0] if device_resample else decode_audio(audio, channel=pick)
        elif pick is not None:
            raise ValueError("audio_channel picks a channel of a file: an array input is already mono")
        audio = np.asarray(audio)
        if audio.ndim != 1:
            # asr_core.py:156 loads with mono=False; faster-whisper rejects 2-D input the same way
            raise ValueError(f"audio must be mono float32 [n] @16 kHz, got shape {audio.shape}")
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        if beam_size < 1:
            raise ValueError("beam_size must be >= 1")
        if beam_size > 7:
            raise ValueError(f"beam_size={beam_size}: the beam-search kernel keeps at most 7 hypotheses per clip")
        if beam_size > self.max_batch:
            raise ValueError(f"beam_size={beam_size} needs {beam_size} decode rows but this model was built with "
                             f"max_batch={self.max_batch}; construct WhisperModel(..., max_batch>={beam_size})")
        if int(language_detection_segments) < 1:
            raise ValueError("language_detection_segments must be >= 1")
        chunks = None
        clips = parse_clip_timestamps(clip_timestamps, _frames_of(len(audio)))
        if vad_filter and clips != [(0, _frames_of(len(audio)))]:
            # faster-whisper filters only at the default clip_timestamps (from memory: unpinned); the clips are times of the recording
            warnings.warn("vad_filter=True is skipped: clip_timestamps already names the spans to decode", stacklevel=2)
            vad_filter = False
        if dsp_params is not None:   # every argument is checked: the first device work of the call, in front of the VAD
            audio = self.engine.enhance([audio], params=dsp_params)[0]
        if vad_filter:
            # faster-whisper: Silero VAD -> speech chunks -> transcribe their concatenation -> restore the time line.
            # The network is not available offline: with a speech-probability function supplied by the operator
            # (`vad_speech_prob_fn=` here or `model.vad_speech_prob_fn`), or with the explicit opt-in
            # vad_parameters={"backend": "energy"}, the full pipeline runs; otherwise the whole clip counts as speech.
            # With a VAD network loaded (WhisperModel(vad_model=...)) the probabilities come from the device.
            params = dict(kwargs.get("vad_parameters") or {})
            kind, prob_fn = self._vad_source(params, kwargs.get("vad_speech_prob_fn") or self.vad_speech_prob_fn)
            if kind == "device":
                prob_fn = lambda a: self.engine.vad_probs([a])[0]
            if kind != "none":
                chunks = vad.get_speech_timestamps(audio, vad.VadOptions(**params), prob_fn)
                audio_full_len = len(audio)
                audio = vad.collect_chunks(audio, chunks)
                clips = parse_clip_timestamps("0", _frames_of(len(audio)))
        duration_after_vad = len(audio) / SAMPLE_RATE
        duration = (audio_full_len if chunks is not None else len(audio)) / SAMPLE_RATE
        if language is None:
            if self.is_multilingual:
                k = int(language_detection_segments)
                first = clips[0][0] * HOP   # detection reads the windows that start where the first clip does
                found = self.detect_language_batch([audio[first + i * self.n_window:] for i in range(k)
                                                    if i == 0 or first + i * self.n_window < len(audio)])
                language, lang_p, i = select_language([(f[0], f[1]) for f in found], language_detection_threshold)
                all_p = found[i][2]
            else:
                language, lang_p, all_p = "en", 1.0, None
        else:
            lang_p, all_p = 1.0, None
        info = TranscriptionInfo(language=language, language_probability=lang_p, duration=duration,
                                 duration_after_vad=duration_after_vad, all_language_probs=all_p,
                                 transcription_options=dict(beam_size=beam_size, task=task, without_timestamps=without_timestamps,
                                                            condition_on_previous_text=condition_on_previous_text,
                                                            initial_prompt=initial_prompt))
        segments = self._generate_segments(audio, language, task, condition_on_previous_text, initial_prompt,
                                           without_timestamps, max_new_tokens, no_speech_threshold, log_prob_threshold,
                                           max_initial_timestamp, suppress_blank, beam_size, kwargs.get("patience", 1.0),
                                           tuple(temperature) if isinstance(temperature, (list, tuple)) else (float(temperature),),
                                           best_of, compression_ratio_threshold, bool(word_timestamps),
                                           kwargs.get("hotwords"), kwargs.get("prefix"),
                                           multilingual=bool(multilingual) and self.is_multilingual, clips=clips,
                                           suppress_tokens=suppress, prompt_reset_on_temperature=float(prompt_reset_on_temperature),
                                           hallucination_silence_threshold=threshold)
        if bias_table is not None:
            segments = self._biased_segments(segments, bias_table)
        if chunks is not None:
            segments = vad.restore_speech_timestamps(segments, chunks)
        return segments, info

    def transcribe_batched(self, audio: Union[str, np.ndarray], **kw) -> Tuple[Iterator[Segment], TranscriptionInfo]:
        """One long recording through faster-whisper's batched form (batched.BatchedInferencePipeline(self).transcribe, which
        documents the keywords): VAD chunks packed into groups of at most one window, every group an independent clip of one
        continuous-batching beam session, fallbacks retried on the held cross-KV.  audio_channel (path input only) picks one
        channel of the file instead of the mean of its channels; dsp_mode (as in `transcribe`) enhances the recording once, before
        the VAD and before the session opens."""
        from .batched import BatchedInferencePipeline
        seq_bias.refuse_in_session("transcribe_batched", kw.pop("sequence_bias", None), kw.pop("prompt_words", None))
        kw.pop("prompt_word_boost", None)
        return BatchedInferencePipeline(self).transcribe(audio, **kw)

    # -- pieces of faster-whisper's generate_segments / generate_with_fallback, shared by the single-file loop and by
    #    transcribe_many (several files in lock step through one engine pass) -------------------------------------
    def _user_suppress(self, suppress_tokens) -> Optional[Tuple[int, ...]]:
        """`suppress_tokens` of transcribe() checked: None for the default [-1] (the model's list, as _window_opts builds it), else
        the ids as a tuple.  An id other than -1 outside the vocabulary raises ValueError."""
        ids = [] if suppress_tokens is None else [int(t) for t in suppress_tokens]
        for t in ids:
            if t != -1 and not 0 <= t < self.dims.vocab:
                raise ValueError(f"suppress_tokens: id {t} is outside the vocabulary [0, {self.dims.vocab})")
        return None if ids and all(t == -1 for t in ids) else tuple(ids)

    @staticmethod
    def _silence_threshold(threshold, word_timestamps: bool, stacklevel: int = 3) -> Optional[float]:
        """`hallucination_silence_threshold` checked: it works on word times, so without word_timestamps it is None here after one
        warning (openai-whisper's command line says the same)."""
        if threshold is None:
            return None
        threshold = float(threshold)
        if not np.isfinite(threshold) or threshold < 0:
            raise ValueError(f"hallucination_silence_threshold={threshold!r}: a finite, non-negative number of seconds or None")
        if not word_timestamps:
            warnings.warn("hallucination_silence_threshold has no effect without word_timestamps=True", stacklevel=stacklevel)
            return None
        return threshold

    def _score(self, res, row: int):
        """(tokens, avg_logprob, no_speech_prob, compression_ratio) of one decoded row."""
        st = self.special
        toks = res.tokens[row]
        # faster-whisper: avg_logprob = cum_logprob / (seq_len + 1), seq_len without <|endoftext|> (whose
        # log-probability is part of the sum): the same divisor whether or not this path returns the EOT
        n_tok = len([t for t in toks if t != st.eot]) + 1
        avg_lp = float(res.sum_logprob[row]) / n_tok
        raw = self.tokenizer.decode([t for t in toks if t < st.eot]).encode("utf-8")
        cr = (len(raw) / max(1, len(zlib.compress(raw)))) if raw else 0.0
        return toks, avg_lp, float(res.no_speech_prob[row]), cr

    @staticmethod
    def _needs_fallback(avg_lp, ns, cr, p) -> bool:
        """faster-whisper generate_with_fallback: retry at the next temperature when the text is too repetitive or too
        unlikely; the retry is cancelled only for a window that is BOTH probably silent and unlikely (no_speech_prob above
        its threshold, log_prob_threshold set and avg_logprob below it) - a silent-looking window with an acceptable
        log-probability but a high compression ratio is still retried."""
        needs = False
        if p["compression_ratio_threshold"] is not None and cr > p["compression_ratio_threshold"]:
            needs = True
        if p["log_prob_threshold"] is not None and avg_lp < p["log_prob_threshold"]:
            needs = True
        if p["no_speech_threshold"] is not None and ns > p["no_speech_threshold"] and \
                p["log_prob_threshold"] is not None and avg_lp < p["log_prob_threshold"]:
            needs = False  # silence
        return needs

    def _decode_with_fallback(self, prompt, opts, seek: int, p, first=None):
        """generate_with_fallback for the clip resident at index 0: temperature 0 = beam/greedy (or `first`, an already
        scored temperature-0 attempt), then sampled retries (best_of hypotheses) while the result is too repetitive
        (zlib compression ratio) or too unlikely (avg log-prob).  -> (temperature, tokens, avg_lp, no_speech, ratio)"""
        eng = self.engine
        attempts = []
        for temp in p["temperatures"]:
            if temp <= 0.0 and first is not None:
                toks, avg_lp, ns, cr = first
            else:
                if temp <= 0.0:
                    res = eng.generate_beam([prompt], p["beam_size"], opts, p["patience"]) if p["beam_size"] > 1 \
                        else eng.generate([prompt], opts)
                else:
                    rows = max(1, min(p["best_of"], self.max_batch))
                    res = eng.generate_sample([prompt], rows, opts, temp, seed=self._fallback_seed(seek, temp))
                toks, avg_lp, ns, cr = self._score(res, 0)
            attempts.append((temp, toks, avg_lp, ns, cr))
            if not self._needs_fallback(avg_lp, ns, cr, p):
                return attempts[-1]
        return self._best_attempt(attempts, p)

    @staticmethod
    def _best_attempt(attempts, p):
        """Every temperature failed: keep the most likely attempt among the non-repetitive ones."""
        thr = p["compression_ratio_threshold"]
        ok = [a for a in attempts if thr is None or a[4] <= thr]
        return max(ok or attempts, key=lambda a: a[2])

    @staticmethod
    def _fallback_seed(seek: int, temp: float) -> int:
        return (seek * 1000003 + int(temp * 1000)) & 0x7FFFFFFF

    def _window_opts(self, prompt_len: int, sot_index: int, p):
        st = self.special
        budget = min(p["max_new"], self.dims.n_text_ctx - prompt_len)
        # the model directory's own lists win (CTranslate2 config.json "suppress_ids" / "suppress_ids_begin", what
        # faster-whisper reads for suppress_tokens=[-1] / suppress_blank); otherwise the published defaults
        cfg = self.ct2_config
        sup = None
        if cfg.get("suppress_ids"):
            sup = sorted({int(t) for t in cfg["suppress_ids"] if 0 <= int(t) < self.dims.vocab} |
                         {st.transcribe, st.translate, st.sot, st.sot_prev} | ({st.sot_lm} if st.sot_lm >= 0 else set()))
        user = p.get("suppress_tokens")
        if user is not None:   # faster-whisper get_suppressed_tokens: -1 = the model's list, the rest is added; never the task / start tokens
            from .engine import default_suppress
            model_list = default_suppress(st, self.dims.vocab)
            always = [t for t in (st.translate, st.transcribe, st.sot, st.sot_prev, st.no_speech, st.sot_lm) if t >= 0]
            sup = sorted({t for t in user if t >= 0} | set((sup or model_list) if -1 in user else always))
        bsup = [int(t) for t in cfg["suppress_ids_begin"] if 0 <= int(t) < self.dims.vocab] if cfg.get("suppress_ids_begin") else [220, st.eot]
        return self.engine.gen_opts(budget, timestamps=not p["without_timestamps"], sot_index=sot_index, suppress=sup,
                                    begin_suppress=bsup if p["suppress_blank"] else [],
                                    max_initial_timestamp_index=int(round(p["max_initial_timestamp"] / 0.02)), check_interval=4)

    def _finish_window(self, fs: dict, clip_index: int, attempt, win_frames: int, p, defer: Optional[list] = None) -> List[Segment]:
        """Turns one window's chosen attempt into segments and advances the file state `fs` (seek, previous tokens,
        prompt reset, segment counter).  The window's encoder state must still be resident at `clip_index` when word
        timestamps are wanted.
        defer (a list; the continuous form with word_timestamps): the alignment is NOT run here.  A window with kept segments
        appends one record to `defer` and returns []; the file state advances as always - seek, previous text and the segment
        counter do not depend on the words - and `_deferred_segments(record, words)` builds the segments once the caller has
        aligned the window.  A silent or empty window appends nothing."""
        eng, st = self.engine, self.special
        temp_used, toks, avg_lp, ns, cr = attempt
        seek = fs["seek"]
        time_offset = seek * HOP / SAMPLE_RATE
        if p["no_speech_threshold"] is not None and ns > p["no_speech_threshold"] and \
                (p["log_prob_threshold"] is None or avg_lp < p["log_prob_threshold"]):
            fs["seek"] += win_frames  # silent window: skip it entirely
            return []
        segs, advance = self._split_segments(toks, seek, win_frames, time_offset, p["without_timestamps"])
        limit = time_offset + win_frames * HOP / SAMPLE_RATE  # never report times past the audio that exists
        kept = []
        for (s0, s1, stoks) in segs:
            text = self.tokenizer.decode([t for t in stoks if t < st.eot])
            s0, s1 = min(s0, limit), min(s1, limit)
            if s0 >= s1 or not text.strip():
                continue
            kept.append(dict(start=s0, end=s1, tokens=list(stoks), text=text, eot=st.eot, words=None))
        deferred = defer is not None and p["word_timestamps"] and bool(kept)
        if p["word_timestamps"] and kept:
            # faster-whisper add_word_timestamps: one alignment pass over the window's text tokens (the encoder
            # state of this window is still resident), then words are dealt to the segments
            text_tokens = [t for seg in kept for t in seg["tokens"] if t < st.eot]
            task_tok = st.translate if p["task"] == "translate" else st.transcribe
            if deferred:
                defer.append(dict(fs=fs, kept=kept, text_tokens=text_tokens, frames=win_frames, offset=time_offset, limit=limit,
                                  idx=fs["idx"], seek=seek, stats=(temp_used, avg_lp, cr, ns),
                                  language=fs.get("language", p["language"]), lang_tok=fs.get("lang_tok", p["lang_tok"]), task_tok=task_tok))
            else:
                found = alignment.find_alignment(eng, self.tokenizer, st, clip_index, text_tokens, win_frames, self.alignment_heads,
                                                 fs.get("language", p["language"]), fs.get("lang_tok", p["lang_tok"]), task_tok)
                alignment.add_word_timestamps(kept, found, time_offset)
                for seg in kept:
                    seg["start"], seg["end"] = min(seg["start"], limit), min(seg["end"], limit)
        next_seek = seek + (min(advance, win_frames) if advance > 0 else win_frames)
        if p.get("hallucination_silence_threshold") is not None and p["word_timestamps"] and not deferred:
            body = [t for t in toks if t != st.eot]
            single_end = len(body) >= 2 and body[-1] >= st.timestamp_begin and body[-2] < st.timestamp_begin
            kept, next_seek, nothing = skip_hallucinations(kept, single_end, seek, win_frames, next_seek,
                                                           p["hallucination_silence_threshold"], fs.get("last_speech_end", 0.0),
                                                           fs["n_total"], self.dims.n_frames)
            if nothing:   # leading silence before invented text: the window is looked at again from where that text starts
                fs["seek"] = next_seek
                return []
            ends = [seg["words"][-1].end for seg in kept if seg["words"]]
            if ends:
                fs["last_speech_end"] = ends[-1]
        out = []
        for seg in kept:
            if not deferred:
                out.append(Segment(fs["idx"], seek, round(seg["start"], 3), round(seg["end"], 3), seg["text"], seg["tokens"],
                                   temp_used, avg_lp, cr, ns, seg["words"]))
            fs["idx"] += 1
            # faster-whisper's all_tokens: the tokens of every YIELDED segment, timestamp tokens included (the
            # previous-text prompt carries them), <|endoftext|> and the undecided tail after the last pair excluded
            fs["prev"].extend(t for t in seg["tokens"] if t != st.eot)
        if not p["condition"] or temp_used > p.get("prompt_reset_on_temperature", 0.5):  # faster-whisper's default: 0.5
            fs["prompt_reset"] = len(fs["prev"])  # prompt_reset_since: nothing carries over
        fs["seek"] = next_seek
        return out

    @staticmethod
    def _deferred_segments(rec: dict, words: List[dict]) -> List[Segment]:
        """The segments of a window whose alignment `_finish_window(defer=...)` put off: words dealt to its kept segments as
        `_finish_window` deals them, ids and statistics as recorded when the window settled."""
        temp_used, avg_lp, cr, ns = rec["stats"]
        alignment.add_word_timestamps(rec["kept"], words, rec["offset"])
        out = []
        for k, seg in enumerate(rec["kept"]):
            s0, s1 = min(seg["start"], rec["limit"]), min(seg["end"], rec["limit"])
            out.append(Segment(rec["idx"] + k, rec["seek"], round(s0, 3), round(s1, 3), seg["text"], seg["tokens"], temp_used, avg_lp,
                               cr, ns, seg["words"]))
        return out

    def _align_held(self, s, recs: List[dict]) -> None:
        """The windows that settled in one poll, each held by the session under rec["id"]: ONE Session.align call (first_row = the
        sot sequence's length, num_frames = the window's frames, as find_alignment_batch builds them; every window with its own
        language token), then each window's segments go to its file.  The call releases the clips."""
        st = self.special
        sots = [[st.sot, r["lang_tok"], r["task_tok"]] for r in recs]
        seqs = [sot + [st.no_timestamps] + list(r["text_tokens"]) + [st.eot] for sot, r in zip(sots, recs)]
        res = s.align([r["id"] for r in recs], seqs, [3] * len(recs), [int(r["frames"]) for r in recs], self.alignment_heads)
        for k, r in enumerate(recs):
            words = alignment.words_from_alignment(self.tokenizer, st, r["text_tokens"], res.start_frames[k] / alignment.TOKENS_PER_SECOND,
                                                   res.logprobs[k], 3, r["language"])
            r["fs"]["segments"].extend(self._deferred_segments(r, words))

    def _file_feature_max(self, audio: np.ndarray) -> float:
        """faster-whisper extracts the features of the whole (VAD-filtered) recording once, so the dynamic-range floor
        `max - 8` is the FILE's, not the window's: a first pass over all windows (max_batch at a time; ~1 ms per 32 windows)
        returns the per-window log-mel maxima, their maximum is handed to every window's feature call."""
        n_frames = len(audio) // HOP
        if n_frames <= 0:
            return 0.0
        # the seeks below step by the model's FULL window: a reduced audio context left behind by transcribe_windows(audio_ctx=...)
        # would make every call cover only part of its 3000 frames and the maximum miss most of the recording
        self.engine.set_audio_ctx(0)
        seeks = list(range(0, n_frames, self.dims.n_frames))
        best = -np.inf
        for i in range(0, len(seeks), self.max_batch):
            _, mx = self.engine.log_mel_windows(audio, seeks[i:i + self.max_batch], want_max=True)
            best = max(best, float(np.max(mx)))
        return best

    def _new_file_state(self, audio: np.ndarray, initial_prompt: Optional[str], clips: Optional[List[Tuple[int, int]]] = None) -> dict:
        """clips: the (start, end) frame pairs of parse_clip_timestamps; None = the whole recording."""
        prev: List[int] = []
        if initial_prompt:
            prev.extend(self.tokenizer.encode(" " + initial_prompt.strip()))
        n_total = _frames_of(len(audio))
        clips = list(clips) if clips else [(0, n_total)]
        return dict(audio=audio, n_total=n_total, prev=prev, prompt_reset=0, seek=clips[0][0], idx=0, clips=clips, clip=0)

    def _next_window(self, fs: dict) -> Optional[int]:
        """Moves fs["seek"] to the next frame a clip of the file wants decoded - up to the start of the current clip, or on to the
        next clip once the current one is used up (openai-whisper's seek_clips loop) - and returns the frames of the window that
        starts there: min(the model's window, frames left in the recording, frames left in the clip).  None: the file is done."""
        clips = fs["clips"]
        while fs["clip"] < len(clips):
            start, end = clips[fs["clip"]]
            if fs["seek"] < start:
                fs["seek"] = start
            if fs["seek"] < min(end, fs["n_total"]):
                return min(self.dims.n_frames, fs["n_total"] - fs["seek"], end - fs["seek"])
            fs["clip"] += 1
            if fs["clip"] < len(clips):
                fs["seek"] = clips[fs["clip"]][0]
        return None

    def _window_features(self, group: Sequence[dict], frames: Sequence[int]) -> None:
        """The feature call of one pass: window i starts at group[i]'s seek and keeps frames[i] frames.  The cut form of the call is
        used only when a clip ends a window before the model's window or the recording would."""
        eng = self.engine
        whole = [min(self.dims.n_frames, fs["n_total"] - fs["seek"]) for fs in group]
        cut = dict(n_frames=list(frames)) if any(n < w for n, w in zip(frames, whole)) else {}
        eng.log_mel_windows([fs["audio"] for fs in group], [fs["seek"] for fs in group], floor_max=[fs["file_max"] for fs in group], **cut)

    def _params(self, language, task, condition, without_timestamps, max_new_tokens, no_speech_threshold, log_prob_threshold,
                max_initial_timestamp, suppress_blank, beam_size, patience, temperatures, best_of,
                compression_ratio_threshold, word_timestamps, hotwords=None, prefix=None, suppress_tokens=None,
                prompt_reset_on_temperature=0.5, hallucination_silence_threshold=None) -> dict:
        enc = lambda t: self.tokenizer.encode(" " + t.strip()) if t else None
        return dict(hotwords_tokens=enc(hotwords), prefix_tokens=enc(prefix), language=language, lang_tok=self._lang_token(language), task=task, condition=condition,
                    without_timestamps=without_timestamps, max_new=max_new_tokens or (self.dims.n_text_ctx // 2),
                    no_speech_threshold=no_speech_threshold, log_prob_threshold=log_prob_threshold,
                    max_initial_timestamp=max_initial_timestamp, suppress_blank=suppress_blank, beam_size=beam_size,
                    patience=patience, temperatures=tuple(temperatures), best_of=best_of,
                    compression_ratio_threshold=compression_ratio_threshold, word_timestamps=word_timestamps,
                    suppress_tokens=suppress_tokens, prompt_reset_on_temperature=prompt_reset_on_temperature,
                    hallucination_silence_threshold=hallucination_silence_threshold)

    def _generate_segments(self, audio, language, task, condition, initial_prompt, without_timestamps, max_new_tokens,
                           no_speech_threshold, log_prob_threshold, max_initial_timestamp, suppress_blank, beam_size=1,
                           patience=1.0, temperatures=(0.0,), best_of=5, compression_ratio_threshold=2.4,
                           word_timestamps=False, hotwords=None, prefix=None, multilingual=False, clips=None, suppress_tokens=None,
                           prompt_reset_on_temperature=0.5, hallucination_silence_threshold=None) -> Iterator[Segment]:
        eng = self.engine
        p = self._params(language, task, condition, without_timestamps, max_new_tokens, no_speech_threshold,
                         log_prob_threshold, max_initial_timestamp, suppress_blank, beam_size, patience, temperatures, best_of,
                         compression_ratio_threshold, word_timestamps, hotwords, prefix, suppress_tokens,
                         prompt_reset_on_temperature, hallucination_silence_threshold)
        fs = self._new_file_state(audio, initial_prompt, clips)
        eng.set_audio_ctx(0)
        # before the first window: the floor is the recording's, not the window's - and not the clips'
        fs["file_max"] = self._file_feature_max(audio)
        while True:
            win_frames = self._next_window(fs)
            if win_frames is None:
                break
            seek = fs["seek"]
            eng.set_audio_ctx(0)
            self._window_features([fs], [win_frames])
            eng.encode(1)
            if multilingual:   # this window's language, from the encoder state that is resident anyway
                p["language"] = self._detect_resident(1)[0][0]
                p["lang_tok"] = self._lang_token(p["language"])
            prompt, sot_index = self._prompt(p["lang_tok"], task, without_timestamps, fs["prev"][fs["prompt_reset"]:],
                                             p["hotwords_tokens"], p["prefix_tokens"] if seek == 0 else None)
            attempt = self._decode_with_fallback(prompt, self._window_opts(len(prompt), sot_index, p), seek, p)
            yield from self._finish_window(fs, 0, attempt, win_frames, p)

    @_lock_step_bias
    def transcribe_many(self, audios: Sequence[Union[str, np.ndarray]],
                        language: Union[None, str, Sequence[Optional[str]]] = "zh", task: str = "transcribe",
                        beam_size: int = 5, word_timestamps: bool = False, condition_on_previous_text: bool = True,
                        initial_prompt: Optional[str] = None, without_timestamps: bool = False,
                        max_new_tokens: Optional[int] = None, no_speech_threshold: Optional[float] = 0.6,
                        log_prob_threshold: Optional[float] = -1.0, max_initial_timestamp: float = 1.0,
                        suppress_blank: bool = True, temperature: Union[float, Sequence[float]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                        best_of: int = 5, compression_ratio_threshold: Optional[float] = 2.4, patience: float = 1.0,
                        hotwords: Optional[str] = None, prefix: Optional[str] = None, continuous: bool = False,
                        multilingual: bool = False, detect_in_session: bool = False, session_prefill: Union[int, bool] = 0,
                        vad_filter: bool = False, vad_parameters: Optional[dict] = None, device_resample: bool = False,
                        retry_held: Optional[bool] = None, audio_channel=None,
                        clip_timestamps: Union[str, Sequence] = "0", hallucination_silence_threshold: Optional[float] = None,
                        prompt_reset_on_temperature: float = 0.5, suppress_tokens: Optional[Sequence[int]] = (-1,),
                        dsp_mode=None) -> List[Tuple[List[Segment], TranscriptionInfo]]:
        """dsp_mode (as in `transcribe`; lock-step and continuous=True alike): every file is enhanced in ONE Engine.enhance call
        over the group once the files are mono float32 at 16 kHz - before the VAD, before language detection and before a session
        begins.
        sequence_bias, prompt_words, prompt_word_boost (keywords; as in `transcribe`): the table is installed on this call's
        engine context for the call and cleared when it ends; refused with continuous=True (ValueError before any device work).

        Several FILES in lock step: every round takes the next 30-s window of each unfinished file and runs them as
        ONE engine pass (log-mel, encoder, beam search with one previous-text prompt per file), so a folder is
        transcribed at batch throughput while each file keeps exactly the sequential algorithm of `transcribe` — its
        own seek, prompt, thresholds.  A window that fails the temperature-0 thresholds is re-decoded alone through the
        same fallback ladder.  Files are sharded by file across GPUs by the caller (batch_cli), never by window.

        continuous=True: one continuous-batching beam session instead of lock-step passes (DESIGN.md "Long-form files in the
        session"): every file keeps one window in flight, a window that fails the thresholds goes back in at the next
        temperature (sampled attempts run in the session too), and a file's next window is submitted as soon as its current
        one is settled.  Each file gets exactly `transcribe()`'s algorithm.
        continuous=True with word_timestamps=True: the session runs in hold mode with option
        align_packed = 1.  A window that settles with kept segments stays held and its file's next window is submitted at once
        (seek and previous text do not depend on the words); when a poll's results are handled, the windows that settled in it
        are aligned in ONE Session.align call and their words dealt to their segments as `transcribe` deals them; a window that
        settles silent or empty is released.  Nothing stays held across a poll.  The packed pass makes a window's word times
        independent of the windows aligned with it: a file gets the same words alone and in any folder.
        retry_held (continuous=True; default None = True with word_timestamps, else False): a window that fails its thresholds
        goes up the temperature ladder with Session.retry on its HELD cross-KV - same prompt (carrying a language already
        detected), budget, rows and seed as the re-submission - so a fallback attempt costs no encoder pass; False re-submits the
        window as before.  retry_held=True without word_timestamps runs hold mode and releases settled windows.  Both need an
        engine whose sessions can hold (Engine.session_hold).

        language: one code for every file (as before), None (detect every file) or one entry per file, each a code or None.
        The None files are detected from their first windows in batched passes BEFORE decoding starts - with continuous=True
        before the session begins, which costs one extra encoder pass over those first windows (a session owns the encoder
        while it is open).  Each file's TranscriptionInfo carries its own language, probability and all_language_probs.
        detect_in_session=True (continuous=True only): no pass before the session - a None file's first window goes in with the
        language placeholder (Session.DETECT), its first decode step finds the language on the device, and that answer fills the
        file's TranscriptionInfo and the prompts of its later windows; a fallback attempt carries the language already found.
        multilingual=True: every window is detected again - lock-step form: between its encoder pass and its search, from the
        encoder state that is resident anyway; continuous=True: inside the session, every window goes in with the placeholder -
        and its prompt carries that window's language token (info.window_languages lists them); info.language stays the
        file-level answer.
        session_prefill=N (continuous=True only; True = config.SESSION_PREFILL_DEFAULT): a window whose prompt has at least N
        prefillable positions - the previous text of condition_on_previous_text, up to <|startoftranscript|> - gets them from one
        admission pass of the session instead of N forced decode steps (Engine.session(prefill=N)); windows
        that go in with the language placeholder are forced as before.
        vad_filter=True (lock-step and continuous=True alike): every file is filtered as `transcribe` filters it, BEFORE decoding
        starts - with a VAD network loaded, ONE device call over all files (Engine.vad_probs; with continuous=True before the
        session begins), else the model's vad_speech_prob_fn, the vad_parameters={"backend": "energy"} opt-in or the warning of
        `transcribe`.  Each file decodes the concatenation of its speech chunks; its segments are mapped back to the original
        time line and its info carries duration / duration_after_vad as `transcribe` fills them.  A file the VAD empties yields no
        segments and takes no decode row.
        device_resample=True: the paths among `audios` are converted, downmixed and resampled in ONE device call for the group
        (decode_audio_many) before the VAD and before a session begins, instead of file by file on the calling thread; an engine
        without `ingest` ignores the flag.
        audio_channel (None / "mix", "left", "right" or an index from 0): that channel of every path instead of the mean of its
        channels, with or without device_resample; refused when an array is among `audios`.
        clip_timestamps, hallucination_silence_threshold, prompt_reset_on_temperature, suppress_tokens: as in `transcribe`;
        clip_timestamps is one value for every file (a string or a flat list of seconds) or one such value per file, and a file
        with clips other than its whole recording is not VAD-filtered (a warning).  With a threshold a window's words decide
        its file's next seek: the lock-step form aligns a window before its file advances, as it always did.  continuous=True
        refuses the first two at any but their neutral values with a ValueError before the session opens ([0, duration] too:
        refuse_in_session): a session's window cannot end before the recording does, and it aligns a window after its file
        has moved on."""
        from .engine import session_prefill_value
        eng = self.engine
        dsp_params = dsp.resolve(dsp_mode)
        if continuous:
            refuse_in_session("transcribe_many(continuous=True)", clip_timestamps, hallucination_silence_threshold)
        session_prefill = session_prefill_value(session_prefill)
        if session_prefill and not continuous:
            raise ValueError("session_prefill needs continuous=True (the lock-step passes prefill their prompts already: option prefill)")
        if continuous and not callable(getattr(eng, "session", None)):
            raise ValueError("continuous=True needs an engine with continuous-batching sessions (Engine.session)")
        if detect_in_session and not continuous:
            raise ValueError("detect_in_session=True needs continuous=True (the lock-step form detects from its resident passes)")
        if retry_held is None:
            retry_held = bool(continuous and word_timestamps)
        if retry_held and not continuous:
            raise ValueError("retry_held=True needs continuous=True (the lock-step form re-decodes a failed window alone)")
        if continuous and (word_timestamps or retry_held) and not getattr(eng, "session_hold", False):
            raise ValueError("word_timestamps=True / retry_held=True with continuous=True need an engine whose sessions can hold "
                             "finished windows (Engine.session_hold: Session.hold / align / retry)")
        beam = max(1, min(beam_size, 7, self.max_batch))
        per_pass = max(1, self.max_batch // beam)
        temps = tuple(temperature) if isinstance(temperature, (list, tuple)) else (float(temperature),)
        langs = self._check_languages(language, len(audios), "file")
        p = self._params(next((l for l in langs if l is not None), "en"), task, condition_on_previous_text, without_timestamps,
                         max_new_tokens, no_speech_threshold, log_prob_threshold, max_initial_timestamp, suppress_blank, beam,
                         patience, temps, best_of, compression_ratio_threshold, bool(word_timestamps), hotwords, prefix,
                         self._user_suppress(suppress_tokens), float(prompt_reset_on_temperature),
                         self._silence_threshold(hallucination_silence_threshold, word_timestamps))
        if continuous:
            p["beam_size"] = int(beam_size)
        pcm = []
        pick = parse_audio_channel(audio_channel)
        if pick is not None and any(not isinstance(a, str) for a in audios):
            raise ValueError("audio_channel picks a channel of a file: an array input is already mono")
        for a in (self.decode_audio_many(audios, audio_channel=pick) if device_resample else audios):
            a = decode_audio(a, channel=pick) if isinstance(a, str) else np.asarray(a)
            if a.ndim != 1:
                raise ValueError(f"audio must be mono float32 [n] @16 kHz, got shape {a.shape}")
            pcm.append(np.ascontiguousarray(a, dtype=np.float32))
        full_len = [len(a) for a in pcm]
        speech: List[Optional[list]] = [None] * len(pcm)   # per file: its speech chunks on the original time line (None: not filtered)
        file_clips = [parse_clip_timestamps(c, _frames_of(len(a))) for c, a in zip(_clip_lists(clip_timestamps, len(pcm)), pcm)]
        clipped = [c != [(0, _frames_of(len(a)))] for c, a in zip(file_clips, pcm)]
        if vad_filter and any(clipped):
            warnings.warn("vad_filter=True is skipped for the files whose clip_timestamps already name the spans to decode", stacklevel=2)
        if dsp_params is not None and pcm:   # the arguments are checked: one call for the group, in front of the VAD
            pcm = list(eng.enhance(pcm, params=dsp_params))
        if vad_filter and pcm:
            params = dict(vad_parameters or {})
            kind, prob_fn = self._vad_source(params, self.vad_speech_prob_fn)
            if kind != "none":
                options = vad.VadOptions(**params)
                probs = self.engine.vad_probs(pcm) if kind == "device" else None   # all files, one device call
                for i, a in enumerate(pcm):
                    if clipped[i]:
                        continue
                    speech[i] = vad.get_speech_timestamps(a, options, (lambda _a, q=probs[i]: q) if probs is not None else prob_fn)
                    pcm[i] = vad.collect_chunks(a, speech[i])
        files = []
        for a, chunks, n_full, clips in zip(pcm, speech, full_len, file_clips):
            fs = self._new_file_state(a, initial_prompt, clips if chunks is None else None)
            fs["segments"], fs["speech"], fs["full_len"] = [], chunks, n_full
            fs["file_max"] = self._file_feature_max(fs["audio"])   # whole-file dynamic-range floor, as `transcribe`
            files.append(fs)
        multilingual = bool(multilingual) and self.is_multilingual
        session_stats = None   # Session.stats() of a continuous run in hold mode (word_timestamps / retry_held), in every file's info
        # files whose language the session itself finds: they skip the detection pass; "decided" = the file-level answer is known
        late = [l is None and bool(detect_in_session) and self.is_multilingual for l in langs]
        found = self._resolve_languages(["en" if w else l for l, w in zip(langs, late)],
                                        [fs["audio"][fs["clips"][0][0] * HOP:] for fs in files], "file")   # from the first clip's start
        for fs, (lang, lang_p, all_p), w in zip(files, found, late):
            fs["language"], fs["lang_tok"], fs["lang_info"] = lang, self._lang_token(lang), (lang, lang_p, all_p)
            fs["decided"] = not w
        if continuous:
            session_stats = self._run_continuous(files, p, per_window=multilingual, session_prefill=session_prefill,
                                                 retry_held=bool(retry_held))
        while not continuous:
            active = []
            for fs in files:
                fs["frames"] = self._next_window(fs)   # None: the file is done
                if fs["frames"] is not None:
                    active.append(fs)
            if not active:
                break
            for g in range(0, len(active), per_pass):
                group = active[g:g + per_pass]
                eng.set_audio_ctx(0)
                self._window_features(group, [fs["frames"] for fs in group])
                eng.encode(len(group))
                if multilingual:   # the windows' own languages, from the encoder state of the pass
                    for fs, r in zip(group, self._detect_resident(len(group))):
                        fs["language"], fs["lang_tok"] = r[0], self._lang_token(r[0])
                prompts, sots = [], []
                for fs in group:
                    pr, si = self._prompt(fs["lang_tok"], task, without_timestamps, fs["prev"][fs["prompt_reset"]:],
                                          p["hotwords_tokens"], p["prefix_tokens"] if fs["seek"] == 0 else None)
                    prompts.append(pr)
                    sots.append(si)
                # one budget for the pass: the shortest prompt's; the 448-token context cuts longer prompts' rows short
                opts = self._window_opts(min(len(pr) for pr in prompts), 0, p)
                res = eng.generate_beam(prompts, beam, opts, patience, sot_index=sots)
                first = [self._score(res, i) for i in range(len(group))]
                redo = []
                for i, fs in enumerate(group):
                    toks, avg_lp, ns, cr = first[i]
                    win_frames = fs["frames"]
                    if temps[0] <= 0.0 and self._needs_fallback(avg_lp, ns, cr, p) and len(temps) > 1:
                        redo.append((fs, prompts[i], sots[i], first[i], win_frames))
                    else:
                        fs["segments"].extend(self._finish_window(fs, i, (temps[0], toks, avg_lp, ns, cr), win_frames, p))
                for fs, pr, si, fst, win_frames in redo:   # rare: this window alone, through the whole ladder
                    self._window_features([fs], [win_frames])
                    eng.encode(1)
                    attempt = self._decode_with_fallback(pr, self._window_opts(len(pr), si, p), fs["seek"], p, first=fst)
                    fs["segments"].extend(self._finish_window(fs, 0, attempt, win_frames, p))
        out = []
        for fs in files:
            dur_after = len(fs["audio"]) / SAMPLE_RATE
            dur = fs["full_len"] / SAMPLE_RATE
            if fs["speech"] is not None:   # back to the original time line, as `transcribe` does
                fs["segments"] = list(vad.restore_speech_timestamps(fs["segments"], fs["speech"]))
            lang, lang_p, all_p = fs["lang_info"]
            info = TranscriptionInfo(language=lang, language_probability=lang_p, duration=dur, duration_after_vad=dur_after,
                                     all_language_probs=all_p,
                                     transcription_options=dict(beam_size=beam, task=task, without_timestamps=without_timestamps,
                                                                condition_on_previous_text=condition_on_previous_text,
                                                                initial_prompt=initial_prompt),
                                     window_languages=fs.get("window_languages"), session=session_stats)
            out.append((fs["segments"], info))
        return out

    def _session_language(self, r) -> Tuple[str, float, List[Tuple[str, float]]]:
        """(language, probability, all probabilities) of a SessionResult that was detected inside its session."""
        return LANGUAGES[r.language], float(r.language_probs[r.language]), self._ranked(r.language_probs)

    def _run_continuous(self, files: List[dict], p: dict, per_window: bool = False, session_prefill: int = 0, retry_held: bool = False):
        """transcribe_many(continuous=True): the windows of all files through one beam session, one window per file in flight.
        A window's attempts follow `_decode_with_fallback` (temperature 0: beam search of beam_size rows, or greedy with one;
        temperature > 0: best_of samples seeded as `transcribe` seeds them), its result `_finish_window`.
        A window of a file whose language is not decided yet (fs["decided"] False: detect_in_session), and with per_window
        (multilingual) every window, goes in with the language placeholder; the session's answer replaces it in the window's
        prompt, so a fallback attempt carries the language already found.
        p["word_timestamps"] or retry_held: hold mode (transcribe_many's docstring).  Every finished attempt is then held; it is
        retried (retry_held), released (re-submitted, silent, empty, or no words wanted) or - settled with kept segments and words
        wanted - aligned behind the poll's results with the others of the poll.  Without either, exactly the calls of before."""
        eng = self.engine
        temps, beam = p["temperatures"], p["beam_size"]
        if not 1 <= beam <= 7:
            raise ValueError(f"beam_size={beam} outside [1, 7]")
        if beam > self.max_batch:
            raise ValueError(f"beam_size={beam} needs {beam} decode rows but this model was built with max_batch={self.max_batch}")
        rows_sampled = max(1, min(p["best_of"], self.max_batch))
        width = max(beam, rows_sampled) if any(t > 0.0 for t in temps) else beam
        if width > 7:
            raise ValueError(f"best_of={p['best_of']}: a continuous session holds at most 7 rows per window")
        todo = [fs for fs in files if fs["seek"] < fs["n_total"]]
        if not todo:
            return None
        n_ctx = self.dims.n_text_ctx
        opts = self._window_opts(1, 0, p)   # the session's rules; budgets and sot indices are per window
        eng.set_audio_ctx(0)
        arm = per_window or any(not fs["decided"] for fs in todo)
        kw = dict(detect_language=True) if arm else {}   # armed only when a window asks for it
        if session_prefill:
            kw["prefill"] = int(session_prefill)          # prompts of at least that many positions: one admission pass, not steps
        words = bool(p["word_timestamps"])
        hold = words or retry_held
        if words:
            eng.set_option("align_packed", 1)   # read by every Session.align of the run; put back below
        try:
            return self._continuous_session(todo, p, opts, n_ctx, width, kw, per_window, rows_sampled, hold, retry_held)
        finally:
            if words:
                eng.set_option("align_packed", 0)

    def _continuous_session(self, todo, p, opts, n_ctx, width, kw, per_window, rows_sampled, hold, retry_held):
        """The session of `_run_continuous`, open from here to the last window; -> in hold mode Session.stats() plus "windows" (windows
        decoded) and "retries" (attempts that ran on a held clip's cross-KV), else None."""
        from .engine import GenResult, Session, TtasrError
        eng = self.engine
        temps, beam = p["temperatures"], p["beam_size"]
        with eng.session(opts, n_ctx - 1, beam=width, patience=p["patience"], **kw) as s:
            inflight: Dict[int, dict] = {}
            if hold:
                s.hold()
            settled: List[dict] = []   # this poll's windows that wait for their alignment (held)
            count = dict(windows=0, retries=0)

            def retry(fs: dict, held_id: int):
                w = fs["window"]
                temp = temps[len(w["attempts"])]
                ids = s.retry([held_id], [w["prompt"]], [w["sot"]], max_new=[w["budget"]], temperature=[temp],
                              rows=[rows_sampled if temp > 0.0 else beam], seed=[self._fallback_seed(fs["seek"], temp)])
                inflight[ids[0]] = fs
                count["retries"] += 1

            def submit(fs: dict):
                w = fs["window"]
                temp = temps[len(w["attempts"])]
                ids = s.submit_windows([fs["audio"]], [fs["seek"]], [w["prompt"]], [w["sot"]], max_new=[w["budget"]],
                                       floor_max=[fs["file_max"]], temperature=[temp],
                                       rows=[rows_sampled if temp > 0.0 else beam], seed=[self._fallback_seed(fs["seek"], temp)])
                inflight[ids[0]] = fs

            def next_window(fs: dict):
                detect = per_window or not fs["decided"]
                pr, si = self._prompt(Session.DETECT if detect else fs.get("lang_tok", p["lang_tok"]), p["task"], p["without_timestamps"],
                                      fs["prev"][fs["prompt_reset"]:], p["hotwords_tokens"], p["prefix_tokens"] if fs["seek"] == 0 else None)
                fs["window"] = dict(prompt=pr, sot=si, budget=min(p["max_new"], n_ctx - len(pr)), attempts=[],
                                    frames=min(self.dims.n_frames, fs["n_total"] - fs["seek"]))
                count["windows"] += 1
                submit(fs)

            for fs in todo:
                next_window(fs)
            while inflight:
                got = s.poll()
                if not got:
                    raise TtasrError(f"session idle with {len(inflight)} windows unfinished")
                for r in got:
                    fs = inflight.pop(r.id)
                    w = fs["window"]
                    if r.language is not None:   # detected inside the session: this window's language, and the file's if undecided
                        found = self._session_language(r)
                        fs["language"], fs["lang_tok"] = found[0], self._lang_token(found[0])
                        w["prompt"][w["sot"] + 1] = fs["lang_tok"]
                        if not fs["decided"]:
                            fs["lang_info"], fs["decided"] = found, True
                        if per_window:
                            fs.setdefault("window_languages", []).append(found[0])
                    temp = temps[len(w["attempts"])]
                    res = GenResult([r.tokens], np.asarray([r.sum_logprob], np.float32), np.asarray([r.no_speech_prob], np.float32))
                    toks, avg_lp, ns, cr = self._score(res, 0)
                    w["attempts"].append((temp, toks, avg_lp, ns, cr))
                    if self._needs_fallback(avg_lp, ns, cr, p):
                        if len(w["attempts"]) < len(temps):
                            if retry_held:
                                retry(fs, r.id)   # the next temperature of the ladder, on the held cross-KV
                            else:
                                if hold:
                                    s.release([r.id])
                                submit(fs)        # the next temperature of the ladder
                            continue
                        attempt = self._best_attempt(w["attempts"], p)
                    else:
                        attempt = w["attempts"][-1]
                    n_wait = len(settled)
                    fs["segments"].extend(self._finish_window(fs, 0, attempt, w["frames"], p, defer=settled if hold else None))
                    if len(settled) > n_wait:
                        settled[-1]["id"] = r.id          # stays held until the poll's alignment below
                    elif hold:
                        s.release([r.id])                 # silent, empty, or no words wanted
                    if fs["seek"] < fs["n_total"]:
                        next_window(fs)
                if settled:                               # nothing stays held across a poll
                    self._align_held(s, settled)
                    settled.clear()
            if not hold:
                return None                               # without hold mode the session sees exactly the calls of before
            stats = dict(s.stats())
            stats["windows"], stats["retries"] = float(count["windows"]), float(count["retries"])
            return stats

    # ------------------------------------------------------------------------------------------
    def _pass_languages(self, langs: Sequence[Optional[str]], info: List[Tuple[str, float]]) -> List[str]:
        """Languages of one resident pass: the None entries are detected from the pass's encoder state (no extra encoder pass);
        (language, probability) of every clip is appended to `info`."""
        found: List[Tuple[str, float]] = [(l, 1.0) for l in langs]   # type: ignore[misc]
        if any(l is None for l in langs):
            det = self._detect_resident(len(langs)) if self.is_multilingual else [("en", 1.0, None)] * len(langs)
            found = [(d[0], d[1]) if l is None else (l, 1.0) for l, d in zip(langs, det)]
        info.extend(found)
        return [f[0] for f in found]

    def transcribe_batch(self, clips: Sequence[np.ndarray], language: Union[None, str, Sequence[Optional[str]]] = "zh",
                         task: str = "transcribe", without_timestamps: bool = True, max_new_tokens: int = 224) -> List[List[int]]:
        """Batched single-window path (clips <= 30 s each): one engine pass for up to max_batch clips.
        Returns the sampled token ids per clip.  This is the unit the data-parallel layer shards.
        language: one code, None (detect every clip) or one entry per clip (a code or None); None clips are detected from the
        pass's own encoder state.  (language, probability) per clip of the last call: `last_language_info`."""
        eng = self.engine
        out: List[List[int]] = []
        langs = self._check_languages(language, len(clips), "clip")
        info: List[Tuple[str, float]] = []
        for i in range(0, len(clips), self.max_batch):
            chunk = [np.ascontiguousarray(c[: self.n_window], dtype=np.float32) for c in clips[i:i + self.max_batch]]
            eng.set_audio_ctx(0)
            eng.log_mel(chunk, want_output=False)
            eng.encode(len(chunk))
            prompts = [self._prompt(self._lang_token(l), task, without_timestamps, []) for l in
                       self._pass_languages(langs[i:i + self.max_batch], info)]
            prompt, sot_index = prompts[0]
            opts = eng.gen_opts(min(max_new_tokens, self.dims.n_text_ctx - len(prompt)), timestamps=not without_timestamps,
                                sot_index=sot_index)
            out.extend(eng.generate([pr for pr, _ in prompts], opts).tokens)
        self.last_language_info = info
        return out

    def transcribe_stream(self, clips: Sequence[np.ndarray], language: Union[None, str, Sequence[Optional[str]]] = "zh",
                          task: str = "transcribe",
                          without_timestamps: bool = True, max_new_tokens: int = 224,
                          row_max_new: Optional[Sequence[int]] = None, beam_size: int = 1, patience: float = 1.0,
                          initial_prompt: Optional[str] = None, word_timestamps: bool = False, detect_in_session: bool = False,
                          session_prefill: Union[int, bool] = 0, clip_timestamps="0", hallucination_silence_threshold=None,
                          sequence_bias=None, prompt_words=None, dsp_mode=None):
        """transcribe_batch's contract (clips <= 30 s each, sampled token ids per clip, input order) for any number of clips,
        through a continuous-batching session: a clip that finishes hands its decode row to the next one instead of waiting for
        the rest of its batch.  row_max_new (optional): one token budget per clip, each in [1, max_new_tokens].
        beam_size > 1: beam search (a clip takes a group of beam_size rows; tokens without EOT, as transcribe_windows decodes
        them); initial_prompt: previous text in front of <|startoftranscript|>, as transcribe_windows builds it.
        word_timestamps=True: (tokens, words) per clip, words as transcribe_windows returns them; the session runs in hold mode
        (a finished clip keeps its row and cross-KV slot) and the clips one poll returned are aligned in one device pass.
        language: one code, None (detect every clip) or one entry per clip (a code or None).  None clips are detected in batched
        passes BEFORE the session begins (a session owns the encoder while it is open): one extra encoder pass over those
        clips.  detect_in_session=True: no pass before the session - a None clip goes in with the language placeholder
        (Session.DETECT) and its first decode step finds the language on the device (one more decode step, no encoder work).
        (language, probability) per clip of the last call: `last_language_info`.
        session_prefill=N (True = config.SESSION_PREFILL_DEFAULT): a clip whose prompt - the initial_prompt's previous text - has
        at least N prefillable positions gets them from one admission pass of the session instead of N forced decode steps
        (Engine.session(prefill=N)); clips that go in with the language placeholder are forced as before.
        clip_timestamps / hallucination_silence_threshold: accepted at their neutral values only; anything else is a ValueError
        before the session opens (they belong to the window loop: transcribe, lock-step transcribe_many).
        sequence_bias / prompt_words: refused when given (a session's kernels do not apply the table).
        dsp_mode: refused when it asks for enhancement (dsp.refuse_streaming): a live utterance needs a causal, stateful noise
        tracker, which is out of scope."""
        dsp.refuse_streaming(dsp_mode, "transcribe_stream")
        from .engine import Session, session_prefill_value
        refuse_in_session("transcribe_stream", clip_timestamps, hallucination_silence_threshold)
        seq_bias.refuse_in_session("transcribe_stream", sequence_bias, prompt_words)
        session_prefill = session_prefill_value(session_prefill)
        if len(clips) == 0:
            self.last_language_info = []
            return []
        eng = self.engine
        beam = int(beam_size)
        if not 1 <= beam <= 7:
            raise ValueError(f"beam_size {beam} outside [1, 7]")
        for c in clips:
            if len(c) > self.n_window:
                raise ValueError(f"transcribe_stream takes clips of at most one window ({self.n_window} samples)")
        langs = self._check_languages(language, len(clips), "clip")
        late = [l is None and bool(detect_in_session) and self.is_multilingual for l in langs]   # found by the session itself
        found = self._resolve_languages(["en" if w else l for l, w in zip(langs, late)], clips, "clip")
        info = [(f[0], f[1]) for f in found]
        self.last_language_info = info
        clip_lang = [f[0] for f in found]
        prev = self.tokenizer.encode(" " + initial_prompt.strip()) if initial_prompt else []
        prompts = [self._prompt(Session.DETECT if w else self._lang_token(l), task, without_timestamps, prev)[0]
                   for l, w in zip(clip_lang, late)]
        prompt, sot_index = self._prompt(self._lang_token(clip_lang[0]), task, without_timestamps, prev)
        n_new = min(max_new_tokens, self.dims.n_text_ctx - len(prompt))
        caps = None
        if row_max_new is not None:
            caps = [int(v) for v in row_max_new]
            if len(caps) != len(clips) or min(caps) < 1 or max(caps) > n_new:
                raise ValueError(f"row_max_new needs one budget in [1, {n_new}] per clip")
        eng.set_audio_ctx(0)
        opts = eng.gen_opts(n_new, timestamps=not without_timestamps, sot_index=sot_index)
        out: List[Optional[List[int]]] = [None] * len(clips)
        kw = dict(detect_language=True) if any(late) else {}   # armed only when a clip asks for it
        if session_prefill:
            kw["prefill"] = int(session_prefill)
        with (eng.session(opts, len(prompt), beam=beam, patience=patience, **kw) if beam > 1 else eng.session(opts, len(prompt), **kw)) as s:
            ids = s.submit([np.ascontiguousarray(c, dtype=np.float32) for c in clips], prompts, caps)
            where = {cid: i for i, cid in enumerate(ids)}

            def note_languages(got):
                for r in got:
                    if r.language is not None:
                        lang, prob, _ = self._session_language(r)
                        clip_lang[where[r.id]], info[where[r.id]] = lang, (lang, prob)
            if not word_timestamps:
                got = s.drain()
                note_languages(got)
                for r in got:
                    out[where[r.id]] = r.tokens
                return out  # type: ignore[return-value]
            s.hold()
            while s.pending > 0:
                got = s.poll()
                if not got:
                    raise RuntimeError(f"session idle with {s.pending} clips unfinished")
                note_languages(got)
                for lang in sorted({clip_lang[where[r.id]] for r in got}):   # one alignment pass per language of the poll
                    grp = [r for r in got if clip_lang[where[r.id]] == lang]
                    words = self._window_words(s, [r.id for r in grp], [r.tokens for r in grp],
                                               [len(clips[where[r.id]]) for r in grp], lang, self._lang_token(lang), task)
                    for r, w in zip(grp, words):
                        out[where[r.id]] = (r.tokens, w)
        return out  # type: ignore[return-value]

    def _window_words(self, aligner, refs: Sequence[int], tokens: Sequence[Sequence[int]], n_samples: Sequence[int],
                      language: str, lang_tok: int, task: str = "transcribe") -> List[List[dict]]:
        """Words of single-window results, one batched alignment pass (alignment.find_alignment_batch) for all of them:
        `aligner` is the engine (refs = clip indices of the resident pass) or a session in hold mode (refs = held clip ids).
        -> per clip [{word, start, end, probability}], seconds from the start of the clip."""
        st = self.special
        text = [[t for t in toks if t < st.eot] for toks in tokens]
        found = alignment.find_alignment_batch(aligner, self.tokenizer, st, list(refs), text, [n // 160 for n in n_samples],
                                               self.alignment_heads, language=language, lang_token=lang_tok,
                                               task_token=st.translate if task == "translate" else st.transcribe)
        out = []
        for toks, txt, al, n in zip(tokens, text, found, n_samples):
            # one segment over the window: add_word_timestamps clamps over-long words and merges punctuation as in transcribe()
            seg = dict(tokens=txt, start=0.0, end=self.window_text(toks, n)[1], eot=st.eot)
            alignment.add_word_timestamps([seg], al, 0.0)
            out.append([dict(word=w.word, start=w.start, end=w.end, probability=w.probability) for w in seg["words"]])
        return out

    def _pick_audio_ctx(self, audio_ctx: Union[None, int, str], longest_samples: int) -> int:
        full = self.dims.n_audio_ctx
        if audio_ctx is None:
            return full
        if audio_ctx == "auto":
            need = -(-longest_samples // 320) + 25
            return min(full, max(50, -(-need // 50) * 50))
        n = int(audio_ctx)
        if n < 4 or n > full or n % 2:
            raise ValueError(f"audio_ctx={audio_ctx!r}: need an even value in [4, {full}], 'auto' or None")
        return n

    def transcribe_windows(self, clips: Sequence[np.ndarray], language: Union[None, str, Sequence[Optional[str]]] = "zh",
                           beam_size: int = 5,
                           initial_prompt: Optional[str] = None, without_timestamps: bool = False,
                           max_new_tokens: int = 224, audio_ctx: Union[None, int, str] = None,
                           word_timestamps: bool = False) -> List[Tuple[str, float]]:
        """Batched single-window transcription for the streaming path: every clip (<= 30 s) is one row group of the
        same engine pass (beam_size rows per clip sharing its cross-KV).  Returns (text, end_time_seconds) per clip.

        audio_ctx (opt-in): encode only that many positions (20 ms each) instead of the 30-s window;
        "auto" = the longest clip of the pass + 0.5 s, rounded up to a multiple of 50.  None keeps Whisper's window.

        word_timestamps=True: (text, end_time_seconds, words) per clip, words = [{word, start, end, probability}] in seconds
        from the start of the clip; all clips of a pass are aligned in ONE device pass (Engine.align_batch) against the
        pass's encoder state, reduced audio_ctx included.  (transcribe() and transcribe_many() keep the one-window path.)

        language: one code, None (detect every clip) or one entry per clip (a code or None); None clips are detected from the
        pass's own encoder state (reduced audio_ctx included).  (language, probability) per clip of the last call:
        `last_language_info`."""
        eng = self.engine
        beam = max(1, min(beam_size, 7))
        per_pass = max(1, self.max_batch // beam)
        langs = self._check_languages(language, len(clips), "clip")
        info: List[Tuple[str, float]] = []
        prev = self.tokenizer.encode(" " + initial_prompt.strip()) if initial_prompt else []
        out: List[Tuple[str, float]] = []
        try:
            for i in range(0, len(clips), per_pass):
                chunk = [np.ascontiguousarray(c[: self.n_window], dtype=np.float32) for c in clips[i:i + per_pass]]
                eng.set_audio_ctx(self._pick_audio_ctx(audio_ctx, max(len(c) for c in chunk)))
                eng.log_mel(chunk, want_output=False)
                eng.encode(len(chunk))
                pass_lang = self._pass_languages(langs[i:i + per_pass], info)
                prompts = [self._prompt(self._lang_token(l), "transcribe", without_timestamps, prev)[0] for l in pass_lang]
                prompt, sot_index = self._prompt(self._lang_token(pass_lang[0]), "transcribe", without_timestamps, prev)
                opts = eng.gen_opts(min(max_new_tokens, self.dims.n_text_ctx - len(prompt)), timestamps=not without_timestamps,
                                    sot_index=sot_index)
                res = eng.generate_beam(prompts, beam, opts) if beam > 1 else eng.generate(prompts, opts)
                words: List = [None] * len(chunk)
                if word_timestamps:   # one alignment pass per language of the pass
                    for lang in sorted(set(pass_lang)):
                        ks = [k for k, l in enumerate(pass_lang) if l == lang]
                        for k, w in zip(ks, self._window_words(eng, ks, [res.tokens[k] for k in ks], [len(chunk[k]) for k in ks],
                                                               lang, self._lang_token(lang))):
                            words[k] = w
                for k, (c, toks) in enumerate(zip(chunk, res.tokens)):
                    out.append(self.window_text(toks, len(c)) + ((words[k],) if word_timestamps else ()))
            self.last_language_info = info
        finally:
            eng.set_audio_ctx(0)   # never leave a reduced window behind: the file-level paths assume the model's 30-s window
        return out

    def window_text(self, toks: Sequence[int], n_samples: int) -> Tuple[str, float]:
        """(text, end_time_seconds) of one window's tokens, as transcribe_windows returns them: the text of the tokens below
        EOT, the end at the last timestamp token or, without one, at the clip's length."""
        st = self.special
        toks = [t for t in toks if t != st.eot]
        ts = [t for t in toks if t >= st.timestamp_begin]
        end = (ts[-1] - st.timestamp_begin) * 0.02 if ts else n_samples / SAMPLE_RATE
        return self.tokenizer.decode([t for t in toks if t < st.eot]), float(end)
