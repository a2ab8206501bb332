"""Voice-activity pre-filter (`vad_filter=True` at every reference call site: asr_core.py:163, file_asr.py:284,461,
faster_whisper_asr.py:142) — SURVEY §8 row a4 / §8f N4.

faster-whisper runs the Silero VAD network (an ONNX file shipped inside the package) to get one speech probability
per 32-ms frame, turns the probabilities into speech chunks with Silero's published hysteresis rule, transcribes the
concatenation of the chunks, and maps every timestamp back to the original time line.  Neither the package nor the
network weights exist offline, so:

* everything AROUND the network is restated here — the chunking state machine (`get_speech_timestamps`),
  `collect_chunks`, and the time restoration (`SpeechTimestampsMap`, `restore_speech_timestamps`) — from the published
  algorithm, UNPINNED (no executable reference here; tested on hand-derived cases);
* the per-frame speech probability is pluggable: `speech_prob_fn(audio) -> float32[n_frames]` (e.g. an operator-supplied
  Silero ONNX session); the default `energy_speech_prob` is a plain short-time-energy detector and is NOT equivalent to
  Silero — `WhisperModel.transcribe` says so in a warning when it is used.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _lib, audio_io

SAMPLING_RATE = 16000
WINDOW = 512          # samples per probability frame (32 ms), Silero's frame at 16 kHz


@dataclass
class VadOptions:
    """faster-whisper's VadOptions defaults."""
    threshold: float = 0.5
    neg_threshold: Optional[float] = None
    min_speech_duration_ms: int = 0
    max_speech_duration_s: float = float("inf")
    min_silence_duration_ms: int = 2000
    speech_pad_ms: int = 400


# encoding name -> (TTASR_PCM_* code of include/ttasr.h, bytes per sample): the sample formats audio_io.read_audio_raw reports and
# the two G.711 laws.  IMA ADPCM is a block codec, not a stream.
WIRE_ENCODINGS = {name: (code, _lib.CODED_BYTES[code] if code in _lib.CODED_BYTES else _lib.PCM_BYTES[code]) for name, code in (
    ("u8", _lib.PCM_U8), ("s16", _lib.PCM_S16), ("s24", _lib.PCM_S24), ("s32", _lib.PCM_S32), ("f32", _lib.PCM_F32),
    ("f64", _lib.PCM_F64), ("alaw", _lib.PCM_ALAW), ("ulaw", _lib.PCM_ULAW))}


@dataclass(frozen=True)
class WireFormat:
    """What a live connection sends (the streaming server's `rate` / `channel` query parameters, the config message's sampleRate /
    channels): interleaved little-endian samples of `encoding` (WIRE_ENCODINGS) at `rate` Hz, `channels` (1 ... 8) per frame;
    audio_channel picks one of them in audio_io.parse_audio_channel's spellings (None / "mix" = their mean, "left", "right", an
    index)."""
    rate: int
    channels: int = 1
    encoding: str = "s16"
    audio_channel: object = None

    def __post_init__(self):
        if self.encoding not in WIRE_ENCODINGS:
            raise ValueError(f"encoding {self.encoding!r}: expected one of {sorted(WIRE_ENCODINGS)}")
        if isinstance(self.rate, bool) or int(self.rate) != self.rate or self.rate < 1:
            raise ValueError(f"rate {self.rate!r} must be a positive integer")
        if isinstance(self.channels, bool) or int(self.channels) != self.channels or not 1 <= self.channels <= 8:
            raise ValueError(f"channels {self.channels!r} outside 1 ... 8")
        if self.pick is not None and self.pick >= self.channels:
            raise ValueError(f"audio_channel {self.audio_channel!r} asked of {self.channels} channel{'s' if self.channels != 1 else ''}")

    @property
    def format(self) -> int:
        return WIRE_ENCODINGS[self.encoding][0]

    @property
    def frame_bytes(self) -> int:
        return WIRE_ENCODINGS[self.encoding][1] * int(self.channels)

    @property
    def pick(self) -> Optional[int]:
        return audio_io.parse_audio_channel(self.audio_channel)

    def wire_args(self):
        """(rate, channels, format, pick) of ttasr_vad_stream_open_wire."""
        return int(self.rate), int(self.channels), self.format, -1 if self.pick is None else self.pick

    def to_mono(self, raw) -> np.ndarray:
        """The whole frames of `raw` on the host -> float32 mono at `rate`: decode_audio's conversion (G.711 through its int16)."""
        raw = bytes(raw)
        x = audio_io.samples_to_float(raw[:len(raw) - len(raw) % self.frame_bytes], self.format, int(self.channels))
        return np.ascontiguousarray(audio_io.downmix(x, self.pick), dtype=np.float32)

    def to_16k(self, raw) -> np.ndarray:
        """`to_mono`, then the package's host resampler (audio_io.resample: scipy's resample_poly over the WHOLE buffer - run
        piece by piece it is not cut-invariant, which is what wire streams are for)."""
        return audio_io.resample(self.to_mono(raw), int(self.rate), SAMPLING_RATE)

    @staticmethod
    def of_client(client) -> "WireFormat":
        """The format a streaming client declares: client.sampling_rate and client.samples_width (bytes per sample), and the
        optional attributes client.channels, client.encoding and client.audio_channel.  Without an encoding the width decides -
        2 s16, 3 s24, 4 s32, 8 f64 - and width 1 is refused: u8, A-law and mu-law are all one byte."""
        width, enc = int(client.samples_width), getattr(client, "encoding", None)
        if enc is None:
            if width == 1:
                raise ValueError("samples_width 1 is ambiguous (u8, alaw, ulaw): the client must carry an encoding")
            enc = {2: "s16", 3: "s24", 4: "s32", 8: "f64"}.get(width)
            if enc is None:
                raise ValueError(f"samples_width {width} is no sample format")
        elif enc not in WIRE_ENCODINGS or WIRE_ENCODINGS[enc][1] != width:
            raise ValueError(f"encoding {enc!r} does not have samples_width {width}")
        return WireFormat(int(client.sampling_rate), int(getattr(client, "channels", 1) or 1), enc, getattr(client, "audio_channel", None))


def resolve_wire(wire, client=None) -> Optional[WireFormat]:
    """The `wire=` keyword of the streaming surfaces: None (16 kHz mono s16, as ever), a WireFormat, or "client" = what the client
    declares (WireFormat.of_client)."""
    if wire is None or isinstance(wire, WireFormat):
        return wire
    if wire == "client":
        if client is None:
            raise ValueError('wire="client" needs a client')
        return WireFormat.of_client(client)
    raise ValueError(f"wire {wire!r}: expected None, a WireFormat or 'client'")


def energy_speech_prob(audio: np.ndarray, window: int = WINDOW) -> np.ndarray:
    """Stand-in for the Silero network: logistic of the frame's RMS level over an adaptive noise floor
    (10th percentile of the frame levels, at least -60 dBFS).  6 dB above the floor -> 0.5."""
    n = int(np.ceil(len(audio) / window)) if len(audio) else 0
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    padded = np.zeros(n * window, dtype=np.float32)
    padded[: len(audio)] = audio
    rms = np.sqrt(np.mean(padded.reshape(n, window) ** 2, axis=1) + 1e-12)
    db = 20.0 * np.log10(rms)
    floor = max(float(np.percentile(db, 10)), -60.0)
    return (1.0 / (1.0 + np.exp(-(db - floor - 6.0) / 1.5))).astype(np.float32)


# The Silero-v5-shaped network (16 kHz branch) the engine runs on the device (include/ttasr.h ttasr_vad_*; DESIGN.md section
# 4.20): THE name / shape table of the Python side.  A leading "_model." of a state-dict key is stripped.  UNPINNED: the names and
# shapes are those of the published v5 TorchScript file as far as they are publicly described; no such file exists offline, so
# faithfulness to it is not checked anywhere - the network is held to the float64 restatement of tests/vad_reference.py.
SILERO_V5_TENSORS: Dict[str, tuple] = {
    "stft.forward_basis_buffer": (258, 1, 256),
    "encoder.0.reparam_conv.weight": (128, 129, 3), "encoder.0.reparam_conv.bias": (128,),
    "encoder.1.reparam_conv.weight": (64, 128, 3), "encoder.1.reparam_conv.bias": (64,),
    "encoder.2.reparam_conv.weight": (64, 64, 3), "encoder.2.reparam_conv.bias": (64,),
    "encoder.3.reparam_conv.weight": (128, 64, 3), "encoder.3.reparam_conv.bias": (128,),
    "decoder.rnn.weight_ih": (512, 128), "decoder.rnn.weight_hh": (512, 128),
    "decoder.rnn.bias_ih": (512,), "decoder.rnn.bias_hh": (512,),
    "decoder.decoder.2.weight": (1, 128, 1), "decoder.decoder.2.bias": (1,),
}
SYNTH_SILERO_SEED = 1   # the seed tests and tools use: on the suite's test signal its probabilities keep clear of both thresholds


def stft_basis() -> np.ndarray:
    """The Hann-windowed DFT basis of the network's STFT, float32 [258, 1, 256]: row b < 129 is cos(2 pi b m / 256) hann[m], row
    129 + b is -sin(2 pi b m / 256) hann[m] (periodic Hann), so S[b] + i S[129 + b] = rfft(frame * hann)[b]."""
    m = np.arange(256, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * m / 256.0)
    ang = 2.0 * np.pi * np.arange(129, dtype=np.float64)[:, None] * m[None, :] / 256.0
    return np.concatenate([np.cos(ang) * hann, -np.sin(ang) * hann])[:, None, :].astype(np.float32)


def synth_silero_weights(seed: int = SYNTH_SILERO_SEED) -> Dict[str, np.ndarray]:
    """Seeded synthetic weights in the shapes of SILERO_V5_TENSORS (float32): the STFT basis is the true Hann-windowed DFT basis,
    everything else is drawn - fan-in scaled, with an output head whose positive weights and negative bias put silence below
    and noise above 0.5.  Deterministic per seed.  NOT a voice-activity detector: a stand-in that exercises the network."""
    rng = np.random.default_rng([0x51E20, int(seed)])
    out: Dict[str, np.ndarray] = {}
    for name, shape in SILERO_V5_TENSORS.items():
        if name == "stft.forward_basis_buffer":
            w = stft_basis()
        elif name.endswith("reparam_conv.weight"):
            w = rng.standard_normal(shape) * (1.6 / np.sqrt(shape[1] * shape[2]))
        elif name.endswith("reparam_conv.bias"):
            w = rng.standard_normal(shape) * 0.05
        elif name in ("decoder.rnn.weight_ih", "decoder.rnn.weight_hh"):
            w = rng.standard_normal(shape) * (1.0 / np.sqrt(shape[1]))
        elif name in ("decoder.rnn.bias_ih", "decoder.rnn.bias_hh"):
            w = rng.standard_normal(shape) * 0.1
        elif name == "decoder.decoder.2.weight":
            w = np.abs(rng.standard_normal(shape)) * 0.6
        else:
            w = np.full(shape, -3.5)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def load_silero_state(path_or_mapping) -> Dict[str, np.ndarray]:
    """The VAD tensors of SILERO_V5_TENSORS as float32 arrays, from a mapping (state dict; torch tensors or arrays), an `.npz`
    file, or - when torch imports - a TorchScript module / state-dict file.  A leading "_model." is stripped; keys outside the
    table (the 8 kHz branch) are ignored; a missing tensor or a wrong shape raises ValueError."""
    src = path_or_mapping
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        path = os.fspath(src)
        if str(path).lower().endswith(".npz"):
            with np.load(path) as z:
                src = {k: z[k] for k in z.files}
        else:
            try:
                import torch
            except ImportError as e:
                raise RuntimeError(f"{path}: reading a TorchScript / state-dict file needs torch; convert it to .npz") from e
            try:
                src = torch.jit.load(path, map_location="cpu").state_dict()
            except Exception:
                src = torch.load(path, map_location="cpu", weights_only=True)
                if hasattr(src, "state_dict"):
                    src = src.state_dict()
    out: Dict[str, np.ndarray] = {}
    for key, value in dict(src).items():
        name = key[len("_model."):] if key.startswith("_model.") else key
        if name not in SILERO_V5_TENSORS:
            continue
        if hasattr(value, "detach"):
            value = value.detach().cpu().float().numpy()
        a = np.ascontiguousarray(value, dtype=np.float32)
        if a.shape != SILERO_V5_TENSORS[name]:
            raise ValueError(f"VAD tensor {name}: shape {a.shape}, expected {SILERO_V5_TENSORS[name]}")
        out[name] = a
    missing = [n for n in SILERO_V5_TENSORS if n not in out]
    if missing:
        raise ValueError(f"VAD state is missing {missing}")
    return out


# The PyanNet-shaped segmentation network the engine runs on the device (include/ttasr.h ttasr_seg_*):
# THE name / shape table of the Python side, "C" standing for the number of classes (1 ... 8, classifier.weight's first
# dimension).  UNPINNED against the published pyannote/segmentation checkpoint: the tensor names, the ParamSincFB filter formula
# (sinc_filters), the aggregation window and the Binarize rules (pyannote_speech_timestamps) are restated from memory - neither
# pyannote.audio nor the checkpoint exists offline - and the network is held to the float64 restatement of
# tests/pyannet_reference.py on synthetic weights.  "sincnet.conv1d.0.filters" is DERIVED: load_pyannet_state builds it from the
# checkpoint's sincnet.conv1d.0.filterbank.low_hz_ / band_hz_ [40, 1].
PYANNET_CHUNK, PYANNET_STEP, PYANNET_FRAMES = 80000, 8000, 293      # samples of a chunk, between chunk starts; frames of a chunk
PYANNET_FRAME_STEP, PYANNET_FRAME_CENTRE = 270, 495                 # frame j is centred on sample 495 + 270 j
PYANNET_MAX_CLASSES = 8
PYANNET_CUTOFFS = ("sincnet.conv1d.0.filterbank.low_hz_", "sincnet.conv1d.0.filterbank.band_hz_")


def _pyannet_table() -> Dict[str, tuple]:
    t: Dict[str, tuple] = {"sincnet.wav_norm1d.weight": (1,), "sincnet.wav_norm1d.bias": (1,),
                           "sincnet.conv1d.0.filters": (80, 1, 251)}
    for i, ch in enumerate((80, 60, 60)):
        t[f"sincnet.norm1d.{i}.weight"] = (ch,)
        t[f"sincnet.norm1d.{i}.bias"] = (ch,)
    t["sincnet.conv1d.1.weight"], t["sincnet.conv1d.1.bias"] = (60, 80, 5), (60,)
    t["sincnet.conv1d.2.weight"], t["sincnet.conv1d.2.bias"] = (60, 60, 5), (60,)
    for layer in range(4):
        for sfx in (f"_l{layer}", f"_l{layer}_reverse"):
            t["lstm.weight_ih" + sfx] = (512, 60 if layer == 0 else 256)
            t["lstm.weight_hh" + sfx] = (512, 128)
            t["lstm.bias_ih" + sfx] = (512,)
            t["lstm.bias_hh" + sfx] = (512,)
    t["linear.0.weight"], t["linear.0.bias"] = (128, 256), (128,)
    t["linear.1.weight"], t["linear.1.bias"] = (128, 128), (128,)
    t["classifier.weight"], t["classifier.bias"] = ("C", 128), ("C",)
    return t


PYANNET_TENSORS: Dict[str, tuple] = _pyannet_table()   # 51 tensors
# the seed tests and tools use, with the classifier's gain and bias: on the suite's test signal the float64 reference's aggregated
# score goes below 0.35 and above 0.65 and Binarize finds at least 3 segments
SYNTH_PYANNET_SEED, SYNTH_PYANNET_GAIN, SYNTH_PYANNET_BIAS = 0, 4.0, -1.0


def sinc_filters(low_hz_, band_hz_, sample_rate: int = SAMPLING_RATE) -> np.ndarray:
    """The materialised sinc filterbank, float32 [80, 1, 251], from the 40 learnable cutoff pairs - ParamSincFB's formula, restated
    from memory (UNPINNED), in float64: low = 50 + |low_hz_|, high = clip(low + 50 + |band_hz_|, 50, sr / 2), band = high - low;
    with n = 2 pi m / sr for m = -125 ... -1 and win = the first 125 points of the 251-point periodic Hamming window
    0.54 - 0.46 cos(2 pi i / 251):  cosine filter = [L | 2 band | reversed L], L = (sin(high n) - sin(low n)) / (n / 2) * win;
    sine filter = [L | 0 | -reversed L], L = (cos(low n) - cos(high n)) / (n / 2) * win; each divided by 2 band; the 40 cosine
    filters first, then the 40 sine filters."""
    low_p = np.asarray(low_hz_, dtype=np.float64).reshape(-1)
    band_p = np.asarray(band_hz_, dtype=np.float64).reshape(-1)
    if low_p.shape != (40,) or band_p.shape != (40,):
        raise ValueError(f"sinc cutoffs: {low_p.size} low and {band_p.size} band values, expected 40 of each")
    low = 50.0 + np.abs(low_p)
    high = np.clip(low + 50.0 + np.abs(band_p), 50.0, sample_rate / 2.0)
    band = high - low
    n = 2.0 * np.pi * np.arange(-125, 0, dtype=np.float64) / sample_rate
    win = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(125, dtype=np.float64) / 251.0)
    fl, fh = low[:, None] * n[None, :], high[:, None] * n[None, :]
    cos_left = (np.sin(fh) - np.sin(fl)) / (n / 2.0) * win
    sin_left = (np.cos(fl) - np.cos(fh)) / (n / 2.0) * win
    cos_f = np.concatenate([cos_left, 2.0 * band[:, None], cos_left[:, ::-1]], axis=1)
    sin_f = np.concatenate([sin_left, np.zeros((40, 1)), -sin_left[:, ::-1]], axis=1)
    filters = np.concatenate([cos_f, sin_f]) / (2.0 * np.concatenate([band, band])[:, None])
    return np.ascontiguousarray(filters[:, None, :], dtype=np.float32)


def mel_cutoffs(sample_rate: int = SAMPLING_RATE):
    """(low_hz_, band_hz_) [40, 1] of a freshly initialised filterbank: 41 points equally spaced on the mel scale from 30 Hz to
    sr / 2 - 100 Hz; low = the first 40, band = their differences."""
    to_mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)   # noqa: E731
    hz = 700.0 * (10.0 ** (np.linspace(to_mel(30.0), to_mel(sample_rate / 2.0 - 100.0), 41) / 2595.0) - 1.0)
    return hz[:-1, None].astype(np.float32), np.diff(hz)[:, None].astype(np.float32)


def synth_pyannet_weights(seed: int = SYNTH_PYANNET_SEED, classes: int = 3) -> Dict[str, np.ndarray]:
    """Seeded synthetic weights in the shapes of PYANNET_TENSORS (float32): the filters are sinc_filters of the mel-spaced initial
    cutoffs, every matrix is drawn N(0, 1.5 / sqrt(fan_in)), the norms' weights around 1, the biases small, and the classifier
    carries SYNTH_PYANNET_GAIN and SYNTH_PYANNET_BIAS so that the scores move across 0.5.  Deterministic per (seed, classes).
    NOT a voice-activity detector: a stand-in that exercises the network."""
    if not 1 <= int(classes) <= PYANNET_MAX_CLASSES:
        raise ValueError(f"classes {classes} outside 1 ... {PYANNET_MAX_CLASSES}")
    rng = np.random.default_rng([0x9A22E7, int(seed)])
    out: Dict[str, np.ndarray] = {}
    for name, shape in PYANNET_TENSORS.items():
        shape = tuple(int(classes) if d == "C" else d for d in shape)
        if name == "sincnet.conv1d.0.filters":
            w = sinc_filters(*mel_cutoffs())
        elif "norm1d" in name:
            w = (1.0 + 0.1 * rng.standard_normal(shape)) if name.endswith("weight") else 0.1 * rng.standard_normal(shape)
        elif name == "classifier.weight":
            w = rng.standard_normal(shape) * (SYNTH_PYANNET_GAIN * 1.5 / np.sqrt(shape[1]))
        elif name == "classifier.bias":
            w = np.full(shape, SYNTH_PYANNET_BIAS)
        elif name.endswith("weight") or "weight_" in name:
            w = rng.standard_normal(shape) * (1.5 / np.sqrt(np.prod(shape[1:])))
        else:
            w = rng.standard_normal(shape) * 0.05
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def load_pyannet_state(path_or_mapping) -> Dict[str, np.ndarray]:
    """The tensors of PYANNET_TENSORS as float32 arrays, from a mapping (state dict; torch tensors or arrays), an `.npz` file, or -
    when torch imports - a torch file, with an optional "state_dict" level (a Lightning checkpoint).  The filters come from
    "sincnet.conv1d.0.filters" when the source has it, else from the cutoffs PYANNET_CUTOFFS through sinc_filters.  Keys outside
    the table are ignored; a missing tensor or a wrong shape raises ValueError."""
    src = path_or_mapping
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        path = os.fspath(src)
        if str(path).lower().endswith(".npz"):
            with np.load(path) as z:
                src = {k: z[k] for k in z.files}
        else:
            try:
                import torch
            except ImportError as e:
                raise RuntimeError(f"{path}: reading a torch checkpoint needs torch; convert it to .npz") from e
            src = torch.load(path, map_location="cpu", weights_only=True)
    src = dict(src)
    if "state_dict" in src and hasattr(src["state_dict"], "items"):
        src = dict(src["state_dict"])
    to_np = lambda v: np.asarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else v)   # noqa: E731
    out: Dict[str, np.ndarray] = {}
    if "sincnet.conv1d.0.filters" not in src and all(k in src for k in PYANNET_CUTOFFS):
        out["sincnet.conv1d.0.filters"] = sinc_filters(*(to_np(src[k]) for k in PYANNET_CUTOFFS))
    classes = None
    for name, shape in PYANNET_TENSORS.items():
        if name not in src:
            continue
        a = np.ascontiguousarray(to_np(src[name]), dtype=np.float32)
        if "C" in shape:
            if a.ndim != len(shape) or not 1 <= a.shape[0] <= PYANNET_MAX_CLASSES or (classes is not None and a.shape[0] != classes):
                raise ValueError(f"segmentation tensor {name}: shape {a.shape}, expected {shape} with one C in 1 ... {PYANNET_MAX_CLASSES}")
            classes = a.shape[0]
            shape = tuple(classes if d == "C" else d for d in shape)
        if a.shape != shape:
            raise ValueError(f"segmentation tensor {name}: shape {a.shape}, expected {shape}")
        out[name] = a
    missing = [n for n in PYANNET_TENSORS if n not in out]
    if missing:
        raise ValueError(f"segmentation state is missing {missing}")
    return {n: out[n] for n in PYANNET_TENSORS}


def pyannote_speech_timestamps(n_samples: int, scores, onset: float = 0.5, offset: float = 0.5, min_duration_on: float = 0.3,
                               min_duration_off: float = 0.3, pad_onset: float = 0.0, pad_offset: float = 0.0,
                               sampling_rate: int = SAMPLING_RATE) -> List[Dict[str, int]]:
    """pyannote's Binarize over a recording's aggregated scores (Engine.segmentation_scores), restated (UNPINNED) ->
    [{'start': sample, 'end': sample}], the chunk-list format of get_speech_timestamps.  Frame j stands at
    t_j = (495 + 270 j) / 16 000 s.  Hysteresis: a segment opens at the frame whose score goes above `onset` (at frame 0 when
    the first score is above it) and closes at the frame whose score goes below `offset`; a segment still open ends at the last
    frame.  Then the pads are applied (start - pad_onset, end + pad_offset), segments whose gap is <= min_duration_off are merged,
    segments shorter than min_duration_on are dropped, and the rest is clipped to [0, n_samples]."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    at = lambda j: (PYANNET_FRAME_CENTRE + PYANNET_FRAME_STEP * j) / float(sampling_rate)   # noqa: E731
    segs: List[List[float]] = []
    if len(scores):
        active, start = bool(scores[0] > onset), at(0)
        for j in range(1, len(scores)):
            if active and scores[j] < offset:
                segs.append([start - pad_onset, at(j) + pad_offset])
                active = False
            elif not active and scores[j] > onset:
                start, active = at(j), True
        if active:
            segs.append([start - pad_onset, at(len(scores) - 1) + pad_offset])
    merged: List[List[float]] = []
    for s in segs:
        if merged and s[0] - merged[-1][1] <= min_duration_off:
            merged[-1][1] = max(merged[-1][1], s[1])
        else:
            merged.append(list(s))
    out = []
    for a, b in merged:
        if b - a < min_duration_on:
            continue
        a, b = max(int(round(a * sampling_rate)), 0), min(int(round(b * sampling_rate)), int(n_samples))
        if b > a:
            out.append({"start": a, "end": b})
    return out


def silero_speech_prob_fn(step: Callable[[np.ndarray, np.ndarray], "tuple[float, np.ndarray]"], context: int = 64,
                          state_shape: Sequence[int] = (2, 1, 128)) -> Callable[[np.ndarray], np.ndarray]:
    """Adapter for an operator-supplied Silero VAD network (the ONNX file faster-whisper ships; not available offline):
    `step(frame, state) -> (speech_probability, new_state)` is ONE forward of the network, e.g.
        lambda x, h: (lambda o: (float(o[0].squeeze()), o[1]))(session.run(None, {"input": x, "state": h, "sr": np.array(16000)}))
    and the returned function is what `WhisperModel.vad_speech_prob_fn` / `vad_speech_prob_fn=` expect.  It drives the
    network the way Silero's v5 graph is specified: 512-sample frames (32 ms), each prefixed with the last `context` = 64
    samples of the previous frame (zeros before the first), float32 [1, 576]; the recurrent state ([2, 1, 128], zeros at
    the start of a recording) is threaded from call to call; the last frame is zero-padded."""
    def fn(audio: np.ndarray) -> np.ndarray:
        audio = np.asarray(audio, dtype=np.float32)
        n = int(np.ceil(len(audio) / WINDOW)) if len(audio) else 0
        padded = np.zeros(n * WINDOW, dtype=np.float32)
        padded[: len(audio)] = audio
        state = np.zeros(tuple(state_shape), dtype=np.float32)
        ctx = np.zeros(context, dtype=np.float32)
        out = np.zeros(n, dtype=np.float32)
        for i in range(n):
            frame = padded[i * WINDOW:(i + 1) * WINDOW]
            p, state = step(np.concatenate([ctx, frame])[None, :], state)
            out[i] = float(p)
            ctx = frame[-context:] if context else ctx
        return out
    return fn


def get_speech_timestamps(audio: np.ndarray, options: Optional[VadOptions] = None,
                          speech_prob_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                          sampling_rate: int = SAMPLING_RATE) -> List[Dict[str, int]]:
    """Speech chunks [{'start': sample, 'end': sample}] by Silero's rule: a chunk opens at the first frame with
    p >= threshold, closes once p stayed below neg_threshold (threshold - 0.15) for min_silence_duration_ms, is
    dropped if shorter than min_speech_duration_ms, is cut at the last >= 98 ms pause when it exceeds
    max_speech_duration_s, and is finally padded by speech_pad_ms (gaps shorter than two pads are split in half)."""
    o = options or VadOptions()
    probs = np.asarray((speech_prob_fn or energy_speech_prob)(audio), dtype=np.float32)
    n_audio = len(audio)
    neg = o.neg_threshold if o.neg_threshold is not None else max(o.threshold - 0.15, 0.01)
    min_speech = sampling_rate * o.min_speech_duration_ms / 1000
    pad = int(sampling_rate * o.speech_pad_ms / 1000)
    max_speech = sampling_rate * o.max_speech_duration_s - WINDOW - 2 * pad
    min_silence = sampling_rate * o.min_silence_duration_ms / 1000
    min_silence_at_max = sampling_rate * 98 / 1000
    speeches: List[Dict[str, int]] = []
    cur: Dict[str, int] = {}
    triggered = False
    temp_end = prev_end = next_start = 0
    for i, p in enumerate(probs):
        at = WINDOW * i
        if p >= o.threshold and temp_end:
            temp_end = 0
            if next_start < prev_end:
                next_start = at
        if p >= o.threshold and not triggered:
            triggered = True
            cur["start"] = at
            continue
        if triggered and at - cur["start"] > max_speech:
            if prev_end:
                cur["end"] = prev_end
                speeches.append(cur)
                cur = {}
                if next_start < prev_end:
                    triggered = False
                else:
                    cur["start"] = next_start
                prev_end = next_start = temp_end = 0
            else:
                cur["end"] = at
                speeches.append(cur)
                cur = {}
                prev_end = next_start = temp_end = 0
                triggered = False
                continue
        if p < neg and triggered:
            if not temp_end:
                temp_end = at
            if at - temp_end > min_silence_at_max:
                prev_end = temp_end
            if at - temp_end < min_silence:
                continue
            cur["end"] = temp_end
            if cur["end"] - cur["start"] > min_speech:
                speeches.append(cur)
            cur = {}
            prev_end = next_start = temp_end = 0
            triggered = False
    if cur and n_audio - cur["start"] > min_speech:
        cur["end"] = n_audio
        speeches.append(cur)
    for i, sp in enumerate(speeches):
        if i == 0:
            sp["start"] = int(max(0, sp["start"] - pad))
        if i != len(speeches) - 1:
            gap = speeches[i + 1]["start"] - sp["end"]
            if gap < 2 * pad:
                sp["end"] += int(gap // 2)
                speeches[i + 1]["start"] = int(max(0, speeches[i + 1]["start"] - gap // 2))
            else:
                sp["end"] = int(min(n_audio, sp["end"] + pad))
                speeches[i + 1]["start"] = int(max(0, speeches[i + 1]["start"] - pad))
        else:
            sp["end"] = int(min(n_audio, sp["end"] + pad))
    return speeches


class StreamingSpeechDetector:
    """Speech chunks of ONE recording that arrives in pieces, on a device stream (Engine.vad_stream_*): holds the stream id and
    the probabilities so far, so every `feed` costs only the frames its samples complete - the network never runs over the same
    audio twice, and its state stays on the device between calls.

    The trailing partial frame is NOT evaluated until it fills: `segments` is `get_speech_timestamps` over the audio cut to whole
    512-sample frames.  That is the one deliberate difference from running the offline VAD over the whole buffer (which
    zero-pads the last frame); the part left out is never more than 32 ms, well under the 100 ms the streaming trigger allows
    behind the last segment."""

    def __init__(self, engine, stream_id: Optional[int] = None, wire: Optional[WireFormat] = None):
        """wire=WireFormat(...): a WIRE stream - `feed_bytes` takes the connection's bytes in that format, however they are cut,
        the device converts, downmixes and resamples them in front of the network, and `audio` is the 16 kHz float32 so far
        (bit for bit Engine.ingest of the bytes fed, up to the samples whose inputs have not all arrived).  `segments` stays in
        16 kHz samples."""
        self.engine = engine
        self.wire = wire
        if stream_id is None:
            stream_id = engine.vad_stream_open() if wire is None else engine.vad_stream_open(wire=wire)
        self.stream_id = int(stream_id)
        self.n_samples = 0
        self._probs: List[np.ndarray] = []
        self._audio: List[np.ndarray] = []

    @property
    def probs(self) -> np.ndarray:
        if len(self._probs) != 1:
            self._probs = [np.concatenate(self._probs) if self._probs else np.zeros(0, dtype=np.float32)]
        return self._probs[0]

    def feed(self, samples: np.ndarray) -> None:
        """Append float32 PCM (16 kHz) and evaluate the frames it completes."""
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        self.extend(len(samples), self.engine.vad_stream_push([self.stream_id], [samples])[0])

    @property
    def audio(self) -> np.ndarray:
        """A wire stream's 16 kHz float32 samples so far (empty for a float stream: its caller has them)."""
        if len(self._audio) != 1:
            self._audio = [np.concatenate(self._audio) if self._audio else np.zeros(0, dtype=np.float32)]
        return self._audio[0]

    def feed_bytes(self, raw, finish: bool = False) -> None:
        """Append bytes in the stream's wire format (any length: a piece may end inside a sample).  finish=True also releases the
        samples that wait for inputs behind the end, evaluates the zero-padded last frame and leaves the device stream as reset."""
        if self.wire is None:
            raise ValueError("feed_bytes is for a detector opened with wire=")
        pcm, probs = self.engine.vad_stream_push_wire([self.stream_id], [raw], finish=[bool(finish)])
        self.extend(len(pcm[0]), probs[0], pcm[0])

    def extend(self, n_samples: int, probs: np.ndarray, pcm: Optional[np.ndarray] = None) -> None:
        """Book what a push made elsewhere returned for this stream (a backend that pushes many streams in one call); pcm: the
        16 kHz samples a wire push returned."""
        self.n_samples += int(n_samples)
        if len(probs):
            self._probs.append(np.asarray(probs, dtype=np.float32))
        if pcm is not None and len(pcm):
            self._audio.append(np.asarray(pcm, dtype=np.float32))

    def segments(self, options: Optional[VadOptions] = None) -> List[Dict[str, int]]:
        """[{'start': sample, 'end': sample}] of the audio fed so far, cut to whole frames."""
        probs = self.probs
        cut = np.broadcast_to(np.float32(0), (len(probs) * WINDOW,))   # get_speech_timestamps reads its length only
        return get_speech_timestamps(cut, options, lambda _a: probs)

    def reset(self) -> None:
        self.engine.vad_stream_reset(self.stream_id)
        self.clear()

    def clear(self) -> None:
        """Forget the bookkeeping only (the stream itself was reset elsewhere)."""
        self.n_samples = 0
        self._probs = []
        self._audio = []

    def close(self) -> None:
        if self.stream_id is not None:
            self.engine.vad_stream_close(self.stream_id)
            self.stream_id = None


def collect_chunks(audio: np.ndarray, chunks: Sequence[Dict[str, int]]) -> np.ndarray:
    if not chunks:
        return np.zeros(0, dtype=np.float32)
    return np.concatenate([audio[c["start"]: c["end"]] for c in chunks]).astype(np.float32, copy=False)


def merge_chunks(chunks: Sequence[Dict[str, int]], max_samples: int) -> List[Dict]:
    """Packs speech chunks greedily into groups of at most max_samples (faster-whisper's merge_segments for its batched
    pipeline; UNPINNED like the rest of this module): a chunk joins the open group while chunk.end - group.start <= max_samples,
    otherwise it opens the next group; a chunk longer than max_samples is first cut into pieces of max_samples.
    -> [{'start', 'end', 'segments': [{'start', 'end'}, ...]}] in chunk order; a group's audio is the concatenation of its
    segments (collect_chunks), at most end - start <= max_samples samples, and its time line a SpeechTimestampsMap over them."""
    max_samples = int(max_samples)
    if max_samples < 1:
        raise ValueError(f"max_samples {max_samples} must be >= 1")
    pieces: List[Dict[str, int]] = []
    for c in chunks:
        a, b = int(c["start"]), int(c["end"])
        while b - a > max_samples:
            pieces.append(dict(start=a, end=a + max_samples))
            a += max_samples
        if b > a:
            pieces.append(dict(start=a, end=b))
    groups: List[Dict] = []
    for c in pieces:
        if groups and c["end"] - groups[-1]["start"] <= max_samples:
            groups[-1]["end"] = c["end"]
            groups[-1]["segments"].append(c)
        else:
            groups.append(dict(start=c["start"], end=c["end"], segments=[c]))
    return groups


class SpeechTimestampsMap:
    """Maps a time on the concatenated-speech axis back to the original recording."""

    def __init__(self, chunks: Sequence[Dict[str, int]], sampling_rate: int = SAMPLING_RATE, time_precision: int = 2):
        self.sampling_rate = sampling_rate
        self.time_precision = time_precision
        self.chunk_end_sample: List[int] = []
        self.total_silence_before: List[float] = []
        previous_end = 0
        silent = 0
        for c in chunks:
            silent += c["start"] - previous_end
            previous_end = c["end"]
            self.chunk_end_sample.append(c["end"] - silent)
            self.total_silence_before.append(silent / sampling_rate)

    def get_chunk_index(self, time: float) -> int:
        sample = int(time * self.sampling_rate)
        idx = int(np.searchsorted(self.chunk_end_sample, sample, side="right"))
        return min(idx, len(self.chunk_end_sample) - 1)

    def get_original_time(self, time: float, chunk_index: Optional[int] = None) -> float:
        if not self.chunk_end_sample:
            return round(time, self.time_precision)
        if chunk_index is None:
            chunk_index = self.get_chunk_index(time)
        return round(self.total_silence_before[chunk_index] + time, self.time_precision)


def restore_speech_timestamps(segments, chunks: Sequence[Dict[str, int]], sampling_rate: int = SAMPLING_RATE):
    """Generator over segment-like objects with `_replace` (NamedTuple): start/end (and word times) moved back to the
    original time line.  Words are mapped individually: each word goes with the chunk its MIDDLE falls in, so a word
    is never stretched across a removed pause."""
    ts_map = SpeechTimestampsMap(chunks, sampling_rate)
    for seg in segments:
        if getattr(seg, "words", None):
            words = []
            for w in seg.words:
                idx = ts_map.get_chunk_index((w.start + w.end) / 2)
                words.append(type(w)(start=ts_map.get_original_time(w.start, idx), end=ts_map.get_original_time(w.end, idx),
                                     word=w.word, probability=w.probability))
            yield seg._replace(start=words[0].start, end=words[-1].end, words=words)
        else:
            yield seg._replace(start=ts_map.get_original_time(seg.start), end=ts_map.get_original_time(seg.end))
