"""Thin Python owner of one libttasr context (one GPU, one stream).  numpy in / numpy out; every compute
method is a single C-ABI call into the HIP library."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, NON_SPEECH_TOKENS_MULTI, SpecialTokens, WhisperDims


class TtasrError(RuntimeError):
    pass


@dataclass
class DeviceTensor:
    """A tensor in device memory of the engine's GPU: address, TTASR_DTYPE_* (0 float32, 1 bfloat16 bits, 2 float16 bits), shape."""
    ptr: int
    dtype: int
    shape: Tuple[int, ...]


@dataclass
class GenResult:
    tokens: List[List[int]]
    sum_logprob: np.ndarray
    no_speech_prob: np.ndarray


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def default_suppress(st: SpecialTokens, vocab: int) -> List[int]:
    """suppress_tokens=[-1] of faster-whisper (get_suppressed_tokens): the non-speech symbols plus <|transcribe|>,
    <|translate|>, <|startoftranscript|>, <|startofprev|>, <|startoflm|>; <|nospeech|> is masked as well, as in the
    generation_config.json of the released checkpoints and openai-whisper (its probability is read from the raw logits
    before the mask, and it is never a legitimate output)."""
    ids = [t for t in NON_SPEECH_TOKENS_MULTI if t < min(vocab, st.eot)]
    ids += [st.translate, st.transcribe, st.sot, st.sot_prev, st.no_speech]
    if st.sot_lm >= 0:
        ids.append(st.sot_lm)
    return sorted(set(ids))


class Engine:
    # capability: this engine's sessions can hold finished clips (Session.hold / align / retry / release) and align them with the
    # packed, pass-mate-independent pass (option "align_packed"); what transcribe_many(continuous=True, word_timestamps=True) needs
    session_hold = True

    def __init__(self, dims: WhisperDims, compute_type: int = COMPUTE_BF16, max_batch: int = 1, device: int = 0,
                 share_weights_with: Optional["Engine"] = None):
        """share_weights_with: another Engine on the same GPU whose (finalized) device weights this one reads instead of loading
        its own copy (ttasr_create_shared): a second context for keeping two batches in flight costs workspaces only."""
        self.lib = _lib.load()
        self.dims = dims
        self.compute_type = compute_type
        self.max_batch = max_batch
        self.device = device
        h = C.c_void_p()
        if share_weights_with is not None:
            o = share_weights_with
            if o.dims != dims or o.compute_type != compute_type or o.device != device:
                raise ValueError("a weight-sharing engine must have its owner's geometry, compute type and device")
            rc = self.lib.ttasr_create_shared(o.h, max_batch, C.byref(h))
            what = "ttasr_create_shared"
        else:
            cfg = _lib.Config(dims.n_mels, dims.n_audio_ctx, dims.d_model, dims.n_heads, dims.ffn_dim, dims.enc_layers,
                              dims.dec_layers, dims.vocab, dims.n_text_ctx, compute_type, max_batch, 0)
            rc = self.lib.ttasr_create(C.byref(cfg), device, C.byref(h))
            what = "ttasr_create"
        if rc != 0:
            raise TtasrError(f"{what} failed ({rc}): {self.lib.ttasr_last_error(None).decode()}")
        self.h = h
        self.shares_weights = share_weights_with is not None
        self.special = SpecialTokens.for_vocab(dims.vocab)
        self.audio_ctx = dims.n_audio_ctx
        self.has_vad = False   # load_vad() has put the VAD network on this context
        self.has_segmentation = False   # load_segmentation() has put the segmentation network on this context
        self.seg_classes = 0
        self.has_speaker_embedding = False   # load_speaker_embedding() has put the speaker-embedding network on this context
        self.spk_dim = 0
        self._wire_streams = {}   # wire stream id -> (rate, bytes per frame, samples a finish releases): sizes vad_stream_push_wire's result rows

    # -- plumbing ------------------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise TtasrError(f"{what} failed ({rc}): {self.lib.ttasr_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.ttasr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -------------------------------------------------------------------------------
    def load_weights(self, tensors: Iterable[Tuple[str, "np.ndarray | DeviceTensor"]]):
        """(name, float32 host array) pairs, or (name, DeviceTensor) for tensors already resident in this GPU's memory
        (the multi-GPU start-up: dist.broadcast_weights hands over the RCCL buckets without a host round trip)."""
        for name, arr in tensors:
            if isinstance(arr, DeviceTensor):
                dims = (C.c_int64 * len(arr.shape))(*arr.shape)
                self._check(self.lib.ttasr_load_tensor_device(self.h, name.encode(), C.c_void_p(arr.ptr), arr.dtype, dims,
                                                              len(arr.shape)), f"load_tensor_device({name})")
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.ttasr_load_tensor(self.h, name.encode(), _ptr(a), dims, a.ndim), f"load_tensor({name})")
        self._check(self.lib.ttasr_finalize_weights(self.h), "finalize_weights")

    # -- voice activity detection ----------------------------------------------------------------
    def load_vad(self, mapping):
        """The Silero-v5-shaped VAD network of this context (ttasr_vad_load_tensor + ttasr_vad_finalize): a mapping, or
        (name, array) pairs, with the names and shapes of vad.SILERO_V5_TENSORS (a leading "_model." is stripped).  Every context
        holds its own copy, weight-sharing contexts included."""
        items = mapping.items() if hasattr(mapping, "items") else mapping
        for name, arr in items:
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self.lib.ttasr_vad_load_tensor(self.h, str(name).encode(), _ptr(a), dims, a.ndim), f"vad_load_tensor({name})")
        self._check(self.lib.ttasr_vad_finalize(self.h), "vad_finalize")
        self.has_vad = True

    def vad_probs(self, audios: Sequence[np.ndarray], return_logits: bool = False):
        """Speech probability per 512-sample frame of every recording (ttasr_vad_probs): a list of float32 arrays of
        ceil(len / 512) entries; return_logits=True: (probabilities, pre-sigmoid logits).  More recordings than max_batch go
        through several calls; a recording's values do not depend on its neighbours, so the split is not observable."""
        pcm = []
        for i, a in enumerate(audios):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"recording {i}: PCM must be one-dimensional, got shape {a.shape}")
            pcm.append(a)
        probs = [np.zeros(-(-len(a) // 512), dtype=np.float32) for a in pcm]
        logits = [np.zeros_like(p) for p in probs] if return_logits else None
        for i0 in range(0, len(pcm), self.max_batch):
            sl = slice(i0, i0 + self.max_batch)
            n = len(pcm[sl])
            ptrs = (C.c_void_p * n)(*[a.ctypes.data if len(a) else None for a in pcm[sl]])
            outs = (C.c_void_p * n)(*[p.ctypes.data if len(p) else None for p in probs[sl]])
            louts = (C.c_void_p * n)(*[p.ctypes.data if len(p) else None for p in logits[sl]]) if return_logits else None
            ns = np.asarray([len(a) for a in pcm[sl]], dtype=np.int64)
            self._check(self.lib.ttasr_vad_probs(self.h, n, ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), outs, louts), "vad_probs")
        return (probs, logits) if return_logits else probs

    # -- segmentation VAD (the PyanNet-shaped network) ---------------------------------------------
    def load_segmentation(self, weights):
        """The PyanNet-shaped segmentation network of this context (ttasr_seg_load_tensor + ttasr_seg_finalize): a mapping, or
        (name, array) pairs, with the names and shapes of vad.PYANNET_TENSORS (vad.load_pyannet_state builds the sinc filters
        from a checkpoint's cutoffs).  Every context holds its own copy."""
        items = weights.items() if hasattr(weights, "items") else weights
        for name, arr in items:
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self.lib.ttasr_seg_load_tensor(self.h, str(name).encode(), _ptr(a), dims, a.ndim), f"seg_load_tensor({name})")
        self._check(self.lib.ttasr_seg_finalize(self.h), "seg_finalize")
        self.seg_classes = int(self.lib.ttasr_seg_classes(self.h))
        self.has_segmentation = True

    def segmentation_scores(self, audios: Sequence[np.ndarray], return_chunks: bool = False):
        """The aggregated speech score per 270-sample frame of every recording (ttasr_seg_scores): a list of float32 arrays of
        ttasr_seg_frames(len) entries.  return_chunks=True: (scores, probabilities, logits), the last two per recording as
        float32 [chunks, 293, classes] - what every 80 000-sample chunk gave before the overlap-add.  More recordings than
        max_batch go through several calls; a recording's values do not depend on its neighbours."""
        if not getattr(self, "has_segmentation", False):
            raise TtasrError("no segmentation network on this engine: load_segmentation first")
        pcm = []
        for i, a in enumerate(audios):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"recording {i}: PCM must be one-dimensional, got shape {a.shape}")
            pcm.append(a)
        ncls = self.seg_classes
        scores = [np.zeros(self.lib.ttasr_seg_frames(len(a)), dtype=np.float32) for a in pcm]
        shapes = [(self.lib.ttasr_seg_chunks(len(a)), _lib.SEG_CHUNK_FRAMES, ncls) for a in pcm]
        probs = [np.zeros(s, dtype=np.float32) for s in shapes] if return_chunks else None
        logits = [np.zeros(s, dtype=np.float32) for s in shapes] if return_chunks else None
        rows = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data if a.size else None for a in arrs])   # noqa: E731
        for i0 in range(0, len(pcm), self.max_batch):
            sl = slice(i0, i0 + self.max_batch)
            ns = np.asarray([len(a) for a in pcm[sl]], dtype=np.int64)
            self._check(self.lib.ttasr_seg_scores(self.h, len(ns), rows(pcm[sl]), ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  rows(scores[sl]), rows(probs[sl]) if return_chunks else None,
                                                  rows(logits[sl]) if return_chunks else None), "seg_scores")
        return (scores, probs, logits) if return_chunks else scores

    # -- speaker embeddings (the XVectorSincNet-shaped network) --------------------------------------
    def load_speaker_embedding(self, weights):
        """The XVectorSincNet-shaped speaker-embedding network of this context (ttasr_spk_load_tensor + ttasr_spk_finalize): a
        mapping, or (name, array) pairs, with the names and shapes of diarization.XVECTOR_TENSORS
        (diarization.load_xvector_state builds the sinc filters from a checkpoint's cutoffs).  Every context holds its own copy."""
        items = weights.items() if hasattr(weights, "items") else weights
        for name, arr in items:
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self.lib.ttasr_spk_load_tensor(self.h, str(name).encode(), _ptr(a), dims, a.ndim), f"spk_load_tensor({name})")
        self._check(self.lib.ttasr_spk_finalize(self.h), "spk_finalize")
        self.spk_dim = int(self.lib.ttasr_spk_dim(self.h))
        self.has_speaker_embedding = True

    def speaker_embeddings(self, audios: Sequence[np.ndarray], weights: Sequence[np.ndarray], return_stats: bool = False):
        """One embedding per (chunk, mask) of every recording (ttasr_spk_embed): weights[i] is [chunks, S, 293] frame weights
        >= 0 on the segmentation network's chunks and frames, one S for the call; the result is a list of float32
        [chunks, S, D] arrays, rows of quiet NaN where a mask's resampled weights sum to 0.  return_stats=True:
        (embeddings, pooled statistics [chunks, S, 3000]).  More recordings than max_batch go through several calls; a row's
        values do not depend on its neighbours."""
        if not getattr(self, "has_speaker_embedding", False):
            raise TtasrError("no speaker-embedding network on this engine: load_speaker_embedding first")
        pcm, wts = [], []
        if len(audios) != len(weights):
            raise ValueError(f"{len(audios)} recordings and {len(weights)} weight arrays")
        n_masks = None
        for i, (a, w) in enumerate(zip(audios, weights)):
            a = np.ascontiguousarray(a, dtype=np.float32)
            w = np.ascontiguousarray(w, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"recording {i}: PCM must be one-dimensional, got shape {a.shape}")
            k = int(self.lib.ttasr_seg_chunks(len(a)))
            if w.ndim != 3 or w.shape[0] != k or w.shape[2] != _lib.SEG_CHUNK_FRAMES or (n_masks is not None and w.shape[1] != n_masks):
                raise ValueError(f"recording {i}: weights of shape {w.shape}, expected ({k}, S, {_lib.SEG_CHUNK_FRAMES}) with one S for the call")
            n_masks = w.shape[1]
            pcm.append(a)
            wts.append(w)
        if n_masks is None or not 1 <= n_masks <= _lib.SPK_MAX_MASKS:
            raise ValueError(f"masks per chunk {n_masks} outside 1 ... {_lib.SPK_MAX_MASKS}")
        emb = [np.zeros((w.shape[0], n_masks, self.spk_dim), dtype=np.float32) for w in wts]
        stats = [np.zeros((w.shape[0], n_masks, _lib.SPK_STATS), dtype=np.float32) for w in wts] if return_stats else None
        rows = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data if a.size else None for a in arrs])   # noqa: E731
        for i0 in range(0, len(pcm), self.max_batch):
            sl = slice(i0, i0 + self.max_batch)
            ns = np.asarray([len(a) for a in pcm[sl]], dtype=np.int64)
            self._check(self.lib.ttasr_spk_embed(self.h, len(ns), rows(pcm[sl]), ns.ctypes.data_as(C.POINTER(C.c_int64)), n_masks,
                                                 rows(wts[sl]), rows(emb[sl]), rows(stats[sl]) if return_stats else None), "spk_embed")
        return (emb, stats) if return_stats else emb

    # -- streaming voice activity detection --------------------------------------------------------
    def vad_stream_open(self, wire=None) -> int:
        """A new VAD stream of this context - one recording that arrives in pieces - with zero state and nothing pending
        (ttasr_vad_stream_open).  The first open allocates everything the stream path needs, so it is refused inside an open
        session; at most _lib.VAD_MAX_STREAMS streams of both kinds are open at a time.
        wire = (rate, channels, format, pick) with format one of _lib.PCM_* (not PCM_IMA4) and pick None / -1 for the mean of the
        channels or a channel index, or an object with `.wire_args()` (vad.WireFormat): a WIRE stream
        (ttasr_vad_stream_open_wire), fed bytes through `vad_stream_push_wire`."""
        sid = C.c_int32(-1)
        if wire is None:
            self._check(self.lib.ttasr_vad_stream_open(self.h, C.byref(sid)), "vad_stream_open")
            return int(sid.value)
        rate, channels, fmt, pick = wire.wire_args() if hasattr(wire, "wire_args") else wire
        self._check(self.lib.ttasr_vad_stream_open_wire(self.h, int(rate), int(channels), int(fmt), -1 if pick is None else int(pick),
                                                        C.byref(sid)), "vad_stream_open_wire")
        tail = self.ingest_stream_len(rate, 1 << 20, True) - self.ingest_stream_len(rate, 1 << 20, False)   # what a finish releases
        self._wire_streams[int(sid.value)] = (int(rate), int(channels) * (_lib.CODED_BYTES.get(int(fmt)) or _lib.PCM_BYTES[int(fmt)]),
                                              tail)
        return int(sid.value)

    def ingest_stream_len(self, rate: int, n_frames: int, finished: bool = False) -> int:
        """Final 16 kHz samples of a wire stream after n_frames frames at `rate` (ttasr_ingest_stream_len): K(n_frames), or all
        ceil(n_frames up / down) when finished; negative when `rate` is no stream rate."""
        return int(self.lib.ttasr_ingest_stream_len(int(rate), int(n_frames), 1 if finished else 0))

    def vad_stream_push_wire(self, ids: Sequence[int], raws: Sequence, finish: Optional[Sequence[bool]] = None,
                             return_logits: bool = False):
        """Append raws[i] (bytes-like, any length - a piece may end inside a sample) to WIRE stream ids[i], all rows in ONE call
        (ttasr_vad_stream_push_wire): (pcm, probs[, logits]), one float32 array per row each - the 16 kHz mono samples that became
        final and the probabilities of the 512-sample frames they completed.  The concatenated pcm of a stream whose last push has
        finish equals `ingest` of the whole recording bit for bit, and the probabilities `vad_probs` of that, however the bytes
        are cut.  Legal inside an open session, between its calls."""
        n = len(ids)
        if len(raws) != n or (finish is not None and len(finish) != n):
            raise ValueError("ids, raws and finish must have one entry per row")
        if n == 0:
            return ([], [], []) if return_logits else ([], [])
        bufs = [np.frombuffer(r, dtype=np.uint8) if isinstance(r, (bytes, bytearray, memoryview))
                else np.ascontiguousarray(r).reshape(-1).view(np.uint8) for r in raws]
        # room for every sample the bytes can make final: all held frames + the new ones, finished (the library checks it)
        caps = []
        for sid, b in zip(ids, bufs):
            # an id that is no wire stream of this engine: any size will do, the library refuses the call
            rate, fb, tail = self._wire_streams.get(int(sid), (16000, 1, 0))
            caps.append(self.ingest_stream_len(rate, len(b) // fb + 2, True) + tail + 2)
        pcm = [np.zeros(k, dtype=np.float32) for k in caps]
        probs = [np.zeros(k // 512 + 3, dtype=np.float32) for k in caps]
        logits = [np.zeros_like(p) for p in probs] if return_logits else None
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        idv = np.asarray(list(ids), dtype=np.int32)
        nb = np.asarray([len(b) for b in bufs], dtype=np.int64)
        cap = np.asarray(caps, dtype=np.int64)
        got = np.zeros(n, dtype=np.int64)
        fin = np.asarray([1 if f else 0 for f in finish], dtype=np.int32) if finish is not None else None
        frames = np.zeros(n, dtype=np.int32)
        ptrs = (C.c_void_p * n)(*[b.ctypes.data if len(b) else None for b in bufs])
        pouts = (C.c_void_p * n)(*[p.ctypes.data for p in pcm])
        outs = (C.c_void_p * n)(*[p.ctypes.data for p in probs])
        louts = (C.c_void_p * n)(*[p.ctypes.data for p in logits]) if return_logits else None
        self._check(self.lib.ttasr_vad_stream_push_wire(self.h, n, idv.ctypes.data_as(i32p), ptrs, nb.ctypes.data_as(i64p),
                                                        fin.ctypes.data_as(i32p) if fin is not None else None, pouts,
                                                        cap.ctypes.data_as(i64p), got.ctypes.data_as(i64p), outs, louts,
                                                        frames.ctypes.data_as(i32p)), "vad_stream_push_wire")
        pcm = [p[:k].copy() for p, k in zip(pcm, got)]
        probs = [p[:k].copy() for p, k in zip(probs, frames)]
        if return_logits:
            return pcm, probs, [l[:k].copy() for l, k in zip(logits, frames)]
        return pcm, probs

    def vad_stream_reset(self, stream_id: int):
        """The stream is as freshly opened (ttasr_vad_stream_reset); legal inside an open session."""
        self._check(self.lib.ttasr_vad_stream_reset(self.h, int(stream_id)), "vad_stream_reset")

    def vad_stream_close(self, stream_id: int):
        self._check(self.lib.ttasr_vad_stream_close(self.h, int(stream_id)), "vad_stream_close")
        self._wire_streams.pop(int(stream_id), None)

    def vad_stream_push(self, ids: Sequence[int], audios: Sequence[np.ndarray], finish: Optional[Sequence[bool]] = None,
                        return_logits: bool = False):
        """Append audios[i] (float32 PCM, 0 samples is legal) to stream ids[i], all rows in ONE call (ttasr_vad_stream_push): a
        list with one float32 array per row, the probabilities of the 512-sample frames the row completed (samples that fill no
        frame stay pending in the stream); finish[i] evaluates the zero-padded remainder too and leaves the stream as reset.
        return_logits=True: (probabilities, pre-sigmoid logits).  The concatenated outputs of a stream equal `vad_probs` on the
        concatenated pieces bit for bit, however the recording is cut and whatever else shares the calls.  Legal inside an open
        session, between its calls."""
        n = len(ids)
        if len(audios) != n or (finish is not None and len(finish) != n):
            raise ValueError("ids, audios and finish must have one entry per row")
        if n == 0:
            return ([], []) if return_logits else []
        pcm = []
        for i, a in enumerate(audios):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"row {i}: PCM must be one-dimensional, got shape {a.shape}")
            pcm.append(a)
        probs = [np.zeros(len(a) // 512 + 2, dtype=np.float32) for a in pcm]
        logits = [np.zeros_like(p) for p in probs] if return_logits else None
        i32p = C.POINTER(C.c_int32)
        idv = np.asarray(list(ids), dtype=np.int32)
        ns = np.asarray([len(a) for a in pcm], dtype=np.int64)
        fin = np.asarray([1 if f else 0 for f in finish], dtype=np.int32) if finish is not None else None
        frames = np.zeros(n, dtype=np.int32)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data if len(a) else None for a in pcm])
        outs = (C.c_void_p * n)(*[p.ctypes.data for p in probs])
        louts = (C.c_void_p * n)(*[p.ctypes.data for p in logits]) if return_logits else None
        self._check(self.lib.ttasr_vad_stream_push(self.h, n, idv.ctypes.data_as(i32p), ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   fin.ctypes.data_as(i32p) if fin is not None else None, outs, louts,
                                                   frames.ctypes.data_as(i32p)), "vad_stream_push")
        probs = [p[:k].copy() for p, k in zip(probs, frames)]
        if return_logits:
            return probs, [l[:k].copy() for l, k in zip(logits, frames)]
        return probs

    # -- file ingest -----------------------------------------------------------------------------
    def ingest(self, raws: Sequence, rates: Sequence[int], channels: Sequence[int], formats: Sequence[int],
               block_aligns: Optional[Sequence[int]] = None, picks: Optional[Sequence[Optional[int]]] = None,
               n_frames: Optional[Sequence[Optional[int]]] = None) -> List[np.ndarray]:
        """Raw interleaved samples of n recordings -> float32 mono 16 kHz, in ONE device call: raws[i] is a bytes-like object or a
        C-contiguous array holding whole frames of channels[i] samples in formats[i] (_lib.PCM_*) at rates[i] Hz.  Rates and
        formats may differ; n is not limited by max_batch; no weights are needed.  A rate the device does not take (see
        `ingest_accepts`) raises TtasrError: the caller converts that file on the host.
        The coded formats (_lib.PCM_ALAW, PCM_ULAW, PCM_IMA4; block_aligns[i] = the file's block size for IMA, whose trailing
        bytes short of a block are ignored), picks (None / -1 = the mean of the channels, c = channel c alone) and n_frames (a
        frame count below what the bytes hold: an IMA file's `fact`) go through ttasr_ingest_wave; a call without any of them
        is ttasr_ingest_pcm, as before.
        A FLAC recording (_lib.PCM_FLAC) is the whole file as read, tags and metadata included, with the stream's own rate and
        channel count; its frame count comes from the library's probe (ttasr_flac_probe) unless n_frames[i] gives a smaller one,
        and a stream the library refuses raises TtasrError with the library's reason."""
        n = len(raws)
        if not (len(rates) == len(channels) == len(formats) == n):
            raise ValueError("raws, rates, channels and formats must have one entry per recording")
        for name, v in (("block_aligns", block_aligns), ("picks", picks), ("n_frames", n_frames)):
            if v is not None and len(v) != n:
                raise ValueError(f"{name} must have one entry per recording")
        wave = not (block_aligns is None and picks is None and n_frames is None) or any(int(f) >= _lib.PCM_ALAW for f in formats)
        bufs, frames = [], np.zeros(max(n, 1), dtype=np.int64)
        nbytes, bal = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int32)
        for i, r in enumerate(raws):
            b = np.frombuffer(r, dtype=np.uint8) if isinstance(r, (bytes, bytearray, memoryview)) else np.ascontiguousarray(r).reshape(-1).view(np.uint8)
            ch, fmt = int(channels[i]), int(formats[i])
            if fmt == _lib.PCM_FLAC:      # the whole file as read: the samples held come from the probe, unless the caller has them
                if n_frames is None or n_frames[i] is None:
                    try:
                        frames[i] = _lib.flac_probe(b).samples
                    except ValueError as e:
                        raise TtasrError(f"ingest_wave: recording {i}: {e}") from None
            elif fmt == _lib.PCM_IMA4:
                bal[i] = int(block_aligns[i]) if block_aligns is not None and block_aligns[i] is not None else 0
                ok = ch > 0 and bal[i] >= 8 * ch and bal[i] % (4 * ch) == 0       # otherwise the library refuses the call with a message
                frames[i] = len(b) // int(bal[i]) * (1 + 2 * (int(bal[i]) // ch - 4)) if ok else len(b)
            else:
                width = _lib.CODED_BYTES.get(fmt) or (_lib.PCM_BYTES[fmt] if 0 <= fmt < len(_lib.PCM_BYTES) else 0)
                fb = width * ch if ch > 0 else 0
                if fb and len(b) % fb:
                    raise ValueError(f"recording {i}: {len(b)} bytes are no whole number of {fb}-byte frames")
                frames[i] = len(b) // fb if fb else len(b)   # bad channels / format: the library refuses the call with a message
            if n_frames is not None and n_frames[i] is not None:
                frames[i] = int(n_frames[i])
            nbytes[i] = len(b)
            bufs.append(b)
        rate = np.asarray(list(rates) or [0], dtype=np.int32)
        chan = np.asarray(list(channels) or [0], dtype=np.int32)
        fmts = np.asarray(list(formats) or [0], dtype=np.int32)
        outs = [np.zeros(max(int(self.lib.ttasr_ingest_len(int(rate[i]), int(frames[i]))), 0), dtype=np.float32) for i in range(n)]
        if n == 0:
            return outs
        ptrs = (C.c_void_p * n)(*[b.ctypes.data if len(b) else None for b in bufs])
        optr = (C.c_void_p * n)(*[o.ctypes.data if len(o) else None for o in outs])
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        if not wave:
            self._check(self.lib.ttasr_ingest_pcm(self.h, n, ptrs, frames.ctypes.data_as(i64p), rate.ctypes.data_as(i32p),
                                                  chan.ctypes.data_as(i32p), fmts.ctypes.data_as(i32p), optr), "ingest_pcm")
            return outs
        pk = np.asarray([-1 if p is None else int(p) for p in (picks if picks is not None else [None] * n)], dtype=np.int32)
        self._check(self.lib.ttasr_ingest_wave(self.h, n, ptrs, nbytes.ctypes.data_as(i64p), frames.ctypes.data_as(i64p),
                                               rate.ctypes.data_as(i32p), chan.ctypes.data_as(i32p), fmts.ctypes.data_as(i32p),
                                               bal.ctypes.data_as(i32p), pk.ctypes.data_as(i32p), optr), "ingest_wave")
        return outs

    def ingest_accepts(self, rate: int) -> bool:
        """Whether ttasr_ingest_pcm takes recordings at `rate` (max(up, down) of the ratio to 16 kHz at most 1024)."""
        return self.lib.ttasr_ingest_len(int(rate), 0) >= 0

    # -- a5 ------------------------------------------------------------------------------------
    def set_audio_ctx(self, n_ctx: int = 0):
        """Opt-in short window (ttasr_set_audio_ctx): the next log_mel/encode/generate use n_ctx encoder positions
        (n_ctx * 320 samples); 0 restores the model's 30-s window."""
        n = int(n_ctx) or self.dims.n_audio_ctx
        self._check(self.lib.ttasr_set_audio_ctx(self.h, n), "set_audio_ctx")
        self.audio_ctx = n

    def log_mel(self, clips: Sequence[np.ndarray], want_output: bool = True) -> Optional[np.ndarray]:
        B = len(clips)
        n_win = 2 * self.audio_ctx * 160
        stride = max(1, min(n_win, max((len(c) for c in clips), default=1)))
        pcm = np.zeros((B, stride), dtype=np.float32)
        ns = np.zeros(B, dtype=np.int64)
        for b, c in enumerate(clips):
            n = min(len(c), stride)
            pcm[b, :n] = np.asarray(c[:n], dtype=np.float32)
            ns[b] = n
        out = np.empty((B, self.dims.n_mels, 2 * self.audio_ctx), dtype=np.float32) if want_output else None
        self._check(self.lib.ttasr_log_mel(self.h, _ptr(pcm), stride, ns.ctypes.data_as(C.POINTER(C.c_int64)), B, 0,
                                           _ptr(out) if want_output else None), "log_mel")
        return out

    def log_mel_windows(self, audio, seeks: Sequence[int], floor_max: Optional[Sequence[float]] = None,
                        want_output: bool = False, want_max: bool = False, n_frames: Optional[Sequence[int]] = None):
        """Windows of recordings (ttasr_log_mel_windows): window b starts at 10-ms frame seeks[b] of `audio` (one float32
        array = all windows belong to that recording) or of audio[b] (a sequence: one recording per window, several files in
        lock step); frames are those of the whole-file STFT, frames past the end of the recording are 0 in feature space,
        and the dynamic-range floor comes from floor_max[b] (the whole-file log-mel maximum) when given.
        n_frames (ttasr_log_mel_windows_cut): window b keeps at most n_frames[b] >= 1 frames - a clip that ends before the
        recording does; the kept frames are those of the uncut window, the rest is 0 and the maxima cover the kept frames.
        Returns (mel or None, per-window maxima or None)."""
        sk = np.ascontiguousarray(seeks, dtype=np.int64)
        B = len(sk)
        files = [audio] * B if isinstance(audio, np.ndarray) else list(audio)
        files = [np.ascontiguousarray(a, dtype=np.float32) for a in files]
        ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in files])
        lens = np.asarray([len(a) for a in files], dtype=np.int64)
        fm = None if floor_max is None else np.ascontiguousarray(floor_max, dtype=np.float32)
        out = np.empty((B, self.dims.n_mels, 2 * self.audio_ctx), dtype=np.float32) if want_output else None
        mx = np.empty(B, dtype=np.float32) if want_max else None
        i64p = C.POINTER(C.c_int64)
        args = (self.h, ptrs, lens.ctypes.data_as(i64p), sk.ctypes.data_as(i64p), B, _ptr(fm) if fm is not None else None,
                _ptr(mx) if want_max else None, _ptr(out) if want_output else None)
        if n_frames is None:
            self._check(self.lib.ttasr_log_mel_windows(*args), "log_mel_windows")
        else:
            nf = np.ascontiguousarray(n_frames, dtype=np.int64)
            if nf.shape != (B,):
                raise ValueError(f"n_frames needs one frame count per window ({B}), got shape {nf.shape}")
            self._check(self.lib.ttasr_log_mel_windows_cut(*args, nf.ctypes.data_as(i64p)), "log_mel_windows_cut")
        return out, mx

    def log_mel_device(self, dev_ptr: int, stride: int, n_samples: Sequence[int]):
        """PCM already resident in HBM (bench): dev_ptr = device address of float32 [B][stride]."""
        ns = np.asarray(n_samples, dtype=np.int64)
        self._check(self.lib.ttasr_log_mel(self.h, C.c_void_p(dev_ptr), stride, ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                           len(ns), 1, None), "log_mel(device)")

    def log_mel_host_ptr(self, host_ptr: int, stride: int, n_samples: Sequence[int]):
        """PCM in a caller-owned (ideally pinned) host buffer: the call includes the H2D copy."""
        ns = np.asarray(n_samples, dtype=np.int64)
        self._check(self.lib.ttasr_log_mel(self.h, C.c_void_p(host_ptr), stride, ns.ctypes.data_as(C.POINTER(C.c_int64)),
                                           len(ns), 0, None), "log_mel(host)")

    def set_mel(self, mel: np.ndarray):
        mel = np.ascontiguousarray(mel, dtype=np.float32)
        assert mel.shape[1:] == (self.dims.n_mels, 2 * self.audio_ctx), mel.shape
        self._check(self.lib.ttasr_set_mel(self.h, _ptr(mel), mel.shape[0]), "set_mel")

    def set_option(self, key: str, value: int):
        """Kernel-selection override for tests / A-B measurements (ttasr_set_option; keys in include/ttasr.h).  The library
        reads no environment variable: this call is the only way to leave the measured configuration."""
        self._check(self.lib.ttasr_set_option(self.h, key.encode(), int(value)), f"set_option({key})")
        if key == "session_prefill":
            self._session_prefill = int(value)   # what Session restores when its prefill keyword has changed the option

    # -- a6..a8 --------------------------------------------------------------------------------
    def encode(self, B: int, want_output: bool = False) -> Optional[np.ndarray]:
        out = np.empty((B, self.audio_ctx, self.dims.d_model), dtype=np.float32) if want_output else None
        self._check(self.lib.ttasr_encode(self.h, B, _ptr(out) if want_output else None), "encode")
        return out

    def set_encoder_output(self, enc: np.ndarray):
        enc = np.ascontiguousarray(enc, dtype=np.float32)
        self._check(self.lib.ttasr_set_encoder_output(self.h, _ptr(enc), enc.shape[0]), "set_encoder_output")

    def cross_kv(self, layer: int, which: int, B: int) -> np.ndarray:
        out = np.empty((B, self.dims.n_heads, self.audio_ctx, 64), dtype=np.float32)
        self._check(self.lib.ttasr_get_cross_kv(self.h, layer, which, B, _ptr(out)), "get_cross_kv")
        return out

    def cross_kv_fp8(self, layer: int, which: int, B: int):
        """The resident e4m3 copy (ttasr_get_cross_kv_fp8): (codes uint8 [B][H][T][64], scales float32 [B][H]).  In an open
        session B counts cross-KV slots."""
        codes = np.empty((B, self.dims.n_heads, self.audio_ctx, 64), dtype=np.uint8)
        scale = np.empty((B, self.dims.n_heads), dtype=np.float32)
        self._check(self.lib.ttasr_get_cross_kv_fp8(self.h, layer, which, B, codes.ctypes.data_as(C.c_void_p),
                                                    _ptr(scale)), "get_cross_kv_fp8")
        return codes, scale

    def cross_attn_probe(self, layer: int, q: np.ndarray, kv_div: int = 1, done: Optional[np.ndarray] = None):
        """One launch of the decode step's cross-attention on the caller's queries (ttasr_cross_attn_probe).  q: float32
        [n_rows][d_model], or [n_slab][n_rows][d_model] partial tiles (n_slab 1..4).  Returns (out float32 [n_rows][d_model],
        signature of the kernel that ran)."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        n_slab = q.shape[0] if q.ndim == 3 else 0
        n_rows = q.shape[-2]
        assert q.shape[-1] == self.dims.d_model, q.shape
        out = np.empty((n_rows, self.dims.d_model), dtype=np.float32)
        flags = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
        assert flags is None or flags.shape == (n_rows,)
        buf = C.create_string_buffer(256)
        self._check(self.lib.ttasr_cross_attn_probe(self.h, layer, n_rows, kv_div, _ptr(q), n_slab,
                                                    None if flags is None else flags.ctypes.data_as(C.c_void_p), _ptr(out), buf, 256),
                    "cross_attn_probe")
        return out, buf.value.decode()

    def align_attn_probe(self, layer: int, q: np.ndarray, lens: Sequence[int], slots: Sequence[int], head_pair: Sequence[int]):
        """The cross-attention of the packed alignment pass on the caller's queries (ttasr_align_attn_probe).  q: float32
        [sum(lens)][d_model], sequence i = lens[i] consecutive rows reading the cross-KV of clip slots[i]; head_pair [n_heads]:
        -1 or the index of the map that head writes.  Returns (out float32 [rows][d_model], maps float32 [n_pairs][rows][T])."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        ln, sl = np.ascontiguousarray(lens, dtype=np.int32), np.ascontiguousarray(slots, dtype=np.int32)
        hp = np.ascontiguousarray(head_pair, dtype=np.int32)
        rows = int(ln.sum())
        if q.shape != (rows, self.dims.d_model) or ln.shape != sl.shape or hp.shape != (self.dims.n_heads,):
            raise ValueError(f"q {q.shape}, lens {ln.shape}, slots {sl.shape}, head_pair {hp.shape}")
        n_pairs = int((hp >= 0).sum())
        out = np.empty((rows, self.dims.d_model), dtype=np.float32)
        maps = np.empty((n_pairs, rows, self.audio_ctx), dtype=np.float32)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.ttasr_align_attn_probe(self.h, layer, len(ln), ln.ctypes.data_as(i32p), sl.ctypes.data_as(i32p), _ptr(q),
                                                    hp.ctypes.data_as(i32p), n_pairs, _ptr(out), _ptr(maps) if n_pairs else None),
                    "align_attn_probe")
        return out, maps

    # -- known-answer hooks of the decoder self-attention ------------------
    SELF_FORMS = {"step": 0, "rows": 1, "prefill": 2, "packed": 3, "copy": 4}   # TTASR_SELF_* of include/ttasr.h

    @property
    def pages_per_seq(self) -> int:
        return (self.dims.n_text_ctx + 15) // 16

    def self_kv_fill(self, layer: int, pattern: int):
        """Every element of the layer's self-attention KV pool (-1: of every layer) = the bit pattern (ttasr_self_kv_fill)."""
        self._check(self.lib.ttasr_self_kv_fill(self.h, layer, pattern & 0xffffffff), "self_kv_fill")

    def self_kv_set(self, layer: int, pages: Sequence[int], kv: np.ndarray, n: int = 16):
        """Positions [0, n) of the listed pool pages from float32 page images [n_pages][2][H][16][64] (ttasr_self_kv_set)."""
        pg = np.ascontiguousarray(pages, dtype=np.int32)
        kv = np.ascontiguousarray(kv, dtype=np.float32)
        assert kv.shape == (len(pg), 2, self.dims.n_heads, 16, 64), kv.shape
        self._check(self.lib.ttasr_self_kv_set(self.h, layer, pg.ctypes.data_as(C.c_void_p), len(pg), n, _ptr(kv)), "self_kv_set")

    def self_kv_get(self, layer: int, pages: Optional[Sequence[int]] = None) -> np.ndarray:
        """Pool pages of a layer as float32 [n_pages][2][H][16][64], exactly; pages None = the whole layer (ttasr_self_kv_get)."""
        pg = None if pages is None else np.ascontiguousarray(pages, dtype=np.int32)
        n = self.max_batch * self.pages_per_seq if pg is None else len(pg)
        out = np.empty((n, 2, self.dims.n_heads, 16, 64), dtype=np.float32)
        self._check(self.lib.ttasr_self_kv_get(self.h, layer, None if pg is None else pg.ctypes.data_as(C.c_void_p), n, _ptr(out)), "self_kv_get")
        return out

    def self_attn_probe(self, form: str, layer: int = 0, qkv: Optional[np.ndarray] = None, geom: Sequence[int] = (),
                        aux: Optional[Sequence[int]] = None, identity_pages: bool = True, row0: int = 0, done: Optional[np.ndarray] = None):
        """One launch of a named form of the decoder self-attention (ttasr_self_attn_probe).  qkv: float32 [n_rows][3 d_model], or
        [n_slab][n_rows][3 d_model] partial tiles; geom: the position (step), the rows' positions (rows), (n_seq, npos) (prefill) or
        the sequences' lengths (packed); aux: the page table [max_batch][pages_per_seq] (step, rows, prefill; None = identity), the
        page lists (packed) or the (source, destination) pairs (copy).  Returns (out float32 [n_rows][d_model] or None for copy,
        signature of what ran)."""
        gm = np.ascontiguousarray(geom, dtype=np.int32).reshape(-1)
        ax = np.zeros(0, np.int32) if aux is None else np.ascontiguousarray(aux, dtype=np.int32).reshape(-1)
        buf = C.create_string_buffer(256)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        if form == "copy":
            self._check(self.lib.ttasr_self_attn_probe(self.h, 4, 0, 0, None, 0, None, 0, vp(ax), ax.size, 0, 0, None, None, buf, 256), "self_attn_probe")
            return None, buf.value.decode()
        qkv = np.ascontiguousarray(qkv, dtype=np.float32)
        n_slab = qkv.shape[0] if qkv.ndim == 3 else 0
        n_rows = qkv.shape[-2]
        assert qkv.shape[-1] == 3 * self.dims.d_model, qkv.shape
        out = np.empty((n_rows, self.dims.d_model), dtype=np.float32)
        flags = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
        assert flags is None or flags.shape == (n_rows,)
        self._check(self.lib.ttasr_self_attn_probe(self.h, self.SELF_FORMS[form], layer, n_rows, _ptr(qkv), n_slab, vp(gm), gm.size, vp(ax), ax.size,
                                                   1 if identity_pages else 0, row0, vp(flags), _ptr(out), buf, 256), "self_attn_probe")
        return out, buf.value.decode()

    def enc_attn_probe(self, qkv: Optional[np.ndarray] = None, q: Optional[np.ndarray] = None, k: Optional[np.ndarray] = None,
                       v: Optional[np.ndarray] = None):
        """One launch of the encoder attention on the caller's operands (ttasr_enc_attn_probe).  Self form: qkv float32
        [B][T][3 d_model].  Cross form (16-bit engines): q float32 [clips][n_q][d_model], k and v float32 [clips][n_heads][Tk][64].
        Returns (out float32 [B][T][d_model] - NaN where no kernel wrote, signature of what ran, whether the guard row behind the
        output kept its fill pattern)."""
        d, buf = self.dims.d_model, C.create_string_buffer(256)
        if qkv is not None:
            assert q is None and k is None and v is None
            a = np.ascontiguousarray(qkv, dtype=np.float32)
            assert a.ndim == 3 and a.shape[2] == 3 * d, a.shape
            form, kk, vv, Tk = 0, None, None, 0
        else:
            a = np.ascontiguousarray(q, dtype=np.float32)
            kk, vv = np.ascontiguousarray(k, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
            assert a.ndim == 3 and a.shape[2] == d, a.shape
            assert kk.shape == vv.shape == (a.shape[0], self.dims.n_heads, kk.shape[2], 64), (kk.shape, vv.shape)
            form, Tk = 1, kk.shape[2]
        out = np.empty((a.shape[0], a.shape[1], d), dtype=np.float32)
        rc = self.lib.ttasr_enc_attn_probe(self.h, form, a.shape[0], a.shape[1], _ptr(a), None if kk is None else _ptr(kk),
                                           None if vv is None else _ptr(vv), Tk, _ptr(out), buf, 256)
        if rc != 1:   # TTASR_ENC_GUARD_TOUCHED: the output is there, the guard row is not what it was
            self._check(rc, "enc_attn_probe")
        return out, buf.value.decode(), rc == 0

    # -- a9, a10 -------------------------------------------------------------------------------
    def gen_opts(self, max_new_tokens: int, timestamps: bool, suppress: Optional[Sequence[int]] = None,
                 begin_suppress: Optional[Sequence[int]] = None, suppress_eot: bool = False, no_speech: bool = True,
                 sot_index: int = 0, max_initial_timestamp_index: Optional[int] = 50, check_interval: int = 8):
        st = self.special
        sup = np.asarray(default_suppress(st, self.dims.vocab) if suppress is None else list(suppress), dtype=np.int32)
        bsup = np.asarray([220, st.eot] if begin_suppress is None else list(begin_suppress), dtype=np.int32)
        o = _lib.GenOpts()
        o.max_new_tokens = max_new_tokens
        o.eot, o.no_timestamps, o.timestamp_begin = st.eot, st.no_timestamps, st.timestamp_begin
        o.no_speech = st.no_speech if no_speech else -1
        o.sot_index = sot_index
        o.timestamps = int(timestamps)
        o.max_initial_timestamp_index = -1 if max_initial_timestamp_index is None else max_initial_timestamp_index
        o.suppress_eot = int(suppress_eot)
        o.n_suppress, o.n_begin_suppress = len(sup), len(bsup)
        o.check_interval = check_interval
        o.suppress = sup.ctypes.data_as(C.POINTER(C.c_int32))
        o.begin_suppress = bsup.ctypes.data_as(C.POINTER(C.c_int32))
        o._keep = (sup, bsup)  # keep the arrays alive
        return o

    def generate(self, prompts: Sequence[Sequence[int]], opts, row_max_new: Optional[Sequence[int]] = None) -> GenResult:
        """Greedy search.  row_max_new (optional, one entry per row, each in [1, opts.max_new_tokens]) = per-row token budgets
        (ttasr_generate_capped): a row is finished at its budget or at EOT, and finished rows leave the decode step's attention
        kernels - the rows that go on are bit-identical to a run without budgets."""
        B = len(prompts)
        max_prompt = max(len(p) for p in prompts)
        pr = np.zeros((B, max_prompt), dtype=np.int32)
        pl = np.zeros(B, dtype=np.int32)
        for b, p in enumerate(prompts):
            pr[b, :len(p)] = p
            pl[b] = len(p)
        toks = np.zeros((B, opts.max_new_tokens), dtype=np.int32)
        lens = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        ns = np.zeros(B, dtype=np.float32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        if row_max_new is not None:
            caps = np.ascontiguousarray(row_max_new, dtype=np.int32)
            if caps.shape != (B,):
                raise ValueError(f"row_max_new needs one entry per row ({B}), got shape {caps.shape}")
            if caps.min() < 1 or caps.max() > opts.max_new_tokens:
                raise ValueError(f"row_max_new entries must lie in [1, max_new_tokens={opts.max_new_tokens}], got {caps.tolist()}")
            self._check(self.lib.ttasr_generate_capped(self.h, B, pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p), max_prompt,
                                                       C.byref(opts), caps.ctypes.data_as(i32p), toks.ctypes.data_as(i32p),
                                                       lens.ctypes.data_as(i32p), lp.ctypes.data_as(f32p),
                                                       ns.ctypes.data_as(f32p)), "generate_capped")
            return GenResult([toks[b, :lens[b]].tolist() for b in range(B)], lp, ns)
        self._check(self.lib.ttasr_generate(self.h, B, pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p), max_prompt,
                                            C.byref(opts), toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                            lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p)), "generate")
        return GenResult([toks[b, :lens[b]].tolist() for b in range(B)], lp, ns)

    def session(self, opts, max_prompt: int, temperature: float = 0.0, beam: int = 1,
                patience: Optional[float] = None, detect_language=False, prefill: int = 0) -> "Session":
        """Continuous-batching session (ttasr_session_*): greedy, single-window decoding of clips submitted at any time; each clip
        takes a free row of the max_batch-row decode batch and hands it to the next queued clip when it finishes.  A context
        manager: the session ends when the block is left.  While it is open the engine's other search / encode calls are refused.

        beam > 1, or beam given together with a patience (default 1.0): beam search (ttasr_session_begin_beam); a clip takes a
        group of `beam` rows, and its result equals ttasr_generate_beam's (tokens without EOT).

        detect_language=True, or (sot, first language token, count): the session is armed for language identification
        (ttasr_session_detect_language; True = this engine's <|startoftranscript|> and language_span()).  A prompt may then hold
        Session.DETECT directly behind <|startoftranscript|>: the clip's first step finds its language on the device and writes
        it over the placeholder; SessionResult.language / language_probs carry the answer.

        prefill = N (option "session_prefill"; True = config.SESSION_PREFILL_DEFAULT, 0 = off): a clip whose prompt has at least N
        prefillable positions gets them from one admission pass instead of N forced decode steps; Session.stats() reports the
        passes.  The keyword OWNS the option for this session: whatever Engine.set_option("session_prefill", ...) left is
        replaced for the session_begin and put back when the session closes (options cannot change while a session is open)."""
        return Session(self, opts, max_prompt, temperature, beam, patience, detect_language, prefill)

    def generate_beam(self, prompts: Sequence[Sequence[int]], beam: int, opts, patience: float = 1.0,
                      sot_index: Optional[Sequence[int]] = None) -> GenResult:
        """Beam search over len(prompts) clips; rows = clips * beam <= max_batch.  Prompts may differ in length (one
        previous-text prompt per file); sot_index then gives each prompt's <|startoftranscript|> position."""
        A = len(prompts)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        toks = np.zeros((A, opts.max_new_tokens), dtype=np.int32)
        lens = np.zeros(A, dtype=np.int32)
        lp = np.zeros(A, dtype=np.float32)
        ns = np.zeros(A, dtype=np.float32)
        plen = len(prompts[0])
        if all(len(p) == plen for p in prompts) and sot_index is None:
            pr = np.asarray(prompts, dtype=np.int32).reshape(A, plen)
            self._check(self.lib.ttasr_generate_beam(self.h, A, beam, pr.ctypes.data_as(i32p), plen, C.byref(opts),
                                                     C.c_float(patience), toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                                     lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p)), "generate_beam")
        else:
            max_prompt = max(len(p) for p in prompts)
            pr = np.zeros((A, max_prompt), dtype=np.int32)
            pl = np.zeros(A, dtype=np.int32)
            for a, p in enumerate(prompts):
                pr[a, :len(p)] = p
                pl[a] = len(p)
            so = None if sot_index is None else np.ascontiguousarray(sot_index, dtype=np.int32)
            self._check(self.lib.ttasr_generate_beam_ragged(
                self.h, A, beam, pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p),
                so.ctypes.data_as(i32p) if so is not None else None, max_prompt, C.byref(opts), C.c_float(patience),
                toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p)),
                "generate_beam_ragged")
        return GenResult([toks[a, :lens[a]].tolist() for a in range(A)], lp, ns)

    def generate_sample(self, prompts: Sequence[Sequence[int]], best_of: int, opts, temperature: float, seed: int = 0
                        ) -> GenResult:
        """Temperature sampling: best_of rows per clip (shared cross-KV), best average log-prob per clip returned."""
        A = len(prompts)
        plen = len(prompts[0])
        assert all(len(p) == plen for p in prompts), "sampling needs equal-length prompts"
        pr = np.asarray(prompts, dtype=np.int32).reshape(A, plen)
        toks = np.zeros((A, opts.max_new_tokens), dtype=np.int32)
        lens = np.zeros(A, dtype=np.int32)
        lp = np.zeros(A, dtype=np.float32)
        ns = np.zeros(A, dtype=np.float32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        self._check(self.lib.ttasr_generate_sample(self.h, A, best_of, pr.ctypes.data_as(i32p), plen, C.byref(opts),
                                                   C.c_float(temperature), C.c_uint32(seed & 0xFFFFFFFF),
                                                   toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                                   lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p)), "generate_sample")
        return GenResult([toks[a, :lens[a]].tolist() for a in range(A)], lp, ns)

    def align(self, clip: int, tokens: Sequence[int], heads: Sequence[Tuple[int, int]], want_logprob: bool = True):
        """Cross-attention rows of the (layer, head) pairs for a teacher-forced token sequence of one resident clip:
        (weights float32 [n_heads][n_tokens][audio_ctx], logprob float32 [n_tokens - 1] or None)."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        pr = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1, 2)
        w = np.empty((len(pr), len(tok), self.audio_ctx), dtype=np.float32)
        lp = np.empty(max(len(tok) - 1, 1), dtype=np.float32) if want_logprob else None
        self._check(self.lib.ttasr_align(self.h, clip, tok.ctypes.data_as(C.POINTER(C.c_int32)), len(tok),
                                         pr.ctypes.data_as(C.POINTER(C.c_int32)), len(pr),
                                         w.ctypes.data_as(C.POINTER(C.c_float)),
                                         lp.ctypes.data_as(C.POINTER(C.c_float)) if want_logprob else None), "align")
        return w, (lp[: len(tok) - 1] if want_logprob else None)

    def align_batch(self, clips: Sequence[int], tokens: Sequence[Sequence[int]], first_row: Sequence[int],
                    num_frames: Sequence[int], heads: Sequence[Tuple[int, int]], medfilt_width: int = 7,
                    debug: bool = False) -> AlignBatchResult:
        """Word alignment of len(tokens) teacher-forced sequences in one device pass (ttasr_align_batch): sequence i belongs to
        the resident clip clips[i] (several may share a clip); first_row[i] is the first token row of its cost matrix,
        num_frames[i] the clip's length in 10-ms frames.  Normalisation, median filter and DTW run on the device; only the
        start frames and the token log-probs come back (debug=True: the cost matrices and raw maps too).  Arguments are checked
        here before the library is called."""
        packed = _align_batch_args(self, tokens, first_row, num_frames, heads, medfilt_width)
        cl = np.ascontiguousarray(clips, dtype=np.int32)
        if cl.shape != (len(tokens),):
            raise ValueError(f"need one clip index per sequence ({len(tokens)}), got shape {cl.shape}")
        if cl.min() < 0 or cl.max() >= self.max_batch:
            raise ValueError(f"clip indices must lie in [0, {self.max_batch})")
        return _align_batch_call(self, self.lib.ttasr_align_batch, "align_batch", cl.ctypes.data_as(C.POINTER(C.c_int32)), packed,
                                 debug)

    def language_span(self) -> Tuple[int, int]:
        """(first language token, number of language tokens): sot + 1 up to the first of <|translate|> / <|transcribe|>, capped at
        the languages this build can name."""
        from .model import LANGUAGES
        st = self.special
        n = min(st.translate, st.transcribe) - (st.sot + 1)
        return st.sot + 1, max(1, min(n, len(LANGUAGES)))

    def detect_language(self, B: int, want_logits: bool = False, span: Optional[Tuple[int, int]] = None):
        """Language identification of the B clips whose encoder state is resident (ttasr_detect_language: one decoder pass at
        <|startoftranscript|> ending in the language head; no vocabulary projection, no second encoder pass).
        -> (indices int32 [B] into the span, probs float32 [B][n_lang][, span logits float32 [B][n_lang]]).
        span = (first token, count), default language_span().  Invalidates any step-level decode state."""
        begin, n_lang = self.language_span() if span is None else (int(span[0]), int(span[1]))
        B = int(B)
        idx = np.zeros(max(B, 1), dtype=np.int32)
        probs = np.zeros((max(B, 1), max(n_lang, 1)), dtype=np.float32)
        logits = np.zeros_like(probs) if want_logits else None
        self._check(self.lib.ttasr_detect_language(self.h, B, self.special.sot, begin, n_lang,
                                                   idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   probs.ctypes.data_as(C.POINTER(C.c_float)),
                                                   logits.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None),
                    "detect_language")
        return (idx, probs, logits) if want_logits else (idx, probs)

    def decode_reset(self, B: int):
        self._check(self.lib.ttasr_decode_reset(self.h, B), "decode_reset")

    def decode_step(self, tokens: Sequence[int], want_logits: bool = True) -> Optional[np.ndarray]:
        t = np.asarray(tokens, dtype=np.int32)
        out = np.empty((len(t), self.dims.vocab), dtype=np.float32) if want_logits else None
        self._check(self.lib.ttasr_decode_step(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), len(t),
                                               _ptr(out) if want_logits else None), "decode_step")
        return out

    def apply_rules(self, rows: np.ndarray, hist: np.ndarray, opts) -> Tuple[np.ndarray, np.ndarray]:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        n = rows.shape[0]
        out = np.empty_like(rows)
        choice = np.empty(n, dtype=np.int32)
        self._check(self.lib.ttasr_apply_rules(self.h, _ptr(rows), hist.ctypes.data_as(C.POINTER(C.c_int32)), hist.shape[1],
                                               n, C.byref(opts), _ptr(out), choice.ctypes.data_as(C.POINTER(C.c_int32))),
                    "apply_rules")
        return out, choice

    def select_probe(self, form: str, rows: np.ndarray, opts=None, hist: Optional[np.ndarray] = None, positions=None,
                     temperature: float = 0.0, seed: int = 0, prompt: Optional[np.ndarray] = None, prompt_len=None, done=None,
                     row_cap=None, sum_logprob=None, n_done: int = 0, entries=None, entry_temp=None, entry_seed=None, k: int = 0,
                     want_no_speech: bool = False, targets=None, token: int = 0) -> Dict[str, object]:
        """One launch of a named form of the token-selection kernels on the caller's raw logits rows float32 [n][vocab]
        (ttasr_select_probe): "step", "rows" (the whole search state after the launch, by field name, plus "positions"),
        "session" ("choice" int32, "lp", "no_speech" per entry), "topk" ("lp", "id" [n][k], "no_speech"), "logprob", "prob"
        ("out" [n]).  Every result carries "sig", the instantiation that ran.  The search state is undefined afterwards."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = rows.shape[0]
        assert rows.ndim == 2 and rows.shape[1] == self.dims.vocab, rows.shape
        io = _lib.SelectIO()
        keep = [rows]

        def arr(a, dt, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            assert shape is None or a.shape == shape, (a.shape, shape)
            keep.append(a)
            return a.ctypes.data

        def out(name, shape, dt):
            a = np.zeros(shape, dtype=dt)
            setattr(io, name, a.ctypes.data)
            return a

        io.rows_host, io.n = rows.ctypes.data, n
        io.opts = C.addressof(opts) if opts is not None else None
        if hist is not None:
            hist = np.ascontiguousarray(hist, dtype=np.int32)
            assert hist.ndim == 2 and hist.shape[0] == n, hist.shape
            io.hist_host, io.hist_stride = arr(hist, np.int32), hist.shape[1]
        io.temperature, io.seed = float(temperature), int(seed) & 0xFFFFFFFF
        res: Dict[str, object] = {}
        if form in ("step", "rows"):
            io.positions_host = arr(np.atleast_1d(positions), np.int32, (1,) if form == "step" else (n,))
            if prompt is not None:
                prompt = np.ascontiguousarray(prompt, dtype=np.int32)
                assert prompt.ndim == 2 and prompt.shape[0] == n, prompt.shape
                io.prompt_host, io.max_prompt = arr(prompt, np.int32), prompt.shape[1]
                io.prompt_len_host = arr(prompt_len, np.int32, (n,))
            io.done_host, io.row_cap_host = arr(done, np.int32, (n,)), arr(row_cap, np.int32, (n,))
            io.sum_logprob_host, io.n_done = arr(sum_logprob, np.float32, (n,)), int(n_done)
            for f in ("cur_tok", "n_sampled", "last_tok", "pen_tok", "last_ts", "done"):
                res[f] = out("out_" + f, n, np.int32)
            res["positions"] = out("out_positions", 2 if form == "step" else n, np.int32)
            res["n_done"] = out("out_n_done", 1, np.int32)
            res["sum_logprob"], res["no_speech"] = out("out_sum_logprob", n, np.float32), out("out_no_speech", n, np.float32)
            res["out_tokens"] = out("out_tokens", (n, opts.max_new_tokens), np.int32)
        elif form == "session":
            ent = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1, 4)
            io.entries_host, io.n_entries = arr(ent, np.int32), len(ent)
            io.entry_temp_host, io.entry_seed_host = arr(entry_temp, np.float32, (len(ent),)), arr(entry_seed, np.uint32, (len(ent),))
            raw = out("out_f32", (len(ent), 3), np.float32)
        elif form == "topk":
            io.k, io.want_no_speech = int(k), int(bool(want_no_speech))
            res["lp"], res["id"] = out("out_f32", (n, k), np.float32), out("out_i32", (n, k), np.int32)
            if want_no_speech:
                res["no_speech"] = out("out_no_speech", n, np.float32)
        elif form == "logprob":
            io.targets_host = arr(targets, np.int32, (n,))
            res["out"] = out("out_f32", n, np.float32)
        elif form == "prob":
            io.token = int(token)
            res["out"] = out("out_f32", n, np.float32)
        buf = C.create_string_buffer(192)
        self._check(self.lib.ttasr_select_probe(self.h, _lib.SELECT_FORMS[form], C.byref(io), buf, 192), "select_probe")
        if form == "session":
            res["choice"], res["lp"], res["no_speech"] = raw[:, 0].copy().view(np.int32), raw[:, 1].copy(), raw[:, 2].copy()
        res["sig"] = buf.value.decode()
        return res

    # -- sequence bias ---------------------------------------------------------------------------
    def set_sequence_bias(self, mapping=None):
        """Installs a sequence-bias table on this engine context ({tuple of ids: bias}, or an iterable of (ids, bias), in table
        order; None or empty clears it): ttasr_set_sequence_bias.  While installed, generate / generate_beam / generate_sample add
        the table's biases to the raw logits in front of the Whisper rules (HF SequenceBiasLogitsProcessor) and sessions are
        refused.  Everything the library would refuse raises ValueError here, before the library is called."""
        from . import seq_bias
        table = seq_bias.check_table(mapping, self.dims.vocab) if mapping else []
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        if not table:
            self._check(self.lib.ttasr_set_sequence_bias(self.h, 0, None, None, None), "set_sequence_bias")
            return
        tokens, offsets, biases = seq_bias.flatten(table)
        self._check(self.lib.ttasr_set_sequence_bias(self.h, len(table), tokens.ctypes.data_as(i32p), offsets.ctypes.data_as(i32p),
                                                     biases.ctypes.data_as(f32p)), "set_sequence_bias")

    def seq_bias_probe(self, form: str, rows: np.ndarray, hist: Optional[np.ndarray] = None, hist_len=None,
                       prompt: Optional[np.ndarray] = None, prompt_len=None, out_tokens: Optional[np.ndarray] = None,
                       n_sampled=None, done=None, position: int = 0) -> Tuple[np.ndarray, str]:
        """One launch of the sequence-bias kernel with the installed table on raw logits rows float32 [n][vocab]
        (ttasr_seq_bias_probe) -> (the processed rows, the instantiation that ran).  "window": hist int32 [n][15] with
        hist[r][15 - k] = the k-th token back and hist_len [n] = min(history length, 16) or -1 (row left alone).  "state":
        out_tokens [n][max_new] with n_sampled [n], optionally prompt [n][max_prompt] with prompt_len [n] and done [n], and the
        position of the token being fed.  The search state is undefined afterwards."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = rows.shape[0]
        assert rows.ndim == 2 and rows.shape[1] == self.dims.vocab, rows.shape
        io = _lib.SeqBiasIO()
        keep = [rows]

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.int32)
            assert a.shape == shape, (a.shape, shape)
            keep.append(a)
            return a.ctypes.data

        out = np.empty_like(rows)
        io.rows_host, io.out_rows_host, io.n, io.position = rows.ctypes.data, out.ctypes.data, n, int(position)
        if form == "window":
            io.hist_host, io.hist_len_host = arr(hist, (n, 15)), arr(hist_len, (n,))
        else:
            out_tokens = np.ascontiguousarray(out_tokens, dtype=np.int32)
            io.max_new = out_tokens.shape[1]
            io.out_tokens_host, io.n_sampled_host = arr(out_tokens, (n, io.max_new)), arr(n_sampled, (n,))
            if prompt is not None:
                prompt = np.ascontiguousarray(prompt, dtype=np.int32)
                io.max_prompt = prompt.shape[1]
                io.prompt_host, io.prompt_len_host = arr(prompt, (n, io.max_prompt)), arr(prompt_len, (n,))
            io.done_host = arr(done, (n,))
        buf = C.create_string_buffer(192)
        self._check(self.lib.ttasr_seq_bias_probe(self.h, _lib.SEQ_BIAS_FORMS[form], C.byref(io), buf, 192), "seq_bias_probe")
        return out, buf.value.decode()

    # -- audio enhancement ("dspMode") ------------------------------------------------------------
    def _dsp_params(self, params, fields):
        from . import dsp
        p = params if params is not None else dsp.DspParams()
        own = {k: v for k, v in fields.items() if k != "flags"}   # flags=: the raw TTASR_DSP_* word, as given (tests of the refusals)
        if own:
            p = dsp.replace(p, **own)
        c = _lib.DspParamsC()
        c.strength_db, c.oversubtract, c.peak_target, c.max_gain = p.strength_db, p.oversubtract, p.peak_target, p.max_gain
        c.flags = int(fields["flags"]) if "flags" in fields else p.flags
        return c

    def enhance(self, audios: Sequence[np.ndarray], params=None, return_gain: bool = False, **fields):
        """Denoise, high-pass and level float32 mono 16 kHz recordings on the device (ttasr_enhance; dsp.DspParams, or its fields
        as keywords, default all three stages): a list of float32 arrays of the inputs' lengths; return_gain=True: (that list,
        the level gains float32 [n]).  A recording's result depends on its samples and the parameters alone, bit for bit.  The
        parameters go to the library as given: what it refuses raises TtasrError."""
        p = self._dsp_params(params, fields)
        pcm = []
        for i, a in enumerate(audios):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"recording {i}: PCM must be one-dimensional, got shape {a.shape}")
            pcm.append(a)
        n = len(pcm)
        outs = [np.empty_like(a) for a in pcm]
        gain = np.ones(n, dtype=np.float32)
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if len(a) else None for a in pcm])
        optrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if len(a) else None for a in outs])
        ns = np.asarray([len(a) for a in pcm], dtype=np.int64)
        self._check(self.lib.ttasr_enhance(self.h, n, ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p), optrs,
                                           gain.ctypes.data_as(C.POINTER(C.c_float))), "enhance")
        return (outs, gain) if return_gain else outs

    def enhance_probe(self, audio: np.ndarray, params=None, **fields) -> Dict[str, Optional[np.ndarray]]:
        """The enhancement's known-answer hook (ttasr_enhance_probe): one recording through the launchers Engine.enhance runs ->
        {"S", "Nf", "G": float32 [T][257] (None for a recording shorter than 512 samples), "out": the result BEFORE the level
        stage}."""
        p = self._dsp_params(params, fields)
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"PCM must be one-dimensional, got shape {a.shape}")
        T = int(self.lib.ttasr_enhance_frames(len(a)))
        if T < 0:
            raise ValueError(f"{len(a)} samples: not a length ttasr_enhance takes")
        res: Dict[str, Optional[np.ndarray]] = {k: (np.zeros((T, 257), dtype=np.float32) if T else None) for k in ("S", "Nf", "G")}
        res["out"] = np.zeros(len(a), dtype=np.float32)
        ptr = lambda v: v.ctypes.data if v is not None and v.size else None   # noqa: E731
        self._check(self.lib.ttasr_enhance_probe(self.h, ptr(a), len(a), C.byref(p), ptr(res["S"]), ptr(res["Nf"]), ptr(res["G"]),
                                                 ptr(res["out"])), "enhance_probe")
        return res

    # -- measurement ---------------------------------------------------------------------------
    def phase_ms(self) -> Dict[str, float]:
        a = (C.c_float * 4)()
        self._check(self.lib.ttasr_phase_ms(self.h, a), "phase_ms")
        return dict(mel=a[0], encoder=a[1], cross_kv=a[2], decode=a[3])

    def beam_profile(self) -> Dict[str, float]:
        """Host-side split of the last beam search (ttasr_beam_profile): ms enqueueing / waiting for the GPU / selecting, positions."""
        a = (C.c_float * 4)()
        self._check(self.lib.ttasr_beam_profile(self.h, a), "beam_profile")
        return dict(enqueue_ms=a[0], gpu_wait_ms=a[1], host_select_ms=a[2], positions=int(a[3]))

    def encoder_kernel_ms(self) -> Dict[str, float]:
        """Per-class in-situ times of the last encode() run with option enc_kernel_timing = 1 (ttasr_encoder_kernel_ms)."""
        a = (C.c_float * 8)()
        self._check(self.lib.ttasr_encoder_kernel_ms(self.h, a), "encoder_kernel_ms")
        return dict(zip(("conv", "layernorm", "qkv", "attention", "out_proj", "fc1", "fc2", "cross_kv"), (float(v) for v in a)))

    def bench_kernel(self, name: str, B: int, iters: int = 20) -> Dict[str, float]:
        ms, by, fl = C.c_float(), C.c_double(), C.c_double()
        self._check(self.lib.ttasr_bench_kernel(self.h, name.encode(), B, iters, C.byref(ms), C.byref(by), C.byref(fl)),
                    f"bench_kernel({name})")
        buf = C.create_string_buffer(256)
        self._check(self.lib.ttasr_bench_kernel_signature(self.h, buf, 256), "bench_kernel_signature")
        return dict(ms=ms.value, bytes=by.value, flops=fl.value, signature=buf.value.decode())

    def sync(self):
        self._check(self.lib.ttasr_sync(self.h), "sync")


@dataclass
class AlignBatchResult:
    """Engine.align_batch / Session.align: per sequence the start frame (encoder frames of 20 ms) of the token each row
    first_row .. n_tokens - 2 predicts, and log p(tokens[t + 1] | tokens[..t]) for t = 0 .. n_tokens - 2; with debug=True also
    the cost matrices [rows][F] and the raw attention maps [n_pairs][n_tokens][audio_ctx]."""
    start_frames: List[np.ndarray]
    logprobs: List[np.ndarray]
    costs: Optional[List[np.ndarray]] = None
    weights: Optional[List[np.ndarray]] = None


def _align_batch_args(engine: "Engine", tokens, first_row, num_frames, heads, medfilt_width):
    """Validates and packs the arguments ttasr_align_batch / ttasr_session_align share (raises ValueError before the library
    is called) -> (tok [n][max_tokens], n_tokens, first_row, num_frames, pairs)."""
    n = len(tokens)
    if n < 1 or n > engine.max_batch:
        raise ValueError(f"{n} sequences outside [1, max_batch = {engine.max_batch}]")
    if len(first_row) != n or len(num_frames) != n:
        raise ValueError(f"need one first_row and one num_frames per sequence ({n}), got {len(first_row)} and {len(num_frames)}")
    medfilt_width = int(medfilt_width)
    if not 1 <= medfilt_width <= 15 or medfilt_width % 2 == 0:
        raise ValueError(f"medfilt_width {medfilt_width} must be odd and in [1, 15]")
    d = engine.dims
    tok_max = min(d.n_text_ctx, d.n_audio_ctx)
    nt = np.asarray([len(t) for t in tokens], dtype=np.int32)
    if nt.min() < 2 or nt.max() > tok_max:
        raise ValueError(f"every sequence needs between 2 and {tok_max} tokens, got {nt.min()} .. {nt.max()}")
    if n * int(nt.max()) > engine.max_batch * d.n_audio_ctx:
        raise ValueError(f"{n} sequences x {nt.max()} positions exceed the pass's {engine.max_batch * d.n_audio_ctx} rows")
    fr = np.ascontiguousarray(first_row, dtype=np.int32)
    nf = np.ascontiguousarray(num_frames, dtype=np.int32)
    if fr.shape != (n,) or nf.shape != (n,):
        raise ValueError("first_row and num_frames must be one-dimensional")
    if np.any(fr < 0) or np.any(fr > nt - 2):
        raise ValueError("first_row entries must lie in [0, n_tokens - 2]")
    if nf.min() < 0:
        raise ValueError("num_frames entries must be >= 0")
    tok = np.zeros((n, int(nt.max())), dtype=np.int32)
    for i, t in enumerate(tokens):
        tok[i, :len(t)] = t
        if min(t) < 0 or max(t) >= d.vocab:
            raise ValueError(f"sequence {i}: token outside the vocabulary")
    pr = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1, 2)
    if len(pr) < 1:
        raise ValueError("need at least one alignment head")
    if np.any(pr < 0) or np.any(pr[:, 0] >= d.dec_layers) or np.any(pr[:, 1] >= d.n_heads):
        raise ValueError("alignment head outside the decoder")
    if len({(int(l), int(h)) for l, h in pr}) != len(pr):
        raise ValueError("an alignment head is listed twice")
    return tok, nt, fr, nf, pr, medfilt_width


def _align_batch_call(engine: "Engine", fn, what: str, lead, packed, debug: bool) -> AlignBatchResult:
    tok, nt, fr, nf, pr, width = packed
    n, mt = tok.shape
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    start = np.zeros((n, mt), dtype=np.int32)
    lp = np.zeros((n, mt), dtype=np.float32)
    cost = np.zeros((n, mt, engine.audio_ctx), dtype=np.float32) if debug else None
    w = np.zeros((n, len(pr), mt, engine.audio_ctx), dtype=np.float32) if debug else None
    engine._check(fn(engine.h, n, lead, tok.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), mt, fr.ctypes.data_as(i32p),
                     nf.ctypes.data_as(i32p), pr.ctypes.data_as(i32p), len(pr), width, start.ctypes.data_as(i32p),
                     lp.ctypes.data_as(f32p), cost.ctypes.data_as(f32p) if debug else None,
                     w.ctypes.data_as(f32p) if debug else None), what)
    rows = nt - 1 - fr
    frames = np.minimum(engine.audio_ctx, np.maximum(1, nf // 2))
    return AlignBatchResult(
        [start[i, :rows[i]].copy() for i in range(n)], [lp[i, :nt[i] - 1].copy() for i in range(n)],
        [cost[i, :rows[i], :frames[i]].copy() for i in range(n)] if debug else None,
        [w[i, :, :nt[i]].copy() for i in range(n)] if debug else None)


def session_prefill_positions(prompt_len: int, sot_index: Optional[int], threshold: int, placeholder: bool = False) -> int:
    """The per-clip rule of option session_prefill, as the library applies it at admission (csrc/prefill_tables.hpp): how many
    leading prompt positions an admission pass computes, 0 = the clip is forced token by token.  sot_index = the clip's
    <|startoftranscript|> index when the no-speech probability is wanted (that position stays a real step), else None;
    placeholder = the prompt carries Session.DETECT (never prefilled)."""
    if threshold <= 0 or placeholder:
        return 0
    p = prompt_len - 1
    if sot_index is not None and sot_index >= 0:
        p = min(p, sot_index)
    return p if p >= threshold else 0


def session_prefill_value(v) -> int:
    """session_prefill keyword -> option value: False / None / 0 off, True = config.SESSION_PREFILL_DEFAULT, else the integer."""
    from .config import SESSION_PREFILL_DEFAULT
    if v is None or v is False:
        return 0
    if v is True:
        return SESSION_PREFILL_DEFAULT
    v = int(v)
    if v < 0:
        raise ValueError(f"session_prefill {v} must be >= 0")
    return v


@dataclass
class SessionResult:
    id: int
    tokens: List[int]
    sum_logprob: float
    no_speech_prob: float
    language: Optional[int] = None               # index into the session's language span; None: the clip carried no placeholder
    language_probs: Optional[np.ndarray] = None  # float32 [n_lang] softmax over the span
    language_logits: Optional[np.ndarray] = None # float32 [n_lang] raw span logits


class Session:
    """Engine.session(): submit(clips, prompts, max_new) -> clip ids; poll() -> finished clips (SessionResult, any order)."""

    DETECT = -1   # TTASR_TOKEN_DETECT: the language placeholder of an armed session's prompts

    def __init__(self, engine: Engine, opts, max_prompt: int, temperature: float = 0.0, beam: int = 1,
                 patience: Optional[float] = None, detect_language=False, prefill: int = 0):
        self.engine, self.opts, self.max_prompt = engine, opts, int(max_prompt)
        self.prefill = session_prefill_value(prefill)
        self.max_new_tokens = int(opts.max_new_tokens)
        self.window = 2 * engine.audio_ctx * 160
        self.open = False
        self.holding = False
        self.pending = 0
        self.lang_span: Optional[Tuple[int, int, int]] = None   # (sot, first language token, count) once armed
        beam = int(beam)
        if not 1 <= beam <= 7:
            raise ValueError(f"beam {beam} outside [1, 7]")
        self.beam = beam if (beam > 1 or patience is not None) else 0   # 0: the greedy session
        if self.beam:
            patience = 1.0 if patience is None else float(patience)
            if not patience > 0:
                raise ValueError(f"patience {patience} must be > 0")
            if temperature != 0.0:
                raise ValueError("a beam session decodes without sampling (temperature must be 0)")
            if beam > engine.max_batch:
                raise ValueError(f"max_batch {engine.max_batch} holds no group of {beam} rows")
        # the option is read by session_begin; the keyword owns it for this session: the value the engine had is put back at close()
        # (a refused begin puts it back at once).  Nothing is called when the option already has the value.
        self._prefill_before = int(getattr(engine, "_session_prefill", 0))
        if self.prefill != self._prefill_before:
            engine.set_option("session_prefill", self.prefill)
        try:
            if self.beam:
                rc, what = engine.lib.ttasr_session_begin_beam(engine.h, C.byref(opts), self.max_prompt, beam, C.c_float(patience)), \
                    "session_begin_beam"
            else:
                rc, what = engine.lib.ttasr_session_begin(engine.h, C.byref(opts), self.max_prompt, C.c_float(temperature)), \
                    "session_begin"
            self.open = rc == 0
        finally:
            if self.prefill != self._prefill_before and not self.open:
                engine.set_option("session_prefill", self._prefill_before)
        engine._check(rc, what)
        if detect_language:   # armed before the first submit; a refusal closes the session again
            try:
                if detect_language is True:
                    span = (engine.special.sot,) + tuple(engine.language_span())
                else:
                    span = tuple(int(v) for v in detect_language)
                    if len(span) != 3:
                        raise ValueError("detect_language is True or (sot, first language token, count)")
                engine._check(engine.lib.ttasr_session_detect_language(engine.h, span[0], span[1], span[2]),
                              "session_detect_language")
                self.lang_span = span
            except Exception:
                self.close()
                raise

    def __enter__(self) -> "Session":
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.open:
            self.open = False
            self.engine._check(self.engine.lib.ttasr_session_end(self.engine.h), "session_end")
            if self.prefill != self._prefill_before:   # options are refused while a session is open: put back here, behind its end
                self.engine.set_option("session_prefill", self._prefill_before)

    def submit(self, clips: Sequence[np.ndarray], prompts: Sequence[Sequence[int]], max_new: Optional[Sequence[int]] = None
               ) -> List[int]:
        """Queue clips (float32 PCM, at most one window each) with one prompt each; max_new = per-clip token budgets in
        [1, opts.max_new_tokens] (default: opts.max_new_tokens).  Shapes and budgets are checked here before the library is called."""
        if not self.open:
            raise TtasrError("session is closed")
        n = len(clips)
        if n < 1 or len(prompts) != n:
            raise ValueError(f"need >= 1 clip and one prompt per clip (clips {n}, prompts {len(prompts)})")
        caps = np.full(n, self.max_new_tokens, dtype=np.int32) if max_new is None else np.ascontiguousarray(max_new, dtype=np.int32)
        if caps.shape != (n,):
            raise ValueError(f"max_new needs one entry per clip ({n}), got shape {caps.shape}")
        if caps.min() < 1 or caps.max() > self.max_new_tokens:
            raise ValueError(f"max_new entries must lie in [1, {self.max_new_tokens}]")
        pcm = []
        for i, c in enumerate(clips):
            a = np.ascontiguousarray(c, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"clip {i}: PCM must be one-dimensional, got shape {a.shape}")
            if len(a) > self.window:
                raise ValueError(f"clip {i}: {len(a)} samples is longer than one window ({self.window})")
            pcm.append(a)
        pr = np.zeros((n, self.max_prompt), dtype=np.int32)
        pl = np.zeros(n, dtype=np.int32)
        for i, p in enumerate(prompts):
            if not 1 <= len(p) <= self.max_prompt:
                raise ValueError(f"clip {i}: prompt length {len(p)} outside [1, {self.max_prompt}]")
            pr[i, :len(p)] = p
            pl[i] = len(p)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        ns = np.asarray([len(a) for a in pcm], dtype=np.int64)
        ids = np.zeros(n, dtype=np.int64)
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self.engine._check(self.engine.lib.ttasr_session_submit(
            self.engine.h, n, ptrs, ns.ctypes.data_as(i64p), pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p),
            caps.ctypes.data_as(i32p), ids.ctypes.data_as(i64p)), "session_submit")
        self.pending += n
        return ids.tolist()

    def submit_windows(self, files: Sequence[np.ndarray], seeks: Sequence[int], prompts: Sequence[Sequence[int]],
                       sot_index: Sequence[int], max_new: Optional[Sequence[int]] = None,
                       floor_max: Optional[Sequence[float]] = None, temperature: Optional[Sequence[float]] = None,
                       rows: Optional[Sequence[int]] = None, seed: Optional[Sequence[int]] = None) -> List[int]:
        """Queue 30-s windows of recordings (beam sessions only; ttasr_session_submit_windows): window i starts at 10-ms frame
        seeks[i] of files[i] (float32 PCM), with its prompt, <|startoftranscript|> index, budget (default opts.max_new_tokens),
        dynamic-range maximum (floor_max, default: the window's own), temperature (default 0), rows (default: the session's
        beam width) and sampling seed (default 0).  Temperature 0 with rows > 1 is beam search; one row at temperature 0 is
        greedy; temperature > 0 draws `rows` samples.  Shapes and ranges are checked here before the library is called."""
        if not self.open:
            raise TtasrError("session is closed")
        if not self.beam:
            raise ValueError("window clips need a beam session (Engine.session(beam=..., patience=...))")
        n = len(files)
        if n < 1 or any(len(x) != n for x in (seeks, prompts, sot_index)):
            raise ValueError(f"need >= 1 window and one seek, prompt and sot index per window (files {n}, seeks {len(seeks)}, "
                             f"prompts {len(prompts)}, sot_index {len(sot_index)})")

        def per_window(v, default, dtype, name):
            a = np.full(n, default, dtype=dtype) if v is None else np.ascontiguousarray(v, dtype=dtype)
            if a.shape != (n,):
                raise ValueError(f"{name} needs one entry per window ({n}), got shape {a.shape}")
            return a
        caps = per_window(max_new, self.max_new_tokens, np.int32, "max_new")
        if caps.min() < 1 or caps.max() > self.max_new_tokens:
            raise ValueError(f"max_new entries must lie in [1, {self.max_new_tokens}]")
        sk = per_window(seeks, 0, np.int64, "seeks")
        temps = per_window(temperature, 0.0, np.float32, "temperature")
        if not (np.all(np.isfinite(temps)) and temps.min() >= 0):
            raise ValueError("temperatures must be finite and >= 0")
        rw = per_window(rows, self.beam, np.int32, "rows")
        if rw.min() < 1 or rw.max() > self.beam:
            raise ValueError(f"rows entries must lie in [1, {self.beam}] (the session's group width)")
        sd = per_window(seed, 0, np.int64, "seed")
        if sd.min() < 0 or sd.max() > 0xFFFFFFFF:
            raise ValueError("seeds must lie in [0, 2**32)")
        sd = sd.astype(np.uint32)
        fm = None if floor_max is None else per_window(floor_max, 0.0, np.float32, "floor_max")
        if fm is not None and not np.all(np.isfinite(fm)):
            raise ValueError("floor_max entries must be finite")
        pcm = []
        for i, f in enumerate(files):
            a = np.ascontiguousarray(f, dtype=np.float32)
            if a.ndim != 1:
                raise ValueError(f"window {i}: PCM must be one-dimensional, got shape {a.shape}")
            if not 0 <= sk[i] * 160 < len(a):
                raise ValueError(f"window {i}: seek {sk[i]} lies outside the recording ({len(a)} samples)")
            pcm.append(a)
        pr = np.zeros((n, self.max_prompt), dtype=np.int32)
        pl = np.zeros(n, dtype=np.int32)
        so = per_window(sot_index, 0, np.int32, "sot_index")
        for i, p in enumerate(prompts):
            if not 1 <= len(p) <= self.max_prompt:
                raise ValueError(f"window {i}: prompt length {len(p)} outside [1, {self.max_prompt}]")
            if not 0 <= so[i] < len(p):
                raise ValueError(f"window {i}: sot_index {so[i]} outside the {len(p)}-token prompt")
            pr[i, :len(p)] = p
            pl[i] = len(p)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in pcm])
        ns = np.asarray([len(a) for a in pcm], dtype=np.int64)
        ids = np.zeros(n, dtype=np.int64)
        i32p, i64p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
        self.engine._check(self.engine.lib.ttasr_session_submit_windows(
            self.engine.h, n, ptrs, ns.ctypes.data_as(i64p), sk.ctypes.data_as(i64p), fm.ctypes.data_as(f32p) if fm is not None else None,
            pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p), so.ctypes.data_as(i32p), caps.ctypes.data_as(i32p),
            temps.ctypes.data_as(f32p), rw.ctypes.data_as(i32p), sd.ctypes.data_as(C.POINTER(C.c_uint32)), ids.ctypes.data_as(i64p)),
            "session_submit_windows")
        self.pending += n
        return ids.tolist()

    def poll(self, max_steps: int = 1 << 30, cap: Optional[int] = None, with_language: bool = True) -> List[SessionResult]:
        """Admit ready clips, decode until at least one clip finished (or nothing is left, or max_steps steps ran); returns the
        finished clips (at most `cap`, default max_batch).  An armed session returns each clip's language too
        (ttasr_session_poll_lang); with_language=False takes the plain poll, which drops it."""
        if not self.open:
            raise TtasrError("session is closed")
        cap = self.engine.max_batch if cap is None else int(cap)
        if cap < 1 or max_steps < 1:
            raise ValueError("cap and max_steps must be >= 1")
        ids = np.zeros(cap, dtype=np.int64)
        toks = np.zeros((cap, self.max_new_tokens), dtype=np.int32)
        lens = np.zeros(cap, dtype=np.int32)
        lp = np.zeros(cap, dtype=np.float32)
        nsp = np.zeros(cap, dtype=np.float32)
        n_out = C.c_int32(0)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        if self.lang_span is not None and with_language:   # only an armed session calls the entry point that returns languages
            n_lang = self.lang_span[2]
            lang = np.full(cap, -1, dtype=np.int32)
            probs = np.zeros((cap, n_lang), dtype=np.float32)
            logits = np.zeros((cap, n_lang), dtype=np.float32)
            self.engine._check(self.engine.lib.ttasr_session_poll_lang(
                self.engine.h, int(min(max_steps, 2**31 - 1)), cap, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), nsp.ctypes.data_as(f32p),
                lang.ctypes.data_as(i32p), probs.ctypes.data_as(f32p), logits.ctypes.data_as(f32p), C.byref(n_out)),
                "session_poll_lang")
            k = n_out.value
            self.pending -= k
            return [SessionResult(int(ids[i]), toks[i, :lens[i]].tolist(), float(lp[i]), float(nsp[i]),
                                  int(lang[i]) if lang[i] >= 0 else None, probs[i].copy() if lang[i] >= 0 else None,
                                  logits[i].copy() if lang[i] >= 0 else None) for i in range(k)]
        self.engine._check(self.engine.lib.ttasr_session_poll(
            self.engine.h, int(min(max_steps, 2**31 - 1)), cap, ids.ctypes.data_as(C.POINTER(C.c_int64)), toks.ctypes.data_as(i32p),
            lens.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), nsp.ctypes.data_as(f32p), C.byref(n_out)), "session_poll")
        k = n_out.value
        self.pending -= k
        return [SessionResult(int(ids[i]), toks[i, :lens[i]].tolist(), float(lp[i]), float(nsp[i])) for i in range(k)]

    def drain(self) -> List[SessionResult]:
        """Poll until every submitted clip has finished."""
        out: List[SessionResult] = []
        while self.pending > 0:
            got = self.poll()
            if not got:
                raise TtasrError(f"session idle with {self.pending} clips unfinished")
            out.extend(got)
        return out

    def hold(self, on: bool = True):
        """Hold mode (ttasr_session_hold): a clip that finishes keeps its row (beam: group) and cross-KV slot until align() or
        release(); the caller must do one of the two for every clip poll() returns, or queued clips cannot start.  Not
        available with option refill_overlap = 1.  hold(False) releases whatever is held."""
        if not self.open:
            raise TtasrError("session is closed")
        self.engine._check(self.engine.lib.ttasr_session_hold(self.engine.h, 1 if on else 0), "session_hold")
        self.holding = bool(on)

    def _ids(self, ids) -> np.ndarray:
        if not self.open:
            raise TtasrError("session is closed")
        if not getattr(self, "holding", False):
            raise ValueError("hold mode is off (Session.hold() first)")
        a = np.ascontiguousarray(ids, dtype=np.int64)
        if a.ndim != 1 or not 1 <= len(a) <= self.engine.max_batch:
            raise ValueError(f"need between 1 and {self.engine.max_batch} clip ids")
        if len(set(a.tolist())) != len(a):
            raise ValueError("a clip id is listed twice")
        return a

    def align(self, ids: Sequence[int], tokens: Sequence[Sequence[int]], first_row: Sequence[int], num_frames: Sequence[int],
              heads: Sequence[Tuple[int, int]], medfilt_width: int = 7, debug: bool = False) -> AlignBatchResult:
        """Engine.align_batch for held clips (ttasr_session_align): sequence i belongs to the held clip ids[i]; the clips are
        released when the call has succeeded.  Arguments are checked here before the library is called."""
        a = self._ids(ids)
        if len(tokens) != len(a):
            raise ValueError(f"need one token sequence per clip id ({len(a)}), got {len(tokens)}")
        packed = _align_batch_args(self.engine, tokens, first_row, num_frames, heads, medfilt_width)
        return _align_batch_call(self.engine, self.engine.lib.ttasr_session_align, "session_align",
                                 a.ctypes.data_as(C.POINTER(C.c_int64)), packed, debug)

    def release(self, ids: Sequence[int]):
        """Free held clips without aligning them (ttasr_session_release)."""
        a = self._ids(ids)
        self.engine._check(self.engine.lib.ttasr_session_release(self.engine.h, len(a), a.ctypes.data_as(C.POINTER(C.c_int64))),
                           "session_release")

    def retry(self, ids: Sequence[int], prompts: Sequence[Sequence[int]], sot_index: Sequence[int],
              max_new: Optional[Sequence[int]] = None, temperature: Optional[Sequence[float]] = None,
              rows: Optional[Sequence[int]] = None, seed: Optional[Sequence[int]] = None) -> List[int]:
        """A new search on held clips with no encoder work (beam sessions only; ttasr_session_retry): the group of held clip
        ids[i] starts over under a new clip id (returned; the old id stops being held) with its own prompt,
        <|startoftranscript|> index, budget (default opts.max_new_tokens), temperature (default 0), rows (default: the
        session's beam width) and seed (default 0), all as in submit_windows.  The clip's cross-KV slot is reused as it is.
        The language placeholder is refused: the language is known by then.  Shapes and ranges are checked here before the
        library is called."""
        if self.open and not self.beam:
            raise ValueError("a retry needs a beam session (Engine.session(beam=..., patience=...))")
        a = self._ids(ids)
        n = len(a)
        if any(len(x) != n for x in (prompts, sot_index)):
            raise ValueError(f"need one prompt and sot index per clip id ({n}), got prompts {len(prompts)}, sot_index {len(sot_index)}")

        def per_clip(v, default, dtype, name):
            b = np.full(n, default, dtype=dtype) if v is None else np.ascontiguousarray(v, dtype=dtype)
            if b.shape != (n,):
                raise ValueError(f"{name} needs one entry per clip id ({n}), got shape {b.shape}")
            return b
        caps = per_clip(max_new, self.max_new_tokens, np.int32, "max_new")
        if caps.min() < 1 or caps.max() > self.max_new_tokens:
            raise ValueError(f"max_new entries must lie in [1, {self.max_new_tokens}]")
        temps = per_clip(temperature, 0.0, np.float32, "temperature")
        if not (np.all(np.isfinite(temps)) and temps.min() >= 0):
            raise ValueError("temperatures must be finite and >= 0")
        rw = per_clip(rows, self.beam, np.int32, "rows")
        if rw.min() < 1 or rw.max() > self.beam:
            raise ValueError(f"rows entries must lie in [1, {self.beam}] (the session's group width)")
        sd = per_clip(seed, 0, np.int64, "seed")
        if sd.min() < 0 or sd.max() > 0xFFFFFFFF:
            raise ValueError("seeds must lie in [0, 2**32)")
        sd = sd.astype(np.uint32)
        so = per_clip(sot_index, 0, np.int32, "sot_index")
        pr = np.zeros((n, self.max_prompt), dtype=np.int32)
        pl = np.zeros(n, dtype=np.int32)
        for i, p in enumerate(prompts):
            if not 1 <= len(p) <= self.max_prompt:
                raise ValueError(f"clip {i}: prompt length {len(p)} outside [1, {self.max_prompt}]")
            if not 0 <= so[i] < len(p):
                raise ValueError(f"clip {i}: sot_index {so[i]} outside the {len(p)}-token prompt")
            if any(int(t) == self.DETECT for t in p):
                raise ValueError(f"clip {i}: a retried clip's prompt cannot hold the language placeholder")
            pr[i, :len(p)] = p
            pl[i] = len(p)
        out = np.zeros(n, dtype=np.int64)
        i32p, i64p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
        self.engine._check(self.engine.lib.ttasr_session_retry(
            self.engine.h, n, a.ctypes.data_as(i64p), pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p), so.ctypes.data_as(i32p),
            caps.ctypes.data_as(i32p), temps.ctypes.data_as(f32p), rw.ctypes.data_as(i32p),
            sd.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(i64p)), "session_retry")
        self.pending += n
        return out.tolist()

    def rows(self) -> Dict[str, np.ndarray]:
        """The batch's rows now (ttasr_session_rows): position, finished flag (1 = finished or free), clip id (-1 = free)."""
        B = self.engine.max_batch
        pos, done, clip = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int64)
        i32p = C.POINTER(C.c_int32)
        self.engine._check(self.engine.lib.ttasr_session_rows(self.engine.h, pos.ctypes.data_as(i32p), done.ctypes.data_as(i32p),
                                                              clip.ctypes.data_as(C.POINTER(C.c_int64))), "session_rows")
        return dict(row_pos=pos, done=done, clip=clip)

    def stats(self) -> Dict[str, float]:
        a = (C.c_double * 8)()
        self.engine._check(self.engine.lib.ttasr_session_stats(self.engine.h, a), "session_stats")
        out = dict(zip(("steps", "polls", "encodes", "clips_encoded", "live_row_steps", "encode_ms", "decode_ms", "queued"),
                       (float(v) for v in a)))
        b = (C.c_double * 4)()   # the admission passes of option session_prefill (all 0 with the option off)
        self.engine._check(self.engine.lib.ttasr_session_prefill_stats(self.engine.h, b), "session_prefill_stats")
        out.update(zip(("prefill_passes", "prefill_clips", "prefill_positions", "prefill_ms"), (float(v) for v in b)))
        return out
