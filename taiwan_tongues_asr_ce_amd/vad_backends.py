"""Plugin-level drop-in: the reference's VAD adapter interface (api/stt_streaming/src/vad/vad_interface.py:1-16,
vad_factory.py:7-44, simple_vad.py:7-45, pyannote_vad.py:12-62) with two MI355X backends: the streaming Silero-shaped one
registered under "silero" / "mi355x_silero" and the PyanNet-shaped segmentation one under "pyannote" / "mi355x_pyannote".  The
streaming server's `VADFactory.create_vad_pipeline(args.vad_type, **vad_args)` call (main.py:196) needs no change beyond the type
and `vad_model`.

The server's trigger (SilenceAtEndOfChunk, buffering_strategies.py:110-126; streaming.should_transcribe) asks
`vad_pipeline.detect_activity(client)` for the voiced segments of the client's WHOLE scratch buffer after every chunk.  The
reference's real VAD writes that buffer to a wav file and runs its network over all of it each time; `DeviceStreamVAD` keeps one
device stream per client (Engine.vad_stream_*), evaluates only the samples that arrived since the last call, and puts the calls
of all clients that arrive together into one device push."""
from __future__ import annotations

import asyncio
import logging
import threading
import zlib
from typing import Any, Dict, List, Optional

from . import vad
from .asr import pcm16_bytes_to_float

logger = logging.getLogger(__name__)


class VADInterface:
    async def detect_activity(self, client) -> List[Dict[str, float]]:
        """[{"start", "end", "confidence"}] in seconds, of client.scratch_buffer (vad_interface.py:6-16)."""
        raise NotImplementedError("This method should be implemented by subclasses.")


class SimpleVAD(VADInterface):
    """All audio is speech (simple_vad.py:22-45): [] for an empty buffer and for one shorter than min_duration, else one segment
    over the whole buffer."""

    def __init__(self, **kwargs):
        self.min_duration = kwargs.get("min_duration", 0.1)   # simple_vad.py:19

    async def detect_activity(self, client):
        if len(client.scratch_buffer) == 0:
            return []
        duration = len(client.scratch_buffer) / (client.sampling_rate * client.samples_width)
        if duration < self.min_duration:
            return []
        return [{"start": 0.0, "end": duration, "confidence": 1.0}]


# pyannote_vad.py:37-45 instantiates its pipeline with onset / offset 0.5 and 0.3 s minimum on and off.  faster-whisper's own
# default of 2 s of silence never closes a segment inside the 3-s buffers the trigger looks at.
DEFAULT_STREAM_VAD_OPTIONS = dict(threshold=0.5, min_speech_duration_ms=300, min_silence_duration_ms=300, speech_pad_ms=0)


class _Coalescer:
    """The coalescing worker the device backends share: `submit(key, payload)` calls that arrive within `max_wait` seconds go
    into ONE batch [(key, payload, future)], handed to the coroutine `run_batch`, which resolves the futures.  A key takes one
    row of a batch (a second call with the same key goes into the next one), and a batch does not wait once `n_known()` keys are
    in it.  A new event loop gets its own queue and worker."""

    def __init__(self, max_wait: float, n_known, run_batch):
        self.max_wait, self.n_known, self.run_batch = max_wait, n_known, run_batch
        self._queue: Optional[asyncio.Queue] = None
        self._task: Optional[asyncio.Task] = None
        self._loop = None

    async def submit(self, key, payload):
        loop = asyncio.get_running_loop()
        if self._loop is not loop:   # a new event loop: its own queue and worker
            self._loop, self._queue, self._task = loop, asyncio.Queue(), None
        if self._task is None or self._task.done():
            self._task = loop.create_task(self._worker())
        fut = loop.create_future()
        await self._queue.put((key, payload, fut))
        return await fut

    def cancel(self) -> None:
        if self._task is not None and not self._task.done():
            self._task.cancel()
        self._task = None

    async def _worker(self):
        loop = asyncio.get_running_loop()
        held: list = []
        while True:
            batch: list = []
            carry: list = []

            def place(item):   # a key takes one row of a batch: a second call of the same client goes into the next one
                (carry if any(item[0] is b[0] for b in batch) else batch).append(item)

            for item in held or [await self._queue.get()]:
                place(item)
            deadline = loop.time() + self.max_wait
            while len(batch) < self.n_known():   # every known client is in: nobody to wait for
                timeout = deadline - loop.time()
                if timeout <= 0:
                    break
                try:
                    place(await asyncio.wait_for(self._queue.get(), timeout))
                except asyncio.TimeoutError:
                    break
            held = carry
            await self.run_batch(batch)


class _ClientStream:
    """One client's stream: the detector, how many bytes of its scratch buffer the stream has consumed, and their CRC."""
    __slots__ = ("detector", "consumed", "crc", "needs_reset", "wire")

    def __init__(self, wire: Optional[vad.WireFormat] = None):
        self.detector: Optional[vad.StreamingSpeechDetector] = None   # opened by the first push
        self.consumed = 0
        self.crc = 0
        self.needs_reset = False
        self.wire = wire              # None: 16 kHz mono s16 through the float push


class DeviceStreamVAD(VADInterface):
    """VADInterface backend on the device's stateful streaming VAD.

    One stream per `client.client_id`, opened on first sight.  Each `detect_activity` converts and pushes only the bytes of
    `client.scratch_buffer` (s16le, as asr.pcm16_bytes_to_float reads them) beyond what that client's stream has consumed, and
    returns the detector's segments in seconds with confidence 1.0.  The buffering strategy clears the scratch buffer after a
    transcription (buffering_strategies.py:113,179): the backend keeps the zlib.crc32 of the consumed prefix, and when the buffer
    is shorter than what was consumed, or its prefix has another CRC, it resets the stream and starts over.  `forget(client)`
    closes a client's stream (call it when the client disconnects).

    Concurrent calls that arrive within `max_wait_ms` are coalesced into ONE Engine.vad_stream_push, which runs in an executor
    thread so the event loop stays free; a push does not wait once every known client is in it.  `pushes_run` records the rows of
    every push.  The trailing partial frame (< 32 ms) is not evaluated until it fills (vad.StreamingSpeechDetector).

    `vad_parameters`: vad.VadOptions fields over DEFAULT_STREAM_VAD_OPTIONS (the reference's pyannote arguments).

    `engine=None`: the backend owns a VAD-only context (micro geometry, no Whisper weights, max_batch=64) with `vad_model` loaded
    (a mapping, an .npz or a TorchScript / state-dict file: vad.load_silero_state), so it never contends with the ASR context's
    calls or session.  `engine=`: it shares that context - whose VAD weights are loaded already, or come from `vad_model` - and
    the caller serialises the calls; a stream cannot be OPENED while a session is open on that context (a new client's first call
    then fails), pushes and resets can.

    `wire=None`: every client sends 16 kHz mono s16, as above.  `wire=vad.WireFormat(...)`: every client sends that format;
    `wire="client"`: each client declares its own (vad.WireFormat.of_client: sampling_rate, samples_width and the optional
    channels / encoding / audio_channel attributes; width 1 without an encoding is refused).  The clients' streams are then WIRE
    streams: the raw tail of the scratch buffer goes to Engine.vad_stream_push_wire as it is - cut nowhere, a byte that ends
    inside a sample waits inside the library - and the device converts, downmixes and resamples in front of the network.  The
    segments stay in seconds of the client's audio.  `audio(client)` is the converted 16 kHz PCM that mirrors the consumed
    scratch bytes (what an ASR adapter with audio_from= transcribes): the samples whose inputs have all arrived - up to
    ceil(half / down) samples (10 periods of the lower of the two rates, 1.25 ms at 8 kHz) at the end are not final yet."""

    def __init__(self, vad_model=None, engine=None, max_wait_ms: float = 2.0, vad_parameters: Optional[Dict[str, Any]] = None,
                 wire=None, **kwargs):
        if wire is not None and wire != "client" and not isinstance(wire, vad.WireFormat):
            raise ValueError(f"wire {wire!r}: expected None, a vad.WireFormat or 'client'")
        self.wire = wire
        self.owns_engine = engine is None
        if engine is None:
            if vad_model is None:
                raise ValueError("DeviceStreamVAD needs vad_model= (the Silero-v5 tensors) or an engine= that has them loaded")
            from .config import COMPUTE_F32, PRESETS
            from .engine import Engine
            engine = Engine(PRESETS["micro"], COMPUTE_F32, 64, device=int(kwargs.get("device_index", 0)))
        if vad_model is not None and not getattr(engine, "has_vad", False):
            engine.load_vad(vad.load_silero_state(vad_model))
        self.engine = engine
        opts = dict(DEFAULT_STREAM_VAD_OPTIONS)
        opts.update(vad_parameters or {})
        self.options = vad.VadOptions(**opts)
        self.max_wait = max_wait_ms / 1000.0
        self.pushes_run: List[int] = []   # rows of the pushes actually executed (observability / tests)
        self._streams: Dict[Any, _ClientStream] = {}
        self._lock = threading.Lock()     # one engine call at a time from this object
        self._coalescer = _Coalescer(self.max_wait, lambda: len(self._streams), self._run_batch)

    # -- the reference's surface -------------------------------------------------------------------
    async def detect_activity(self, client):
        st = self._streams.get(client.client_id)
        if st is None:
            st = _ClientStream(vad.resolve_wire(self.wire, client))   # a client whose declaration is refused gets no stream
            self._streams[client.client_id] = st
        chunks = await self._coalescer.submit(st, bytes(client.scratch_buffer))
        rate = float(vad.SAMPLING_RATE)
        return [{"start": c["start"] / rate, "end": c["end"] / rate, "confidence": 1.0} for c in chunks]

    def audio(self, client, covering: Optional[bytes] = None):
        """A wire client's converted 16 kHz float32 PCM so far, or None: for a client without a wire stream, and - with
        covering= the client's scratch bytes - when the stream has not consumed exactly those bytes (another length or CRC)."""
        st = self._streams.get(getattr(client, "client_id", client))
        if st is None or st.wire is None or st.detector is None or st.needs_reset:
            return None
        if covering is not None and (len(covering) != st.consumed or zlib.crc32(bytes(covering)) != st.crc):
            return None
        return st.detector.audio

    def forget(self, client) -> None:
        st = self._streams.pop(getattr(client, "client_id", client), None)
        if st is not None and st.detector is not None:
            with self._lock:
                st.detector.close()

    def close(self) -> None:
        self._coalescer.cancel()
        for key in list(self._streams):
            self.forget(key)
        if self.owns_engine and self.engine is not None:
            self.engine.close()
        self.engine = None

    # -- coalescing ----------------------------------------------------------------------------------
    async def _run_batch(self, batch):
        loop = asyncio.get_running_loop()
        rows = [self._plan(st, buf) for st, buf, _ in batch]
        try:
            probs = await loop.run_in_executor(None, self._run_push, [st for st, _, _ in batch], rows)
        except Exception as e:
            logger.error("VAD stream push failed: %s", e)
            for st, _, fut in batch:
                st.needs_reset, st.consumed, st.crc = True, 0, 0   # start over from the whole buffer next time
                if not fut.done():
                    fut.set_exception(e)
            return
        self.pushes_run.append(len(batch))
        for (st, _, fut), (reset, new), p in zip(batch, rows, probs):
            if reset:
                st.detector.clear()
                st.consumed, st.crc = 0, 0
            st.needs_reset = False
            if st.wire is None:
                st.detector.extend(len(new) // 2, p)
            else:                      # p = (probabilities, the 16 kHz samples the bytes made final)
                st.detector.extend(len(p[1]), p[0], p[1])
            st.consumed += len(new)
            st.crc = zlib.crc32(new, st.crc)
            if not fut.done():
                fut.set_result(st.detector.segments(self.options))

    @staticmethod
    def _plan(st: _ClientStream, buf: bytes):
        """(reset, new bytes): the whole samples of `buf` behind the consumed prefix - or, when the buffer is not a continuation
        of what the stream consumed (shorter, or another CRC over the prefix), a reset and the whole buffer."""
        reset = st.needs_reset or len(buf) < st.consumed or zlib.crc32(buf[:st.consumed]) != st.crc
        start = 0 if reset else st.consumed
        if st.wire is not None:   # a wire stream takes the tail as it is: bytes that fill no frame wait inside the library
            return reset, buf[start:]
        return reset, buf[start:len(buf) - (len(buf) - start) % 2]

    def _run_push(self, streams, rows):
        with self._lock:
            for st, (reset, _) in zip(streams, rows):
                if st.detector is None:
                    st.detector = (vad.StreamingSpeechDetector(self.engine) if st.wire is None
                                   else vad.StreamingSpeechDetector(self.engine, wire=st.wire))
                elif reset:
                    self.engine.vad_stream_reset(st.detector.stream_id)
            if self.wire is None:
                return self.engine.vad_stream_push([st.detector.stream_id for st in streams],
                                                   [pcm16_bytes_to_float(new) for _, new in rows])
            pcm, probs = self.engine.vad_stream_push_wire([st.detector.stream_id for st in streams], [new for _, new in rows])
            return list(zip(probs, pcm))


# pyannote_vad.py:37-45: the arguments the reference instantiates its VoiceActivityDetection pipeline with
DEFAULT_PYANNOTE_ARGS = dict(onset=0.5, offset=0.5, min_duration_on=0.3, min_duration_off=0.3)


class DevicePyannoteVAD(VADInterface):
    """VADInterface backend on the device's PyanNet-shaped segmentation network: the reference's PyannoteVAD
    (pyannote_vad.py:12-62) without the wav file and without pyannote.audio.

    Like the reference it evaluates the client's WHOLE scratch buffer (s16le, as asr.pcm16_bytes_to_float reads it) at every
    `detect_activity`: the network's norms span a 5-s chunk, so there is no state to carry.  It returns the Binarize segments of
    the aggregated scores (vad.pyannote_speech_timestamps) in seconds with confidence 1.0, [] for an empty buffer.  Concurrent
    calls that arrive within `max_wait_ms` go into ONE Engine.segmentation_scores call (the coalescing worker DeviceStreamVAD
    uses), which runs in an executor thread; `calls_run` records the rows of every call.

    `pyannote_args`: the reference's keyword - onset, offset, min_duration_on, min_duration_off (and pad_onset, pad_offset)
    over DEFAULT_PYANNOTE_ARGS.  `engine=None`: the backend owns a VAD-only context (micro geometry, no Whisper weights,
    max_batch=64) with `vad_model` loaded (a mapping, an .npz or a torch checkpoint: vad.load_pyannet_state); `engine=`: it
    shares that context, whose segmentation weights are loaded already or come from `vad_model`, and the caller serialises the
    calls (a `vad_model` given beside an engine that holds a network already is ignored with a warning).  Other keywords:
    `device_index` (the GPU of an owned context) and the reference's `model_name` / `auth_token`, ignored with a warning; any
    further keyword raises ValueError.  `forget(client)` drops a client from the count the coalescer waits for."""

    def __init__(self, vad_model=None, engine=None, pyannote_args: Optional[Dict[str, Any]] = None, max_wait_ms: float = 2.0, **kwargs):
        # the reference's own keywords (pyannote_vad.py:26-30) name a hub model and its token: nothing here downloads, they are
        # accepted and logged; device_index picks the GPU of an owned context; anything else is a mistake
        unknown = set(kwargs) - {"device_index", "model_name", "auth_token"}
        if unknown:
            raise ValueError(f"DevicePyannoteVAD: unknown keywords {sorted(unknown)}")
        for k in ("model_name", "auth_token"):
            if k in kwargs:
                logger.warning("DevicePyannoteVAD ignores %s=: the network comes from vad_model= or engine=", k)
        self.owns_engine = engine is None
        if engine is None:
            if vad_model is None:
                raise ValueError("DevicePyannoteVAD needs vad_model= (the PyanNet tensors) or an engine= that has them loaded")
            from .config import COMPUTE_F32, PRESETS
            from .engine import Engine
            engine = Engine(PRESETS["micro"], COMPUTE_F32, 64, device=int(kwargs.get("device_index", 0)))
        if vad_model is not None and getattr(engine, "has_segmentation", False):
            logger.warning("DevicePyannoteVAD ignores vad_model=: the engine already holds a segmentation network")
        elif vad_model is not None:
            engine.load_segmentation(vad.load_pyannet_state(vad_model))
        if not getattr(engine, "has_segmentation", False):
            raise ValueError("DevicePyannoteVAD: the engine has no segmentation weights and no vad_model= was given")
        self.engine = engine
        self.args = dict(DEFAULT_PYANNOTE_ARGS)
        self.args.update(pyannote_args or {})
        unknown = set(self.args) - {"onset", "offset", "min_duration_on", "min_duration_off", "pad_onset", "pad_offset"}
        if unknown:
            raise ValueError(f"pyannote_args: unknown keys {sorted(unknown)}")
        self.max_wait = max_wait_ms / 1000.0
        self.calls_run: List[int] = []    # rows of the device calls actually executed (observability / tests)
        self._clients: Dict[Any, object] = {}   # client id -> the key of its row in a batch
        self._lock = threading.Lock()     # one engine call at a time from this object
        self._coalescer = _Coalescer(self.max_wait, lambda: len(self._clients), self._run_batch)

    async def detect_activity(self, client):
        buf = bytes(client.scratch_buffer)
        if len(buf) < 2:
            return []
        key = self._clients.setdefault(client.client_id, object())
        chunks = await self._coalescer.submit(key, buf)
        rate = float(vad.SAMPLING_RATE)
        return [{"start": c["start"] / rate, "end": c["end"] / rate, "confidence": 1.0} for c in chunks]

    def forget(self, client) -> None:
        self._clients.pop(getattr(client, "client_id", client), None)

    def close(self) -> None:
        self._coalescer.cancel()
        self._clients.clear()
        if self.owns_engine and self.engine is not None:
            self.engine.close()
        self.engine = None

    async def _run_batch(self, batch):
        audios = [pcm16_bytes_to_float(buf[:len(buf) - len(buf) % 2]) for _, buf, _ in batch]
        try:
            scores = await asyncio.get_running_loop().run_in_executor(None, self._run_scores, audios)
        except Exception as e:
            logger.error("segmentation VAD call failed: %s", e)
            for _, _, fut in batch:
                if not fut.done():
                    fut.set_exception(e)
            return
        self.calls_run.append(len(batch))
        for (_, _, fut), a, s in zip(batch, audios, scores):
            if not fut.done():
                fut.set_result(vad.pyannote_speech_timestamps(len(a), s, **self.args))

    def _run_scores(self, audios):
        with self._lock:
            return self.engine.segmentation_scores(audios)


class VADFactory:
    @staticmethod
    def create_vad_pipeline(type, **kwargs):
        """vad_factory.py:13-44 knows "simple" and "pyannote"; "silero" / "mi355x_silero" is the device's streaming backend (its
        keywords, wire= among them, pass through), "pyannote" / "mi355x_pyannote" the device's segmentation backend
        (vad_model= or engine=, pyannote_args=, max_wait_ms=)."""
        if type == "simple":
            return SimpleVAD(**kwargs)
        if type in ("silero", "mi355x_silero"):
            return DeviceStreamVAD(**kwargs)
        if type in ("pyannote", "mi355x_pyannote"):
            return DevicePyannoteVAD(**kwargs)
        raise ValueError(f"unsupported VAD pipeline type: {type} (supported: 'simple', 'silero', 'mi355x_silero', 'pyannote', "
                         "'mi355x_pyannote')")
