"""Streaming side of the hot path (BASELINE.json configs[4]).

The reference's WebSocket server hands ~3-second utterances of up to 10 concurrent clients to ONE model and
serialises them on the event loop: `transcribe` is a blocking call inside `async def`
(faster_whisper_asr.py:170), so every client waits for every other client's full 30-s-padded decode.
This module keeps the reference's trigger rule and result shape but coalesces concurrent requests into one
batched engine pass (clips x beams = rows of one decode batch, cross-KV shared per clip) that runs in a worker
thread, so the event loop stays free."""
from __future__ import annotations

import asyncio
import logging
import queue
import threading
import warnings
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .asr import MI355XWhisperASR, pcm16_bytes_to_float

logger = logging.getLogger(__name__)


def should_transcribe(scratch_bytes: int, vad_end_seconds: float, chunk_offset_seconds: float, sampling_rate: int = 16000,
                      samples_width: int = 2) -> bool:
    """The SilenceAtEndOfChunk trigger (buffering_strategies.py:118-126): transcribe when the last voiced
    segment ends before (buffered seconds - offset), or when more than 2 s (after the offset) are buffered."""
    last_segment_should_end_before = scratch_bytes / (sampling_rate * samples_width) - chunk_offset_seconds
    return vad_end_seconds < last_segment_should_end_before or last_segment_should_end_before > 2


def chunk_ready(buffer_bytes: int, chunk_length_seconds: float, sampling_rate: int = 16000, samples_width: int = 2) -> bool:
    """buffering_strategies.py:66-71: a chunk is handed over once MORE than chunk_length seconds are buffered."""
    return buffer_bytes > chunk_length_seconds * sampling_rate * samples_width


class BatchedWhisperASR(MI355XWhisperASR):
    """ASRInterface backend that micro-batches concurrent `transcribe(client)` calls.

    max_clips * beam_size must fit the model's row budget (max_batch, <= 32 on the bf16 fast path).
    `audio_ctx="auto"` additionally encodes only as many positions as the longest utterance of a batch needs
    (a 3-s utterance: 200 of 1500 positions), which is a behavioural change and therefore opt-in.

    `continuous=True` (opt-in) replaces the lock-step passes with one continuous-batching session (WhisperModel engine,
    ttasr_session_begin_beam): a request is submitted as it arrives, takes a free group of beam_size rows and resolves when
    its own search ends, not when the longest clip of its pass does.  max_clips groups of beam_size rows; the full 30-s window
    is encoded, so it cannot be combined with audio_ctx.

    `cross_kv_fp8=True` (opt-in, both modes; passed on to WhisperModel): the decode steps read the e4m3 copy of the
    cross-attention cache (16-bit compute types only).

    `word_timestamps=True` (opt-in, both modes): "words" holds {"word", "start", "end", "probability"} with the client's
    last_start_time added to start and end, and "duration" is the last word's end, as in the reference's result; the clips of
    a pass (lock-step) or of a poll (continuous: the session runs in hold mode) are aligned in one device pass.

    `language` (default "zh", the reference's forced language): None detects every utterance from its pass's encoder state
    (WhisperModel.transcribe_windows(language=None)) and reports the detected language and probability instead of "zh" and
    1.0, with a warning when the probability is under 0.5 as the reference's adapter logs it.  In continuous mode None needs
    `detect_in_session=True` (opt-in): a session owns the encoder while it is open, so every request goes in with the language
    placeholder and its first decode step finds the language on the device (Engine.session(detect_language=True)).

    `session_prefill=N` (opt-in, continuous=True only; True = config.SESSION_PREFILL_DEFAULT): the initial_prompt's positions in
    front of <|startoftranscript|> come from one admission pass of the session instead of one forced decode step each, when there
    are at least N of them (Engine.session(prefill=N)); requests that carry the language placeholder are forced as before.

    `clip_timestamps` / `hallucination_silence_threshold`: options of the file-level window loop (WhisperModel.transcribe and the
    lock-step transcribe_many); here they are accepted at their neutral values only, anything else is a ValueError before a model
    is built - with continuous=True because a session cannot run them (the message names the lock-step transcribe_many), and with
    continuous=False as well, where an utterance is a single window of transcribe_windows and neither option has a meaning
    (refused rather than ignored).

    `wire=` / `audio_from=` (opt-in, both modes; MI355XWhisperASR.client_audio): what the clients' scratch bytes are when they
    are not 16 kHz mono s16 - a vad.WireFormat, or "client" for each client's own declaration - and the
    vad_backends.DeviceStreamVAD(wire=...) whose device streams have converted the same bytes already."""

    def __init__(self, max_clips: int = 6, max_wait_ms: float = 5.0, audio_ctx=None, max_new_tokens: int = 224,
                 continuous: bool = False, word_timestamps: bool = False, detect_in_session: bool = False,
                 session_prefill=0, clip_timestamps="0", hallucination_silence_threshold=None, **kwargs):
        from .dsp import refuse_streaming
        from .engine import session_prefill_value
        from .model import refuse_in_session
        # enhancement reads a whole recording: refused before a model is built or a worker starts
        refuse_streaming(kwargs.get("dsp_mode"), "BatchedWhisperASR")
        kwargs.pop("dsp_mode", None)
        # the window-loop options of WhisperModel.transcribe: an utterance here is one window, and a session cannot run them
        try:
            refuse_in_session("BatchedWhisperASR(continuous=True)", clip_timestamps, hallucination_silence_threshold)
        except ValueError:
            if continuous:
                raise
            raise ValueError("BatchedWhisperASR decodes single-window utterances: clip_timestamps and hallucination_silence_threshold "
                             "belong to the file-level loop (WhisperModel.transcribe / transcribe_many)") from None
        if continuous:   # keyword biasing is a lock-step feature: a session's kernels do not apply the table
            from .seq_bias import refuse_in_session as refuse_bias
            refuse_bias("BatchedWhisperASR(continuous=True)", kwargs.get("sequence_bias"), kwargs.get("prompt_words"))
        if continuous and audio_ctx is not None:
            raise ValueError("continuous=True encodes the full window: audio_ctx must be None")
        self.session_prefill = session_prefill_value(session_prefill)
        if self.session_prefill and not continuous:
            raise ValueError("session_prefill is for continuous=True (the lock-step passes prefill their prompts already)")
        self.continuous = bool(continuous)
        self.word_timestamps = bool(word_timestamps)
        beam = int(kwargs.pop("beam_size", 5))
        self.language = kwargs.pop("language", "zh")
        self.detect_in_session = bool(detect_in_session)
        if self.detect_in_session and not (continuous and self.language is None):
            raise ValueError("detect_in_session=True is for continuous=True with language=None")
        if continuous and self.language is None and not self.detect_in_session:
            raise ValueError("language=None in continuous mode needs detect_in_session=True (or the lock-step mode, continuous=False)")
        self.audio_ctx = audio_ctx            # None = Whisper's 30-s window; "auto"/int = opt-in short window (N2)
        self.max_new_tokens = max_new_tokens
        kwargs.setdefault("max_batch", max(8, max_clips * beam))
        super().__init__(**kwargs)
        self.default_transcribe_kwargs["beam_size"] = beam
        self.max_clips = max(1, min(max_clips, self.asr_pipeline.max_batch // max(beam, 1)))
        self.max_wait = max_wait_ms / 1000.0
        self._queue: Optional[asyncio.Queue] = None
        self._worker_task: Optional[asyncio.Task] = None
        self.batches_run: List[int] = []  # sizes of the batches actually executed (observability / tests)
        self._cq: Optional[queue.Queue] = None          # continuous mode: requests for the session thread (None = stop)
        self._session_thread: Optional[threading.Thread] = None

    def _ensure_worker(self):
        if self._queue is None:
            self._queue = asyncio.Queue()
        if self._worker_task is None or self._worker_task.done():
            self._worker_task = asyncio.get_running_loop().create_task(self._worker())

    async def _worker(self):
        loop = asyncio.get_running_loop()
        while True:
            first = await self._queue.get()
            batch = [first]
            deadline = loop.time() + self.max_wait
            while len(batch) < self.max_clips:
                timeout = deadline - loop.time()
                if timeout <= 0:
                    break
                try:
                    batch.append(await asyncio.wait_for(self._queue.get(), timeout))
                except asyncio.TimeoutError:
                    break
            audios = [a for a, _, _ in batch]
            langs: List[Tuple[str, float]] = [("zh", 1.0)] * len(batch)
            try:
                results = await loop.run_in_executor(None, self._run_batch, audios)
                if self.language is None:
                    langs = list(self.asr_pipeline.last_language_info)
            except Exception as e:  # the reference logs and returns None per request
                logger.error("batched transcribe failed: %s", e)
                results = [None] * len(batch)
            self.batches_run.append(len(batch))
            for (_, last_start, fut), res, lang in zip(batch, results, langs):
                if not fut.done():
                    fut.set_result(self._result_dict(res, last_start, lang))

    def _run_batch(self, audios: Sequence[np.ndarray]) -> List[Optional[Tuple[str, float]]]:
        kw = self.default_transcribe_kwargs
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs = self.asr_pipeline.transcribe_windows(audios, language=self.language, beam_size=kw["beam_size"],
                                                        initial_prompt=kw["initial_prompt"], audio_ctx=self.audio_ctx,
                                                        max_new_tokens=self.max_new_tokens, word_timestamps=self.word_timestamps)
        return [_window_result(audio, *o) for audio, o in zip(audios, outs)]

    def _ensure_session(self):
        if self._cq is None:
            self._cq = queue.Queue()
        if self._session_thread is None or not self._session_thread.is_alive():
            self._session_thread = threading.Thread(target=self._session_loop, args=(self._cq,), name="ttasr-session", daemon=True)
            self._session_thread.start()

    def _session_loop(self, q: "queue.Queue"):
        """Continuous mode: this thread owns one open session on the model's engine; requests are submitted as they arrive and
        their futures resolve as polls return them.  The prompt and options are transcribe_windows' for the same arguments."""
        model = self.asr_pipeline
        eng, kw = model.engine, self.default_transcribe_kwargs
        beam = max(1, min(int(kw["beam_size"]), 7))
        prev = model.tokenizer.encode(" " + kw["initial_prompt"].strip()) if kw.get("initial_prompt") else []
        from .engine import Session
        detect = self.language is None and model.is_multilingual
        fixed = "zh"   # what the session decodes with when nothing is detected (the reference's forced language)
        prompt, sot_index = model._prompt(Session.DETECT if detect else model._lang_token(fixed), "transcribe", False, prev)
        pending: Dict[int, Tuple[np.ndarray, float, Any, Any]] = {}

        def resolve(fut, loop, value):
            loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(value))

        try:
            eng.set_audio_ctx(0)
            opts = eng.gen_opts(min(self.max_new_tokens, model.dims.n_text_ctx - len(prompt)), timestamps=True, sot_index=sot_index)
            kw_s = dict(detect_language=True) if detect else {}
            if self.session_prefill:
                kw_s["prefill"] = self.session_prefill
            with (eng.session(opts, len(prompt), beam=beam, **kw_s) if beam > 1 else eng.session(opts, len(prompt), **kw_s)) as s:
                if self.word_timestamps:
                    s.hold()
                while True:
                    items = [] if pending else [q.get()]        # idle: wait for a request
                    while True:
                        try:
                            items.append(q.get_nowait())
                        except queue.Empty:
                            break
                    if any(it is None for it in items):
                        for it in items:
                            if it is not None:
                                resolve(it[2], it[3], None)
                        break
                    for audio, last_start, fut, loop in items:
                        a = np.ascontiguousarray(audio[: model.n_window], dtype=np.float32)
                        pending[s.submit([a], [prompt])[0]] = (audio, last_start, fut, loop)
                    got = s.poll(max_steps=1 if beam > 1 else 8)
                    sizes = [min(len(pending[r.id][0]), model.n_window) for r in got]
                    langs = [model._session_language(r)[:2] if r.language is not None else (fixed, 1.0) for r in got]
                    words: List[Any] = [None] * len(got)
                    for lang in sorted({l for l, _ in langs}) if self.word_timestamps else ():   # one alignment pass per language
                        k = [i for i, (l, _) in enumerate(langs) if l == lang]
                        for i, w in zip(k, model._window_words(s, [got[i].id for i in k], [got[i].tokens for i in k],
                                                               [sizes[i] for i in k], lang, model._lang_token(lang))):
                            words[i] = w
                    for r, n, w, lang in zip(got, sizes, words, langs):
                        audio, last_start, fut, loop = pending.pop(r.id)
                        res = model.window_text(r.tokens, n) + ((w,) if w is not None else ())
                        resolve(fut, loop, self._result_dict(_window_result(audio, *res), last_start, lang))
        except Exception as e:  # the reference logs and returns None per request
            logger.error("continuous transcribe failed: %s", e)
        finally:
            for _, _, fut, loop in pending.values():
                resolve(fut, loop, None)

    def _result_dict(self, res, last_start, lang: Tuple[str, float] = ("zh", 1.0)) -> Optional[Dict[str, Any]]:
        if res is None:
            return None
        if lang[1] < 0.5:   # the reference's adapter logs a low-confidence detection the same way
            logger.warning("language %s detected with probability %.2f", lang[0], lang[1])
        text, duration = res[0], res[1]
        words = [{"word": w["word"], "start": w["start"] + last_start, "end": w["end"] + last_start, "probability": w["probability"]}
                 for w in (res[2] if len(res) > 2 else [])]
        if words:
            duration = res[2][-1]["end"]
        if self.text_filter is not None:
            filtered = self.text_filter(text)
            text = text if filtered is None else filtered
        return {"language": lang[0], "language_probability": lang[1], "final": True, "text": text, "duration": duration, "words": words}

    async def transcribe(self, client) -> Optional[Dict[str, Any]]:
        try:
            audio = self.client_audio(client)   # wire=None: the s16 bytes at 16 kHz, as ever (MI355XWhisperASR.client_audio)
            if self.continuous:
                self._ensure_session()
                loop = asyncio.get_running_loop()
                fut = loop.create_future()
                self._cq.put((audio, getattr(client, "last_start_time", 0) or 0, fut, loop))
                return await fut
            self._ensure_worker()
            fut = asyncio.get_running_loop().create_future()
            await self._queue.put((audio, getattr(client, "last_start_time", 0) or 0, fut))
            return await fut
        except Exception as e:
            logger.error("transcribe failed: %s", e)
            return None

    async def aclose(self):
        if self._session_thread is not None:   # continuous mode: the thread ends the session and resolves what is left
            self._cq.put(None)
            await asyncio.get_running_loop().run_in_executor(None, self._session_thread.join)
            self._session_thread = None
        if self._worker_task is not None:
            self._worker_task.cancel()
            try:
                await self._worker_task
            except (asyncio.CancelledError, Exception):
                pass
            self._worker_task = None


def _window_result(audio: np.ndarray, text: str, end_time: float, words: Optional[list] = None) -> Optional[tuple]:
    """(text, end_time[, words]) of one request, its end capped at the audio's length; None when nothing was said."""
    if not text.strip():
        return None
    return (text, min(end_time, len(audio) / 16000.0)) + ((words,) if words is not None else ())
