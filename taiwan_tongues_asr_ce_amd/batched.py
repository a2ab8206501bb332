"""faster-whisper's BatchedInferencePipeline for ONE long recording: VAD -> speech chunks packed into
groups of at most one window (vad.merge_chunks) -> every group decoded as an independent clip of one continuous-batching beam
session -> segments back on the recording's time line, in group order.

A group is decoded exactly as WhisperModel.transcribe_many(continuous=True) decodes a one-window file made of the group's audio:
the same prompt, options, window-form submission at seek 0, scoring and fallback ladder.  The session runs in hold mode, so a
group that fails its thresholds goes up the ladder with Session.retry - a new search on the cross-KV its first attempt encoded,
no encoder work - and a settled group is aligned (word_timestamps) while its encoder state is still there.  There is no
previous-text conditioning between groups."""
from __future__ import annotations

import dataclasses
import warnings
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import alignment, vad
from .audio_io import decode_audio, parse_audio_channel
from .config import HOP, SAMPLE_RATE
from .model import LANGUAGES, Segment, TranscriptionInfo, Word, select_language


def clip_groups(clip_timestamps, n_samples: int, max_samples: int) -> List[Dict]:
    """clip_timestamps -> groups in merge_chunks' form: a list of {"start", "end"} in seconds, or a flat list of seconds
    (start, end, start, end ...; a missing last end is the end of the recording).  Each clip is one group; a clip longer than
    max_samples is cut into groups of max_samples."""
    if isinstance(clip_timestamps, str):   # faster-whisper's "start,end,start,end..." form
        clip_timestamps = [float(t) for t in clip_timestamps.split(",") if t.strip()]
    clips = list(clip_timestamps)
    if clips and not isinstance(clips[0], dict):
        flat = [float(t) for t in clips]
        if len(flat) % 2:
            flat.append(n_samples / SAMPLE_RATE)
        clips = [dict(start=flat[i], end=flat[i + 1]) for i in range(0, len(flat), 2)]
    out: List[Dict] = []
    for c in clips:
        a = min(max(int(round(float(c["start"]) * SAMPLE_RATE)), 0), n_samples)
        b = min(max(int(round(float(c["end"]) * SAMPLE_RATE)), 0), n_samples)
        if b < a:
            raise ValueError(f"clip_timestamps: clip {c!r} ends before it starts")
        while b - a > max_samples:
            out.append(dict(start=a, end=a + max_samples, segments=[dict(start=a, end=a + max_samples)]))
            a += max_samples
        if b > a:
            out.append(dict(start=a, end=b, segments=[dict(start=a, end=b)]))
    return out


def restore_group_times(segments: Sequence[Segment], pieces: Sequence[Dict[str, int]]) -> List[Segment]:
    """Group-local times -> the recording's time line through a SpeechTimestampsMap over the group's speech pieces.  A segment's
    start and end are mapped on their own (it may straddle a seam between two pieces); a word goes with the piece its middle
    falls in and is kept inside that piece, and a segment with words starts and ends with them."""
    ts_map = vad.SpeechTimestampsMap(pieces)
    rate = float(ts_map.sampling_rate)
    out = []
    for seg in segments:
        if seg.words:
            words = []
            for w in seg.words:
                k = ts_map.get_chunk_index((w.start + w.end) / 2)
                lo, hi = pieces[k]["start"] / rate, pieces[k]["end"] / rate
                a = min(max(ts_map.total_silence_before[k] + w.start, lo), hi)
                b = min(max(ts_map.total_silence_before[k] + w.end, a), hi)
                words.append(Word(start=round(a, 2), end=round(b, 2), word=w.word, probability=w.probability))
            out.append(seg._replace(start=words[0].start, end=words[-1].end, words=words))
        else:
            out.append(seg._replace(start=ts_map.get_original_time(seg.start), end=ts_map.get_original_time(seg.end)))
    return out


class BatchedInferencePipeline:
    """BatchedInferencePipeline(model).transcribe(audio, ...) -> (iterator of Segment, TranscriptionInfo)."""

    def __init__(self, model):
        self.model = model

    # -- 1. chunks ----------------------------------------------------------------------------------
    def _groups(self, audio: np.ndarray, vad_filter: bool, vad_parameters, prob_fn, clip_timestamps, chunk_length: float
                ) -> Tuple[List[Dict], Optional[Dict]]:
        m = self.model
        max_samples = int(round(chunk_length * SAMPLE_RATE))
        if clip_timestamps is not None:
            return clip_groups(clip_timestamps, len(audio), max_samples), None
        if not vad_filter:
            if len(audio) > max_samples:
                raise ValueError(f"a recording of {len(audio) / SAMPLE_RATE:.1f} s is longer than chunk_length ({chunk_length:g} s): "
                                 "the batched pipeline needs vad_filter=True or clip_timestamps to cut it into groups")
            return clip_groups([0.0, len(audio) / SAMPLE_RATE], len(audio), max_samples), None
        if dataclasses.is_dataclass(vad_parameters):
            vad_parameters = dataclasses.asdict(vad_parameters)
        params = dict(vad_parameters or {})
        # faster-whisper's defaults for its batched pipeline (UNPINNED: no executable reference here)
        params.setdefault("max_speech_duration_s", chunk_length)
        params.setdefault("min_silence_duration_ms", 160)
        kind, fn = m._vad_source(params, prob_fn, stacklevel=4)
        if kind == "device":
            fn = lambda a: m.vad_speech_probs([a])[0]
        if kind == "none":
            speech = [dict(start=0, end=len(audio))] if len(audio) else []
        else:
            speech = vad.get_speech_timestamps(audio, vad.VadOptions(**params), fn)
        return vad.merge_chunks(speech, max_samples), params

    # -- 4. one settled group -> segments on its own time line -------------------------------------------
    def _group_segments(self, g: dict, attempt, p: dict) -> List[dict]:
        m, st = self.model, self.model.special
        _, toks, avg_lp, ns, _ = attempt
        if p["no_speech_threshold"] is not None and ns > p["no_speech_threshold"] and \
                (p["log_prob_threshold"] is None or avg_lp < p["log_prob_threshold"]):
            return []   # silent by the rule of _finish_window
        frames = g["frames"]
        limit = frames * HOP / SAMPLE_RATE   # the group's duration
        segs, _ = m._split_segments(toks, 0, frames, 0.0, p["without_timestamps"])
        tb = st.timestamp_begin
        body = [t for t in toks if t != st.eot]
        pairs = [i for i in range(1, len(body)) if body[i] >= tb and body[i - 1] >= tb]
        single_end = len(body) >= 2 and body[-1] >= tb and body[-2] < tb
        if pairs and not p["without_timestamps"] and not single_end:
            # tokens behind the last timestamp pair: the sequential loop would decode them again from a later seek; a group is
            # decoded once, so they are its last segment, which ends at the group's duration
            tail = body[pairs[-1]:]
            if any(t < st.eot for t in tail):
                start = (tail[0] - tb) * 0.02 if tail[0] >= tb else (segs[-1][1] if segs else 0.0)
                segs.append((start, limit, tail))
        kept = []
        for (s0, s1, stoks) in segs:
            text = m.tokenizer.decode([t for t in stoks if t < st.eot])
            s0, s1 = min(s0, limit), min(s1, limit)
            if s0 >= s1 or not text.strip():
                continue
            kept.append(dict(start=s0, end=s1, tokens=list(stoks), text=text, words=None))
        return kept

    @staticmethod
    def _deal_words(kept: List[dict], words: List[dict]) -> None:
        """The words of the group's one alignment pass -> its segments, by the text each segment holds."""
        k, seen, total = 0, 0, 0
        for seg in kept:
            total += len(seg["text"])
            mine = []
            while k < len(words) and (seen + len(words[k]["word"]) <= total or seg is kept[-1]):
                seen += len(words[k]["word"])
                mine.append(Word(start=words[k]["start"], end=words[k]["end"], word=words[k]["word"],
                                 probability=words[k]["probability"]))
                k += 1
            seg["words"] = mine or None

    # -- the public call -------------------------------------------------------------------------------
    def transcribe(self, audio: Union[str, np.ndarray], language: Optional[str] = None, task: str = "transcribe",
                   beam_size: int = 5, best_of: int = 5, patience: float = 1.0,
                   temperature: Union[float, Sequence[float]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                   compression_ratio_threshold: Optional[float] = 2.4, log_prob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6, initial_prompt: Optional[str] = None,
                   prefix: Optional[str] = None, hotwords: Optional[str] = None, suppress_blank: bool = True,
                   max_initial_timestamp: float = 1.0, max_new_tokens: Optional[int] = None,
                   without_timestamps: bool = True, word_timestamps: bool = False, multilingual: bool = False,
                   language_detection_threshold: Optional[float] = 0.5, language_detection_segments: int = 1,
                   vad_filter: bool = True, vad_parameters=None, chunk_length: Optional[float] = None,
                   clip_timestamps=None, batch_size: Optional[int] = None, device_resample: bool = False, audio_channel=None,
                   session_prefill: Union[int, bool] = 0, retry_held: bool = True, dsp_mode=None, **kwargs
                   ) -> Tuple[Iterator[Segment], TranscriptionInfo]:
        """The keyword surface of faster-whisper's BatchedInferencePipeline.transcribe; device_resample, audio_channel (path
        input only: one channel of the file instead of the mean, WhisperModel.transcribe), session_prefill and retry_held are
        extensions of this build.  retry_held=False releases a failing group and submits it again (one more
        encoder pass per attempt): the A/B switch, and the form for engines without Session.retry.
        dsp_mode (dsp.resolve; None = off): the recording is enhanced once (Engine.enhance) before the VAD and before the
        session opens.
        info.chunks lists the groups with their attempts; info.session is filled when the iterator is exhausted."""
        from . import dsp
        from .engine import session_prefill_value
        m = self.model
        dsp_params = dsp.resolve(dsp_mode)
        neutral = {"vad_speech_prob_fn": None, "length_penalty": 1, "repetition_penalty": 1, "no_repeat_ngram_size": 0,
                   "hallucination_silence_threshold": None, "prompt_reset_on_temperature": 0.5, "suppress_tokens": [-1],
                   "prepend_punctuations": alignment.PREPEND_PUNCTUATIONS, "append_punctuations": alignment.APPEND_PUNCTUATIONS,
                   "log_progress": False}
        for k, v in kwargs.items():
            if k == "vad_speech_prob_fn":
                continue
            if k not in neutral:
                raise TypeError(f"transcribe() got an unexpected keyword argument {k!r}")
            if v is not None and v != neutral[k]:
                warnings.warn(f"transcribe(): option {k}={v!r} is not implemented in this build and is ignored", stacklevel=2)
        session_prefill = session_prefill_value(session_prefill)
        if not callable(getattr(m.engine, "session", None)):
            raise ValueError("the batched pipeline needs an engine with continuous-batching sessions (Engine.session)")
        pick = parse_audio_channel(audio_channel)
        if isinstance(audio, str):
            audio = m.decode_audio_many([audio], audio_channel=pick)[0] if device_resample else decode_audio(audio, channel=pick)
        elif pick is not None:
            raise ValueError("audio_channel picks a channel of a file: an array input is already mono")
        audio = np.asarray(audio)
        if audio.ndim != 1:
            raise ValueError(f"audio must be mono float32 [n] @16 kHz, got shape {audio.shape}")
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        beam_size = int(beam_size)
        if not 1 <= beam_size <= 7:
            raise ValueError(f"beam_size={beam_size} outside [1, 7]")
        if beam_size > m.max_batch:
            raise ValueError(f"beam_size={beam_size} needs {beam_size} decode rows but this model was built with max_batch={m.max_batch}")
        window_s = m.n_window / SAMPLE_RATE
        chunk_length = window_s if chunk_length is None else float(chunk_length)
        if not 0 < chunk_length <= window_s:
            raise ValueError(f"chunk_length={chunk_length:g} outside (0, {window_s:g}] (a group is at most one window)")
        if int(language_detection_segments) < 1:
            raise ValueError("language_detection_segments must be >= 1")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        temps = tuple(temperature) if isinstance(temperature, (list, tuple)) else (float(temperature),)
        if any(t > 0.0 for t in temps) and max(beam_size, min(int(best_of), m.max_batch)) > 7:
            raise ValueError(f"best_of={best_of}: a session holds at most 7 rows per group")
        if language is not None:
            m._lang_token(language)   # raises on a code this build cannot name
        if dsp_params is not None:   # every argument is checked: the first device work of the call, in front of the VAD
            audio = m.engine.enhance([audio], params=dsp_params)[0]

        groups, vad_options = self._groups(audio, bool(vad_filter), vad_parameters,
                                           kwargs.get("vad_speech_prob_fn") or m.vad_speech_prob_fn, clip_timestamps, chunk_length)
        for g in groups:
            g["audio"] = vad.collect_chunks(audio, g["segments"])
            g["frames"] = max(len(g["audio"]) // HOP, 1)
            g["attempts"] = []
        duration = len(audio) / SAMPLE_RATE
        duration_after_vad = sum(len(g["audio"]) for g in groups) / SAMPLE_RATE

        detect_each = bool(multilingual) and m.is_multilingual
        if language is None:
            if m.is_multilingual and groups:
                found = m.detect_language_batch([g["audio"] for g in groups[:int(language_detection_segments)]])
                language, lang_p, i = select_language([(f[0], f[1]) for f in found], language_detection_threshold)
                all_p = found[i][2]
            else:
                language, lang_p, all_p = "en", 1.0, None
        else:
            lang_p, all_p = 1.0, None
        p = m._params(language, task, False, without_timestamps, max_new_tokens, no_speech_threshold, log_prob_threshold,
                      max_initial_timestamp, suppress_blank, beam_size, patience, temps, best_of, compression_ratio_threshold,
                      bool(word_timestamps), hotwords, prefix)
        info = TranscriptionInfo(language=language, language_probability=lang_p, duration=duration,
                                 duration_after_vad=duration_after_vad, all_language_probs=all_p,
                                 transcription_options=dict(beam_size=beam_size, task=task, without_timestamps=without_timestamps,
                                                            condition_on_previous_text=False, initial_prompt=initial_prompt),
                                 vad_options=vad_options)
        info.chunks = [dict(start=g["start"], end=g["end"], segments=[dict(s) for s in g["segments"]], attempts=g["attempts"])
                       for g in groups]
        if detect_each:
            info.window_languages = [None] * len(groups)
        # before the session opens (it owns the encoder while it is open): each group's dynamic-range floor, as a one-window file's
        for g in groups:
            g["file_max"] = m._file_feature_max(g["audio"])
        return self._decode(groups, p, info, initial_prompt, detect_each, batch_size, session_prefill, bool(retry_held)), info

    # -- 2., 3., 5. the session loop ------------------------------------------------------------------
    def _decode(self, groups: List[dict], p: dict, info: TranscriptionInfo, initial_prompt: Optional[str], detect_each: bool,
                batch_size: Optional[int], session_prefill: int, retry_held: bool) -> Iterator[Segment]:
        from .engine import GenResult, Session, TtasrError
        m, eng = self.model, self.model.engine
        temps, beam = p["temperatures"], p["beam_size"]
        rows_sampled = max(1, min(p["best_of"], m.max_batch))
        width = max(beam, rows_sampled) if any(t > 0.0 for t in temps) else beam
        if not groups:
            info.session = dict(retries=0.0)
            return
        n_ctx = m.dims.n_text_ctx
        units = max(1, m.max_batch // width)
        cap = units if batch_size is None else int(batch_size)
        opts = m._window_opts(1, 0, p)   # the session's rules; budgets and sot indices are per group
        eng.set_audio_ctx(0)
        kw = dict(detect_language=True) if detect_each else {}
        if session_prefill:
            kw["prefill"] = int(session_prefill)
        retries = 0
        ready: Dict[int, List[Segment]] = {}   # settled groups whose turn has not come
        next_out, seg_id = 0, 0
        with eng.session(opts, n_ctx - 1, beam=width, patience=p["patience"], **kw) as s:
            try:
                s.hold()
                inflight: Dict[int, int] = {}   # clip id -> group index
                waiting = list(range(len(groups)))[::-1]

                def attempt_args(g: dict) -> dict:
                    temp = temps[len(g["attempts"])]
                    return dict(max_new=[g["budget"]], temperature=[temp], rows=[rows_sampled if temp > 0.0 else beam],
                                seed=[m._fallback_seed(0, temp)])

                def submit(k: int):
                    g = groups[k]
                    ids = s.submit_windows([g["audio"]], [0], [g["prompt"]], [g["sot"]], floor_max=[g["file_max"]], **attempt_args(g))
                    inflight[ids[0]] = k

                def start(k: int):
                    g = groups[k]
                    fs = m._new_file_state(g["audio"], initial_prompt)
                    g["prompt"], g["sot"] = m._prompt(Session.DETECT if detect_each else p["lang_tok"], p["task"],
                                                      p["without_timestamps"], fs["prev"], p["hotwords_tokens"], p["prefix_tokens"])
                    g["budget"] = min(p["max_new"], n_ctx - len(g["prompt"]))
                    g["language"], g["lang_tok"] = p["language"], p["lang_tok"]
                    submit(k)

                while waiting or inflight:
                    while waiting and len(inflight) < cap:
                        start(waiting.pop())
                    got = s.poll()
                    if not got:
                        raise TtasrError(f"session idle with {len(inflight)} groups unfinished")
                    settled: List[Tuple[int, int, tuple]] = []   # (clip id, group index, chosen attempt)
                    for r in got:
                        k = inflight.pop(r.id)
                        g = groups[k]
                        if r.language is not None:   # detected inside the session: a later attempt carries this language
                            lang = LANGUAGES[r.language]
                            g["language"], g["lang_tok"] = lang, m._lang_token(lang)
                            g["prompt"][g["sot"] + 1] = g["lang_tok"]
                            info.window_languages[k] = lang
                        temp = temps[len(g["attempts"])]
                        res = GenResult([r.tokens], np.asarray([r.sum_logprob], np.float32), np.asarray([r.no_speech_prob], np.float32))
                        toks, avg_lp, ns, cr = m._score(res, 0)
                        g.setdefault("tried", []).append((temp, toks, avg_lp, ns, cr))
                        g["attempts"].append((temp, avg_lp, ns, cr))
                        if m._needs_fallback(avg_lp, ns, cr, p):
                            if len(g["attempts"]) < len(temps):   # the next temperature of the ladder
                                if retry_held:
                                    new, = s.retry([r.id], [g["prompt"]], [g["sot"]], **attempt_args(g))
                                    inflight[new] = k
                                    retries += 1
                                else:
                                    s.release([r.id])
                                    submit(k)
                                continue
                            chosen = m._best_attempt(g["tried"], p)
                        else:
                            chosen = g["tried"][-1]
                        settled.append((r.id, k, chosen))
                    # settled groups: aligned while still held (one pass per language of the poll), or released
                    free, by_lang = [], {}
                    for cid, k, chosen in settled:
                        g = groups[k]
                        g["kept"] = self._group_segments(g, chosen, p)
                        g["chosen"] = chosen
                        if p["word_timestamps"] and g["kept"]:
                            by_lang.setdefault(g["language"], []).append((cid, k))
                        else:
                            free.append(cid)
                    if free:
                        s.release(free)
                    for lang in sorted(by_lang):
                        ids = [cid for cid, _ in by_lang[lang]]
                        ks = [k for _, k in by_lang[lang]]
                        toks = [[t for seg in groups[k]["kept"] for t in seg["tokens"]] for k in ks]
                        words = m._window_words(s, ids, toks, [len(groups[k]["audio"]) for k in ks], lang, m._lang_token(lang), p["task"])
                        for k, w in zip(ks, words):
                            self._deal_words(groups[k]["kept"], w)
                    for _, k, chosen in settled:
                        g = groups[k]
                        temp_used, _, avg_lp, ns, cr = chosen
                        local = [Segment(0, g["start"] // HOP, round(seg["start"], 3), round(seg["end"], 3), seg["text"], seg["tokens"],
                                         temp_used, avg_lp, cr, ns, seg["words"]) for seg in g["kept"]]
                        ready[k] = restore_group_times(local, g["segments"])
                        g.pop("tried", None)
                    while next_out in ready:   # group order; groups that settled early wait here
                        for seg in ready.pop(next_out):
                            yield seg._replace(id=seg_id)
                            seg_id += 1
                        next_out += 1
            finally:
                stats = dict(s.stats()) if getattr(s, "open", True) else {}
                stats["retries"] = float(retries)
                info.session = stats
