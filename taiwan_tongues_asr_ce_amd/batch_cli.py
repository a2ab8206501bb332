"""Folder transcription tool: the caller on the near side of the hot path (SURVEY §3 call stack 1, §8f N3).

Mirrors the observable contract of the reference's batch entry point (asr_core.py:109-369):

* every `*.wav|mp3|flac|m4a|aac` (either case) directly inside the folder is one unit of work (asr_core.py:118-131);
* each is transcribed with `language="zh", word_timestamps=False, vad_filter=True, beam_size=5,
  condition_on_previous_text=True, initial_prompt=""` (asr_core.py:159-167) and ALL lazy segments are consumed;
* the normalised text goes to `<stem>_asr.txt` beside the audio (asr_core.py:181-187); when transcription raises, that
  file holds the file name and the error instead and the run continues (asr_core.py:244-255);
* a transcript named `<stem>.txt`, `<stem>_transcript.txt`, `_original`, `_reference` or `_ground_truth`
  (asr_core.py:86-106) is scored with `scoring.compare_texts`;
* `asr_comparison_results.json` in the working directory holds `summary` + `detailed_results` with the reference's
  keys (asr_core.py:258-334).

Differences: by default several files advance in lock step through one engine pass per window round
(`WhisperModel.transcribe_many`: same per-file algorithm and outputs as one by one, batch throughput; `--group-files 1`
restores strictly sequential processing); files are processed in sorted order (the reference iterates a `set`); with several GPUs
(`torchrun --nproc-per-node N -m taiwan_tongues_asr_ce_amd.batch_cli folder`) files are sharded by rank — never by
window, windows of one file are sequentially dependent — and rank 0 merges the per-rank results; only RIFF/WAV is
decodable without librosa/PyAV, other containers are reported as per-file errors.
"""
from __future__ import annotations

import argparse
import functools
import glob
import json
import os
from typing import Callable, Dict, List, Optional

from . import scoring
from .audio_io import decode_audio, parse_audio_channel

AUDIO_PATTERNS = ("*.wav", "*.mp3", "*.flac", "*.m4a", "*.aac")
TRANSCRIPT_SUFFIXES = ("", "_transcript", "_original", "_reference", "_ground_truth")
TRANSCRIBE_KWARGS = dict(language="zh", word_timestamps=False, vad_filter=True, beam_size=5,
                         condition_on_previous_text=True, initial_prompt="")


def list_audio_files(folder: str) -> List[str]:
    found = set()
    for pat in AUDIO_PATTERNS:
        found.update(glob.glob(os.path.join(folder, pat)))
        found.update(glob.glob(os.path.join(folder, pat.upper())))
    return sorted(found)


def find_original_transcript(audio_file: str) -> Optional[str]:
    stem = os.path.splitext(audio_file)[0]
    for suffix in TRANSCRIPT_SUFFIXES:
        cand = f"{stem}{suffix}.txt"
        if os.path.exists(cand):
            return cand
    return None


def _load_audio(path: str, channel: Optional[int] = None):
    return decode_audio(path, channel=channel)


class _EnhancedOnce:
    """The loader of a run that both enhances (dsp_mode) and diarizes: a file's samples are loaded and enhanced ONCE
    (WhisperModel.decode_audio_many(dsp_mode=...): on the device, from the path itself with device_resample) and kept until
    `forget`, so the transcription and the diarization of the file read the same enhanced samples and neither enhances again."""

    def __init__(self, model, base: Callable, params, from_path: bool, pick: Optional[int]):
        self.model, self.base, self.params, self.from_path, self.pick, self.kept = model, base, params, from_path, pick, {}

    def __call__(self, path: str):
        if path not in self.kept:
            src = _probe(path) if self.from_path else self.base(path)
            self.kept[path] = self.model.decode_audio_many([src], audio_channel=self.pick if self.from_path else None,
                                                           dsp_mode=self.params)[0]
        return self.kept[path]

    def forget(self) -> None:
        self.kept.clear()


def _probe(path: str) -> str:
    """The path itself, once the file has been opened: a missing or unreadable file is that file's error, not its group's."""
    with open(path, "rb"):
        return path


def transcribe_file(model, audio_file: str, load_audio: Callable = _load_audio, log: Callable = print, segments=None,
                    language: Optional[str] = TRANSCRIBE_KWARGS["language"], info=None, batched: bool = False,
                    word_timestamps: bool = False, options: Optional[Dict] = None, diarize: Optional[Dict] = None) -> Dict:
    """diarize: not None = the file is also diarized (model.diarize(audio, **diarize)) and `<name>_dia.srt` is written beside
    `<name>_asr.txt`: one cue per segment, its text prefixed with the speaker whose turns overlap it longest
    (diarization.dia_srt: the reference service's SRT conventions).  A failure there is logged and leaves the ASR result as it is.
    options: further transcribe() keywords of a file transcribed here (clip_timestamps, hallucination_silence_threshold, dsp_mode;
    with batched: dsp_mode alone).
    One unit of work → one entry of `detailed_results`.  word_timestamps: the segments carry words (a file transcribed here
    is transcribed with them); they are written to `<name>_words.json` beside `<name>_asr.txt`.  `segments`: already transcribed (group mode, with its `info`), else
    runs it.  language=None (`--language auto`): the language is detected, and the entry names it with its probability.
    batched: the file goes through the batched pipeline (WhisperModel.transcribe_batched), which has no previous-text option."""
    name = os.path.basename(audio_file)
    out_path = os.path.splitext(audio_file)[0] + "_asr.txt"
    try:
        if isinstance(segments, Exception):
            raise segments
        if segments is None and batched:
            kw = {k: v for k, v in TRANSCRIBE_KWARGS.items() if k != "condition_on_previous_text"}
            segments, info = model.transcribe_batched(load_audio(audio_file), **dict(kw, language=language, **(options or {})))
        elif segments is None:
            extra = dict(options or {}, **(dict(word_timestamps=True) if word_timestamps else {}))
            segments, info = model.transcribe(load_audio(audio_file), **dict(TRANSCRIBE_KWARGS, language=language, **extra))
        segments = list(segments)                               # consumes the lazy generator: this is where it runs
        text = "".join(seg.text for seg in segments)
        if word_timestamps:
            with open(os.path.splitext(audio_file)[0] + "_words.json", "w", encoding="utf-8") as f:
                json.dump([dict(id=seg.id, start=seg.start, end=seg.end, text=seg.text,
                                words=[dict(word=w.word, start=w.start, end=w.end, probability=float(w.probability))
                                       for w in (seg.words or [])]) for seg in segments], f, ensure_ascii=False, indent=1)
        processed = scoring.normalise_transcript(text)
        with open(out_path, "w", encoding="utf-8") as f:
            f.write(processed)
        log(f"{name}: {processed}")
        if diarize is not None:
            try:
                from . import diarization
                turns = model.diarize(load_audio(audio_file), **diarize)
                who = diarization.assign_speakers(segments, turns)
                with open(os.path.splitext(audio_file)[0] + "_dia.srt", "wb") as f:
                    f.write(diarization.dia_srt([(s.start, s.end, w, s.text) for s, w in zip(segments, who)]).encode("utf-8"))
                log(f"{name}: {len(turns)} turns of {len(set(t.speaker for t in turns))} speakers")
            except Exception as e:
                log(f"{name}: diarization failed: {e}")
        entry = {"audio_file": name, "asr_result": processed, "original_transcript": None, "cer_result": None,
                 "has_original_transcript": False}
        if language is None and info is not None:   # auto mode only: the forced-language run keeps the reference's keys exactly
            entry["language"] = info.language
            entry["language_probability"] = float(info.language_probability)
        ref_path = find_original_transcript(audio_file)
        if ref_path is not None:
            try:
                with open(ref_path, "r", encoding="utf-8") as f:
                    original = f.read().strip()
                entry["original_transcript"] = original
                entry["has_original_transcript"] = True
                res = scoring.compare_texts(original, processed)
                if res is not None:
                    entry["cer_result"] = res.as_dict()
                    log(f"{name}: CER {res.cer_rate:.4f} ({res.substitutions_count} sub, {res.deletions_count} del, "
                        f"{res.insertions_count} ins)")
            except Exception as e:  # unreadable transcript: keep the ASR result, as the reference does
                log(f"{name}: transcript unreadable: {e}")
        return entry
    except Exception as e:
        with open(out_path, "w", encoding="utf-8") as f:
            f.write(f"檔案名稱: {name}\n錯誤: {e}\n")
        log(f"{name}: error: {e}")
        return {"audio_file": name, "asr_result": None, "original_transcript": None, "cer_result": None,
                "has_original_transcript": False, "error": str(e)}


def summarise(results: List[Dict]) -> Dict:
    scored = [r["cer_result"] for r in results if r.get("cer_result") is not None]
    n = len(scored)
    return {
        "summary": {
            "total_files": len(results),
            "files_with_transcript": sum(1 for r in results if r.get("has_original_transcript", False)),
            "files_with_cer": n,
            "average_cer": sum(c["cer_rate"] for c in scored) / n if n else 0,
            "average_correct_rate": sum(c["correct_rate"] for c in scored) / n if n else 0,
            "total_substitutions": sum(c["substitutions_count"] for c in scored),
            "total_deletions": sum(c["deletions_count"] for c in scored),
            "total_insertions": sum(c["insertions_count"] for c in scored),
        },
        "detailed_results": results,
    }


def process_audio_folder(folder_path: str, model=None, model_path: str = "models", device: str = "cuda",
                         device_index: int = 0, compute_type: str = "float16", max_batch: int = 120, output_json: Optional[str] = None, rank: int = 0,
                         world: int = 1, load_audio: Callable = _load_audio, log: Callable = print,
                         group_files: int = 0, pipeline_depth: int = 0, continuous: bool = False,
                         cross_kv_fp8: bool = False, language: Optional[str] = TRANSCRIBE_KWARGS["language"],
                         detect_in_session: bool = False, session_prefill: int = 0, vad_model=None,
                         device_resample: bool = False, batched: bool = False, word_timestamps: bool = False,
                         audio_channel=None, clip_timestamps: str = "0",
                         hallucination_silence_threshold: Optional[float] = None, diarize: bool = False, seg_model=None,
                         spk_model=None, num_speakers: Optional[int] = None, prompt_words=None,
                         prompt_word_boost: Optional[float] = None, dsp_mode=None,
                         dsp_strength: Optional[float] = None) -> Optional[Dict]:
    """dsp_mode (`--dsp-mode {0,1} [--dsp-strength DB]`; the reference service's dspMode): 1 = every file is denoised, high-passed
    and levelled on the device before anything reads it (WhisperModel.transcribe: dsp_mode; dsp.DspParams or a dict of its fields
    is accepted here too), with every form of the run; with `diarize` a file is enhanced once and its transcription and its diarization read the
    same samples (_EnhancedOnce); dsp_strength replaces
    DspParams.strength_db.  Off by default; its effect on CER is unmeasured.
    prompt_words (`--prompt-words a,b,c [--prompt-word-boost X]`): names and proper nouns of the recordings (the reference
    service's promptWords); tokens that continue one of them get a bonus on their logits (WhisperModel.transcribe: prompt_words,
    prompt_word_boost).  With the one-by-one and the lock-step form, on every engine context of a pipelined run; refused with
    continuous and with batched (ValueError before a model is built), whose sessions do not apply the table.
    diarize (`--diarize --seg-model PATH --spk-model PATH [--num-speakers N]`): every file is also diarized on the device
    (WhisperModel.load_diarization, WhisperModel.diarize) and `<name>_dia.srt`, the speaker-labelled subtitle, is written beside
    the unchanged `<name>_asr.txt`; with every form of the run, after the file's segments are there.  A model handed in that
    already holds the networks needs no paths.
    clip_timestamps (`--clip-timestamps "a,b,..."`): only those spans (seconds: start,end,start,end,...) of every file are
    decoded (WhisperModel.transcribe).  hallucination_silence_threshold (`--hallucination-silence-threshold S`): silence longer
    than S seconds around text whose words look invented is skipped; it works on word times and so implies word_timestamps.
    Both go with the one-by-one and the lock-step form; refused with continuous (ValueError before a model is built) and with
    batched, which has its own clip_timestamps meaning.
    audio_channel (`--audio-channel mix|left|right|N`): None / "mix" averages a file's channels as before; "left", "right" or
    an index from 0 transcribes that channel alone (two-party call recordings; the reference service's audioChannel 0 / 1 / 2 is
    mix / left / right).  On the host loader and, with device_resample, in the group's one device call.
    word_timestamps (`--word-timestamps`, with the lock-step form or continuous; not with batched): every file's segments are
    transcribed with words (continuous: one Session.align call per poll through the packed, pass-mate-independent alignment
    pass, WhisperModel.transcribe_many(continuous=True, word_timestamps=True)) and written to `<name>_words.json` beside
    `<name>_asr.txt`; texts and scores do not change.
    batched (`--batched`): every file is decoded by the batched pipeline (WhisperModel.transcribe_batched): its VAD chunks packed
    into groups of at most 30 s, all groups independent clips of one session.  One file at a time on one engine context; refused
    together with continuous, which batches across files instead.
    device_resample (`--device-resample`): the grouped paths hand every group's files to the model as paths and the model
    converts, downmixes and resamples them in one device call per group (WhisperModel.transcribe_many(device_resample=True))
    instead of `load_audio` file by file on this thread; the one-by-one path keeps `load_audio`.
    vad_model (`--vad-model PATH`): the Silero-v5 VAD network for the device (WhisperModel(vad_model=...)); with it the folder
    keeps its lock-step / continuous / pipelined path and every group is filtered in one device call (vad_filter=True).  A
    Python vad_speech_prob_fn on the model still means file by file.
    language: the forced language of every file (the reference's "zh"), or None = detect each file's language (`--language
    auto`); the detected language and its probability are then part of every entry of `detailed_results`.
    detect_in_session (`--detect-in-session`, with continuous and language None): the session finds each file's language in the
    first decode step of its first window instead of a detection pass, with its own encoder pass, before the session.
    session_prefill (`--session-prefill N`, with continuous): windows whose prompt has at least N prefillable positions get them from
    one admission pass of the session instead of N forced decode steps (WhisperModel.transcribe_many(session_prefill=N))."""
    if session_prefill and not continuous:
        raise ValueError("session_prefill needs continuous=True")
    if batched and continuous:
        raise ValueError("batched and continuous exclude each other (one file's groups, or many files' windows, per session)")
    if batched and word_timestamps:
        raise ValueError("word_timestamps goes with the lock-step form or continuous, not with batched")
    options = {}
    if clip_timestamps is not None and str(clip_timestamps).strip() not in ("", "0"):
        options["clip_timestamps"] = clip_timestamps
    if hallucination_silence_threshold is not None:
        options["hallucination_silence_threshold"] = float(hallucination_silence_threshold)
        word_timestamps = True
    if options and continuous:
        from .model import refuse_in_session
        refuse_in_session("process_audio_folder(continuous=True) / --continuous", clip_timestamps, hallucination_silence_threshold)
    if options and batched:
        raise ValueError("clip_timestamps / hallucination_silence_threshold go with the one-by-one or the lock-step form, not with batched")
    if prompt_words:
        from .seq_bias import refuse_in_session as refuse_bias
        if continuous or batched:
            refuse_bias("process_audio_folder(continuous=True / batched=True) / --continuous / --batched", prompt_words=prompt_words)
        options["prompt_words"] = prompt_words
        if prompt_word_boost is not None:
            options["prompt_word_boost"] = float(prompt_word_boost)
    from . import dsp
    dsp_params = dsp.resolve(dsp_mode)
    if dsp_strength is not None:
        if dsp_params is None:
            raise ValueError("dsp_strength goes with dsp_mode (--dsp-strength with --dsp-mode 1)")
        dsp_params = dsp.replace(dsp_params, strength_db=float(dsp_strength)).check()
    dsp_options = {} if dsp_params is None else {"dsp_mode": dsp_params}
    options.update(dsp_options)
    if continuous:
        if int(pipeline_depth or getattr(model, "pipeline_depth", 1)) > 1:
            log("continuous mode runs one session on one engine context: pipeline depth 1")
        pipeline_depth = 1
    pick = parse_audio_channel(audio_channel)
    if pick is not None:
        if load_audio is not _load_audio:
            raise ValueError("audio_channel goes with the built-in loader (a custom load_audio picks its own channel)")
        load_audio = functools.partial(_load_audio, channel=pick)
    files = list_audio_files(folder_path)
    if not files:
        log(f"no audio files in {folder_path}")
        return None
    if model is None:
        from .model import WhisperModel
        model = WhisperModel(model_path, device=device, device_index=device_index, compute_type=compute_type,
                             max_batch=max_batch, pipeline_depth=max(1, pipeline_depth), cross_kv_fp8=cross_kv_fp8,
                             vad_model=vad_model)
    dia = None
    if diarize:
        if seg_model is not None and spk_model is not None:
            model.load_diarization(seg_model, spk_model)
        elif not getattr(model, "has_diarization", False):
            raise ValueError("diarize needs seg_model and spk_model (--seg-model, --spk-model)")
        dia = dict(num_speakers=num_speakers)
    once = None
    if dia is not None and dsp_params is not None:
        # two passes read every file: the loader enhances it once for both, and neither pass is asked to enhance
        once = load_audio = _EnhancedOnce(model, load_audio, dsp_params, bool(device_resample), pick)
        options = {k: v for k, v in options.items() if k != "dsp_mode"}
        dsp_options = {}

    def one_file(f, **kw):
        try:
            return transcribe_file(model, f, load_audio, log, language=language, diarize=dia, **kw)
        finally:
            if once is not None:
                once.forget()
    mine = files[rank::world]                                   # shard by file
    results = []
    many = getattr(model, "transcribe_many", None)
    group = group_files if group_files > 0 else max(1, getattr(model, "max_batch", 1) // TRANSCRIBE_KWARGS["beam_size"])
    if batched:
        results = [one_file(f, batched=True, options=dsp_options) for f in mine]
    elif many is None or group < 2 or getattr(model, "vad_speech_prob_fn", None) is not None:
        results = [one_file(f, word_timestamps=word_timestamps, options=options) for f in mine]
    else:
        # MI355X-first: `group` files advance in lock step through one engine pass per window round; every file keeps the
        # sequential algorithm (own seek / prompt / fallback), so the outputs equal the one-by-one run
        kw = {k: v for k, v in TRANSCRIBE_KWARGS.items() if k != "vad_filter"}   # no VAD source configured: all-speech
        if getattr(model, "has_device_vad", False):
            kw["vad_filter"] = True   # the device network filters a whole group in one call: the reference's vad_filter=True
        kw["language"] = language
        if continuous:
            # one continuous-batching session per group on one engine context: windows of the group's files refill decode rows
            # as others finish, fallback attempts included (WhisperModel.transcribe_many(continuous=True))
            kw["continuous"] = True
            if detect_in_session and language is None:
                kw["detect_in_session"] = True
            if session_prefill:
                kw["session_prefill"] = int(session_prefill)
        if device_resample and once is None:
            kw["device_resample"] = True
            if pick is not None:
                kw["audio_channel"] = pick
        if word_timestamps:
            kw["word_timestamps"] = True
        kw.update(options)   # with vad_filter and clips, transcribe_many decides per file and warns, as transcribe does
        depth0 = max(1, int(pipeline_depth or getattr(model, "pipeline_depth", 1)))
        if group_files <= 0 and depth0 > 1 and len(mine) < group * depth0:
            group = max(1, -(-len(mine) // depth0))            # few files: one group per context rather than one big group and an idle lane
        parts = [mine[g:g + group] for g in range(0, len(mine), group)]
        # round 6: with pipeline_depth > 1 the groups are transcribed by that many engine contexts of the model at once (one shared
        # copy of the weights; one group's log-mel / encoder under another's decode) - same groups, same results, in file order.
        # Audio is loaded a few groups ahead only (a folder may hold many hours).
        depth = max(1, int(pipeline_depth or getattr(model, "pipeline_depth", 1)))
        if continuous:
            depth = 1
        groups_fn = getattr(model, "transcribe_groups", None) if depth > 1 else None
        span = 2 * depth if groups_fn is not None else 1
        for g0 in range(0, len(parts), span):
            chunk = parts[g0:g0 + span]
            if once is not None:
                once.forget()   # the chunk before is written: its enhanced samples go
            loaded_of, audios_of = [], []
            for part in chunk:
                audios, loaded = [], []
                for f in part:
                    try:
                        audios.append(_probe(f) if device_resample and once is None else load_audio(f))
                        loaded.append(None)
                    except Exception as e:
                        loaded.append(e)
                audios_of.append(audios)
                loaded_of.append(loaded)
            done_of = None
            if groups_fn is not None and len(chunk) > 1:
                try:
                    done_of = groups_fn(audios_of, pipeline_depth=depth, **kw)
                except Exception as e:
                    log(f"pipelined transcription failed ({e}); retrying group by group")
            for gi, part in enumerate(chunk):
                try:
                    if done_of is not None:
                        done = iter(done_of[gi])
                    else:
                        done = iter(many(audios_of[gi], **kw)) if audios_of[gi] else iter(())
                    pairs = [(err, None) if err is not None else next(done) for err in loaded_of[gi]]
                except Exception as e:  # engine-level failure of the group: fall back to one by one
                    log(f"group transcription failed ({e}); retrying file by file")
                    pairs = [(None, None)] * len(part)
                results.extend(transcribe_file(model, f, load_audio, log, segments=sg, language=language, info=nfo,
                                               word_timestamps=word_timestamps, options=options, diarize=dia)
                               for f, (sg, nfo) in zip(part, pairs))
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, results)
        order = {os.path.basename(f): i for i, f in enumerate(files)}
        results = sorted((r for part in gathered for r in part), key=lambda r: order[r["audio_file"]])
    final = summarise(results)
    # the opt-in e4m3 cross-attention cache (WhisperModel(cross_kv_fp8=True)) is named in the summary; a run on the 16-bit cache
    # keeps the reference's summary keys exactly
    if getattr(model, "cross_kv_fp8", False):
        final["summary"]["cross_kv_cache"] = "fp8_e4m3"
    if rank == 0:
        path = output_json or os.path.join(os.getcwd(), "asr_comparison_results.json")
        with open(path, "w", encoding="utf-8") as f:
            json.dump(final, f, ensure_ascii=False, indent=2)
        s = final["summary"]
        log(f"{s['total_files']} files, {s['files_with_cer']} scored, average CER {s['average_cer']:.4f}; wrote {path}")
    return final


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Transcribe every audio file of a folder on MI355X and score against transcripts")
    ap.add_argument("folder")
    ap.add_argument("--output", default="transcription_results.txt", help="accepted for compatibility; unused")
    ap.add_argument("--model", default="models", help="HF-format Whisper directory, or synthetic:<preset>")
    ap.add_argument("--compute-type", default="float16")
    ap.add_argument("--group-files", type=int, default=0,
                    help="files transcribed in lock step per engine pass (0 = as many as fit: max_batch // beam; 1 = one by one)")
    ap.add_argument("--max-batch", type=int, default=120,
                    help="decode rows of an engine context (files in a group x beam 5; the weight-streaming decode GEMMs carry up to 128 "
                         "rows).  Measured on 48 x 60 s files with two contexts: 30 rows 893, 60 rows 1 064, 120 rows 1 212 audio-s/s; a "
                         "context holds 11 / 23 / 44 GB of KV caches and workspaces at 30 / 60 / 120 rows of large-v3")
    ap.add_argument("--pipeline-depth", type=int, default=2,
                    help="groups of files in flight per GPU (engine contexts sharing one copy of the weights; 1 = the reference's "
                         "serial loop, asr_core.py:151); results do not depend on it")
    ap.add_argument("--continuous", action="store_true",
                    help="opt-in: decode each group's windows in one continuous-batching session (finished rows are refilled, "
                         "fallback attempts run in the session); pipeline depth 1.  Same per-file algorithm")
    ap.add_argument("--batched", action="store_true",
                    help="opt-in: decode each file through the batched pipeline (VAD chunks packed into groups of at most 30 s, all "
                         "groups of a file in one session, no previous-text conditioning); not together with --continuous")
    ap.add_argument("--xkv-fp8", action="store_true",
                    help="opt-in serving mode: decode from the e4m3 copy of the cross-attention cache (16-bit compute types; "
                         "WhisperModel(cross_kv_fp8=True)); the summary JSON names the cache that was read")
    ap.add_argument("--vad-model", default=None, metavar="PATH",
                    help="Silero-v5 VAD weights (.npz, or a TorchScript / state-dict file when torch is installed): vad_filter=True "
                         "then runs the network on the device, one call per group of files, and the folder keeps its grouped path")
    ap.add_argument("--language", default=TRANSCRIBE_KWARGS["language"],
                    help="language code forced on every file (default: the reference's zh), or 'auto': detect each file's language "
                         "on the device; the summary JSON then holds language and language_probability per file")
    ap.add_argument("--detect-in-session", action="store_true",
                    help="opt-in, with --continuous --language auto: each file's language is found inside the session, in the first "
                         "decode step of its first window, instead of a detection pass with its own encoder pass beforehand")
    ap.add_argument("--session-prefill", type=int, default=0, metavar="N",
                    help="opt-in, with --continuous: a window whose prompt has at least N prefillable positions (previous text up to "
                         "<|startoftranscript|>) gets them from one admission pass of the session instead of N forced decode steps; "
                         "0 = off")
    ap.add_argument("--word-timestamps", action="store_true",
                    help="opt-in: word-level timestamps; every file's segments with their words are written to <name>_words.json "
                         "beside <name>_asr.txt.  With --continuous the windows that settle in one poll are aligned in one device pass "
                         "whose result for a file does not depend on the other files; not together with --batched")
    ap.add_argument("--clip-timestamps", default="0", metavar="a,b,...",
                    help="decode only these spans of every file: seconds as start,end,start,end,... (an odd count runs the last span "
                         "to the end of the file); not together with --continuous or --batched")
    ap.add_argument("--hallucination-silence-threshold", type=float, default=None, metavar="S",
                    help="skip silence longer than S seconds around text whose words look invented; implies --word-timestamps; not "
                         "together with --continuous or --batched")
    ap.add_argument("--prompt-words", default=None, metavar="a,b,c",
                    help="keywords of the recordings' content - names, proper nouns - separated by commas: tokens that continue one "
                         "of them get a bonus on their logits; not together with --continuous or --batched")
    ap.add_argument("--prompt-word-boost", type=float, default=None, metavar="X",
                    help="with --prompt-words: the bonus (default 2.0, a starting value that has not been measured on real speech)")
    ap.add_argument("--dsp-mode", type=int, choices=(0, 1), default=0,
                    help="audio optimisation (the reference service's dspMode): 1 = denoise, high-pass and level every file on the device "
                         "before it is transcribed (default 0 = off; the effect on CER has not been measured)")
    ap.add_argument("--dsp-strength", type=float, default=None, metavar="DB",
                    help="with --dsp-mode 1: the deepest attenuation of the denoiser in dB, 0 ... 40 (default 12)")
    ap.add_argument("--device-resample", action="store_true",
                    help="opt-in: convert, downmix and resample each group's files in one device call instead of file by file on "
                         "the host (RIFF/WAVE of any PCM / float format; FLAC files, decoded on the device frame by frame; other "
                         "containers through soundfile; rates the device "
                         "does not take fall back to the host path per file)")
    ap.add_argument("--audio-channel", default="mix", metavar="{mix,left,right,N}", type=_audio_channel_arg,
                    help="which channel of a multichannel file is transcribed: mix = the mean of all (default), left / right = "
                         "channel 0 / 1, N = channel N counted from 0 (the reference service's audioChannel 0 / 1 / 2 is mix / "
                         "left / right); a file without that channel is that file's error")
    ap.add_argument("--diarize", action="store_true",
                    help="opt-in: also answer who spoke when; <name>_dia.srt, the speaker-labelled subtitle (cues 'SPEAKER_xx: text'), "
                         "is written beside <name>_asr.txt.  Needs --seg-model and --spk-model")
    ap.add_argument("--seg-model", default=None, metavar="PATH",
                    help="with --diarize: pyannote/segmentation-shaped weights (.npz, or a torch checkpoint when torch is installed)")
    ap.add_argument("--spk-model", default=None, metavar="PATH",
                    help="with --diarize: pyannote/embedding-shaped (XVectorSincNet) weights, same formats")
    ap.add_argument("--num-speakers", type=int, default=None, metavar="N",
                    help="with --diarize: the number of speakers of every file, when it is known (default: found by clustering)")
    return ap


def _audio_channel_arg(value: str) -> str:
    try:
        parse_audio_channel(value)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return value


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.session_prefill < 0 or (args.session_prefill and not args.continuous):
        print("--session-prefill needs a value >= 0 and --continuous")
        return 1
    if args.batched and args.continuous:
        print("--batched and --continuous exclude each other")
        return 1
    if args.batched and args.word_timestamps:
        print("--word-timestamps goes with the lock-step form or --continuous, not with --batched")
        return 1
    if args.clip_timestamps.strip() not in ("", "0") or args.hallucination_silence_threshold is not None:
        if args.continuous or args.batched:
            print("--clip-timestamps / --hallucination-silence-threshold go with the one-by-one or the lock-step form "
                  "(--group-files), not with --continuous or --batched")
            return 1
    if args.prompt_words and (args.continuous or args.batched):
        print("--prompt-words goes with the one-by-one or the lock-step form (--group-files), not with --continuous or --batched")
        return 1
    if args.prompt_word_boost is not None and not args.prompt_words:
        print("--prompt-word-boost goes with --prompt-words")
        return 1
    if args.dsp_strength is not None and not args.dsp_mode:
        print("--dsp-strength goes with --dsp-mode 1")
        return 1
    if args.diarize and not (args.seg_model and args.spk_model):
        print("--diarize needs --seg-model PATH and --spk-model PATH")
        return 1
    if not args.diarize and (args.seg_model or args.spk_model or args.num_speakers is not None):
        print("--seg-model / --spk-model / --num-speakers go with --diarize")
        return 1
    if not os.path.exists(args.folder):
        print(f"folder does not exist: {args.folder}")
        return 1
    rank, world, local = 0, 1, 0
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        from .dist import init_process_group
        rank, world, local = init_process_group()
    process_audio_folder(args.folder, model_path=args.model, device="cuda", device_index=local,
                         compute_type=args.compute_type, rank=rank, world=world, group_files=args.group_files,
                         max_batch=args.max_batch, pipeline_depth=args.pipeline_depth, continuous=args.continuous,
                         cross_kv_fp8=args.xkv_fp8, language=None if args.language == "auto" else args.language,
                         detect_in_session=args.detect_in_session, session_prefill=args.session_prefill,
                         vad_model=args.vad_model, device_resample=args.device_resample, batched=args.batched,
                         word_timestamps=args.word_timestamps, audio_channel=args.audio_channel,
                         clip_timestamps=args.clip_timestamps, hallucination_silence_threshold=args.hallucination_silence_threshold,
                         diarize=args.diarize, seg_model=args.seg_model, spk_model=args.spk_model, num_speakers=args.num_speakers,
                         prompt_words=args.prompt_words, prompt_word_boost=args.prompt_word_boost,
                         dsp_mode=args.dsp_mode, dsp_strength=args.dsp_strength)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
