"""GPU: BatchedInferencePipeline - one long recording cut into groups, every group an independent clip of one hold-mode beam
session, fallbacks by Session.retry.

Every group must come out exactly as transcribe_many(continuous=True) decodes a one-window file made of that group's audio
(tokens, text, temperature and scores bit for bit; times through the group's map), whether a failing group is retried on its held
cross-KV or released and submitted again, and whatever the number of groups in flight.  Words are those of a hand-made
hold-mode session plus WhisperModel._window_words; VAD groups are merge_chunks over the device network's probabilities;
detected languages are detect_language_batch's.

Geometry: preset tiny, synthetic weights, max_batch 6, beam 2 (3 groups of rows in flight)."""
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import BatchedInferencePipeline, synth, vad
from taiwan_tongues_asr_ce_amd.batched import restore_group_times
from taiwan_tongues_asr_ce_amd.engine import Engine, Session
from taiwan_tongues_asr_ce_amd.model import Segment, WhisperModel, Word, select_language
from vad_reference import test_signal as vad_signal

pytestmark = pytest.mark.gpu

SR = 16000
# 7 groups of 2-6 s in a 60-s recording
CLIPS = [(1.0, 4.0), (6.5, 8.5), (10.0, 16.0), (20.25, 24.75), (30.0, 33.5), (40.0, 45.0), (52.0, 57.5)]
KW = dict(language="zh", beam_size=2, best_of=2, temperature=(0.0, 0.4, 0.8), max_new_tokens=12, without_timestamps=True)
OFF = dict(log_prob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)


def _recording():
    return np.concatenate([synth.noise_clip(800), synth.noise_clip(801)]).astype(np.float32)


def _clip_ts():
    return [dict(start=a, end=b) for a, b in CLIPS]


def _run(m, audio, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        segs, info = BatchedInferencePipeline(m).transcribe(audio, **kw)
        return list(segs), info


@pytest.fixture(scope="module")
def model():
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="bfloat16", max_batch=6)
    yield m
    m.close()


@pytest.fixture(scope="module")
def runs(model):
    """The pipeline's runs over the 60-s recording, decoded once and shared."""
    audio = _recording()
    out = dict(audio=audio)
    out["retry"] = _run(model, audio, clip_timestamps=_clip_ts(), **KW)
    out["resubmit"] = _run(model, audio, clip_timestamps=_clip_ts(), retry_held=False, **KW)
    out["one"] = _run(model, audio, clip_timestamps=_clip_ts(), batch_size=1, **KW)
    out["off"] = _run(model, audio, clip_timestamps=_clip_ts(), **KW, **OFF)
    return out


def test_every_group_equals_transcribe_many_of_its_audio(model, runs):
    audio = runs["audio"]
    segs, info = runs["retry"]
    groups = [audio[int(a * SR):int(b * SR)] for a, b in CLIPS]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = model.transcribe_many(groups, continuous=True, condition_on_previous_text=False, **KW)
    assert len(info.chunks) == 7 and [s.id for s in segs] == list(range(len(segs)))
    assert [s.seek for s in segs] == sorted(s.seek for s in segs)                        # group order
    n_checked = 0
    for (a, b), chunk, (ref, _) in zip(CLIPS, info.chunks, want):
        mine = [s for s in segs if s.seek == chunk["start"] // 160]
        assert (chunk["start"], chunk["end"]) == (int(a * SR), int(b * SR)) and chunk["segments"] == [dict(start=chunk["start"], end=chunk["end"])]
        assert len(mine) == len(ref)
        for s, r in zip(mine, ref):
            assert (s.tokens, s.text, s.temperature) == (r.tokens, r.text, r.temperature)
            assert (s.avg_logprob, s.no_speech_prob, s.compression_ratio) == (r.avg_logprob, r.no_speech_prob, r.compression_ratio)
            mapped, = restore_group_times([r], chunk["segments"])
            assert (s.start, s.end) == (mapped.start, mapped.end) == (round(a + r.start, 2), round(a + r.end, 2))
            n_checked += 1
    assert n_checked >= 5
    assert info.duration == 60.0 and abs(info.duration_after_vad - sum(b - a for a, b in CLIPS)) < 1e-9
    assert info.language == "zh" and info.transcription_options["condition_on_previous_text"] is False


def test_retries_encode_each_group_once_and_change_nothing(runs):
    segs, info = runs["retry"]
    again, info2 = runs["resubmit"]
    assert again == segs and [c["attempts"] for c in info2.chunks] == [c["attempts"] for c in info.chunks]
    attempts = sum(len(c["attempts"]) for c in info.chunks)
    assert info.session["clips_encoded"] == 7 and info.session["retries"] == attempts - 7 >= 1
    assert info2.session["clips_encoded"] == attempts and info2.session["retries"] == 0
    assert info2.session["encode_ms"] > 0 and info.session["steps"] > 0
    off, info3 = runs["off"]
    assert info3.session["retries"] == 0 and info3.session["clips_encoded"] == 7
    assert all(len(c["attempts"]) == 1 and c["attempts"][0][0] == 0.0 for c in info3.chunks) and len(off) == 7


def test_one_group_in_flight_gives_the_same_segments(runs):
    assert runs["one"][0] == runs["retry"][0]
    assert [c["attempts"] for c in runs["one"][1].chunks] == [c["attempts"] for c in runs["retry"][1].chunks]


def test_words_equal_a_hand_made_hold_session(model):
    m = model
    audio = _recording()
    kw = dict(language="zh", beam_size=2, best_of=2, temperature=0.0, max_new_tokens=12, without_timestamps=True, **OFF)
    # one group in flight: every alignment pass holds one sequence, as the hand-made session's does, and the words are equal
    # bit for bit.  At the default three groups in flight a pass holds several sequences padded to the longest; such a pass and
    # the one-sequence pass are not bit-identical, and the project's bars for that comparison apply:
    # the same words, probabilities within 0.15 in log space (bf16: test_gpu_align_batch.py), start and end equal for >= 90 %
    alone, info = _run(m, audio, clip_timestamps=_clip_ts(), word_timestamps=True, batch_size=1, **kw)
    together, info3 = _run(m, audio, clip_timestamps=_clip_ts(), word_timestamps=True, **kw)
    assert len(alone) == len(together) == 7 and all(s.words for s in alone + together)
    p = m._params("zh", "transcribe", False, True, 12, None, None, 1.0, True, 2, 1.0, (0.0,), 2, None, True, None, None)
    n_ctx = m.dims.n_text_ctx
    prompt, sot = m._prompt(p["lang_tok"], "transcribe", True, [], None, None)
    same = total = 0
    for seg, seg3, (a, b) in zip(alone, together, CLIPS):
        g = np.ascontiguousarray(audio[int(a * SR):int(b * SR)])
        floor = m._file_feature_max(g)
        with m.engine.session(m._window_opts(1, 0, p), n_ctx - 1, beam=2, patience=1.0) as s:
            s.hold()
            cid, = s.submit_windows([g], [0], [prompt], [sot], max_new=[min(12, n_ctx - len(prompt))], floor_max=[floor],
                                    temperature=[0.0], rows=[2], seed=[m._fallback_seed(0, 0.0)])
            r, = s.drain()
            words, = m._window_words(s, [cid], [r.tokens], [len(g)], "zh", p["lang_tok"], "transcribe")
        assert r.tokens == seg.tokens == seg3.tokens
        local = Segment(0, 0, 0.0, (b - a), seg.text, seg.tokens, 0.0, 0.0, 0.0, 0.0, [Word(**w) for w in words])
        want, = restore_group_times([local], [dict(start=int(a * SR), end=int(b * SR))])
        assert [(w.word, w.start, w.end, w.probability) for w in seg.words] == \
            [(w.word, w.start, w.end, w.probability) for w in want.words]
        assert (seg.start, seg.end) == (want.start, want.end)
        assert [w.word for w in seg3.words] == [w.word for w in want.words]
        for w3, w in zip(seg3.words, want.words):
            assert abs(np.log(w3.probability) - np.log(w.probability)) < 0.15
            same += (w3.start, w3.end) == (w.start, w.end)
            total += 1
        for w in seg.words + seg3.words:
            assert a - 1e-9 <= w.start <= w.end <= b + 1e-9                 # inside the group's one speech piece
    assert same >= 0.9 * total
    for i in (info, info3):
        assert i.session["retries"] == 0 and i.session["clips_encoded"] == 7


def test_device_vad_groups_and_segments(model):
    m = model
    m.load_vad(vad.synth_silero_weights())
    sig = vad_signal()
    quiet = dict(language="zh", beam_size=2, temperature=0.0, max_new_tokens=8, **OFF)
    probs = m.vad_speech_probs([sig])[0]
    for chunk_length, single in ((5.0, True), (12.0, False)):
        # max_speech_duration_s = chunk_length, min_silence_duration_ms = 160: the pipeline's VAD defaults
        speech = vad.get_speech_timestamps(sig, vad.VadOptions(max_speech_duration_s=chunk_length, min_silence_duration_ms=160),
                                           lambda a: probs)
        want = vad.merge_chunks(speech, int(chunk_length * SR))
        segs, info = _run(m, sig, chunk_length=chunk_length, **quiet)
        assert len(want) >= 3
        assert [(c["start"], c["end"], c["segments"]) for c in info.chunks] == [(g["start"], g["end"], g["segments"]) for g in want]
        assert abs(info.duration_after_vad - sum(e["end"] - e["start"] for e in speech) / SR) < 1e-9
        assert info.session["clips_encoded"] == len(want) and len(segs) >= 3
        if single:
            # bursts of at most 3 s, pads of 0.4 s and gaps of at least 2.5 s: no two chunks fit 5 s, every group is one piece,
            # and the same sample ranges given as clip_timestamps decode the same audio
            assert all(len(g["segments"]) == 1 for g in want)
            clips, _ = _run(m, sig, clip_timestamps=[dict(start=g["start"] / SR, end=g["end"] / SR) for g in want], **quiet)
            assert segs == clips
        else:
            assert any(len(g["segments"]) > 1 for g in want)
            for s in segs:
                g = next(g for g in want if g["start"] // 160 == s.seek)
                assert g["start"] / SR - 0.005 <= s.start < s.end <= g["end"] / SR + 0.005   # times are rounded to 10 ms


def _decisive_factory():
    """tiny with the language rows of embed_tokens multiplied by 16, so that the clips' languages are decided (and differ)."""
    class DecisiveEngine(Engine):
        def load_weights(self, tensors):
            b, n = self.language_span()

            def scaled():
                for name, arr in tensors:
                    if name == "model.decoder.embed_tokens.weight":
                        arr = np.array(arr, dtype=np.float32)
                        arr[b:b + n] *= 16.0
                    yield name, arr
            super().load_weights(scaled())
    return DecisiveEngine


def test_detected_languages_are_those_of_detect_language_batch(monkeypatch):
    # three groups of one full window each: the window form of a group's log-mel and detect_language_batch's single-clip form
    # are then the same features
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="bfloat16", max_batch=6, _engine_factory=_decisive_factory())
    try:
        audio = np.concatenate([synth.tonal_clip(1), synth.burst_clip(2), synth.noise_clip(5)]).astype(np.float32)
        n = m.n_window
        groups = [audio[i * n:(i + 1) * n] for i in range(3)]
        found = m.detect_language_batch(groups)
        assert len({f[0] for f in found}) >= 2
        kw = dict(beam_size=2, best_of=2, temperature=(0.0, 0.4), max_new_tokens=6, log_prob_threshold=0.0, no_speech_threshold=None,
                  clip_timestamps=[0.0, 30.0, 30.0, 60.0, 60.0, 90.0])
        # language=None: the file's language from the first two groups, by select_language
        segs, info = _run(m, audio, language=None, language_detection_segments=2, **kw)
        lang, prob, i = select_language([(f[0], f[1]) for f in found[:2]], 0.5)
        assert (info.language, info.language_probability) == (lang, prob) and info.all_language_probs == found[i][2]
        assert info.window_languages is None and all(len(c["attempts"]) == 2 for c in info.chunks)
        # multilingual=True: every group is detected inside the session; a retry carries the language its first attempt found
        retried = []
        retry = Session.retry

        def recording(self, ids, prompts, sot_index, **k):
            retried.extend((list(p), int(s)) for p, s in zip(prompts, sot_index))
            return retry(self, ids, prompts, sot_index, **k)
        monkeypatch.setattr(Session, "retry", recording)
        segs, info = _run(m, audio, language=None, multilingual=True, **kw)
        assert info.window_languages == [f[0] for f in found] and info.language == found[0][0]
        assert info.session["retries"] == 3 == len(retried) and info.session["clips_encoded"] == 3
        tokens = sorted(m._lang_token(f[0]) for f in found)
        assert sorted(p[s + 1] for p, s in retried) == tokens and all(Session.DETECT not in p for p, _ in retried)
    finally:
        m.close()
