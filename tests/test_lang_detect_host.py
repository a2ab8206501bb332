"""CPU: the host side of language detection - the segments / threshold rule, the `language` argument of the batched surfaces,
the options that used to be ignored, per-window detection through the window loop (driven by the CPU oracle standing in for the
engine) and the folder tool's `--language auto`."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from oracle_engine import OracleEngine
from taiwan_tongues_asr_ce_amd import batch_cli, synth
from taiwan_tongues_asr_ce_amd.model import LANGUAGES, TranscriptionInfo, WhisperModel, select_language

torch.set_grad_enabled(False)


@pytest.mark.parametrize("tops, threshold, want", [
    ([("zh", 0.9), ("en", 0.99)], 0.5, ("zh", 0.9, 0)),                                  # early stop at the first window
    ([("zh", 0.4), ("en", 0.7), ("zh", 0.45)], 0.5, ("en", 0.7, 1)),                     # ... at a later one
    ([("zh", 0.4), ("en", 0.45), ("zh", 0.3)], 0.5, ("zh", 0.4, 0)),                     # majority, its largest probability
    ([("en", 0.2), ("zh", 0.3), ("zh", 0.45), ("en", 0.1)], 0.5, ("en", 0.2, 0)),        # tie: the language seen first
    ([("zh", 0.5)], 0.5, ("zh", 0.5, 0)),                                                # "exceeds" is strict: a vote of one
    ([("ja", 0.1)], 0.5, ("ja", 0.1, 0)),                                                # k larger than the file: what there is
    ([("ja", 0.1), ("ko", 0.2)], None, ("ja", 0.1, 0)),                                  # no threshold: the first window
])
def test_select_language_rule(tops, threshold, want):
    assert select_language(tops, threshold) == want


def test_select_language_needs_a_window():
    with pytest.raises(ValueError):
        select_language([], 0.5)


class DetectingOracle(OracleEngine):
    """The oracle engine with Engine.detect_language: softmax over the language span of the logits after <|startoftranscript|>."""

    def language_span(self):
        st = self.special
        return st.sot + 1, max(1, min(min(st.translate, st.transcribe) - st.sot - 1, len(LANGUAGES)))

    def load_weights(self, tensors):
        b, n = self.language_span()
        sd = {k: np.array(v, dtype=np.float32) for k, v in tensors}
        sd["model.decoder.embed_tokens.weight"][b:b + n] *= 16.0      # a decisive language head (test_gpu_lang_detect.py)
        super().load_weights(sd.items())

    def detect_language(self, B, want_logits=False, span=None):
        b, n = span or self.language_span()
        self.calls.append(("detect_language", B))
        lg = R.decoder_forward(torch.full((B, 1), self.special.sot), R.SelfCache.empty(self.rd.dec_layers),
                               R.cross_kv(self.enc[:B], self.W, self.rd), self.W, self.rd)[:, 0, b:b + n]
        probs = torch.softmax(lg.double(), dim=-1).numpy().astype(np.float32)
        idx = probs.argmax(axis=1).astype(np.int32)
        return (idx, probs, lg.numpy()) if want_logits else (idx, probs)


KINDS = (synth.noise_clip, synth.tonal_clip, synth.burst_clip, synth.noise_clip)
QUIET = dict(temperature=0.0, no_speech_threshold=None, log_prob_threshold=None, compression_ratio_threshold=None,
             max_new_tokens=3, condition_on_previous_text=False)


@pytest.fixture(scope="module")
def oracle_model():
    return WhisperModel("synthetic:tiny", compute_type="float32", max_batch=2, _engine_factory=DetectingOracle)


def test_multilingual_detects_every_window_between_encode_and_generate(oracle_model):
    """clip 2 then clip 5 as one file: the two prompts carry LANGUAGES[24] then LANGUAGES[5]; one encoder pass per window plus
    the file-level detection's, and each window's detection sits between its encode and its generate."""
    m = oracle_model
    m.engine.calls.clear()
    audio = np.concatenate([KINDS[2](2), KINDS[1](5)])
    segs, info = m.transcribe(audio, language=None, beam_size=1, multilingual=True, without_timestamps=True, **QUIET)
    list(segs)
    sot = m.special.sot
    calls = m.engine.calls
    assert [c[0] for c in calls] == ["detect_language", "detect_language", "generate", "detect_language", "generate"]
    assert [c[1][c[1].index(sot) + 1] - sot - 1 for c in calls if c[0] == "generate"] == [24, 5]
    assert info.language == LANGUAGES[24] and info.all_language_probs[0] == (info.language, info.language_probability)
    assert len(info.all_language_probs) == 99
    # without multilingual the file-level language is in every prompt
    m.engine.calls.clear()
    segs, _ = m.transcribe(audio, language=None, beam_size=1, without_timestamps=True, **QUIET)
    list(segs)
    assert [c[1][c[1].index(sot) + 1] - sot - 1 for c in m.engine.calls if c[0] == "generate"] == [24, 24]


def test_detection_segments_and_threshold_reach_the_rule(oracle_model, monkeypatch):
    m = oracle_model
    seen = {}

    def fake_batch(windows):
        seen["n"] = [len(w) for w in windows]
        return [("zh", 0.4, [("zh", 0.4)]), ("en", 0.3, [("en", 0.3)]), ("zh", 0.45, [("zh", 0.45)])][:len(windows)]
    monkeypatch.setattr(m, "detect_language_batch", fake_batch)
    monkeypatch.setattr(m, "_generate_segments", lambda *a, **k: iter(()))
    audio = np.zeros(m.n_window * 2 + 1600, np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # the three options are implemented: no "ignored" warning
        _, info = m.transcribe(audio, language=None, beam_size=1, language_detection_segments=5,
                               language_detection_threshold=0.6, multilingual=False)
        assert (info.language, info.language_probability, info.all_language_probs) == ("zh", 0.45, [("zh", 0.45)])
        assert seen["n"] == [len(audio), len(audio) - m.n_window, 1600]    # k larger than the file: its three windows
        _, info = m.transcribe(audio, language=None, beam_size=1, language_detection_segments=2,
                               language_detection_threshold=0.25)
        assert (info.language, info.language_probability) == ("zh", 0.4) and len(seen["n"]) == 2
        _, info = m.transcribe(audio, language="ja", beam_size=1, multilingual=True)
        assert (info.language, info.language_probability, info.all_language_probs) == ("ja", 1.0, None)
    with pytest.raises(ValueError):
        m.transcribe(audio, language=None, beam_size=1, language_detection_segments=0)


def test_language_lists_are_validated(oracle_model):
    m = oracle_model
    clips = [np.zeros(1600, np.float32)] * 3
    for fn in (m.transcribe_many, m.transcribe_batch, m.transcribe_windows, m.transcribe_stream):
        with pytest.raises(ValueError, match="one entry per"):
            fn(clips, language=["zh", None])
        with pytest.raises(ValueError, match="unknown language"):
            fn(clips, language=["zh", "xx", None])
        with pytest.raises(ValueError, match="language code or None"):
            fn(clips, language=["zh", 3, None])
    with pytest.raises(ValueError, match="continuous"):
        m.transcribe_many(clips, language=None, continuous=True, multilingual=True)
    assert m._check_languages("zh", 2, "file") == ["zh", "zh"] and m._check_languages(None, 2, "file") == [None, None]
    assert m._check_languages(("en", None), 2, "file") == ["en", None]


def test_transcribe_many_reports_each_files_language(oracle_model):
    m = oracle_model
    files = [KINDS[2](2)[:m.n_window], KINDS[1](5)[:m.n_window]]
    auto = m.transcribe_many(files, language=[None, None], beam_size=1, **QUIET)
    assert [i.language for _, i in auto] == [LANGUAGES[24], LANGUAGES[5]]
    assert all(i.all_language_probs[0] == (i.language, i.language_probability) for _, i in auto)
    given = m.transcribe_many(files, language=[LANGUAGES[24], LANGUAGES[5]], beam_size=1, **QUIET)
    assert [s for s, _ in auto] == [s for s, _ in given]
    assert all(i.language_probability == 1.0 and i.all_language_probs is None for _, i in given)


class _Seg:
    text = "好"


class _AutoModel:
    max_batch = 10

    def __init__(self):
        self.languages = []

    def transcribe_many(self, audios, language=None, **kw):
        self.languages.append(language)
        return [([_Seg()], TranscriptionInfo("yue" if language is None else language, 0.75 if language is None else 1.0, 1.0, 1.0))
                for _ in audios]

    def transcribe(self, audio, language=None, **kw):
        self.languages.append(language)
        return [_Seg()], TranscriptionInfo("yue" if language is None else language, 0.75 if language is None else 1.0, 1.0, 1.0)


@pytest.mark.parametrize("group", [1, 2])
def test_folder_tool_language_auto(tmp_path, monkeypatch, group):
    folder = tmp_path / "audio"
    folder.mkdir()
    for n in ("a.wav", "b.wav"):
        (folder / n).write_bytes(b"")
    assert batch_cli.build_parser().parse_args(["x"]).language == "zh"
    assert batch_cli.build_parser().parse_args(["x", "--language", "auto"]).language == "auto"
    made = []
    monkeypatch.setattr(batch_cli, "process_audio_folder", lambda *a, **k: made.append(k))
    batch_cli.main([str(folder), "--language", "auto"])
    batch_cli.main([str(folder)])
    assert [k["language"] for k in made] == [None, "zh"]
    monkeypatch.undo()
    model = _AutoModel()
    out = tmp_path / "out.json"
    batch_cli.process_audio_folder(str(folder), model=model, output_json=str(out), log=lambda *_: None, group_files=group,
                                   pipeline_depth=1, load_audio=lambda f: np.zeros(16, np.float32), language=None)
    got = json.load(open(out, encoding="utf-8"))["detailed_results"]
    assert [(r["language"], r["language_probability"]) for r in got] == [("yue", 0.75)] * 2 and set(model.languages) == {None}
    batch_cli.process_audio_folder(str(folder), model=model, output_json=str(out), log=lambda *_: None, group_files=group,
                                   pipeline_depth=1, load_audio=lambda f: np.zeros(16, np.float32))
    got = json.load(open(out, encoding="utf-8"))["detailed_results"]
    assert all("language" not in r for r in got) and model.languages[-1] == "zh"      # the default run keeps the reference's keys


def test_streaming_backend_language_argument(caplog):
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    with pytest.raises(ValueError, match="lock-step"):
        BatchedWhisperASR(continuous=True, language=None)         # refused before any model is built
    asr = BatchedWhisperASR.__new__(BatchedWhisperASR)
    asr.text_filter = None
    assert asr._result_dict(("好", 1.0), 0.0)["language"] == "zh" and asr._result_dict(("好", 1.0), 0.0)["language_probability"] == 1.0
    with caplog.at_level("WARNING"):
        d = asr._result_dict(("好", 1.0), 0.0, ("yue", 0.4))
    assert (d["language"], d["language_probability"]) == ("yue", 0.4) and "0.40" in caplog.text
