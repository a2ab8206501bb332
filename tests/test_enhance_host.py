"""Host: audio enhancement above the library (taiwan_tongues_asr_ce_amd/dsp.py and the surfaces that take dsp_mode) - the
dsp_mode mapping, the folder tool's flags, the refusal on the live surfaces before a session or worker starts, and the one rule
of every file-level surface: enhancement runs once per file, before the VAD, and every later consumer reads the enhanced samples.
No GPU: the engines are the scripted doubles of tests/window_loop_stub.py with a recording `enhance`."""
import threading

import numpy as np
import pytest

import window_loop_stub as stub
from taiwan_tongues_asr_ce_amd import batch_cli, dsp


class DspEngine(stub.ScriptEngine):
    """`enhance` halves every recording (a result no other stage produces) and notes the call; the feature call notes whether the
    samples it was given are enhanced ones."""
    log = []          # ("enhance", engine id, lengths, params, thread) / ("vad", enhanced?) / ("mel", enhanced?) in order
    opened = []

    def __init__(self, dims, compute_type=0, max_batch=1, device=0, share_weights_with=None):
        super().__init__(dims, compute_type, max_batch, device)

    def enhance(self, audios, params=None, return_gain=False, **fields):
        assert isinstance(params, dsp.DspParams) and not fields
        DspEngine.log.append(("enhance", id(self), [len(a) for a in audios], params, threading.current_thread().name))
        return [np.asarray(a, np.float32) * np.float32(0.5) for a in audios]

    def log_mel_windows(self, audio, seeks, floor_max=None, want_output=False, want_max=False, **kw):
        files = [audio] if isinstance(audio, np.ndarray) else list(audio)
        if not want_max:
            DspEngine.log.append(("mel", all(_enhanced(a) for a in files)))
        return super().log_mel_windows(audio, seeks, floor_max, want_output, want_max, **kw)

    def session(self, *a, **k):
        DspEngine.opened.append((a, k))
        raise AssertionError("a session was opened")


AUDIO = np.full(16000 * 3, 0.25, np.float32)
SCRIPT = lambda n, seek, frames: dict(tokens=[stub.ts(0.0), 400, 401, stub.ts(2.0), stub.ST.eot], lp=-1.0)   # noqa: E731


def _enhanced(a) -> bool:
    return len(a) > 0 and bool(np.all(np.asarray(a) == np.float32(0.125)))


def _vad_fn(a):
    DspEngine.log.append(("vad", _enhanced(a)))
    return np.ones(-(-len(a) // 512), np.float32)


@pytest.fixture
def model():
    DspEngine.log, DspEngine.opened = [], []
    m = stub.make_model(SCRIPT, cls=DspEngine)
    yield m
    m.close()


def _kinds():
    return [e[0] for e in DspEngine.log]


# ---- the mapping ----------------------------------------------------------------------------------------------------------
def test_dsp_mode_mapping():
    for off in (None, 0, False):
        assert dsp.resolve(off) is None
    for on in (1, True):
        p = dsp.resolve(on)
        assert p == dsp.DspParams() and p.flags == 7
    assert (dsp.DSP_DENOISE, dsp.DSP_HIGHPASS, dsp.DSP_LEVEL) == (1, 2, 4)
    d = dsp.DspParams()
    assert (d.strength_db, d.oversubtract, d.max_gain) == (12.0, 3.0, 10.0) and abs(d.peak_target - 10 ** (-1 / 20)) < 1e-15
    p = dsp.resolve({"level": False, "strength_db": 18})
    assert p.flags == 3 and p.strength_db == 18 and p.oversubtract == 3.0
    given = dsp.DspParams(denoise=False, highpass=False, max_gain=4.0)
    assert dsp.resolve(given) is given and given.flags == 4


@pytest.mark.parametrize("bad, word", [
    (2, "must be None, 0, 1"), ("1", "must be None, 0, 1"), ({"gain": 2}, "unknown field"),
    ({"denoise": False, "highpass": False, "level": False}, "at least one"), ({"strength_db": -1}, r"outside \[0, 40\]"),
    ({"strength_db": 41}, r"outside \[0, 40\]"), ({"strength_db": float("nan")}, "finite"), ({"oversubtract": 0}, r"outside \(0, 16\]"),
    ({"oversubtract": 17}, r"outside \(0, 16\]"), ({"peak_target": 0}, r"outside \(0, 1\]"), ({"peak_target": 1.5}, r"outside \(0, 1\]"),
    ({"max_gain": 0.5}, "below 1"), ({"max_gain": float("inf")}, "finite"), (dsp.DspParams(max_gain=0.0), "below 1"),
])
def test_dsp_mode_refusals(bad, word):
    with pytest.raises(ValueError, match=word):
        dsp.resolve(bad)


# ---- the folder tool ------------------------------------------------------------------------------------------------------
def test_batch_cli_flags(tmp_path, capsys):
    args = batch_cli.build_parser().parse_args([str(tmp_path)])
    assert args.dsp_mode == 0 and args.dsp_strength is None
    args = batch_cli.build_parser().parse_args([str(tmp_path), "--dsp-mode", "1", "--dsp-strength", "18"])
    assert args.dsp_mode == 1 and args.dsp_strength == 18.0
    with pytest.raises(SystemExit):
        batch_cli.build_parser().parse_args([str(tmp_path), "--dsp-mode", "2"])
    capsys.readouterr()
    assert batch_cli.main([str(tmp_path), "--dsp-strength", "18"]) == 1
    assert "--dsp-strength" in capsys.readouterr().out
    with pytest.raises(ValueError, match="dsp_strength goes with dsp_mode"):
        batch_cli.process_audio_folder(str(tmp_path), model=object(), dsp_strength=18.0)
    with pytest.raises(ValueError, match=r"outside \[0, 40\]"):
        batch_cli.process_audio_folder(str(tmp_path), model=object(), dsp_mode=1, dsp_strength=50.0)


def test_folder_tool_hands_dsp_mode_to_every_file(tmp_path):
    for name in ("a.wav", "b.wav"):
        (tmp_path / name).write_bytes(b"")
    seen = []

    class Model:
        max_batch = 1

        def transcribe(self, audio, **kw):
            seen.append(kw.get("dsp_mode", "absent"))
            return [], None
    quiet = lambda *a: None   # noqa: E731
    out = str(tmp_path / "results.json")
    batch_cli.process_audio_folder(str(tmp_path), model=Model(), load_audio=lambda f: AUDIO, log=quiet, output_json=out, dsp_mode=1, dsp_strength=20)
    assert seen == [dsp.DspParams(strength_db=20.0)] * 2
    seen.clear()
    batch_cli.process_audio_folder(str(tmp_path), model=Model(), load_audio=lambda f: AUDIO, log=quiet, output_json=out)
    assert seen == ["absent"] * 2                     # off: the call is the one it was
    batch_cli.process_audio_folder(str(tmp_path), model=Model(), load_audio=lambda f: AUDIO, log=quiet, output_json=out, dsp_mode=0)
    assert seen == ["absent"] * 4


# ---- the live surfaces ----------------------------------------------------------------------------------------------------
def test_streaming_surfaces_refuse_before_a_session_or_worker_starts(model):
    with pytest.raises(ValueError, match="causal, stateful noise tracker"):
        model.transcribe_stream([AUDIO], dsp_mode=1)
    with pytest.raises(ValueError, match="causal, stateful noise tracker"):
        model.transcribe_stream([AUDIO], dsp_mode={"level": False})
    assert DspEngine.opened == [] and DspEngine.log == [] and model.engine.calls == []
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    before = threading.active_count()
    for kw in (dict(), dict(continuous=True)):
        with pytest.raises(ValueError, match="causal, stateful noise tracker"):
            BatchedWhisperASR(dsp_mode=1, model_path="synthetic:tiny", **kw)
    assert threading.active_count() == before
    dsp.refuse_streaming(None, "x"), dsp.refuse_streaming(0, "x")   # off: nothing to refuse
    with pytest.raises(ValueError, match="must be None, 0, 1"):
        model.transcribe_stream([AUDIO], dsp_mode=3)


# ---- once per file, before the VAD ----------------------------------------------------------------------------------------
def test_transcribe_enhances_once_and_before_the_vad(model):
    segs, _ = model.transcribe(AUDIO, language="zh", beam_size=1, temperature=0.0, dsp_mode=1, vad_filter=True, vad_speech_prob_fn=_vad_fn)
    assert [s.text for s in segs] != []
    assert _kinds()[:2] == ["enhance", "vad"] and _kinds().count("enhance") == 1
    assert DspEngine.log[0][2] == [len(AUDIO)] and DspEngine.log[0][3] == dsp.DspParams()
    assert all(e[1] for e in DspEngine.log if e[0] in ("vad", "mel")) and "mel" in _kinds()   # every consumer read the enhanced samples


def test_off_calls_exactly_what_it_calls_today(model):
    for kw in ({}, {"dsp_mode": None}, {"dsp_mode": 0}, {"dsp_mode": False}):
        DspEngine.log = []
        model.engine.calls = []
        segs, _ = model.transcribe(AUDIO, language="zh", beam_size=1, temperature=0.0, **kw)
        list(segs)
        assert "enhance" not in _kinds() and not any(e[1] for e in DspEngine.log if e[0] == "mel")
        calls = list(model.engine.calls)
        if kw:
            assert calls == first
        first = calls
    out = model.transcribe_many([AUDIO], language="zh", beam_size=1, temperature=0.0, dsp_mode=0)
    assert len(out) == 1 and "enhance" not in _kinds()


def test_transcribe_many_enhances_the_group_in_one_call_before_the_vad(model):
    model.vad_speech_prob_fn = _vad_fn
    files = [AUDIO, AUDIO[:16000 * 2]]
    out = model.transcribe_many(files, language="zh", beam_size=1, temperature=0.0, vad_filter=True, dsp_mode={"strength_db": 20})
    assert len(out) == 2
    assert _kinds()[:3] == ["enhance", "vad", "vad"] and _kinds().count("enhance") == 1
    assert DspEngine.log[0][2] == [len(a) for a in files] and DspEngine.log[0][3].strength_db == 20
    assert all(e[1] for e in DspEngine.log if e[0] in ("vad", "mel"))


def test_a_refused_dsp_mode_reaches_no_engine(model):
    for call in (lambda: model.transcribe(AUDIO, language="zh", dsp_mode=2),
                 lambda: model.transcribe_many([AUDIO], language="zh", dsp_mode={"max_gain": 0}),
                 lambda: model.transcribe_many([AUDIO], language="zh", continuous=True, dsp_mode="on"),
                 lambda: model.transcribe_groups([[AUDIO]], language="zh", dsp_mode={"nope": 1}),
                 lambda: model.transcribe_batched(AUDIO, dsp_mode=5),
                 lambda: model.transcribe_diarized(AUDIO, dsp_mode=5),
                 lambda: model.decode_audio_many([AUDIO], dsp_mode=5)):
        with pytest.raises(ValueError, match="dsp_mode"):
            call()
    assert DspEngine.log == [] and DspEngine.opened == [] and model.engine.calls == []


def test_bad_arguments_raise_before_the_enhancement_runs(model):
    """dsp_mode on, another argument wrong: the ValueError comes before any device work."""
    for call in (lambda: model.transcribe(AUDIO, language="zh", dsp_mode=1, beam_size=0),
                 lambda: model.transcribe(AUDIO, language="zh", dsp_mode=1, beam_size=9),
                 lambda: model.transcribe(AUDIO, language="zh", dsp_mode=1, language_detection_segments=0),
                 lambda: model.transcribe(AUDIO, language="zh", dsp_mode=1, clip_timestamps="-1"),
                 lambda: model.transcribe(np.zeros((2, 100), np.float32), language="zh", dsp_mode=1),
                 lambda: model.transcribe_many([AUDIO], language="zh", dsp_mode=1, clip_timestamps="-1"),
                 lambda: model.transcribe_many([AUDIO], language="zh", dsp_mode=1, session_prefill=4)):
        with pytest.raises(ValueError):
            call()
    assert DspEngine.log == [] and model.engine.calls == []


def test_folder_tool_enhances_once_per_file_when_it_also_diarizes(tmp_path):
    """dsp_mode with diarize: the loader enhances a file once (decode_audio_many(dsp_mode=...)) and neither the transcription nor
    the diarization is asked to enhance; one by one and in groups."""
    for name in ("a.wav", "b.wav", "c.wav"):
        (tmp_path / name).write_bytes(b"")
    log = []

    class Model:
        max_batch = 10
        has_diarization = True

        def decode_audio_many(self, audios, audio_channel=None, dsp_mode=None):
            log.append(("enhance", len(audios), dsp_mode))
            return [np.asarray(a) * np.float32(0.5) for a in audios]

        def transcribe(self, audio, **kw):
            log.append(("asr", _enhanced(audio), kw.get("dsp_mode", "absent")))
            return [], None

        def transcribe_many(self, audios, **kw):
            return [self.transcribe(a, **kw) for a in audios]

        def diarize(self, audio, **kw):
            log.append(("dia", _enhanced(audio), kw.get("dsp_mode", "absent")))
            return []
    quiet = lambda *a: None   # noqa: E731
    out = str(tmp_path / "results.json")
    for group_files in (1, 2):
        log.clear()
        batch_cli.process_audio_folder(str(tmp_path), model=Model(), load_audio=lambda f: AUDIO, log=quiet, output_json=out, dsp_mode=1,
                                       diarize=True, group_files=group_files)
        assert [e for e in log if e[0] == "enhance"] == [("enhance", 1, dsp.DspParams())] * 3      # once per file
        assert [e for e in log if e[0] == "asr"] == [("asr", True, "absent")] * 3
        assert [e for e in log if e[0] == "dia"] == [("dia", True, "absent")] * 3


def test_decode_audio_many_enhances_what_it_returns(model):
    out = model.decode_audio_many([AUDIO, AUDIO[:1000]], dsp_mode=1)
    assert _kinds() == ["enhance"] and DspEngine.log[0][2] == [len(AUDIO), 1000] and all(_enhanced(a) for a in out)
    DspEngine.log = []
    out = model.decode_audio_many([AUDIO])
    assert DspEngine.log == [] and out[0] is not None and not _enhanced(out[0])


def test_transcribe_diarized_enhances_once_for_both_passes(model, monkeypatch):
    seen = {}

    def diarize(audio, num_speakers=None, **kw):
        seen["dia"] = (_enhanced(audio), kw)
        return []

    def transcribe(audio, **kw):
        seen["asr"] = (_enhanced(audio), kw)
        return [], None
    monkeypatch.setattr(model, "diarize", diarize)
    monkeypatch.setattr(model, "transcribe", transcribe)
    model.transcribe_diarized(AUDIO, dsp_mode=1, language="zh")
    assert _kinds() == ["enhance"]
    assert seen["dia"] == (True, {}) and seen["asr"] == (True, {"language": "zh"})    # neither pass enhances again


def test_every_lane_enhances_its_own_groups(model):
    model.pipeline_depth = 2
    both, met = threading.Barrier(2), set()

    def script(n, seek, frames):
        me = threading.current_thread().name
        if me not in met:
            met.add(me)
            both.wait(timeout=30)
        return SCRIPT(n, seek, frames)
    for i in range(2):
        model._lane(i).script = script
    out = model.transcribe_groups([[AUDIO], [AUDIO], [AUDIO], [AUDIO]], pipeline_depth=2, language="zh", beam_size=1, temperature=0.0,
                                  dsp_mode=1)
    assert len(out) == 4
    calls = [e for e in DspEngine.log if e[0] == "enhance"]
    assert len(calls) == 4 and {e[1] for e in calls} == {id(lane) for lane in model._lanes}
    assert {e[4] for e in calls} == {"ttasr-lane0", "ttasr-lane1"}
    assert all(e[1] for e in DspEngine.log if e[0] == "mel")


def test_asr_adapter_passes_dsp_mode_to_transcribe_path():
    from taiwan_tongues_asr_ce_amd.asr import MI355XWhisperASR
    a = MI355XWhisperASR.__new__(MI355XWhisperASR)
    seen = {}

    class Pipe:
        def transcribe(self, path, **kw):
            seen.clear()
            seen.update(kw)
            return [], None
        transcribe_batched = transcribe
    a.asr_pipeline, a.default_transcribe_kwargs, a.device_resample, a.batched, a.audio_channel = Pipe(), {}, False, False, None
    a.bias_options, a.dsp_mode = {}, dsp.resolve(1)
    a.transcribe_path("x.wav")
    assert seen["dsp_mode"] == dsp.DspParams()
    a.transcribe_path("x.wav", dsp_mode=0)
    assert seen["dsp_mode"] == 0
    a.batched = True
    a.transcribe_path("x.wav")
    assert seen["dsp_mode"] == dsp.DspParams()
    a.dsp_mode = None
    a.transcribe_path("x.wav")
    assert "dsp_mode" not in seen
