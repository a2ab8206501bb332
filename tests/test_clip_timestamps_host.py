"""CPU: clip_timestamps in WhisperModel's window loop, on a scripted engine double that records its calls (window_loop_stub).

The option restates openai-whisper's transcribe() from memory (unpinned); these tables pin the restatement.  All expected values
are worked out by hand: the model's window is 3000 frames (30 s), a seek point is round(seconds * 100) frames."""
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd.model import parse_clip_timestamps, refuse_in_session
from window_loop_stub import NoCutEngine, ScriptEngine, W, by_seek, make_model, run, ts

SR = 16000
AUDIO_100S = np.zeros(100 * SR, np.float32)      # 10 000 frames


# ---------------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("given, n_total, want", [
    ("0", 10000, [(0, 10000)]),                              # the default: one clip, the whole recording
    ("", 10000, [(0, 10000)]),
    ([], 10000, [(0, 10000)]),
    ([0], 10000, [(0, 10000)]),
    ([0, 100.0], 10000, [(0, 10000)]),
    ("10,45", 10000, [(1000, 4500)]),                        # a string of seconds
    (" 10 , 45.5 ,60,70 ", 10000, [(1000, 4550), (6000, 7000)]),
    ([10, 45, 60.004, 70.006], 10000, [(1000, 4500), (6000, 7001)]),   # a list; round(t * 100)
    ((1.5, 2.25), 10000, [(150, 225)]),
    (np.asarray([1.5, 2.25]), 10000, [(150, 225)]),
    ("90", 10000, [(9000, 10000)]),                          # an odd count: the last clip runs to the end
    ([10, 20, 30], 10000, [(1000, 2000), (3000, 10000)]),
    ("80,150", 10000, [(8000, 10000)]),                      # an end past the recording is clamped
    ("120,150", 10000, [(10000, 10000)]),                    # so is a start: the clip is empty
    ("20,20", 10000, [(2000, 2000)]),
    ("50,40", 10000, [(5000, 4000)]),                        # ends before it starts: walked as an empty clip
    ("0", 0, [(0, 0)]),
])
def test_parse_clip_timestamps(given, n_total, want):
    assert parse_clip_timestamps(given, n_total) == want


@pytest.mark.parametrize("bad", ["-1", [3, -0.5], "1,x", [float("nan")], [float("inf"), 2], "1,,2", None, 5.0, [None], [[1, 2]]])
def test_parse_clip_timestamps_refuses(bad):
    with pytest.raises(ValueError, match="clip_timestamps"):
        parse_clip_timestamps(bad, 10000)


# ----------------------------------------------------------------------------------- the (seek, frames) the loop requests
# every window silent: the loop advances by the frames it decoded
CLIP_TABLE = [
    ("10,45", [(1000, 3000), (4000, 500)]),                                  # one clip inside the file
    ("10,45,60,70", [(1000, 3000), (4000, 500), (6000, 1000)]),              # two clips
    ("5,12.5", [(500, 750)]),                                                # a clip shorter than a window
    ("0,70", [(0, 3000), (3000, 3000), (6000, 1000)]),                       # longer than two windows
    ("80,150", [(8000, 2000)]),                                              # ends past the file
    ("20,20,30,31", [(3000, 100)]),                                          # an empty clip is stepped over
    ("50,40,30,31", [(3000, 100)]),
    ("120,150", []),                                                         # starts past the file
    ("0,10,10,20", [(0, 1000), (1000, 1000)]),                               # back to back
    ("90", [(9000, 1000)]),                                                  # odd count
    ([95.5], [(9550, 450)]),
]


@pytest.mark.parametrize("clips, want", CLIP_TABLE)
def test_windows_requested_for_clips(clips, want):
    m = make_model()
    segs, info = run(m, AUDIO_100S, clip_timestamps=clips)
    assert segs == [] and info.duration == 100.0
    assert m.engine.windows() == want and [k for k, _ in m.engine.prompts()] == [seek for seek, _ in want]
    # the cut goes to the feature call only where the clip ends the window before the model's window or the recording would
    assert m.engine.asked() == [(seek, frames if frames < min(W, 10000 - seek) else None) for seek, frames in want]
    # the dynamic-range floor stays the WHOLE recording's: the maxima pass covers every window of the file, before the first window
    calls = [c for c in m.engine.calls if c[0] in ("max", "win")]
    assert calls[0] == ("max", [0, 3000, 6000, 9000]) and all(c[0] == "win" for c in calls[1:])


def test_windows_follow_the_segments_inside_a_clip():
    """A window that ends in a closed pair advances to its last timestamp; the next window is cut where the clip ends."""
    script = by_seek({1000: dict(tokens=[ts(0.0), 97, ts(20.0), ts(20.0)]),          # advance 2000 -> seek 3000, 1500 left in the clip
                      3000: dict(tokens=[ts(0.0), 98, ts(40.0)])})                   # single ending timestamp: the whole window
    m = make_model(script)
    segs, _ = run(m, AUDIO_100S, clip_timestamps="10,45")
    assert m.engine.windows() == [(1000, 3000), (3000, 1500)]
    assert [c[1] for c in m.engine.calls if c[0] == "win"] == [[(1000, None)], [(3000, 1500)]]
    # times never pass the clip's end (45 s), and only segments inside the clip come out
    assert [(s.seek, s.start, s.end) for s in segs] == [(1000, 10.0, 30.0), (3000, 30.0, 45.0)]
    # previous-text conditioning carries across windows of a clip ...
    assert m.engine.prompts()[1][1][0] == m.special.sot_prev and 97 in m.engine.prompts()[1][1]


def test_previous_text_carries_across_clips():
    script = by_seek({1000: dict(tokens=[ts(0.0), 97, ts(4.0)]), 6000: dict(tokens=[ts(0.0), 98, ts(4.0)])})
    m = make_model(script)
    segs, _ = run(m, AUDIO_100S, clip_timestamps="10,15,60,65")
    assert [(s.id, s.seek, s.start, s.end) for s in segs] == [(0, 1000, 10.0, 14.0), (1, 6000, 60.0, 64.0)]
    (_, first), (_, second) = m.engine.prompts()
    assert first[0] == m.special.sot and second[0] == m.special.sot_prev and 97 in second


@pytest.mark.parametrize("default", ["0", [0], [0, 100.0], "", (0,)])
def test_default_forms_request_exactly_todays_sequence(default):
    """On an engine whose feature call has no n_frames keyword at all (the call as it was): same calls, same order."""
    script = by_seek({0: dict(tokens=[ts(0.0), 97, ts(12.0), ts(12.0)]), 1200: dict(tokens=[ts(0.0), 98, ts(30.0)])})
    plain = make_model(script, cls=NoCutEngine)
    want_segs, want_info = run(plain, AUDIO_100S)
    assert plain.engine.windows() == [(0, 3000), (1200, 3000), (4200, 3000), (7200, 2800)]
    m = make_model(script, cls=NoCutEngine)
    segs, info = run(m, AUDIO_100S, clip_timestamps=default)
    assert m.engine.calls == plain.engine.calls and segs == want_segs and info == want_info


def test_detection_windows_start_at_the_first_clip():
    m = make_model()
    seen = []

    def spy(windows):
        seen.extend(windows)
        return [("zh", 0.4, [("zh", 0.4)])] * len(windows)
    m.detect_language_batch = spy
    audio = np.arange(100 * SR, dtype=np.float32)      # a ramp: every sample names its own position
    _, info = run(m, audio, language=None, language_detection_segments=2, clip_timestamps="10,80")
    assert [float(w[0]) for w in seen] == [10.0 * SR, 40.0 * SR] and info.language == "zh"
    seen.clear()
    run(m, audio, language=None, language_detection_segments=2)
    assert [float(w[0]) for w in seen] == [0.0, 30.0 * SR]
    seen.clear()
    run(m, audio, language=None, language_detection_segments=3, clip_timestamps="80")   # no third window inside the recording
    assert [float(w[0]) for w in seen] == [80.0 * SR]


def test_vad_with_clips_warns_and_skips_the_vad():
    m = make_model()
    called = []

    def prob_fn(a):
        called.append(len(a))
        return np.ones(len(a) // 512, np.float32)
    m.vad_speech_prob_fn = prob_fn
    with pytest.warns(UserWarning, match="vad_filter=True is skipped"):
        _, info = run(m, AUDIO_100S, vad_filter=True, clip_timestamps="10,45")
    assert not called and m.engine.windows() == [(1000, 3000), (4000, 500)] and info.duration_after_vad == 100.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        run(m, AUDIO_100S, vad_filter=True, clip_timestamps="0")          # the default still filters
    assert called == [len(AUDIO_100S)]


# ----------------------------------------------------------------------------------------------------- many files
def _two_file_script(n, seek, frames):
    a, b = 100 * SR, 47 * SR
    table = {(a, 1000): dict(tokens=[ts(0.0), 97, ts(20.0), ts(20.0)]), (a, 3000): dict(tokens=[ts(0.0), 98, ts(10.0)]),
             (b, 500): dict(tokens=[ts(0.0), 99, ts(2.0), ts(2.0), 100, ts(3.0)]), (b, 4000): dict(tokens=[ts(1.0), 101, ts(5.0)])}
    return table.get((n, seek))


def test_transcribe_many_with_per_file_clips_equals_transcribe():
    files = [AUDIO_100S, np.zeros(47 * SR, np.float32)]
    clips = ["10,45", [5, 12.5, 40]]
    alone = []
    for f, c in zip(files, clips):
        m = make_model(_two_file_script)
        segs, _ = run(m, f, clip_timestamps=c)
        alone.append((segs, m.engine.windows()))
    assert alone[0][1] == [(1000, 3000), (3000, 1500)] and alone[1][1] == [(500, 750), (4000, 700)]
    m = make_model(_two_file_script)
    got = m.transcribe_many(files, language="zh", beam_size=1, temperature=0.0, clip_timestamps=clips)
    for (segs, info), (want, _) in zip(got, alone):
        assert segs == want and segs
    # lock step: round 1 holds both files' first windows in one call, each with its own cut
    assert [c[1] for c in m.engine.calls if c[0] == "win"] == [[(1000, 3000), (500, 750)], [(3000, 1500), (4000, 700)]]
    # one value for every file
    m = make_model(_two_file_script)
    got = m.transcribe_many(files, language="zh", beam_size=1, temperature=0.0, clip_timestamps="10,45")
    assert [c[1] for c in m.engine.calls if c[0] == "win"][0] == [(1000, None), (1000, None)]   # neither window is cut
    with pytest.raises(ValueError, match="one entry per file"):
        m.transcribe_many(files, language="zh", clip_timestamps=["1,2", "3,4", "5,6"])
    # transcribe_groups passes the option through
    m = make_model(_two_file_script)
    grouped = m.transcribe_groups([[files[0]], [files[0]]], language="zh", beam_size=1, temperature=0.0, clip_timestamps="10,45")
    assert [g[0][0] for g in grouped] == [alone[0][0], alone[0][0]]


# -------------------------------------------------------------------------------------------- continuous surfaces
@pytest.mark.parametrize("kw", [dict(clip_timestamps="10,45"), dict(clip_timestamps=[5]), dict(hallucination_silence_threshold=2.0),
                                dict(clip_timestamps=[0, 100.0])])
def test_continuous_surfaces_refuse_the_window_loop_options(kw, tmp_path):
    from taiwan_tongues_asr_ce_amd import batch_cli
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    opened = []

    class E(ScriptEngine):
        session_hold = True

        def session(self, *a, **k):
            opened.append(a)
            raise AssertionError("a session was opened")
    m = make_model(cls=E)
    with pytest.raises(ValueError, match="lock-step form"):
        m.transcribe_many([AUDIO_100S], language="zh", continuous=True, **kw)
    with pytest.raises(ValueError, match="lock-step form"):
        m.transcribe_stream([AUDIO_100S[: 3 * SR]], language="zh", **kw)
    with pytest.raises(ValueError, match="lock-step form"):
        BatchedWhisperASR(continuous=True, model_size="does-not-exist", **kw)      # before any model is built
    with pytest.raises(ValueError, match="single-window"):
        BatchedWhisperASR(model_size="does-not-exist", **kw)
    (tmp_path / "a.wav").write_bytes(b"")
    cli = {k: (",".join(str(v) for v in x) if isinstance(x, list) else x) for k, x in kw.items()}
    with pytest.raises(ValueError, match="lock-step form"):
        batch_cli.process_audio_folder(str(tmp_path), model=m, continuous=True, log=lambda s: None, **cli)
    argv = [str(tmp_path), "--continuous"]
    for k, v in cli.items():
        argv += ["--" + k.replace("_", "-"), str(v)]
    assert batch_cli.main(argv) == 1
    assert not opened and not m.engine.calls


def test_neutral_values_pass_every_continuous_check():
    for clips in ("0", "", [0], [], None):
        refuse_in_session("x", clips, None)


def test_batch_cli_passes_the_options_to_both_folder_paths(tmp_path):
    """One by one (transcribe) and grouped (lock-step transcribe_many): the clips as given, the threshold with word timestamps."""
    from taiwan_tongues_asr_ce_amd import batch_cli
    for name in ("a.wav", "b.wav"):
        (tmp_path / name).write_bytes(b"")
    seen = []

    class Model:
        max_batch = 10

        def transcribe(self, audio, **kw):
            seen.append(("one", kw))
            return iter(()), None

        def transcribe_many(self, audios, **kw):
            seen.append(("many", kw))
            return [([], None) for _ in audios]
    args = batch_cli.build_parser().parse_args([str(tmp_path), "--clip-timestamps", "1,2.5", "--hallucination-silence-threshold", "1.5"])
    assert args.clip_timestamps == "1,2.5" and args.hallucination_silence_threshold == 1.5
    for group_files, want in ((1, ["one", "one"]), (2, ["many"])):
        seen.clear()
        batch_cli.process_audio_folder(str(tmp_path), model=Model(), group_files=group_files, log=lambda s: None,
                                       load_audio=lambda f: np.zeros(SR, np.float32), output_json=str(tmp_path / "out.json"),
                                       clip_timestamps=args.clip_timestamps,
                                       hallucination_silence_threshold=args.hallucination_silence_threshold)
        assert [k for k, _ in seen] == want
        for _, kw in seen:
            assert kw["clip_timestamps"] == "1,2.5" and kw["hallucination_silence_threshold"] == 1.5 and kw["word_timestamps"] is True
    seen.clear()
    batch_cli.process_audio_folder(str(tmp_path), model=Model(), group_files=1, log=lambda s: None,
                                   load_audio=lambda f: np.zeros(SR, np.float32), output_json=str(tmp_path / "out.json"))
    assert all("clip_timestamps" not in kw and "hallucination_silence_threshold" not in kw for _, kw in seen) and seen
    with pytest.raises(ValueError, match="batched"):
        batch_cli.process_audio_folder(str(tmp_path), model=Model(), batched=True, clip_timestamps="1,2", log=lambda s: None)
    # with a VAD network the grouped path keeps vad_filter=True beside the clips: transcribe_many decides per file, and warns
    seen.clear()
    vad_model = Model()
    vad_model.has_device_vad = True
    batch_cli.process_audio_folder(str(tmp_path), model=vad_model, group_files=2, log=lambda s: None,
                                   load_audio=lambda f: np.zeros(SR, np.float32), output_json=str(tmp_path / "out.json"),
                                   clip_timestamps="1,2.5")
    assert [(k, kw["vad_filter"], kw["clip_timestamps"]) for k, kw in seen] == [("many", True, "1,2.5")]


# ------------------------------------------------------------------------------------------- the window-cut reference
def _cut_window(features, seek, n, window):
    """pad_or_trim(features[:, seek:seek + n]) to one window: the feature slice of the clip, zeros in feature space behind it."""
    piece = features[:, seek:seek + n][:, :window]
    out = np.zeros((features.shape[0], window), np.float32)
    out[:, :piece.shape[1]] = piece
    return out


def test_window_cut_reference():
    """What a window that ends with its clip must hold, from the oracle's whole-file features (R.log_mel_file): a recording with
    a tail that is no whole window; seeks at the start, mid-file and near the end; cuts of 1 and F - 1 frames, F being the
    frames the uncut window holds.  The cut window differs from the uncut one for every n < F, equals it for n >= F, and the
    oracle engine double the GPU loop test runs beside the HIP engine (cut_oracle.CutOracle) returns exactly it."""
    from cut_oracle import CutOracle
    from oracle import whisper_ref as R
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import PRESETS
    dims = PRESETS["tiny"]
    n_total = W + 1500 + 1213
    audio = synth.noise_clip(7, n_total * 160 + 77)
    f = R.log_mel_file(audio, dims.n_mels)
    assert f.shape == (dims.n_mels, n_total)
    eng = CutOracle(dims)
    for k in (0, W // 2 + 3, n_total - W // 3):
        F = min(W, n_total - k)
        uncut = R.file_window(f, k, W)
        assert np.array_equal(_cut_window(f, k, F, W), uncut) and np.array_equal(_cut_window(f, k, F + 5, W), uncut)
        plain, _ = eng.log_mel_windows(audio, [k], want_output=True)
        assert np.array_equal(plain[0], uncut)
        for n in (1, F - 1):
            want = _cut_window(f, k, n, W)
            assert np.array_equal(want, R.file_window(f[:, k:k + n], 0, W))
            assert np.array_equal(want[:, :n], uncut[:, :n]) and not want[:, n:].any()
            assert not np.array_equal(want, uncut) and uncut[:, n:F].any()          # the cut really removes frames of the recording
            got, mx = eng.log_mel_windows(audio, [k], want_output=True, want_max=True, n_frames=[n])
            assert np.array_equal(got[0], want)
    # rows of one call are cut independently
    seeks, cuts = [0, W // 2 + 3, n_total - W // 3], [2, W - 1, 7]
    got, _ = eng.log_mel_windows(audio, seeks, want_output=True, n_frames=cuts)
    for b, (k, n) in enumerate(zip(seeks, cuts)):
        assert np.array_equal(got[b], _cut_window(f, k, n, W))
