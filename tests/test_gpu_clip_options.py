"""GPU: clip_timestamps and hallucination_silence_threshold of WhisperModel.transcribe / lock-step transcribe_many on the HIP
engine (synthetic tiny model), against the window table of tests/test_clip_timestamps_host.py, against the same loop driven by
the CPU oracle (tests/oracle_engine.py with the cut of tests/cut_oracle.py) in f32, and against the run without the options."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import alignment, synth
from taiwan_tongues_asr_ce_amd import model as model_module
from test_longform_golden import recording

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

W = 3000
CLIPS = "5,41.5,52,60"                       # 36.5 s: more than one window, the second one cut by the clip; then 8 s
CLIP_FRAMES = [(500, 4150), (5200, 6000)]
# no thresholds: a random-weight model's windows would otherwise all count as silence or climb the temperature ladder
KW = dict(language="zh", beam_size=1, temperature=0.0, max_new_tokens=24, no_speech_threshold=None, log_prob_threshold=None,
          compression_ratio_threshold=None)


@pytest.fixture(scope="module", params=["float32", "bfloat16"])
def model(request):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type=request.param, max_batch=4)
    yield m
    m.close()


@pytest.fixture(scope="module")
def audio():
    return recording()                       # 70 s


@contextlib.contextmanager
def spied(m):
    """Records (seek, cut or None) of every window feature call and (seek, prompt) of every greedy search of the model's engine."""
    eng = m.engine
    log = dict(windows=[], prompts=[])
    feat, gen = eng.log_mel_windows, eng.generate

    def log_mel_windows(audio, seeks, floor_max=None, want_output=False, want_max=False, **kw):
        if not want_max:
            cut = kw.get("n_frames")
            log["windows"].extend((int(k), None if cut is None else int(cut[b])) for b, k in enumerate(seeks))
            log["seek"] = int(seeks[0])
        return feat(audio, seeks, floor_max=floor_max, want_output=want_output, want_max=want_max, **kw)

    def generate(prompts, opts, *a, **k):
        log["prompts"].append((log["seek"], list(prompts[0])))
        return gen(prompts, opts, *a, **k)
    eng.log_mel_windows, eng.generate = log_mel_windows, generate
    try:
        yield log
    finally:
        del eng.log_mel_windows, eng.generate


def _run(m, audio, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        segs, info = m.transcribe(audio, **dict(KW, **kw))
        return list(segs), info


def _clip_of(seek):
    return next((s, e) for s, e in CLIP_FRAMES if s <= seek < e)


def test_clips_bound_the_windows_and_the_segments(model, audio):
    with spied(model) as log:
        segs, info = _run(model, audio, clip_timestamps=CLIPS)
    assert info.duration == 70.0 and segs
    n_total = len(audio) // 160
    seeks = [k for k, _ in log["windows"]]
    assert seeks[0] == 500 and 5200 in seeks and seeks == sorted(seeks) and len(seeks) >= 3
    for k, cut in log["windows"]:
        s, e = _clip_of(k)                                         # every window starts inside a clip ...
        frames = min(W, n_total - k, e - k)                        # ... and holds the frames of the host table's rule
        assert cut == (frames if frames < min(W, n_total - k) else None), (k, cut)
    assert any(cut is not None for _, cut in log["windows"])
    for seg in segs:
        s, e = _clip_of(seg.seek)
        assert s / 100 <= seg.start < seg.end <= e / 100, (seg.seek, seg.start, seg.end)
    assert {seg.seek for seg in segs} <= set(seeks) and [seg.id for seg in segs] == list(range(len(segs)))


def test_clip_loop_equals_the_oracle_driven_loop(audio):
    """f32: the HIP engine and the CPU oracle, each under the same host loop with the same clips: tokens, seeks, times."""
    from cut_oracle import CutOracle
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    ref = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=1, _engine_factory=CutOracle)
    gpu = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=2)
    try:
        want, _ = _run(ref, audio, clip_timestamps=CLIPS)
        got, _ = _run(gpu, audio, clip_timestamps=CLIPS)
    finally:
        gpu.close()
    assert want and len({s.seek for s in want}) >= 3
    assert [s.tokens for s in got] == [s.tokens for s in want]
    assert [(s.id, s.seek, s.start, s.end) for s in got] == [(s.id, s.seek, s.start, s.end) for s in want]


@pytest.mark.parametrize("default", ["0", [0], [0, 70.0]])
def test_default_clip_forms_are_the_run_without_the_option(model, audio, default):
    with spied(model) as plain:
        want, want_info = _run(model, audio)
    with spied(model) as log:
        got, info = _run(model, audio, clip_timestamps=default)
    assert got == want and want and info == want_info              # Segment tuples: tokens, times and the float statistics
    assert log == plain and all(cut is None for _, cut in log["windows"])


def test_threshold_none_with_words_is_the_run_without_the_option(model, audio):
    short = audio[: 40 * 16000]
    want, _ = _run(model, short, word_timestamps=True)
    got, _ = _run(model, short, word_timestamps=True, hallucination_silence_threshold=None)
    assert got == want and want and all(s.words is not None for s in want)


def test_threshold_run_completes_and_drops_leave_no_trace(model, audio, monkeypatch):
    short = audio[: 40 * 16000]
    dealt = {}                                                     # window offset -> the words the aligner dealt to its segments
    deal = alignment.add_word_timestamps

    def add_word_timestamps(segments, found, time_offset):
        deal(segments, found, time_offset)
        dealt[round(time_offset * 100)] = [(list(s["tokens"]), list(s["words"])) for s in segments]
    monkeypatch.setattr(alignment, "add_word_timestamps", add_word_timestamps)
    acted = []                                                     # per window with words: what the rules did to it
    rules = model_module.skip_hallucinations

    def skip_hallucinations(kept, single_end, seek, win_frames, next_seek, *a, **k):
        out, seek_out, nothing = rules(kept, single_end, seek, win_frames, next_seek, *a, **k)
        acted.append(dict(seek=seek, dropped=len(kept) - len(out), moved=seek_out - next_seek, nothing=nothing))
        return out, seek_out, nothing
    monkeypatch.setattr(model_module, "skip_hallucinations", skip_hallucinations)
    with spied(model) as plain:
        _run(model, short, word_timestamps=True)
    acted.clear()
    with spied(model) as log:
        segs, info = _run(model, short, word_timestamps=True, hallucination_silence_threshold=2.0)
    # the checks below would be empty if the rules never acted.  They must act here: a random-weight model gives its own tokens
    # probabilities far below 0.15, so every segment with words is anomalous.  In the first window (time 0, nothing kept before
    # it) the first such segment starts either more than 2 s in - rule 2 yields nothing - or less, which counts as silence
    # before it; silence after it holds too: a next segment is anomalous as well, and without one either more than 2 s of the
    # window's audio follow its end or fewer than 2 s of the window do
    assert any(a["dropped"] or a["nothing"] for a in acted), acted
    assert log["windows"] != plain["windows"]
    seeks = [k for k, _ in log["windows"]]
    assert seeks and seeks == sorted(set(seeks)) and seeks[-1] < 4000          # every window moves on; the run ends
    assert [s.id for s in segs] == list(range(len(segs)))
    for s in segs:                                                 # a yielded segment carries exactly the aligner's words
        assert (s.tokens, s.words) in dealt[s.seek], s.seek
    # a later window's previous text is the tokens of the segments that were YIELDED before it, nothing else
    st = model.special
    for k, prompt in log["prompts"]:
        told = [t for s in segs if s.seek < k for t in s.tokens if t != st.eot]
        prev = prompt[1:prompt.index(st.sot)] if prompt[0] == st.sot_prev else []
        assert prev == told[len(told) - len(prev):] and len(prev) == min(len(told), model.dims.n_text_ctx // 2 - 1), k
    assert dealt and len(acted) == len(dealt)


def test_lock_step_with_clips_and_threshold_equals_transcribe(audio):
    """f32, as test_transcribe_many_equals_file_by_file: per-file clip lists and a threshold, file by file and in lock step."""
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=4)
    files = [audio[: 50 * 16000], np.concatenate([synth.tonal_clip(3), synth.noise_clip(4)[: 12 * 16000]])]     # 50 s, 42 s
    clips = ["4,36.5,41", [2.5, 20]]
    kw = dict(language="zh", beam_size=1, temperature=0.0, log_prob_threshold=None, max_new_tokens=16, word_timestamps=True,
              hallucination_silence_threshold=1.0)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            many = m.transcribe_many(files, clip_timestamps=clips, **kw)
            for f, c, (segs, info) in zip(files, clips, many):
                ref, ref_info = m.transcribe(f, clip_timestamps=c, **kw)
                ref = list(ref)
                assert info.duration == ref_info.duration
                assert [s.tokens for s in segs] == [s.tokens for s in ref]
                assert [(s.id, s.seek, s.start, s.end) for s in segs] == [(s.id, s.seek, s.start, s.end) for s in ref]
                assert [[(w.word, w.start, w.end) for w in s.words] for s in segs] == \
                       [[(w.word, w.start, w.end) for w in s.words] for s in ref]
        assert any(segs for segs, _ in many)
    finally:
        m.close()
