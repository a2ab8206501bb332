"""CPU: hallucination_silence_threshold, prompt_reset_on_temperature and suppress_tokens of WhisperModel.transcribe.

The anomaly score and the skipping rules restate openai-whisper's transcribe() from memory (unpinned); the tables below pin the
restatement around every constant, and a scripted engine double (window_loop_stub: tokens and word lists per window) drives
each rule of the loop once.  Expected values are worked out by hand in the comments."""
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd.alignment import Word, is_segment_anomaly, word_anomaly_score
from taiwan_tongues_asr_ce_amd.engine import default_suppress
from window_loop_stub import ST, by_seek, make_model, patch_alignment, run, ts, word

SR = 16000
AUDIO_100S = np.zeros(100 * SR, np.float32)
THR = 2.0


def _w(duration=0.5, probability=0.9, text=" a", start=1.0):
    return Word(start=start, end=start + duration, word=text, probability=probability)


# ------------------------------------------------------------------------------------------------------ the score
@pytest.mark.parametrize("duration, probability, want", [
    (0.5, 0.9, 0.0),
    (0.5, 0.15, 0.0), (0.5, 0.1499, 1.0),                         # probability: below 0.15 only
    (0.133, 0.9, 0.0), (0.1, 0.9, 15 * 0.033), (0.0, 0.9, 15 * 0.133),   # duration below 0.133 s: 15 per second short
    (2.0, 0.9, 0.0), (3.5, 0.9, 1.5),                             # beyond 2 s: the excess
    (0.05, 0.1, 1.0 + 15 * 0.083),                                # both
])
def test_word_anomaly_score(duration, probability, want):
    assert word_anomaly_score(_w(duration, probability, start=0.0)) == pytest.approx(want, abs=1e-9)
    assert word_anomaly_score(dict(word=" a", start=0.0, end=duration, probability=probability)) == pytest.approx(want, abs=1e-9)


LOW, OK, SHORT = dict(probability=0.1), dict(), dict(duration=0.05, probability=0.1)   # scores 1.0, 0.0, 2.245


@pytest.mark.parametrize("words, want", [
    ([], False), (None, False),                                   # no words
    ([OK], False),                                                # 0 + 0.01 < 1
    ([LOW], True),                                                # 1 + 0.01 >= 1
    ([LOW, OK], False),                                           # 1.01 < 2
    ([LOW, dict(duration=0.066)], True),                          # 1 + 1.005 + 0.01 >= 2
    ([LOW, dict(duration=0.068)], False),                         # 1 + 0.975 + 0.01 < 2
    ([LOW, LOW, OK, OK, OK, OK, OK, OK], False),                  # 2 < 3 and 2.01 < 8
    ([LOW, LOW, LOW, OK, OK, OK, OK, OK], True),                  # 3 >= 3
    ([dict(duration=4.99), OK, OK, OK, OK, OK], False),           # 2.99 < 3, 3.0 < 6
    ([dict(duration=5.0), OK, OK, OK, OK, OK], True),             # 3.0 >= 3
    ([SHORT, SHORT], True),                                       # 4.49
    ([OK] * 8 + [LOW] * 5, False),                                # only the first 8 words count
    ([LOW] * 3 + [OK] * 10, True),
    ([LOW, LOW] + [OK] * 6 + [LOW], False),                       # the ninth word would have made 3
    ([dict(text=","), LOW], True),                                # punctuation is not counted: one word, score 1
    ([dict(text="。", probability=0.1)] * 3 + [OK] * 4, False),   # nor scored
    ([dict(text="。", probability=0.1)] * 3 + [OK] * 8 + [LOW] * 3, False),   # and does not use up the 8
])
def test_is_segment_anomaly(words, want):
    seg = None if words is None else dict(words=[_w(**w) for w in words])
    assert is_segment_anomaly(seg) is want
    if words == []:
        assert is_segment_anomaly(dict(words=None)) is False


# ------------------------------------------------------------------------------------------------------- the loop
A, B, C, D, E, X, Y = 97, 98, 99, 100, 101, 120, 121     # byte tokens: the stub tokenizer renders them as letters
ODD = dict(probability=0.1)                              # with a 0.05-s duration: score 2.245, an anomalous one-word segment

# window at seek 0: two ordinary segments, closed by a timestamp pair at 10 s; the last word ends at 9.0 s
RESEEK = {0: dict(tokens=[ts(0), A, B, ts(4), ts(4), C, D, ts(10), ts(10)],
                  words=[word(" a", 0.2, 0.7), word(" b", 0.7, 1.2), word(" c", 4.5, 5.0), word(" d", 8.5, 9.0)])}
# the last word ends 1.5 s before the window does
FULL = {0: dict(tokens=[ts(0), A, B, ts(29), ts(29)], words=[word(" a", 0.2, 0.7), word(" b", 28.0, 28.5)])}
# a single ending timestamp: rule 1 does not apply
SINGLE = {0: dict(tokens=[ts(0), A, ts(5)], words=[word(" a", 0.2, 0.7)])}
# 5 s of silence, then an invented word; looked at again from 5 s, where it is surrounded by silence
LEADING = {0: dict(tokens=[ts(5), X, ts(6), ts(6)], words=[word(" x", 5.0, 5.05, **ODD)]),
           500: dict(tokens=[ts(0), X, ts(1), ts(1)], words=[word(" x", 0.0, 0.05, **ODD)])}
# speech, 8.8 s of silence, an invented word, 10 s of silence, speech
DROP = {0: dict(tokens=[ts(0), A, B, ts(3), ts(10), X, ts(11), ts(20), C, D, ts(22), ts(22)],
                words=[word(" a", 0.2, 0.7), word(" b", 0.7, 1.2), word(" x", 10.0, 10.05, **ODD), word(" c", 20.2, 20.7), word(" d", 21.0, 21.5)]),
        1000: dict(tokens=[ts(0), E, ts(2)], words=[word(" e", 0.5, 1.0)])}
# the invented word comes half a second after speech, 10 s into the window: no silence before it
KEPT = {0: dict(tokens=[ts(8), A, B, ts(9.6), ts(10), X, ts(11), ts(11)],
                words=[word(" a", 8.2, 8.7), word(" b", 9.0, 9.5), word(" x", 10.0, 10.05, **ODD)])}


def _seeks(m):
    return [k for k, _ in m.engine.windows()]


def _run(table, monkeypatch, audio=AUDIO_100S, **kw):
    patch_alignment(monkeypatch)
    m = make_model(by_seek(table))
    segs, _ = run(m, audio, word_timestamps=True, **kw)
    return m, segs


@pytest.mark.parametrize("table, with_threshold, without", [
    # rule 1: 30 - 9.0 > 2 -> go on at the last word's end; today: at the closing pair, 10 s
    (RESEEK, [0, 900, 3900, 6900, 9900], [0, 1000, 4000, 7000]),
    # rule 1: 30 - 28.5 <= 2 -> behind the window; today: at the closing pair, 29 s
    (FULL, [0, 3000, 6000, 9000], [0, 2900, 5900, 8900]),
    (SINGLE, [0, 3000, 6000, 9000], [0, 3000, 6000, 9000]),
])
def test_reseek_to_the_last_word_or_full_advance(table, with_threshold, without, monkeypatch):
    m, segs = _run(table, monkeypatch, hallucination_silence_threshold=THR)
    assert _seeks(m) == with_threshold
    m0, segs0 = _run(table, monkeypatch)
    assert _seeks(m0) == without                 # without a threshold the project does not re-seek to the last word
    assert segs == segs0 and segs                # nothing is anomalous: the same segments either way
    m1, segs1 = _run(table, monkeypatch, hallucination_silence_threshold=None)
    assert m1.engine.calls == m0.engine.calls and segs1 == segs0


def test_leading_silence_before_an_invented_word_is_skipped(monkeypatch):
    """Window 0: the first segment with words is anomalous and starts 5 s in (> 2): nothing is yielded, seek = 0 + 500.
    Window 500: the same word at the window's start; silence before (5.0 - 0 > 2) and after (no next segment: 35 - 5.05 > 2):
    dropped, seek = max(5 + 1, 5.0) s = 600."""
    m, segs = _run(LEADING, monkeypatch, hallucination_silence_threshold=THR)
    assert segs == [] and _seeks(m) == [0, 500, 600, 3600, 6600, 9600]
    assert all(p[0] == ST.sot for _, p in m.engine.prompts())      # no dropped text reached a prompt
    m0, segs0 = _run(LEADING, monkeypatch)
    assert [(s.seek, s.start, s.end) for s in segs0] == [(0, 5.0, 5.05)] and _seeks(m0) == [0, 600, 3600, 6600, 9600]


def test_an_invented_word_between_silences_is_dropped_with_what_follows(monkeypatch):
    """S1 0.2-1.2 s, S2 10.0-10.05 s (anomalous), S3 20.2-21.5 s.  Before S2: 10.0 - 1.2 > 2; after: 20.2 - 10.05 > 2: S2 and S3
    go, seek = max(0 + 1, 10.0) s = 1000 (rule 1 alone would have said 2150).  The next window's prompt and ids see S1 only."""
    m, segs = _run(DROP, monkeypatch, hallucination_silence_threshold=THR)
    assert [(s.id, s.seek, s.start, s.end, s.text) for s in segs] == [(0, 0, 0.2, 1.2, "ab"), (1, 1000, 10.5, 11.0, "e")]
    assert _seeks(m) == [0, 1000, 4000, 7000]
    prompt = m.engine.prompts()[1][1]
    assert prompt[:5] == [ST.sot_prev, ts(0), A, B, ts(3)] and prompt[5] == ST.sot
    assert not {X, C, D} & set(prompt)
    # every yielded segment's words are the aligner's
    assert [(w.word, w.start, w.end) for w in segs[0].words] == [(" a", 0.2, 0.7), (" b", 0.7, 1.2)]
    m0, segs0 = _run(DROP, monkeypatch)
    assert [s.text for s in segs0] == ["ab", "x", "cd"] and _seeks(m0) == [0, 2200, 5200, 8200]
    assert {X, C, D} <= set(m0.engine.prompts()[1][1])


def test_a_drop_near_the_end_of_the_recording_ends_it(monkeypatch):
    """A 40-s recording; the window at 30 s holds speech (30.2-31.2), then two invented words (38.5-38.55, 39.2-39.25).  The first is
    preceded by silence (38.5 - 31.2 > 2) and followed by another anomaly: dropped; 40 - 38.55 < 2 s of audio follow: seek = the end."""
    table = {3000: dict(tokens=[ts(0), A, B, ts(3), ts(8.5), X, ts(9), ts(9.2), Y, ts(9.6), ts(9.6)],
                        words=[word(" a", 0.2, 0.7), word(" b", 0.7, 1.2), word(" x", 8.5, 8.55, **ODD), word(" y", 9.2, 9.25, **ODD)])}
    m, segs = _run(table, monkeypatch, audio=np.zeros(40 * SR, np.float32), hallucination_silence_threshold=THR)
    assert [(s.start, s.end, s.text) for s in segs] == [(30.2, 31.2, "ab")] and _seeks(m) == [0, 3000]
    # with more audio behind it the loop goes on at the dropped segment's start instead: max(30 + 1, 38.5) s
    m, segs = _run(table, monkeypatch, audio=np.zeros(50 * SR, np.float32), hallucination_silence_threshold=THR)
    assert [s.text for s in segs] == ["ab"] and _seeks(m) == [0, 3000, 3850]


def test_an_anomalous_segment_without_silence_around_it_is_kept(monkeypatch):
    """S2 starts 0.5 s after S1 ends, 10 s into the recording and the window: no silence before it, so it stays; rule 1 moves the
    seek to its end, 10.05 s."""
    m, segs = _run(KEPT, monkeypatch, hallucination_silence_threshold=THR)
    assert [(s.start, s.end, s.text) for s in segs] == [(8.2, 9.5, "ab"), (10.0, 10.05, "x")]
    assert _seeks(m) == [0, 1005, 4005, 7005]


def test_threshold_without_word_timestamps_warns_once_and_changes_nothing(monkeypatch):
    patch_alignment(monkeypatch)
    m0 = make_model(by_seek(DROP))
    want, _ = run(m0, AUDIO_100S)
    m = make_model(by_seek(DROP))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        segs, _ = run(m, AUDIO_100S, hallucination_silence_threshold=THR)
    assert [str(w.message) for w in seen] == ["hallucination_silence_threshold has no effect without word_timestamps=True"]
    assert segs == want and m.engine.calls == m0.engine.calls
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="hallucination_silence_threshold"):
            m.transcribe(AUDIO_100S, language="zh", word_timestamps=True, hallucination_silence_threshold=bad)


def test_lock_step_transcribe_many_equals_transcribe_with_a_threshold(monkeypatch):
    patch_alignment(monkeypatch)
    files = [AUDIO_100S, np.zeros(90 * SR, np.float32)]
    script = lambda n, seek, frames: (DROP if n == len(files[0]) else LEADING).get(seek)   # noqa: E731
    alone = []
    for f in files:
        m = make_model(script)
        alone.append(run(m, f, word_timestamps=True, hallucination_silence_threshold=THR)[0])
    m = make_model(script)
    got = m.transcribe_many(files, language="zh", beam_size=1, temperature=0.0, word_timestamps=True, hallucination_silence_threshold=THR)
    assert [g[0] for g in got] == alone and [s.text for s in alone[0]] == ["ab", "e"] and alone[1] == []
    # the words of a window decide its file's next seek: round 2 holds seek 1000 of the first file and 500 of the second
    assert [c[1] for c in m.engine.calls if c[0] == "win"][:3] == [[(0, None), (0, None)], [(1000, None), (500, None)],
                                                                   [(4000, None), (600, None)]]


# ------------------------------------------------------------------------------------- prompt_reset_on_temperature
@pytest.mark.parametrize("reset_above, carried", [(None, True), (0.5, True), (0.4, True), (0.3, False)])
def test_prompt_reset_on_temperature(reset_above, carried):
    """The first window fails its log-probability threshold at temperature 0 (-30 / 4 < -1) and is settled by the sampled attempt
    at 0.4: carried into the next prompt unless 0.4 exceeds the option."""
    table = {0: dict(tokens=[ts(0), A, ts(5)], lp=-30.0, sampled=dict(tokens=[ts(0), B, ts(5)], lp=-1.0))}
    m = make_model(by_seek(table))
    kw = {} if reset_above is None else dict(prompt_reset_on_temperature=reset_above)
    segs, _ = run(m, AUDIO_100S, temperature=(0.0, 0.4), **kw)
    assert [(s.text, s.temperature) for s in segs] == [("b", 0.4)]
    second = [p for k, p in m.engine.prompts() if k == 3000][0]
    if carried:
        assert second[:4] == [ST.sot_prev, ts(0), B, ts(5)]
    else:
        assert second[0] == ST.sot


# -------------------------------------------------------------------------------------------------- suppress_tokens
def _suppress_seen(m, **kw):
    m.engine.calls.clear()
    run(m, np.zeros(SR, np.float32), **kw)
    seen = [c[1] for c in m.engine.calls if c[0] == "opts"]
    assert len(seen) == 1
    return seen[0]


def test_suppress_tokens_table():
    m = make_model()
    model_list = default_suppress(ST, m.dims.vocab)
    always = sorted({ST.transcribe, ST.translate, ST.sot, ST.sot_prev, ST.sot_lm, ST.no_speech} - {-1})
    assert _suppress_seen(m) is None                                        # today: the engine's own default list
    assert _suppress_seen(m, suppress_tokens=[-1]) is None                  # the default value gives today's call
    assert _suppress_seen(m, suppress_tokens=(-1,)) is None
    assert _suppress_seen(m, suppress_tokens=[-1, 7]) == sorted(set(model_list + [7]))      # 7 (a quote mark) is in the list already
    assert 300 not in model_list and _suppress_seen(m, suppress_tokens=[-1, 300]) == sorted(model_list + [300])
    assert _suppress_seen(m, suppress_tokens=[300, -1, 300, model_list[0]]) == sorted(model_list + [300])
    assert _suppress_seen(m, suppress_tokens=[]) == always                  # only what no search may emit
    assert _suppress_seen(m, suppress_tokens=None) == always
    assert _suppress_seen(m, suppress_tokens=[7, 300]) == sorted(always + [7, 300])
    for bad in ([m.dims.vocab], [-2], [-1, 10 ** 6]):
        with pytest.raises(ValueError, match="suppress_tokens"):
            m.transcribe(np.zeros(SR, np.float32), language="zh", suppress_tokens=bad)
    # a model directory's own list (CTranslate2 config.json suppress_ids) is what -1 stands for
    m.ct2_config = {"suppress_ids": [5, 9]}
    today = _suppress_seen(m)
    assert today == sorted({5, 9, ST.transcribe, ST.translate, ST.sot, ST.sot_prev} | ({ST.sot_lm} - {-1}))
    assert _suppress_seen(m, suppress_tokens=[-1]) == today
    assert _suppress_seen(m, suppress_tokens=[-1, 7]) == sorted(today + [7])
    # transcribe_many takes the same option
    m.ct2_config = {}
    m.engine.calls.clear()
    m.transcribe_many([np.zeros(SR, np.float32)], language="zh", beam_size=1, temperature=0.0, suppress_tokens=[-1, 300])
    assert [c[1] for c in m.engine.calls if c[0] == "opts"] == [sorted(model_list + [300])]
