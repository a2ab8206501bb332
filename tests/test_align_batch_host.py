"""Host checks (no GPU) of the batched word alignment: the four new C-ABI names, their NULL-context answers, the Python
argument checks in front of the library, the shared word-building tail and the streaming result dict."""
import os
import re
import types

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd import alignment as A
from taiwan_tongues_asr_ce_amd.config import PRESETS, SpecialTokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ttasr_align_batch", "ttasr_session_hold", "ttasr_session_align", "ttasr_session_release"]


def test_header_map_and_symbols_agree_on_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"TTASR_API\s+[\w\s\*]+?\b(ttasr_\w+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert "global: ttasr_*;" in open(os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc", "ttasr.map")).read()


def test_null_context_is_invalid():
    lib = _lib.load()
    assert lib.ttasr_align_batch(None, 1, None, None, None, 2, None, None, None, 1, 7, None, None, None, None) == -1
    assert lib.ttasr_session_hold(None, 1) == -1
    assert lib.ttasr_session_align(None, 1, None, None, None, 2, None, None, None, 1, 7, None, None, None, None) == -1
    assert lib.ttasr_session_release(None, 1, None) == -1


class _Recorder:
    """Stands in for the library: records every call, answers 0."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def _fake_engine(max_batch=4):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e.h, e.dims, e.max_batch, e.audio_ctx = _Recorder(), None, PRESETS["tiny"], max_batch, 1500
    return e


GOOD = dict(clips=[0, 1], tokens=[[1, 2, 3, 4, 5], [1, 2, 3]], first_row=[1, 0], num_frames=[3000, 100], heads=[(3, 0), (2, 1)])


@pytest.mark.parametrize("bad", [
    dict(tokens=[]), dict(clips=[0] * 5, tokens=[[1, 2]] * 5, first_row=[0] * 5, num_frames=[1] * 5), dict(first_row=[1]),
    dict(num_frames=[1, 2, 3]), dict(medfilt_width=6), dict(medfilt_width=17), dict(medfilt_width=0), dict(tokens=[[1], [1, 2]]),
    dict(tokens=[[1] * 449, [1, 2]]), dict(first_row=[4, 0]), dict(first_row=[-1, 0]), dict(num_frames=[-1, 0]),
    dict(tokens=[[1, 2, 60000], [1, 2]]), dict(tokens=[[1, -2, 3], [1, 2]]), dict(heads=[]), dict(heads=[(4, 0)]), dict(heads=[(3, 6)]),
    dict(heads=[(3, 0), (3, 0)]), dict(clips=[0]), dict(clips=[0, 4]), dict(clips=[-1, 0])])
def test_align_batch_checks_fire_before_the_library(bad):
    e = _fake_engine()
    kw = dict(GOOD)
    kw.update(bad)
    with pytest.raises(ValueError):
        e.align_batch(**kw)
    assert e.lib.calls == []


def test_good_arguments_reach_the_library_once():
    e = _fake_engine()
    r = e.align_batch(**GOOD)
    assert e.lib.calls == ["ttasr_align_batch"]
    assert [len(x) for x in r.start_frames] == [3, 2] and [len(x) for x in r.logprobs] == [4, 2]


def test_session_checks_fire_before_the_library():
    from taiwan_tongues_asr_ce_amd.engine import Session, TtasrError
    e = _fake_engine()
    s = Session.__new__(Session)
    s.engine, s.open, s.holding, s.pending = e, True, False, 0
    kw = {k: v for k, v in GOOD.items() if k != "clips"}
    with pytest.raises(ValueError):
        s.align([7, 8], **kw)                                   # hold mode is off
    with pytest.raises(ValueError):
        s.release([7])
    s.hold()
    assert e.lib.calls == ["ttasr_session_hold"]
    for ids in ([], [7, 7], [7], list(range(5))):
        with pytest.raises(ValueError):
            s.align(ids, **kw)
    with pytest.raises(ValueError):
        s.align([7, 8], **dict(kw, medfilt_width=4))
    with pytest.raises(ValueError):
        s.release([3, 3])
    assert e.lib.calls == ["ttasr_session_hold"]
    s.align([7, 8], **kw)
    s.release([9])
    assert e.lib.calls == ["ttasr_session_hold", "ttasr_session_align", "ttasr_session_release"]
    s.open = False
    with pytest.raises(TtasrError):
        s.hold()


class _ZhTok:
    """token -> one CJK character; 20 / 21 are the punctuation marks that merge into the preceding word"""
    CHARS = {1: "一", 2: "丂", 3: "七", 20: "，", 21: "。"}

    def decode(self, toks):
        return "".join(self.CHARS[t] for t in toks if t < 50000)


def test_word_tail_literal_zh_case():
    """words_from_alignment (the tail find_alignment had inline before it was shared) on fixed start frames and log-probs, and
    add_word_timestamps' punctuation merging behind it: the literal result of the code before the refactor."""
    st = SpecialTokens.for_vocab(51865)
    text = [1, 2, 20, 3, 21]
    starts = np.array([10, 25, 40, 41, 60, 61, 90]) / A.TOKENS_PER_SECOND            # rows <|notimestamps|>, 5 text tokens, (eot row unused)
    logprob = np.log(np.array([1.0, 1.0, 1.0, 0.5, 0.25, 1.0, 0.125, 0.5, 0.9]))
    words = A.words_from_alignment(_ZhTok(), st, text, starts, logprob, 3, "zh")
    assert [(w["word"], w["tokens"], w["start"], w["end"]) for w in words] == [
        ("一", [1], 0.2, 0.5), ("丂", [2], 0.5, 0.8), ("，", [20], 0.8, 0.82), ("七", [3], 0.82, 1.2), ("。", [21], 1.2, 1.22)]
    np.testing.assert_allclose([w["probability"] for w in words], [0.5, 0.25, 1.0, 0.125, 0.5])
    seg = dict(tokens=text, start=0.0, end=2.0, eot=st.eot)
    A.add_word_timestamps([seg], words, 0.0)
    assert [(w.word, w.start, w.end) for w in seg["words"]] == [("一", 0.2, 0.5), ("丂，", 0.5, 0.8), ("七。", 0.82, 1.2)]


def test_find_alignment_batch_builds_the_sequences_find_alignment_feeds():
    st = SpecialTokens.for_vocab(51865)
    seen = {}

    class Fake:
        def align_batch(self, clips, seqs, first_row, num_frames, heads, medfilt_width):
            seen.update(clips=clips, seqs=seqs, first_row=first_row, num_frames=num_frames, width=medfilt_width)
            return types.SimpleNamespace(start_frames=[np.arange(len(s) - 4) * 5 for s in seqs],
                                         logprobs=[np.zeros(len(s) - 1, np.float32) for s in seqs])
    out = A.find_alignment_batch(Fake(), _ZhTok(), st, [2, 0, 1], [[1, 2], [], [3]], [3000, 10, 500], [(3, 0)])
    assert seen["clips"] == [2, 1] and seen["first_row"] == [3, 3] and seen["num_frames"] == [3000, 500] and seen["width"] == 7
    assert seen["seqs"] == [[st.sot, st.lang_zh, st.transcribe, st.no_timestamps, 1, 2, st.eot],
                            [st.sot, st.lang_zh, st.transcribe, st.no_timestamps, 3, st.eot]]
    assert out[1] == [] and [w["word"] for w in out[0]] == ["一", "丂"] and [w["start"] for w in out[0]] == [0.0, 0.1]


def test_result_dict_words_shape():
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR, _window_result
    asr = BatchedWhisperASR.__new__(BatchedWhisperASR)
    asr.text_filter = None
    words = [dict(word="一", start=0.2, end=0.5, probability=0.5), dict(word="丂。", start=0.5, end=0.9, probability=0.25)]
    audio = np.zeros(32000, np.float32)
    d = asr._result_dict(_window_result(audio, "一丂。", 1.5, words), 100.0)
    assert d["words"] == [dict(word="一", start=100.2, end=100.5, probability=0.5), dict(word="丂。", start=100.5, end=100.9, probability=0.25)]
    assert d["duration"] == 0.9 and d["text"] == "一丂。" and d["final"] is True
    plain = asr._result_dict(_window_result(audio, "一丂。", 1.5), 100.0)
    assert plain["words"] == [] and plain["duration"] == 1.5
    assert asr._result_dict(_window_result(audio, "一丂。", 1.5, []), 7.0)["words"] == []
    assert asr._result_dict(None, 0.0) is None
