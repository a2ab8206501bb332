"""CPU-only checks of language detection inside sessions (ttasr_session_detect_language, ttasr_session_poll_lang): header,
binding list and library agree; a NULL context is refused; the Python Session arms before the first submit, passes the
placeholder through and calls the new poll only when armed; and the facade's detect_in_session surfaces run no detection pass
before the session and build prompts with the placeholder behind <|startoftranscript|>."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd.engine import Engine, Session, SessionResult, TtasrError
from taiwan_tongues_asr_ce_amd.model import LANGUAGES, WhisperModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ttasr_session_detect_language", "ttasr_session_poll_lang")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_library_and_binding_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in NEW:
        assert fn in declared and fn in exported and fn in _lib.SYMBOLS, fn
    assert exported == set(_lib.SYMBOLS) == declared
    assert re.search(r"#define\s+TTASR_TOKEN_DETECT\s+\(-1\)", hdr) and Session.DETECT == -1
    sig = re.search(r"int\s+ttasr_session_poll_lang\s*\(([^)]*)\)", hdr).group(1)
    assert re.sub(r"\s+", " ", sig) == (
        "ttasr_ctx* ctx, int32_t max_steps, int32_t cap, int64_t* ids, int32_t* tokens, int32_t* lens, float* sum_lp, "
        "float* no_speech, int32_t* lang, float* lang_probs, float* lang_logits, int32_t* n_out")


def test_null_context_is_refused(lib):
    i64, i32 = ctypes.c_int64(0), ctypes.c_int32(0)
    assert lib.ttasr_session_detect_language(None, 1, 2, 3) == -1
    assert lib.ttasr_session_poll_lang(None, 8, 1, ctypes.byref(i64), ctypes.byref(i32), ctypes.byref(i32), None, None,
                                       ctypes.byref(i32), None, None, ctypes.byref(i32)) == -1


# ---- the Python Session against a recording library ----

class _RecordingLib:
    """Stands in for libttasr: records every call the wrapper makes; `known` = the entry points it has (None: all)."""

    def __init__(self, known=None):
        self.calls, self.known = [], known

    def __getattr__(self, name):
        if self.known is not None and name not in self.known:
            raise AttributeError(name)

        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


class _FakeEngine:
    max_batch = 4
    audio_ctx = 1500

    def __init__(self, known=None):
        self.lib = _RecordingLib(known)
        self.h = None

    def _check(self, rc, what):
        if rc != 0:
            raise TtasrError(what)


def _opts(max_new=16):
    opts = _lib.GenOpts()
    opts.max_new_tokens = max_new
    return opts


def test_session_arms_before_the_first_submit_and_passes_the_placeholder_through():
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 6, detect_language=(100, 101, 99))
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin", "ttasr_session_detect_language"]
    assert eng.lib.calls[1][1][1:] == (100, 101, 99) and s.lang_span == (100, 101, 99)
    clip = np.zeros(16000, np.float32)
    s.submit([clip, clip], [[100, Session.DETECT, 7], [3, 4, 100, Session.DETECT, 7, 8]], [4, 5])
    name, args = eng.lib.calls[-1]
    assert name == "ttasr_session_submit"
    assert [args[4][i] for i in range(12)] == [100, -1, 7, 0, 0, 0, 3, 4, 100, -1, 7, 8]      # prompt rows, max_prompt 6
    s.poll()
    name, args = eng.lib.calls[-1]
    assert name == "ttasr_session_poll_lang" and len(args) == 12
    s.poll(with_language=False)
    assert eng.lib.calls[-1][0] == "ttasr_session_poll"
    s.close()
    # beam session: armed the same way
    eng = _FakeEngine()
    Engine.session(eng, _opts(), 6, beam=2, detect_language=(100, 101, 99))
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin_beam", "ttasr_session_detect_language"]
    with pytest.raises(ValueError):
        Engine.session(_FakeEngine(), _opts(), 6, detect_language=(100, 101))


def test_unarmed_session_needs_only_the_calls_it_always_made():
    """A library that knows only the session calls of before (the fakes of the other CPU tests): an unarmed session works."""
    eng = _FakeEngine(known={"ttasr_session_begin", "ttasr_session_submit", "ttasr_session_poll", "ttasr_session_end"})
    s = Engine.session(eng, _opts(), 4)
    assert s.lang_span is None
    s.submit([np.zeros(1600, np.float32)], [[1, 2]])
    assert s.poll() == []
    s.close()
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin", "ttasr_session_submit", "ttasr_session_poll", "ttasr_session_end"]


def test_a_refused_arming_closes_the_session():
    class Refusing(_RecordingLib):
        def __getattr__(self, name):
            f = super().__getattr__(name)
            return (lambda *a: (f(*a), -1)[1]) if name == "ttasr_session_detect_language" else f
    eng = _FakeEngine()
    eng.lib = Refusing()
    with pytest.raises(TtasrError):
        Engine.session(eng, _opts(), 4, detect_language=(1, 2, 3))
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin", "ttasr_session_detect_language", "ttasr_session_end"]


# ---- the facade: prompts and calls of the detect_in_session surfaces, against a scripted session ----

class _ScriptedSession:
    """Records what the facade submits; every clip comes back with two text tokens and, where its prompt held the placeholder,
    language `lang_of(clip index)` with probability 0.75."""

    def __init__(self, eng, kw):
        self.eng, self.kw, self.pending, self.next_id, self.ready = eng, kw, 0, 0, []
        self.prompts, self.armed = [], bool(kw.get("detect_language"))
        self.beam = kw.get("beam", 1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _queue(self, prompts):
        ids = []
        for p in prompts:
            p = list(p)
            assert self.armed or Session.DETECT not in p
            self.prompts.append(p)
            lang = probs = None
            if Session.DETECT in p:
                lang = self.eng.lang_of(self.next_id)
                probs = np.full(len(LANGUAGES) - 1, 0.25 / (len(LANGUAGES) - 2), np.float32)
                probs[lang] = 0.75
            self.ready.append(SessionResult(self.next_id, [11, 12], -0.5, 0.0, lang, probs, probs))
            ids.append(self.next_id)
            self.next_id += 1
        self.pending += len(ids)
        return ids

    def submit(self, clips, prompts, max_new=None):
        return self._queue(prompts)

    def submit_windows(self, files, seeks, prompts, sot_index, **kw):
        for p, si in zip(prompts, sot_index):
            assert p[si] == self.eng.special.sot
        return self._queue(prompts)

    def poll(self, *a, **k):
        out, self.ready = self.ready, []
        self.pending -= len(out)
        return out

    def drain(self):
        return self.poll()


def _scripted_engine_class():
    from oracle_engine import OracleEngine

    class ScriptedEngine(OracleEngine):
        sessions = []
        lang_of = staticmethod(lambda i: (24, 5, 94)[i % 3])

        def session(self, opts, max_prompt, temperature=0.0, beam=1, patience=None, **kw):
            s = _ScriptedSession(self, dict(kw, beam=beam))
            self.sessions.append(s)
            return s

    return ScriptedEngine


@pytest.fixture(scope="module")
def model():
    m = WhisperModel("synthetic:tiny", compute_type="float32", max_batch=4, _engine_factory=_scripted_engine_class())

    def boom(*a, **k):
        raise AssertionError("a detection pass ran before the session")
    m.detect_language_batch = boom
    return m


def _behind_sot(m, prompt):
    i = prompt.index(m.special.sot)
    return prompt[i + 1]


@pytest.mark.parametrize("initial_prompt", [None, "hello there"])
def test_transcribe_stream_detects_in_the_session(model, initial_prompt):
    m = model
    m.engine.sessions.clear()
    clips = [np.zeros(1600, np.float32)] * 3
    out = m.transcribe_stream(clips, language=[None, "ja", None], max_new_tokens=4, initial_prompt=initial_prompt,
                              detect_in_session=True)
    s = m.engine.sessions[-1]
    assert s.armed and out == [[11, 12]] * 3
    assert [_behind_sot(m, p) for p in s.prompts] == [Session.DETECT, m._lang_token("ja"), Session.DETECT]
    assert all((p[0] == m.special.sot_prev) == bool(initial_prompt) for p in s.prompts)
    assert all(p.count(Session.DETECT) <= 1 for p in s.prompts)
    assert m.last_language_info == [(LANGUAGES[24], 0.75), ("ja", 1.0), (LANGUAGES[94], 0.75)]
    # every language given: the session is not armed, even when asked
    m.transcribe_stream(clips, language="zh", max_new_tokens=4, detect_in_session=True)
    assert not m.engine.sessions[-1].armed
    # the default detects before the session, as before
    with pytest.raises(AssertionError, match="before the session"):
        m.transcribe_stream(clips, language=None, max_new_tokens=4)


QUIET = dict(temperature=0.0, no_speech_threshold=None, log_prob_threshold=None, compression_ratio_threshold=None,
             max_new_tokens=3, condition_on_previous_text=False, without_timestamps=True)


@pytest.mark.parametrize("initial_prompt", [None, "hello there"])
def test_transcribe_many_continuous_detects_in_the_session(model, initial_prompt):
    m = model
    m.engine.sessions.clear()
    n = m.n_window
    files = [np.zeros(2 * n, np.float32), np.zeros(n, np.float32)]
    out = m.transcribe_many(files, language=None, beam_size=2, continuous=True, detect_in_session=True,
                            initial_prompt=initial_prompt, **QUIET)
    s = m.engine.sessions[-1]
    # ids 0, 1: the first windows (placeholder); id 2: file 0's second window, with the language its first window found
    assert s.armed and len(s.prompts) == 3
    assert [_behind_sot(m, p) for p in s.prompts] == [Session.DETECT, Session.DETECT, m._lang_token(LANGUAGES[24])]
    assert all((p[0] == m.special.sot_prev) == bool(initial_prompt) for p in s.prompts[:2])
    infos = [info for _, info in out]
    assert [i.language for i in infos] == [LANGUAGES[24], LANGUAGES[5]]
    assert all(i.language_probability == 0.75 and i.all_language_probs[0] == (i.language, 0.75) for i in infos)
    assert all(i.window_languages is None for i in infos)
    with pytest.raises(ValueError, match="continuous"):
        m.transcribe_many(files, language=None, detect_in_session=True, **QUIET)


def test_transcribe_many_continuous_multilingual_detects_every_window(model):
    m = model
    m.engine.sessions.clear()
    n = m.n_window
    files = [np.zeros(2 * n, np.float32), np.zeros(n, np.float32)]
    out = m.transcribe_many(files, language=["ja", None], beam_size=2, continuous=True, multilingual=True, detect_in_session=True,
                            **QUIET)
    s = m.engine.sessions[-1]
    assert s.armed and [_behind_sot(m, p) for p in s.prompts] == [Session.DETECT] * 3
    infos = [info for _, info in out]
    assert [(i.language, i.language_probability) for i in infos] == [("ja", 1.0), (LANGUAGES[5], 0.75)]   # the file-level answers
    assert [i.window_languages for i in infos] == [[LANGUAGES[24], LANGUAGES[94]], [LANGUAGES[5]]]
