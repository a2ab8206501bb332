"""CPU-only checks of the beam-search mode of the continuous-batching session (ttasr_session_begin_beam): the header declares it,
the library exports it and nothing beyond the header, a NULL context is refused without a crash, Engine.session reaches the new
entry point with the caller's arguments and refuses a bad beam or patience before the library is called, and the streaming
backend refuses a continuous mode with a shortened encoder window."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_library_and_binding_agree_on_the_beam_session(lib):
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "ttasr_session_begin_beam" in declared
    assert "ttasr_session_begin_beam" in exported
    assert "ttasr_session_begin_beam" in _lib.SYMBOLS
    # the one new symbol and nothing else: header, binding list and export table name the same functions
    assert exported == set(_lib.SYMBOLS) == declared
    sig = re.search(r"int\s+ttasr_session_begin_beam\s*\(([^)]*)\)", hdr).group(1)
    assert re.sub(r"\s+", " ", sig) == ("ttasr_ctx* ctx, const ttasr_gen_opts* opts, int32_t max_prompt, int32_t beam, "
                                        "float patience")


def test_null_context_is_refused(lib):
    opts = _lib.GenOpts()
    opts.max_new_tokens = 8
    assert lib.ttasr_session_begin_beam(None, ctypes.byref(opts), 4, 5, ctypes.c_float(1.0)) == -1
    assert lib.ttasr_session_begin_beam(None, None, 4, 0, ctypes.c_float(0.0)) == -1


class _RecordingLib:
    """Stands in for libttasr: records every call the wrapper makes, with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


class _FakeEngine:
    max_batch = 30
    audio_ctx = 1500

    def __init__(self):
        self.lib = _RecordingLib()
        self.h = None

    def _check(self, rc, what):
        if rc != 0:
            raise TtasrError(what)


def _opts(max_new=16):
    opts = _lib.GenOpts()
    opts.max_new_tokens = max_new
    return opts


def test_engine_session_reaches_the_beam_entry_point_with_its_arguments():
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 4, beam=5, patience=1.5)
    (name, args), = eng.lib.calls
    assert name == "ttasr_session_begin_beam"
    assert args[2] == 4 and args[3] == 5 and args[4].value == pytest.approx(1.5)
    assert s.beam == 5
    s.close()
    assert eng.lib.calls[-1][0] == "ttasr_session_end"
    # beam 1 with an explicit patience is a beam session too; without one, and by default, the greedy session
    eng = _FakeEngine()
    Engine.session(eng, _opts(), 4, beam=1, patience=1.0)
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin_beam"] and eng.lib.calls[0][1][3] == 1
    for kw in (dict(), dict(beam=1)):
        eng = _FakeEngine()
        assert Engine.session(eng, _opts(), 4, **kw).beam == 0
        assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin"]


@pytest.mark.parametrize("kw", [dict(beam=0, patience=1.0), dict(beam=8), dict(beam=-5), dict(beam=5, patience=0.0),
                                dict(beam=5, patience=-1.0), dict(beam=5, patience=float("nan")),
                                dict(beam=5, temperature=0.5)])
def test_bad_beam_or_patience_is_refused_before_the_library(kw):
    eng = _FakeEngine()
    with pytest.raises(ValueError):
        Engine.session(eng, _opts(), 4, **kw)
    assert eng.lib.calls == []


def test_continuous_streaming_refuses_a_short_encoder_window():
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    with pytest.raises(ValueError):
        BatchedWhisperASR(continuous=True, audio_ctx="auto")
    with pytest.raises(ValueError):
        BatchedWhisperASR(continuous=True, audio_ctx=500)
