"""CPU-only checks of the continuous-batching session's interface (ttasr_session_*): the header declares it, the library exports
it, a NULL context is refused without a crash, and the Python wrapper rejects bad shapes and budgets before it calls the library."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd.engine import Session, TtasrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_FNS = ("ttasr_session_begin", "ttasr_session_submit", "ttasr_session_poll", "ttasr_session_stats", "ttasr_session_rows",
              "ttasr_session_end")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_declares_and_library_exports_the_session(lib):
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in SESSION_FNS:
        assert fn in declared and fn in exported and fn in _lib.SYMBOLS, fn
    # the option that picks the overlapped encode is documented with the other ttasr_set_option keys
    doc = hdr[hdr.index("kernel-selection overrides"):hdr.index("int ttasr_set_option")]
    assert '"refill_overlap"' in doc


def test_null_context_is_refused(lib):
    opts = _lib.GenOpts()
    opts.max_new_tokens = 8
    i64 = ctypes.c_int64(0)
    i32 = ctypes.c_int32(0)
    assert lib.ttasr_session_begin(None, ctypes.byref(opts), 4, ctypes.c_float(0.0)) == -1
    assert lib.ttasr_session_submit(None, 1, None, None, None, None, None, None) == -1
    assert lib.ttasr_session_poll(None, 8, 1, ctypes.byref(i64), ctypes.byref(i32), ctypes.byref(i32), None, None,
                                  ctypes.byref(i32)) == -1
    assert lib.ttasr_session_stats(None, (ctypes.c_double * 8)()) == -1
    assert lib.ttasr_session_rows(None, None, None, None) == -1
    assert lib.ttasr_session_end(None) == -1


class _RecordingLib:
    """Stands in for libttasr: records every call the wrapper makes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            return 0
        return f


class _FakeEngine:
    max_batch = 4
    audio_ctx = 1500

    def __init__(self):
        self.lib = _RecordingLib()
        self.h = None

    def _check(self, rc, what):
        if rc != 0:
            raise TtasrError(what)


def _session(max_new=16, max_prompt=4):
    opts = _lib.GenOpts()
    opts.max_new_tokens = max_new
    eng = _FakeEngine()
    s = Session(eng, opts, max_prompt)
    assert eng.lib.calls == ["ttasr_session_begin"]
    return s, eng.lib


def test_wrapper_rejects_bad_shapes_and_budgets_before_the_library():
    s, lib = _session()
    clip = np.zeros(16000, dtype=np.float32)
    bad = [
        dict(clips=[clip, clip], prompts=[[1, 2]], max_new=None),                                 # one prompt for two clips
        dict(clips=[], prompts=[], max_new=None),                                                 # nothing
        dict(clips=[clip], prompts=[[1, 2]], max_new=[0]),                                        # budget below 1
        dict(clips=[clip], prompts=[[1, 2]], max_new=[17]),                                       # budget above max_new_tokens
        dict(clips=[clip, clip], prompts=[[1], [1]], max_new=[4]),                                # one budget for two clips
        dict(clips=[clip], prompts=[[1, 2, 3, 4, 5]], max_new=None),                              # prompt longer than max_prompt
        dict(clips=[clip], prompts=[[]], max_new=None),                                           # empty prompt
        dict(clips=[np.zeros(30 * 16000 + 1, dtype=np.float32)], prompts=[[1]], max_new=None),    # longer than one window
        dict(clips=[np.zeros((2, 100), dtype=np.float32)], prompts=[[1]], max_new=None),          # not one-dimensional
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            s.submit(kw["clips"], kw["prompts"], kw["max_new"])
    with pytest.raises(ValueError):
        s.poll(cap=0)
    with pytest.raises(ValueError):
        s.poll(max_steps=0)
    assert lib.calls == ["ttasr_session_begin"]          # nothing reached the library
    assert s.submit([clip, clip], [[1, 2], [1, 2, 3, 4]], [1, 16]) == [0, 0]
    assert lib.calls[-1] == "ttasr_session_submit"
    s.close()
    assert lib.calls[-1] == "ttasr_session_end"
    with pytest.raises(TtasrError):
        s.submit([clip], [[1]])
