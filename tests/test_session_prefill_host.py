"""CPU-only checks of prompt prefill at a session's admission (option session_prefill, ttasr_session_prefill_stats): header,
binding list and library agree; the option is documented and refused on a NULL context; the per-clip rule as a pure helper; the
packed-row tables of an admission pass (csrc/prefill_tables.hpp, through tests/prefill_tables_driver.cpp); and the keyword reaches
Engine.session(prefill=N) from transcribe_many(continuous=True), transcribe_stream, BatchedWhisperASR and batch_cli."""
import ctypes
import os
import re
import shutil
import subprocess
import types
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, config, synth
from taiwan_tongues_asr_ce_amd.engine import (Engine, Session, SessionResult, TtasrError, session_prefill_positions,
                                              session_prefill_value)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    name = "ttasr_session_prefill_stats"
    assert name in declared and name in exported and name in _lib.SYMBOLS
    assert exported == set(_lib.SYMBOLS) == declared
    assert re.search(r"int\s+ttasr_session_prefill_stats\s*\(\s*ttasr_ctx\*\s*ctx,\s*double\s+out\[4\]\s*\)", hdr)
    assert re.search(r"int\s+ttasr_session_stats\s*\(\s*ttasr_ctx\*\s*ctx,\s*double\s+out\[8\]\s*\)", hdr)     # keeps its eight values
    doc = hdr[hdr.index("kernel-selection overrides"):hdr.index("int ttasr_set_option")]
    assert '"session_prefill" [0]' in doc
    out4 = (ctypes.c_double * 4)()
    assert lib.ttasr_session_prefill_stats(None, out4) == -1
    assert lib.ttasr_set_option(None, b"session_prefill", 8) == -1


def test_the_rule_as_a_pure_helper():
    assert session_prefill_positions(64, 61, 8) == 61              # no-speech wanted: <|startoftranscript|> stays a real step
    assert session_prefill_positions(64, None, 8) == 63            # not wanted: all but the last prompt token
    assert session_prefill_positions(9, None, 8) == 8 and session_prefill_positions(8, None, 8) == 0
    assert session_prefill_positions(64, 5, 8) == 0                # capped below the threshold: forced
    assert session_prefill_positions(64, 61, 0) == 0               # the option off
    assert session_prefill_positions(64, 61, 8, placeholder=True) == 0
    assert session_prefill_value(True) == config.SESSION_PREFILL_DEFAULT == 16
    assert session_prefill_value(False) == session_prefill_value(None) == session_prefill_value(0) == 0
    assert session_prefill_value(12) == 12
    with pytest.raises(ValueError):
        session_prefill_value(-1)


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_packed_row_tables_through_the_driver(tmp_path):
    """The C++ builder (the engine's own header) against hand-written cases: lengths 1, 128, 129 and 446, a split at the
    workspace's 512 rows, and the rule; the Python helper above states the same rule."""
    exe = str(tmp_path / "prefill_tables_driver")
    cc = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "prefill_tables_driver.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "prefill tables: ok" in run.stdout


# ---- the Python Session against a recording library ----

class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


class _FakeEngine:
    max_batch = 8
    audio_ctx = 1500

    def __init__(self):
        self.lib = _RecordingLib()
        self.h = None
        self.options = []

    def _check(self, rc, what):
        if rc != 0:
            raise TtasrError(what)

    def set_option(self, key, value):
        self.options.append((key, value))


def _opts(max_new=16):
    opts = _lib.GenOpts()
    opts.max_new_tokens = max_new
    return opts


def test_session_sets_the_option_for_its_begin_and_restores_it():
    eng = _FakeEngine()
    with Engine.session(eng, _opts(), 8, prefill=12) as s:
        assert eng.options == [("session_prefill", 12)] and [c[0] for c in eng.lib.calls] == ["ttasr_session_begin"]
        st = s.stats()
        assert {"prefill_passes", "prefill_clips", "prefill_positions", "prefill_ms"} <= set(st) and "steps" in st
    assert eng.options == [("session_prefill", 12), ("session_prefill", 0)]
    assert [c[0] for c in eng.lib.calls][-1] == "ttasr_session_end"
    eng = _FakeEngine()
    with Engine.session(eng, _opts(), 8, beam=3, patience=1.0, prefill=True):
        pass
    assert eng.options == [("session_prefill", config.SESSION_PREFILL_DEFAULT), ("session_prefill", 0)]
    eng = _FakeEngine()
    with Engine.session(eng, _opts(), 8):                  # the default: the option is never touched
        pass
    assert eng.options == []
    with pytest.raises(ValueError):
        Engine.session(_FakeEngine(), _opts(), 8, prefill=-2)
    # the keyword owns the option: a value the caller had set is replaced for the session and put back behind it
    eng = _FakeEngine()
    eng._session_prefill = 8                                # as Engine.set_option("session_prefill", 8) leaves it
    with Engine.session(eng, _opts(), 8, prefill=24):
        pass
    assert eng.options == [("session_prefill", 24), ("session_prefill", 8)]
    eng.options.clear()
    with Engine.session(eng, _opts(), 8) as s:              # prefill=0: off for this session, whatever was set
        assert s.prefill == 0 and eng.options == [("session_prefill", 0)]
    assert eng.options == [("session_prefill", 0), ("session_prefill", 8)]
    eng.options.clear()
    with Engine.session(eng, _opts(), 8, prefill=8):        # already the value: no call at all
        pass
    assert eng.options == []


# ---- the facade: the keyword reaches Engine.session(prefill=N) ----

def _oracle_engine_class():
    from oracle_engine import OracleEngine
    from test_session_longform_host import _FakeSession

    class SessionOracleEngine(OracleEngine):
        sessions, kwargs = [], []

        def session(self, opts, max_prompt, temperature=0.0, beam=1, patience=None, **kw):
            self.kwargs.append(dict(kw))
            s = _FakeSession(self, opts, max_prompt, beam, 1.0 if patience is None else patience)
            self.sessions.append(s)
            return s

    return SessionOracleEngine


def _model(max_batch=1):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    return WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=max_batch,
                        _engine_factory=_oracle_engine_class())


def test_transcribe_many_passes_session_prefill_to_the_session():
    m = _model()
    audio = synth.noise_clip(5)[:100000]
    kw = dict(language="zh", beam_size=1, temperature=0.0, max_new_tokens=8, no_speech_threshold=None, log_prob_threshold=None,
              compression_ratio_threshold=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        base = m.transcribe_many([audio], continuous=True, **kw)
        assert m.engine.kwargs[-1] == {}                                     # off by default: the session call of before
        got = m.transcribe_many([audio], continuous=True, session_prefill=16, **kw)
        assert m.engine.kwargs[-1] == {"prefill": 16}
        m.transcribe_many([audio], continuous=True, session_prefill=True, **kw)
        assert m.engine.kwargs[-1] == {"prefill": config.SESSION_PREFILL_DEFAULT}
    assert [s.tokens for s in got[0][0]] == [s.tokens for s in base[0][0]]
    n = len(m.engine.sessions)
    with pytest.raises(ValueError):
        m.transcribe_many([audio], session_prefill=16, **kw)                 # refused without continuous
    assert len(m.engine.sessions) == n


def test_batch_cli_parses_and_passes_the_flag(tmp_path):
    from taiwan_tongues_asr_ce_amd import batch_cli
    args = batch_cli.build_parser().parse_args([str(tmp_path), "--continuous", "--session-prefill", "24"])
    assert args.continuous and args.session_prefill == 24
    assert batch_cli.build_parser().parse_args([str(tmp_path)]).session_prefill == 0
    assert batch_cli.main([str(tmp_path), "--session-prefill", "24"]) == 1   # needs --continuous
    for i in range(3):
        (tmp_path / f"a{i}.wav").write_bytes(b"")
    seen = []

    class M:
        max_batch, pipeline_depth, vad_speech_prob_fn = 10, 1, None

        def transcribe_many(self, audios, **kw):
            seen.append(kw)
            return [([], None) for _ in audios]

    load = lambda f: np.zeros(160, np.float32)
    batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=load, log=lambda *_: None,
                                   output_json=str(tmp_path / "out.json"), continuous=True, session_prefill=24)
    assert seen and all(kw.get("session_prefill") == 24 and kw.get("continuous") is True for kw in seen)
    seen.clear()
    batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=load, log=lambda *_: None,
                                   output_json=str(tmp_path / "out.json"), continuous=True)
    assert seen and all("session_prefill" not in kw for kw in seen)
    with pytest.raises(ValueError):
        batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=load, log=lambda *_: None, session_prefill=24)


def test_streaming_backend_refuses_the_keyword_without_continuous():
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    with pytest.raises(ValueError):
        BatchedWhisperASR(continuous=False, session_prefill=16)
