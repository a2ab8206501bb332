"""CPU-only checks of long-form files in the beam session (ttasr_session_submit_windows, transcribe_many(continuous=True)):
the header, the binding list and the library agree on the new entry point and a NULL context is refused without a crash;
Session.submit_windows refuses bad arguments before the library is called; and the continuous scheduler of transcribe_many,
run against a session whose windows are decoded by the CPU oracle (log_mel_windows, encode(1) and the static generate /
generate_beam / generate_sample of each attempt), reproduces the HF long-form goldens and transcribe()'s per-file results
with fallbacks, whatever order the session returns windows in."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import types
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, synth
from taiwan_tongues_asr_ce_amd.engine import Engine, SessionResult, TtasrError

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(ROOT, "golden")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_library_and_binding_agree_on_submit_windows(lib):
    hdr = open(os.path.join(os.path.dirname(ROOT), "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    name = "ttasr_session_submit_windows"
    assert name in declared and name in exported and name in _lib.SYMBOLS
    assert exported == set(_lib.SYMBOLS) == declared
    sig = re.search(r"int\s+ttasr_session_submit_windows\s*\(([^)]*)\)", hdr).group(1)
    assert re.sub(r"\s+", " ", sig) == (
        "ttasr_ctx* ctx, int32_t n, const float* const* file_pcm, const int64_t* file_samples, const int64_t* seek_frames, "
        "const float* floor_max, const int32_t* prompt, const int32_t* prompt_len, const int32_t* sot_index, "
        "const int32_t* max_new, const float* temperature, const int32_t* rows, const uint32_t* seed, int64_t* out_ids")


def test_null_context_is_refused(lib):
    assert lib.ttasr_session_submit_windows(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -1


# ---- Session.submit_windows argument checks (no library: a recorder stands in) ----

class _RecordingLib:
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


def _good(n=1):
    return dict(files=[np.zeros(16000 * 40, np.float32)] * n, seeks=[0] * n, prompts=[[1, 2, 3]] * n, sot_index=[0] * n)


def test_submit_windows_reaches_the_library_with_its_arguments():
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 8, beam=5, patience=1.0)
    ids = s.submit_windows(**_good(2), max_new=[4, 5], floor_max=[1.0, 2.0], temperature=[0.0, 0.4], rows=[5, 3], seed=[7, 8])
    name, args = eng.lib.calls[-1]
    assert name == "ttasr_session_submit_windows" and args[1] == 2 and len(ids) == 2 and s.pending == 2
    assert [args[3][i] for i in range(2)] == [640000, 640000]            # file lengths
    assert [args[11][i] for i in range(2)] == [5, 3]                     # rows
    assert [args[12][i] for i in range(2)] == [7, 8]                     # seeds
    assert args[5] is not None and args[10] is not None
    s.submit_windows(**_good(1))                                          # defaults: own floor, temperature 0, rows = beam
    name, args = eng.lib.calls[-1]
    assert args[5] is None and args[10][0] == 0.0 and args[11][0] == 5


@pytest.mark.parametrize("bad", [dict(rows=[0]), dict(rows=[6]), dict(temperature=[-0.1]), dict(temperature=[float("nan")]),
                                 dict(temperature=[float("inf")]), dict(seeks=[4000]), dict(seeks=[-1]),
                                 dict(sot_index=[3]), dict(sot_index=[-1]), dict(prompts=[[]]), dict(prompts=[list(range(9))]),
                                 dict(max_new=[0]), dict(max_new=[17]), dict(floor_max=[float("nan")]), dict(seed=[-1]),
                                 dict(seeks=[0, 0]), dict(files=[np.zeros((2, 100), np.float32)]), dict(rows=[1, 1])])
def test_submit_windows_argument_errors_are_raised_before_the_library(bad):
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 8, beam=5, patience=1.0)
    n_calls = len(eng.lib.calls)
    kw = _good(1)
    kw.update(bad)
    with pytest.raises(ValueError):
        s.submit_windows(**kw)
    assert len(eng.lib.calls) == n_calls and s.pending == 0


def test_submit_windows_needs_a_beam_session():
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 8)
    with pytest.raises(ValueError):
        s.submit_windows(**_good(1))
    assert [c[0] for c in eng.lib.calls] == ["ttasr_session_begin"]


# ---- the continuous scheduler against an oracle-decoded session ----

def _oracle_engine_class():
    from oracle_engine import OracleEngine

    class SessionOracleEngine(OracleEngine):
        """OracleEngine with a session(): each submitted window is decoded at once by the oracle's static calls (what a session
        clip equals bit for bit on the GPU); poll() hands the results back in REVERSE order of submission."""
        sessions = []

        def session(self, opts, max_prompt, temperature=0.0, beam=1, patience=None):
            s = _FakeSession(self, opts, max_prompt, beam, 1.0 if patience is None else patience)
            self.sessions.append(s)
            return s

    return SessionOracleEngine


class _FakeSession:
    def __init__(self, eng, opts, max_prompt, beam, patience):
        self.eng, self.opts, self.max_prompt, self.beam, self.patience = eng, opts, max_prompt, beam, patience
        self.ready, self.next_id, self.submitted, self.open = [], 0, [], True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.open = False

    def submit_windows(self, files, seeks, prompts, sot_index, max_new=None, floor_max=None, temperature=None, rows=None,
                       seed=None):
        assert self.open
        ids = []
        for i in range(len(files)):
            temp = 0.0 if temperature is None else float(temperature[i])
            nrow = self.beam if rows is None else int(rows[i])
            assert 1 <= nrow <= self.beam and len(prompts[i]) <= self.max_prompt and 0 <= sot_index[i] < len(prompts[i])
            o = types.SimpleNamespace(**vars(self.opts))
            o.max_new_tokens = int(max_new[i]) if max_new is not None else self.opts.max_new_tokens
            o.sot_index = int(sot_index[i])
            self.eng.log_mel_windows(files[i], [int(seeks[i])], floor_max=None if floor_max is None else [floor_max[i]])
            self.eng.encode(1)
            if temp > 0.0:
                res = self.eng.generate_sample([list(prompts[i])], nrow, o, temp, seed=int(seed[i]))
            elif nrow > 1:
                res = self.eng.generate_beam([list(prompts[i])], nrow, o, self.patience)
            else:
                res = self.eng.generate([list(prompts[i])], o)
            self.submitted.append(dict(seek=int(seeks[i]), temp=temp, rows=nrow, seed=None if seed is None else int(seed[i]),
                                       budget=o.max_new_tokens, plen=len(prompts[i])))
            self.ready.append(SessionResult(self.next_id, list(res.tokens[0]), float(res.sum_logprob[0]),
                                            float(res.no_speech_prob[0])))
            ids.append(self.next_id)
            self.next_id += 1
        return ids

    def poll(self, max_steps=1 << 30, cap=None):
        out, self.ready = self.ready[::-1], []
        return out


def _model(max_batch=1):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    return WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=max_batch,
                        _engine_factory=_oracle_engine_class())


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "longform.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["cond_prev_48", "no_cond_48"])
def test_continuous_transcribe_many_reproduces_hf_long_form_on_the_oracle(golden, name):
    from test_longform_golden import recording
    case = golden["cases"][name]
    kw = case["options"]
    audio_seconds = golden["n_samples"] / 16000.0
    m = _model()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (segs, _), = m.transcribe_many([recording()], language="zh", beam_size=1, temperature=0.0,
                                       condition_on_previous_text=kw["condition_on_prev_tokens"],
                                       max_new_tokens=kw["max_new_tokens"], no_speech_threshold=None, log_prob_threshold=None,
                                       compression_ratio_threshold=None, continuous=True)
    # the assertions of test_longform_golden.check_against_hf
    want = [h for h in case["segments"] if h["start"] < audio_seconds]
    assert len(segs) == len(want) >= 7
    seeks = set()
    for s, h in zip(segs, want):
        assert s.tokens in (h["tokens"], h["tokens"][:-1]), (s.tokens, h["tokens"])
        assert abs(s.start - h["start"]) < 1e-6
        assert abs(s.end - min(h["end"], audio_seconds)) < 1e-6
        seeks.add(s.seek)
    assert len(seeks) == 3 and min(seeks) == 0
    # every window went through the session once, greedily, with its own prompt, sot index and budget
    sess, = m.engine.sessions
    assert [w["seek"] for w in sess.submitted] == sorted(seeks)
    assert all(w["temp"] == 0.0 and w["rows"] == 1 for w in sess.submitted)
    assert all(w["budget"] == min(kw["max_new_tokens"], m.dims.n_text_ctx - w["plen"]) for w in sess.submitted)
    if kw["condition_on_prev_tokens"]:
        assert sess.submitted[1]["plen"] > 3


def _files():
    return [np.concatenate([synth.tonal_clip(3), synth.noise_clip(4)[:90000]]),
            synth.noise_clip(5)[:200000],
            np.concatenate([synth.noise_clip(6), synth.tonal_clip(7), synth.noise_clip(8)[:30000]])]


def test_continuous_transcribe_many_equals_transcribe_with_fallbacks():
    # thresholds every attempt fails (log-prob threshold 0): each window walks the whole ladder, the best attempt is kept,
    # and an attempt above temperature 0.5 resets the previous-text prompt
    kw = dict(language="zh", beam_size=2, best_of=2, temperature=(0.0, 0.4, 0.8), max_new_tokens=24, log_prob_threshold=0.0,
              no_speech_threshold=None, compression_ratio_threshold=2.4, condition_on_previous_text=True)
    files = _files()
    m = _model(max_batch=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [list(m.transcribe(a, **kw)[0]) for a in files]
        got = m.transcribe_many(files, continuous=True, **kw)
    assert len(got) == len(files)
    for (segs, _), ref in zip(got, want):
        assert segs == ref
        assert [s.seek for s in segs] == [s.seek for s in ref] and [s.avg_logprob for s in segs] == [s.avg_logprob for s in ref]
    assert {s.temperature for _, segs in zip(files, want) for s in segs} - {0.0}   # the fallback ladder was used
    sess = m.engine.sessions[-1]
    assert sess.beam == 2
    sampled = [w for w in sess.submitted if w["temp"] > 0]
    assert sampled and all(w["rows"] == 2 and w["seed"] == ((w["seek"] * 1000003 + int(w["temp"] * 1000)) & 0x7FFFFFFF)
                           for w in sampled)
    assert all(w["rows"] == 2 for w in sess.submitted if w["temp"] == 0.0)    # temperature 0: beam search of beam_size rows
    # files are independent: one file alone gives the same segments
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (alone, _), = m.transcribe_many([files[1]], continuous=True, **kw)
    assert alone == want[1]


def test_continuous_refuses_word_timestamps():
    m = _model()
    with pytest.raises(ValueError):
        m.transcribe_many([np.zeros(16000, np.float32)], continuous=True, word_timestamps=True)
    assert not m.engine.sessions


def test_batch_cli_passes_continuous_and_depth_one(tmp_path):
    from taiwan_tongues_asr_ce_amd import batch_cli
    for i in range(3):
        (tmp_path / f"a{i}.wav").write_bytes(b"")
    seen = []

    class M:
        max_batch, pipeline_depth, vad_speech_prob_fn = 10, 2, None

        def transcribe_many(self, audios, **kw):
            seen.append(kw)
            return [([], None) for _ in audios]

        def transcribe_groups(self, *a, **kw):
            raise AssertionError("continuous mode runs one context")

    logs = []
    batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=lambda f: np.zeros(160, np.float32), log=logs.append,
                                   output_json=str(tmp_path / "out.json"), continuous=True)
    assert seen and all(kw.get("continuous") is True for kw in seen)
    assert any("pipeline depth 1" in line for line in logs)
    seen.clear()
    batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=lambda f: np.zeros(160, np.float32), log=logs.append,
                                   output_json=str(tmp_path / "out.json"))
    assert all("continuous" not in kw for kw in seen)
