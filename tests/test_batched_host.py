"""CPU-only checks of the batched single-recording path: ttasr_session_retry's declaration, export and binding; the argument
checks of Session.retry (a recording fake library); vad.merge_chunks and the group time line on hand-computed cases; and
BatchedInferencePipeline against a session double whose groups are decoded by the CPU oracle - every group must come out as
transcribe() decodes that group's audio alone, whatever order the session returns groups in."""
import os
import re
import shutil
import subprocess
import types
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, synth, vad
from taiwan_tongues_asr_ce_amd.engine import Engine, SessionResult, TtasrError

ROOT = os.path.dirname(os.path.abspath(__file__))
SR = 16000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- the entry point ----

def test_header_library_and_binding_agree_on_session_retry(lib):
    hdr = open(os.path.join(os.path.dirname(ROOT), "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    name = "ttasr_session_retry"
    assert name in declared and name in exported and name in _lib.SYMBOLS
    sig = re.search(r"int\s+ttasr_session_retry\s*\(([^)]*)\)", hdr).group(1)
    assert re.sub(r"\s+", " ", sig) == (
        "ttasr_ctx* ctx, int32_t n, const int64_t* ids, const int32_t* prompt, const int32_t* prompt_len, "
        "const int32_t* sot_index, const int32_t* max_new, const float* temperature, const int32_t* rows, "
        "const uint32_t* seed, int64_t* out_ids")
    assert len(lib.ttasr_session_retry.argtypes) == 11
    assert lib.ttasr_session_retry(None, 1, None, None, None, None, None, None, None, None, None) == -1   # NULL context


# ---- Session.retry argument checks (no library: a recorder stands in) ----

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


def _held_session(beam=5):
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 8, beam=beam, patience=1.0) if beam else Engine.session(eng, _opts(), 8)
    s.hold()
    return eng, s


def test_retry_reaches_the_library_with_its_arguments():
    eng, s = _held_session()
    ids = s.retry([3, 9], [[1, 2, 3], [4, 5]], [0, 1], max_new=[4, 5], temperature=[0.0, 0.4], rows=[5, 3], seed=[7, 8])
    name, args = eng.lib.calls[-1]
    assert name == "ttasr_session_retry" and args[1] == 2 and len(ids) == 2 and s.pending == 2
    assert [args[2][i] for i in range(2)] == [3, 9]                              # held ids
    assert [args[3][i] for i in range(16)] == [1, 2, 3, 0, 0, 0, 0, 0, 4, 5, 0, 0, 0, 0, 0, 0]   # prompts [n][max_prompt]
    assert [args[4][i] for i in range(2)] == [3, 2] and [args[5][i] for i in range(2)] == [0, 1]
    assert [args[6][i] for i in range(2)] == [4, 5] and [args[8][i] for i in range(2)] == [5, 3]
    assert abs(args[7][1] - 0.4) < 1e-7 and [args[9][i] for i in range(2)] == [7, 8]
    s.retry([3], [[1, 2, 3]], [0])                                               # defaults: budget, temperature 0, rows = beam
    name, args = eng.lib.calls[-1]
    assert args[6][0] == 16 and args[7][0] == 0.0 and args[8][0] == 5 and args[9][0] == 0


@pytest.mark.parametrize("bad", [dict(ids=[3, 3], prompts=[[1], [1]], sot_index=[0, 0]), dict(ids=[]), dict(ids=[[3]]),
                                 dict(prompts=[[1], [2]]), dict(sot_index=[0, 0]), dict(prompts=[[]]), dict(prompts=[list(range(9))]),
                                 dict(prompts=[[1, -1, 2]]), dict(sot_index=[3]), dict(sot_index=[-1]),
                                 dict(max_new=[0]), dict(max_new=[17]), dict(max_new=[4, 4]), dict(rows=[0]), dict(rows=[6]),
                                 dict(rows=[1, 1]), dict(temperature=[-0.1]), dict(temperature=[float("nan")]),
                                 dict(temperature=[float("inf")]), dict(seed=[-1]), dict(seed=[2 ** 32])])
def test_retry_argument_errors_are_raised_before_the_library(bad):
    eng, s = _held_session()
    n_calls = len(eng.lib.calls)
    kw = dict(ids=[3], prompts=[[1, 2, 3]], sot_index=[0])
    kw.update(bad)
    with pytest.raises(ValueError):
        s.retry(**kw)
    assert len(eng.lib.calls) == n_calls and s.pending == 0


def test_retry_needs_hold_mode_and_a_beam_session():
    eng = _FakeEngine()
    s = Engine.session(eng, _opts(), 8, beam=5, patience=1.0)
    with pytest.raises(ValueError):
        s.retry([3], [[1, 2, 3]], [0])                    # hold mode is off
    eng, s = _held_session(beam=0)
    with pytest.raises(ValueError):
        s.retry([3], [[1, 2, 3]], [0])                    # a greedy session
    assert "ttasr_session_retry" not in [c[0] for c in eng.lib.calls]


# ---- merge_chunks ----

def _spans(*pairs):
    return [dict(start=int(a * SR), end=int(b * SR)) for a, b in pairs]


def _shape(groups):
    return [(g["start"] / SR, g["end"] / SR, [(c["start"] / SR, c["end"] / SR) for c in g["segments"]]) for g in groups]


def test_merge_chunks_on_hand_computed_cases():
    got = vad.merge_chunks(_spans((0, 10), (12, 25), (26, 31), (50, 52), (70, 101)), 30 * SR)
    # (26-31) would end 31 s after the first group began; (50-52) ends 26 s after (26-31) began; the 31-s chunk is cut at 30 s,
    # its first piece ends exactly 30 s after it began and its last second cannot join it
    assert _shape(got) == [(0, 25, [(0, 10), (12, 25)]), (26, 52, [(26, 31), (50, 52)]), (70, 100, [(70, 100)]),
                           (100, 101, [(100, 101)])]
    # a chunk ending exactly at the limit joins; one sample more does not
    assert _shape(vad.merge_chunks(_spans((0, 10), (20, 30)), 30 * SR)) == [(0, 30, [(0, 10), (20, 30)])]
    late = _spans((0, 10)) + [dict(start=20 * SR, end=30 * SR + 1)]
    assert [len(g["segments"]) for g in vad.merge_chunks(late, 30 * SR)] == [1, 1]
    # a chunk of 2.5 limits: two whole pieces and a half, each its own group (a piece of the limit fills a group)
    assert _shape(vad.merge_chunks(_spans((5, 80)), 30 * SR)) == [(5, 35, [(5, 35)]), (35, 65, [(35, 65)]), (65, 80, [(65, 80)])]
    assert vad.merge_chunks([], 30 * SR) == []
    with pytest.raises(ValueError):
        vad.merge_chunks(_spans((0, 1)), 0)


@pytest.mark.parametrize("seed", range(5))
def test_merge_chunks_invariants(seed):
    rng = np.random.default_rng(seed)
    t, chunks = 0, []
    for _ in range(40):
        t += int(rng.integers(1, 9 * SR))
        n = int(rng.integers(1, 45 * SR)) if rng.random() < 0.15 else int(rng.integers(1, 12 * SR))
        chunks.append(dict(start=t, end=t + n))
        t += n
    limit = 30 * SR
    groups = vad.merge_chunks(chunks, limit)
    audio = np.arange(t + 1, dtype=np.float32)    # a sample is its own index
    joined = np.concatenate([vad.collect_chunks(audio, g["segments"]) for g in groups])
    assert np.array_equal(joined, vad.collect_chunks(audio, chunks))          # every sample of every chunk once, in chunk order
    for g in groups:
        assert sum(c["end"] - c["start"] for c in g["segments"]) <= g["end"] - g["start"] <= limit
        assert g["start"] == g["segments"][0]["start"] and g["end"] == g["segments"][-1]["end"]
    assert all(a["end"] <= b["start"] for a, b in zip(groups, groups[1:]))


# ---- the group time line ----

def test_group_times_map_back_across_a_seam():
    from taiwan_tongues_asr_ce_amd.batched import restore_group_times
    from taiwan_tongues_asr_ce_amd.model import Segment, Word
    pieces = _spans((10, 14), (20, 23))       # group audio: 4 s from 10 s, then 3 s from 20 s; the seam is at local 4 s
    seg = lambda a, b, words=None: Segment(0, 0, a, b, "x", [1], 0.0, -0.5, 1.0, 0.1, words)
    inside, straddling, last = restore_group_times([seg(0.5, 3.0), seg(3.0, 5.5), seg(5.5, 7.0)], pieces)
    assert (inside.start, inside.end) == (10.5, 13.0)
    assert (straddling.start, straddling.end) == (13.0, 21.5)     # 3.0 lies in the first piece, 5.5 - 4 = 1.5 s into the second
    assert (last.start, last.end) == (21.5, 23.0)                 # the group's duration maps to the end of its last piece
    words = [Word(3.0, 3.6, " a", 0.9),      # first piece
             Word(3.6, 4.2, " b", 0.8),      # middle 3.9: first piece, its end is kept inside the piece (14.0, not 14.2)
             Word(3.9, 4.5, " c", 0.7),      # middle 4.2: second piece (silence before: 16 s), its start kept at the piece's start
             Word(4.5, 5.5, " d", 0.6)]
    got, = restore_group_times([seg(3.0, 5.5, words)], pieces)
    assert [(w.start, w.end) for w in got.words] == [(13.0, 13.6), (13.6, 14.0), (20.0, 20.5), (20.5, 21.5)]
    assert [w.word for w in got.words] == [" a", " b", " c", " d"] and (got.start, got.end) == (13.0, 21.5)
    for w in got.words:
        assert any(p["start"] / SR <= w.start <= w.end <= p["end"] / SR for p in pieces)


# ---- the pipeline against an oracle-decoded session ----

class _FakeSession:
    """A hold-mode beam session whose clips are decoded at once by the engine's static calls (what a session clip equals bit
    for bit on the GPU); poll() hands results back in REVERSE order of submission.  `script`, when given, supplies the tokens."""

    def __init__(self, eng, opts, max_prompt, beam, patience, script=None):
        self.eng, self.opts, self.max_prompt, self.beam, self.patience, self.script = eng, opts, max_prompt, beam, patience, script
        self.ready, self.next_id, self.open, self.holding = [], 0, True, False
        self.audio, self.held, self.log = {}, set(), []
        self.n_encoded = self.max_inflight = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.open = False

    def hold(self, on=True):
        self.holding = bool(on)

    def _decode(self, what, key, prompt, sot, budget, temp, nrow, seed):
        assert self.open and 1 <= nrow <= self.beam and len(prompt) <= self.max_prompt and 0 <= sot < len(prompt)
        file, seek, floor = self.audio[key]
        o = types.SimpleNamespace(**vars(self.opts))
        o.max_new_tokens, o.sot_index = int(budget), int(sot)
        if self.script is not None:
            res = types.SimpleNamespace(tokens=[self.script(file)], sum_logprob=[-1.0], no_speech_prob=[0.0])
        else:
            self.eng.log_mel_windows(file, [seek], floor_max=[floor])
            self.eng.encode(1)
            if temp > 0.0:
                res = self.eng.generate_sample([list(prompt)], nrow, o, temp, seed=int(seed))
            elif nrow > 1:
                res = self.eng.generate_beam([list(prompt)], nrow, o, self.patience)
            else:
                res = self.eng.generate([list(prompt)], o)
        cid = self.next_id
        self.next_id += 1
        self.audio[cid] = self.audio[key]
        self.log.append(dict(what=what, temp=temp, rows=nrow, seed=int(seed), budget=int(budget), samples=len(file)))
        self.ready.append(SessionResult(cid, list(res.tokens[0]), float(res.sum_logprob[0]), float(res.no_speech_prob[0])))
        self.max_inflight = max(self.max_inflight, len(self.ready) + len(self.held))
        return cid

    def submit_windows(self, files, seeks, prompts, sot_index, max_new=None, floor_max=None, temperature=None, rows=None, seed=None):
        ids = []
        for i in range(len(files)):
            self.audio["new"] = (files[i], int(seeks[i]), None if floor_max is None else floor_max[i])
            self.n_encoded += 1
            ids.append(self._decode("submit", "new", prompts[i], sot_index[i], max_new[i], float(temperature[i]), int(rows[i]), seed[i]))
        return ids

    def retry(self, ids, prompts, sot_index, max_new=None, temperature=None, rows=None, seed=None):
        assert self.holding and all(i in self.held for i in ids) and len(set(ids)) == len(ids)
        out = []
        for k, i in enumerate(ids):
            self.held.discard(i)
            out.append(self._decode("retry", i, prompts[k], sot_index[k], max_new[k], float(temperature[k]), int(rows[k]), seed[k]))
        return out

    def release(self, ids):
        assert self.holding and all(i in self.held for i in ids)
        self.held -= set(ids)

    def poll(self, max_steps=1 << 30, cap=None):
        out, self.ready = self.ready[::-1], []
        self.held |= {r.id for r in out}
        return out

    def stats(self):
        return dict(clips_encoded=float(self.n_encoded), encodes=float(self.n_encoded))


def _oracle_engine_class(script=None):
    from oracle_engine import OracleEngine

    class SessionOracleEngine(OracleEngine):
        sessions = []

        def session(self, opts, max_prompt, temperature=0.0, beam=1, patience=None, detect_language=False, prefill=0):
            s = _FakeSession(self, opts, max_prompt, beam, 1.0 if patience is None else patience, script)
            self.sessions.append(s)
            return s

    return SessionOracleEngine


def _model(max_batch=6, script=None):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    return WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=max_batch,
                        _engine_factory=_oracle_engine_class(script))


CLIPS = [(1.0, 3.5), (6.0, 8.0), (9.5, 13.0)]


def _recording():
    return np.concatenate([synth.noise_clip(31, 5 * SR), synth.tonal_clip(32, 5 * SR), synth.noise_clip(33, 5 * SR)]).astype(np.float32)


# thresholds every attempt fails (log-prob threshold 0): each group walks the whole ladder and keeps its best attempt
KW = dict(language="zh", beam_size=2, best_of=2, temperature=(0.0, 0.4, 0.8), max_new_tokens=10, log_prob_threshold=0.0,
          no_speech_threshold=None, compression_ratio_threshold=2.4)


@pytest.fixture(scope="module")
def decoded():
    """The pipeline (retry on and off, and one group at a time) and transcribe() of every group, on one oracle engine."""
    from taiwan_tongues_asr_ce_amd import BatchedInferencePipeline
    m = _model()
    audio = _recording()
    clip_ts = [dict(start=a, end=b) for a, b in CLIPS]
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, kw in (("retry", {}), ("resubmit", dict(retry_held=False)), ("one", dict(batch_size=1))):
            if name == "one":     # the model's forwarder
                segs, info = m.transcribe_batched(audio, clip_timestamps=clip_ts, **KW, **kw)
            else:
                segs, info = BatchedInferencePipeline(m).transcribe(audio, clip_timestamps=clip_ts, **KW, **kw)
            out[name] = (list(segs), info, m.engine.sessions[-1])
        groups = [audio[int(a * SR):int(b * SR)] for a, b in CLIPS]
        out["alone"] = [list(m.transcribe(g, condition_on_previous_text=False, without_timestamps=True, vad_filter=False, **KW)[0])
                        for g in groups]
    return out


def test_every_group_equals_transcribe_of_its_audio(decoded):
    segs, info, sess = decoded["retry"]
    assert len(segs) == 3 and [s.id for s in segs] == [0, 1, 2]
    for s, (a, b), alone in zip(segs, CLIPS, decoded["alone"]):
        ref, = alone
        assert (s.text, s.tokens, s.temperature) == (ref.text, ref.tokens, ref.temperature)
        assert (s.avg_logprob, s.no_speech_prob, s.compression_ratio) == (ref.avg_logprob, ref.no_speech_prob, ref.compression_ratio)
        assert (s.start, s.end) == (round(a + ref.start, 2), round(a + ref.end, 2)) == (a, b)
    assert {s.temperature for s in segs} - {0.0}                          # the ladder was used
    assert info.duration == 15.0 and info.duration_after_vad == 8.0 and info.language == "zh"
    assert info.transcription_options["condition_on_previous_text"] is False
    assert [(c["start"], c["end"]) for c in info.chunks] == [(int(a * SR), int(b * SR)) for a, b in CLIPS]
    assert all(len(c["attempts"]) == 3 and [t[0] for t in c["attempts"]] == [0.0, 0.4, 0.8] for c in info.chunks)
    # one submission per group, every later attempt a retry with the ladder's parameters and transcribe()'s seeds
    assert [e["what"] for e in sess.log].count("submit") == 3 and [e["what"] for e in sess.log].count("retry") == 6
    assert all(e["rows"] == 2 and e["seed"] == int(e["temp"] * 1000) for e in sess.log)
    assert info.session["retries"] == 6 and info.session["clips_encoded"] == 3 and not sess.held and sess.holding


def test_resubmission_and_a_batch_of_one_give_the_same_segments(decoded):
    segs = decoded["retry"][0]
    again, info, sess = decoded["resubmit"]
    assert again == segs
    assert info.session["retries"] == 0 and info.session["clips_encoded"] == 9 == sum(len(c["attempts"]) for c in info.chunks)
    assert not sess.held
    one, info, sess = decoded["one"]
    assert one == segs and sess.max_inflight == 1 and decoded["retry"][2].max_inflight == 3


def test_timestamp_pairs_and_a_tail_give_three_segments():
    from taiwan_tongues_asr_ce_amd import BatchedInferencePipeline
    from taiwan_tongues_asr_ce_amd.config import PRESETS, SpecialTokens
    tb = SpecialTokens.for_vocab(PRESETS["tiny"].vocab).timestamp_begin
    script = lambda file: [tb, 1000, 1001, tb + 50, tb + 50, 1002, tb + 100, tb + 100, 1003, 1004]
    m = _model(script=script)
    audio = _recording()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        segs, info = BatchedInferencePipeline(m).transcribe(audio, clip_timestamps=[6.0, 10.0], language="zh", beam_size=1, temperature=0.0,
                                                            without_timestamps=False, log_prob_threshold=None,
                                                            compression_ratio_threshold=None, no_speech_threshold=None)
        segs = list(segs)
    assert [(s.start, s.end) for s in segs] == [(6.0, 7.0), (7.0, 8.0), (8.0, 10.0)]      # the last ends at the group's duration
    assert [s.tokens for s in segs] == [[tb, 1000, 1001, tb + 50], [tb + 50, 1002, tb + 100], [tb + 100, 1003, 1004]]
    assert [s.id for s in segs] == [0, 1, 2] and info.session["retries"] == 0


def test_a_long_recording_needs_vad_or_clip_timestamps_and_an_emptied_one_yields_nothing():
    from taiwan_tongues_asr_ce_amd import BatchedInferencePipeline
    m = _model()
    pipe = BatchedInferencePipeline(m)
    long = np.zeros(31 * SR, np.float32)
    with pytest.raises(ValueError, match="vad_filter.*clip_timestamps"):
        pipe.transcribe(long, language="zh", vad_filter=False)
    with pytest.raises(ValueError):
        pipe.transcribe(long, language="zh", chunk_length=31)
    with pytest.raises(TypeError):
        pipe.transcribe(long, language="zh", no_such_option=1)
    with pytest.warns(UserWarning, match="repetition_penalty"):
        segs, info = pipe.transcribe(long, language="zh", repetition_penalty=1.2,
                                     vad_speech_prob_fn=lambda a: np.zeros(-(-len(a) // 512), np.float32))
    assert list(segs) == [] and info.duration == 31.0 and info.duration_after_vad == 0.0 and info.chunks == []
    assert info.session == dict(retries=0.0) and not m.engine.sessions
    assert info.vad_options["max_speech_duration_s"] == 30.0 and info.vad_options["min_silence_duration_ms"] == 160


# ---- the surfaces ----

def test_batch_cli_batched_decodes_file_by_file_and_excludes_continuous(tmp_path):
    from taiwan_tongues_asr_ce_amd import batch_cli
    for i in range(2):
        (tmp_path / f"a{i}.wav").write_bytes(b"")
    seen = []

    class M:
        max_batch, pipeline_depth, vad_speech_prob_fn = 10, 1, None

        def transcribe_batched(self, audio, **kw):
            seen.append(kw)
            return iter([]), None

        def transcribe_many(self, *a, **kw):
            raise AssertionError("--batched decodes one file per session")

        transcribe = transcribe_many

    batch_cli.process_audio_folder(str(tmp_path), model=M(), load_audio=lambda f: np.zeros(160, np.float32), log=lambda *_: None,
                                   output_json=str(tmp_path / "out.json"), batched=True)
    assert len(seen) == 2 and all("condition_on_previous_text" not in kw and kw["vad_filter"] is True and kw["beam_size"] == 5
                                  and kw["language"] == "zh" for kw in seen)
    with pytest.raises(ValueError):
        batch_cli.process_audio_folder(str(tmp_path), model=M(), batched=True, continuous=True)
    assert batch_cli.main([str(tmp_path), "--batched", "--continuous"]) == 1
    assert batch_cli.build_parser().parse_args([str(tmp_path), "--batched"]).batched is True


def test_adapter_batched_sends_paths_through_the_pipeline():
    from taiwan_tongues_asr_ce_amd.asr import MI355XWhisperASR
    calls = []

    class M:
        def transcribe(self, path, **kw):
            calls.append(("transcribe", kw))

        def transcribe_batched(self, path, **kw):
            calls.append(("batched", kw))

    asr = MI355XWhisperASR.__new__(MI355XWhisperASR)
    asr.asr_pipeline, asr.device_resample = M(), False
    asr.default_transcribe_kwargs = {"word_timestamps": False, "vad_filter": True, "beam_size": 5, "condition_on_previous_text": True}
    for flag in (False, True):
        asr.batched = flag
        asr.transcribe_path("x.wav", beam_size=2)
    assert [c[0] for c in calls] == ["transcribe", "batched"]
    assert calls[0][1]["condition_on_previous_text"] is True and "condition_on_previous_text" not in calls[1][1]
    assert calls[1][1]["beam_size"] == 2 and calls[1][1]["language"] == "zh" and calls[1][1]["device_resample"] is False
