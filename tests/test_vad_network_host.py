"""CPU: the Silero-v5-shaped VAD network around the device - the float64 restatement against the adapter's framing, the
synthetic weights, the suite's test signal, `transcribe_many(vad_filter=True)` against `transcribe` on a stub engine whose
vad_probs returns the reference probabilities, and the folder tool's choice of path."""
import os
import types
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, batch_cli, vad
from taiwan_tongues_asr_ce_amd.engine import GenResult, SessionResult
from vad_reference import SileroRef, cached_probs, test_signal

SEED = vad.SYNTH_SILERO_SEED
LENGTHS = (0, 1, 511, 512, 513, 576, 1024, 1100)


def _noise(n, seed=3):
    return (np.random.default_rng([0xA0D10, seed]).standard_normal(n) * 0.2).astype(np.float32)


# ---- the reference against the adapter's contract ----

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_step_through_the_adapter_equals_the_whole_recording(dtype):
    ref = SileroRef(vad.synth_silero_weights(SEED), dtype)
    fn = vad.silero_speech_prob_fn(lambda frame, state: ref.step(frame, state))
    for n in LENGTHS:
        audio = _noise(n, seed=n)
        whole = ref.probs(audio)
        assert whole.dtype == np.dtype(dtype) and len(whole) == -(-n // 512)
        assert np.array_equal(fn(audio), whole.astype(np.float32)), n


def test_reference_is_causal_and_stateful():
    ref = SileroRef(vad.synth_silero_weights(SEED))
    audio = _noise(512 * 6)
    p = ref.probs(audio)
    assert np.array_equal(ref.probs(audio[:512 * 3]), p[:3])            # a frame sees the past only
    assert not np.array_equal(ref.probs(audio[512 * 3:]), p[3:])         # ... and does see it: state and context carry over


# ---- synthetic weights ----

def test_synth_weights_are_deterministic_and_have_the_table_shapes():
    a, b, c = vad.synth_silero_weights(5), vad.synth_silero_weights(5), vad.synth_silero_weights(6)
    assert list(a) == list(vad.SILERO_V5_TENSORS)
    for name, shape in vad.SILERO_V5_TENSORS.items():
        assert a[name].shape == shape and a[name].dtype == np.float32
        assert np.array_equal(a[name], b[name])
    assert not np.array_equal(a["decoder.rnn.weight_hh"], c["decoder.rnn.weight_hh"])
    assert np.array_equal(a["stft.forward_basis_buffer"], c["stft.forward_basis_buffer"])   # the basis is no random draw


def test_stft_basis_reproduces_rfft_of_the_hann_windowed_frame():
    basis = vad.synth_silero_weights(SEED)["stft.forward_basis_buffer"][:, 0, :].astype(np.float64)
    x = np.random.default_rng(11).standard_normal(256)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(256) / 256)
    want = np.fft.rfft(x * hann)
    got = basis @ x
    assert np.abs(got[:129] - want.real).max() < 1e-5 and np.abs(got[129:] - want.imag).max() < 1e-5   # float32 storage of O(1) entries x 256


def test_load_silero_state_accepts_mappings_npz_and_strips_the_prefix(tmp_path):
    w = vad.synth_silero_weights(SEED)
    prefixed = {"_model." + k: v for k, v in w.items()}
    prefixed["_model_8k.stft.forward_basis_buffer"] = np.zeros((130, 1, 128), np.float32)   # the other branch is ignored
    got = vad.load_silero_state(prefixed)
    assert list(got) == list(w) and all(np.array_equal(got[k], w[k]) for k in w)
    path = str(tmp_path / "vad.npz")
    np.savez(path, **w)
    got = vad.load_silero_state(path)
    assert all(np.array_equal(got[k], w[k]) for k in w)
    with pytest.raises(ValueError):
        vad.load_silero_state({k: v for k, v in w.items() if k != "decoder.rnn.bias_hh"})
    with pytest.raises(ValueError):
        vad.load_silero_state(dict(w, **{"decoder.rnn.weight_ih": np.zeros((512, 64), np.float32)}))


def test_binding_mirrors_the_header_chunk():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ttasr.h")).read()
    assert f"#define TTASR_VAD_CHUNK_FRAMES {_lib.VAD_CHUNK_FRAMES}\n" in hdr
    assert all(s in _lib.SYMBOLS for s in ("ttasr_vad_load_tensor", "ttasr_vad_finalize", "ttasr_vad_probs"))


# ---- the test signal: conditions on the inputs, asserted ----

def test_signal_and_seed_keep_clear_of_the_thresholds():
    sig = test_signal()
    assert 38 * 16000 <= len(sig) <= 60 * 16000
    p, _ = cached_probs(SEED, "signal", sig)
    o = vad.VadOptions()
    neg = o.threshold - 0.15
    chunks = vad.get_speech_timestamps(sig, o, lambda a: p.astype(np.float32))
    print(f"test signal: {len(sig) / 16000:.1f} s, {len(chunks)} chunks, min |p - threshold| {np.abs(p - o.threshold).min():.3e}, "
          f"min |p - neg_threshold| {np.abs(p - neg).min():.3e}, p in [{p.min():.3f}, {p.max():.3f}]")
    assert len(chunks) >= 3
    assert np.abs(p - o.threshold).min() > 1e-3 and np.abs(p - neg).min() > 1e-3
    assert p.min() < 0.5 < p.max()


# ---- transcribe_many(vad_filter=True) against transcribe(vad_filter=True, vad_speech_prob_fn=reference) ----

class _StubEngine:
    """The Engine methods the window loops call, decoding every window into one deterministic segment whose letter depends on
    the window's samples and whose end timestamp is the window's length; vad_probs returns the float64 reference."""

    def __init__(self, dims, compute_type=0, max_batch=1, device=0):
        from taiwan_tongues_asr_ce_amd.config import SpecialTokens
        self.dims, self.max_batch = dims, max_batch
        self.special = SpecialTokens.for_vocab(dims.vocab)
        self.audio_ctx = dims.n_audio_ctx
        self.vad_state, self.vad_calls, self.windows, self.rows_decoded = None, [], [], 0

    def load_weights(self, tensors):
        pass

    def close(self):
        pass

    def set_audio_ctx(self, n_ctx=0):
        pass

    def load_vad(self, state):
        self.vad_state = state

    def vad_probs(self, audios, return_logits=False):
        assert self.vad_state is not None
        self.vad_calls.append(len(audios))
        return [cached_probs(SEED, ("stub", len(a), float(np.abs(a).sum())), a)[0].astype(np.float32) for a in audios]

    def log_mel_windows(self, audio, seeks, floor_max=None, want_output=False, want_max=False):
        files = [audio] * len(seeks) if isinstance(audio, np.ndarray) else list(audio)
        self.windows = [a[int(k) * 160:int(k) * 160 + self.dims.n_frames * 160] for a, k in zip(files, seeks)]
        return None, (np.zeros(len(seeks), np.float32) if want_max else None)

    def encode(self, B, want_output=False):
        assert B == len(self.windows)

    def gen_opts(self, max_new_tokens, timestamps, **kw):
        return types.SimpleNamespace(max_new_tokens=max_new_tokens, timestamps=timestamps, **kw)

    def _decode(self, n):
        tb = self.special.timestamp_begin
        toks = []
        for w in self.windows[:n]:
            units = max(1, min(self.dims.n_audio_ctx, len(w) // 320))
            toks.append([tb, 97 + int(np.abs(w).sum() * 1000) % 26, 98, tb + units])
        self.rows_decoded += n
        return GenResult(toks, np.full(n, -0.4, np.float32), np.zeros(n, np.float32))

    def generate(self, prompts, opts, row_max_new=None):
        return self._decode(len(prompts))

    def generate_beam(self, prompts, beam, opts, patience=1.0, sot_index=None):
        return self._decode(len(prompts))

    def session(self, opts, max_prompt, temperature=0.0, beam=1, patience=None, **kw):
        return _StubSession(self)


class _StubSession:
    def __init__(self, eng):
        self.eng, self.ready, self.next_id = eng, [], 0
        assert eng.vad_calls or eng.vad_state is None, "the VAD call comes before the session begins"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def submit_windows(self, files, seeks, prompts, sot_index, **kw):
        ids = []
        for f, k in zip(files, seeks):
            self.eng.log_mel_windows(f, [k])
            r = self.eng._decode(1)
            self.ready.append(SessionResult(self.next_id, r.tokens[0], float(r.sum_logprob[0]), 0.0))
            ids.append(self.next_id)
            self.next_id += 1
        return ids

    def poll(self, max_steps=1 << 30, cap=None):
        out, self.ready = self.ready[::-1], []
        return out


QUIET = dict(language="zh", beam_size=2, temperature=0.0, no_speech_threshold=None, log_prob_threshold=None,
             compression_ratio_threshold=None, max_new_tokens=8, condition_on_previous_text=False)


def _stub_model():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    return WhisperModel("synthetic:micro", compute_type="float32", max_batch=4, _engine_factory=_StubEngine,
                        vad_model=vad.synth_silero_weights(SEED))


@pytest.mark.parametrize("continuous", [False, True])
def test_transcribe_many_with_vad_equals_transcribe_file_by_file(continuous):
    m = _stub_model()
    assert m.has_device_vad and m.engine.vad_state is not None
    sig = test_signal()
    files = [sig, np.zeros(5 * 16000, np.float32), sig[: 20 * 16000]]
    ref_fn = lambda a: cached_probs(SEED, ("stub", len(a), float(np.abs(a).sum())), a)[0].astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # no "not available" / "energy" warning on this path
        many = m.transcribe_many(files, vad_filter=True, continuous=continuous, **QUIET)
        assert m.engine.vad_calls == [3]                                 # ONE call over all files
        rows_many = m.engine.rows_decoded
        for audio, (segs, info) in zip(files, many):
            want, want_info = m.transcribe(audio, vad_filter=True, vad_speech_prob_fn=ref_fn, **QUIET)
            want = list(want)
            assert segs == want
            assert (info.duration, info.duration_after_vad, info.language) == \
                   (want_info.duration, want_info.duration_after_vad, want_info.language)
    segs, info = many[0]
    chunks = vad.get_speech_timestamps(sig, vad.VadOptions(), ref_fn)
    assert len(segs) >= len(chunks) >= 3 and info.duration == len(sig) / 16000 > info.duration_after_vad > 0
    # times are on the ORIGINAL time line: every segment starts and ends inside a speech chunk (a window may straddle a removed
    # pause), the last one in the last chunk - later than the filtered audio is long
    spans = [(c["start"] / 16000 - 0.011, c["end"] / 16000 + 0.011) for c in chunks]
    inside = lambda t: any(a <= t <= b for a, b in spans)
    assert all(inside(s.start) and inside(s.end) and s.start < s.end for s in segs)
    assert segs[-1].end > spans[-1][0] > info.duration_after_vad
    assert many[1][0] == [] and many[1][1].duration == 5.0 and many[1][1].duration_after_vad == 0.0   # emptied by the VAD
    # the emptied file took no decode row: the rows are the windows of the other two files
    n_windows = sum(-(-max(len(vad.collect_chunks(a, vad.get_speech_timestamps(a, vad.VadOptions(), ref_fn))) // 160, 1)
                      // m.dims.n_frames) for a in (files[0], files[2]))
    assert rows_many == n_windows


def test_transcribe_many_rejects_nothing_new_without_vad_filter():
    m = _stub_model()
    sig = test_signal()[: 6 * 16000]
    plain = m.transcribe_many([sig], **QUIET)
    assert m.engine.vad_calls == [] and plain[0][1].duration == plain[0][1].duration_after_vad == 6.0


def test_source_order_explicit_function_then_device_then_energy_then_warning():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = _stub_model()
    sig = test_signal()[: 12 * 16000]
    seen = []
    m.transcribe(sig, vad_filter=True, vad_speech_prob_fn=lambda a: (seen.append(len(a)), np.ones(-(-len(a) // 512), np.float32))[1], **QUIET)
    assert seen == [len(sig)] and m.engine.vad_calls == []              # 1. the explicit function wins over the device
    m.transcribe(sig, vad_filter=True, **QUIET)
    assert m.engine.vad_calls == [1]                                     # 2. the device network
    m.transcribe(sig, vad_filter=True, vad_parameters={"backend": "energy"}, **QUIET)
    assert m.engine.vad_calls == [1, 1]                                  # ... also over the energy opt-in
    bare = WhisperModel("synthetic:micro", compute_type="float32", max_batch=4, _engine_factory=_StubEngine)
    assert not bare.has_device_vad
    with pytest.warns(UserWarning, match="energy"):                      # 3. the opt-in
        bare.transcribe(sig, vad_filter=True, vad_parameters={"backend": "energy"}, **QUIET)
    with pytest.warns(UserWarning, match="not available"):               # 4. today's warning
        bare.transcribe_many([sig], vad_filter=True, **QUIET)
    with pytest.raises(RuntimeError):
        bare.vad_speech_probs([sig])
    assert len(m.vad_speech_probs([sig, sig[:512]])[1]) == 1


def test_adapter_reports_an_active_vad_with_a_device_network():
    from taiwan_tongues_asr_ce_amd.asr import MI355XWhisperASR
    a = MI355XWhisperASR.__new__(MI355XWhisperASR)
    a.default_transcribe_kwargs = {}
    a.asr_pipeline = types.SimpleNamespace(vad_speech_prob_fn=None, has_device_vad=False)
    assert not a._vad_is_active()
    a.asr_pipeline.has_device_vad = True
    assert a._vad_is_active()


# ---- the folder tool ----

class _FolderModel:
    max_batch, pipeline_depth, vad_speech_prob_fn = 10, 1, None

    def __init__(self, device_vad):
        self.has_device_vad, self.many_kw, self.single = device_vad, [], 0

    def transcribe_many(self, audios, **kw):
        self.many_kw.append(kw)
        info = types.SimpleNamespace(language="zh", language_probability=1.0)
        return [([types.SimpleNamespace(text="x")], info) for _ in audios]

    def transcribe(self, audio, **kw):
        self.single += 1
        return [types.SimpleNamespace(text="y")], types.SimpleNamespace(language="zh", language_probability=1.0)


def _folder(tmp_path, n=3):
    d = tmp_path / "audio"
    d.mkdir()
    for i in range(n):
        (d / f"f{i}.wav").write_bytes(b"")
    return str(d)


def test_folder_tool_keeps_the_grouped_path_with_a_device_vad(tmp_path):
    run = lambda m, **kw: batch_cli.process_audio_folder(_folder(tmp_path), model=m, output_json=str(tmp_path / "o.json"),
                                                         log=lambda *_: None, load_audio=lambda f: np.zeros(16000, np.float32), **kw)
    m = _FolderModel(device_vad=True)
    run(m)
    assert m.single == 0 and len(m.many_kw) == 2 and all(kw["vad_filter"] is True for kw in m.many_kw)   # groups of 10 // 5 files
    import shutil
    shutil.rmtree(str(tmp_path / "audio"))
    m = _FolderModel(device_vad=True)
    run(m, continuous=True)
    assert m.single == 0 and m.many_kw[0]["vad_filter"] is True and m.many_kw[0]["continuous"] is True
    shutil.rmtree(str(tmp_path / "audio"))
    m = _FolderModel(device_vad=False)                                   # no VAD source: the grouped path without the option, as before
    run(m)
    assert m.single == 0 and "vad_filter" not in m.many_kw[0]
    shutil.rmtree(str(tmp_path / "audio"))
    m = _FolderModel(device_vad=True)                                    # a Python callable still means file by file
    m.vad_speech_prob_fn = lambda a: np.zeros(1, np.float32)
    run(m)
    assert m.single == 3 and m.many_kw == []
    assert batch_cli.build_parser().parse_args(["x", "--vad-model", "v.npz"]).vad_model == "v.npz"
