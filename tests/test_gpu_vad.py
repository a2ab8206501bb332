"""GPU: the Silero-v5-shaped VAD network on the device (ttasr_vad_*, kernels_vad.hip) against the float64 restatement of
tests/vad_reference.py on synthetic weights, its bit-level contracts, its isolation from the rest of the context, and
`vad_filter=True` through the facade.

Tolerances: every pre-sigmoid logit within 1e-3 absolute of float64 (the project's f32 parity tolerance, README.md), every
probability within 2.5e-4 (the sigmoid's slope is at most 1/4).  Each case prints its measured maximum and, beside it, the
distance of the float32 run of the same reference from float64 - what the number format itself costs."""
import ctypes as C
import json
import os
import warnings
import wave

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, batch_cli, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
from vad_reference import cached_probs, test_signal

pytestmark = pytest.mark.gpu

SEED = vad.SYNTH_SILERO_SEED
CHUNK = _lib.VAD_CHUNK_FRAMES
LENGTHS = (1, 511, 512, 513, 576, 1024, 1100)
MIXED = ((1, 511, 512, 513, 576), (1100, 1024, 513, 1, 576))
LOGIT_TOL, PROB_TOL = 1e-3, 2.5e-4
_engines = {}


def _noise(n, seed):
    return (np.random.default_rng([0xA0D10, seed]).standard_normal(n) * 0.2).astype(np.float32)


def _long():
    """512 (2 C + 3) samples of noise whose level changes every 0.7 s (silence included), so the probabilities move."""
    n = 512 * (2 * CHUNK + 3)
    rng = np.random.default_rng([0xA0D10, 77])
    level = np.repeat(rng.choice([0.0, 0.02, 0.1, 0.3], size=n // 11200 + 1), 11200)[:n]
    return (rng.standard_normal(n) * level).astype(np.float32)


def _engine(mode=COMPUTE_F32, max_batch=5):
    """One micro engine per compute mode with the synthetic VAD loaded, shared by the tests of this module."""
    key = (mode, max_batch)
    if key not in _engines:
        e = Engine(PRESETS["micro"], mode, max_batch)
        e.load_weights(synth.iter_weights(PRESETS["micro"]))
        e.load_vad(vad.synth_silero_weights(SEED))
        _engines[key] = e
    return _engines[key]


def _check(name, audios, keys, got_p, got_l):
    worst_l = worst_p = ref32_l = ref32_p = 0.0
    for a, k, p, l in zip(audios, keys, got_p, got_l):
        want_p, want_l = cached_probs(SEED, k, a)
        f32_p, f32_l = cached_probs(SEED, k, a, np.float32)
        assert p.shape == want_p.shape and l.shape == want_l.shape and p.dtype == np.float32
        if len(p):
            worst_l, worst_p = max(worst_l, float(np.abs(l - want_l).max())), max(worst_p, float(np.abs(p - want_p).max()))
            ref32_l, ref32_p = max(ref32_l, float(np.abs(f32_l - want_l).max())), max(ref32_p, float(np.abs(f32_p - want_p).max()))
    print(f"vad {name}: device vs float64 logits {worst_l:.3e} probs {worst_p:.3e}; float32 reference vs float64 logits "
          f"{ref32_l:.3e} probs {ref32_p:.3e}")
    assert worst_l <= LOGIT_TOL, worst_l
    assert worst_p <= PROB_TOL, worst_p


# ---- accuracy against float64 ----

def test_single_files_at_every_short_length():
    e = _engine()
    audios = [_noise(n, n) for n in LENGTHS]
    out = [e.vad_probs([a], return_logits=True) for a in audios]
    _check("n=1 short lengths", audios, [("noise", n) for n in LENGTHS], [o[0][0] for o in out], [o[1][0] for o in out])


def test_mixed_lengths_in_one_call_and_each_file_alone():
    e = _engine()
    for lens in MIXED:
        audios = [_noise(n, n) for n in lens]
        p, l = e.vad_probs(audios, return_logits=True)
        _check(f"n=5 mixed {lens}", audios, [("noise", n) for n in lens], p, l)
        for a, pi, li in zip(audios, p, l):          # file independence, bit for bit
            p1, l1 = e.vad_probs([a], return_logits=True)
            assert np.array_equal(p1[0], pi) and np.array_equal(l1[0], li)
    empty = e.vad_probs([np.zeros(0, np.float32), _noise(513, 513)])
    assert len(empty[0]) == 0 and np.array_equal(empty[1], e.vad_probs([_noise(513, 513)])[0])


def test_the_test_signal_and_its_chunk_list():
    e = _engine()
    sig = test_signal()
    assert -(-len(sig) // 512) > CHUNK                       # the signal crosses a time-chunk boundary of the call
    p, l = e.vad_probs([sig], return_logits=True)
    _check("40-s test signal", [sig], ["signal"], p, l)
    want = cached_probs(SEED, "signal", sig)[0].astype(np.float32)
    o = vad.VadOptions()
    got_chunks = vad.get_speech_timestamps(sig, o, lambda a: p[0])
    assert got_chunks == vad.get_speech_timestamps(sig, o, lambda a: want) and len(got_chunks) >= 3
    assert p[0].min() < 0.35 and p[0].max() > 0.5


def test_files_around_the_chunk_boundary():
    e = _engine()
    base = _long()
    lens = (512 * CHUNK - 1, 512 * CHUNK, 512 * CHUNK + 1, 512 * (2 * CHUNK + 3))
    audios = [base[:n] for n in lens]
    p, l = e.vad_probs(audios, return_logits=True)
    _check("chunk boundary", audios, [("long", n) for n in lens], p, l)
    assert [len(x) for x in p] == [CHUNK, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    assert float(np.ptp(p[3])) > 0.3                          # the values do move


# ---- bit-level contracts ----

def test_reproducible_and_causal():
    e = _engine()
    base = _long()
    full = e.vad_probs([base])[0]
    assert np.array_equal(full, e.vad_probs([base])[0])
    ks = (1, 2, CHUNK, CHUNK + 1)
    cut = e.vad_probs([base[:512 * k] for k in ks])
    for k, c in zip(ks, cut):
        assert len(c) == k and np.array_equal(c, full[:k]), k


def test_compute_mode_does_not_change_a_bit():
    audios = [_noise(n, n) for n in MIXED[1][:4]] + [test_signal()[: 512 * 40 + 7]]
    want = _engine(COMPUTE_F32).vad_probs(audios, return_logits=True)
    for mode in (COMPUTE_BF16, COMPUTE_F16):
        got = _engine(mode).vad_probs(audios, return_logits=True)
        for x, y in zip(want[0] + want[1], got[0] + got[1]):
            assert np.array_equal(x, y), mode


# ---- state isolation and refusals ----

def _generate(e):
    st = e.special
    opts = e.gen_opts(12, True, suppress=[1, 2, 7, st.sot], begin_suppress=[5, st.eot], check_interval=1)
    return e.generate([[st.sot, st.lang_zh, st.transcribe]] * 2, opts)


def test_generate_after_vad_probs_is_bit_identical():
    e = _engine(COMPUTE_BF16)
    n = PRESETS["micro"].n_frames * 160
    clips = [synth.noise_clip(i, n) for i in range(2)]
    e.log_mel(clips, want_output=False)
    e.encode(2)
    a = _generate(e)
    e.log_mel(clips, want_output=False)
    e.encode(2)
    e.vad_probs([_noise(1100, 1), test_signal()[: 16000 * 3]])
    b = _generate(e)
    assert a.tokens == b.tokens and np.array_equal(a.sum_logprob, b.sum_logprob) and np.array_equal(a.no_speech_prob, b.no_speech_prob)
    e.vad_probs([_noise(600, 2)])                                # ... and between the two generates of one encoder state
    c = _generate(e)
    assert a.tokens == c.tokens and np.array_equal(a.sum_logprob, c.sum_logprob)


def _raw_load(e, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    dims = (C.c_int64 * a.ndim)(*a.shape)
    return e.lib.ttasr_vad_load_tensor(e.h, name.encode(), a.ctypes.data_as(C.c_void_p), dims, a.ndim)


def _raw_probs(e, audios):
    n = len(audios)
    outs = [np.zeros(max(1, -(-len(a) // 512)), np.float32) for a in audios]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in audios])
    optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ns = np.asarray([len(a) for a in audios], dtype=np.int64)
    return e.lib.ttasr_vad_probs(e.h, n, ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), optr, None)


def test_refusals_leave_the_context_usable():
    w = vad.synth_silero_weights(SEED)
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))
    a = _noise(1100, 5)
    E_INVALID, E_WEIGHTS = -1, -4
    assert _raw_probs(e, [a]) == E_INVALID                        # nothing loaded
    assert _raw_load(e, "decoder.rnn.weight_ih", np.zeros((512, 64))) == E_WEIGHTS          # wrong shape
    assert _raw_load(e, "decoder.rnn.weight_xx", np.zeros((512, 128))) == E_WEIGHTS         # unknown name
    names = list(w)
    for k in names[:-1]:
        assert _raw_load(e, "_model." + k, w[k]) == 0             # the prefix is stripped
    assert e.lib.ttasr_vad_finalize(e.h) == E_WEIGHTS             # one tensor missing
    assert _raw_probs(e, [a]) == E_INVALID                        # not finalized
    assert _raw_load(e, names[-1], w[names[-1]]) == 0
    assert e.lib.ttasr_vad_finalize(e.h) == 0
    assert _raw_load(e, names[0], w[names[0]]) == E_INVALID       # read-only from here on
    want = _engine().vad_probs([a])[0]
    assert np.array_equal(e.vad_probs([a])[0], want)
    assert _raw_probs(e, [a, a, a]) == E_INVALID                  # n > max_batch
    assert e.lib.ttasr_vad_probs(e.h, 0, None, None, None, None) == E_INVALID
    ns = np.asarray([-1], dtype=np.int64)
    one = (C.c_void_p * 1)(a.ctypes.data)
    out = np.zeros(8, np.float32)
    optr = (C.c_void_p * 1)(out.ctypes.data)
    i64p = C.POINTER(C.c_int64)
    assert e.lib.ttasr_vad_probs(e.h, 1, one, ns.ctypes.data_as(i64p), optr, None) == E_INVALID     # negative length
    ns[0] = 1100
    null = (C.c_void_p * 1)(None)
    assert e.lib.ttasr_vad_probs(e.h, 1, null, ns.ctypes.data_as(i64p), optr, None) == E_INVALID    # NULL pcm with samples
    opts = e.gen_opts(4, True)
    with e.session(opts, 4):
        assert _raw_probs(e, [a]) == E_INVALID                    # an open session
        with pytest.raises(TtasrError):
            e.vad_probs([a])
    assert np.array_equal(e.vad_probs([a])[0], want)              # usable after every refusal
    sharer = Engine(PRESETS["micro"], COMPUTE_F32, 2, share_weights_with=e)
    assert _raw_probs(sharer, [a]) == E_INVALID                   # VAD weights are per context ...
    sharer.load_vad(w)
    assert np.array_equal(sharer.vad_probs([a])[0], want)         # ... and its own copy computes the same
    sharer.close()
    e.close()


# ---- the facade, tiny geometry, f32 engine ----

KW = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, max_new_tokens=20)


def test_transcribe_many_with_vad_equals_transcribe_file_by_file():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=8, vad_model=vad.synth_silero_weights(SEED))
    sig = test_signal()
    files = [sig, np.zeros(5 * 16000, np.float32)]
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)               # the device network filters: no "not available" warning
        single = []
        for f in files:
            segs, info = m.transcribe(f, vad_filter=True, **KW)
            single.append((list(segs), info))
        for continuous in (False, True):
            many = m.transcribe_many(files, vad_filter=True, continuous=continuous, **KW)
            for (segs, info), (want, want_info) in zip(many, single):
                assert [s.tokens for s in segs] == [s.tokens for s in want], continuous
                assert [(s.seek, s.start, s.end, s.temperature) for s in segs] == [(s.seek, s.start, s.end, s.temperature) for s in want]
                assert (info.duration, info.duration_after_vad) == (want_info.duration, want_info.duration_after_vad)
    (segs, info), (none, silent) = single
    assert info.duration == len(sig) / 16000 and 0 < info.duration_after_vad < 0.8 * info.duration
    assert none == [] and silent.duration == 5.0 and silent.duration_after_vad == 0.0
    chunks = vad.get_speech_timestamps(sig, vad.VadOptions(), lambda a: cached_probs(SEED, "signal", sig)[0].astype(np.float32))
    assert abs(info.duration_after_vad - sum(c["end"] - c["start"] for c in chunks) / 16000) < 1e-9
    m.close()


def _write_wav(path, x):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_folder_tool_with_vad_model_pipelined_equals_serial(tmp_path, monkeypatch):
    folder = tmp_path / "audio"
    folder.mkdir()
    sig = test_signal()
    for i, x in enumerate((sig[: 9 * 16000], np.zeros(3 * 16000, np.float32), sig[20 * 16000: 27 * 16000])):
        _write_wav(str(folder / f"f{i}.wav"), x)
    npz = str(tmp_path / "vad.npz")
    np.savez(npz, **vad.synth_silero_weights(SEED))
    monkeypatch.chdir(tmp_path)
    seen = []
    real = batch_cli.process_audio_folder
    monkeypatch.setattr(batch_cli, "process_audio_folder", lambda *a, **k: seen.append(real(*a, log=lambda *_: None, **k)))
    for depth in ("1", "2"):
        assert batch_cli.main([str(folder), "--model", "synthetic:tiny", "--compute-type", "float32", "--max-batch", "10",
                               "--group-files", "2", "--pipeline-depth", depth, "--vad-model", npz]) == 0
    serial, piped = ([(r["audio_file"], r["asr_result"], r.get("error")) for r in s["detailed_results"]] for s in seen)
    assert serial == piped and len(serial) == 3 and all(err is None for _, _, err in serial)   # two groups: 2 files + 1
    assert serial[1][1] == ""                                    # the silent file: emptied by the VAD
    assert json.load(open(tmp_path / "asr_comparison_results.json", encoding="utf-8"))["summary"]["total_files"] == 3
