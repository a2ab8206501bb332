"""GPU: the contracts of the audio enhancement call (ttasr_enhance) and of dsp_mode on the file-level surfaces.

  - a recording's result is a function of its samples and the parameters alone, BIT FOR BIT: alone, in a batch of five mixed
    lengths, in the reversed batch, and under enhance_chunk values that put chunk boundaries inside a frame (1 000 samples: no
    multiple of the hop), inside a block (5 000: blocks are 4 096 samples) and inside the floor's 13-block window (33 000)
  - every refusal of include/ttasr.h, each followed by a successful call on the same context
  - transcribe(audio, dsp_mode=1) is transcribe(Engine.enhance([audio])[0]), tokens and segments; the same for lock-step and
    continuous transcribe_many; dsp_mode None and 0 are the call without the keyword"""
import ctypes as C
import threading

import numpy as np
import pytest

import enhance_cases as EC
from taiwan_tongues_asr_ce_amd import _lib, dsp, synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
from taiwan_tongues_asr_ce_amd.model import WhisperModel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))   # the call needs none; the session of the refusal test does
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=8)
    yield m
    m.close()


BATCH = [EC.bursts(80000, 31), EC.silence_mid(40000), EC.bursts(511, 32), np.zeros(0, np.float32), EC.rumble(4097)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


# ---- the contract -----------------------------------------------------------------------------------------------------------
def test_a_recording_alone_equals_itself_in_any_batch(eng):
    alone = [eng.enhance([a], return_gain=True) for a in BATCH]
    z_alone, g_alone = [z[0] for z, _ in alone], np.asarray([g[0] for _, g in alone])
    assert [len(z) for z in z_alone] == [len(a) for a in BATCH] and g_alone[3] == 1.0
    z, g = eng.enhance(BATCH, return_gain=True)
    assert _same(z, z_alone) and np.array_equal(g, g_alone)
    z, g = eng.enhance(BATCH[::-1], return_gain=True)
    assert _same(z[::-1], z_alone) and np.array_equal(g[::-1], g_alone)
    z2, _ = eng.enhance(BATCH, return_gain=True)          # the run
    assert _same(z2, z_alone)
    # in place: the output rows are the input rows (include/ttasr.h)
    rows = [a.copy() for a in BATCH]
    ptrs = (C.c_void_p * len(rows))(*[a.ctypes.data if len(a) else None for a in rows])
    ns = np.asarray([len(a) for a in rows], dtype=np.int64)
    p = _lib.DspParamsC(12.0, 3.0, dsp.DspParams().peak_target, 10.0, 7)
    assert eng.lib.ttasr_enhance(eng.h, len(rows), ptrs, ns.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(p), ptrs, None) == 0
    assert _same(rows, z_alone)
    # the result differs from the input (the call did something) and from one parameter set to the next
    assert not np.array_equal(z_alone[0], BATCH[0])
    assert not np.array_equal(eng.enhance([BATCH[0]], strength_db=20.0)[0], z_alone[0])


@pytest.mark.parametrize("chunk", [1000, 5000, 33000])
def test_chunk_boundaries_change_no_bit(eng, chunk):
    want, g_want = eng.enhance(BATCH, return_gain=True)
    probe_want = eng.enhance_probe(BATCH[0])
    eng.set_option("enhance_chunk", chunk)
    try:
        got, g = eng.enhance(BATCH, return_gain=True)
        probe = eng.enhance_probe(BATCH[0])
    finally:
        eng.set_option("enhance_chunk", 0)
    assert _same(got, want) and np.array_equal(g, g_want)
    assert all(np.array_equal(probe[k], probe_want[k]) for k in ("S", "Nf", "G", "out"))


def test_enhance_chunk_refuses_a_negative_value(eng):
    with pytest.raises(TtasrError):
        eng.set_option("enhance_chunk", -1)
    eng.set_option("enhance_chunk", 0)


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def _ok(e):
    z = e.enhance([BATCH[4]])
    assert len(z) == 1 and len(z[0]) == len(BATCH[4]) and np.isfinite(z[0]).all()


@pytest.mark.parametrize("fields, word", [
    (dict(flags=0), "flags"), (dict(flags=8), "flags"), (dict(flags=15), "flags"), (dict(flags=-1), "flags"),
    (dict(strength_db=float("nan")), "not finite"), (dict(max_gain=float("inf")), "not finite"),
    (dict(oversubtract=float("-inf")), "not finite"), (dict(peak_target=float("nan")), "not finite"),
    (dict(strength_db=-0.5), "strength_db"), (dict(strength_db=40.5), "strength_db"),
    (dict(oversubtract=0.0), "oversubtract"), (dict(oversubtract=16.5), "oversubtract"),
    (dict(peak_target=0.0), "peak_target"), (dict(peak_target=1.5), "peak_target"), (dict(max_gain=0.5), "max_gain"),
])
def test_parameters_are_refused_and_the_context_stays_usable(eng, fields, word):
    with pytest.raises(TtasrError, match=word):
        eng.enhance([BATCH[4]], **fields)
    with pytest.raises(TtasrError, match=word):
        eng.enhance_probe(BATCH[4], **fields)
    _ok(eng)


def test_the_ends_of_the_ranges_are_accepted(eng):
    eng.enhance([BATCH[4]], strength_db=0.0), eng.enhance([BATCH[4]], strength_db=40.0)
    eng.enhance([BATCH[4]], oversubtract=16.0), eng.enhance([BATCH[4]], peak_target=1.0), eng.enhance([BATCH[4]], max_gain=1.0)
    assert eng.enhance([]) == []


def test_lengths_rows_sessions_and_calls_in_flight_are_refused(eng):
    lib, h = eng.lib, eng.h
    p = _lib.DspParamsC(12.0, 3.0, 0.89, 10.0, 7)
    a = BATCH[4]
    out = np.zeros_like(a)
    i64p = C.POINTER(C.c_int64)

    def call(n, rows, lens, outs, params=p):
        ns = np.asarray(lens, dtype=np.int64)
        return lib.ttasr_enhance(h, n, (C.c_void_p * max(len(rows), 1))(*rows), ns.ctypes.data_as(i64p),
                                 C.byref(params) if params is not None else None, (C.c_void_p * max(len(outs), 1))(*outs), None)
    err = lambda: lib.ttasr_last_error(h).decode()   # noqa: E731
    assert call(1, [a.ctypes.data], [-1], [out.ctypes.data]) != 0 and "samples" in err()
    _ok(eng)
    assert call(1, [None], [len(a)], [out.ctypes.data]) != 0 and "NULL" in err()
    _ok(eng)
    assert call(1, [a.ctypes.data], [len(a)], [None]) != 0 and "NULL" in err()
    _ok(eng)
    assert call(-1, [a.ctypes.data], [len(a)], [out.ctypes.data]) != 0
    assert call(1, [a.ctypes.data], [len(a)], [out.ctypes.data], params=None) != 0 and "params" in err()
    assert lib.ttasr_enhance_probe(h, None, len(a), C.byref(p), None, None, None, out.ctypes.data) != 0 and "NULL" in err()
    assert lib.ttasr_enhance_probe(h, a.ctypes.data, -5, C.byref(p), None, None, None, out.ctypes.data) != 0
    _ok(eng)
    assert call(2, [None, a.ctypes.data], [0, len(a)], [None, out.ctypes.data]) == 0    # a recording of 0 samples is legal
    assert np.array_equal(out, eng.enhance([a], peak_target=0.89)[0])
    # an open session
    with eng.session(eng.gen_opts(8, True), 4):
        with pytest.raises(TtasrError, match="session"):
            eng.enhance([a])
        with pytest.raises(TtasrError, match="session"):
            eng.enhance_probe(a)
    _ok(eng)
    # a call in flight: the intruder is refused, the running call is not disturbed
    long = EC.bursts(4_000_000, 33)
    ref = eng.enhance([long])[0]
    eng.set_option("enhance_chunk", 4096)      # a thousand chunks: the call stays in flight for a while
    got, errors = {}, []

    def long_call():           # were an intruder to take the context first, this call would be the one refused: it tries again
        for _ in range(100):
            try:
                got["z"] = eng.enhance([long])[0]
                return
            except TtasrError:
                pass
    t = threading.Thread(target=long_call)
    t.start()
    for _ in range(5000):
        try:
            eng.enhance([BATCH[2]])
        except TtasrError as ex:
            errors.append(ex)
        if not t.is_alive():
            break
    t.join()
    eng.set_option("enhance_chunk", 0)
    assert np.array_equal(got["z"], ref) and len(errors) > 0
    _ok(eng)


# ---- dsp_mode on the surfaces ---------------------------------------------------------------------------------------------------
def _audio():
    # 40 s: two windows; quiet enough for the level stage to act, with a DC offset for the high-pass
    a = np.concatenate([synth.tonal_clip(0), synth.noise_clip(1)[: 10 * 16000]])
    return (np.float32(0.05) * a + np.float32(0.02)).astype(np.float32)


def _segs(segments):
    return [(s.start, s.end, s.text, tuple(s.tokens), s.avg_logprob, s.no_speech_prob) for s in segments]


def test_transcribe_with_dsp_mode_is_transcribe_of_the_enhanced_recording(model):
    a = _audio()
    kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, no_speech_threshold=None, max_new_tokens=20)
    enhanced = model.engine.enhance([a])[0]
    assert not np.array_equal(enhanced, a)
    want, info_want = model.transcribe(enhanced, **kw)
    want = _segs(want)
    got, info = model.transcribe(a, dsp_mode=1, **kw)
    assert _segs(got) == want and want and info.duration == info_want.duration
    got, _ = model.transcribe(a, dsp_mode=dsp.DspParams(), **kw)
    assert _segs(got) == want
    plain = _segs(model.transcribe(a, **kw)[0])
    for off in (None, 0):
        assert _segs(model.transcribe(a, dsp_mode=off, **kw)[0]) == plain
    # the parameters reach the device: level alone is another recording
    other = model.engine.enhance([a], params=dsp.DspParams(denoise=False, highpass=False))[0]
    assert _segs(model.transcribe(a, dsp_mode={"denoise": False, "highpass": False}, **kw)[0]) == _segs(model.transcribe(other, **kw)[0])


@pytest.mark.parametrize("continuous", [False, True])
def test_transcribe_many_with_dsp_mode_is_transcribe_many_of_the_enhanced_recordings(model, continuous):
    files = [_audio(), _audio()[: 12 * 16000][::-1].copy()]
    kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, no_speech_threshold=None, max_new_tokens=20,
              continuous=continuous)
    enhanced = model.engine.enhance(files)
    want = [_segs(s) for s, _ in model.transcribe_many(enhanced, **kw)]
    got = [_segs(s) for s, _ in model.transcribe_many(files, dsp_mode=1, **kw)]
    assert got == want and any(want)
    plain = [_segs(s) for s, _ in model.transcribe_many(files, **kw)]
    for off in (None, 0):
        assert [_segs(s) for s, _ in model.transcribe_many(files, dsp_mode=off, **kw)] == plain


def test_transcribe_batched_with_dsp_mode_is_transcribe_batched_of_the_enhanced_recording(model):
    import warnings
    a = _audio()
    kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, no_speech_threshold=None,
              compression_ratio_threshold=None, max_new_tokens=20, without_timestamps=False,
              clip_timestamps=[dict(start=0.0, end=25.0), dict(start=25.0, end=40.0)])   # two groups of one session
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enhanced = model.engine.enhance([a])[0]
        want = _segs(model.transcribe_batched(enhanced, **kw)[0])
        got = _segs(model.transcribe_batched(a, dsp_mode=1, **kw)[0])
        plain = _segs(model.transcribe_batched(a, **kw)[0])
        assert got == want and want
        assert _segs(model.transcribe_batched(a, dsp_mode=0, **kw)[0]) == plain


def test_live_surfaces_refuse_on_the_device_build_too(model):
    with pytest.raises(ValueError, match="causal, stateful noise tracker"):
        model.transcribe_stream([_audio()[:16000]], dsp_mode=1)
