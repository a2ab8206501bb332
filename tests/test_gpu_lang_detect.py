"""GPU: batched on-device language detection (ttasr_detect_language: a decoder pass at <|startoftranscript|> that ends in the
language head, kernels_lang.hip) against the CPU oracle, against the engine's own full vocabulary path, through odd shapes of the
raw C ABI, and end to end through the facade.

Weights: synth seed 0, profile gauss.  Clips: kinds[i % 4](i), kinds = (noise, tonal, burst, noise).
Tolerances: f32 span logits 1e-3 (the project's f32 tolerance), so log-probabilities 2e-3 (a difference of two values, each
within 1e-3 of its reference: |lse - lse_ref| <= max |x - x_ref|); bf16 0.08, fp16 0.015 below large-v3 width and 0.02 at it
(test_gpu_f16.py); winners must agree wherever the oracle's top-2 margin exceeds twice the tolerance.  Against the engine's own
vocabulary projection the 16-bit inputs are bit-identical and 16-bit products are exact in f32, so only the f32 summation order
differs: 1e-3."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import batch_cli, synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.model import LANGUAGES, WhisperModel

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KINDS = (synth.noise_clip, synth.tonal_clip, synth.burst_clip, synth.noise_clip)
CT = {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
_cache = {}


def _clip(i, preset="tiny"):
    n = 2 * PRESETS[preset].n_audio_ctx * 160
    return KINDS[i % 4](i)[:n]


def _engine(preset, mode, max_batch):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(PRESETS[preset], CT[mode], max_batch)
    e.load_weights(synth.iter_weights(PRESETS[preset]))
    return e


def _span(preset):
    """(first token, count): the model's language span; micro (one language token) takes an arbitrary span of its vocabulary."""
    if preset == "micro":
        return 7, 100
    from taiwan_tongues_asr_ce_amd.config import SpecialTokens
    st = SpecialTokens.for_vocab(PRESETS[preset].vocab)
    return st.sot + 1, min(min(st.translate, st.transcribe) - st.sot - 1, len(LANGUAGES))


def _oracle_span_logits(preset, mode, B):
    """Span logits [B][n_lang] of the oracle (weights rounded to the engine's storage type) at position 0 with [sot]; computed
    once per (preset, mode) and shared."""
    key = (preset, mode, B)
    if key not in _cache:
        pd = PRESETS[preset]
        rd = R.Dims(**pd.as_dict())
        if ("mel", preset, B) not in _cache:
            n = 2 * pd.n_audio_ctx * 160
            _cache[("mel", preset, B)] = np.stack([R.log_mel(_clip(i, preset), pd.n_mels, n) for i in range(B)])
        W = R.to_torch(synth.state_dict(pd), round_bf16=mode == "bf16", round_f16=mode == "f16")
        enc = R.encoder_forward(torch.from_numpy(_cache[("mel", preset, B)]), W, rd)
        from taiwan_tongues_asr_ce_amd.config import SpecialTokens
        sot = SpecialTokens.for_vocab(pd.vocab).sot
        lg = R.decoder_forward(torch.full((B, 1), sot), R.SelfCache.empty(rd.dec_layers), R.cross_kv(enc, W, rd), W, rd)[:, 0]
        b, n = _span(preset)
        out = lg[:, b:b + n].double().numpy()
        out.flags.writeable = False
        _cache[key] = out
    return _cache[key]


def _log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _tol(preset, mode):
    if mode == "f32":
        return 1e-3
    if mode == "bf16":
        return 0.08
    return 0.02 if preset == "large-v3-w2" else 0.015


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("preset", ["micro", "tiny", "large-v3-w2"])
def test_span_logits_probabilities_and_winner_against_the_oracle(preset, mode):
    """1 + 2: the language head against the oracle, and (16-bit) against the slice of the engine's own decode_step logits."""
    B = 8 if preset == "large-v3-w2" else 4
    tol = _tol(preset, mode)
    want = _oracle_span_logits(preset, mode, B)
    begin, n_lang = _span(preset)
    e = _engine(preset, mode, B)
    e.log_mel([_clip(i, preset) for i in range(B)], want_output=False)
    e.encode(B)
    idx, probs, logits = e.detect_language(B, want_logits=True, span=(begin, n_lang))
    err = float(np.abs(logits - want).max())
    lp_err = float(np.abs(np.log(probs.astype(np.float64)) - _log_softmax(want)).max())
    srt = np.sort(want, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    print(f"lang_detect {preset} {mode}: span logits max err {err:.3e}, log-prob max err {lp_err:.3e}, oracle margins "
          f"{np.round(margin, 3).tolist()}, winners {idx.tolist()}")
    assert err <= tol, err
    assert lp_err <= 2 * tol, lp_err
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, atol=1e-5)
    clear = margin > 2 * tol
    assert np.array_equal(idx[clear], want.argmax(axis=1)[clear])
    if preset == "large-v3-w2":   # checked on the CPU: margins >= 0.81 in every mode, one shared winner - so the vectors count
        assert clear.all() and (idx == 1).all(), (margin.tolist(), idx.tolist())
        assert np.abs(probs - np.exp(_log_softmax(want))).max() <= 2 * tol
    # the engine's own full path at the same position: decode_reset + decode_step([sot] * B), sliced
    e.decode_reset(B)
    full = e.decode_step([e.special.sot] * B)[:, begin:begin + n_lang]
    own = float(np.abs(logits - full).max())
    print(f"lang_detect {preset} {mode}: against the vocabulary projection of the same pass max {own:.3e}")
    assert own <= 1e-3, own
    assert np.array_equal(idx, np.argmax(logits, axis=1))
    e.close()


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_shapes_through_the_c_abi_on_micro(mode, generic):
    """3: spans of 1 .. 128 tokens starting at 0 and ending exactly at V, 1 / 2 / 5 clips; every row against the slice of the
    full step of the same batch, the softmax and the first maximum recomputed on the host."""
    V = PRESETS["micro"].vocab
    e = _engine("micro", mode, 5)
    if generic:
        e.set_option("generic_kernels", 1)
    e.log_mel([_clip(i, "micro") for i in range(5)], want_output=False)
    e.encode(5)
    for B in (1, 2, 5):
        e.decode_reset(B)
        full = e.decode_step([e.special.sot] * B)
        for n_lang in (1, 3, 64, 65, 99, 100, 128):
            for begin in (0, V - n_lang):
                idx, probs, logits = e.detect_language(B, want_logits=True, span=(begin, n_lang))
                assert np.abs(logits - full[:, begin:begin + n_lang]).max() <= 1e-3, (B, n_lang, begin)
                assert np.array_equal(idx, np.argmax(logits, axis=1)), (B, n_lang, begin)
                np.testing.assert_allclose(probs, np.exp(_log_softmax(logits)), atol=2e-6, err_msg=str((B, n_lang, begin)))
    # ties: a one-token span is certain, and the first of equal maxima wins
    idx, probs = e.detect_language(5, span=(V - 1, 1))
    assert (idx == 0).all() and (probs == 1.0).all()
    e.close()


def test_second_row_group_at_large_width():
    """3: 33 rows at large-v3 width (bf16); clip 32 repeats clip 0, so its row must repeat row 0 bit for bit."""
    B = 33
    e = _engine("large-v3-w2", "bf16", B)
    clips = [_clip(i % 32) for i in range(B)]
    e.log_mel(clips, want_output=False)
    e.encode(B)
    idx, probs, logits = e.detect_language(B, want_logits=True)
    e.decode_reset(B)
    b, n = e.language_span()
    full = e.decode_step([e.special.sot] * B)[:, b:b + n]
    assert np.abs(logits - full).max() <= 1e-3
    assert np.array_equal(logits[32], logits[0]) and np.array_equal(probs[32], probs[0]) and idx[32] == idx[0]
    assert np.array_equal(idx, np.argmax(logits, axis=1))
    e.close()


def test_isolation_state_and_refusals():
    """4: replay and permutation are bit-exact, a detection between encode and generate changes nothing, every refused call
    returns TTASR_E_INVALID with a message and leaves the context usable."""
    B = 4
    e = _engine("tiny", "bf16", B)
    st = e.special
    clips = [_clip(i) for i in range(B)]
    begin, n_lang = e.language_span()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    out = np.zeros(B, np.int32)

    def raw(B_=B, sot=st.sot, begin_=begin, n=n_lang, out_=out):
        return e.lib.ttasr_detect_language(e.h, B_, sot, begin_, n, out_.ctypes.data_as(i32p) if out_ is not None else None,
                                           None, None)

    assert raw() == -1 and b"encoder" in e.lib.ttasr_last_error(e.h)          # nothing resident yet
    e.log_mel(clips, want_output=False)
    e.encode(B)
    a = e.detect_language(B, want_logits=True)
    b = e.detect_language(B, want_logits=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(12, False)
    e.encode(B)
    g0 = e.generate([prompt] * B, opts)
    e.encode(B)
    e.detect_language(B)
    g1 = e.generate([prompt] * B, opts)
    assert g0.tokens == g1.tokens and np.array_equal(g0.sum_logprob, g1.sum_logprob)
    assert np.array_equal(g0.no_speech_prob, g1.no_speech_prob)
    for bad in (dict(out_=None), dict(B_=0), dict(B_=B + 1), dict(sot=-1), dict(sot=e.dims.vocab), dict(n=0), dict(n=129),
                dict(begin_=e.dims.vocab - n_lang + 1), dict(begin_=-1)):
        assert raw(**bad) == -1, bad
        assert len(e.lib.ttasr_last_error(e.h)) > 0
        assert raw() == 0, bad                                                 # the context stays usable
    with e.session(opts, len(prompt)):
        assert raw() == -1 and b"session" in e.lib.ttasr_last_error(e.h)
    e.log_mel(clips, want_output=False)
    e.encode(B)
    again = e.detect_language(B, want_logits=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))
    perm = [2, 0, 3, 1]
    e.log_mel([clips[p] for p in perm], want_output=False)
    e.encode(B)
    pa = e.detect_language(B, want_logits=True)
    assert all(np.array_equal(x[perm], y) for x, y in zip(a, pa))
    e.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------
# tiny with the language rows of embed_tokens multiplied by 16: those rows are never an input at position 0, so the span logits
# scale exactly and the synthetic model becomes decisive.  Checked on the CPU oracle: the files whose first windows are clips
# 1, 2, 5, 6 have margins 0.82, 2.58, 1.79, 2.63 in f32 (0.92, 2.60, 1.81, 2.65 with bf16 weights).
E2E_CLIPS = (1, 2, 5, 6)
E2E_LANGS = [LANGUAGES[94], LANGUAGES[24], LANGUAGES[5], LANGUAGES[24]]
QUIET = dict(temperature=0.0, no_speech_threshold=None, log_prob_threshold=None, compression_ratio_threshold=None,
             max_new_tokens=8, condition_on_previous_text=False)


def _decisive_factory():
    from taiwan_tongues_asr_ce_amd.engine import Engine

    class DecisiveEngine(Engine):
        def load_weights(self, tensors):
            b, n = self.language_span()

            def scaled():
                for name, arr in tensors:
                    if name == "model.decoder.embed_tokens.weight":
                        arr = np.array(arr, dtype=np.float32)
                        arr[b:b + n] *= 16.0
                    yield name, arr
            super().load_weights(scaled())
    return DecisiveEngine


def _model(compute_type, max_batch=8):
    return WhisperModel("synthetic:tiny", compute_type=compute_type, max_batch=max_batch, _engine_factory=_decisive_factory())


@pytest.mark.parametrize("compute_type", ["float32", "bfloat16"])
def test_transcribe_many_detects_each_file(compute_type):
    m = _model(compute_type)
    files = [_clip(i) for i in E2E_CLIPS]
    auto = m.transcribe_many(files, language=None, beam_size=2, **QUIET)
    assert [info.language for _, info in auto] == E2E_LANGS
    for _, info in auto:
        assert 0.0 < info.language_probability <= 1.0 and info.all_language_probs[0] == (info.language, info.language_probability)
        assert len(info.all_language_probs) == len(LANGUAGES) - (0 if m.dims.vocab == 51866 else 1)
    given = m.transcribe_many(files, language=E2E_LANGS, beam_size=2, **QUIET)
    assert [s for s, _ in auto] == [s for s, _ in given]
    assert all(info.language_probability == 1.0 and info.all_language_probs is None for _, info in given)
    mixed = m.transcribe_many(files, language=[None, E2E_LANGS[1], None, E2E_LANGS[3]], beam_size=2, **QUIET)
    assert [info.language for _, info in mixed] == E2E_LANGS and [s for s, _ in mixed] == [s for s, _ in given]
    cont = m.transcribe_many(files, language=None, beam_size=2, continuous=True, **QUIET)
    assert [info.language for _, info in cont] == E2E_LANGS
    # the other single-file entry points sit on the same call
    lang, p, allp = m.detect_language(files[1])
    assert lang == E2E_LANGS[1] and allp[0] == (lang, p)
    assert [r[0] for r in m.detect_language_batch(files)] == E2E_LANGS
    m.close()


def test_stream_batch_windows_and_folder_tool_detect():
    m = _model("bfloat16", max_batch=10)
    files = [_clip(i) for i in E2E_CLIPS]
    auto = m.transcribe_stream(files, language=None, max_new_tokens=8)
    assert [l for l, _ in m.last_language_info] == E2E_LANGS
    assert auto == m.transcribe_stream(files, language=E2E_LANGS, max_new_tokens=8)
    auto = m.transcribe_batch(files, language=None, max_new_tokens=8)
    assert [l for l, _ in m.last_language_info] == E2E_LANGS
    assert auto == m.transcribe_batch(files, language=E2E_LANGS, max_new_tokens=8)
    auto = m.transcribe_windows(files, language=None, beam_size=2, max_new_tokens=8)
    assert [l for l, _ in m.last_language_info] == E2E_LANGS
    assert auto == m.transcribe_windows(files, language=E2E_LANGS, beam_size=2, max_new_tokens=8)
    m.close()


def test_folder_tool_language_auto(tmp_path):
    m = _model("bfloat16", max_batch=10)
    folder = tmp_path / "audio"
    folder.mkdir()
    audio = {"a.wav": _clip(2), "b.wav": _clip(5)}
    for name in audio:
        (folder / name).write_bytes(b"")
    out = tmp_path / "out.json"
    final = batch_cli.process_audio_folder(str(folder), model=m, output_json=str(out), log=lambda *_: None, group_files=2,
                                           pipeline_depth=1, load_audio=lambda f: audio[os.path.basename(f)], language=None)
    got = json.load(open(out, encoding="utf-8"))["detailed_results"]
    assert [r["language"] for r in got] == [LANGUAGES[24], LANGUAGES[5]] == [r["language"] for r in final["detailed_results"]]
    assert all(0.0 < r["language_probability"] <= 1.0 for r in got)
    m.close()


def test_streaming_backend_reports_the_detected_language():
    """BatchedWhisperASR(language=None): every request's result names its own detected language and probability."""
    import asyncio
    import types
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    asr = BatchedWhisperASR(model_path="synthetic:micro", compute_type="bfloat16", beam_size=2, max_clips=4, max_new_tokens=8,
                            max_wait_ms=3000.0, language=None)
    asr.asr_pipeline.close()
    asr.asr_pipeline = _model("bfloat16")
    clients = [types.SimpleNamespace(scratch_buffer=(np.clip(_clip(i), -1, 1) * 32767).astype("<i2").tobytes(), last_start_time=0)
               for i in E2E_CLIPS]

    async def run():
        try:
            return await asyncio.gather(*[asr.transcribe(c) for c in clients])
        finally:
            await asr.aclose()
    seen, build = [], asr._result_dict      # what each request's result is built from (a blank text resolves to None)
    asr._result_dict = lambda res, last_start, lang=("zh", 1.0): (seen.append(lang), build(res, last_start, lang))[1]
    got = asyncio.run(run())
    assert asr.batches_run == [4]
    assert [l for l, _ in seen] == E2E_LANGS and all(0.0 < p <= 1.0 for _, p in seen)
    for r, (lang, prob) in zip(got, seen):
        assert r is None or (r["language"], r["language_probability"]) == (lang, prob)
    assert build(("x", 1.0), 0.0, seen[1])["language"] == E2E_LANGS[1]
    with pytest.raises(ValueError):
        BatchedWhisperASR(continuous=True, language=None)
    asr.asr_pipeline.close()


def test_transcribe_multilingual_detects_every_window():
    """5: a two-window file made of clip 2 followed by clip 5 puts LANGUAGES[24] and then LANGUAGES[5] into the two prompts."""
    m = _model("bfloat16")
    audio = np.concatenate([_clip(2), _clip(5)])
    prompts = []
    gen = m.engine.generate
    m.engine.generate = lambda ps, opts, *a, **k: (prompts.extend(list(p) for p in ps), gen(ps, opts, *a, **k))[1]
    segs, info = m.transcribe(audio, language=None, beam_size=1, multilingual=True, without_timestamps=True, **QUIET)
    list(segs)
    sot = m.special.sot
    assert [p[p.index(sot) + 1] - sot - 1 for p in prompts] == [24, 5], prompts
    assert info.language == LANGUAGES[24]
    m.close()
