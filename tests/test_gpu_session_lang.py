"""GPU: language identification inside continuous-batching sessions (ttasr_session_detect_language, ttasr_session_poll_lang,
lang_head_rows_kernel; Engine.session(detect_language=...), the detect_in_session surfaces of WhisperModel).

A clip whose prompt holds Session.DETECT directly behind <|startoftranscript|> first runs one detect step (<|startoftranscript|>
at position 0 against its own cross-KV); the language head runs behind that step on the device, the winner's token replaces the
placeholder and the row starts over at position 0.  Checked for every detected clip:
 (a) winner, probabilities and span logits are bit-identical to Engine.detect_language on the same clips in static passes of
     exactly max_batch clips (prompts never enter; in 16-bit the static encoder runs the session's GEMM family, option
     enc_gemm = 3, as for the static side of tests/test_gpu_session_beam.py - a static pass of 4 or 8 clips would otherwise take
     another family than the 32-clip passes of tests/test_gpu_session.py, which rounds differently);
 (b) the span logits are within test_gpu_lang_detect.py's tolerances of the CPU oracle at position 0 with [sot] (f32 1e-3, bf16
     0.08, fp16 0.015 / 0.02 at large width), winners equal wherever the oracle's margin exceeds twice the tolerance;
 (c) tokens, sum_logprob and no_speech are bit-identical to the same clip in a fresh unarmed session with the detected token
     written out;
 (d) the clips that gave their language are bit-identical to the same run in an unarmed session;
 (e) every clip is encoded once, and ttasr_session_stats out[4] grows by one live row-step per detected clip.
Weights: synth seed 0; clips kinds[i % 4](i) as in test_gpu_lang_detect.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS, SpecialTokens
from taiwan_tongues_asr_ce_amd.engine import Engine, Session, TtasrError
from taiwan_tongues_asr_ce_amd.model import LANGUAGES, WhisperModel

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KINDS = (synth.noise_clip, synth.tonal_clip, synth.burst_clip, synth.noise_clip)
CT = {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
DET = Session.DETECT
_cache = {}


def _clip(i, preset="tiny"):
    return KINDS[i % 4](i)[:2 * PRESETS[preset].n_audio_ctx * 160]


def _engine(preset, mode, max_batch):
    e = Engine(PRESETS[preset], CT[mode], max_batch)
    e.load_weights(synth.iter_weights(PRESETS[preset]))
    return e


def _span(preset):
    """(sot, first token, count): the model's language span; micro (one language token) takes an arbitrary span."""
    st = SpecialTokens.for_vocab(PRESETS[preset].vocab)
    if preset == "micro":
        return st.sot, 7, 100
    return st.sot, st.sot + 1, min(min(st.translate, st.transcribe) - st.sot - 1, len(LANGUAGES))


def _tol(preset, mode):
    if mode == "f32":
        return 1e-3
    if mode == "bf16":
        return 0.08
    return 0.02 if preset == "large-v3-w2" else 0.015


def _oracle_span_logits(preset, mode, clip_ids):
    """Span logits of the oracle (weights rounded to the storage type) at position 0 with [sot], one row per clip id; computed
    once per (preset, mode, clips) and shared, read-only."""
    key = (preset, mode, tuple(clip_ids))
    if key not in _cache:
        pd = PRESETS[preset]
        rd = R.Dims(**pd.as_dict())
        n = 2 * pd.n_audio_ctx * 160
        mkey = ("mel", preset, tuple(clip_ids))
        if mkey not in _cache:
            _cache[mkey] = np.stack([R.log_mel(_clip(i, preset), pd.n_mels, n) for i in clip_ids])
        W = R.to_torch(synth.state_dict(pd), round_bf16=mode == "bf16", round_f16=mode == "f16")
        enc = R.encoder_forward(torch.from_numpy(_cache[mkey]), W, rd)
        sot, b, k = _span(preset)
        lg = R.decoder_forward(torch.full((len(clip_ids), 1), sot), R.SelfCache.empty(rd.dec_layers), R.cross_kv(enc, W, rd), W, rd)[:, 0]
        out = lg[:, b:b + k].double().numpy()
        out.flags.writeable = False
        _cache[key] = out
    return _cache[key]


def _check_oracle(preset, mode, clip_ids, idx, logits):
    want = _oracle_span_logits(preset, mode, clip_ids)
    tol = _tol(preset, mode)
    err = float(np.abs(logits - want).max())
    srt = np.sort(want, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    print(f"session lang {preset} {mode}: span logits max err {err:.3e} (tol {tol}), oracle margins {np.round(margin, 3).tolist()}")
    assert err <= tol, err
    clear = margin > 2 * tol
    assert np.array_equal(np.asarray(idx)[clear], want.argmax(axis=1)[clear])


def _static_detect(e, clips, span, per_pass, mode, enc_gemm=None):
    """Engine.detect_language over static passes of exactly per_pass clips (the last pass is filled up with its first clip)."""
    enc_gemm = (3 if mode != "f32" else 0) if enc_gemm is None else enc_gemm
    e.set_option("prefill", 0)
    e.set_option("enc_gemm", enc_gemm)
    idx, probs, logits = [], [], []
    try:
        for i in range(0, len(clips), per_pass):
            chunk = list(clips[i:i + per_pass])
            k = len(chunk)
            chunk += [chunk[0]] * (per_pass - k)
            if isinstance(chunk[0], tuple):                    # (file, seek): a window clip
                e.log_mel_windows([f for f, _ in chunk], [s for _, s in chunk])
            else:
                e.log_mel(chunk, want_output=False)
            e.encode(per_pass)
            a, p, l = e.detect_language(per_pass, want_logits=True, span=span[1:])
            idx += a[:k].tolist()
            probs += list(p[:k])
            logits += list(l[:k])
    finally:
        e.set_option("prefill", 1)
        e.set_option("enc_gemm", 0)
    return idx, np.asarray(probs), np.asarray(logits)


def _run(s, submit):
    """submit(s) -> ids; drains the session; results in submission order and the statistics."""
    ids = submit(s)
    got = s.drain()
    where = {cid: i for i, cid in enumerate(ids)}
    assert sorted(where[r.id] for r in got) == list(range(len(ids)))
    out = [None] * len(ids)
    for r in got:
        out[where[r.id]] = r
    return out, s.stats()


def _same_decode(a, b, what):
    assert a.tokens == b.tokens, (what, a.tokens, b.tokens)
    assert np.float32(a.sum_logprob).tobytes() == np.float32(b.sum_logprob).tobytes(), (what, a.sum_logprob, b.sum_logprob)
    assert np.float32(a.no_speech_prob).tobytes() == np.float32(b.no_speech_prob).tobytes(), (what, a.no_speech_prob, b.no_speech_prob)


def _prompts(e, span, n, lang_tok):
    """The four kinds in turn: placeholder at index 1; placeholder behind a 3-token previous-text prefix; the language given;
    given, with the prefix."""
    st = e.special
    prefix = [st.sot_prev, 11, 12]
    tail = [st.transcribe, st.no_timestamps]
    out = []
    for i in range(n):
        k = i % 4
        out.append((prefix if k in (1, 3) else []) + [span[0], DET if k < 2 else lang_tok] + tail)
    return out


GREEDY = [("micro", 4, 10), ("tiny", 4, 10), ("large-v3-w2", 8, 12)]


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("preset,max_batch,n_clips", GREEDY, ids=[g[0] for g in GREEDY])
def test_greedy_session_detects_on_the_device(preset, max_batch, n_clips, mode):
    e = _engine(preset, mode, max_batch)
    span = _span(preset)
    clips = [_clip(i, preset) for i in range(n_clips)]
    caps = np.asarray([3 + i % 6 for i in range(n_clips)], np.int32)
    prompts = _prompts(e, span, n_clips, span[1] + 2)
    det = [i for i in range(n_clips) if DET in prompts[i]]
    max_prompt = max(len(p) for p in prompts)
    ref = _static_detect(e, [clips[i] for i in det], span, max_batch, mode)
    first = None
    for interval in (1, 8):   # 8: the detect step of a refilled row sits inside a replayed multi-step graph
        opts = e.gen_opts(8, False, suppress_eot=True, check_interval=interval)
        with e.session(opts, max_prompt, detect_language=span) as s:
            armed, st_armed = _run(s, lambda s: s.submit(clips, prompts, caps))
        assert [len(r.tokens) for r in armed] == caps.tolist()
        for i, r in enumerate(armed):
            assert (r.language is not None) == (i in det), i
        # (a) the static call on the same clips
        assert [armed[i].language for i in det] == ref[0]
        assert np.array_equal(np.stack([armed[i].language_probs for i in det]), ref[1])
        assert np.array_equal(np.stack([armed[i].language_logits for i in det]), ref[2])
        # (c) + (d) an unarmed session with every language written out
        plain = [[span[1] + armed[i].language if t == DET else t for t in p] for i, p in enumerate(prompts)]
        with e.session(opts, max_prompt) as s:
            unarmed, st_plain = _run(s, lambda s: s.submit(clips, plain, caps))
            assert all(r.language is None for r in unarmed)
        for i in range(n_clips):
            _same_decode(armed[i], unarmed[i], (interval, i))
        # (e)
        assert st_armed["clips_encoded"] == n_clips == st_plain["clips_encoded"]
        assert st_armed["live_row_steps"] == st_plain["live_row_steps"] + len(det)
        assert st_plain["live_row_steps"] == sum(len(p) - 1 + int(c) for p, c in zip(prompts, caps))
        if first is None:
            first = armed
        else:   # the polling interval changes nothing
            for i in range(n_clips):
                _same_decode(first[i], armed[i], ("interval", i))
    # (b) the oracle
    _check_oracle(preset, mode, det, ref[0], ref[2])
    e.close()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("beam", [2, 5])
def test_beam_session_detects_plain_and_window_clips(beam, mode):
    preset, max_batch = "tiny", 8
    e = _engine(preset, mode, max_batch)
    st, span = e.special, _span(preset)
    tail = [st.transcribe, st.no_timestamps]
    given = span[1] + 2
    opts = e.gen_opts(8, False, suppress_eot=True)
    n_win = 2 * PRESETS[preset].n_audio_ctx * 160
    long_file = np.concatenate([_clip(9), _clip(10)])[: n_win + 4000]
    # plain clips 0 (placeholder), 1 (given); window clips: greedy row 2 / 3, two sampled rows 4 / 5, beam group 6 / 7
    plain_clips = [_clip(0), _clip(1)]
    wins = [(_clip(2), 0), (_clip(3), 0), (long_file, 700), (_clip(5), 0), (_clip(6), 0), (long_file, 100)]
    rows = [1, 1, 2, 2, beam, beam]
    temps = [0.0, 0.0, 0.4, 0.4, 0.0, 0.0]
    seeds = [0, 0, 7, 8, 0, 0]

    def submit(lang_of):
        """lang_of[k]: the token at the language position of clip k (k = 0, 1 plain; 2 .. 7 windows)"""
        def go(s):
            ids = s.submit(plain_clips, [[st.sot, lang_of[0]] + tail, [st.sot, lang_of[1]] + tail], [6, 5])
            prefix = [st.sot_prev, 11, 12]
            pr = [(prefix if k % 3 == 0 else []) + [st.sot, lang_of[2 + k]] + tail for k in range(6)]
            ids += s.submit_windows([f for f, _ in wins], [sk for _, sk in wins], pr, [p.index(st.sot) for p in pr],
                                    max_new=[4, 5, 6, 7, 8, 3], temperature=temps, rows=rows, seed=seeds)
            return ids
        return go

    det = [0, 2, 4, 6]
    armed_lang = [DET if k in det else given for k in range(8)]
    with e.session(opts, 7, beam=beam, patience=1.0, detect_language=span) as s:
        armed, st_armed = _run(s, submit(armed_lang))
    for k, r in enumerate(armed):
        assert (r.language is not None) == (k in det), k
    # (c) + (d)
    written = [span[1] + armed[k].language if k in det else given for k in range(8)]
    with e.session(opts, 7, beam=beam, patience=1.0) as s:
        unarmed, st_plain = _run(s, submit(written))
    for k in range(8):
        _same_decode(armed[k], unarmed[k], k)
    # (e) one more live row-step per live row of a detected group
    assert st_armed["clips_encoded"] == 8 == st_plain["clips_encoded"]
    assert st_armed["live_row_steps"] == st_plain["live_row_steps"] + beam + 1 + 2 + beam
    # (a) static passes of max_batch clips: the plain clip in a plain pass, the window clips in a window pass
    ref_p = _static_detect(e, [plain_clips[0]], span, max_batch, mode)
    ref_w = _static_detect(e, [wins[0], wins[2], wins[4]], span, max_batch, mode)
    idx = ref_p[0] + ref_w[0]
    probs, logits = np.concatenate([ref_p[1], ref_w[1]]), np.concatenate([ref_p[2], ref_w[2]])
    assert [armed[k].language for k in det] == idx
    assert np.array_equal(np.stack([armed[k].language_probs for k in det]), probs)
    assert np.array_equal(np.stack([armed[k].language_logits for k in det]), logits)
    # (b) the plain clip and the two windows that are whole clips
    _check_oracle(preset, mode, [0, 2, 6], [idx[0], idx[1], idx[3]], logits[[0, 1, 3]])
    e.close()


def test_e4m3_cross_kv_session_detects():
    preset, mode, max_batch, n_clips = "large-v3-w2", "bf16", 16, 18
    e = _engine(preset, mode, max_batch)
    e.set_option("xkv_fp8", 2)
    span = _span(preset)
    clips = [_clip(i, preset) for i in range(n_clips)]
    caps = np.asarray([3 + i % 6 for i in range(n_clips)], np.int32)
    prompts = _prompts(e, span, n_clips, span[1] + 2)
    det = [i for i in range(n_clips) if DET in prompts[i]]
    opts = e.gen_opts(8, False, suppress_eot=True, check_interval=8)
    with e.session(opts, 7, detect_language=span) as s:
        armed, _ = _run(s, lambda s: s.submit(clips, prompts, caps))
    plain = [[span[1] + armed[i].language if t == DET else t for t in p] for i, p in enumerate(prompts)]
    with e.session(opts, 7) as s:
        unarmed, _ = _run(s, lambda s: s.submit(clips, plain, caps))
    for i in range(n_clips):
        _same_decode(armed[i], unarmed[i], i)
    ref = _static_detect(e, [clips[i] for i in det], span, max_batch, mode)   # the option stays at 2
    assert [armed[i].language for i in det] == ref[0]
    assert np.array_equal(np.stack([armed[i].language_probs for i in det]), ref[1])
    assert np.array_equal(np.stack([armed[i].language_logits for i in det]), ref[2])
    # the e4m3 cache was read: the 16-bit cache gives other logits
    e.set_option("xkv_fp8", 0)
    other = _static_detect(e, [clips[i] for i in det], span, max_batch, mode)
    assert not np.array_equal(other[2], ref[2])
    e.close()


def test_refusals_leave_context_and_session_usable():
    e = _engine("tiny", "bf16", 4)
    st = e.special
    sot, begin, n_lang = _span("tiny")
    V = e.dims.vocab
    tail = [st.transcribe, st.no_timestamps]
    good = [sot, begin + 2] + tail
    opts = e.gen_opts(6, False, suppress_eot=True, check_interval=1)
    clips = [_clip(i) for i in range(3)]
    arm = lambda *a: e.lib.ttasr_session_detect_language(e.h, *a)
    err = lambda: e.lib.ttasr_last_error(e.h)

    assert arm(sot, begin, n_lang) == -1 and b"session" in err()                # no session open
    with e.session(opts, 7) as s:                                               # unarmed
        want, _ = _run(s, lambda s: s.submit(clips, [good] * 3, [4, 5, 6]))
    with e.session(opts, 7) as s:
        with pytest.raises(TtasrError):                                         # the placeholder in an unarmed session
            s.submit(clips[:1], [[sot, DET] + tail])
        for bad in ((sot, begin, 0), (sot, begin, 129), (sot, V - n_lang + 1, n_lang), (sot, -1, n_lang), (-1, begin, n_lang),
                    (V, begin, n_lang)):
            assert arm(*bad) == -1 and len(err()) > 0, bad
        assert arm(sot, begin, n_lang) == 0
        assert arm(sot, begin, n_lang) == -1 and b"already" in err()            # twice
        s.lang_span = (sot, begin, n_lang)
        for bad in ([DET, sot] + tail, [sot, st.transcribe, DET], [sot, DET, sot, DET], [st.sot_prev, DET] + tail):
            with pytest.raises(TtasrError):                                     # not behind sot; twice
                s.submit(clips[:1], [bad])
        assert s.stats()["queued"] == 0
        got, _ = _run(s, lambda s: s.submit(clips, [good, [sot, DET] + tail, good], [4, 5, 6]))
        assert got[1].language is not None and got[0].language is None
        for i in (0, 2):
            _same_decode(got[i], want[i], i)
        assert arm(sot, begin, n_lang) == -1                                    # after a submit (and armed)
    with e.session(opts, 7) as s:
        s.submit(clips[:1], [good], [4])
        assert arm(sot, begin, n_lang) == -1 and b"submit" in err()             # after a submit
        r = s.drain()
        _same_decode(r[0], want[0], "after a refused arming")
    # the plain poll on an armed session returns the usual fields and drops the language
    with e.session(opts, 7, detect_language=True) as s:
        ids = s.submit(clips, [[sot, DET] + tail] * 3, [4, 5, 6])
        got = []
        while s.pending:
            got += s.poll(with_language=False)
        assert sorted(r.id for r in got) == ids and all(r.language is None for r in got)
        by_id = {r.id: r for r in got}
    lang_tok = begin + _armed_language(e, clips[0], (sot, begin, n_lang))
    with e.session(opts, 7) as s:
        r = _run(s, lambda s: s.submit(clips[:1], [[sot, lang_tok] + tail], [4]))[0][0]
    _same_decode(by_id[ids[0]], r, "plain poll")
    e.close()


def _armed_language(e, clip, span):
    opts = e.gen_opts(1, False, suppress_eot=True, check_interval=1)
    with e.session(opts, 2, detect_language=span) as s:
        s.submit([clip], [[span[0], DET]], [1])
        return s.drain()[0].language


# ---- the facade: tiny with the language rows of embed_tokens multiplied by 16 (test_gpu_lang_detect.py's decisive engine) ----
E2E_CLIPS = (1, 2, 5, 6)
E2E_LANGS = [LANGUAGES[94], LANGUAGES[24], LANGUAGES[5], LANGUAGES[24]]
QUIET = dict(temperature=0.0, no_speech_threshold=None, log_prob_threshold=None, compression_ratio_threshold=None,
             max_new_tokens=8, condition_on_previous_text=False)


def _decisive_factory():
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


def _model(compute_type="bfloat16", max_batch=8):
    return WhisperModel("synthetic:tiny", compute_type=compute_type, max_batch=max_batch, _engine_factory=_decisive_factory())


def _no_static_detection(m):
    def boom(*a, **k):
        raise AssertionError("detect_in_session=True must not run a detection pass before the session")
    m.detect_language_batch = boom


@pytest.mark.parametrize("beam_size", [1, 2])
def test_transcribe_stream_detects_in_the_session(beam_size):
    m = _model()
    files = [_clip(i) for i in E2E_CLIPS]
    want_langs = [r[0] for r in m.detect_language_batch(files)]
    assert want_langs == E2E_LANGS
    given = m.transcribe_stream(files, language=E2E_LANGS, max_new_tokens=8, beam_size=beam_size)
    keep = m.detect_language_batch
    _no_static_detection(m)
    auto = m.transcribe_stream(files, language=None, max_new_tokens=8, beam_size=beam_size, detect_in_session=True)
    m.detect_language_batch = keep
    assert auto == given
    assert [l for l, _ in m.last_language_info] == E2E_LANGS
    assert all(0.0 < p <= 1.0 for _, p in m.last_language_info)
    m.close()


def test_transcribe_many_continuous_detects_in_the_session():
    m = _model()
    files = [_clip(i) for i in E2E_CLIPS]
    given = m.transcribe_many(files, language=E2E_LANGS, beam_size=2, continuous=True, **QUIET)
    keep = m.detect_language_batch
    _no_static_detection(m)
    auto = m.transcribe_many(files, language=None, beam_size=2, continuous=True, detect_in_session=True, **QUIET)
    m.detect_language_batch = keep
    assert [info.language for _, info in auto] == E2E_LANGS
    assert [s for s, _ in auto] == [s for s, _ in given]
    for _, info in auto:
        assert 0.0 < info.language_probability <= 1.0 and info.all_language_probs[0] == (info.language, info.language_probability)
    m.close()


def test_transcribe_many_continuous_multilingual_detects_every_window():
    m = _model()
    two = [np.concatenate([_clip(2), _clip(5)]), np.concatenate([_clip(1), _clip(6)])]
    prompts = []
    sub = Session.submit_windows

    def spy(self, files, seeks, prs, *a, **k):
        prompts.extend((int(sk), list(p)) for sk, p in zip(seeks, prs))
        return sub(self, files, seeks, prs, *a, **k)
    Session.submit_windows = spy
    try:
        out = m.transcribe_many(two, language=None, beam_size=2, continuous=True, multilingual=True, without_timestamps=True, **QUIET)
    finally:
        Session.submit_windows = sub
    assert len(out) == 2 and all(DET in p for _, p in prompts)
    n = m.n_window
    for f, (segs, info) in zip(two, out):
        per_window = [r[0] for r in m.detect_language_batch([f[:n], f[n:]])]
        assert info.language == per_window[0]
        assert info.window_languages == per_window, (info.window_languages, per_window)
    assert [info.language for _, info in out] == [LANGUAGES[24], LANGUAGES[94]]
    m.close()
