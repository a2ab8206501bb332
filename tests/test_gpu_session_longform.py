"""GPU: long-form windows and independent rows in the beam session (ttasr_session_submit_windows, Session.submit_windows,
WhisperModel.transcribe_many(continuous=True)).

A window clip's log-mel is ttasr_log_mel_windows' for the same (file, seek, floor_max); a group decodes it by beam search
(temperature 0, rows > 1) or as independent rows (session_rows_select_kernel: greedy, or best_of Gumbel-max samples keyed by
the row's index in its group).  So each clip must equal, bit for bit (tokens, sum_logprob, no_speech), its static counterpart
on the same context with prefill = 0 and enc_gemm = 3: a ttasr_generate_beam pass of G windows built with log_mel_windows
(ragged previous-text prompts, per-window sot indices), slot 0 of a ttasr_generate_sample pass of G windows with best_of = 5
and the same seed, and, for plain clips, a ttasr_generate_beam pass of G clips.

Geometry: large-v3-w2, max_batch 30, beam 5 (G = 6).  The EOT row of the token embedding is scaled (test_gpu_session_beam) so
that hypotheses finish at spread positions."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS, SpecialTokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DIMS = PRESETS["large-v3-w2"]
B = 30
BEAM = 5
G = B // BEAM
N_NEW = 40
COMPUTES = [(COMPUTE_F32, "f32"), (COMPUTE_BF16, "bf16"), (COMPUTE_F16, "f16")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _files():
    a = np.concatenate([synth.noise_clip(400), synth.tonal_clip(401), synth.burst_clip(402)[:160000]])   # 70 s: 7000 frames
    b = np.concatenate([synth.tonal_clip(403), synth.noise_clip(404)[:288000]])                           # 48 s: 4800 frames
    return a.astype(np.float32), b.astype(np.float32)


@pytest.fixture(scope="module")
def state():
    sd = dict(synth.state_dict(DIMS))
    st = SpecialTokens.for_vocab(DIMS.vocab)
    e = sd["model.decoder.embed_tokens.weight"].copy()
    e[st.eot] *= 5.0
    sd["model.decoder.embed_tokens.weight"] = e
    return sd


def _engine(compute, sd):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, compute, B)
    e.load_weights(sd.items())
    return e


def _floor(e, f):
    _, mx = e.log_mel_windows(f, list(range(0, len(f) // 160, 3000)), want_max=True)
    return float(np.max(mx))


def _windows(e):
    """Six windows of two files (seeks 0, 3000 and the ragged 1000-frame tail of the 70-s file; 0, 2500 and the 800-frame tail
    of the 48-s one), each with its own previous-text prompt length and sot index."""
    a, b = _files()
    st = e.special
    files, seeks = [a, a, a, b, b, b], [0, 3000, 6000, 0, 2500, 4000]
    prompts, sots = [], []
    for k in range(6):
        prev = [st.sot_prev] + [1000 + 37 * j for j in range(4 * k)] if k else []
        prompts.append(prev + [st.sot, st.lang_zh, st.transcribe, st.no_timestamps])
        sots.append(len(prev))
    floors = {id(a): _floor(e, a), id(b): _floor(e, b)}
    return files, seeks, prompts, sots, [floors[id(f)] for f in files]


def _static_opts(e, max_new=N_NEW, sot=0):
    return e.gen_opts(max_new, timestamps=False, sot_index=sot)


def _static(e, fn):
    e.set_option("prefill", 0)
    e.set_option("enc_gemm", 3)
    try:
        return fn()
    finally:
        e.set_option("prefill", 1)
        e.set_option("enc_gemm", 0)


def _reference(e):
    """Static counterparts: the six beam windows (one ragged pass), two sampled windows (slot 0 of a pass each), six plain clips."""
    files, seeks, prompts, sots, floors = _windows(e)
    out = {}

    def run():
        e.log_mel_windows(files, seeks, floor_max=floors)
        e.encode(G)
        r = e.generate_beam(prompts, BEAM, _static_opts(e), 1.0, sot_index=sots)
        out["beam"] = (r.tokens, np.asarray(r.sum_logprob), np.asarray(r.no_speech_prob))
        for k, (w, temp) in enumerate([(1, 0.2), (4, 1.0)]):
            order = [w] + [i for i in range(6) if i != w]
            e.log_mel_windows([files[i] for i in order], [seeks[i] for i in order], floor_max=[floors[i] for i in order])
            e.encode(G)
            r = e.generate_sample([prompts[w]] * G, BEAM, _static_opts(e, sot=sots[w]), temp, seed=1234 + k)
            out[f"sample{k}"] = (r.tokens[0], float(r.sum_logprob[0]), float(r.no_speech_prob[0]))
        clips = [synth.noise_clip(410 + i)[: 160000 + 40000 * i] for i in range(G)]
        pr = [e.special.sot, e.special.lang_zh, e.special.transcribe, e.special.no_timestamps]
        e.log_mel(clips, want_output=False)
        e.encode(G)
        r = e.generate_beam([pr] * G, BEAM, _static_opts(e), 1.0)
        out["plain"] = (clips, pr, r.tokens, np.asarray(r.sum_logprob), np.asarray(r.no_speech_prob))
        return out
    return _static(e, run), (files, seeks, prompts, sots, floors)


def _session(e, win, ref, overlap):
    files, seeks, prompts, sots, floors = win
    clips, pr, *_ = ref["plain"]
    e.set_option("refill_overlap", overlap)
    try:
        with e.session(_static_opts(e), 64, beam=BEAM, patience=1.0) as s:
            beam_ids = s.submit_windows(files, seeks, prompts, sots, floor_max=floors, rows=[BEAM] * 6)
            sample_ids = s.submit_windows([files[1], files[4]], [seeks[1], seeks[4]], [prompts[1], prompts[4]], [sots[1], sots[4]],
                                          floor_max=[floors[1], floors[4]], temperature=[0.2, 1.0], rows=[BEAM, BEAM],
                                          seed=[1234, 1235])
            plain_ids = s.submit(clips, [pr] * G)
            got = {r.id: r for r in s.drain()}
            stats = s.stats()
    finally:
        e.set_option("refill_overlap", 0)
    return [got[i] for i in beam_ids], [got[i] for i in sample_ids], [got[i] for i in plain_ids], stats


@pytest.mark.parametrize("compute,name", COMPUTES)
def test_window_sampled_and_plain_clips_equal_their_static_passes(state, compute, name):
    e = _engine(compute, state)
    try:
        ref, win = _reference(e)
        for overlap in ((0, 1) if compute == COMPUTE_F32 else (0,)):
            beam, sampled, plain, stats = _session(e, win, ref, overlap)
            toks, lp, ns = ref["beam"]
            for i, r in enumerate(beam):
                assert r.tokens == toks[i], (name, overlap, "window", i)
                assert np.float32(r.sum_logprob) == lp[i] and np.float32(r.no_speech_prob) == ns[i], (name, overlap, "window", i)
            for k, r in enumerate(sampled):
                t, l, n = ref[f"sample{k}"]
                assert r.tokens == t and np.float32(r.sum_logprob) == np.float32(l), (name, overlap, "sample", k)
                assert np.float32(r.no_speech_prob) == np.float32(n), (name, overlap, "sample", k)
            _, _, ptoks, plp, pns = ref["plain"]
            for i, r in enumerate(plain):
                assert r.tokens == ptoks[i] and np.float32(r.sum_logprob) == plp[i] and np.float32(r.no_speech_prob) == pns[i]
            assert stats["live_row_steps"] > 0
        assert len({len(p) for p in win[2]}) == 6 and len(set(win[3])) == 6   # ragged prompts, six sot indices
    finally:
        e.close()


def test_continuous_transcribe_many_reproduces_hf_long_form_on_the_gpu():
    from test_longform_golden import recording
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    with open(os.path.join(GOLDEN, "longform.json")) as f:
        golden = json.load(f)
    audio_seconds = golden["n_samples"] / 16000.0
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=2)
    try:
        for name in ("cond_prev_48", "no_cond_48"):
            case = golden["cases"][name]
            kw = case["options"]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                (segs, _), = m.transcribe_many([recording()], language="zh", beam_size=1, temperature=0.0,
                                               condition_on_previous_text=kw["condition_on_prev_tokens"],
                                               max_new_tokens=kw["max_new_tokens"], no_speech_threshold=None,
                                               log_prob_threshold=None, compression_ratio_threshold=None, continuous=True)
            want = [h for h in case["segments"] if h["start"] < audio_seconds]
            assert len(segs) == len(want) >= 7, name
            seeks = set()
            for s, h in zip(segs, want):
                assert s.tokens in (h["tokens"], h["tokens"][:-1]), (name, s.tokens, h["tokens"])
                assert abs(s.start - h["start"]) < 1e-6
                assert abs(s.end - min(h["end"], audio_seconds)) < 1e-6
                seeks.add(s.seek)
            assert len(seeks) == 3 and min(seeks) == 0
    finally:
        m.close()


def test_continuous_results_do_not_depend_on_file_order_or_overlap(monkeypatch):
    from taiwan_tongues_asr_ce_amd import engine as engine_mod
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    attempts = []
    submit = engine_mod.Session.submit_windows

    def counting(self, *a, **kw):
        attempts.extend(kw.get("temperature") or [0.0])
        return submit(self, *a, **kw)
    monkeypatch.setattr(engine_mod.Session, "submit_windows", counting)
    files = [np.concatenate([synth.noise_clip(420 + i), synth.tonal_clip(430 + i)[: 80000 * (i % 4 + 1)]]).astype(np.float32)
             for i in range(8)]
    # every attempt fails the log-prob threshold 0: each window walks the whole ladder in the session
    kw = dict(language="zh", beam_size=5, best_of=5, temperature=(0.0, 0.4, 0.8), max_new_tokens=12, log_prob_threshold=0.0,
              no_speech_threshold=None)
    m = WhisperModel("synthetic:large-v3-w2", device="cuda", compute_type="bfloat16", max_batch=B)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = [segs for segs, _ in m.transcribe_many(files, continuous=True, **kw)]
            b = [segs for segs, _ in m.transcribe_many(files[::-1], continuous=True, **kw)][::-1]
            m.engine.set_option("refill_overlap", 1)
            try:
                c = [segs for segs, _ in m.transcribe_many(files, continuous=True, **kw)]
            finally:
                m.engine.set_option("refill_overlap", 0)
        assert a == b == c
        assert sum(len(s) for s in a) > 0
        n_windows = 3 * sum(len({seg.seek for seg in segs}) for segs in a)
        assert len(attempts) >= 3 * n_windows and attempts.count(0.8) == attempts.count(0.4) == attempts.count(0.0)
    finally:
        m.close()
