"""GPU: prompt prefill at a continuous-batching session's admission (option session_prefill, ttasr_session_prefill_stats,
Engine.session(prefill=N)).

A clip whose own prompt has p >= N prefillable positions gets positions 0 .. p - 1 from one admission pass over the packed prompt
rows of the clips admitted together, and its row (beam: group) starts stepping at position p.  What is held here:
  * f32: the tokens of the forced session and of the CPU oracle, sum_logprob within 1e-3, no_speech within rtol 1e-3, the stats;
  * 16 bit: a prefilled clip's bits depend on the clip alone - not on its pass-mates, the number of passes, refill_overlap - and a
    clip below the threshold is bit-identical to the option at 0; the oracle grades the tokens with the session tolerances;
  * pass splitting at the workspace's 512 rows, short audio windows (tile tails, Tk < 64), refusals and untouched paths.

The greedy session knows ONE <|startoftranscript|> index (opts.sot_index) for all its clips; the rule caps a clip's prefill at
min(prompt_len - 1, that index).  Where prompts of different lengths share a greedy session the index is the longest prompt's."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS, SpecialTokens
from taiwan_tongues_asr_ce_amd.engine import Engine, Session, default_suppress, session_prefill_positions

from oracle_checks import Graded, encode_chunked, teacher_forced_causal

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
_cache = {}


def _engine(preset, compute, max_batch, sd=None):
    e = Engine(PRESETS[preset], compute, max_batch)
    e.load_weights(sd.items() if sd is not None else synth.iter_weights(PRESETS[preset]))
    return e


def _prev_prompt(st, rng, n_prev):            # as tests/test_gpu_prefill.py
    prev = rng.integers(300, 20000, size=n_prev).tolist()
    return [st.sot_prev] + prev + [st.sot, st.lang_zh, st.transcribe]


def _rules(e, dims, timestamps=True, suppress_eot=False):
    st = e.special
    r = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                suppress=default_suppress(st, dims.vocab), begin_suppress=[220, st.eot], timestamps=timestamps)
    if suppress_eot:
        r.suppress_eot = True
    return r


def _run(e, opts, clips, prompts, caps=None, prefill=0, beam=1, patience=None, waves=None, overlap=0, detect=False, windows=None):
    """The clips through one session, results in input order: (tokens, sum_logprob, no_speech, stats, languages).
    waves = index lists submitted one after the other with a poll in between; windows = {clip index: (temperature, rows, seed)}
    for clips that go in as window clips of a beam session."""
    n = len(clips)
    caps = [opts.max_new_tokens] * n if caps is None else caps
    waves = [list(range(n))] if waves is None else waves
    if overlap:
        e.set_option("refill_overlap", 1)
    ids, got = {}, []
    try:
        with e.session(opts, max(len(p) for p in prompts), beam=beam, patience=patience, detect_language=detect, prefill=prefill) as s:
            for w, idx in enumerate(waves):
                plain = [i for i in idx if not (windows and i in windows)]
                if plain:
                    for i, cid in zip(plain, s.submit([clips[i] for i in plain], [prompts[i] for i in plain], [caps[i] for i in plain])):
                        ids[cid] = i
                for i in idx:
                    if windows and i in windows:
                        t, rows, seed = windows[i]
                        sot = prompts[i].index(e.special.sot)
                        ids[s.submit_windows([clips[i]], [0], [prompts[i]], [sot], [caps[i]], temperature=[t], rows=[rows], seed=[seed])[0]] = i
                if w + 1 < len(waves):
                    got += s.poll(max_steps=4)
            got += s.drain()
            stats = s.stats()
    finally:
        if overlap:
            e.set_option("refill_overlap", 0)
    assert sorted(ids[r.id] for r in got) == list(range(n))
    toks, lp, ns, lang = [None] * n, np.zeros(n, np.float32), np.zeros(n, np.float32), [None] * n
    for r in got:
        i = ids[r.id]
        toks[i], lp[i], ns[i], lang[i] = r.tokens, r.sum_logprob, r.no_speech_prob, (r.language, r.language_logits)
    return toks, lp, ns, stats, lang


def _same(a, b, idx=None):
    idx = range(len(a[0])) if idx is None else idx
    for i in idx:
        assert a[0][i] == b[0][i], (i, a[0][i], b[0][i])
        assert a[1][i] == b[1][i] and a[2][i] == b[2][i], (i, a[1][i], b[1][i], a[2][i], b[2][i])


# ------------------------------------------------------------------------------------------------ 1. f32 exact, greedy
def test_greedy_f32_equals_the_forced_session_and_the_oracle():
    pd = PRESETS["tiny"]
    dims = R.Dims(**pd.as_dict())
    e = _engine("tiny", COMPUTE_F32, 4)
    st = e.special
    rng = np.random.default_rng(5)
    n_prev = (0, 5, 15, 16, 17, 60)
    clips = [KINDS[i % 3](i) for i in range(6)]
    prompts = [_prev_prompt(st, rng, n) for n in n_prev]
    sot = prompts[-1].index(st.sot)                       # the session's one sot index: the longest prompt's (61)
    N = 8
    opts = e.gen_opts(10, True, sot_index=sot)
    forced = _run(e, opts, clips, prompts)
    pre = _run(e, opts, clips, prompts, prefill=N)
    want_p = [session_prefill_positions(len(p), sot, N) for p in prompts]
    assert want_p == [0, 8, 18, 19, 20, 61]               # one clip below the threshold; the last stops at <|startoftranscript|>
    assert pre[0] == forced[0]
    print("sum_logprob |prefill - forced|", np.abs(pre[1] - forced[1]).tolist(), "no_speech", pre[2].tolist(), forced[2].tolist())
    np.testing.assert_allclose(pre[1], forced[1], atol=1e-3)
    np.testing.assert_allclose(pre[2], forced[2], rtol=1e-3)
    assert pre[1][0] == forced[1][0] and pre[2][0] == forced[2][0]        # the clip that was not prefilled: bit-identical
    W = R.to_torch(synth.state_dict(pd))
    rules = _rules(e, dims)
    enc = R.encoder_forward(torch.from_numpy(np.stack([R.log_mel(c, pd.n_mels) for c in clips])), W, dims)
    for i, p in enumerate(prompts):
        last = i == len(prompts) - 1                      # the only prompt that reaches the session's sot position
        ref = R.greedy_decode(enc[i:i + 1], p, W, dims, rules, 10, no_speech_token=st.no_speech if last else None, sot_index=sot if last else 0)
        assert pre[0][i] == ref.tokens[0], i
        if last:
            np.testing.assert_allclose(pre[2][i], ref.no_speech_prob[0], rtol=1e-3)
    s0, s1 = forced[3], pre[3]
    assert s0["prefill_passes"] == s0["prefill_clips"] == s0["prefill_positions"] == 0
    assert s1["prefill_clips"] == sum(p > 0 for p in want_p) and s1["prefill_positions"] == sum(want_p)
    assert 1 <= s1["prefill_passes"] <= s1["prefill_clips"] and s1["prefill_ms"] > 0
    assert s1["steps"] < s0["steps"], (s1["steps"], s0["steps"])
    assert s1["live_row_steps"] == s0["live_row_steps"] - sum(want_p)
    # the page edges at 16 with each clip's OWN sot index (one session per clip): 16, 17 and 18 prefilled positions
    for i in (2, 3, 4):
        o = e.gen_opts(10, True, sot_index=prompts[i].index(st.sot))
        a, b = _run(e, o, clips[i:i + 1], prompts[i:i + 1]), _run(e, o, clips[i:i + 1], prompts[i:i + 1], prefill=N)
        assert b[3]["prefill_positions"] == n_prev[i] + 1 and a[0] == b[0]
        np.testing.assert_allclose(b[1], a[1], atol=1e-3)
        np.testing.assert_allclose(b[2], a[2], rtol=1e-3)
        ref = R.greedy_decode(enc[i:i + 1], prompts[i], W, dims, rules, 10, no_speech_token=st.no_speech, sot_index=o.sot_index)
        assert b[0][0] == ref.tokens[0]
        np.testing.assert_allclose(b[2], ref.no_speech_prob, rtol=1e-3)
    e.close()


# ------------------------------------------------------------------------------------------------ 2. f32 exact, beam session
def test_beam_session_f32_equals_the_forced_session_and_the_oracle():
    pd = PRESETS["tiny"]
    dims = R.Dims(**pd.as_dict())
    e = _engine("tiny", COMPUTE_F32, 8)
    st = e.special
    rng = np.random.default_rng(9)
    prompts = [_prev_prompt(st, rng, n) for n in (21, 13, 12)]      # 25 tokens (partially filled 2nd page: copy-on-write), 17, 16
    assert [len(p) for p in prompts] == [25, 17, 16]
    clips = [KINDS[i % 3](i) for i in range(3)]
    opts = e.gen_opts(10, True, no_speech=False)
    forced = _run(e, opts, clips, prompts, beam=3, patience=1.0)
    pre = _run(e, opts, clips, prompts, beam=3, patience=1.0, prefill=8)
    assert pre[3]["prefill_clips"] == 3 and pre[3]["prefill_positions"] == 24 + 16 + 15
    assert pre[3]["steps"] < forced[3]["steps"]
    assert pre[0] == forced[0]
    np.testing.assert_allclose(pre[1], forced[1], atol=1e-3)
    W = R.to_torch(synth.state_dict(pd))
    rules = _rules(e, dims)
    enc = R.encoder_forward(torch.from_numpy(np.stack([R.log_mel(c, pd.n_mels) for c in clips])), W, dims)
    for i, p in enumerate(prompts):
        ref = R.beam_decode(enc[i:i + 1], p, W, dims, rules, 3, 10)
        assert pre[0][i] == [t for t in ref.tokens[0] if t != st.eot], i
    # a sampled window clip (temperature 0.6, 3 rows): a ROWS group shares its prefilled prefix the same way
    win = {0: (0.6, 3, 11)}
    a = _run(e, opts, clips[:1], prompts[:1], beam=3, patience=1.0, windows=win)
    b = _run(e, opts, clips[:1], prompts[:1], beam=3, patience=1.0, windows=win, prefill=8)
    assert b[3]["prefill_clips"] == 1 and a[0] == b[0]
    e.close()


# ------------------------------------------------------------------------------------------------ 3 / 4. 16 bit: independence, grading
P16 = (1, 31, 32, 33, 127, 128, 129, 223)     # prefilled positions: the MFMA block edges, the second work item, the longest real prompt
NEW16 = 12


def _world16():
    if "w16" not in _cache:
        pd = PRESETS["large-v3-w2"]
        sd = synth.state_dict(pd)
        clips = [(synth.noise_clip, synth.tonal_clip, synth.noise_clip, synth.burst_clip)[i % 4](300 + i) for i in range(8)]
        _cache["w16"] = (pd, sd, clips)
    return _cache["w16"]


def _prompts16(st):
    rng = np.random.default_rng(21)
    out = [[st.sot, st.no_timestamps]]                                   # 1 position
    out += [_prev_prompt(st, rng, p - 4) + [st.no_timestamps] for p in P16[1:]]
    assert [len(p) - 1 for p in out] == list(P16)
    return out


def _runs16(compute):
    """The runs of tests 3 and 4 for one compute mode, computed once: forced, (a) one submit, (b) two waves reversed, (c) overlap,
    and the option at 200."""
    key = ("runs16", compute)
    if key not in _cache:
        pd, sd, clips = _world16()
        e = _engine("large-v3-w2", compute, 32, sd)
        prompts = _prompts16(e.special)
        opts = e.gen_opts(NEW16, False, suppress_eot=True, sot_index=223)   # every prompt ends at or before position 223
        forced = _run(e, opts, clips, prompts)
        a = _run(e, opts, clips, prompts, prefill=1)
        b = _run(e, opts, clips, prompts, prefill=1, waves=[[7, 6, 5], [4, 3, 2, 1, 0]])
        c = _run(e, opts, clips, prompts, prefill=1, overlap=1)
        d = _run(e, opts, clips, prompts, prefill=200)
        e.close()
        _cache[key] = (prompts, opts, forced, a, b, c, d)
    return _cache[key]


@pytest.mark.parametrize("compute", [COMPUTE_BF16, COMPUTE_F16], ids=["bf16", "f16"])
def test_a_prefilled_clip_does_not_depend_on_its_pass_mates(compute):
    prompts, opts, forced, a, b, c, d = _runs16(compute)
    assert a[3]["prefill_clips"] == 8 and a[3]["prefill_positions"] == sum(P16) and a[3]["prefill_passes"] >= 2   # 904 rows > 512
    assert b[3]["prefill_clips"] == 8 and b[3]["prefill_passes"] >= 2
    assert a[3]["steps"] < forced[3]["steps"]
    assert all(len(t) == NEW16 for t in a[0]) and np.isfinite(a[1]).all()
    _same(a, b)
    _same(a, c)
    # the option at 200: only the 223-position clip is prefilled - it equals run (a), the others the option at 0, bit for bit
    assert d[3]["prefill_clips"] == 1 and d[3]["prefill_positions"] == 223
    _same(d, forced, idx=range(7))
    _same(d, a, idx=[7])


@pytest.mark.parametrize("compute", [COMPUTE_BF16, COMPUTE_F16], ids=["bf16", "f16"])
def test_the_oracle_grades_prefilled_clips_like_forced_ones(compute):
    pd, sd, clips = _world16()
    prompts, opts, forced, a = _runs16(compute)[:4]
    rd = R.Dims(**pd.as_dict())
    W = R.to_torch(sd, round_bf16=compute == COMPUTE_BF16, round_f16=compute == COMPUTE_F16)
    if "mel16" not in _cache:
        _cache["mel16"] = np.stack([R.log_mel(c, pd.n_mels) for c in clips])
    enc_ref = encode_chunked(_cache["mel16"], W, rd)
    st = SpecialTokens.for_vocab(pd.vocab)
    rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                    suppress=default_suppress(st, pd.vocab), begin_suppress=[220, st.eot], timestamps=False)
    rules.suppress_eot = True
    worst = {}
    for name, run in (("prefilled", a), ("forced", forced)):
        g = Graded()
        for i in range(8):
            g.add(teacher_forced_causal([run[0][i]], prompts[i], enc_ref[i:i + 1], W, rd, rules, tol=0.15, margin=0.16, rows_per_pass=1))
        assert g.n_steps == 8 * NEW16
        assert g.n_clear >= 0.6 * g.n_steps, (name, g.n_clear, g.n_steps)     # held to token equality, not only to the tolerance
        worst[name] = g.worst
    print("Graded.worst", worst)
    # the record: one line per compute mode, replaced by every run
    out = os.path.join(ROOT, "profiles", "session_prefill_grading.jsonl")
    name = "bf16" if compute == COMPUTE_BF16 else "f16"
    try:
        old = [json.loads(l) for l in open(out)] if os.path.exists(out) else []
        rows = [r for r in old if r.get("compute") != name]
        rows.append({"geometry": "large-v3-w2", "compute": name, "positions": list(P16), "new_tokens": NEW16, "tol": 0.15, "margin": 0.16,
                     "worst": worst})
        with open(out, "w") as f:
            for r in sorted(rows, key=lambda r: r["compute"]):
                f.write(json.dumps(r) + "\n")
    except OSError:
        pass                                   # a read-only checkout still grades


# ------------------------------------------------------------------------------------------------ 5. pass splitting, the longest prompt
def test_pass_splitting_and_the_longest_prompt_bf16():
    pd, sd, clips = _world16()
    e = _engine("large-v3-w2", COMPUTE_BF16, 32, sd)
    st = e.special
    rng = np.random.default_rng(33)
    long_p = [_prev_prompt(st, rng, 446 - 4) + [st.no_timestamps] for _ in range(2)]
    prompts = long_p + [_prev_prompt(st, rng, 223 - 4) + [st.no_timestamps]]
    assert [len(p) - 1 for p in prompts] == [446, 446, 223] and len(long_p[0]) == pd.n_text_ctx - 1
    opts = e.gen_opts(NEW16, False, suppress_eot=True, no_speech=False)
    alone = [_run(e, opts, clips[i:i + 1], prompts[i:i + 1], prefill=1) for i in range(3)]
    both = _run(e, opts, clips[:3], prompts, prefill=1)
    assert both[3]["prefill_positions"] == 1115 and both[3]["prefill_passes"] == 3     # 446 | 446 | 223: whole sequences, <= 512 rows each
    for i in range(3):
        assert alone[i][3]["prefill_passes"] == 1
        assert both[0][i] == alone[i][0][0] and both[1][i] == alone[i][1][0], i
    assert [len(t) for t in both[0]] == [1, 1, NEW16]              # the budget is clamped to n_text_ctx - prompt_len
    e.close()


# ------------------------------------------------------------------------------------------------ 6. short audio windows
@pytest.mark.parametrize("n_ctx", [150, 20])
def test_short_audio_windows_bf16(n_ctx):
    pd, sd, _ = _world16()
    e = _engine("large-v3-w2", COMPUTE_BF16, 32, sd)
    st = e.special
    e.set_audio_ctx(n_ctx)
    clip = synth.noise_clip(90, n_ctx * 320)
    prompt = _prev_prompt(st, np.random.default_rng(40), 40 - 4) + [st.no_timestamps]
    opts = e.gen_opts(NEW16, False, suppress_eot=True, no_speech=False)
    got = _run(e, opts, [clip], [prompt], prefill=1)
    assert got[3]["prefill_positions"] == 40 and len(got[0][0]) == NEW16
    rd = R.Dims(**pd.as_dict())
    W = R.to_torch(sd, round_bf16=True)
    mel = R.log_mel(clip, pd.n_mels, n_samples=n_ctx * 320)[None]
    enc_ref = R.encoder_forward(torch.from_numpy(mel), W, rd)
    assert enc_ref.shape[1] == n_ctx
    rules = _rules(e, pd, timestamps=False, suppress_eot=True)
    g = teacher_forced_causal([got[0][0]], prompt, enc_ref, W, rd, rules, tol=0.15, margin=0.16, rows_per_pass=1)
    print("audio_ctx", n_ctx, "Graded.worst", g.worst, "clear", g.n_clear, "of", g.n_steps)
    assert g.n_steps == NEW16 and g.n_clear >= 0.6 * g.n_steps, (g.n_clear, g.n_steps)
    e.set_audio_ctx(0)
    e.close()


# ------------------------------------------------------------------------------------------------ 6b. the numbers behind a prefilled prefix
# The grading above holds tokens; with these weights a token survives large errors of the prompt's cross-attention (a dropped key
# tile, an unmasked tile tail, a second work item on another slot move sum_logprob by 1 ... 9 and leave every token in place).  So
# the NUMBERS of a prefilled clip are held to the forced 16-bit session of the same clip: same weights, same steps after the
# prompt, only the prompt's K / V come from the pass (tiled GEMM family, MFMA cross-attention) instead of forced steps (K-split
# GEMMs, per-row cross-attention).  The two paths differ by 16-bit rounding of the prompt's K / V only.  The bound is the logit
# tolerance this project holds a 16-bit engine to at this geometry (tests/test_gpu_session_lang.py _tol: bf16 0.08, fp16 0.02):
#   * no_speech is one softmax value of a real <|startoftranscript|> step BEHIND the prefilled prefix: a logit error of tol on the
#     token and on the normaliser moves ln(no_speech) by at most 2 tol;
#   * sum_logprob adds NEW16 token log-probabilities, each off by that much at most and with independent signs: sqrt(NEW16) tol
#     (bf16 0.28, fp16 0.07) - several times below the 1.1 the mildest of the errors above costs.
# Shapes: 1500 keys (23 tiles + 28 keys) with 129 prefilled positions = two work items, the second of one row; 150 keys (two
# tiles + 22) and 20 keys (Tk < 64) with 40 positions.
TOL16 = {COMPUTE_BF16: 0.08, COMPUTE_F16: 0.02}


@pytest.mark.parametrize("n_ctx,n_pos", [(0, 129), (150, 40), (20, 40)], ids=["Tk1500", "Tk150", "Tk20"])
@pytest.mark.parametrize("compute", [COMPUTE_BF16, COMPUTE_F16], ids=["bf16", "f16"])
def test_numbers_behind_a_prefilled_prefix_agree_with_the_forced_session(compute, n_ctx, n_pos):
    pd, sd, _ = _world16()
    e = _engine("large-v3-w2", compute, 32, sd)
    st = e.special
    e.set_audio_ctx(n_ctx)
    n_keys = n_ctx or pd.n_audio_ctx
    clip = synth.noise_clip(91, n_keys * 320)
    prompt = _prev_prompt(st, np.random.default_rng(60 + n_pos), n_pos - 1) + [st.no_timestamps]
    sot = prompt.index(st.sot)
    assert sot == n_pos
    opts = e.gen_opts(NEW16, False, suppress_eot=True, sot_index=sot)          # no-speech wanted: the prefill stops at sot
    forced = _run(e, opts, [clip], [prompt])
    pre = _run(e, opts, [clip], [prompt], prefill=1)
    e.set_audio_ctx(0)
    e.close()
    assert pre[3]["prefill_positions"] == n_pos and pre[3]["steps"] < forced[3]["steps"]
    tol = TOL16[compute]
    d_lp = abs(float(pre[1][0]) - float(forced[1][0]))
    d_ns = abs(float(np.log(pre[2][0])) - float(np.log(forced[2][0])))
    print(f"keys {n_keys} positions {n_pos}: sum_logprob {pre[1][0]:.5f} / {forced[1][0]:.5f} (|d| {d_lp:.5f}, bound {np.sqrt(NEW16) * tol:.3f}); "
          f"no_speech {pre[2][0]:.6e} / {forced[2][0]:.6e} (|d ln| {d_ns:.5f}, bound {2 * tol:.3f})")
    assert pre[0] == forced[0], (pre[0], forced[0])
    assert 0.0 < pre[2][0] < 1.0 and 0.0 < forced[2][0] < 1.0
    assert d_ns <= 2 * tol, d_ns
    assert d_lp <= np.sqrt(NEW16) * tol, d_lp


# ------------------------------------------------------------------------------------------------ 7. refusals and untouched paths
def test_refusals_and_untouched_paths():
    pd, sd, clips = _world16()
    e = _engine("large-v3-w2", COMPUTE_BF16, 32, sd)
    st = e.special
    for bad in (-1, pd.n_text_ctx - 1):
        assert e.lib.ttasr_set_option(e.h, b"session_prefill", bad) == -1
    assert e.lib.ttasr_set_option(e.h, b"session_prefill", pd.n_text_ctx - 2) == 0
    assert e.lib.ttasr_set_option(e.h, b"session_prefill", 0) == 0
    out4 = (ctypes.c_double * 4)()
    assert e.lib.ttasr_session_prefill_stats(e.h, out4) == -1               # no session is open
    rng = np.random.default_rng(50)
    long_p = _prev_prompt(st, rng, 60) + [st.no_timestamps]
    short_p = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(NEW16, False, suppress_eot=True, no_speech=False)
    with e.session(opts, len(long_p), prefill=4) as s:
        assert e.lib.ttasr_set_option(e.h, b"session_prefill", 8) == -1      # refused like every option while a session is open
        assert e.lib.ttasr_session_prefill_stats(e.h, None) == -1
        assert s.submit(clips[:1], [short_p]) == [0] and len(s.drain()) == 1  # the refusals changed nothing
    # a placeholder clip in an armed session is never prefilled; its results do not see the prefilled neighbour of its admission
    det_p = [st.sot_prev] + rng.integers(300, 20000, size=20).tolist() + [st.sot, Session.DETECT, st.transcribe, st.no_timestamps]
    base = _run(e, opts, clips[:2], [det_p, long_p], detect=True)
    mixed = _run(e, opts, clips[:2], [det_p, long_p], detect=True, prefill=4)
    assert mixed[3]["prefill_clips"] == 1 and mixed[3]["prefill_positions"] == len(long_p) - 1
    _same(mixed, base, idx=[0])
    assert mixed[4][0][0] == base[4][0][0] and np.array_equal(mixed[4][0][1], base[4][0][1])
    # xkv_fp8 = 2: the pass reads the 16-bit live slot; the clip is graded like the others
    e.set_option("xkv_fp8", 2)
    fp8 = _run(e, opts, clips[1:2], [long_p], prefill=4)
    e.set_option("xkv_fp8", 0)
    assert fp8[3]["prefill_clips"] == 1
    rd = R.Dims(**pd.as_dict())
    W = R.to_torch(sd, round_bf16=True)
    enc_ref = encode_chunked(np.stack([R.log_mel(clips[1], pd.n_mels)]), W, rd)
    g = teacher_forced_causal([fp8[0][0]], long_p, enc_ref, W, rd, _rules(e, pd, timestamps=False, suppress_eot=True),
                              tol=0.15, margin=0.16, rows_per_pass=1)
    print("xkv_fp8 = 2: Graded.worst", g.worst, "clear", g.n_clear, "of", g.n_steps)
    assert g.n_steps == NEW16 and g.n_clear >= 0.6 * g.n_steps, (g.n_clear, g.n_steps)
    # a session after the prefilled ones, the option back at 0, equals a fresh engine's
    after = _run(e, opts, clips[:2], [long_p, short_p])
    assert after[3]["prefill_passes"] == 0
    f = _engine("large-v3-w2", COMPUTE_BF16, 32, sd)
    _same(after, _run(f, opts, clips[:2], [long_p, short_p]))
    f.close()
    e.close()
