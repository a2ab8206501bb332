"""GPU: the sequence-bias logits processor end to end - tiny synthetic model, one 12-s clip, one window.

The reference is the oracle's own greedy_decode / beam_decode / sample_decode with apply_rules wrapped here: the wrapper adds the
restated bias (tests/seq_bias_cases.py reference, pinned to HF by tests/test_seq_bias_reference_host.py), computed from prompt +
sampled, in front of the rules.  Every parametrisation builds a table that must change the output: with the plain tokens g and
the first position i >= 1 whose bigram (g[i-1], g[i]) is new in the history, the sequences (g[i-1], g[i], x) and (g[i], x, y)
with bias 1e4 turn the continuation into x, y (x != g[i+1] a text token, y a token the rules allow); the test checks on the CPU
that the reference with the table differs from the one without.  f32 engine: tokens equal the reference's for greedy, beam 3 and
temperature 0.4 with best_of 2, the greedy sum_logprob within test_gpu_parity's 2e-3 * 20.  bf16 / fp16 engines: the engine's own
plain run up to i, then x, y."""
import numpy as np
import pytest
import torch

import seq_bias_cases as S
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import seq_bias, synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MAX_NEW = 16     # with the 4-token prompt the histories outgrow the 16 tokens a match can need
BIAS = 1e4
CLIP = lambda: synth.noise_clip(11, 12 * 16000)   # noqa: E731


def _engine(compute, max_batch=4):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(PRESETS["tiny"], compute, max_batch)
    e.load_weights(synth.iter_weights(PRESETS["tiny"]))
    e.log_mel([CLIP()], want_output=False)
    e.encode(1)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine(COMPUTE_F32)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle():
    dims = R.Dims(**PRESETS["tiny"].as_dict())
    W = R.to_torch(synth.state_dict(PRESETS["tiny"]))
    enc = R.encoder_forward(torch.from_numpy(R.log_mel(CLIP(), 80)[None]), W, dims)
    return dims, W, enc


def setup(e):
    """prompt, engine options and oracle rules of the run: no timestamps, EOT suppressed so that every run has MAX_NEW tokens"""
    st = e.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(MAX_NEW, False, suppress_eot=True, sot_index=0)
    rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                    suppress=[opts.suppress[i] for i in range(opts.n_suppress)], begin_suppress=[220, st.eot], timestamps=False,
                    suppress_eot=True)
    return prompt, opts, rules


def build_table(prompt, g, rules, salt=0):
    """-> (i, x, y, table) for the plain tokens g, as the module docstring says; salt picks other x, y"""
    hist = list(prompt) + list(g)
    p = len(prompt)
    seen, i = set(), None
    for k in range(1, len(hist)):
        if k - p >= 1 and (hist[k - 1], hist[k]) not in seen:
            i = k - p
            break
        seen.add((hist[k - 1], hist[k]))
    assert i is not None and i + 1 < len(g), (i, g)
    banned = set(rules.suppress) | {rules.eot, rules.no_timestamps, 220, g[i + 1]}
    text = [t for t in range(1000 + 37 * salt, rules.eot) if t not in banned]
    x, y = text[0], text[1]
    return i, x, y, [((g[i - 1], g[i], x), BIAS), ((g[i], x, y), BIAS)]


def with_bias(monkeypatch, prompt, table):
    """oracle.apply_rules with the restated bias in front of it"""
    plain = R.apply_rules

    def biased(logits, sampled, rules, *a, **k):
        row = S.reference(logits.float().numpy()[None], [list(prompt) + list(sampled)], table)[0]
        return plain(torch.from_numpy(row), sampled, rules, *a, **k)
    monkeypatch.setattr(R, "apply_rules", biased)


def test_greedy_f32_equals_the_biased_oracle(eng, oracle, monkeypatch):
    dims, W, enc = oracle
    prompt, opts, rules = setup(eng)
    plain = R.greedy_decode(enc, prompt, W, dims, rules, MAX_NEW)
    g = plain.tokens[0]
    i, x, y, table = build_table(prompt, g, rules)
    with_bias(monkeypatch, prompt, table)
    ref = R.greedy_decode(enc, prompt, W, dims, rules, MAX_NEW)
    assert ref.tokens[0] != g and ref.tokens[0][:i + 3] == g[:i + 1] + [x, y]
    base = eng.generate([prompt], opts)            # this context has never had a table
    assert base.tokens[0] == g
    eng.set_sequence_bias(dict(table))
    res = eng.generate([prompt], opts)
    assert res.tokens[0] == ref.tokens[0]
    np.testing.assert_allclose(res.sum_logprob, ref.sum_logprob, atol=2e-3 * 20)
    # replacing the table between two calls takes effect, graphs on (the step graphs of the call above are replayed)
    i2, x2, y2, table2 = build_table(prompt, g, rules, salt=1)
    assert (x2, y2) != (x, y)
    eng.set_sequence_bias(dict(table2))
    assert eng.generate([prompt], opts).tokens[0][:i2 + 3] == g[:i2 + 1] + [x2, y2]
    # sessions are refused while a table is installed, and the context stays usable
    with pytest.raises(Exception, match="sequence-bias table is installed"):
        eng.session(opts, len(prompt))
    with pytest.raises(Exception, match="sequence-bias table is installed"):
        eng.session(opts, len(prompt), beam=2)
    assert eng.generate([prompt], opts).tokens[0][:i2 + 3] == g[:i2 + 1] + [x2, y2]
    # cleared: bit-identical to the run before the context ever had a table, and sessions open again
    eng.set_sequence_bias(None)
    again = eng.generate([prompt], opts)
    assert again.tokens == base.tokens and np.array_equal(again.sum_logprob.view(np.uint32), base.sum_logprob.view(np.uint32))
    assert np.array_equal(again.no_speech_prob.view(np.uint32), base.no_speech_prob.view(np.uint32))
    with eng.session(opts, len(prompt)):
        pass
    eng.log_mel([CLIP()], want_output=False)      # the session rewrote the encoder state
    eng.encode(1)


def test_beam_f32_equals_the_biased_oracle(eng, oracle, monkeypatch):
    dims, W, enc = oracle
    prompt, opts, rules = setup(eng)
    g = R.beam_decode(enc, prompt, W, dims, rules, 3, MAX_NEW).tokens[0]
    i, x, y, table = build_table(prompt, g, rules)
    with_bias(monkeypatch, prompt, table)
    ref = R.beam_decode(enc, prompt, W, dims, rules, 3, MAX_NEW)
    assert ref.tokens[0] != g and ref.tokens[0][:i + 3] == g[:i + 1] + [x, y]
    base = eng.generate_beam([prompt], 3, opts)
    assert base.tokens[0] == g
    eng.set_sequence_bias(dict(table))
    try:
        res = eng.generate_beam([prompt], 3, opts)
    finally:
        eng.set_sequence_bias(None)
    assert res.tokens[0] == ref.tokens[0]
    again = eng.generate_beam([prompt], 3, opts)
    assert again.tokens == base.tokens and np.array_equal(again.sum_logprob.view(np.uint32), base.sum_logprob.view(np.uint32))


def test_sampled_f32_equals_the_biased_oracle(eng, oracle, monkeypatch):
    dims, W, enc = oracle
    prompt, opts, rules = setup(eng)
    T, seed = 0.4, 7
    g = R.sample_decode(enc, prompt, W, dims, rules, 2, T, seed, MAX_NEW).tokens[0]
    i, x, y, table = build_table(prompt, g, rules)
    with_bias(monkeypatch, prompt, table)
    ref = R.sample_decode(enc, prompt, W, dims, rules, 2, T, seed, MAX_NEW)
    assert ref.tokens[0] != g
    assert eng.generate_sample([prompt], 2, opts, T, seed).tokens[0] == g
    eng.set_sequence_bias(dict(table))
    try:
        res = eng.generate_sample([prompt], 2, opts, T, seed)
    finally:
        eng.set_sequence_bias(None)
    assert res.tokens[0] == ref.tokens[0]


@pytest.mark.parametrize("compute", [COMPUTE_BF16, COMPUTE_F16], ids=["bf16", "fp16"])
def test_sixteen_bit_engines_turn_where_the_table_says(compute):
    e = _engine(compute)
    try:
        prompt, opts, rules = setup(e)
        g = e.generate([prompt], opts).tokens[0]
        i, x, y, table = build_table(prompt, g, rules)
        e.set_sequence_bias(dict(table))
        got = e.generate([prompt], opts).tokens[0]
        assert got[:i + 3] == g[:i + 1] + [x, y], (got, g, i, x, y)
        e.set_sequence_bias(None)
        assert e.generate([prompt], opts).tokens[0] == g
        plain_beam = e.generate_beam([prompt], 2, opts).tokens[0]
        ib, xb, yb, tb = build_table(prompt, plain_beam, rules)
        e.set_sequence_bias(dict(tb))
        assert e.generate_beam([prompt], 2, opts).tokens[0][:ib + 3] == plain_beam[:ib + 1] + [xb, yb]
    finally:
        e.close()


def test_transcribe_prompt_words_installs_the_expected_table_and_clears_it():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=2)
    try:
        calls = []
        real = m.engine.set_sequence_bias

        def spy(mapping=None):
            calls.append(None if mapping is None else list(mapping))
            return real(mapping)
        m.engine.set_sequence_bias = spy
        words, boost = "台北, Kaohsiung", 3.0
        segs, _ = m.transcribe(CLIP(), language="zh", beam_size=1, temperature=0.0, prompt_words=words, prompt_word_boost=boost)
        assert calls == []                       # nothing is installed before the segments are produced
        list(segs)
        enc = m.tokenizer.encode
        want = {}
        for p in ("台北", "Kaohsiung"):
            for ids in {tuple(enc(p)), tuple(enc(" " + p))}:
                ids = ids[:16]
                want[ids[:1]] = max(want.get(ids[:1], boost / 2), boost / 2)
                for k in range(2, len(ids) + 1):
                    want[ids[:k]] = boost
        assert len(calls) == 2 and calls[1] is None
        assert dict(calls[0]) == want and len(calls[0]) == len(want)
        # and the library holds exactly that table: a probe row with an empty history shows the length-1 halves alone
        real(calls[0])
        raw = np.zeros((1, m.dims.vocab), np.float32)
        got, _ = m.engine.seq_bias_probe("window", raw, hist=np.full((1, 15), -1, np.int32), hist_len=[0])
        S.same(got, S.reference(raw, [[]], seq_bias.check_table(want, m.dims.vocab)), raw)
        assert np.count_nonzero(got) == sum(1 for k in want if len(k) == 1)
        real(None)
        with pytest.raises(ValueError, match="lock-step"):
            m.transcribe_many([CLIP()], language="zh", continuous=True, prompt_words=words)
        with pytest.raises(ValueError, match="lock-step"):
            m.transcribe_stream([CLIP()], prompt_words=words)
    finally:
        m.close()
