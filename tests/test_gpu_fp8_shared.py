"""GPU: option xkv_fp8 = 2 in static passes - rows that share a clip's cross-KV (the hypotheses of a beam, the rows of a sampled
attempt) read the e4m3 copy through cross_attn_mq_fp8_kernel (kernels_fp8.hip).

Two bf16 engines on preset large-v3-w2 (20 heads, 2 + 2 layers): e16 (option 0) and e8 (option 2).  The fp8 engine is graded
against the 16-bit engine it approximates:
  * liveness: its beam scores differ from e16's in at least one clip (f32 sums of log-probs: any e4m3 read moves them);
  * reproducibility: a second call is bit-identical (no atomics);
  * agreement: at least half of the clips return e16's tokens (the share test_gpu_fp8.py requires of greedy rows), and for those
    |delta sum_logprob| <= 0.24 x (len + 1): equal histories with logits within eps give log-probabilities within 2 eps per
    scored position, eps = 0.12 being the bound test_gpu_fp8.py holds the same e4m3 copy to on this preset;
  * A/B: with xattn_mq_fp8 = 0, and after xkv_fp8 = 0 plus a fresh encode, e8 equals e16 bit for bit.
Shapes: every instantiation the dispatch reaches in the suite's budget (NQ = 2, 5, 7), one slice (direct store), 4 and 8
slices, the clamped tail of a short audio window, and 200 (row, head) items, which stay on the 16-bit frame-split kernels.
The EOT row of the token embedding is scaled (as in test_gpu_session_beam.py) so that hypotheses and sampled rows end at spread
positions and the finished-group exit is exercised."""
import numpy as np
import pytest
import torch

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F32, PRESETS, SpecialTokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DIMS = PRESETS["large-v3-w2"]
N_NEW = 12
EPS = 0.12   # logit bound of the e4m3 copy on this preset (test_gpu_fp8.py)


def _clips(n, seed=300, samples=None):
    kinds = (synth.noise_clip, synth.tonal_clip, synth.noise_clip, synth.burst_clip)
    return [kinds[i % 4](seed + i) if samples is None else kinds[i % 4](seed + i, samples) for i in range(n)]


@pytest.fixture(scope="module")
def state():
    sd = dict(synth.state_dict(DIMS))
    st = SpecialTokens.for_vocab(DIMS.vocab)
    e = sd["model.decoder.embed_tokens.weight"].copy()
    e[st.eot] *= 5.0
    sd["model.decoder.embed_tokens.weight"] = e
    return sd


def _engine(sd, max_batch, fp8):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, COMPUTE_BF16, max_batch)
    e.load_weights(sd.items())
    if fp8:
        e.set_option("xkv_fp8", fp8)
    return e


def _encode(e, clips, audio_ctx=None):
    if audio_ctx:
        e.set_audio_ctx(audio_ctx)
    e.log_mel(clips, want_output=False)
    e.encode(len(clips))


def _prompt(e):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def _bits(r):
    return r.tokens, np.asarray(r.sum_logprob).tobytes(), np.asarray(r.no_speech_prob).tobytes()


def _three_checks(base, e8, run):
    """liveness, reproducibility, agreement of e8's `run()` against e16's result `base`."""
    res = run(e8)
    print("sum_logprob 16-bit", np.asarray(base.sum_logprob), "e4m3", np.asarray(res.sum_logprob))
    assert not np.array_equal(res.sum_logprob, base.sum_logprob), "the e4m3 kernel did not run: scores equal the 16-bit engine's"
    assert _bits(run(e8)) == _bits(res)
    same = [i for i in range(len(base.tokens)) if res.tokens[i] == base.tokens[i]]
    print("clips with equal tokens", len(same), "of", len(base.tokens))
    assert 2 * len(same) >= len(base.tokens), (len(same), len(base.tokens))
    for i in same:
        d = abs(float(res.sum_logprob[i]) - float(base.sum_logprob[i]))
        print("clip", i, "len", len(res.tokens[i]), "delta sum_logprob", d)
        assert d <= 2 * EPS * (len(res.tokens[i]) + 1), (i, d, len(res.tokens[i]))
    return res


@pytest.fixture(scope="module")
def six(state):
    """The 6-clip x 5-row reference shared by the tests of that shape: e16 with its clips encoded, and its beam result."""
    clips = _clips(6)
    e16 = _engine(state, 30, 0)
    _encode(e16, clips)
    opts = e16.gen_opts(N_NEW, False)
    base = e16.generate_beam([_prompt(e16)] * 6, 5, opts)
    yield {"e16": e16, "clips": clips, "beam": base}
    e16.close()


def test_beam5_six_clips_liveness_agreement_and_ab_switch(state, six):
    """30 rows, 4 frame slices (6 x 20 = 120 (clip, head) items), NQ = 5, workspace + merge."""
    e16, clips = six["e16"], six["clips"]
    e8 = _engine(state, 30, 2)
    try:
        _encode(e8, clips)
        prompts = [_prompt(e8)] * 6
        opts = e8.gen_opts(N_NEW, False)
        _three_checks(six["beam"], e8, lambda e: e.generate_beam(prompts, 5, opts))
        for prefill in (0, 1):
            for e in (e16, e8):
                e.set_option("prefill", prefill)
            base = six["beam"] if prefill else e16.generate_beam(prompts, 5, opts)
            e8.set_option("xattn_mq_fp8", 0)                  # mode 2, shared rows on the 16-bit cache: no encode needed
            assert _bits(e8.generate_beam(prompts, 5, opts)) == _bits(base), prefill
            e8.set_option("xattn_mq_fp8", 1)
            assert _bits(e8.generate_beam(prompts, 5, opts)) != _bits(base), prefill     # and back on the e4m3 copy
            e8.set_option("xkv_fp8", 0)
            _encode(e8, clips)
            assert _bits(e8.generate_beam(prompts, 5, opts)) == _bits(base), prefill
            e8.set_option("xkv_fp8", 2)
            _encode(e8, clips)
    finally:
        e16.set_option("prefill", 1)
        e8.close()


def _order_stable(e16, e16b, prompts, beam, opts):
    """Do the inputs now encoded in both 16-bit engines give the same tokens whatever the summation order of the 16-bit
    shared-clip kernel (1 and 2 frame slices instead of the automatic count)?  A property of the inputs, not of any e4m3 code:
    clips whose beam flips under a reordering of f32 additions carry no information about a quantised cache."""
    base = e16.generate_beam(prompts, beam, opts)
    ok = True
    for slices in (1, 2):
        e16b.set_option("xattn_mq_slices", slices)
        ok &= e16b.generate_beam(prompts, beam, opts).tokens == base.tokens
    e16b.set_option("xattn_mq_slices", 0)
    return base, ok


@pytest.mark.parametrize("beam,n_clips,audio_ctx", [(2, 13, None), (7, 2, None), (5, 3, 150)],
                         ids=["beam2x13-one-slice", "beam7x2-eight-slices", "beam5x3-ctx150-clamped-tail"])
def test_other_instantiations_and_slice_shapes(state, beam, n_clips, audio_ctx):
    """beam 2 x 13: 260 items, one slice, stored directly (NQ = 2).  beam 7 x 2: 40 items, 8 slices (NQ = 7).  beam 5 x 3 at 150
    encoder positions: slices of 64, 64 and 22 frames - a last slice shorter than one 32-frame iteration of the workgroup.

    Clip seeds: the agreement check needs inputs on which the 16-bit engine agrees with ITSELF.  Observed on an MI355X at 150
    positions of 3-s noise, seed 500: sum_logprob e16 -25.84 / -6.48 / -38.36 against e4m3 -37.43 / -6.54 / -37.52, one clip of
    three with equal tokens - the boosted-EOT beam ends in near-ties there.  Whether e16 itself flips on those clips has not
    been recorded, so the seed is not hard-coded yet: the clips are the first of a fixed list of seeds whose e16 tokens do not
    change when only the 16-bit kernel's frame-slice count does (_order_stable; the chosen seed is printed).  The e4m3 engine
    plays no part in the choice, and the share it must reach stays one half ("Measured")."""
    e16, e16b, e8 = (_engine(state, beam * n_clips, m) for m in (0, 0, 2))
    try:
        opts = e16.gen_opts(N_NEW, False)
        prompts = [_prompt(e16)] * n_clips
        for seed in (500, 520, 540, 560, 580, 600):
            clips = _clips(n_clips, seed=seed, samples=48000 if audio_ctx else None)
            for e in (e16, e16b):
                _encode(e, clips, audio_ctx)
            base, ok = _order_stable(e16, e16b, prompts, beam, opts)
            print("seed", seed, "16-bit tokens independent of the slice count:", ok)
            if ok:
                break
        else:
            pytest.fail("no seed of the list gives clips on which the 16-bit engine agrees with itself")
        _encode(e8, clips, audio_ctx)
        _three_checks(base, e8, lambda e: e.generate_beam(prompts, beam, opts))
    finally:
        e16.close(); e16b.close(); e8.close()


def test_below_256_items_the_16bit_frame_split_kernels_keep_the_shape(state):
    """beam 5 x 2 clips = 200 (row, head) items: not the shared-clip kernel's shape in either mode - bit-identical to e16."""
    clips = _clips(2, seed=700)
    e16, e8 = _engine(state, 10, 0), _engine(state, 10, 2)
    try:
        for e in (e16, e8):
            _encode(e, clips)
        prompts = [_prompt(e16)] * 2
        opts = e16.gen_opts(N_NEW, False)
        assert _bits(e8.generate_beam(prompts, 5, opts)) == _bits(e16.generate_beam(prompts, 5, opts))
    finally:
        e16.close(); e8.close()


def test_sampled_rows_read_the_copy_and_finished_rows_change_nothing(state, six):
    """best_of 5 x 6 clips, temperature 0.4: live, reproducible, and rows that end early leave the clips still running
    unchanged (ragged_exit = 0 keeps every row streaming until the last one ends)."""
    e16, clips = six["e16"], six["clips"]
    e8 = _engine(state, 30, 2)
    try:
        _encode(e8, clips)
        prompts = [_prompt(e8)] * 6
        opts = e8.gen_opts(N_NEW, False)
        run = lambda e: e.generate_sample(prompts, 5, opts, 0.4, seed=4242)
        base, res = run(e16), run(e8)
        assert not np.array_equal(res.sum_logprob, base.sum_logprob)
        assert _bits(run(e8)) == _bits(res)
        assert len({len(t) for t in res.tokens}) > 1 or min(len(t) for t in res.tokens) < N_NEW   # some rows did end early
        e8.set_option("ragged_exit", 0)
        assert _bits(run(e8)) == _bits(res)
    finally:
        e8.close()


def test_mode_one_keeps_the_16bit_beam(state, six):
    e1 = _engine(state, 30, 1)
    try:
        _encode(e1, six["clips"])
        prompts = [_prompt(e1)] * 6
        assert _bits(e1.generate_beam(prompts, 5, e1.gen_opts(N_NEW, False))) == _bits(six["beam"])
    finally:
        e1.close()


def test_option_range_and_the_f32_engine():
    from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
    e = Engine(PRESETS["micro"], COMPUTE_BF16, 2)
    for bad in (3, -1):
        with pytest.raises(TtasrError):
            e.set_option("xkv_fp8", bad)
    for ok in (2, 1, 0):
        e.set_option("xkv_fp8", ok)
    e.close()
    f = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    for v in (1, 2):
        with pytest.raises(TtasrError):
            f.set_option("xkv_fp8", v)
    f.set_option("xkv_fp8", 0)
    f.close()
