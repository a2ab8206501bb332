"""GPU: beam search in the continuous-batching session (ttasr_session_begin_beam, Engine.session(beam=...),
WhisperModel.transcribe_stream(beam_size=...), BatchedWhisperASR(continuous=True)).

A clip takes a group of `beam` rows and cross-KV slot g; the batch runs at G*beam rows whatever the occupancy, every row carries
its own position, rows are computed independently, and the candidate kernel and the selection code are those of
ttasr_generate_beam.  So a clip decoded in a beam session must equal, bit for bit (tokens, sum_logprob, no_speech), the same clip
in a static ttasr_generate_beam pass of exactly G clips on the same context with prefill = 0 and, in 16-bit, enc_gemm = 3 (the
session's encoder family).

Geometry: large-v3-w2 (d 1280, 20 heads, 2 + 2 layers), max_batch 30, beam 5 (G = 6).  Synthetic weights emit no real EOT; the
EOT row of the token embedding is scaled (as in test_gpu_beam._micro_state) so hypotheses finish at spread positions."""
import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS, SpecialTokens

from oracle_checks import encode_chunked

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DIMS = PRESETS["large-v3-w2"]
B = 30
BEAM = 5
G = B // BEAM
N_NEW = 48
EOT_BOOST = 5.0
COMPUTES = [(COMPUTE_F32, "f32"), (COMPUTE_BF16, "bf16"), (COMPUTE_F16, "f16")]


def _clips(n, seed=300):
    kinds = (synth.noise_clip, synth.tonal_clip, synth.noise_clip, synth.burst_clip)
    return [kinds[i % 4](seed + i) for i in range(n)]


def _state(boost=EOT_BOOST):
    sd = dict(synth.state_dict(DIMS))
    if boost:
        st = SpecialTokens.for_vocab(DIMS.vocab)
        e = sd["model.decoder.embed_tokens.weight"].copy()
        e[st.eot] *= boost
        sd["model.decoder.embed_tokens.weight"] = e
    return sd


@pytest.fixture(scope="module")
def boosted():
    return _state()


@pytest.fixture(scope="module")
def plain():
    return _state(0.0)


def _engine(compute, sd, max_batch=B):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, compute, max_batch)
    e.load_weights(sd.items())
    return e


def _prompt(e, ts=False):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe] + ([] if ts else [st.no_timestamps])


def _static(e, clips, prompts, opts, patience=1.0, per_pass=G, ragged=False):
    """ttasr_generate_beam over static passes of exactly per_pass clips (prefill = 0, the session's encoder family)."""
    assert len(clips) % per_pass == 0
    e.set_option("prefill", 0)
    e.set_option("enc_gemm", 3)
    toks, lp, ns = [], [], []
    try:
        for i in range(0, len(clips), per_pass):
            e.log_mel(clips[i:i + per_pass], want_output=False)
            e.encode(per_pass)
            pr = prompts[i:i + per_pass]
            r = e.generate_beam(pr, BEAM, opts, patience, sot_index=[opts.sot_index] * per_pass if ragged else None)
            toks += r.tokens
            lp += list(r.sum_logprob)
            ns += list(r.no_speech_prob)
    finally:
        e.set_option("prefill", 1)
        e.set_option("enc_gemm", 0)
    return toks, np.asarray(lp, np.float32), np.asarray(ns, np.float32)


def _session(e, clips, prompts, opts, patience=1.0, caps=None, waves=1, snapshots=None):
    """All clips through one beam session (input order).  waves > 1: the clips arrive in that many waves, each submitted after
    a poll; snapshots: a list that receives ttasr_session_rows after every poll."""
    n = len(clips)
    toks, lp, ns = [None] * n, np.zeros(n, np.float32), np.zeros(n, np.float32)
    cuts = np.linspace(0, n, waves + 1).astype(int)
    max_prompt = max(len(p) for p in prompts)
    ids, got = [], []
    with e.session(opts, max_prompt, beam=BEAM, patience=patience) as s:
        for w in range(waves):
            a, b = cuts[w], cuts[w + 1]
            ids += s.submit(clips[a:b], prompts[a:b], None if caps is None else caps[a:b])
            if w + 1 < waves:
                for _ in range(3):
                    got += s.poll(max_steps=7)
                    if snapshots is not None:
                        snapshots.append(s.rows())
        while s.pending > 0:
            r = s.poll(max_steps=5)
            if snapshots is not None:
                snapshots.append(s.rows())
            got += r
            assert r or s.stats()["steps"] > 0
        stats = s.stats()
    where = {cid: i for i, cid in enumerate(ids)}
    assert len(got) == n and sorted(where[r.id] for r in got) == list(range(n))
    for r in got:
        i = where[r.id]
        toks[i], lp[i], ns[i] = r.tokens, r.sum_logprob, r.no_speech_prob
    return toks, lp, ns, stats


def _same(a, b):
    ta, la, na = a[:3]
    tb, lb, nb = b[:3]
    assert len(ta) == len(tb)
    for i in range(len(ta)):
        assert ta[i] == tb[i], (i, ta[i], tb[i])
    assert np.array_equal(la, lb), (np.flatnonzero(la != lb), la, lb)
    assert np.array_equal(na, nb), (np.flatnonzero(na != nb), na, nb)


@pytest.mark.parametrize("compute", [c for c, _ in COMPUTES], ids=[n for _, n in COMPUTES])
def test_beam_session_is_bit_identical_to_static_passes(boosted, compute):
    clips = _clips(36)
    e = _engine(compute, boosted)
    prompt = _prompt(e)
    opts = e.gen_opts(N_NEW, False)
    prompts = [prompt] * len(clips)
    ses = _session(e, clips, prompts, opts)
    lens = [len(t) for t in ses[0]]
    # hypotheses finished at spread positions, so groups were handed over mid-flight
    assert len(set(lens)) >= 3 and min(lens) < N_NEW, lens
    assert all(e.special.eot not in t for t in ses[0])
    _same(ses, _static(e, clips, prompts, opts))
    stats = ses[3]
    assert stats["clips_encoded"] == len(clips) and stats["steps"] > 0
    if compute == COMPUTE_F32:   # six clips graded by the oracle's beam search
        st = e.special
        rd = R.Dims(**DIMS.as_dict())
        W = R.to_torch(boosted)
        graded = (0, 7, 14, 21, 28, 35)
        enc = encode_chunked(np.stack([R.log_mel(clips[i], DIMS.n_mels) for i in graded]), W, rd)
        rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                        suppress=[opts.suppress[i] for i in range(opts.n_suppress)],
                        begin_suppress=[opts.begin_suppress[i] for i in range(opts.n_begin_suppress)], timestamps=False)
        for k, i in enumerate(graded):
            ref = R.beam_decode(enc[k:k + 1], prompt, W, rd, rules, BEAM, N_NEW)
            assert ses[0][i] == [t for t in ref.tokens[0] if t != st.eot], i
            assert abs(float(ses[1][i]) - ref.sum_logprob[0]) < 2e-2, (i, ses[1][i], ref.sum_logprob[0])
    e.close()


def test_per_clip_budgets_equal_static_passes_at_that_budget(plain):
    budgets = (24, 48, 96)
    clips = _clips(18, seed=500)
    caps = np.asarray([budgets[(i * 7) % 3] for i in range(len(clips))], np.int32)
    e = _engine(COMPUTE_BF16, plain)
    prompt = _prompt(e)
    opts = e.gen_opts(max(budgets), False, suppress_eot=True)
    ses = _session(e, clips, [prompt] * len(clips), opts, caps=caps)
    assert [len(t) for t in ses[0]] == caps.tolist()
    # the reference: clips grouped by budget, each pass padded to G clips (rows are independent in the static pass)
    for bud in budgets:
        idx = [i for i in range(len(clips)) if caps[i] == bud]
        pad = idx + [idx[0]] * (-len(idx) % G)
        ref = _static(e, [clips[i] for i in pad], [prompt] * len(pad), e.gen_opts(bud, False, suppress_eot=True))
        n = len(idx)
        _same(([ses[0][i] for i in idx], ses[1][idx], ses[2][idx]), (ref[0][:n], ref[1][:n], ref[2][:n]))
    e.close()


def test_patience_ragged_prompts_and_timestamps(boosted):
    clips = _clips(12, seed=700)
    e = _engine(COMPUTE_BF16, boosted)
    st = e.special
    extra = [[], [1000], [1000, 2000, 3000], [4000, 5000]]
    prompts = [_prompt(e, ts=True) + extra[i % 4] for i in range(len(clips))]
    opts = e.gen_opts(N_NEW, True, sot_index=0)
    ses = _session(e, clips, prompts, opts, patience=2.0)
    ref = _static(e, clips, prompts, opts, patience=2.0, ragged=True)
    _same(ses, ref)
    assert any(t >= st.timestamp_begin for toks in ses[0] for t in toks)
    e.close()


def test_waves_and_overlap_give_identical_results(boosted):
    clips = _clips(24, seed=900)
    e = _engine(COMPUTE_BF16, boosted)
    prompt = _prompt(e)
    opts = e.gen_opts(N_NEW, False)
    prompts = [prompt] * len(clips)
    snaps = []
    base = _session(e, clips, prompts, opts, waves=3, snapshots=snaps)
    e.set_option("refill_overlap", 1)
    over = _session(e, clips, prompts, opts, waves=3)
    e.set_option("refill_overlap", 0)
    _same(base, over)
    _same(base, _static(e, clips, prompts, opts))
    # rows of one group share clip and position; groups run at different positions at some point of the run
    staggered = False
    for sn in snaps:
        pos, clip = sn["row_pos"], sn["clip"]
        for g in range(G):
            assert len(set(clip[g * BEAM:(g + 1) * BEAM].tolist())) == 1
            assert len(set(pos[g * BEAM:(g + 1) * BEAM].tolist())) == 1
        live = [int(pos[g * BEAM]) for g in range(G) if clip[g * BEAM] >= 0]
        staggered |= len(set(live)) > 1
    assert staggered
    e.close()


def test_wide_batch_of_twelve_groups(boosted):
    clips = _clips(24, seed=1100)
    e = _engine(COMPUTE_BF16, boosted, max_batch=60)
    prompt = _prompt(e)
    opts = e.gen_opts(N_NEW, False)
    prompts = [prompt] * len(clips)
    _same(_session(e, clips, prompts, opts), _static(e, clips, prompts, opts, per_pass=12))
    e.close()


def test_refusals_leave_the_context_usable(boosted):
    from taiwan_tongues_asr_ce_amd import _lib
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    import ctypes as C
    clips = _clips(G, seed=1300)
    e = _engine(COMPUTE_BF16, boosted)
    prompt = _prompt(e)
    opts = e.gen_opts(N_NEW, False)
    before = _static(e, clips, [prompt] * G, opts)
    lib = _lib.load()
    for beam, patience in ((0, 1.0), (8, 1.0), (5, 0.0), (5, -1.0)):
        assert lib.ttasr_session_begin_beam(e.h, C.byref(opts), len(prompt), beam, C.c_float(patience)) != 0
    e.set_option("xkv_fp8", 1)
    assert lib.ttasr_session_begin_beam(e.h, C.byref(opts), len(prompt), BEAM, C.c_float(1.0)) != 0
    e.set_option("xkv_fp8", 0)
    small = _engine(COMPUTE_BF16, boosted, max_batch=4)
    assert lib.ttasr_session_begin_beam(small.h, C.byref(opts), len(prompt), BEAM, C.c_float(1.0)) != 0
    small.close()
    with e.session(opts, len(prompt), beam=BEAM) as s:
        assert lib.ttasr_session_begin_beam(e.h, C.byref(opts), len(prompt), BEAM, C.c_float(1.0)) != 0
        assert lib.ttasr_session_begin(e.h, C.byref(opts), len(prompt), C.c_float(0.0)) != 0
        with pytest.raises(TtasrError):
            e.generate_beam([prompt] * G, BEAM, opts)
        with pytest.raises(TtasrError):
            e.encode(G)
        s.submit(clips[:2], [prompt] * 2)
        assert len(s.drain()) == 2
    _same(_static(e, clips, [prompt] * G, opts), before)
    e.close()


def test_transcribe_stream_beam_equals_transcribe_windows_passes():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", compute_type="float32", max_batch=B)
    clips = [c[: m.n_window] for c in _clips(2 * G, seed=1500)]
    got = m.transcribe_stream(clips, beam_size=BEAM)
    eng = m.engine
    prompt, sot_index = m._prompt(m._lang_token("zh"), "transcribe", True, [])
    opts = eng.gen_opts(min(224, m.dims.n_text_ctx - len(prompt)), timestamps=False, sot_index=sot_index)
    eng.set_option("prefill", 0)
    ref = []
    for i in range(0, len(clips), G):
        eng.log_mel(clips[i:i + G], want_output=False)
        eng.encode(G)
        ref += eng.generate_beam([prompt] * G, BEAM, opts).tokens
    eng.set_option("prefill", 1)
    assert got == ref
    assert m.transcribe_stream(clips[:3]) is not None   # the greedy default is still there


def test_continuous_streaming_backend_equals_lock_step():
    import asyncio
    import types
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR

    utter = []
    for i in range(6):
        a = _clips(6, seed=1700)[i][: 16000 * (2 + i % 3)]
        utter.append((np.clip(a, -1, 1) * 32767).astype(np.int16).tobytes())

    async def run(asr):
        clients = [types.SimpleNamespace(scratch_buffer=utter[i], last_start_time=0, client_id=i) for i in range(6)]
        try:
            return await asyncio.gather(*[asr.transcribe(c) for c in clients])
        finally:
            await asr.aclose()

    kw = dict(model_path="synthetic:tiny", compute_type="float32", max_clips=6, beam_size=BEAM, max_wait_ms=3000.0)
    lock = BatchedWhisperASR(**kw)
    lock.asr_pipeline.engine.set_option("prefill", 0)
    ref = asyncio.run(run(lock))
    assert lock.batches_run == [6]
    cont = BatchedWhisperASR(continuous=True, **kw)
    got = asyncio.run(run(cont))
    assert got == ref
    assert any(r is not None for r in ref)
