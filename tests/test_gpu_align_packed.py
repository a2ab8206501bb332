"""GPU: the packed, pass-mate-independent alignment pass of a session (option `align_packed`) and the
cross-attention kernel that writes its maps (`ttasr_align_attn_probe`).
(a) the probe against the float64 reference of tests/align_packed_cases.py inside its derived bound; (b) a held clip's outputs
are the same bits alone, together, reversed, over two calls and over two passes; (c) the chain behind the maps - DTW, cost
matrices, log-probs; (d) with the option off nothing changes."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import align_packed_cases as X
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import alignment as A
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HEADS = [(3, 0), (3, 5), (2, 1), (1, 4)]
CT = {COMPUTE_F32: "f32", COMPUTE_BF16: "bf16", COMPUTE_F16: "f16"}
COMPUTES = [COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16]


def _pool(n):
    makers = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
    return [makers[i % 3](i)[: (4 + i % 5) * 16000] for i in range(n)]


def _engine(compute, max_batch):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    pd = PRESETS["tiny"]
    e = Engine(pd, compute, max_batch)
    e.load_weights(synth.iter_weights(pd))
    return e


def _sequences(st, lengths, seed=3):
    """token sequences of exactly `lengths` tokens (4 prompt tokens, text, <|endoftext|>)"""
    rng = np.random.default_rng(seed)
    return [[st.sot, st.lang_zh, st.transcribe, st.no_timestamps] + rng.integers(300, 20000, size=n - 5).tolist() + [st.eot]
            for n in lengths]


# ---- (a) the probe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", X.WINDOWS)
@pytest.mark.parametrize("compute", COMPUTES)
def test_probe_against_reference(compute, window):
    """Sequences of 2, 31, 32, 33, 128, 129 and 224 rows (one item, item boundaries, two items) reading three clips, at audio
    windows of 20 (one clamped tile), 150 (a clamped last tile) and 1500 frames; layer 0 with no head selected, layer 1 with one,
    layer 2 with all.  Attention output and every map inside the derived bound; a map row sums to 1."""
    ct = CT[compute]
    e = _engine(compute, 4)
    e.set_audio_ctx(window)
    e.log_mel(_pool(X.N_CLIPS), want_output=False)
    e.encode(X.N_CLIPS)
    H = e.dims.n_heads
    selections = {0: [-1] * H, 1: [-1, -1, -1, 0, -1, -1], 2: [2, 0, 5, 1, 4, 3]}
    for layer, head_pair in selections.items():
        K, V = e.cross_kv(layer, 0, X.N_CLIPS), e.cross_kv(layer, 1, X.N_CLIPS)
        for call in X.CALLS:
            lens = [X.SEQ_LENS[i] for i in call]
            slots = X.seq_slots(len(lens))
            q = X.make_q(K, lens, slots, X.rounder(ct), salt=layer)
            ref = X.reference(q, K, V, lens, slots, ct)
            out, maps = e.align_attn_probe(layer, q.reshape(len(q), -1), lens, slots, head_pair)
            r_out, r_map = X.check(out, maps, head_pair, ref)
            print(f"{ct} window {window} layer {layer} rows {sum(lens)}: output at {r_out:.3f}, maps at {r_map:.3f} of the bound")
            assert np.all(np.isfinite(out)) and np.all(np.isfinite(maps))
            assert r_out <= 1.0 and r_map <= 1.0, (layer, lens, r_out, r_map)
            if len(maps):
                np.testing.assert_allclose(maps.sum(-1), 1.0, atol=1e-4)
    e.close()


def test_probe_refusals():
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e = _engine(COMPUTE_BF16, 4)
    d, H = e.dims.d_model, e.dims.n_heads
    q = np.zeros((4, d), np.float32)
    with pytest.raises(TtasrError):
        e.align_attn_probe(0, q, [4], [0], [-1] * H)                       # no resident encoder state
    e.log_mel(_pool(2), want_output=False)
    e.encode(2)
    e.align_attn_probe(0, q, [4], [1], [-1] * H)
    for bad in (dict(layer=4), dict(slots=[2]), dict(head_pair=[1] + [-1] * (H - 1)), dict(head_pair=[0, 0] + [-1] * (H - 2))):
        a = dict(layer=0, slots=[1], head_pair=[-1] * H)
        a.update(bad)
        with pytest.raises(TtasrError):
            e.align_attn_probe(a["layer"], q, [4], a["slots"], a["head_pair"])
    with pytest.raises(TtasrError):
        e.align_attn_probe(0, np.zeros((513, d), np.float32), [513], [0], [-1] * H)    # more rows than a pass holds
    with e.session(e.gen_opts(8, False, no_speech=False), max_prompt=4):
        with pytest.raises(TtasrError):
            e.align_attn_probe(0, q, [4], [0], [-1] * H)                   # refused while a session is open
    e.close()


# ---- held clips ---------------------------------------------------------------------------------------------------------------
def _align_forms(e, clips, seqs, forms, packed=True, touch=True):
    """One session per form: the clips are held, then aligned by the form's calls (lists of clip indices).  -> per form
    {clip index: (start frames, log-probs, cost matrix, maps)}"""
    st = e.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(24, timestamps=False, sot_index=0)
    if touch:
        e.set_option("align_packed", 1 if packed else 0)
    res = []
    for calls in forms:
        got = {}
        with e.session(opts, len(prompt)) as s:
            s.hold()
            ids = s.submit(clips, [prompt] * len(clips), [3] * len(clips))
            n_done = 0
            while s.pending > 0:
                n_done += len(s.poll())
            assert n_done == len(clips)
            for idx in calls:
                a = s.align([ids[i] for i in idx], [seqs[i] for i in idx], [3] * len(idx), [len(clips[i]) // 160 for i in idx], HEADS,
                            debug=True)
                for k, i in enumerate(idx):
                    got[i] = (a.start_frames[k], a.logprobs[k], a.costs[k], a.weights[k])
        res.append(got)
    return res


def _same(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("compute", COMPUTES)
def test_outputs_do_not_depend_on_pass_mates(compute):
    """(b) six held clips, sequences of 5 to 224 tokens, three of 224 (672 rows: two passes): aligned all together, reversed,
    over two calls and each alone - start frames, log-probs, cost matrices and maps bit-equal in every form."""
    e = _engine(compute, 8)
    clips = _pool(6)
    seqs = _sequences(e.special, [5, 33, 130, 224, 224, 224])
    every = list(range(6))
    forms = [[every], [every[::-1]], [every[:3], every[3:]], [[i] for i in every]]
    together, reverse, split, alone = _align_forms(e, clips, seqs, forms)
    for i in every:
        assert len(together[i][0]) == len(seqs[i]) - 4 and np.all(np.diff(together[i][0]) >= 0) and np.all(np.isfinite(together[i][1]))
        for name, other in (("reversed", reverse), ("two calls", split), ("alone", alone)):
            assert _same(together[i], other[i]), (i, name)
    e.close()


@lru_cache(maxsize=None)
def _oracle(compute):
    pd = PRESETS["tiny"]
    W = R.to_torch(synth.state_dict(pd), round_bf16=compute == COMPUTE_BF16, round_f16=compute == COMPUTE_F16)
    dims = R.Dims(**pd.as_dict())
    enc = R.encoder_forward(torch.from_numpy(np.stack([R.log_mel(c, pd.n_mels) for c in _pool(3)])), W, dims)
    return W, dims, enc


def _host_cost(w, first_row, last_row, num_frames, width, dtype):
    """alignment.token_start_times' expressions up to the dtw call, in `dtype` (as tests/test_gpu_align_batch.py)"""
    w = w[..., : max(1, num_frames // 2)]
    w = w[:, first_row:last_row, :].astype(dtype)
    std = w.std(axis=-2, keepdims=True)
    mean = w.mean(axis=-2, keepdims=True)
    return -A.median_filter((w - mean) / np.where(std > 0, std, 1.0), width).mean(axis=0)


def _host_starts(cost):
    ti, tj = A.dtw(cost)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    return tj[jumps]


@pytest.mark.parametrize("compute,lp_tol", [(COMPUTE_F32, 2e-3), (COMPUTE_BF16, 0.15), (COMPUTE_F16, 0.15)])
def test_chain_behind_the_maps(compute, lp_tol):
    """(c) start frames equal ttasr_dtw on the returned cost matrices; the cost matrices against the float64 formula on the
    returned maps within the bound of test_gpu_align_batch.py (4x the error of the float32 host expressions); log-probs against
    the oracle's teacher-forced pass at that test's engine tolerances."""
    e = _engine(compute, 4)
    clips = _pool(3)
    seqs = _sequences(e.special, [17, 42, 95], seed=5)
    (got,) = _align_forms(e, clips, seqs, [[[2, 0, 1]]])
    W, dims, enc = _oracle(compute)
    for i, tok in enumerate(seqs):
        start, lp, cost, w = got[i]
        frames = len(clips[i]) // 160
        assert w.shape == (len(HEADS), len(tok), 1500) and lp.shape == (len(tok) - 1,)
        np.testing.assert_allclose(w.sum(-1), 1.0, atol=1e-4)
        rw, rlp = R.alignment_weights(enc[i:i + 1], tok, W, dims, HEADS, return_logprobs=True)
        print(f"{CT[compute]} sequence {i}: maps err {np.abs(w - rw.numpy()).max():.3e}  log-prob err {np.abs(lp - rlp.numpy()).max():.3e}")
        assert np.abs(lp - rlp.numpy()).max() < lp_tol, i          # (the maps have their own derived bound: the probe test)
        want64 = _host_cost(w, 3, len(tok) - 1, frames, 7, np.float64)
        host32 = _host_cost(w, 3, len(tok) - 1, frames, 7, np.float32)
        assert cost.shape == want64.shape
        assert np.abs(cost - want64).max() <= 4 * np.abs(host32 - want64).max(), i
        np.testing.assert_array_equal(start, _host_starts(cost))
    e.close()


@pytest.mark.parametrize("compute", [COMPUTE_F32, COMPUTE_BF16])
def test_option_off_changes_nothing(compute):
    """(d) align_packed set to 1 and back to 0: ttasr_session_align's outputs bit-equal to a context that never touched the
    option (the padded pass)."""
    clips = _pool(3)
    a, b = _engine(compute, 4), _engine(compute, 4)
    seqs = _sequences(a.special, [9, 40, 21], seed=7)
    a.set_option("align_packed", 1)
    (off,) = _align_forms(a, clips, seqs, [[[0, 1, 2]]], packed=False)
    (never,) = _align_forms(b, clips, seqs, [[[0, 1, 2]]], touch=False)
    for i in range(3):
        assert _same(off[i], never[i]), i
    a.close(); b.close()
