"""GPU: batched on-device word alignment (`ttasr_align_batch`): the teacher-forced pass for several sequences against the
oracle, the post-processing kernel against its formula in float64, the device DTW against the host DTW (exact), the batched
path against the one-clip path, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import alignment as A
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

HEADS = [(3, 0), (3, 5), (2, 1), (1, 4)]
N_CLIPS = 5


def _clips():
    return [synth.noise_clip(0), synth.tonal_clip(7), synth.burst_clip(2), synth.tonal_clip(3), synth.noise_clip(5)]


def _engine(compute, max_batch=6):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    pd = PRESETS["tiny"]
    e = Engine(pd, compute, max_batch)
    e.load_weights(synth.iter_weights(pd))
    e.log_mel(_clips(), want_output=False)
    e.encode(N_CLIPS)
    return e, pd


def _sequences(st, lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [[st.sot, st.lang_zh, st.transcribe, st.no_timestamps] + rng.integers(300, 20000, size=n).tolist() + [st.eot]
            for n in lengths]


def _host_cost(w, first_row, last_row, num_frames, width, dtype):
    """alignment.token_start_times' expressions up to the dtw call, in `dtype`."""
    w = w[..., : max(1, num_frames // 2)]
    w = w[:, first_row:last_row, :].astype(dtype)
    std = w.std(axis=-2, keepdims=True)
    mean = w.mean(axis=-2, keepdims=True)
    return -A.median_filter((w - mean) / np.where(std > 0, std, 1.0), width).mean(axis=0)


def _host_starts(cost):
    ti, tj = A.dtw(cost)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    return tj[jumps]


# sequence -> clip: mixed order, clips 1 and 2 twice
SEQ_CLIP = [2, 0, 1, 4, 2, 1]
SEQ_LEN = [12, 37, 90, 5, 61, 20]
SEQ_FRAMES = [1100, 2400, 3000, 3000, 1, 777]      # F = 550, 1200, 1500, 1500, 1, 388


@pytest.mark.parametrize("compute,w_tol,lp_tol", [(COMPUTE_F32, 2e-5, 2e-3), (COMPUTE_BF16, 6e-3, 0.15), (COMPUTE_F16, 6e-3, 0.15)])
def test_pass_cost_and_dtw(compute, w_tol, lp_tol):
    """1. maps and log-probs of every sequence against the oracle (tolerances of test_gpu_align.py); 2. the cost matrices against
    the float64 formula on the same call's maps, at most 4x the error of the f32 host expressions; 3. the start frames equal
    the host DTW's on the same call's cost matrices, element for element."""
    e, pd = _engine(compute)
    dims = R.Dims(**pd.as_dict())
    st = e.special
    W = R.to_torch(synth.state_dict(pd), round_bf16=compute == COMPUTE_BF16, round_f16=compute == COMPUTE_F16)
    enc = R.encoder_forward(torch.from_numpy(np.stack([R.log_mel(c, pd.n_mels) for c in _clips()])), W, dims)
    seqs = _sequences(st, SEQ_LEN)
    first = [3] * len(seqs)
    first[3] = 0
    r = e.align_batch(SEQ_CLIP, seqs, first, SEQ_FRAMES, HEADS, medfilt_width=7, debug=True)
    worst_dev = worst_host = 0.0
    for i, tok in enumerate(seqs):
        w, lp = r.weights[i], r.logprobs[i]
        assert w.shape == (len(HEADS), len(tok), 1500) and lp.shape == (len(tok) - 1,)
        np.testing.assert_allclose(w.sum(-1), 1.0, atol=1e-4)
        rw, rlp = R.alignment_weights(enc[SEQ_CLIP[i]:SEQ_CLIP[i] + 1], tok, W, dims, HEADS, return_logprobs=True)
        assert np.abs(w - rw.numpy()).max() < w_tol, (i, np.abs(w - rw.numpy()).max())
        assert np.abs(lp - rlp.numpy()).max() < lp_tol, (i, np.abs(lp - rlp.numpy()).max())
        want64 = _host_cost(w, first[i], len(tok) - 1, SEQ_FRAMES[i], 7, np.float64)
        host32 = _host_cost(w, first[i], len(tok) - 1, SEQ_FRAMES[i], 7, np.float32)
        assert r.costs[i].shape == want64.shape
        err_dev, err_host = np.abs(r.costs[i] - want64).max(), np.abs(host32 - want64).max()
        print(f"compute {compute} sequence {i}: cost {want64.shape} |C| <= {np.abs(want64).max():.3g}  device err {err_dev:.3e}  host f32 err {err_host:.3e}")
        worst_dev, worst_host = max(worst_dev, err_dev), max(worst_host, err_host)
        assert err_dev <= 4 * err_host, (i, err_dev, err_host)
        np.testing.assert_array_equal(r.start_frames[i], _host_starts(r.costs[i]))
    print(f"compute {compute}: worst device err {worst_dev:.3e}, worst host f32 err {worst_host:.3e}")
    e.close()


def test_dtw_exact_long_rows_and_unfiltered():
    """3, the cases: a sequence of more than 224 rows whose trace stays in LDS, one whose trace spills to global memory
    (rows x ceil(F / 16) words beyond 150 KiB), F = 1, and medfilt_width = 1."""
    e, pd = _engine(COMPUTE_F32)
    st = e.special
    lengths = [300, 436, 9, 30]
    frames = [3000, 3000, 2, 1500]
    seqs = _sequences(st, lengths, seed=11)
    for width in (1, 7):
        r = e.align_batch([1, 3, 0, 2], seqs, [3] * 4, frames, HEADS, medfilt_width=width, debug=True)
        for i, tok in enumerate(seqs):
            want = _host_cost(r.weights[i], 3, len(tok) - 1, frames[i], width, np.float64)
            assert r.costs[i].shape == want.shape == (lengths[i] + 1, max(1, frames[i] // 2))
            assert np.abs(r.costs[i] - want).max() < 1e-4
            np.testing.assert_array_equal(r.start_frames[i], _host_starts(r.costs[i]))
    assert r.costs[1].shape[0] * ((1500 + 15) // 16) * 4 > 150 * 1024      # the spilled-trace path ran
    e.close()


class _Tok:
    """One character per token: enough for the word-building code."""
    def decode(self, toks):
        return "".join(chr(0x4E00 + (t % 2000)) for t in toks if t < 50000)


def test_batch_against_one_clip_path():
    """4. find_alignment_batch against find_alignment per clip after the same static pass, f32: same words and token groups,
    probabilities within 2e-3 in log space, start and end equal for >= 90 % of all words (the bar of test_gpu_align.py:44)."""
    e, pd = _engine(COMPUTE_F32)
    st = e.special
    rng = np.random.default_rng(5)
    texts = [rng.integers(300, 20000, size=n).tolist() for n in (12, 37, 90, 24, 55)]
    frames = [1100, 2400, 3000, 2000, 2999]
    got = A.find_alignment_batch(e, _Tok(), st, list(range(N_CLIPS)), texts, frames, HEADS)
    same = total = 0
    for clip in range(N_CLIPS):
        want = A.find_alignment(e, _Tok(), st, clip, texts[clip], frames[clip], HEADS)
        assert [w["word"] for w in got[clip]] == [w["word"] for w in want] and len(want) > 0
        assert [w["tokens"] for w in got[clip]] == [w["tokens"] for w in want]
        for a, b in zip(got[clip], want):
            assert abs(np.log(a["probability"]) - np.log(b["probability"])) < 2e-3
            same += (a["start"] == b["start"]) and (a["end"] == b["end"])
            total += 1
    print(f"words with equal start and end: {same} / {total}")
    assert same >= 0.9 * total
    e.close()


def test_refusals_leave_the_context_usable():
    """5. every range of the C ABI, a duplicate head, n > max_batch and an open session: TTASR_E_INVALID, and a generate works."""
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e, pd = _engine(COMPUTE_F32, max_batch=5)
    st = e.special
    lib, i32p, f32p = e.lib, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    tok = np.zeros((2, 10), dtype=np.int32)
    tok[:] = _sequences(st, [5, 5])[0]
    good = dict(n=2, clip=[0, 1], n_tokens=[10, 10], max_tokens=10, first_row=[3, 3], num_frames=[3000, 3000],
                pairs=[3, 0, 2, 1], n_pairs=2, width=7, tokens=tok)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        arr = lambda v: np.ascontiguousarray(v, dtype=np.int32)
        clip, nt, fr, nf, pr, tk = arr(a["clip"]), arr(a["n_tokens"]), arr(a["first_row"]), arr(a["num_frames"]), arr(a["pairs"]), arr(a["tokens"])
        start = np.zeros((8, 16), dtype=np.int32)
        lp = np.zeros((8, 16), dtype=np.float32)
        return lib.ttasr_align_batch(e.h, a["n"], clip.ctypes.data_as(i32p), tk.ctypes.data_as(i32p), nt.ctypes.data_as(i32p),
                                     a["max_tokens"], fr.ctypes.data_as(i32p), nf.ctypes.data_as(i32p), pr.ctypes.data_as(i32p),
                                     a["n_pairs"], a["width"], start.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), None, None)

    opts = e.gen_opts(4, True)
    prompts = [[st.sot, st.lang_zh, st.transcribe]] * 3
    assert call() == 0
    bad_tok = tok.copy()
    bad_tok[1, 4] = pd.vocab
    for bad in (dict(n=0), dict(n=6, clip=[0] * 6, n_tokens=[10] * 6, first_row=[3] * 6, num_frames=[3000] * 6, tokens=np.tile(tok[:1], (6, 1))),
                dict(clip=[0, 5]), dict(clip=[-1, 0]), dict(n_tokens=[1, 10]), dict(n_tokens=[11, 10]), dict(max_tokens=1),
                dict(max_tokens=449), dict(first_row=[9, 3]), dict(first_row=[-1, 3]), dict(num_frames=[-2, 3000]), dict(width=0),
                dict(width=6), dict(width=17), dict(pairs=[4, 0, 2, 1]), dict(pairs=[3, 6, 2, 1]), dict(pairs=[3, 0, 3, 0]),
                dict(n_pairs=0), dict(n_pairs=25), dict(tokens=bad_tok)):
        assert call(**bad) == -1, bad                                  # TTASR_E_INVALID
        assert len(e.generate(prompts, opts).tokens) == 3
    with e.session(e.gen_opts(8, False, no_speech=False), max_prompt=4):
        assert call() == -1
        with pytest.raises(TtasrError):
            e.align_batch([0], [tok[0].tolist()], [3], [3000], HEADS)
    e.log_mel(_clips(), want_output=False)
    e.encode(N_CLIPS)
    assert call() == 0
    assert len(e.generate(prompts, opts).tokens) == 3
    e.close()
