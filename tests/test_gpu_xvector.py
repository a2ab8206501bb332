"""GPU: the XVectorSincNet-shaped speaker-embedding network on the device (ttasr_spk_*, kernels_spk.hip) against the float64
restatement of tests/xvector_reference.py on synthetic weights, its bit-level contracts, its isolation from the rest of the
context and its refusals.

Tolerances (tests/xvector_cases.py): max |device - float64| / max |float64| per case, at most EMB_TOL = 16 x 2.4e-5 for the
embeddings and STATS_TOL = 16 x 2.9e-5 for the pooled statistics of the known-answer hook - 16 times what the float32 run of
the reference costs on these very inputs.  Each case prints its measured figures before it asserts.

The one-hot masks: the issue names frames 0, 146 and 292.  The pooling resamples the 293 weights to 279 frames by
w'[j] = w[(293 j) // 279], which reads neither 146 nor 292, so those two masks sum to 0 after the resampling and their rows
are NaN on the device and in the reference alike; frames 145 and 291 - read by pooled frames 139 and 278 - stand beside them
and show the middle and the last block-5 frame."""
import ctypes as C

import numpy as np
import pytest

import xvector_cases as XC
from taiwan_tongues_asr_ce_amd import _lib, diarization, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
from xvector_reference import cached_embeddings

pytestmark = pytest.mark.gpu

GROUP = _lib.SPK_GROUP
_engines = {}
_cases = XC.cases()


def _engine(mode=COMPUTE_F32, dim=192, max_batch=12):
    """One micro engine per (compute mode, D) with the synthetic networks loaded, shared by the tests of this module."""
    key = (mode, dim, max_batch)
    if key not in _engines:
        e = Engine(PRESETS["micro"], mode, max_batch)
        e.load_weights(synth.iter_weights(PRESETS["micro"]))
        e.load_vad(vad.synth_silero_weights(vad.SYNTH_SILERO_SEED))
        e.load_segmentation(vad.synth_pyannet_weights(vad.SYNTH_PYANNET_SEED, 3))
        e.load_speaker_embedding(diarization.synth_xvector_weights(XC.SEED, dim))
        _engines[key] = e
    return _engines[key]


def _check(name, audio, weights, emb, stats, dim=192, key=None):
    want_e, want_s = cached_embeddings(XC.SEED, dim, key or name, audio, weights)
    assert emb.dtype == stats.dtype == np.float32 and emb.shape == want_e.shape and stats.shape == want_s.shape
    re, rs = XC.rel(emb, want_e), XC.rel(stats, want_s)
    e32, s32 = cached_embeddings(XC.SEED, dim, key or name, audio, weights, np.float32)
    print(f"spk {name} (D = {dim}): device vs float64 embeddings {re:.3e} statistics {rs:.3e}; float32 reference vs float64 "
          f"{XC.rel(e32, want_e):.3e} {XC.rel(s32, want_s):.3e}; tolerances {XC.EMB_TOL:.2e} {XC.STATS_TOL:.2e}")
    assert re <= XC.EMB_TOL and rs <= XC.STATS_TOL, (name, re, rs)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for u, v in zip(a, b) for x, y in zip(u, v))


# ---- accuracy against float64 ----

def test_every_length_and_mask_count_alone_and_mixed_in_one_call():
    e = _engine()
    names = [f"noise {n}" for n in XC.LENGTHS]
    alone = {}
    for name in names:
        a, w = _cases[name]
        emb, stats = e.speaker_embeddings([a], [w], return_stats=True)
        _check(name, a, w, emb[0], stats[0])
        alone[name] = (emb[0], stats[0])
    # one call, one S: the recordings with three masks and an empty one between them; each equals itself alone, bit for bit
    three = [n for n in names if _cases[n][1].shape[1] == 3]
    audios = [_cases[three[0]][0], np.zeros(0, np.float32)] + [_cases[n][0] for n in three[1:]]
    wts = [_cases[three[0]][1], np.zeros((0, 3, 293), np.float32)] + [_cases[n][1] for n in three[1:]]
    emb, stats = e.speaker_embeddings(audios, wts, return_stats=True)
    assert emb[1].shape == (0, 3, 192) and stats[1].shape == (0, 3, 3000)
    for i, n in zip((0, 2, 3), three):
        assert np.array_equal(emb[i], alone[n][0]) and np.array_equal(stats[i], alone[n][1]), n


@pytest.mark.parametrize("dim", XC.DIMS)
def test_every_embedding_dimension(dim):
    e = _engine(dim=dim)
    assert e.spk_dim == dim
    a, w = _cases["noise 88001"]
    emb, stats = e.speaker_embeddings([a], [w], return_stats=True)
    _check("noise 88001", a, w, emb[0], stats[0], dim=dim)
    # the statistics do not know D
    assert np.array_equal(stats[0], _engine().speaker_embeddings([a], [w], return_stats=True)[1][0])


def test_silence_constants_scales_and_a_small_variance():
    e = _engine()
    for name in ("zeros", "constant", "noise x 1000", "noise x 1e-4", "0.5 + 1e-3 noise", "short masks"):
        a, w = _cases[name]
        emb, stats = e.speaker_embeddings([a], [w], return_stats=True)
        _check(name, a, w, emb[0], stats[0])


def test_one_hot_masks_show_single_frames_through_the_hook():
    e = _engine()
    a, w = _cases["one-hot"]
    emb, stats = e.speaker_embeddings([a], [w], return_stats=True)
    _check("one-hot", a, w, emb[0], stats[0])
    for s, f in enumerate(XC.ONE_HOT + XC.ONE_HOT_READ):
        if f in (146, 292):                                        # read by no pooled frame: a zero-sum mask
            assert np.isnan(stats[0][0, s]).all() and np.isnan(emb[0][0, s]).all(), f
        else:                                                      # one frame: its mean is the frame, its deviation 0
            assert np.isfinite(emb[0][0, s]).all() and not stats[0][0, s, 1500:].any() and np.ptp(stats[0][0, s, :1500]) > 0.5, f
    assert not np.array_equal(stats[0][0, 0], stats[0][0, 3]) and not np.array_equal(stats[0][0, 3], stats[0][0, 4])


# ---- bit-level contracts ----

def test_a_mask_row_does_not_depend_on_the_mask_count_or_the_other_masks():
    e = _engine()
    a, w8 = _cases["noise 80000"]
    e8, s8 = e.speaker_embeddings([a], [w8], return_stats=True)
    for s in (0, 3, 7):
        e1, s1 = e.speaker_embeddings([a], [w8[:, s:s + 1]], return_stats=True)
        assert np.array_equal(e1[0][:, 0], e8[0][:, s]) and np.array_equal(s1[0][:, 0], s8[0][:, s]), s
    other = w8.copy()
    other[:, 1] = 0.0                                              # a zero-sum mask between its neighbours
    other[:, 5] = XC.masks(1, 1, 999)[0, 0]
    eo, so = e.speaker_embeddings([a], [other], return_stats=True)
    assert np.isnan(eo[0][:, 1]).all() and np.isnan(so[0][:, 1]).all()
    for s in (0, 2, 3, 4, 6, 7):
        assert np.array_equal(eo[0][:, s], e8[0][:, s]) and np.array_equal(so[0][:, s], s8[0][:, s]), s
    assert not np.array_equal(eo[0][:, 5], e8[0][:, 5])


def test_group_boundary_chunk_identity_order_and_repetition():
    """Recordings of GROUP and GROUP + 1 chunks, in one call and alone; chunk k equals the single-chunk call on its samples; the
    reference is asked for three of the chunks only (each costs it a full network)."""
    e = _engine()
    n_more, n_full = 80000 + 8000 * GROUP, 80000 + 8000 * (GROUP - 1)
    sig = XC.noise(n_more, 31337)
    assert XC.n_chunks(n_more) == GROUP + 1 and XC.n_chunks(n_full) == GROUP
    w = XC.masks(GROUP + 1, 2, 31337)
    both = e.speaker_embeddings([sig, sig[:n_full]], [w, w[:GROUP]], return_stats=True)
    more = e.speaker_embeddings([sig], [w], return_stats=True)
    full = e.speaker_embeddings([sig[:n_full]], [w[:GROUP]], return_stats=True)
    assert _same(both, ([more[0][0], full[0][0]], [more[1][0], full[1][0]]))
    assert np.array_equal(more[0][0][:GROUP - 1], full[0][0][:GROUP - 1])       # the chunks that are the same 80 000 samples
    ks = (0, GROUP - 1, GROUP)
    cuts = e.speaker_embeddings([sig[8000 * k:8000 * k + 80000] for k in ks], [w[k:k + 1] for k in ks], return_stats=True)
    for i, k in enumerate(ks):
        assert np.array_equal(cuts[0][i][0], more[0][0][k]) and np.array_equal(cuts[1][i][0], more[1][0][k]), k
        x = np.zeros(80000, np.float32)
        x[:len(sig[8000 * k:8000 * k + 80000])] = sig[8000 * k:8000 * k + 80000]
        _check(f"chunk {k} of {GROUP + 1}", x, w[k:k + 1], more[0][0][k:k + 1], more[1][0][k:k + 1], key=("group", k))
    # call order and repetition
    rev = e.speaker_embeddings([sig[:n_full], sig], [w[:GROUP], w], return_stats=True)
    assert _same(both, tuple(x[::-1] for x in rev)) and _same(both, e.speaker_embeddings([sig, sig[:n_full]], [w, w[:GROUP]], return_stats=True))


def test_compute_mode_does_not_change_a_bit():
    a, w = _cases["noise 88001"]
    want = _engine(COMPUTE_F32).speaker_embeddings([a], [w], return_stats=True)
    for mode in (COMPUTE_BF16, COMPUTE_F16):
        assert _same(want, _engine(mode).speaker_embeddings([a], [w], return_stats=True)), mode


# ---- state isolation and refusals ----

def test_generate_vad_and_segmentation_around_a_call_are_bit_identical():
    e = _engine(COMPUTE_BF16)
    n = PRESETS["micro"].n_frames * 160
    clips = [synth.noise_clip(i, n) for i in range(2)]
    speech = XC.noise(16000 * 3, 11)
    st = e.special
    opts = e.gen_opts(12, True, suppress=[1, 2, 7, st.sot], begin_suppress=[5, st.eot], check_interval=1)
    gen = lambda: e.generate([[st.sot, st.lang_zh, st.transcribe]] * 2, opts)   # noqa: E731
    e.log_mel(clips, want_output=False)
    e.encode(2)
    a, va, sa = gen(), e.vad_probs([speech], return_logits=True), e.segmentation_scores([speech], return_chunks=True)
    x, w = _cases["noise 88001"]
    e.speaker_embeddings([x], [w])
    b, vb, sb = gen(), e.vad_probs([speech], return_logits=True), e.segmentation_scores([speech], return_chunks=True)
    assert a.tokens == b.tokens and np.array_equal(a.sum_logprob, b.sum_logprob) and np.array_equal(a.no_speech_prob, b.no_speech_prob)
    assert np.array_equal(va[0][0], vb[0][0]) and np.array_equal(va[1][0], vb[1][0]) and _same(sa, sb)


def _raw_load(e, name, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    dims = (C.c_int64 * a.ndim)(*a.shape)
    return e.lib.ttasr_spk_load_tensor(e.h, name.encode(), a.ctypes.data_as(C.c_void_p), dims, a.ndim)


def _raw_embed(e, audios, wts, s_n=1, ns=None, null=None, n=None):
    m = len(audios)
    outs = [np.zeros((max(1, XC.n_chunks(len(a))), 8, 512), np.float32) for a in audios]
    ptr = lambda arrs, what: (C.c_void_p * max(m, 1))(*[None if null == what else a.ctypes.data for a in arrs])   # noqa: E731
    ns = np.asarray([len(a) for a in audios] if ns is None else ns, dtype=np.int64)
    return e.lib.ttasr_spk_embed(e.h, m if n is None else n, ptr(audios, "pcm"), ns.ctypes.data_as(C.POINTER(C.c_int64)), s_n,
                                 None if null == "array" else ptr(wts, "weights"), ptr(outs, "out"), None)


def test_refusals_leave_the_context_usable():
    w = diarization.synth_xvector_weights(XC.SEED, 192)
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))
    a, m = _cases["noise 79999"]
    E_INVALID, E_WEIGHTS = -1, -4
    assert _raw_embed(e, [a], [m]) == E_INVALID                   # nothing loaded
    assert e.lib.ttasr_spk_dim(e.h) == E_INVALID
    assert _raw_load(e, "tdnns.3.weight", np.zeros((512, 512, 5))) == E_WEIGHTS             # block 2 has three taps
    assert _raw_load(e, "tdnns.15.weight", np.zeros((512, 512, 1))) == E_WEIGHTS            # unknown name
    assert _raw_load(e, "embedding.weight", np.zeros((513, 3000))) == E_WEIGHTS             # D outside [1, 512]
    names = list(w)
    assert len(names) == 45
    for k in names[:-1]:
        assert _raw_load(e, k, w[k]) == 0
    assert e.lib.ttasr_spk_finalize(e.h) == E_WEIGHTS             # one tensor missing
    assert _raw_load(e, names[-1], np.zeros(2)) == 0
    assert e.lib.ttasr_spk_finalize(e.h) == E_WEIGHTS             # the Linear's weight and bias disagree on D
    assert _raw_embed(e, [a], [m]) == E_INVALID                   # not finalized
    assert _raw_load(e, names[-1], w[names[-1]]) == 0
    assert e.lib.ttasr_spk_finalize(e.h) == 0 and e.lib.ttasr_spk_dim(e.h) == 192
    assert _raw_load(e, names[0], w[names[0]]) == E_INVALID       # read-only from here on
    e.has_speaker_embedding, e.spk_dim = True, 192
    want = _engine().speaker_embeddings([a], [m])[0]
    assert np.array_equal(e.speaker_embeddings([a], [m])[0], want)
    assert _raw_embed(e, [a, a, a], [m, m, m]) == E_INVALID       # n > max_batch
    assert _raw_embed(e, [], []) == E_INVALID
    assert _raw_embed(e, [a], [m], s_n=0) == E_INVALID and _raw_embed(e, [a], [m], s_n=9) == E_INVALID
    assert _raw_embed(e, [a], [m], ns=[-1]) == E_INVALID          # negative length
    assert _raw_embed(e, [a], [m], ns=[(1 << 40) + 1]) == E_INVALID
    for what in ("pcm", "weights", "out", "array"):
        assert _raw_embed(e, [a], [m], null=what) == E_INVALID, what
    for bad in (-1e-3, np.nan, np.inf):
        mb = m.copy()
        mb[0, 0, 17] = bad
        assert _raw_embed(e, [a], [mb]) == E_INVALID, bad
        with pytest.raises(TtasrError):
            e.speaker_embeddings([a], [mb])
    with e.session(e.gen_opts(4, True), 4):
        assert _raw_embed(e, [a], [m]) == E_INVALID               # an open session
        with pytest.raises(TtasrError):
            e.speaker_embeddings([a], [m])
    assert np.array_equal(e.speaker_embeddings([a], [m])[0], want)    # usable after every refusal
    e.close()
