"""CPU: the float64 restatement of the segmentation network (tests/pyannet_reference.py) is itself held to torch's float64
operators on the same synthetic weights, to the frame arithmetic of include/ttasr.h, and to planted errors - a reference that
could not tell a wrong network from a right one would check nothing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pyannet_reference as R
from taiwan_tongues_asr_ce_amd import vad

SEED = vad.SYNTH_PYANNET_SEED
LOGIT_TOL, PROB_TOL = 1e-3, 2.5e-4     # the tolerances of tests/test_gpu_pyannote.py


def _noise(n, seed, level=0.1):
    return (np.random.default_rng([0x5E6, seed]).standard_normal(n) * level).astype(np.float32)


def _torch_forward(weights, x):
    """x [batch, samples] float32 values -> (probabilities, logits) [batch, frames, C] with torch's float64 operators."""
    w = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in weights.items()}
    y = torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None, :]
    y = F.instance_norm(y, weight=w["sincnet.wav_norm1d.weight"], bias=w["sincnet.wav_norm1d.bias"], eps=1e-5)
    y = torch.abs(F.conv1d(y, w["sincnet.conv1d.0.filters"], stride=10))
    for i in range(3):
        if i:
            y = F.conv1d(y, w[f"sincnet.conv1d.{i}.weight"], w[f"sincnet.conv1d.{i}.bias"])
        y = F.max_pool1d(y, 3, 3)
        y = F.leaky_relu(F.instance_norm(y, weight=w[f"sincnet.norm1d.{i}.weight"], bias=w[f"sincnet.norm1d.{i}.bias"], eps=1e-5))
    lstm = torch.nn.LSTM(60, 128, num_layers=4, bidirectional=True, batch_first=True).double()
    lstm.load_state_dict({k[5:]: v for k, v in w.items() if k.startswith("lstm.")})
    with torch.no_grad():
        y = lstm(y.transpose(1, 2))[0]
        for i in range(2):
            lin = torch.nn.Linear(*reversed(w[f"linear.{i}.weight"].shape)).double()
            lin.load_state_dict({"weight": w[f"linear.{i}.weight"], "bias": w[f"linear.{i}.bias"]})
            y = F.leaky_relu(lin(y))
        logits = F.linear(y, w["classifier.weight"], w["classifier.bias"])
    return torch.sigmoid(logits).numpy(), logits.numpy()


@pytest.fixture(scope="module")
def two_chunks():
    x = np.stack([_noise(R.CHUNK, 1), np.concatenate([_noise(30000, 2, 0.3), np.zeros(R.CHUNK - 30000, np.float32)])])
    weights = vad.synth_pyannet_weights(SEED)
    ref = R.PyanNetRef(weights)
    p, l = ref.head(ref.lstm(np.stack([ref.frontend(c) for c in x])))
    return weights, x, p, l


def test_reference_equals_torch_float64_on_two_chunks(two_chunks):
    weights, x, p, l = two_chunks
    tp, tl = _torch_forward(weights, x)
    assert p.shape == tp.shape == (2, 293, 3)
    print(f"reference vs torch float64: logits {np.abs(l - tl).max():.3e} probs {np.abs(p - tp).max():.3e}")
    assert np.abs(l - tl).max() <= 1e-9 and np.abs(p - tp).max() <= 1e-9
    assert np.ptp(p) > 0.2                                   # the values move


def _torch_stack_frames(weights, n):
    """Frames torch's convolutions and pools leave of n samples (the norms keep a length; torch's refuses a length of one)."""
    w = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in weights.items()}
    y = F.max_pool1d(F.conv1d(torch.zeros(1, 1, n, dtype=torch.float64), w["sincnet.conv1d.0.filters"], stride=10), 3, 3)
    for i in (1, 2):
        y = F.max_pool1d(F.conv1d(y, w[f"sincnet.conv1d.{i}.weight"], w[f"sincnet.conv1d.{i}.bias"]), 3, 3)
    return y.shape[2]


def test_frame_counts_of_the_stages():
    weights = vad.synth_pyannet_weights(SEED)
    ref = R.PyanNetRef(weights)
    for n, frames in ((80000, 293), (991, 1), (1261, 2), (1260, 1)):
        assert R.chunk_frames(n) == frames
        assert ref.frontend(_noise(n, n)).shape == (frames, 60)
        assert _torch_stack_frames(weights, n) == frames
    assert _torch_forward(weights, _noise(1261, 1261)[None])[0].shape == (1, 2, 3)
    assert R.chunk_frames(990) == 0
    with pytest.raises(RuntimeError):
        _torch_stack_frames(weights, 990)


def test_receptive_field_of_a_frame():
    """Without the norms (which span the whole input) frame j of the convolution stack depends on samples [270 j, 270 j + 991)."""
    weights = vad.synth_pyannet_weights(SEED)
    ref = R.PyanNetRef(weights)

    def stack(x):   # sinc -> abs -> pool -> conv -> pool -> conv -> pool
        x = np.asarray(x, np.float64)
        cols = np.stack([x[10 * t:10 * t + 251] for t in range((len(x) - 251) // 10 + 1)])
        y = ref._pool(np.abs(cols @ ref.w["sincnet.conv1d.0.filters"][:, 0, :].T))
        for i in (1, 2):
            y = ref._pool(ref._conv5(y, f"sincnet.conv1d.{i}"))
        return y

    x = _noise(1261, 5).astype(np.float64)
    base = stack(x)
    assert base.shape == (2, 60)
    for at, moved in ((0, (True, False)), (269, (True, False)), (270, (True, True)), (990, (True, True)), (991, (False, True)),
                      (1260, (False, True))):
        y = x.copy()
        y[at] += 0.5
        got = tuple(bool(np.any(stack(y)[j] != base[j])) for j in range(2))
        assert got == moved, (at, got)
    assert (R.FRAME_CENTRE, R.FRAME_STEP) == (495, 270) and (991 - 1) // 2 == 495


def test_chunk_and_frame_tables():
    k_table = {0: 0, 1: 1, 990: 1, 80000: 1, 80001: 2, 87999: 2, 88000: 2, 88001: 3, 96000: 3, 160000: 11, 16000 * 3600: 7191}
    for n, k in k_table.items():
        assert R.n_chunks(n) == k, n
    s_table = {0: 0, 1: 30, 2: 59, 3: 89, 9: 267, 10: 296, 27: 800, 7190: 213037}
    for k, s in s_table.items():
        assert R.chunk_start_frame(k) == s, k
    f_table = {0: 0, 1: 1, 270: 1, 271: 2, 990: 4, 991: 4, 1261: 5, 79999: 293, 80000: 293, 80001: 297, 87999: 323, 88000: 323,
               88001: 326, 16000 * 3600: 213330}
    for n, f in f_table.items():
        assert R.n_frames(n) == f, n
    # every frame of a recording is covered by a chunk, and at most ten chunks overlap
    for n in (80001, 88001, 200000):
        cover = np.zeros(R.n_frames(n), int)
        for k in range(R.n_chunks(n)):
            cover[R.chunk_start_frame(k):R.chunk_start_frame(k) + 293] += 1
        assert cover.min() >= 1 and cover.max() <= 10


def test_aggregation_is_the_weighted_mean_of_the_class_maxima():
    ref = R.PyanNetRef(vad.synth_pyannet_weights(SEED))
    n = 96000                                                     # three chunks, starts 0, 30, 59
    rng = np.random.default_rng(3)
    p = rng.uniform(size=(3, 293, 3))
    got = ref.aggregate(n, p)
    w = np.hamming(293).astype(np.float32).astype(np.float64)
    assert got.shape == (R.n_frames(n),) == (352,)
    assert abs(got[0] - p[0, 0].max()) < 1e-15                    # one chunk covers it
    want = (w[100] * p[0, 100].max() + w[70] * p[1, 70].max() + w[41] * p[2, 41].max()) / (w[100] + w[70] + w[41])
    assert abs(got[100] - want) < 1e-15
    assert abs(got[351] - p[2, 292].max()) < 1e-15


@pytest.mark.parametrize("planted", [dict(gate_order="ifog"), dict(reverse_backward=False), dict(unbiased=True),
                                     dict(pool_before_abs=True)], ids=lambda d: next(iter(d)))
def test_planted_errors_move_the_result_by_more_than_the_tolerances(two_chunks, planted):
    weights, x, p, l = two_chunks
    bad = R.PyanNetRef(weights, **planted)
    bp, bl = bad.head(bad.lstm(np.stack([bad.frontend(c) for c in x])))
    print(f"planted {planted}: logits move {np.abs(bl - l).max():.3e}, probabilities {np.abs(bp - p).max():.3e}")
    assert np.abs(bl - l).max() > LOGIT_TOL and np.abs(bp - p).max() > PROB_TOL


def test_float32_restatement_stays_near_float64(two_chunks):
    weights, x, p, l = two_chunks
    r32 = R.PyanNetRef(weights, np.float32)
    p32, l32 = r32.head(r32.lstm(np.stack([r32.frontend(c) for c in x])))
    assert p32.dtype == np.float32
    print(f"float32 restatement vs float64: logits {np.abs(l32 - l).max():.3e} probs {np.abs(p32 - p).max():.3e}")
    assert np.abs(l32 - l).max() < LOGIT_TOL / 4 and np.abs(p32 - p).max() < PROB_TOL / 4


def test_filters_of_the_reference_and_the_package_agree():
    low, band = vad.mel_cutoffs()
    mine, theirs = R.sinc_filters(low, band), vad.sinc_filters(low, band)
    assert theirs.shape == (80, 1, 251) and theirs.dtype == np.float32
    assert np.abs(mine - theirs[:, 0, :]).max() <= 2.0 ** -24 * np.abs(mine).max()
    assert np.array_equal(mine[:40], mine[:40, ::-1]) and np.array_equal(mine[40:], -mine[40:, ::-1])   # cosine even, sine odd
    assert np.all(mine[:40, 125] == 1.0) and np.all(mine[40:, 125] == 0.0)
    with pytest.raises(ValueError):
        vad.sinc_filters(low[:39], band)


T = lambda j: 495 + 270 * j   # noqa: E731


@pytest.mark.parametrize("fn", [R.binarize, vad.pyannote_speech_timestamps], ids=["reference", "package"])
def test_binarize_on_hand_made_tracks(fn):
    n = 270 * 200
    s = np.full(200, 0.2)
    assert fn(n, s) == [] and fn(0, np.zeros(0)) == []
    s[20:60] = 0.9                                               # opens at frame 20, closes at frame 60: 40 frames = 0.675 s
    assert fn(n, s) == [{"start": T(20), "end": T(60)}]
    s[70:80] = 0.9                                               # 10 frames = 0.169 s after a gap of 0.169 s: merged (gap <= 0.3)
    assert fn(n, s) == [{"start": T(20), "end": T(80)}]
    s[110:120] = 0.9                                             # alone and shorter than 0.3 s: dropped
    assert fn(n, s) == [{"start": T(20), "end": T(80)}]
    assert fn(n, s, min_duration_on=0.0, min_duration_off=0.0) == [
        {"start": T(20), "end": T(60)}, {"start": T(70), "end": T(80)}, {"start": T(110), "end": T(120)}]
    s[180:] = 0.9                                                # still open at the end: closes at the last frame, clipped to n
    assert fn(n, s)[-1] == {"start": T(180), "end": min(T(199), n)}
    # hysteresis: between offset and onset nothing changes
    h = np.array([0.1] * 10 + [0.7] * 30 + [0.5] * 30 + [0.35] * 30 + [0.1] * 20)
    assert fn(270 * 120, h, onset=0.6, offset=0.4) == [{"start": T(10), "end": T(70)}]
    assert fn(270 * 120, h, onset=0.8, offset=0.4) == []
    # exactly at the thresholds: neither above onset nor below offset
    assert fn(270 * 120, np.full(120, 0.5)) == []
    # pads, and the clip at both ends
    up = np.full(200, 0.9)
    assert fn(n, up) == [{"start": T(0), "end": n}]
    assert fn(n, up, pad_onset=0.1) == [{"start": 0, "end": n}]
    s2 = np.full(200, 0.2)
    s2[20:60] = 0.9
    assert fn(n, s2, pad_onset=0.01, pad_offset=0.02) == [{"start": T(20) - 160, "end": T(60) + 320}]
