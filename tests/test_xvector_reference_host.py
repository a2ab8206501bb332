"""CPU: the float64 restatement of the speaker-embedding network (tests/xvector_reference.py) is itself held to torch's float64
operators, shown to move under every planted error, and the tolerances of tests/xvector_cases.py are measured again: the
float32 run of the same code against the float64 run over every case of the GPU tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xvector_cases as XC
import xvector_reference as XR
from taiwan_tongues_asr_ce_amd import diarization

torch.set_grad_enabled(False)
_W = diarization.synth_xvector_weights(XC.SEED, 192)
_R64 = XR.XVectorRef(_W, np.float64)
_cache64: dict = {}


def _t(name):
    return torch.from_numpy(_W[name].astype(np.float64))


def _torch_network(x80000: np.ndarray, w293: np.ndarray):
    """The network of include/ttasr.h in torch's float64 operators -> (embedding [D], statistics [3000])."""
    lrelu = lambda v: F.leaky_relu(v, 0.01)   # noqa: E731
    x = torch.from_numpy(x80000.astype(np.float64))[None, None]
    x = F.instance_norm(x, weight=_t("sincnet.wav_norm1d.weight"), bias=_t("sincnet.wav_norm1d.bias"), eps=1e-5)
    x = F.max_pool1d(torch.abs(F.conv1d(x, _t("sincnet.conv1d.0.filters"), stride=10)), 3)
    x = lrelu(F.instance_norm(x, weight=_t("sincnet.norm1d.0.weight"), bias=_t("sincnet.norm1d.0.bias"), eps=1e-5))
    for i in (1, 2):
        x = F.max_pool1d(F.conv1d(x, _t(f"sincnet.conv1d.{i}.weight"), _t(f"sincnet.conv1d.{i}.bias")), 3)
        x = lrelu(F.instance_norm(x, weight=_t(f"sincnet.norm1d.{i}.weight"), bias=_t(f"sincnet.norm1d.{i}.bias"), eps=1e-5))
    assert x.shape == (1, 60, 293)
    frames = []
    for l, (taps, dil) in enumerate(XR.BLOCKS):
        x = lrelu(F.conv1d(x, _t(f"tdnns.{3 * l}.weight"), _t(f"tdnns.{3 * l}.bias"), dilation=dil))
        x = F.batch_norm(x, _t(f"tdnns.{3 * l + 2}.running_mean"), _t(f"tdnns.{3 * l + 2}.running_var"),
                         _t(f"tdnns.{3 * l + 2}.weight"), _t(f"tdnns.{3 * l + 2}.bias"), training=False, eps=1e-5)
        frames.append(x.shape[2])
    assert frames == [289, 285, 279, 279, 279] and x.shape[1] == 1500
    w = F.interpolate(torch.from_numpy(w293.astype(np.float64))[None, None], size=279, mode="nearest")   # [1, 1, 279]
    v1, v2 = w.sum(), (w * w).sum()
    mean = (w * x).sum(dim=2) / v1
    var = (w * (x - mean[:, :, None]) ** 2).sum(dim=2) / (v1 - v2 / v1 + 1e-8)
    stats = torch.cat([mean, torch.sqrt(var)], dim=1)
    return F.linear(stats, _t("embedding.weight"), _t("embedding.bias"))[0].numpy(), stats[0].numpy()


def test_the_reference_equals_torch_float64_operators():
    a = XC.noise(80000, 80000)
    for w in (XC.masks(1, 2, 5)[0, 0], XC.masks(1, 2, 5)[0, 1], XC.one_hot((145,))[0, 0]):
        emb, stats = _R64.embeddings(a, w[None, None], _cache64)
        want_e, want_s = _torch_network(a, w)
        assert np.abs(emb[0, 0] - want_e).max() < 1e-11 and np.abs(stats[0, 0] - want_s).max() < 1e-11
    # the resampling is torch's nearest interpolation, and it never reads fourteen of the 293 frames - 146 and 292 among them
    idx = F.interpolate(torch.arange(293, dtype=torch.float64)[None, None], size=279, mode="nearest")[0, 0].numpy().astype(int)
    assert np.array_equal(idx, (np.arange(279) * 293) // 279)
    unread = sorted(set(range(293)) - set(idx))
    assert unread == list(range(20, 273, 21)) + [292] and 146 in unread and 145 in idx and idx[-1] == 291


def test_table_and_synthetic_weights():
    names = list(diarization.XVECTOR_TENSORS)
    assert len(names) == 45 and names[:13] == [n for n in diarization.vad.PYANNET_TENSORS if n.startswith("sincnet.")]
    assert names[-2:] == ["embedding.weight", "embedding.bias"]
    for dim in XC.DIMS:
        w = diarization.synth_xvector_weights(XC.SEED, dim)
        assert w["embedding.weight"].shape == (dim, 3000) and all(v.dtype == np.float32 for v in w.values())
        assert all(np.array_equal(w[k], _W[k]) for k in names[:-2])          # the network in front of the Linear does not depend on D
    for l in range(5):
        m, v = _W[f"tdnns.{3 * l + 2}.running_mean"], _W[f"tdnns.{3 * l + 2}.running_var"]
        assert np.abs(m).min() > 0 and np.abs(m).mean() > 0.1 and v.min() >= 0.5 and np.abs(v - 1).mean() > 0.1
    with pytest.raises(ValueError):
        diarization.synth_xvector_weights(0, 513)
    # activations stay O(1) through the five blocks
    y = _R64.chunk_tdnn(np.pad(XC.noise(80000, 80000), (0, 0)), _cache64)
    assert 0.2 < np.abs(y).mean() < 5.0


def test_loader_builds_the_filters_and_checks_shapes(tmp_path):
    src = {k: v for k, v in _W.items() if k != "sincnet.conv1d.0.filters"}
    low, band = diarization.vad.mel_cutoffs()
    src.update({diarization.vad.PYANNET_CUTOFFS[0]: low, diarization.vad.PYANNET_CUTOFFS[1]: band,
                "tdnns.2.num_batches_tracked": np.asarray(7)})
    got = diarization.load_xvector_state({"state_dict": src})
    assert list(got) == list(diarization.XVECTOR_TENSORS) and all(np.array_equal(got[k], _W[k]) for k in _W)
    np.savez(tmp_path / "x.npz", **_W)
    assert all(np.array_equal(v, _W[k]) for k, v in diarization.load_xvector_state(str(tmp_path / "x.npz")).items())
    with pytest.raises(ValueError, match="missing"):
        diarization.load_xvector_state({k: v for k, v in _W.items() if k != "tdnns.5.running_var"})
    with pytest.raises(ValueError, match="shape"):
        diarization.load_xvector_state({**_W, "tdnns.3.weight": np.zeros((512, 512, 5), np.float32)})
    with pytest.raises(ValueError, match="one D"):
        diarization.load_xvector_state({**_W, "embedding.bias": np.zeros(191, np.float32)})


def test_float32_cost_on_every_case_is_the_recorded_figure_and_the_tolerance_is_16_times_it():
    r32, cache32 = XR.XVectorRef(_W, np.float32), {}
    worst_e = worst_s = 0.0
    for name, (a, w) in XC.cases().items():
        e64, s64 = _R64.embeddings(a, w, _cache64)
        e32, s32 = r32.embeddings(a, w, cache32)
        re, rs = XC.rel(e32, e64), XC.rel(s32, s64)
        print(f"xvector float32 vs float64, {name}: embeddings {re:.3e} statistics {rs:.3e}")
        worst_e, worst_s = max(worst_e, re), max(worst_s, rs)
    print(f"worst: embeddings {worst_e:.3e} (recorded {XC.F32_EMB:.1e}) statistics {worst_s:.3e} (recorded {XC.F32_STATS:.1e})")
    assert XC.F32_EMB / 4 <= worst_e <= XC.F32_EMB * 1.1 and XC.F32_STATS / 4 <= worst_s <= XC.F32_STATS * 1.1
    assert XC.EMB_TOL == 16 * XC.F32_EMB and XC.STATS_TOL == 16 * XC.F32_STATS


def test_one_hot_rows_are_single_frames_and_unread_frames_are_nan():
    a, w = XC.cases()["one-hot"]
    emb, stats = _R64.embeddings(a, w, _cache64)
    y = _R64.chunk_tdnn(a, _cache64)
    for s, f in enumerate(XC.ONE_HOT + XC.ONE_HOT_READ):
        j = {0: 0, 145: 139, 291: 278}.get(f)
        if j is None:
            assert np.isnan(stats[0, s]).all() and np.isnan(emb[0, s]).all(), f
        else:
            assert np.array_equal(stats[0, s, :1500], y[j]) and not stats[0, s, 1500:].any(), f


@pytest.mark.parametrize("planted", XR.PLANTED)
def test_every_planted_error_lies_ten_tolerances_out(planted):
    a, w = XC.cases()[XC.PLANTED_CASE]
    e64, s64 = _R64.embeddings(a, w, _cache64)
    e, s = XR.XVectorRef(_W, np.float64, planted).embeddings(a, w)
    re, rs = XC.rel(e, e64), XC.rel(s, s64)
    print(f"planted {planted}: embeddings move {re:.3e} ({re / XC.EMB_TOL:.0f} tolerances), statistics {rs:.3e} ({rs / XC.STATS_TOL:.0f})")
    assert re >= 10 * XC.EMB_TOL and rs >= 10 * XC.STATS_TOL
    rec = XC.PLANTED_MOVES[planted]
    assert 0.8 * rec[0] <= re <= 1.25 * rec[0] and 0.8 * rec[1] <= rs <= 1.25 * rec[1]
