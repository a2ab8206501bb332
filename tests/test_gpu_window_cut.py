"""GPU: ttasr_log_mel_windows_cut (Engine.log_mel_windows(n_frames=...)) - a window that ends where a clip does.

The cut limits which frames are VALID, not which samples are read: the kept frames are those of the uncut window of the same
seek bit for bit, every later frame is exactly 0.0 in feature space, and the reported maximum covers the kept frames only.
`F` below is the uncut window's frame count, min(the model's window, frames left in the recording)."""
import numpy as np
import pytest

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu

# preset -> frames of the recording: one full window, a second one, and a tail that is no multiple of the kernels' 8- and
# 32-frame tiles; 77 samples more than whole frames
FILE_FRAMES = {"micro": 100 + 100 + 57, "tiny": 3000 + 1500 + 1213}
CASES = [("micro", COMPUTE_F32), ("micro", COMPUTE_BF16), ("tiny", COMPUTE_F32), ("tiny", COMPUTE_BF16)]
NO_FLOOR = -100.0   # floor_max of the un-floored calls: max - 8 lies below log10(1e-10), the smallest value the kernel writes


@pytest.fixture(scope="module", params=CASES, ids=[f"{n}-{'f32' if c == COMPUTE_F32 else 'bf16'}" for n, c in CASES])
def rig(request):
    """(engine, recording, the oracle's whole-file features on the log10 scale, seeks, uncut windows per seek)."""
    from taiwan_tongues_asr_ce_amd.engine import Engine
    name, compute = request.param
    dims = PRESETS[name]
    eng = Engine(dims, compute, 4)
    eng.load_weights(synth.iter_weights(dims))
    n_total = FILE_FRAMES[name]
    audio = synth.noise_clip(7, n_total * 160 + 77)
    feat = R.log_mel_file(audio, dims.n_mels) * 4.0 - 4.0   # un-normalised; its floor never touches a window's maximum
    W = dims.n_frames
    seeks = [0, W // 2 + 3, n_total - W // 3]               # start, mid-file, a window the recording ends before the model's does
    floor = float(feat.max())
    uncut = {}
    for k in seeks:
        mel, mx = eng.log_mel_windows(audio, [k], floor_max=[floor], want_output=True, want_max=True)
        raw, _ = eng.log_mel_windows(audio, [k], floor_max=[NO_FLOOR], want_output=True)
        uncut[k] = (mel[0].copy(), float(mx[0]), raw[0].copy())
    yield dict(eng=eng, audio=audio, feat=feat, seeks=seeks, uncut=uncut, floor=floor, W=W, n_total=n_total)
    eng.close()


def _cuts(F):
    return [1, 2, F - 1, F, F + 5]


def test_cut_window_keeps_the_uncut_frames_and_zeroes_the_rest(rig):
    eng, audio, W = rig["eng"], rig["audio"], rig["W"]
    for k in rig["seeks"]:
        F = min(W, rig["n_total"] - k)
        want, want_mx, raw = rig["uncut"][k]
        for n in _cuts(F):
            kept = min(n, F)
            mel, mx = eng.log_mel_windows(audio, [k], floor_max=[rig["floor"]], want_output=True, want_max=True, n_frames=[n])
            assert np.array_equal(mel[0][:, :kept], want[:, :kept]), (k, n)      # bit for bit, true neighbours beyond the cut
            assert not mel[0][:, kept:].any() and not np.signbit(mel[0][:, kept:]).any(), (k, n)   # exactly +0.0
            # the maximum over the kept frames: of the uncut call's un-floored values (exact: (v + 4) / 4 is monotone and the
            # device applies it in f32 as numpy does here) ...
            assert (np.float32(mx[0]) + np.float32(4.0)) * np.float32(0.25) == raw[:, :kept].max(), (k, n)
            # ... and of the oracle's slice, within test_gpu_parity's mel tolerance (2e-4 on the (x + 4) / 4 scale)
            assert abs(float(mx[0]) - float(rig["feat"][:, k:k + kept].max())) <= 4 * 2e-4, (k, n)
            if kept == F:
                assert np.array_equal(mel[0], want) and float(mx[0]) == want_mx, (k, n)   # a cut at or past the end: the uncut call


def test_cut_window_against_the_oracle_slice(rig):
    """pad_or_trim(features[:, seek:seek + n]) of the whole-file features, at the tolerance of test_gpu_parity's mel test."""
    eng, audio, W = rig["eng"], rig["audio"], rig["W"]
    f = (rig["feat"] + 4.0) * 0.25
    for k in rig["seeks"]:
        F = min(W, rig["n_total"] - k)
        for n in (1, F - 1):
            mel, _ = eng.log_mel_windows(audio, [k], floor_max=[rig["floor"]], want_output=True, n_frames=[n])
            want = R.file_window(f[:, k:k + n], 0, W)
            np.testing.assert_allclose(mel[0], want, atol=2e-4, rtol=0, err_msg=f"seek {k} cut {n}")


def test_rows_of_one_call_are_independent(rig):
    eng, audio, W = rig["eng"], rig["audio"], rig["W"]
    seeks = rig["seeks"]
    cuts = [2, W - 1, 7]   # the last window has fewer than W frames left: 7 cuts it, W - 1 would not
    mel, mx = eng.log_mel_windows(audio, seeks, floor_max=[rig["floor"]] * 3, want_output=True, want_max=True, n_frames=cuts)
    for b, (k, n) in enumerate(zip(seeks, cuts)):
        one, one_mx = eng.log_mel_windows(audio, [k], floor_max=[rig["floor"]], want_output=True, want_max=True, n_frames=[n])
        assert np.array_equal(mel[b], one[0]) and mx[b] == one_mx[0], (k, n)


def test_no_cut_is_the_old_call_and_a_cut_below_one_frame_is_refused(rig):
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    eng, audio, W = rig["eng"], rig["audio"], rig["W"]
    seeks = rig["seeks"]
    old, old_mx = eng.log_mel_windows(audio, seeks, floor_max=[rig["floor"]] * 3, want_output=True, want_max=True)
    new, new_mx = eng.log_mel_windows(audio, seeks, floor_max=[rig["floor"]] * 3, want_output=True, want_max=True, n_frames=[W + 5] * 3)
    assert np.array_equal(old, new) and np.array_equal(old_mx, new_mx)
    for b, k in enumerate(seeks):
        assert np.array_equal(old[b], rig["uncut"][k][0])
    for bad in ([0], [-3]):
        with pytest.raises(TtasrError, match="n_frames"):
            eng.log_mel_windows(audio, [0], n_frames=bad)
    with pytest.raises(TtasrError, match="n_frames"):
        eng.log_mel_windows(audio, seeks, n_frames=[5, 0, 5])
    with pytest.raises(ValueError, match="n_frames"):
        eng.log_mel_windows(audio, seeks, n_frames=[5])
    # the context still works after the refusals
    again, _ = eng.log_mel_windows(audio, [seeks[0]], floor_max=[rig["floor"]], want_output=True)
    assert np.array_equal(again[0], rig["uncut"][seeks[0]][0])
