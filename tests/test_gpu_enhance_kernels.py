"""GPU: the audio-enhancement kernels (ttasr_enhance, ttasr_enhance_probe, kernels_enhance.hip) against the float64 reference of
tests/enhance_cases.py.

Tolerance (tests/enhance_cases.py): max |device - float64| / max |float64| per output - S, Nf, G and the result before the level
stage through the known-answer hook, the levelled result z through ttasr_enhance - and |device - float64| / float64 for the
level gain, each at most TOL = 16 x 3.1e-6, sixteen times what the float32 run of the reference costs on these very inputs.
Each case prints its measured figures before it asserts."""
import numpy as np
import pytest

import enhance_cases as EC
from taiwan_tongues_asr_ce_amd import dsp
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine

pytestmark = pytest.mark.gpu

_engines = {}
_cases = EC.cases()


def _engine():
    """One micro engine without weights (the call needs none), shared by the tests of this module."""
    if "e" not in _engines:
        _engines["e"] = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    return _engines["e"]


def _run(name):
    audio, flags = _cases[name]
    e = _engine()
    got = e.enhance_probe(audio, flags=flags)
    (z,), g = e.enhance([audio], return_gain=True, flags=flags)
    got["z"], got["g"] = z, float(g[0])
    return got


@pytest.mark.parametrize("name", list(_cases))
def test_device_against_float64(name):
    want = EC.references()[name]
    got = _run(name)
    audio, flags = _cases[name]
    assert got["z"].dtype == np.float32 and got["z"].shape == audio.shape and got["out"].shape == audio.shape
    T = EC.n_frames(len(audio))
    if T:
        for k in ("S", "Nf", "G"):
            assert got[k].shape == (T, EC.BINS) and np.isfinite(got[k]).all(), k
    else:
        assert got["S"] is None and got["Nf"] is None and got["G"] is None
    c = EC.cost(got, want)
    print(f"enhance {name} (flags {flags}): device vs float64 " + " ".join(f"{k} {v:.3e}" for k, v in c.items()) + f"; tolerance {EC.TOL:.2e}")
    assert all(v <= EC.TOL for v in c.values()), (name, c)


def test_shorter_than_a_frame_is_bit_equal_to_its_input():
    audio, _ = _cases["bursts 511"]
    e = _engine()
    assert np.array_equal(e.enhance_probe(audio)["out"], audio)
    for flags in (dsp.DSP_DENOISE, dsp.DSP_HIGHPASS, dsp.DSP_DENOISE | dsp.DSP_HIGHPASS):
        (z,), g = e.enhance([audio], return_gain=True, flags=flags)
        assert np.array_equal(z, audio) and g[0] == 1.0
    # with the level stage: the input times the gain, one float32 product per sample
    (z,), g = e.enhance([audio], return_gain=True, flags=7)
    want = np.float32(min(np.float32(EC.DEFAULTS["peak_target"]) / np.abs(audio).max(), np.float32(EC.DEFAULTS["max_gain"])))
    assert abs(float(g[0]) - float(want)) / float(want) <= EC.TOL and np.array_equal(z, g[0] * audio)


def test_level_gain_below_one_and_at_the_cap():
    e = _engine()
    _, g = e.enhance([_cases["clipped 40000"][0]], return_gain=True)
    assert g[0] < 1.0
    _, g = e.enhance([_cases["quiet 40000"][0]], return_gain=True)
    assert g[0] == np.float32(EC.DEFAULTS["max_gain"])
    z, g = e.enhance([_cases["zeros 40000"][0]], return_gain=True)
    assert g[0] == 1.0 and not z[0].any()


def test_frames_entry_point():
    lib = _engine().lib
    assert [lib.ttasr_enhance_frames(n) for n in (0, 511, 512, 513, 640, 4097, 80000)] == [0, 0, 7, 8, 8, 36, 628]
    assert lib.ttasr_enhance_frames(-1) < 0
