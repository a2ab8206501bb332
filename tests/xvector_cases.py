"""TEST infrastructure: the inputs of the speaker-embedding network's tests, shared by the CPU tests (which measure what float32
costs on exactly these inputs and show the planted errors) and the GPU tests (which hold the device to the float64 reference
on them), and the tolerances that follow.

How the tolerances were obtained (test_xvector_reference_host.py repeats the measurement and fails when it no longer holds):
the float32 run of tests/xvector_reference.py against its float64 run over every case below, as max |difference| / max |float64
value| per case, separately for the embeddings and for the pooled statistics of the known-answer hook; the largest of them is
F32_EMB / F32_STATS.  The GPU tolerance is 16 x that figure (a different f32 summation order; the f32-input MFMA's error is
about 1e-7 x sum |a b|).  Every planted error of xvector_reference.PLANTED moves the float64 reference by at least 10 x the
tolerance on the case PLANTED_CASE (the figures measured are in PLANTED_MOVES)."""
from __future__ import annotations

import numpy as np

SEED = 0
DIMS = (1, 192, 512)
LENGTHS = (1, 79999, 80000, 80001, 88001)
FRAMES = 293
ONE_HOT = (0, 146, 292)        # the frames the issue names; 146 and 292 are read by no pooled frame: their rows are NaN
ONE_HOT_READ = (145, 291)      # their neighbours, which frames 139 and 278 of the 279 read: the middle and the last block-5 frame

# measured on the CPU (float32 numpy against float64 numpy over all cases; see the module text): 2.34e-5 and 2.83e-5, both on
# the case "zeros" - a constant channel's InstanceNorm multiplies the rounding of its mean by 1 / sqrt(eps) = 316; the noise
# cases stay below 1.1e-6 (1.0e-5 for the one-sample recording) - rounded up
F32_EMB, F32_STATS = 2.4e-5, 2.9e-5
EMB_TOL, STATS_TOL = 16 * F32_EMB, 16 * F32_STATS
PLANTED_CASE = "short masks"
# planted error -> (embedding move, statistics move) of the float64 reference on PLANTED_CASE, relative like the tolerances
PLANTED_MOVES = {"no_dilation": (2.0e-1, 1.6e-1), "bn_before_lrelu": (9.0e-1, 7.0e-1), "biased_variance": (4.5e-2, 3.1e-2),
                 "weights_not_resampled": (2.3e-1, 2.0e-1), "std_without_sqrt": (2.3e-1, 1.2e-1), "mean_std_swapped": (2.0, 8.8e-1)}


def noise(n: int, seed: int, level: float = 0.1) -> np.ndarray:
    return (np.random.default_rng([0x5B6A, seed]).standard_normal(n) * level).astype(np.float32)


def masks(k_n: int, s_n: int, seed: int) -> np.ndarray:
    """[K, S, 293] float32 weights >= 0: even masks are runs of ones (a local speaker's frames), odd ones smooth weights."""
    rng = np.random.default_rng([0x3A5C, seed, k_n, s_n])
    w = np.zeros((k_n, s_n, FRAMES), dtype=np.float32)
    for k in range(k_n):
        for s in range(s_n):
            if s % 2 == 0:
                a = int(rng.integers(0, FRAMES - 40))
                w[k, s, a:a + int(rng.integers(20, 200))] = 1.0
            else:
                w[k, s] = rng.uniform(0.0, 1.0, FRAMES) ** 2
    return w


def one_hot(frames) -> np.ndarray:
    w = np.zeros((1, len(frames), FRAMES), dtype=np.float32)
    for s, f in enumerate(frames):
        w[0, s, f] = 1.0
    return w


def n_chunks(n: int) -> int:
    return 0 if n <= 0 else 1 if n <= 80000 else 1 + -(-(n - 80000) // 8000)


def cases() -> dict:
    """name -> (audio, weights [K, S, 293]).  Every length and S of the issue, the special waveforms, the one-hot masks."""
    out = {}
    for n, s_n in zip(LENGTHS, (1, 3, 8, 3, 3)):
        out[f"noise {n}"] = (noise(n, n), masks(n_chunks(n), s_n, n))
    base = noise(80000, 4242)
    special = {
        "zeros": np.zeros(30000, np.float32),
        "constant": np.full(30000, 0.25, np.float32),
        "noise x 1000": base[:40000] * np.float32(1000),
        "noise x 1e-4": base[:40000] * np.float32(1e-4),
        "0.5 + 1e-3 noise": (np.float32(0.5) + np.float32(1e-3) * base / np.float32(0.1)).astype(np.float32),
    }
    for i, (name, a) in enumerate(special.items()):
        out[name] = (a, masks(1, 3, 100 + i))
    short = np.zeros((1, 3, FRAMES), dtype=np.float32)      # a speaker heard for 3 and for 5 frames: where the unbiased
    short[0, 0, 100:103], short[0, 1, 200:205] = 1.0, 1.0   # variance's denominator differs most from the biased one's
    short[0, 2] = masks(1, 1, 77)[0, 0]
    out["short masks"] = (noise(80000, 7), short)
    out["one-hot"] = (noise(80000, 80000), one_hot(ONE_HOT + ONE_HOT_READ))
    return out


def rel(got: np.ndarray, want: np.ndarray) -> float:
    """max |got - want| / max |want| over the entries where `want` is a number; the NaN patterns must agree."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max()) if ok.any() else 0.0
