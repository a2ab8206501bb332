"""TEST infrastructure: the audio enhancement's definition as a float64 numpy reference, its float32 restatement, the inputs of
its tests - shared by the CPU tests (which measure what float32 costs on exactly these inputs and show the planted errors) and
the GPU tests (which hold the device to the float64 reference on them) - and the tolerance that follows.

The definition (this project's own; include/ttasr.h states it as well).  Input x[0..L) float32 mono 16 kHz, output z[0..L).
N = 512, hop 128, bins 0..256, window w[n] = sin(pi (n + 0.5) / N) for analysis and synthesis.  L < N: out = x; only the level
stage may apply.
  1. T = ceil(L / 128) + 3 frames; frame t reads samples t 128 - 384 + n, reflected without repeating the edge
  2. X = DFT of the windowed frame, P = |X|^2
  3. S = box mean of P along t with radius 2, Q with radius 16; clipped to [0, T - 1], divided by the frames summed
  4. M[b] = min of Q over block b of 32 frames; Nf[t] = oversubtract * min of M over the blocks within 6 of floor(t / 32), clipped
  5. DENOISE: G = max(1 - Nf / S, 0) where S > 0, else 0; then max(G, 10^(-strength_db / 20)).  Otherwise G = 1
  6. HIGHPASS: G[t, 0] = G[t, 1] = 0
  7. y_t = w * irfft(G X); out[s] = 0.5 * the sum over the four frames that hold s, ascending t
  8. LEVEL: p = max |out|, g = 1 if p == 0 else min(peak_target / p, max_gain), z = g out

How the tolerance was obtained (test_enhance_reference_host.py repeats the measurement and fails when it no longer holds): the
float32 run of chain() against its float64 run over every case of cases(), as max |difference| / max |float64 value| per
output (S, Nf, G, out, z) and |difference| / g for the level gain; the largest of them all is F32_COST.  The GPU tolerance is
16 x that figure, the project's precedent: numpy's FFT and the kernels' direct DFT round differently."""
from __future__ import annotations

import numpy as np

N, HOP, BINS = 512, 128, 257
DENOISE, HIGHPASS, LEVEL = 1, 2, 4
DEFAULTS = dict(strength_db=12.0, oversubtract=3.0, peak_target=10.0 ** (-1.0 / 20.0), max_gain=10.0)
LENGTHS = (511, 512, 513, 640, 4097, 40000, 80000)   # 40 000: 10 blocks, both clips of the block window meet; 80 000: 20, a free interior
FLAG_CASE = "bursts 4097"                            # the case every flag combination runs on

# measured on the CPU (float32 numpy against float64 numpy over all cases and outputs; see the module text): 3.083e-6, on the
# output G of the case "rumble 40000" - G = 1 - Nf / S turns the rounding of two spectra into an absolute error - while S and Nf
# stay below 2.0e-7, out and z below 2.9e-7 and the level gain below 1.2e-7; rounded up.  The figure belongs to numpy 2.2.6:
# numpy >= 2 transforms float32 input in single precision (pocketfft); an older numpy transforms in float64 and would measure the
# rounding of the result alone, so the float32 run refuses it (single_precision_fft)
F32_COST = 3.1e-6
TOL = 16 * F32_COST

# planted error -> how far it moves the float64 reference's `out` on PLANTED_CASE, relative like the tolerance (measured by
# test_enhance_reference_host.py, which holds each to at least 10 x TOL)
PLANTED = ("zero_padding", "radius2_tracker", "unclipped_block_window", "no_half", "unclipped_divisor")
PLANTED_CASE = "bursts 40000"


def single_precision_fft() -> bool:
    """numpy's FFT keeps float32 (numpy >= 2): what the float32 restatement and F32_COST rest on."""
    return np.fft.rfft(np.zeros(8, np.float32)).dtype == np.complex64


def n_frames(n: int) -> int:
    return 0 if n < N else -(-n // HOP) + 3


def window(dtype=np.float64) -> np.ndarray:
    return np.sin(np.pi * (np.arange(N, dtype=np.float64) + 0.5) / N).astype(dtype)


def _box(P: np.ndarray, radius: int, clip_divisor: bool = True) -> np.ndarray:
    """Box mean along axis 0 over [t - radius, t + radius] clipped to the array, u ascending, divided by the frames summed."""
    T = P.shape[0]
    acc = np.zeros_like(P)
    cnt = np.zeros(T, dtype=P.dtype)
    for d in range(-radius, radius + 1):
        lo, hi = max(0, -d), min(T, T - d)     # the t for which t + d exists
        if lo < hi:
            acc[lo:hi] += P[lo + d:hi + d]
            cnt[lo:hi] += 1
    if not clip_divisor:
        cnt[:] = 2 * radius + 1
    return acc / cnt[:, None]


def chain(x, flags: int, strength_db=DEFAULTS["strength_db"], oversubtract=DEFAULTS["oversubtract"],
          peak_target=DEFAULTS["peak_target"], max_gain=DEFAULTS["max_gain"], dtype=np.float64, planted: str | None = None,
          highpass_bins: int = 2) -> dict:
    """The definition in `dtype` arithmetic (float64: THE reference; float32: the restatement the tolerance is measured with).
    Returns S, Nf, G [T, 257] (None when L < N), out (before the level stage), z and g.  planted: one of PLANTED.  highpass_bins:
    the definition zeroes 2; the host test shows what a third would cost."""
    f = np.dtype(dtype).type
    cdtype = np.complex128 if dtype == np.float64 else np.complex64
    if dtype != np.float64 and not single_precision_fft():
        raise RuntimeError(f"numpy {np.__version__} transforms float32 input in float64: the float32 restatement needs numpy >= 2")
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    L = len(x)
    S = Nf = G = None
    if L < N:
        out = x.copy()
    else:
        T = n_frames(L)
        w = window(dtype)
        s = np.arange(T)[:, None] * HOP - 384 + np.arange(N)[None, :]
        if planted == "zero_padding":
            fr = np.where((s >= 0) & (s < L), x[np.clip(s, 0, L - 1)], f(0))
        else:
            s = np.where(s < 0, -s, s)
            s = np.where(s >= L, 2 * (L - 1) - s, s)
            fr = x[s]
        X = np.fft.rfft(fr * w, axis=1).astype(cdtype)
        P = (X.real * X.real + X.imag * X.imag).astype(dtype)
        clip_div = planted != "unclipped_divisor"
        S = _box(P, 2, clip_div)
        Q = _box(P, 2 if planted == "radius2_tracker" else 16, clip_div)
        NB = -(-T // 32)
        Qp = np.full((NB * 32, BINS), np.inf, dtype=dtype)
        Qp[:T] = Q
        M = Qp.reshape(NB, 32, BINS).min(axis=1)
        pad = f(0) if planted == "unclipped_block_window" else f(np.inf)   # the blocks a window without clipping would read
        Mp = np.full((NB + 12, BINS), pad, dtype=dtype)
        Mp[6:6 + NB] = M
        Mw = np.min(np.stack([Mp[i:i + NB] for i in range(13)]), axis=0)
        Nf = (f(oversubtract) * Mw[np.arange(T) // 32]).astype(dtype)
        if flags & DENOISE:
            with np.errstate(divide="ignore", invalid="ignore"):
                G = np.where(S > 0, np.maximum(f(1) - Nf / np.where(S > 0, S, f(1)), f(0)), f(0)).astype(dtype)
            G = np.maximum(G, f(10.0 ** (-float(strength_db) / 20.0)))
        else:
            G = np.ones((T, BINS), dtype=dtype)
        if flags & HIGHPASS:
            G[:, :highpass_bins] = 0
        y = (np.fft.irfft((G * X).astype(cdtype), n=N, axis=1).astype(dtype) * w).astype(dtype)
        full = np.zeros((T - 1) * HOP + N, dtype=dtype)
        for t in range(T):   # ascending t
            full[t * HOP:t * HOP + N] += y[t]
        out = ((f(1) if planted == "no_half" else f(0.5)) * full[384:384 + L]).astype(dtype)
    g = f(1)
    if flags & LEVEL:
        p = np.abs(out).max() if L else f(0)
        g = f(1) if p == 0 else min(f(peak_target) / p, f(max_gain))
    return dict(S=S, Nf=Nf, G=G, out=out, z=(f(g) * out).astype(dtype), g=float(g))


def reference(x, flags: int = 7, **params) -> dict:
    return chain(x, flags, dtype=np.float64, **params)


# ---- signals -------------------------------------------------------------------------------------------------------------

def _rng(seed: int):
    return np.random.default_rng([0xD5B0, seed])


def bursts(n: int, seed: int = 1, noise: float = 0.02, amp: float = 0.3) -> np.ndarray:
    """Harmonic tone bursts (a 140 Hz fundamental with five partials, 0.25 s on / 0.25 s off) in white noise."""
    t = np.arange(n) / 16000.0
    tone = sum(np.sin(2 * np.pi * 140.0 * h * t + h) / h for h in range(1, 7))
    gate = ((t % 0.5) < 0.25).astype(np.float64)
    return (amp * gate * tone / 2.0 + noise * _rng(seed).standard_normal(n)).astype(np.float32)


def rumble(n: int) -> np.ndarray:
    """DC plus 30 Hz rumble under a quieter burst signal: what the high-pass stage is for."""
    t = np.arange(n) / 16000.0
    return (0.2 + 0.25 * np.sin(2 * np.pi * 30.0 * t) + 0.3 * bursts(n, 2)).astype(np.float32)


def silence_mid(n: int) -> np.ndarray:
    """Digital silence in the middle third: the S = 0 branch, and block minima of exactly 0."""
    a = bursts(n, 3).copy()
    a[n // 3:2 * n // 3] = 0
    return a


def clipped(n: int) -> np.ndarray:
    """A recording driven into the rails: full scale, so the level gain is below 1."""
    return np.clip(8.0 * bursts(n, 4), -1.0, 1.0).astype(np.float32)


def quiet(n: int) -> np.ndarray:
    """Peak 1e-4: the level gain hits the max_gain cap."""
    a = bursts(n, 5).astype(np.float64)
    return (a * (1e-4 / np.abs(a).max())).astype(np.float32)


def cases() -> dict:
    """name -> (audio, flags).  Every length of LENGTHS on the burst signal, the special signals at 40 000 samples (digital
    silence at 80 000 as well), every flag combination on FLAG_CASE."""
    out = {f"bursts {n}": (bursts(n, 10 + i), 7) for i, n in enumerate(LENGTHS)}
    out["rumble 40000"] = (rumble(40000), 7)
    out["silence 40000"] = (silence_mid(40000), 7)
    out["silence 80000"] = (silence_mid(80000), 7)
    out["zeros 40000"] = (np.zeros(40000, np.float32), 7)
    out["clipped 40000"] = (clipped(40000), 7)
    out["quiet 40000"] = (quiet(40000), 7)
    base = out[FLAG_CASE][0]
    for flags in range(1, 7):
        out[f"{FLAG_CASE} flags {flags}"] = (base, flags)
    return out


_REFERENCES: dict = {}


def references() -> dict:
    """name -> the float64 reference of the case, computed once per process and shared (do not modify)."""
    if not _REFERENCES:
        for name, (a, flags) in cases().items():
            _REFERENCES[name] = reference(a, flags)
    return _REFERENCES


def rel(got, want) -> float:
    """max |got - want| / max |want|; where the reference is all zeros the result must be so too (0.0 or inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    top = np.abs(want).max()
    err = np.abs(got - want).max()
    if top == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / top)


def cost(got: dict, want: dict) -> dict:
    """The relative error of every output of a run against the reference's."""
    out = {k: rel(got[k], want[k]) for k in ("S", "Nf", "G", "out", "z") if want[k] is not None and got.get(k) is not None}
    out["g"] = abs(got["g"] - want["g"]) / want["g"]
    return out
