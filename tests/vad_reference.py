"""TEST infrastructure: a numpy restatement of the Silero-v5-shaped VAD network as include/ttasr.h states it (ttasr_vad_*), with
the arithmetic type as a parameter - float64 is the reference the device network is held to, float32 the same code at the
device's precision (its distance from float64 is what the format itself costs).  Also the suite's VAD test signal.  Never
imported by the product."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

WINDOW, CONTEXT = 512, 64
STRIDES = (1, 2, 2, 1)


class SileroRef:
    """One frame at a time, in `dtype`: `step(frame [1, 576], state [2, 1, 128]) -> (probability, new state)` is what
    vad.silero_speech_prob_fn drives; `probs(audio)` walks a whole recording through the very same `step`."""

    def __init__(self, weights: Dict[str, np.ndarray], dtype=np.float64):
        self.dtype = np.dtype(dtype)
        w = {(k[7:] if k.startswith("_model.") else k): np.asarray(v, dtype=self.dtype) for k, v in weights.items()}
        self.basis = w["stft.forward_basis_buffer"][:, 0, :]                                   # [258, 256]
        self.conv = [(w[f"encoder.{l}.reparam_conv.weight"].reshape(w[f"encoder.{l}.reparam_conv.weight"].shape[0], -1),
                      w[f"encoder.{l}.reparam_conv.bias"], STRIDES[l]) for l in range(4)]       # [O, Cin * 3]: index c * 3 + j
        self.w_ih, self.w_hh = w["decoder.rnn.weight_ih"], w["decoder.rnn.weight_hh"]
        self.b_ih, self.b_hh = w["decoder.rnn.bias_ih"], w["decoder.rnn.bias_hh"]
        self.w_out, self.b_out = w["decoder.decoder.2.weight"][0, :, 0], w["decoder.decoder.2.bias"][0]
        self.last_logit = None

    def encode(self, x: np.ndarray) -> np.ndarray:
        """x [576] -> e [128]: reflect pad, STFT magnitude, four Conv1d + ReLU."""
        x = np.concatenate([x, x[574:510:-1]])                                                 # x[576 + j] = x[574 - j]
        s = self.basis @ np.stack([x[128 * t:128 * t + 256] for t in range(4)], axis=1)        # [258, 4]
        a = np.sqrt(s[:129] ** 2 + s[129:] ** 2)
        for w2, b, stride in self.conv:
            xz = np.pad(a, ((0, 0), (1, 1)))
            t_out = (a.shape[1] - 1) // stride + 1
            cols = np.stack([xz[:, stride * t:stride * t + 3].reshape(-1) for t in range(t_out)], axis=1)
            a = np.maximum(w2 @ cols + b[:, None], 0)
        return a[:, 0]

    def step(self, frame: np.ndarray, state: np.ndarray) -> Tuple[float, np.ndarray]:
        one = self.dtype.type(1)
        sig = lambda v: one / (one + np.exp(-v))
        e = self.encode(np.asarray(frame, dtype=self.dtype).reshape(-1))
        h, c = np.asarray(state[0, 0], dtype=self.dtype), np.asarray(state[1, 0], dtype=self.dtype)
        gates = self.w_ih @ e + self.b_ih + self.w_hh @ h + self.b_hh
        i, f, g, o = gates[:128], gates[128:256], gates[256:384], gates[384:]
        c = sig(f) * c + sig(i) * np.tanh(g)
        h = sig(o) * np.tanh(c)
        logit = self.b_out + self.w_out @ np.maximum(h, 0)
        self.last_logit = logit
        return sig(logit), np.stack([h, c])[:, None, :]

    def probs(self, audio: np.ndarray, return_logits: bool = False):
        """Whole recording: n = ceil(len / 512) frames over the zero-padded signal, 64 samples of context (zeros before sample 0),
        zero state at the start.  -> probabilities [n] in `dtype` (and the pre-sigmoid logits)."""
        audio = np.asarray(audio, dtype=np.float32)
        n = -(-len(audio) // WINDOW)
        padded = np.zeros(CONTEXT + n * WINDOW, dtype=np.float32)
        padded[CONTEXT:CONTEXT + len(audio)] = audio
        state = np.zeros((2, 1, 128), dtype=self.dtype)
        p, l = np.zeros(n, dtype=self.dtype), np.zeros(n, dtype=self.dtype)
        for k in range(n):
            p[k], state = self.step(padded[k * WINDOW:k * WINDOW + CONTEXT + WINDOW][None, :], state)
            l[k] = self.last_logit
        return (p, l) if return_logits else p


def test_signal(seed: int = 0, total_s: float = 40.0, sr: int = 16000) -> np.ndarray:
    """Seeded noise bursts of 1-3 s separated by digital silences of 2.5-4 s, about 40 s, float32 (starts with a silence)."""
    rng = np.random.default_rng([0x7E57, int(seed)])
    parts: List[np.ndarray] = []
    n = 0
    while n < total_s * sr:
        gap = int(rng.uniform(2.5, 4.0) * sr)
        burst = int(rng.uniform(1.0, 3.0) * sr)
        parts += [np.zeros(gap, np.float32), (rng.standard_normal(burst) * rng.uniform(0.08, 0.25)).astype(np.float32)]
        n += gap + burst
    parts.append(np.zeros(int(rng.uniform(2.5, 4.0) * sr), np.float32))
    return np.concatenate(parts)


test_signal.__test__ = False   # a fixture builder, not a test


_CACHE: Dict[tuple, tuple] = {}


def cached_probs(weights_seed: int, key, audio: np.ndarray, dtype=np.float64):
    """(probabilities, logits) of the reference with synthetic weights `weights_seed`, computed once per (seed, key, dtype) and
    shared by the tests that need them; the arrays are read-only."""
    from taiwan_tongues_asr_ce_amd import vad
    k = (int(weights_seed), key, np.dtype(dtype).name)
    if k not in _CACHE:
        p, l = SileroRef(vad.synth_silero_weights(weights_seed), dtype).probs(audio, return_logits=True)
        p.setflags(write=False); l.setflags(write=False)
        _CACHE[k] = (p, l)
    return _CACHE[k]
