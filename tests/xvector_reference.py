"""TEST infrastructure: a numpy restatement of the XVectorSincNet-shaped speaker-embedding network as include/ttasr.h states it
(ttasr_spk_*), with the arithmetic type as a parameter - float64 is the reference the device network is held to, float32 the
same code at the device's precision (its distance from float64 is what the number format itself costs, and the GPU tolerance
is 16 x that: tests/xvector_cases.py).  The front end is pyannet_reference's (the same operators, this network's weights); the
TDNN blocks, the pooling and the Linear have their own loops here.  `planted` names ONE deliberate error, for the tests that
show a wrong network is seen.  Never imported by the product."""
from __future__ import annotations

import hashlib
from typing import Dict, Optional, Tuple

import numpy as np

from pyannet_reference import CHUNK, FRAMES, STEP, PyanNetRef, n_chunks

POOL_FRAMES, STATS = 279, 3000
BLOCKS = ((5, 1), (3, 2), (3, 3), (1, 1), (1, 1))   # (kernel, dilation) of block l; Conv1d tdnns.{3 l}, BatchNorm1d tdnns.{3 l + 2}
BN_EPS = 1e-5
PLANTED = ("no_dilation", "bn_before_lrelu", "biased_variance", "weights_not_resampled", "std_without_sqrt", "mean_std_swapped")


class XVectorRef(PyanNetRef):
    def __init__(self, weights: Dict[str, np.ndarray], dtype=np.float64, planted: Optional[str] = None):
        assert planted is None or planted in PLANTED, planted
        self.dtype = np.dtype(dtype)
        self.w = {k: np.asarray(v, dtype=self.dtype) for k, v in weights.items()}
        self.dim = self.w["embedding.weight"].shape[0]
        self.unbiased = self.pool_before_abs = False
        self.planted = planted

    # -- TDNN blocks: x [frames, channels] ------------------------------------------------------------
    def block(self, x: np.ndarray, l: int) -> np.ndarray:
        taps, dil = BLOCKS[l]
        if self.planted == "no_dilation":
            dil = 1
        w, b = self.w[f"tdnns.{3 * l}.weight"], self.w[f"tdnns.{3 * l}.bias"]          # [out, in, taps]
        t_out = len(x) - (taps - 1) * dil
        y = np.tile(b, (t_out, 1))
        for j in range(taps):
            y = y + x[j * dil:j * dil + t_out] @ np.ascontiguousarray(w[:, :, j].T)
        bn = lambda v: ((v - self.w[f"tdnns.{3 * l + 2}.running_mean"])                # noqa: E731
                        / np.sqrt(self.w[f"tdnns.{3 * l + 2}.running_var"] + self.dtype.type(BN_EPS))
                        * self.w[f"tdnns.{3 * l + 2}.weight"] + self.w[f"tdnns.{3 * l + 2}.bias"])
        return self._lrelu(bn(y)) if self.planted == "bn_before_lrelu" else bn(self._lrelu(y))

    def tdnn(self, x: np.ndarray) -> np.ndarray:
        """[293, 60] -> [279, 1500] (fewer frames under "no_dilation"... the pooling then reads the first 279 it is given)."""
        for l in range(len(BLOCKS)):
            x = self.block(x, l)
        return x[:POOL_FRAMES]

    # -- pooling and embedding ---------------------------------------------------------------------------
    def pool(self, x: np.ndarray, w: np.ndarray) -> np.ndarray:
        """x [279, 1500], w [293] -> [3000]; NaN when the resampled weights sum to 0."""
        t = self.dtype.type
        w = np.asarray(w, dtype=self.dtype)
        wr = w[:len(x)] if self.planted == "weights_not_resampled" else w[(np.arange(len(x)) * FRAMES) // len(x)]
        v1, v2 = wr.sum(), (wr * wr).sum()
        if not v1 > 0:
            return np.full(STATS, np.nan, dtype=self.dtype)
        mean = (wr[:, None] * x).sum(axis=0) / v1
        d = x - mean
        den = v1 if self.planted == "biased_variance" else v1 - v2 / v1 + t(1e-8)
        var = (wr[:, None] * d * d).sum(axis=0) / den
        std = var if self.planted == "std_without_sqrt" else np.sqrt(var)
        return np.concatenate([std, mean] if self.planted == "mean_std_swapped" else [mean, std])

    def embed(self, stats: np.ndarray) -> np.ndarray:
        return stats @ self.w["embedding.weight"].T + self.w["embedding.bias"]

    # -- recordings ----------------------------------------------------------------------------------------
    def chunk_tdnn(self, x80000: np.ndarray, cache: Optional[dict] = None) -> np.ndarray:
        digest = hashlib.sha1(np.ascontiguousarray(x80000, dtype=np.float32).tobytes()).digest()
        if cache is not None and digest in cache:
            return cache[digest]
        y = self.tdnn(self.frontend(x80000))
        if cache is not None:
            cache[digest] = y
        return y

    def embeddings(self, audio: np.ndarray, weights: np.ndarray, cache: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
        """audio [n] float32, weights [K, S, 293] -> (embeddings [K, S, D], pooled statistics [K, S, 3000])."""
        audio = np.asarray(audio, dtype=np.float32)
        k_n = n_chunks(len(audio))
        weights = np.asarray(weights)
        assert weights.shape[0] == k_n and weights.shape[2] == FRAMES, (weights.shape, k_n)
        s_n = weights.shape[1]
        emb = np.zeros((k_n, s_n, self.dim), dtype=self.dtype)
        stats = np.zeros((k_n, s_n, STATS), dtype=self.dtype)
        for k in range(k_n):
            x = np.zeros(CHUNK, dtype=np.float32)
            piece = audio[STEP * k:STEP * k + CHUNK]
            x[:len(piece)] = piece
            y = self.chunk_tdnn(x, cache)
            for s in range(s_n):
                stats[k, s] = self.pool(y, weights[k, s])
                emb[k, s] = self.embed(stats[k, s])
        return emb, stats


_NETS: Dict[tuple, XVectorRef] = {}
_TDNN: Dict[tuple, dict] = {}
_OUT: Dict[tuple, tuple] = {}


def cached_embeddings(seed: int, dim: int, key, audio: np.ndarray, weights: np.ndarray, dtype=np.float64):
    """(embeddings, statistics) of the reference with synthetic weights (seed, dim), computed once per (seed, dim, dtype, key)
    and shared by the tests that need them.  The block-5 output of a chunk does not depend on dim or the masks and is computed
    once per (seed, dtype) and chunk.  The arrays are read-only."""
    from taiwan_tongues_asr_ce_amd import diarization
    net = (int(seed), int(dim), np.dtype(dtype).name)
    if net not in _NETS:
        _NETS[net] = XVectorRef(diarization.synth_xvector_weights(seed, dim), dtype)
    k = net + (key,)
    if k not in _OUT:
        out = _NETS[net].embeddings(audio, weights, _TDNN.setdefault((net[0], net[2]), {}))
        for a in out:
            a.setflags(write=False)
        _OUT[k] = out
    return _OUT[k]
