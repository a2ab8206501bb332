"""The inputs, the float64 reference and the derived bound of the packed alignment pass's cross-attention (test infrastructure,
like xattn_cases.py): tests/test_gpu_align_packed.py runs them on the GPU through the known-answer hook ttasr_align_attn_probe;
tests/test_align_packed_reference_host.py checks on the CPU that this reference and this bound reject the bugs they are there for
and accept float32 arithmetic.

The operands are what the kernel reads: query rows and the resident cross-KV, both already rounded to the engine type.  The
reference is the plain softmax attention in float64; nothing of the kernel's schedule (tiles, moving reference, exp2 units) is in it.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

SEQ_LENS = (2, 31, 32, 33, 128, 129, 224)       # 579 rows: more than one pass's 512, so the probe is called twice
CALLS = ((0, 1, 2, 3, 4), (5, 6))               # indices into SEQ_LENS per probe call (226 and 353 rows)
WINDOWS = (20, 150, 1500)
MANTISSA = {"f32": 23, "bf16": 7, "f16": 10}
N_CLIPS = 3


def rounder(ct: str):
    """float32 -> the values of the engine type (as float32)"""
    if ct == "f32":
        return lambda x: np.ascontiguousarray(x, dtype=np.float32)
    import torch
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[ct]
    return lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dt).to(torch.float32).numpy()


def synthetic_cache(ct: str, T: int, H: int = 6, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """K, V [N_CLIPS][H][T][64] of the engine type for the CPU checks (the GPU test reads the engine's own cache back)"""
    g = np.random.Generator(np.random.Philox(key=990 + seed))
    amp = 2.0 ** ((np.arange(N_CLIPS)[:, None] + np.arange(H)[None, :]) % 3)      # V's scale differs between neighbouring heads and clips
    rnd = rounder(ct)
    K = rnd(g.standard_normal((N_CLIPS, H, T, 64)) * 0.5)
    V = rnd(g.standard_normal((N_CLIPS, H, T, 64)) * amp[:, :, None, None])
    return K, V


def seq_slots(n: int) -> List[int]:
    """cross-KV slot of sequence i: neighbours read different clips, and slot 0 is not the first"""
    return [(i + 1) % N_CLIPS for i in range(n)]


def ulp(x: np.ndarray, ct: str) -> np.ndarray:
    """unit in the last place of the engine type at |x| (0 at 0; fp16 subnormals below 2^-14)"""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    if ct == "f16":
        e = np.maximum(e, -14.0)
    return np.where(a > 0, 2.0 ** (e - MANTISSA[ct]), 0.0)


def make_q(K: np.ndarray, lens: Sequence[int], slots: Sequence[int], rnd, salt: int = 0) -> np.ndarray:
    """Query rows [sum(lens)][H][64] against the cache K [clips][H][T][64], rounded to the engine type by `rnd`.  Even rows of a
    sequence are peaked - q = g K[t*] with the gain that puts most of the mass on frame t*, and t* walks over the first, the last
    and the frames on both sides of every multiple of 32 (tile halves and seams of the 64-key tiles) - odd rows are diffuse.  The
    peak of row r of a sequence differs from its neighbours', from the same row of the next sequence and between heads, so a
    swapped row, a wrong head or a wrong slot moves the peak."""
    _, H, T, _ = K.shape
    frames = sorted({0, T - 1} | {f for m in range(32, T, 32) for f in (m - 1, m)})
    g = np.random.Generator(np.random.Philox(key=4240 + salt))
    rows = []
    for s, (n, slot) in enumerate(zip(lens, slots)):
        q = g.standard_normal((n, H, 64)) * 0.25
        for r in range(0, n, 2):
            for h in range(H):
                t = frames[(r // 2 + 5 * h + 11 * s + salt) % len(frames)]
                k = K[slot, h, t].astype(np.float64)
                q[r, h] = k * (12.0 / max(float(k @ k), 1e-6))        # s[t*] = 12: exp(12) against T - 1 frames near exp(0 .. few)
        rows.append(q)
    return rnd(np.concatenate(rows).astype(np.float32))


def reference(q: np.ndarray, K: np.ndarray, V: np.ndarray, lens: Sequence[int], slots: Sequence[int], ct: str) -> Dict[str, np.ndarray]:
    """float64 attention of packed rows: maps [H][rows][T] = softmax_t(q . k_t), out [rows][H][64] = maps V, and the bounds.

    The bound, per map element p (relative, plus the flush of a float32 exponential below 2^-120):
        |p - ref| <= ref (2 delta + (T + 2 ceil(T / 64)) 2^-24 + 2^-22) + 2^-120
        delta = (65 2^-24 + e16) sum_c |q_c| max_t |k_tc|  +  4 2^-24 max_t |s_t|  +  40 2^-23 + 2^-22
    delta bounds the error of one score in natural units: the 64-term float32 dot product; on the 16-bit engines the query is
    multiplied by log2(e) and rounded to the engine type ONCE before the MFMA (e16 = 2^-(mantissa + 1), 0 in f32); the score is
    kept as an absolute value and the reference subtracted again (four roundings at |s|); the exponent's argument (|s - max| <=
    40) and the hardware exp.  The factor 2: the element's own score and the normalisation, whose sum adds T terms and is
    rescaled at most once per 64-key tile.
    Per output channel: |out - ref| <= ulp_T(ref) / 2 (1 + 2^-6) + (2 delta + e16 + (T + 2 ceil(T / 64)) 2^-24 + 2^-22) max_t |v_tc|
    - the same, the weights rounded to the engine type before the second MFMA (e16), and the output's own rounding."""
    rows, H, _ = q.shape
    T = K.shape[2]
    e16 = 0.0 if ct == "f32" else 2.0 ** -(MANTISSA[ct] + 1)
    maps = np.empty((H, rows, T)); out = np.empty((rows, H, 64)); delta = np.empty((rows, H)); vmax = np.empty((rows, H, 64))
    r0 = 0
    for n, slot in zip(lens, slots):
        qq = q[r0:r0 + n].astype(np.float64)
        k, v = K[slot].astype(np.float64), V[slot].astype(np.float64)
        s = np.einsum("rhc,htc->hrt", qq, k)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        maps[:, r0:r0 + n] = p
        out[r0:r0 + n] = np.einsum("hrt,htc->rhc", p, v)
        sqk = (np.abs(qq) * np.abs(k).max(axis=1)[None]).sum(-1)                      # [n][H]
        delta[r0:r0 + n] = (65 * 2.0 ** -24 + e16) * sqk + 4 * 2.0 ** -24 * np.abs(s).max(-1).T + 40 * 2.0 ** -23 + 2.0 ** -22
        vmax[r0:r0 + n] = np.abs(v).max(axis=1)[None]
        r0 += n
    acc = (T + 2 * -(-T // 64)) * 2.0 ** -24 + 2.0 ** -22
    map_bound = maps * (2 * delta.T[:, :, None] + acc) + 2.0 ** -120
    out_bound = ulp(out, ct) / 2 * (1 + 2.0 ** -6) + (2 * delta[..., None] + e16 + acc) * vmax
    return dict(maps=maps, out=out, map_bound=map_bound, out_bound=out_bound)


def ratio(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    """largest |got - want| / bound; above 1 = flagged"""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.nan_to_num(r, nan=np.inf).max())


def check(out: np.ndarray, maps: np.ndarray, head_pair: Sequence[int], ref: Dict[str, np.ndarray]) -> Tuple[float, float]:
    """(output ratio, map ratio) of a probe result: out [rows][H * 64], maps [n_pairs][rows][T] with head h in maps[head_pair[h]]"""
    rows, H, _ = ref["out"].shape
    r_out = ratio(out.reshape(rows, H, 64), ref["out"], ref["out_bound"])
    r_map = 0.0
    for h, p in enumerate(head_pair):
        if p >= 0:
            r_map = max(r_map, ratio(maps[p], ref["maps"][h], ref["map_bound"][h]))
    return r_out, r_map


def f32_attention(q: np.ndarray, K: np.ndarray, V: np.ndarray, lens: Sequence[int], slots: Sequence[int], n_ctx: int = 0,
                  stale: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The arithmetic restated in np.float32, one operation at a time: a 64-term dot product, exp(s - max), the sum over the
    frames, one division -> (out [rows][H * 64], maps [H][rows][T]).  Two of the bugs the reference is there for can be switched
    on: n_ctx > 0 reads the cache of a LONGER window (K, V hold more than n_ctx frames) and lets frame n_ctx into the sums
    although only n_ctx frames are returned - the clamped key of a last tile reaching a map; stale = the rows are normalised
    with the maximum of the first 64 frames instead of the final one (an online softmax whose reference moved but whose stored
    scores were not rescaled)."""
    rows, H, _ = q.shape
    T = n_ctx or K.shape[2]
    T_read = T + 1 if n_ctx else T
    out = np.empty((rows, H, 64), np.float32); maps = np.empty((H, rows, T), np.float32)
    r0 = 0
    for n, slot in zip(lens, slots):
        qq = q[r0:r0 + n].astype(np.float32)
        k, v = K[slot, :, :T_read].astype(np.float32), V[slot, :, :T_read].astype(np.float32)
        s = np.zeros((H, n, T_read), np.float32)
        for c in range(64):
            s = s + qq[:, :, c].T[:, :, None] * k[:, None, :, c]
        m = s.max(-1, keepdims=True)
        p = np.exp(s - m).astype(np.float32)
        den = np.zeros((H, n), np.float32)
        for t in range(T_read):
            den = den + p[:, :, t]
        if stale and T > 64:
            m0 = s[:, :, :64].max(-1, keepdims=True)
            p = np.exp(np.minimum(s - m0, 60.0)).astype(np.float32)           # scores against the first tile's reference ...
        w = (p / den[..., None]).astype(np.float32)                           # ... divided by the sum against the final one
        maps[:, r0:r0 + n] = w[:, :, :T]
        out[r0:r0 + n] = np.einsum("hrt,htc->rhc", w, v).astype(np.float32)
        r0 += n
    return out.reshape(rows, H * 64), maps
