"""The inputs, the case list, the two-tier comparison and the emulations of the encoder attention kernel tests (test infrastructure,
like xattn_cases.py, whose rnd / ulp / error_ratio are reused): tests/test_gpu_enc_attn_kernels.py runs the cases on the GPU through
the known-answer hook ttasr_enc_attn_probe; tests/test_enc_attn_reference_host.py shows on the CPU that these very inputs and
bounds pass every legal implementation of the kernels' arithmetic and flag the listed bugs.

Kernels: enc_attn_flash_kernel<T, false, 2 | 1> (encoder self-attention, 64 | 32 queries per wave), enc_attn_flash_kernel<T, true, 1>
(the cross-attention of many rows per clip, chosen by launch_cross_attn_decode from 32 rows per clip upward) and
enc_attn_simple_kernel<T> (option flash = 0; the f32 engine's only encoder attention).

All operands are one scene per geometry: Q [B][H][Tq][64], K and V [B][H][Tk][64] (the self form interleaves them into qkv with
Tq = Tk), every value exactly representable in bf16 AND fp16, so every engine type sees the same numbers."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from xattn_cases import SIG_TYPE, error_ratio, rnd, ulp  # noqa: F401  (rnd / ulp know bf16 and f16; f32 is handled here)

TYPES16 = ("bf16", "f16")
TYPES = TYPES16 + ("f32",)
KB = 64                                   # keys per tile of both kernels
SELF_T = (1, 20, 64, 65, 127, 128, 129, 150, 192, 257)
FULL_T = 1500
SELF_BH = ((1, 8), (2, 4), (3, 3), (1, 5))           # B H % 8 == 0 twice (the XCD remap), twice not (the plain order)
CROSS_NQ = (31, 32, 33, 128, 129, 160)
CROSS_TK = (20, 64, 150)
CROSS_BH = ((1, 8), (3, 3))                            # 1 clip (remap) and 3 clips (plain order)
CROSS_FULL = (447, 1500)
CROSS_MIN_ROWS = 32                                    # launch_cross_attn_decode: kv_div >= 32 takes the flash kernel
MAX_BATCH = 3
HEADS = tuple(sorted({h for _, h in SELF_BH}))
HALF_ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}      # u: relative rounding error of the storage type
LOG2E_F32 = np.float32(1.4426950408889634)
FA_THR = 6.0                              # kernels_flash.hip: the lazy reference moves when a tile's maximum exceeds it by more


def dims(H: int):
    from taiwan_tongues_asr_ce_amd.config import WhisperDims
    return WhisperDims(f"encattn-h{H}", 80, 1500, 64 * H, H, 64, 1, 2, 531, 448)


def sig_type(ct: str) -> str:
    return "float" if ct == "f32" else SIG_TYPE[ct]


def ulp_t(x: np.ndarray, ct: str) -> np.ndarray:
    if ct != "f32":
        return ulp(x, ct)
    a = np.abs(np.asarray(x, np.float64))
    e = np.maximum(np.floor(np.log2(np.where(a > 0, a, 1.0))), -126.0)
    return np.where(a > 0, 2.0 ** (e - 23), 0.0)


def rnd_t(x: np.ndarray, ct: str) -> np.ndarray:
    return np.asarray(x, np.float32) if ct == "f32" else rnd(x, ct)


# ---- the scene ----------------------------------------------------------------------------------------------------------------
# K channel 62 is the constant 32 / 64 and channel 63 a staircase 4 (j - n_tiles // 2) / 64 over the 64-key tiles j, both times the
# block's power of two: a query can then put a common offset on every score (channel 62) or make the tile maxima climb (63).
ROW_KINDS = ("peaked", "diffuse", "rising", "offset", "flat")


def amp_k(b: int, h: int) -> float:
    return 2.0 ** -((b + 2 * h) % 3)


def amp_v(b: int, h: int) -> float:
    return 2.0 ** -((b + 2 * h + 1) % 3)


def peak_frames(Tk: int) -> List[int]:
    """frame 0, Tk - 1, Tk - 2 and both sides of every multiple of 16 (hence the first and last key of every 64-key tile, the last
    valid key of the masked tile and the key before it)"""
    s = {0, Tk - 1, max(Tk - 2, 0)}
    for m in range(16, Tk, 16):
        s.update((m - 1, m))
    return sorted(s)


def row_kind(b: int, h: int, t: int) -> str:
    r = t % 8
    if r in (0, 2, 4):
        return "peaked"
    if r == 6:
        return ROW_KINDS[2 + (t // 8 + h + b) % 3]
    return "diffuse"


@dataclass
class Scene:
    Q: np.ndarray          # float32 [B][H][Tq][64]
    K: np.ndarray          # float32 [B][H][Tk][64]
    V: np.ndarray
    kind: np.ndarray       # [B][H][Tq] index into ROW_KINDS
    tstar: np.ndarray      # [B][H][Tq] peaked frame or -1


@lru_cache(maxsize=None)
def scene(B: int, H: int, Tq: int, Tk: int) -> Scene:
    g = np.random.Generator(np.random.Philox(key=13000 + 7 * Tk + Tq))
    n_tiles = (Tk + KB - 1) // KB
    Ki = g.integers(-64, 65, size=(B, H, Tk, 64)).astype(np.float64)
    Vi = g.integers(-64, 65, size=(B, H, Tk, 64)).astype(np.float64)
    Ki[..., 62] = 32
    Ki[..., 63] = 4 * (np.arange(Tk) // KB - n_tiles // 2)
    ak = np.array([[amp_k(b, h) for h in range(H)] for b in range(B)])
    av = np.array([[amp_v(b, h) for h in range(H)] for b in range(B)])
    K = Ki / 64 * ak[:, :, None, None]
    V = Vi / 64 * av[:, :, None, None]
    Q = g.integers(-16, 17, size=(B, H, Tq, 64)).astype(np.float64) / 64
    small = g.integers(-4, 5, size=(B, H, Tq, 64)).astype(np.float64) / 64
    kind = np.empty((B, H, Tq), np.int64)
    tstar = np.full((B, H, Tq), -1, np.int64)
    frames = peak_frames(Tk)
    i = 0
    for b in range(B):
        for h in range(H):
            k = K[b, h]
            for t in range(Tq):
                rk = row_kind(b, h, t)
                kind[b, h, t] = ROW_KINDS.index(rk)
                if rk == "peaked":
                    ts = (0, Tk - 1, max(Tk - 2, 0))[i] if i < 3 else frames[(i + Tq) % len(frames)]
                    i += 1
                    s = k @ k[ts]
                    gap = np.delete(s[ts] - s, ts)
                    for m in range(-8, 9):
                        if 1.0 / (1.0 + np.exp(-(2.0 ** m) * gap).sum()) >= 0.93:
                            break
                    else:
                        raise AssertionError(f"no scale makes frame {ts} of (b {b}, head {h}) hold 0.93 of the mass")
                    Q[b, h, t] = 2.0 ** m * k[ts]
                    tstar[b, h, t] = ts
                elif rk == "rising":      # 8 natural units = 11.5 exp2 units per tile from the staircase, small noise on top
                    Q[b, h, t] = small[b, h, t]
                    Q[b, h, t, 62] = 0
                    Q[b, h, t, 63] = 128 / ak[b, h]
                elif rk == "offset":      # every score moves by -256 x 0.5 = -128 natural units = -184.7 exp2 units
                    Q[b, h, t, 62] = -256 / ak[b, h]
                    Q[b, h, t, 63] = 0
                elif rk == "flat":        # every score is 4 x 0.5 = 2: the answer is the plain mean of V
                    Q[b, h, t] = 0
                    Q[b, h, t, 62] = 4 / ak[b, h]
    out = Scene(Q.astype(np.float32), K.astype(np.float32), V.astype(np.float32), kind, tstar)
    for x in (out.Q, out.K, out.V):
        assert np.array_equal(rnd(x, "bf16"), x) and np.array_equal(rnd(x, "f16"), x)
    return out


def qkv_of(sc: Scene) -> np.ndarray:
    """the self form's operand: [B][T][3 d_model], q | k | v per row, head h in channels [64 h, 64 h + 64)"""
    B, H, T, _ = sc.Q.shape
    parts = [x.transpose(0, 2, 1, 3).reshape(B, T, 64 * H) for x in (sc.Q, sc.K, sc.V)]
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def q_rows_of(sc: Scene) -> np.ndarray:
    B, H, T, _ = sc.Q.shape
    return np.ascontiguousarray(sc.Q.transpose(0, 2, 1, 3).reshape(B, T, 64 * H))


def heads_of(out: np.ndarray, H: int) -> np.ndarray:
    """kernel output [B][T][64 H] -> [B][H][T][64]"""
    B, T, _ = out.shape
    return out.reshape(B, T, H, 64).transpose(0, 2, 1, 3)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    form: str                               # self | cross
    ct: str
    variant: str                            # qw2 | qw1 | plain | default (f32 with no option set) | cross
    B: int
    H: int
    Tq: int
    Tk: int

    @property
    def opts(self) -> Dict[str, int]:
        return {"qw2": {"flash": 1, "flash_qw": 2}, "qw1": {"flash": 1, "flash_qw": 1}, "plain": {"flash": 0, "flash_qw": 2},
                "default": {"flash": 1, "flash_qw": 2}, "cross": {"flash": 1, "flash_qw": 2}}[self.variant]

    @property
    def arithmetic(self) -> str:
        """flash | plain (enc_attn_simple_kernel) | decode (the decode step's kernels, below 32 rows per clip)"""
        if self.form == "cross":
            return "flash" if self.Tq >= CROSS_MIN_ROWS else "decode"
        return "flash" if self.variant in ("qw2", "qw1") else "plain"

    @property
    def name(self) -> str:
        return f"{self.form}-{self.ct}-{self.variant}-B{self.B}H{self.H}-q{self.Tq}-k{self.Tk}"

    @property
    def group(self) -> Tuple[str, str]:
        return (f"{self.form}/{self.variant}" + ("/decode" if self.arithmetic == "decode" else ""), self.ct)


VARIANTS = {"bf16": ("qw2", "qw1", "plain"), "f16": ("qw2", "qw1", "plain"), "f32": ("plain", "default")}


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    t: List[Case] = []
    for ct in TYPES:
        for var in VARIANTS[ct]:
            for T in SELF_T:
                for B, H in SELF_BH:
                    t.append(Case("self", ct, var, B, H, T, T))
        t.append(Case("self", ct, "qw2" if ct != "f32" else "default", 1, 8 if ct != "f32" else 5, FULL_T, FULL_T))
    for ct in TYPES16:
        for nq in CROSS_NQ:
            for Tk in CROSS_TK:
                for B, H in CROSS_BH:
                    t.append(Case("cross", ct, "cross", B, H, nq, Tk))
        t.append(Case("cross", ct, "cross", 1, 8, *CROSS_FULL))
    return tuple(t)


def expected_signature(c: Case) -> Optional[str]:
    """the signature the hook must report; None for the cross form below 32 rows per clip: anything but the flash kernel"""
    T = sig_type(c.ct)
    if c.form == "cross":
        return f"enc_attn_flash_kernel<{T}, true, 1> clips {c.B} rows {c.Tq}" if c.Tq >= CROSS_MIN_ROWS else None
    if c.arithmetic == "flash":
        qw = 2 if c.variant == "qw2" else 1
        return f"enc_attn_flash_kernel<{T}, false, {qw}> grid {-(-c.Tq // (128 * qw)) * c.H * c.B * 256}"
    return f"enc_attn_simple_kernel<{T}> grid {-(-c.Tq // 16) * c.H * c.B * 256}"


def sig_ok(sig: str, c: Case) -> bool:
    want = expected_signature(c)
    return sig == want if want is not None else bool(sig) and not sig.startswith("enc_attn_flash_kernel")


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def q_stated(Q: np.ndarray, ct: str) -> np.ndarray:
    """the flash kernel's query operand: q times log2(e) in float32, rounded to the storage type (exp2 units)"""
    return rnd_t(np.asarray(Q, np.float32) * LOG2E_F32, ct).astype(np.float64)


def _softmax_v(S: np.ndarray, V: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """S [.., Tq, Tk] natural units, V [.., Tk, 64] -> (out, sum_t w_t |v_tc|), float64"""
    p = np.exp(S - S.max(-1, keepdims=True))
    w = p / p.sum(-1, keepdims=True)
    return w @ V, w @ np.abs(V)


def references(sc: Scene, ct: str, arithmetic: str) -> Dict[str, Dict[str, np.ndarray]]:
    """Both tiers for a scene, per output element [B][H][Tq][64], against float64:
        bound = ulp_T(ref) / 2 (1 + 2^-6) + (2 delta + Tk 2^-24 + 2^-21 [+ Tk 2^-25: fp16 flash]) max_t |v_tc| [+ u sum_t w_t |v_tc|: flash]
      tier A (the operation): ref = softmax(q k) v on the given q;
              flash: delta = (u + 66 2^-24) sqk + 2^-22, sqk = sum_c |q_c| max_t |k_tc|; plain / decode: delta = 66 2^-24 sqk + 2^-22
      tier B (the flash kernel's stated arithmetic): ref = softmax(ln 2 q' k) v, q' = round_T(float32(q) float32(log2 e));
              delta = 2 x 66 2^-24 sqk' + 2^-22, sqk' = sum_c |q'_c| max_t |k_tc|"""
    Q, K, V = sc.Q.astype(np.float64), sc.K.astype(np.float64), sc.V.astype(np.float64)
    Tk = K.shape[2]
    u = HALF_ULP[ct]
    flash = arithmetic == "flash"
    kmax = np.abs(K).max(axis=2)[:, :, None, :]                     # [B][H][1][64]
    vmax = np.abs(V).max(axis=2)[:, :, None, :]
    f32 = Tk * 2.0 ** -24 + 2.0 ** -21 + (Tk * 2.0 ** -25 if flash and ct == "f16" else 0.0)

    def tier(q: np.ndarray, scale: float, delta_of) -> Dict[str, np.ndarray]:
        ref, wv = _softmax_v(scale * (q @ K.transpose(0, 1, 3, 2)), V)
        sqk = (np.abs(q) * kmax).sum(-1, keepdims=True)             # [B][H][Tq][1]
        bound = ulp_t(ref, ct) / 2 * (1 + 2.0 ** -6) + (2 * delta_of(sqk) + f32) * vmax + (u * wv if flash else 0.0)
        return dict(ref=ref, bound=bound, sqk=sqk[..., 0])
    out = {"A": tier(Q, 1.0, lambda s: ((u if flash else 0.0) + 66 * 2.0 ** -24) * s + 2.0 ** -22)}
    if flash:
        out["B"] = tier(q_stated(sc.Q, ct), float(np.log(2.0)), lambda s: 2 * 66 * 2.0 ** -24 * s + 2.0 ** -22)
    return out


def ratios(out: np.ndarray, refs: Dict[str, Dict[str, np.ndarray]]) -> Dict[str, float]:
    return {tier: error_ratio(out, r) for tier, r in refs.items()}


def worst_element(out: np.ndarray, ref: Dict[str, np.ndarray]) -> str:
    """'b h query channel: got, want, bound' of the element with the largest error / bound"""
    err = np.abs(out.astype(np.float64) - ref["ref"])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.nan_to_num(np.where(ref["bound"] > 0, err / ref["bound"], np.where(err > 0, np.inf, 0.0)), nan=np.inf)
    b, h, t, c = np.unravel_index(int(np.argmax(r)), r.shape)
    return f"batch {b} head {h} query {t} channel {c}: got {out[b, h, t, c]!r}, want {ref['ref'][b, h, t, c]!r}, bound {ref['bound'][b, h, t, c]:.3g}"


# ---- emulations -----------------------------------------------------------------------------------------------------------------
MUTATIONS = ("drop_key", "double_key", "mask_plus", "mask_minus", "swap_v_63_64", "k_chunk_xor", "swap_heads", "swap_kv",
             "move_o_not_l", "move_twice", "first_tile_rescale", "block1_to_block0", "last_query_unwritten")


def _mutate_operands(K: np.ndarray, V: np.ndarray, mut: Optional[str]) -> Tuple[np.ndarray, np.ndarray]:
    Tk = K.shape[2]
    if mut == "swap_v_63_64" and Tk > 64:
        V = V.copy(); V[:, :, [63, 64]] = V[:, :, [64, 63]]
    elif mut == "k_chunk_xor":         # 16-byte chunk c of a key row read as c ^ 1 for the odd row pairs of the LDS image
        odd = ((np.arange(Tk) % KB) >> 1) & 1 == 1
        perm = (np.arange(64) // 8 ^ 1) * 8 + np.arange(64) % 8
        K = K.copy(); K[:, :, odd] = K[:, :, odd][..., perm]
    elif mut == "swap_heads":
        order = np.arange(K.shape[1]); order[[0, 1]] = order[[1, 0]]
        K, V = K[:, order], V[:, order]
    elif mut == "swap_kv":
        K, V = V, K
    return K, V


def emulate_flash(sc: Scene, ct: str, lazy: bool = True, mut: Optional[str] = None, qw: int = 2) -> np.ndarray:
    """The flash kernel's arithmetic in float64 with the roundings the kernel states: q' = round_T(q log2 e), tiles of 64 keys, the
    reference maximum either lazy (moves when a tile's maximum exceeds it by more than 6 exp2 units; the first tile sets it) or
    the running maximum, l sums the unrounded p, the PV product takes p rounded to the storage type, one division, the result
    rounded to the storage type.  mut: one of MUTATIONS.  Returns [B][H][Tq][64] float32 (NaN where nothing is written)."""
    K, V = _mutate_operands(sc.K.astype(np.float64), sc.V.astype(np.float64), mut)
    q = q_stated(sc.Q, ct)
    B, H, Tq, _ = q.shape
    Tk = K.shape[2]
    n_valid = Tk + (mut == "mask_plus") - (mut == "mask_minus" and Tk > 1)
    if n_valid > Tk:                      # the clamp min(key, n_k - 1) without the mask: the last key once more
        K, V = np.concatenate([K, K[:, :, -1:]], 2), np.concatenate([V, V[:, :, -1:]], 2)
    S = q @ K.transpose(0, 1, 3, 2)       # exp2 units
    m = np.zeros((B, H, Tq)); l = np.zeros((B, H, Tq)); o = np.zeros((B, H, Tq, 64))
    drop = Tk // 2
    for kt, k0 in enumerate(range(0, n_valid, KB)):
        k1 = min(k0 + KB, n_valid)
        s = S[..., k0:k1] - m[..., None]
        tmax = s.max(-1)
        move = (tmax > FA_THR) if lazy else (tmax > 0)
        move = np.ones_like(move) if kt == 0 else move
        delta = np.where(move, tmax, 0.0)
        if kt == 0 and mut != "first_tile_rescale":
            alpha = np.ones_like(delta)
        else:
            with np.errstate(over="ignore"):
                alpha = np.exp2(-delta.astype(np.float32)).astype(np.float64)     # float32: +inf past 2^128
        with np.errstate(invalid="ignore"):
            if mut != "move_o_not_l":
                l = l * alpha
            o = o * alpha[..., None]
        s = s - (2 if mut == "move_twice" else 1) * delta[..., None]
        m = m + delta
        p = np.exp2(s)
        if mut == "drop_key" and k0 <= drop < k1:
            p[..., drop - k0] = 0
        if mut == "double_key" and k1 == n_valid:
            p[..., -1] *= 2
        l = l + p.sum(-1)
        with np.errstate(over="ignore", invalid="ignore"):      # mutations only: p past the storage type's range
            o = o + rnd_t(p, ct).astype(np.float64) @ V[:, :, k0:k1]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = rnd_t(o / l[..., None], ct)
    if mut == "block1_to_block0" and Tq > 32:     # a wave's second block of 32 queries stored over its first (qw = 2: 64 per wave)
        out = out.copy()
        for q0 in range(0, Tq, 32 * qw):
            n1 = max(0, min(Tq, q0 + 64) - (q0 + 32))
            out[:, :, q0:q0 + n1] = out[:, :, q0 + 32:q0 + 32 + n1]
            out[:, :, q0 + 32:q0 + 32 + n1] = np.nan
    if mut == "last_query_unwritten" and Tq % 128:
        out = out.copy(); out[:, :, Tq - 1] = np.nan
    return out


def emulate_plain(sc: Scene, ct: str) -> np.ndarray:
    """enc_attn_simple_kernel restated plainly in np.float32: a 64-term dot product, exp(s - max), the sum, the accumulation over
    the keys, one division, the result rounded to the storage type.  Up to 257 keys one operation at a time and in key order; at
    the full window the sums are float32 matrix products (another float32 summation order, as legal as the kernel's own)."""
    Q, K, V = sc.Q, sc.K, sc.V
    B, H, Tq, _ = Q.shape
    if K.shape[2] > 257:
        s = Q @ K.transpose(0, 1, 3, 2)
        p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)
        return rnd_t((p @ V) / p.sum(-1, dtype=np.float32)[..., None], ct)
    out = np.empty((B, H, Tq, 64), np.float32)
    for q0 in range(0, Tq, 64):
        q = Q[:, :, q0:q0 + 64]
        s = np.cumsum(q[:, :, :, None, :] * K[:, :, None, :, :], axis=-1, dtype=np.float32)[..., -1]      # [B][H][q][Tk]
        p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)
        den = np.cumsum(p, axis=-1, dtype=np.float32)[..., -1]
        acc = np.cumsum(p[..., None] * V[:, :, None, :, :], axis=-2, dtype=np.float32)[..., -1, :]
        out[:, :, q0:q0 + 64] = acc / den[..., None]
    return rnd_t(out, ct)


def tile_maxima(sc: Scene) -> np.ndarray:
    """per query the maximum score of every 64-key tile, in exp2 units: [B][H][Tq][n_tiles]"""
    S = (sc.Q.astype(np.float64) @ sc.K.astype(np.float64).transpose(0, 1, 3, 2)) / np.log(2.0)
    Tk = S.shape[-1]
    return np.stack([S[..., k0:k0 + KB].max(-1) for k0 in range(0, Tk, KB)], axis=-1)
