"""The inputs, the case list and the comparison of the cross-attention kernel tests (test infrastructure, like geometry_table.py):
tests/test_gpu_xattn_kernels.py runs the cases on the GPU through the known-answer hooks ttasr_get_cross_kv_fp8 and
ttasr_cross_attn_probe; tests/test_xattn_reference_host.py checks on the CPU that these very inputs and this very tolerance see
the bugs they are meant to see and that the tolerance is not too tight.

Cache contents without a setter hook: the decoder's cross-attention k_proj / v_proj weights are channel permutations (K of layer
l, head h = encoder head h + 2 l; V = encoder head h + 2 l + 1, modulo H; zero V bias), so ttasr_set_encoder_output with values
that are exactly representable in the engine type makes the cache a known permutation of the input.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import WhisperDims

WINDOWS = (4, 6, 14, 16, 18, 30, 32, 34, 62, 64, 66, 126, 130, 150, 254, 258)
FULL_WINDOW = 1500
TYPES = ("bf16", "f16")
HEADS = (20, 16)              # 16 heads: 16 rows are exactly the 256 (row, head) items of the e4m3 per-row form's threshold
MAX_BATCH = 32
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}
SIG_TYPE = {"bf16": "unsigned short", "f16": "f16_t"}
MANTISSA = {"bf16": 7, "f16": 10}


def dims(H: int) -> WhisperDims:
    return WhisperDims(f"xattn-h{H}", 80, 1500, 64 * H, H, 64, 1, 2, 531, 32)


def head_shift(layer: int, which: int) -> int:
    return 2 * layer + which


def state_dict(H: int) -> Dict[str, np.ndarray]:
    d = 64 * H
    sd = dict(synth.state_dict(dims(H)))
    for l in range(2):
        p = f"model.decoder.layers.{l}.encoder_attn."
        for which, name in enumerate(("k_proj", "v_proj")):
            assert sd[p + name + ".weight"].shape == (d, d)
            # out[i] = x[(i + 64 s) % d]: head h of the cache is encoder head (h + s) % H
            sd[p + name + ".weight"] = np.roll(np.eye(d, dtype=np.float32), 64 * head_shift(l, which), axis=1)
        sd[p + "v_proj.bias"] = np.zeros(d, dtype=np.float32)
    return sd


def rnd(x: np.ndarray, ct: str) -> np.ndarray:
    """float32 values rounded to the engine type (and back to float32)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DTYPE[ct]).to(torch.float32).numpy()


def blocks_to_enc(blocks: np.ndarray) -> np.ndarray:
    """encoder-space blocks [B][H][T][64] -> the encoder output [B][T][64 H] that ttasr_set_encoder_output takes."""
    B, H, T, _ = blocks.shape
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(B, T, 64 * H))


def cache_of(blocks: np.ndarray, layer: int, which: int) -> np.ndarray:
    """what the cache [B][H][T][64] of (layer, K | V) must hold for these encoder-space blocks."""
    H = blocks.shape[1]
    return blocks[:, [(h + head_shift(layer, which)) % H for h in range(H)]]


# ---- cache contents ---------------------------------------------------------------------------------------------------------
E4M3_TABLE = R.e4m3_decode(np.arange(256, dtype=np.uint8))
_POS = np.sort(E4M3_TABLE[:127])                      # the 127 finite non-negative values, 0 .. 448
E4M3_MIDPOINTS = (_POS[:-1] + _POS[1:]) / 2           # every midpoint between adjacent finite codes (126 of them)
QUANT_KINDS = ("zero", "outlier", "constant", "ties", "heavy", "negative", "heavy2")
TIES_K = -3                                           # the ties block has amax = 448 * 2^k


def quant_block(kind: str, T: int, ct: str, seed: int) -> np.ndarray:
    g = np.random.Generator(np.random.Philox(key=7000 + seed))
    n = T * 64
    if kind == "zero":
        v = np.zeros(n, np.float32)
    elif kind == "outlier":       # one large value: the rest lands in subnormals and zeros
        v = (0.004 * g.standard_normal(n)).astype(np.float32)
        v[int(g.integers(n))] = 1000.0
    elif kind == "constant":
        v = np.full(n, (0.75, -1.5, 3.0)[seed % 3], np.float32)
    elif kind == "ties":          # amax = 448 * 2^k: inv is a power of two and v * inv falls exactly on e4m3 ties (17, 19, ...)
        m = np.concatenate([E4M3_MIDPOINTS, -E4M3_MIDPOINTS])
        v = np.resize(np.roll(m, seed), n).astype(np.float64)
        v[(seed * 37) % n] = 448.0
        v = (v * 2.0 ** TIES_K).astype(np.float32)
    else:                         # heavy-tailed
        v = (g.standard_normal(n) * np.exp(1.5 * g.standard_normal(n))).astype(np.float32)
        v = np.clip(v, -30000, 30000)
        if kind == "negative":
            v = -np.abs(v) - np.float32(2.0 ** -10)
    out = rnd(v, ct).reshape(T, 64)
    out[out == 0] = 0.0           # no -0 (an fp16 underflow): the projection's f32 sum 0 + ... + (-0) + bias 0 is +0, a different bit pattern
    if kind == "ties":
        assert np.array_equal(out.reshape(-1), v), "tie values must be representable in the engine type"
    return out


def quant_kind(b: int, h: int, window: int) -> str:
    return QUANT_KINDS[(b * 3 + h + window // 2) % len(QUANT_KINDS)]


def quant_blocks(ct: str, window: int, B: int, H: int, salt: int = 0) -> np.ndarray:
    """encoder-space blocks [B][H][window][64] that walk through every block kind."""
    return np.stack([np.stack([quant_block(quant_kind(b + salt, h, window), window, ct, 131 * (b + salt) + h + 17 * window)
                               for h in range(H)]) for b in range(B)])


def attn_amp(b: int, h: int) -> float:
    return 2.0 ** -((b + 2 * h) % 3)


def attn_blocks(ct: str, window: int, B: int, H: int) -> np.ndarray:
    """Blocks for the attention cases: multiples of 1 / 64 in [-1, 1] times a power of two that differs between a head's K and V
    and between neighbouring heads (a swapped or shifted scale is a factor 2 or 4).  Representable in bf16 and fp16, so both
    engine types see the same numbers."""
    g = np.random.Generator(np.random.Philox(key=9000 + window))
    v = g.integers(-64, 65, size=(B, H, window, 64)).astype(np.float32) / 64
    amp = np.array([[attn_amp(b, h) for h in range(H)] for b in range(B)], np.float32)
    out = v * amp[:, :, None, None]
    assert np.array_equal(rnd(out, ct), out)
    return out


def attn_clips(H: int, window: int) -> int:
    return max(c.clips for c in cases(H, window))


# ---- queries ----------------------------------------------------------------------------------------------------------------
def peak_frames(Tk: int) -> List[int]:
    """frame 0, Tk - 1, and both sides of every multiple of 16 (hence of 32 and 64, and of every slice seam: slices are cut at
    multiples of 32)."""
    s = {0, Tk - 1}
    for m in range(16, Tk, 16):
        s.update((m - 1, m))
    return sorted(s)


def make_q(K: np.ndarray, n_rows: int, kv_div: int, salt: int) -> Tuple[np.ndarray, np.ndarray]:
    """q [n_rows][H][64] (float32, representable in either engine type) against the 16-bit K cache [clips][H][T][64].
    Even rows are peaked: q = 2^m K[t*] with the smallest m that gives frame t* >= 0.93 of the softmax mass, t* walking through
    peak_frames over the (row, head) items; odd rows are diffuse (small random multiples of 1 / 64).
    Returns (q, t* [n_rows][H] with -1 for diffuse items)."""
    _, H, T, _ = K.shape
    frames = peak_frames(T)
    g = np.random.Generator(np.random.Philox(key=11000 + salt))
    q = (g.integers(-16, 17, size=(n_rows, H, 64)) / 64).astype(np.float32)
    tstar = np.full((n_rows, H), -1, np.int64)
    K64 = K.astype(np.float64)
    for r in range(0, n_rows, 2):
        clip = r // kv_div
        for h in range(H):
            i = (r // 2) * H + h            # item 0 peaks at frame 0, item 1 at the last frame, the others walk the list
            t = frames[0] if i == 0 else frames[-1] if i == 1 else frames[(i + salt) % len(frames)]
            k = K64[clip, h]
            s = k @ k[t]
            gap = np.delete(s[t] - s, t)
            for m in range(-8, 9):
                if 1.0 / (1.0 + np.exp(-(2.0 ** m) * gap).sum()) >= 0.93:   # 0.93 on the 16-bit cache leaves 0.9 on its e4m3 copy
                    break
            else:
                raise AssertionError(f"no scale makes frame {t} of (clip {clip}, head {h}) hold 0.9 of the mass")
            q[r, h] = (2.0 ** m * k[t]).astype(np.float32)
            tstar[r, h] = t
    return q, tstar


def slab_parts(q: np.ndarray, n_slab: int) -> np.ndarray:
    """q as n_slab partial tiles whose every partial sum is exact in float32 (q has at most 11 significant bits)."""
    w = {1: (1.0,), 4: (0.5, 0.25, 0.125, 0.125)}[n_slab]
    flat = q.reshape(q.shape[0], -1)
    return np.stack([np.float32(x) * flat for x in w])


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    H: int
    n_rows: int
    kv_div: int = 1
    n_slab: int = 0
    fp8_mode: int = 0                       # option xkv_fp8 the case runs under
    opts: Tuple[Tuple[str, int], ...] = ()  # options away from their defaults
    form: str = "pipe"                      # the kernel form the case names: fp8 | mq_fp8 | pipe | decode | split | mq
    layer: int = 0
    full: bool = False                      # also run at the full 1500-frame window (once per form)
    done: Optional[str] = None              # finished-row pattern of the (e) cases: "alt" | "group"

    @property
    def clips(self) -> int:
        return self.n_rows // self.kv_div

    @property
    def reads_fp8(self) -> bool:
        return self.form in ("fp8", "mq_fp8")

    def opt(self, key: str, default: int) -> int:
        return dict(self.opts).get(key, default)


DEFAULT_OPTS = {"xattn_mq_fp8": 1, "xsplit": 1, "xattn_pipeline": 1, "xattn_nontemporal": 1, "xattn_deep_items": 512, "xattn_mq_slices": 0}


def splits(items: int, Tk: int) -> int:
    """cross_attn_splits (kernels_attn.hip): frame slices of `items` (row | group, head) items."""
    if items >= 256:
        return 1
    return max(1, min(8, -(-480 // items), (Tk + 63) // 64))


def slice_plan(Sq: int, Tk: int) -> Tuple[int, int]:
    chunk = ((Tk + Sq - 1) // Sq + 31) // 32 * 32
    return (Tk + chunk - 1) // chunk, chunk


def expected_kernel(c: Case, Tk: int, ct: str) -> Tuple[str, Optional[int]]:
    """(signature prefix, frame slices or None) of the kernel the dispatch must pick for the case at window Tk."""
    T = SIG_TYPE[ct]
    nt = "true" if c.opt("xattn_nontemporal", 1) else "false"
    form = c.form
    if form == "split" and splits(c.n_rows * c.H, Tk) == 1:
        form = "pipe"                       # windows of at most 64 frames have one slice: the single-pass kernel keeps the job
    if form == "fp8":
        return f"cross_attn_fp8_kernel<{T}, {'true' if c.n_slab else 'false'}, 4> grid {c.H * c.n_rows * 256}", None
    if form in ("mq_fp8", "mq"):
        groups = -(-c.kv_div // 8)
        Sq = min(8, c.opt("xattn_mq_slices", 0)) or splits(c.clips * groups * c.H, Tk)
        name = "cross_attn_mq_fp8_kernel" if form == "mq_fp8" else "cross_attn_mq_kernel"
        return f"{name}<{T}, {min(c.kv_div, 8)}> grid", slice_plan(Sq, Tk)[0]
    if form == "split":
        return f"cross_attn_split_kernel<{T}> grid", slice_plan(splits(c.n_rows * c.H, Tk), Tk)[0]
    if form == "decode":
        return f"cross_attn_decode_kernel<{T}, false, 4, 8, {nt}, {1 if c.n_slab else 0}> grid {c.H * c.n_rows * 256}", None
    return f"cross_attn_pipe_kernel<{T}, {nt}, {'true' if c.n_slab else 'false'}, 3> grid {c.H * c.n_rows * 256}", None


def sig_matches(sig: str, c: Case, Tk: int, ct: str) -> bool:
    prefix, slices = expected_kernel(c, Tk, ct)
    return sig.startswith(prefix) and (slices is None or f" slices {slices}" in sig + " ") and \
        (slices is None or slices == 1 or sig.endswith("+ cross_attn_merge_kernel"))


@lru_cache(maxsize=None)
def cases(H: int, window: int = 0) -> Tuple[Case, ...]:
    """Every case of an engine shape; window > 0 keeps the ones that run at that window (the full window: one per form)."""
    t: List[Case] = []
    if H == 20:
        # (c) e4m3 forms.  Per-row: n H >= 256; 13 x 20 = 260 items, 12 x 20 = 240 stays on the 16-bit kernels
        for ns in (0, 1, 4):
            t.append(Case(f"fp8-rows13-slab{ns}", H, 13, n_slab=ns, fp8_mode=1 + (ns == 0), form="fp8", layer=ns % 2, full=ns == 4))
        t.append(Case("fp8-rows12-240-items-16bit", H, 12, fp8_mode=2, form="split", layer=1))
        t.append(Case("fp8-rows12-240-items-16bit-mode1", H, 12, fp8_mode=1, form="split"))
        # shared clip: every NQ instantiation; 13 x 2 one slice, 6 x 5 four slices, 2 x 7 eight slices at the full window
        for clips, beam in ((13, 2), (5, 3), (4, 4), (6, 5), (3, 6), (2, 7)):
            t.append(Case(f"mqfp8-{clips}x{beam}", H, clips * beam, beam, fp8_mode=2, form="mq_fp8", layer=beam % 2, full=beam in (2, 5, 7)))
        for s in (1, 3, 8):
            t.append(Case(f"mqfp8-6x5-slices{s}", H, 30, 5, fp8_mode=2, opts=(("xattn_mq_slices", s),), form="mq_fp8", layer=s % 2, full=s == 3))
        for ns in (1, 4):
            t.append(Case(f"mqfp8-6x5-slab{ns}", H, 30, 5, n_slab=ns, fp8_mode=2, form="mq_fp8", layer=1))
            t.append(Case(f"mqfp8-2x7-slab{ns}", H, 14, 7, n_slab=ns, fp8_mode=2, form="mq_fp8"))
        t.append(Case("mqfp8-off-6x5-16bit", H, 30, 5, fp8_mode=2, opts=(("xattn_mq_fp8", 0),), form="mq"))
        t.append(Case("mode1-6x5-16bit", H, 30, 5, fp8_mode=1, form="mq", layer=1))
        # (d) 16-bit forms.  The pipelined kernel: deep (items <= xattn_deep_items) and shallow on both sides of 512 and with 0
        for n, deep in ((13, 512), (13, 0), (32, 512), (25, 512), (26, 512)):   # 260 | 500 | 520 | 640 items
            for nt in (1, 0):
                for ns in (0, 4):
                    if n in (25, 26, 32) and (nt == 0 or ns):
                        continue
                    t.append(Case(f"pipe-rows{n}-deep{deep}-nt{nt}-slab{ns}", H, n, n_slab=ns, form="pipe", layer=(n + ns) % 2,
                                  opts=(("xattn_deep_items", deep), ("xattn_nontemporal", nt)), full=(n, deep, nt, ns) in ((13, 512, 1, 4), (13, 0, 1, 0))))
        t.append(Case("pipe-rows13-slab1", H, 13, n_slab=1, form="pipe", layer=1))
        for ns in (0, 4):
            t.append(Case(f"decode-rows13-slab{ns}", H, 13, n_slab=ns, form="decode", opts=(("xattn_pipeline", 0),), layer=ns % 2, full=ns == 0))
        t.append(Case("decode-rows13-nt0", H, 13, form="decode", opts=(("xattn_pipeline", 0), ("xattn_nontemporal", 0)), layer=1))
        for n, ns in ((1, 0), (3, 0), (3, 4), (6, 0), (12, 0)):                 # 20, 60, 120, 240 items: 8, 8, 4, 2 slices
            t.append(Case(f"split-rows{n}-slab{ns}", H, n, n_slab=ns, form="split", layer=n % 2, full=(n, ns) in ((3, 4), (12, 0))))
        t.append(Case("xsplit-off-rows3-pipe", H, 3, form="pipe", opts=(("xsplit", 0),)))
        for clips, beam in ((13, 2), (5, 3), (4, 4), (6, 5), (3, 6), (2, 7), (2, 8)):
            t.append(Case(f"mq-{clips}x{beam}", H, clips * beam, beam, form="mq", layer=(beam + 1) % 2, full=beam in (5, 8)))
        t.append(Case("mq-6x5-slab4", H, 30, 5, n_slab=4, form="mq"))
        t.append(Case("mq-2x8-slices3", H, 16, 8, form="mq", opts=(("xattn_mq_slices", 3),), layer=1))
        # (e) finished rows
        t.append(Case("done-fp8-rows13", H, 13, fp8_mode=2, form="fp8", done="alt", layer=1))
        t.append(Case("done-pipe-rows13", H, 13, form="pipe", done="alt", full=True))
        t.append(Case("done-decode-rows13", H, 13, form="decode", opts=(("xattn_pipeline", 0),), done="alt", layer=1))
        t.append(Case("done-split-rows3", H, 3, form="split", done="alt"))
        t.append(Case("done-mqfp8-6x5", H, 30, 5, fp8_mode=2, form="mq_fp8", done="group", layer=1, full=True))
        t.append(Case("done-mqfp8-13x2", H, 26, 2, fp8_mode=2, form="mq_fp8", done="group"))
        t.append(Case("done-mq-6x5", H, 30, 5, form="mq", done="group"))
        t.append(Case("done-mq-13x2", H, 26, 2, form="mq", done="group", layer=1))
    else:
        assert H == 16
        for ns in (0, 4):                                                       # 16 x 16 = exactly 256 items
            t.append(Case(f"fp8-rows16-256-items-slab{ns}", H, 16, n_slab=ns, fp8_mode=2, form="fp8", layer=ns % 2, full=ns == 0))
        t.append(Case("fp8-rows15-240-items-16bit", H, 15, fp8_mode=2, form="split", layer=1))
        t.append(Case("mqfp8-4x4-256-items", H, 16, 4, fp8_mode=2, form="mq_fp8"))
        t.append(Case("mqfp8-3x5-240-items-16bit", H, 15, 5, fp8_mode=2, form="split", layer=1))
        t.append(Case("pipe-rows16-256-items", H, 16, form="pipe", layer=1))
        t.append(Case("mq-4x4-256-items", H, 16, 4, form="mq"))
    if window == FULL_WINDOW:
        t = [c for c in t if c.full]
    return tuple(t)


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def ulp(x: np.ndarray, ct: str) -> np.ndarray:
    """unit in the last place of the engine type at |x| (0 at 0; fp16 subnormals below 2^-14)."""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    if ct == "f16":
        e = np.maximum(e, -14.0)
    return np.where(a > 0, 2.0 ** (e - MANTISSA[ct]), 0.0)


def gather(q: np.ndarray, K: np.ndarray, V: np.ndarray, kv_div: int):
    """per clip: (rows of the clip, K [H][T][64], V [H][T][64])"""
    for clip in range(q.shape[0] // kv_div):
        rows = slice(clip * kv_div, (clip + 1) * kv_div)
        yield rows, K[clip], V[clip]


def reference(q: np.ndarray, K: np.ndarray, V: np.ndarray, kv_div: int, ct: str) -> Dict[str, np.ndarray]:
    """float64 reference of the case's operands and the derived bound, per output channel:
        |out - ref| <= ulp_T(ref) / 2 (1 + 2^-6) + (2 delta + Tk 2^-24) max_t |V[t, c]|
        delta = 65 2^-24 sum_c |q_c| max_t |k_c| + 40 2^-23 + 2^-22
    first term: the output's rounding to the engine type; second: the float32 arithmetic - a 64-term dot product with the scale
    folded into q, the exponent's argument scaling (|s - max s| <= 40), the hardware exp, and the accumulation over Tk frames.
    q [n][H][64]; K, V [clips][H][T][64] float64 (the dequantised copy for the e4m3 forms)."""
    n, H, _ = q.shape
    Tk = K.shape[2]
    ref = np.empty((n, H, 64)); f32 = np.empty((n, H, 64)); sqk = np.empty((n, H)); span = np.empty((n, H)); mass = np.empty((n, H))
    for rows, k, v in gather(q, K, V, kv_div):
        qq = q[rows].astype(np.float64)
        ref[rows], s = R.cross_attn_ref(qq, k, v)
        sqk[rows] = (np.abs(qq) * np.abs(k).max(axis=1)).sum(-1)
        span[rows] = s.max(-1) - s.min(-1)
        p = np.exp(s - s.max(-1, keepdims=True))
        mass[rows] = (p / p.sum(-1, keepdims=True)).max(-1)
        delta = 65 * 2.0 ** -24 * sqk[rows] + 40 * 2.0 ** -23 + 2.0 ** -22
        f32[rows] = (2 * delta[..., None] + Tk * 2.0 ** -24) * np.abs(v).max(axis=1)
    return dict(ref=ref, f32=f32, bound=ulp(ref, ct) / 2 * (1 + 2.0 ** -6) + f32, sqk=sqk, span=span, mass=mass)


def error_ratio(out: np.ndarray, ref: Dict[str, np.ndarray]) -> float:
    """largest |out - ref| / bound over the case; above 1 = the output is flagged.  A bound of 0 (an all-zero V column, whose
    reference is exactly 0) admits only the exact value."""
    err = np.abs(out.reshape(ref["ref"].shape).astype(np.float64) - ref["ref"])
    b = ref["bound"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return float(np.nan_to_num(r, nan=np.inf).max())


def dequant(codes: np.ndarray, scale: np.ndarray) -> np.ndarray:
    return R.e4m3_decode(codes) * scale.astype(np.float64)[..., None, None]


def f32_attention(q: np.ndarray, K: np.ndarray, V: np.ndarray, kv_div: int, ks: Optional[np.ndarray] = None,
                  vs: Optional[np.ndarray] = None) -> np.ndarray:
    """The kernels' arithmetic restated plainly in np.float32, one operation at a time and in frame order: a 64-term dot product,
    exp(s - max), the sum, the accumulation over the frames, one division.  K, V: float32-representable [clips][H][T][64] - the
    16-bit cache, or the decoded e4m3 codes with their scales ks, vs [clips][H]: K scale folded into q, V scale into the
    normalisation, as kernels_fp8.hip does."""
    n, H, _ = q.shape
    Tk = K.shape[2]
    out = np.empty((n, H, 64), np.float32)
    for clip, (rows, k, v) in enumerate(gather(q, K.astype(np.float32), V.astype(np.float32), kv_div)):
        qq = q[rows].astype(np.float32)
        if ks is not None:
            qq = qq * ks[clip].astype(np.float32)[None, :, None]
        s = np.zeros((qq.shape[0], H, Tk), np.float32)
        for c in range(64):
            s = s + qq[:, :, None, c] * k[None, :, :, c]
        p = np.exp(s - s.max(-1, keepdims=True)).astype(np.float32)
        den = np.zeros(p.shape[:2], np.float32)
        acc = np.zeros((qq.shape[0], H, 64), np.float32)
        for t in range(Tk):
            den = den + p[:, :, t]
            acc = acc + p[:, :, t, None] * v[None, :, t, :]
        if vs is not None:
            acc = acc * vs[clip].astype(np.float32)[None, :, None]
        out[rows] = acc / den[..., None]
    return out


@dataclass
class Operands:
    q: np.ndarray                      # float32 [n_rows][H][64]
    tstar: np.ndarray                  # [n_rows][H] peaked frame or -1
    K: np.ndarray                      # float64 [clips][H][T][64]: what the kernel form reads (dequantised for the e4m3 forms)
    V: np.ndarray
    codes: Optional[Tuple[np.ndarray, np.ndarray]] = None    # e4m3 forms: (K codes, V codes)
    scales: Optional[Tuple[np.ndarray, np.ndarray]] = None   # (K scales, V scales) float32 [clips][H]


@lru_cache(maxsize=4)
def scene(H: int, window: int) -> np.ndarray:
    return attn_blocks("bf16", window, attn_clips(H, window), H)


def case_salt(c: Case) -> int:
    return 3 * c.n_rows + c.layer


@lru_cache(maxsize=6)
def _operands(H: int, window: int, layer: int, n_rows: int, kv_div: int, fp8: bool) -> Operands:
    blocks = scene(H, window)[:n_rows // kv_div]
    K16, V16 = cache_of(blocks, layer, 0), cache_of(blocks, layer, 1)
    q, tstar = make_q(K16, n_rows, kv_div, 3 * n_rows + layer)
    if not fp8:
        return Operands(q, tstar, K16.astype(np.float64), V16.astype(np.float64))
    (kc, ksc), (vc, vsc) = R.xkv_quant_ref(K16), R.xkv_quant_ref(V16)
    return Operands(q, tstar, dequant(kc, ksc), dequant(vc, vsc), (kc, vc), (ksc, vsc))


def operands(c: Case, window: int) -> Operands:
    """The operands of a case at a window; the queries are built against the 16-bit cache whichever copy the form reads."""
    return _operands(c.H, window, c.layer, c.n_rows, c.kv_div, c.reads_fp8)


def done_flags(c: Case) -> np.ndarray:
    f = np.zeros(c.n_rows, np.int32)
    if c.done == "alt":
        f[1::2] = 1; f[0] = 1               # finished rows in front of, between and behind live rows
    elif c.done == "group":
        f[:c.kv_div] = 1                    # group 0: every row finished
        f[c.kv_div + 1] = 1                 # group 1: partly finished
        f[-1] = 1                           # the last group: partly finished
    return f
