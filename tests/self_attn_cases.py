"""The inputs, the case table and the comparison of the decoder self-attention kernel tests (test infrastructure, like
xattn_cases.py): tests/test_gpu_self_attn_kernels.py runs the cases on the GPU through the known-answer hooks ttasr_self_kv_fill /
_set / _get and ttasr_self_attn_probe; tests/test_self_attn_reference_host.py checks on the CPU that these very inputs and this very
tolerance see the bugs they are meant to see and that the tolerance is not too tight.

Kernels: self_attn_decode_kernel<T, MODE 0|1|2|3, SLAB, IDENT> and copy_pages_kernel (csrc/kernels_attn.hip), prefill_append_kernel
and prefill_attend_kernel (csrc/kernels_prefill.hip).  A workgroup of 4 waves serves one (row, head).  A lane holds one 16-byte
chunk of a key row: VEC = 8 elements on the 16-bit engines (LPR = 8 lanes per row, RPI = 8 rows per wave-instruction), VEC = 4 on
the f32 engine (LPR = 16, RPI = 4).  Cached key t belongs to SLOT t mod (4 RPI) - 32 slots (16-bit) or 16 (f32) - so a slot sees
keys slot, slot + 4 RPI, ... in order and keeps an online-softmax state (m, l, acc); loads are issued in batches of 4 iterations =
128 (16-bit) or 64 (f32) keys.  The new key is scored from registers in slot 0 after that slot's cached keys; one merge by
exp(m - M) joins the slots.

The bound, per output channel c of a (row, head) with Tk = pos + 1 keys (cached + new), u = 2^-24:

    |out - ref| <= r_T(ref) + 2 (delta + a) max_t |V[t, c]|
    r_T(ref) = ulp_T(ref) / 2 (1 + 2^-6) on the 16-bit engines, ulp_f32(ref) on the f32 engine
    delta    = 65 u sum_c |q_c| max_t |k_c|  +  40 * 2 u  +  (n + 2) 5 u
    a        = (2 n + 12) u
    n        = ceil(pos / (4 RPI)) + 1      keys a slot can see

Derivation.  A key's final weight is the product p * sc * sc * ... * wgt of hardware exponentials whose arguments telescope to
s_t - M.  (1) The score is a 64-term dot product (VEC fused multiply-adds and log2 LPR additions per lane group): at most 65 u
relative to sum |q_c| |k_c|, an absolute error of the exponent.  (2) Every exponent argument is a float32 difference, then scaled
by log2 e inside __expf: two roundings relative to |argument|; the arguments of one key's factors have one sign and sum to
s_t - M, whose magnitude is at most the row's score span <= 40 (asserted for every input set), so together 40 * 2 u whatever the
number of factors.  (3) The running maximum of a slot moves at most once per key of the slot, so a key's weight has at most
n + 2 factors that are not exp(0) = 1 exactly (its own p, one rescale per later key of the slot, the merge weight); each costs the
hardware exp (2^-22 = 4 u relative, twice its documented 1 ulp) and one product rounding (u).  delta bounds the relative error
of every weight, hence of the denominator (the sums below only add to it) and, times max |V|, of the numerator.  (4) The accumulation:
acc = fma(acc, sc, p v) is two roundings per key of the slot (2 n u), the merge multiplies once, adds log2 RPI <= 3 lanes and 3
partial sums of the waves (the denominator: 6 + 3 additions), and one division: at most 12 u more.  Numerator and denominator errors
add: the factor 2.  (5) The output is rounded once to the engine type: half a unit in the last place of the result, which may sit
one binade above the reference's (1 + 2^-6 as in xattn_cases; on the f32 engine a whole float32 ulp covers it).
Nothing here was fitted to a kernel's output: the calibration is the float32 restatement (f32_self_attention), which has to stay
inside 1 / 4 of the second term on every input set.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd.config import WhisperDims
from xattn_cases import slab_parts

POSITIONS = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 446, 447)
TYPES = ("f32", "bf16", "f16")
ENGINES = ((6, "f32"), (6, "bf16"), (6, "f16"), (20, "bf16"))
MAX_BATCH = 8
N_CTX = 448
PPS = N_CTX // 16                      # 28 pages per sequence
N_PAGES = MAX_BATCH * PPS
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SIG_TYPE = {"f32": "float", "bf16": "unsigned short", "f16": "f16_t"}
MANTISSA = {"f32": 23, "bf16": 7, "f16": 10}
POISON = {"f32": 0x7fc00000, "bf16": 0x7fc0, "f16": 0x7e00}      # a quiet NaN of the engine type; reads back as float32 0x7fc00000
RPI = {"f32": 4, "bf16": 8, "f16": 8}                            # rows per wave-instruction
LPR = {"f32": 16, "bf16": 8, "f16": 8}                           # lanes per key row


def slots(ct: str) -> int:
    return 4 * RPI[ct]                 # keys per iteration: 16 | 32


def batch(ct: str) -> int:
    return 4 * slots(ct)               # keys per load batch: 64 | 128


def dims(H: int) -> WhisperDims:
    return WhisperDims(f"sattn-h{H}", 80, 50, 64 * H, H, 64, 1, 2, 531, N_CTX)


def rnd(x: np.ndarray, ct: str) -> np.ndarray:
    """float32 values rounded to the engine type (and back to float32)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DTYPE[ct]).to(torch.float32).numpy()


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- contents ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def history(H: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """K, V [MAX_BATCH logical rows][N_CTX][H][64]: multiples of 1 / 64 in [-1, 1] times a power of two that differs between a
    head's K and V and between neighbouring rows and heads - representable in bf16 and fp16, so every type sees the same numbers."""
    g = np.random.Generator(np.random.Philox(key=21000 + seed))
    out = []
    for which in range(2):
        v = g.integers(-64, 65, size=(MAX_BATCH, N_CTX, H, 64)).astype(np.float32) / 64
        out.append(v * amps(H, which)[:, None, :, None])
    assert all(np.array_equal(rnd(a, "bf16"), a) and np.array_equal(rnd(a, "f16"), a) for a in out)
    return out[0], out[1]


def amps(H: int, which: int) -> np.ndarray:
    """[MAX_BATCH][H] the power of two of a logical row's head, K (0) or V (1)"""
    return np.array([[2.0 ** -((b + 2 * h + which) % 3) for h in range(H)] for b in range(MAX_BATCH)], np.float32)


def peak_keys(pos: int) -> List[int]:
    """Peak targets among the pos + 1 keys, most telling first: the first key, the last cached key, the new key (index pos), both
    sides of every multiple of a load batch (64 covers both geometries), then of every multiple of 32, then of 16."""
    first = [t for t in (0, pos - 1, pos) if 0 <= t <= pos]
    rest: List[int] = []
    for step, skip in ((64, 0), (32, 64), (16, 32)):
        for m in range(step, pos + 1, step):
            if skip and m % skip == 0:
                continue
            rest += [m - 1, m]
    seen, out = set(), []
    for t in first + rest:
        if t not in seen:
            seen.add(t); out.append(t)
    return out


def _peak_q(Kh: np.ndarray, t: int, want: float) -> np.ndarray:
    """q = 2^m K[t] with the smallest m that gives key t at least `want` of the softmax mass.  Kh [Tk][64] float64."""
    s = Kh @ Kh[t]
    gap = np.delete(s[t] - s, t)
    for m in range(-10, 9):
        if 1.0 / (1.0 + np.exp(-(2.0 ** m) * gap).sum()) >= want:
            return (2.0 ** m * Kh[t]).astype(np.float32)
    raise AssertionError(f"no scale makes key {t} of {len(Kh)} hold {want} of the mass")


def make_rows(Kfull: Sequence[np.ndarray], salt: int, sink_row: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    """q [n][H][64] against every row's keys Kfull[r] [H][Tk][64] (the history plus the new key, last).  Even rows are peaked (one
    key holds >= 0.9 of the mass, the key walking through peak_keys over the (row, head) items), odd rows are diffuse; sink_row has
    the attention-sink profile: >= 0.6 on key 0.  Returns (q, t* [n][H]: the peaked key or -1)."""
    n, H = len(Kfull), Kfull[0].shape[0]
    g = np.random.Generator(np.random.Philox(key=23000 + salt))
    q = (g.integers(-16, 17, size=(n, H, 64)) / 64).astype(np.float32)
    tstar = np.full((n, H), -1, np.int64)
    for r in range(n):
        Tk = Kfull[r].shape[1]
        keys = peak_keys(Tk - 1)
        for h in range(H):
            if r == sink_row:
                if Tk > 1:
                    q[r, h] = _peak_q(Kfull[r][h].astype(np.float64), 0, 0.6); tstar[r, h] = 0
            elif r % 2 == 0 and Tk > 1:
                t = keys[((r // 2) * H + h) % len(keys)]            # item i takes entry i of the list: the most telling keys first
                q[r, h] = _peak_q(Kfull[r][h].astype(np.float64), t, 0.9); tstar[r, h] = t
    return q, tstar


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    form: str                               # step | rows | prefill | packed
    pos: Tuple[int, ...] = ()               # step: (position,); rows: the rows' positions; prefill: (n_seq, npos); packed: lengths
    n_rows: int = MAX_BATCH
    table: str = "identity"                 # identity | permuted | beam
    ident: Tuple[bool, ...] = (False,)      # the identity_pages arguments the case runs with (identity table: both, same bits)
    row0: int = 0
    n_slab: int = 0
    done: bool = False                      # also run with the alternating finished pattern
    layer: int = 0
    types: Tuple[str, ...] = TYPES


ROWS_MIX = ((0, 447, 16, 129, 31, 256, 1, 64), (3, 446, 15, 128, 33, 255, 4, 65), (17, 127, 32, 257, 63, 447, 0, 446))
PREFILL_NPOS = (1, 2, 16, 17, 33, 129)
PACKED_LENS = (1, 17, 130, 2)
PACKED_PAGES = ((40,), (7, 201), tuple(range(222, 204, -2)), (3,))      # 1 | 2 | 9 | 1 pages, not contiguous
BEAM_POS = 33                                                           # pages 0, 1 shared inside a group, page 2 a row's own
BEAM_GROUPS = ((0, 1), (2, 3, 4, 5, 6, 7))                              # copy-on-write lists of 1 and 5 pairs
LOWP = ("bf16", "f16")


@lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    t: List[Case] = []
    for p in POSITIONS:
        t.append(Case(f"step-pos{p}", "step", (p,), ident=(True, False), layer=p % 2))
    for i, mix in enumerate(ROWS_MIX):
        t.append(Case(f"rows-mix{i}", "rows", mix, ident=(True, False), layer=i % 2))
    t.append(Case("step-pos257-permuted", "step", (257,), table="permuted", layer=1))
    t.append(Case("rows-mix0-permuted", "rows", ROWS_MIX[0], table="permuted"))
    t.append(Case("step-beam", "step", (BEAM_POS,), table="beam"))
    t.append(Case("rows-beam", "rows", (BEAM_POS,) * MAX_BATCH, table="beam", layer=1))
    for row0 in (0, 4):
        t.append(Case(f"step-pos129-row0-{row0}", "step", (129,), n_rows=4, row0=row0, ident=(True, False), layer=1))
        t.append(Case(f"rows-row0-{row0}", "rows", (447, 0, 65, 128), n_rows=4, row0=row0, ident=(True, False)))
    t.append(Case("rows-row0-4-permuted", "rows", (447, 0, 65, 128), n_rows=4, row0=4, table="permuted", layer=1))
    for ns in (1, 4):
        t.append(Case(f"step-pos128-slab{ns}", "step", (128,), n_slab=ns, ident=(True, False), layer=ns % 2, types=LOWP))
        t.append(Case(f"rows-mix1-slab{ns}", "rows", ROWS_MIX[1], n_slab=ns, ident=(True, False), layer=(ns + 1) % 2, types=LOWP))
    t.append(Case("step-pos447-slab4-permuted", "step", (447,), n_slab=4, table="permuted", types=LOWP))
    t.append(Case("step-pos1-slab4-row0-4", "step", (1,), n_rows=4, row0=4, n_slab=4, ident=(True,), layer=1, types=LOWP))
    t.append(Case("step-pos65-done", "step", (65,), done=True, ident=(True, False)))
    t.append(Case("rows-mix2-done", "rows", ROWS_MIX[2], done=True, ident=(True, False), layer=1))
    t.append(Case("rows-mix0-done-permuted", "rows", ROWS_MIX[0], done=True, table="permuted", layer=1))
    t.append(Case("step-pos16-done-slab4", "step", (16,), done=True, n_slab=4, ident=(True,), types=LOWP))
    for npos in PREFILL_NPOS:
        t.append(Case(f"prefill-npos{npos}", "prefill", (3, npos), n_rows=3 * npos, ident=(True, False), layer=npos % 2))
    t.append(Case("prefill-npos33-permuted", "prefill", (3, 33), n_rows=99, table="permuted"))
    t.append(Case("packed", "packed", PACKED_LENS, n_rows=sum(PACKED_LENS), layer=1))
    return tuple(t)


CASES_BY_NAME = {c.name: c for c in cases()}


def cases_of(ct: str) -> Tuple[Case, ...]:
    return tuple(c for c in cases() if ct in c.types)


def expected_sig(c: Case, ct: str, H: int, ident: bool) -> str:
    T, i = SIG_TYPE[ct], "true" if ident else "false"
    if c.form in ("step", "rows"):
        return f"self_attn_decode_kernel<{T}, {0 if c.form == 'step' else 3}, {'true' if c.n_slab else 'false'}, {i}> grid {H * c.n_rows * 256}"
    if c.form == "prefill":
        g = H * c.n_rows * 256
        return f"self_attn_decode_kernel<{T}, 1, false, {i}> grid {g} + self_attn_decode_kernel<{T}, 2, false, {i}> grid {g}"
    return f"prefill_append_kernel<{T}> grid {c.n_rows * 256} + prefill_attend_kernel<{T}> grid {H * c.n_rows * 256}"


def done_flags(n: int) -> np.ndarray:
    f = np.zeros(n, np.int32)
    f[1::2] = 1; f[0] = 1                   # finished rows in front of, between and behind live rows
    return f


# ---- tables -----------------------------------------------------------------------------------------------------------------
def identity_table() -> np.ndarray:
    return np.arange(N_PAGES, dtype=np.int32).reshape(MAX_BATCH, PPS)


def permuted_table() -> np.ndarray:
    g = np.random.Generator(np.random.Philox(key=25000))
    return g.permutation(N_PAGES).astype(np.int32).reshape(MAX_BATCH, PPS)


def beam_table() -> Tuple[np.ndarray, Tuple[Tuple[int, ...], ...]]:
    """Rows of a group share the parent's full pages and own their last page; (table, one copy-on-write pair list per group)."""
    tab = permuted_table().copy()
    last = BEAM_POS // 16
    pairs = []
    for grp in BEAM_GROUPS:
        parent, flat = grp[0], []
        for child in grp[1:]:
            tab[child, :last] = tab[parent, :last]
            flat += [int(tab[parent, last]), int(tab[child, last])]
        pairs.append(tuple(flat))
    return tab, tuple(pairs)


# ---- scenes: everything one case launches with ----------------------------------------------------------------------------------
@dataclass
class Scene:
    case: Case
    H: int
    ct: str
    table: np.ndarray                       # [MAX_BATCH][PPS] the device page table of the launch (packed: not used)
    lens: Tuple[int, ...]                   # prefill forms: the sequences' lengths; decode forms: ()
    pages: Tuple[Tuple[int, ...], ...]      # per row (decode forms) or per sequence (prefill forms): its page list
    pos: np.ndarray                         # [n_rows] position of every row (prefill forms: its position in its sequence)
    q: np.ndarray                           # [n_rows][H][64] float32, representable in the engine type
    k: np.ndarray
    v: np.ndarray
    tstar: np.ndarray                       # [n_rows][H]
    pool: Dict[int, np.ndarray]             # layer -> [N_PAGES][2][H][16][64] float32 before the launch, NaN = poison
    copies: Tuple[Tuple[int, ...], ...] = ()   # beam: pair lists to run through the copy form before the launch

    @property
    def qkv(self) -> np.ndarray:
        n = len(self.q)
        return np.concatenate([self.q.reshape(n, -1), self.k.reshape(n, -1), self.v.reshape(n, -1)], axis=1)

    def feed(self) -> np.ndarray:
        return slab_parts(self.qkv, self.case.n_slab) if self.case.n_slab else self.qkv

    def geom(self) -> Tuple[int, ...]:
        return self.case.pos

    def aux(self) -> Optional[np.ndarray]:
        if self.case.form == "packed":
            return np.array([p for pl in self.pages for p in pl], np.int32)
        return None if self.case.table == "identity" else self.table


def poisoned(H: int) -> np.ndarray:
    return np.full((N_PAGES, 2, H, 16, 64), np.nan, np.float32)


def place(pool: np.ndarray, pages: Sequence[int], K: np.ndarray, V: np.ndarray) -> None:
    """positions 0 .. n - 1 of a sequence (K, V [n][H][64]) into its pages"""
    t = np.arange(len(K))
    pg = np.asarray(pages, np.int64)[t // 16]
    pool[pg, 0, :, t % 16] = K
    pool[pg, 1, :, t % 16] = V


def copy_pages(pool: np.ndarray, pairs: Sequence[int]) -> None:
    for i in range(0, len(pairs), 2):
        pool[pairs[i + 1]] = pool[pairs[i]]


@lru_cache(maxsize=2)
def scene(c: Case, H: int, ct: str) -> Scene:
    Kh, Vh = history(H)
    layer = c.layer
    pools = {0: poisoned(H), 1: poisoned(H)}
    salt = sum(c.pos) + 7 * layer
    g = np.random.Generator(np.random.Philox(key=27000 + salt))
    if c.form in ("step", "rows"):
        copies: Tuple[Tuple[int, ...], ...] = ()
        table = {"identity": identity_table, "permuted": permuted_table}.get(c.table, lambda: beam_table()[0])()
        pos = np.array(c.pos * c.n_rows if c.form == "step" else c.pos, np.int64)
        assert len(pos) == c.n_rows and c.row0 + c.n_rows <= MAX_BATCH
        rows = [c.row0 + r for r in range(c.n_rows)]                    # batch rows: they pick the pages, never row0-relative
        content = list(rows)                                            # logical history of every row
        if c.table == "beam":
            copies = beam_table()[1]
            content = [grp[0] for r in rows for grp in BEAM_GROUPS if r in grp]
            perm = permuted_table()
            for l in (0, 1):                                            # parents own their history in BOTH layers (the copy covers all)
                for grp in BEAM_GROUPS:
                    src = (grp[0] + 3 * l) % MAX_BATCH
                    place(pools[l], perm[grp[0]], Kh[src][:BEAM_POS], Vh[src][:BEAM_POS])
                    for child in grp[1:]:                               # a child's own page holds STALE values before the copy
                        pools[l][table[child, BEAM_POS // 16], :, :, :1] = Kh[(child + 1) % MAX_BATCH][5, None, :, None, :]
        else:
            for r, b in enumerate(rows):
                place(pools[layer], table[b], Kh[b][:pos[r]], Vh[b][:pos[r]])
        src_of = [(content[r] + 3 * layer) % MAX_BATCH if c.table == "beam" else content[r] for r in range(c.n_rows)]
        kn = (g.integers(-64, 65, size=(c.n_rows, H, 64)) / 64).astype(np.float32) * amps(H, 0)[src_of][:, :, None]
        vn = (g.integers(-64, 65, size=(c.n_rows, H, 64)) / 64).astype(np.float32) * amps(H, 1)[src_of][:, :, None]
        Kfull = [np.concatenate([Kh[src_of[r]][:pos[r]].transpose(1, 0, 2), kn[r][:, None]], axis=1) for r in range(c.n_rows)]
        q, tstar = make_rows(Kfull, salt, sink_row=c.n_rows - 1)
        return Scene(c, H, ct, table, (), tuple(tuple(int(p) for p in table[b]) for b in rows), pos, q, kn, vn, tstar, pools, copies)
    # the two prefill forms: every key is one of the pass's own rows
    if c.form == "prefill":
        n_seq, npos = c.pos
        lens = (npos,) * n_seq
        table = identity_table() if c.table == "identity" else permuted_table()
        pages = tuple(tuple(int(p) for p in table[s]) for s in range(n_seq))
    else:
        lens, pages, table = c.pos, PACKED_PAGES, identity_table()
    k = np.concatenate([Kh[s][:n] for s, n in enumerate(lens)])
    v = np.concatenate([Vh[s][:n] for s, n in enumerate(lens)])
    pos = np.concatenate([np.arange(n) for n in lens])
    Kfull, r0 = [], 0
    for n in lens:
        Kfull += [k[r0:r0 + t + 1].transpose(1, 0, 2) for t in range(n)]
        r0 += n
    q, tstar = make_rows(Kfull, salt, sink_row=len(pos) - 1)
    return Scene(c, H, ct, table, tuple(lens), pages, pos, q, k, v, tstar, pools)


def launch_pool(sc: Scene) -> np.ndarray:
    """the case's layer as the launch finds it: the scene's pool after its copy-on-write lists"""
    pool = sc.pool[sc.case.layer]
    if sc.copies:
        pool = pool.copy()
        for pairs in sc.copies:
            copy_pages(pool, pairs)
    return pool


def pool_after(sc: Scene, done: Optional[np.ndarray] = None) -> Dict[int, np.ndarray]:
    """what both layers must hold after the copies and the launch: the one appended slot per live row, nothing else"""
    out = {l: p.copy() for l, p in sc.pool.items()}
    for pairs in sc.copies:
        for l in out:
            copy_pages(out[l], pairs)
    lay = out[sc.case.layer]
    if sc.lens:
        r0 = 0
        for s, n in enumerate(sc.lens):
            place(lay, sc.pages[s], sc.k[r0:r0 + n], sc.v[r0:r0 + n])
            r0 += n
    else:
        for r, p in enumerate(sc.pos):
            if done is None or not done[r]:
                lay[sc.pages[r][p // 16], 0, :, p % 16] = sc.k[r]
                lay[sc.pages[r][p // 16], 1, :, p % 16] = sc.v[r]
    return out


def pool_mismatch(got: np.ndarray, want: np.ndarray) -> List[Tuple[int, ...]]:
    """(page, K | V, head, position, channel) of the first elements whose BITS differ (poison included)"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return [tuple(int(i) for i in b) for b in bad[:4]]


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def ulp(x: np.ndarray, ct: str) -> np.ndarray:
    """unit in the last place of the engine type at |x| (0 at 0; subnormals of fp16 below 2^-14, of float32 below 2^-126)."""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    if ct == "f16":
        e = np.maximum(e, -14.0)
    if ct == "f32":
        e = np.maximum(e, -126.0)
    return np.where(a > 0, 2.0 ** (e - MANTISSA[ct]), 0.0)


def reference(sc: Scene) -> Dict[str, np.ndarray]:
    """float64 reference of the scene and the derived bound (module docstring), per output channel [n_rows][H][64]"""
    if sc.lens:
        rows = R.self_attn_causal_ref(sc.q, sc.k, sc.v, sc.lens)
    else:
        rows = R.self_attn_ref(sc.q, sc.k, sc.v, launch_pool(sc), sc.pages, sc.pos)
    return bound_rows(rows, sc.q, sc.ct)


def bound_rows(rows, q: np.ndarray, ct: str) -> Dict[str, np.ndarray]:
    n, H, _ = q.shape
    u = 2.0 ** -24
    ref = np.empty((n, H, 64)); f32 = np.empty((n, H, 64)); span = np.empty((n, H)); mass = np.empty((n, H)); m0 = np.empty((n, H))
    for r, (out, s, K, V) in enumerate(rows):
        Tk = s.shape[-1]
        nk = -(-(Tk - 1) // slots(ct)) + 1
        sqk = (np.abs(q[r].astype(np.float64)) * np.abs(K).max(axis=1)).sum(-1)
        delta = 65 * u * sqk + 40 * 2 * u + (nk + 2) * 5 * u
        acc = (2 * nk + 12) * u
        ref[r] = out
        f32[r] = 2 * (delta + acc)[:, None] * np.abs(V).max(axis=1)
        span[r] = s.max(-1) - s.min(-1)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        mass[r] = p.max(-1); m0[r] = p[:, 0]
    rt = ulp(ref, ct) if ct == "f32" else ulp(ref, ct) / 2 * (1 + 2.0 ** -6)
    return dict(ref=ref, f32=f32, bound=rt + f32, span=span, mass=mass, mass0=m0)


def error_ratio(out: np.ndarray, ref: Dict[str, np.ndarray], rows: Optional[np.ndarray] = None) -> Tuple[float, Tuple[int, int, int]]:
    """largest |out - ref| / bound over the rows (all, or the index array) and its (row, head, channel); above 1 = flagged.  A
    non-finite output (a read of poison) is infinitely wrong; a bound of 0 admits only the exact value."""
    err = np.abs(out.reshape(ref["ref"].shape).astype(np.float64) - ref["ref"])
    b = ref["bound"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    r = np.nan_to_num(r, nan=np.inf)
    if rows is not None:
        keep = np.zeros(len(r), bool); keep[rows] = True
        r = np.where(keep[:, None, None], r, 0.0)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(x) for x in i)


def describe(sc: Scene, out: np.ndarray, ref: Dict[str, np.ndarray], where: Tuple[int, int, int]) -> str:
    r, h, ch = where
    o = out.reshape(ref["ref"].shape)
    return (f"{sc.case.name} ({sc.case.form}, {sc.ct}, H {sc.H}): row {r} position {int(sc.pos[r])} head {h} channel {ch}: got {o[r, h, ch]!r}, "
            f"reference {ref['ref'][r, h, ch]!r}, bound {ref['bound'][r, h, ch]:.3e}, peaked key {int(sc.tstar[r, h])}")


# ---- the kernel's arithmetic in float32 -------------------------------------------------------------------------------------
def f32_self_attention(q: np.ndarray, K: np.ndarray, V: np.ndarray, ct: str, new_from_registers: bool = True, den_times: int = 1) -> np.ndarray:
    """One row of the kernels restated plainly in np.float32: q [H][64]; K, V [H][Tk][64] with the new key last.  Slot t mod (4 RPI)
    runs an online softmax over its keys in order; the new key (new_from_registers: the decode kernel; the packed attend kernel
    reads it from the pool like any other) is scored in slot 0 after that slot's cached keys; one merge by exp(m - M)."""
    f = np.float32
    H, Tk, _ = K.shape
    S, vec = slots(ct), 64 // LPR[ct]
    q, K, V = q.astype(f), K.astype(f), V.astype(f)
    prod = q[:, None, :] * K                                             # per lane: VEC products summed in order, then a tree over the lanes
    lane = np.zeros((H, Tk, LPR[ct]), f)
    for j in range(vec):
        lane = lane + prod.reshape(H, Tk, LPR[ct], vec)[:, :, :, j]
    while lane.shape[-1] > 1:
        lane = lane[..., 0::2] + lane[..., 1::2]
    s = lane[..., 0]
    ncached = Tk - 1 if new_from_registers else Tk
    m = np.full((H, S), -1e30, f); l = np.zeros((H, S), f); acc = np.zeros((H, S, 64), f)

    def visit(sl, t):                                                     # slots `sl` (index array) take keys `t` (one each)
        st, vt = s[:, t], V[:, t]
        mn = np.maximum(m[:, sl], st)
        sc, p = np.exp(m[:, sl] - mn).astype(f), np.exp(st - mn).astype(f)
        l[:, sl] = l[:, sl] * sc + p
        acc[:, sl] = acc[:, sl] * sc[..., None] + p[..., None] * vt
        m[:, sl] = mn
    for t0 in range(0, ncached, S):
        t = np.arange(t0, min(t0 + S, ncached))
        visit(t - t0, t)
    if new_from_registers:
        visit(np.array([0]), np.array([Tk - 1]))
    M = m.max(-1, keepdims=True)
    w = np.exp(m - M).astype(f)
    lw = (l * w).reshape(H, 4, -1)
    den = np.zeros((H, 4), f)
    for i in range(lw.shape[-1]):
        den = den + lw[..., i]
    den = (den[:, 0] + den[:, 1]) + (den[:, 2] + den[:, 3])
    den = den * f(den_times)
    a = (acc * w[..., None]).reshape(H, 4, -1, 64)
    part = np.zeros((H, 4, 64), f)
    for i in range(a.shape[2]):
        part = part + a[:, :, i]
    num = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
    return (num / den[:, None]).astype(f)


def restate(sc: Scene) -> np.ndarray:
    """the float32 restatement over a whole scene, [n_rows][H][64] (before the rounding to the engine type)"""
    if sc.lens:
        rows = R.self_attn_causal_ref(sc.q, sc.k, sc.v, sc.lens)
    else:
        rows = R.self_attn_ref(sc.q, sc.k, sc.v, launch_pool(sc), sc.pages, sc.pos)
    return np.stack([f32_self_attention(sc.q[r], K, V, sc.ct, new_from_registers=sc.case.form != "packed") for r, (_, _, K, V) in enumerate(rows)])
