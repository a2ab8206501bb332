"""Case table of the token-selection kernels (kernels_decode.hip) for tests/test_gpu_select_kernels.py and
tests/test_select_reference_host.py: deterministic, constructed rows with their float64 reference (oracle/whisper_ref.py select_ref).

Nothing here is filtered by what a kernel returns.  Every row is BUILT so that its decision is well separated - the winner leads
the runner-up by >= 1e-3 (or is an exact, bit-equal tie), the forced-timestamp margin is >= 1e-3 away from 0 (or exactly 0 by
construction), the perturbed top-2 gap of a sampled row is >= 1e-3 - and check_row() asserts those conditions against the
reference, so a case whose construction slipped fails on the host before any GPU sees it.

Layout the cases aim at (kernels_decode.hip): a row lives in 13 chunks of 4096 elements, thread t of 1024 holds elements
4 t .. 4 t + 3 of every chunk, the V % 4 tail elements V4 .. V - 1 go to threads 0 .. 2; lanes are 64 threads, waves 16.

Tolerances, u = 2^-24, m = the largest allowed logit of the row:
  log-probability increments, top-k values, token_logprob:  |err| <= 8 u max(|m|, 16)
  no-speech probability and token_prob:                     relative error <= 8 u max(16, |m|, |x_tok - m|)
from the rounding of m log2(e) (1.44 u |m|), of the log-normaliser and of the difference (u |m| each), and one-ulp exp2 / log."""
from __future__ import annotations

import dataclasses
import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd.config import WhisperDims

U = 2.0 ** -24
GAP = 1e-3
MAX_BATCH = 16
MAX_NEW = 16
VOCABS = (7, 512, 4097, 51864, 51865, 51866, 53248)   # 7: the smallest that holds eot < no_timestamps < two timestamps and a tail
RELEASED_TB = {51864: 50363, 51865: 50364, 51866: 50365}
SCALES = (1.0, 4.0, 12.0)
OFFSETS = (0.0, 30.0, -30.0, 110.0, -110.0, 128.0, -128.0)   # -110: the trained profile's offset (test_gpu_round6_fixes)
DELTAS = (1e-3, 0.1, 5.0)
TEMPERATURES = (0.3, 1.0)
SEEDS = (1, 20231, 4242)         # committed: check_row asserts the perturbed top-2 gap >= 1e-3 for every sampled row that uses them
TOPK_K = (1, 2, 6, 8)


def dims(V: int) -> WhisperDims:
    return WhisperDims(f"select{V}", 8, 8, 64, 1, 64, 1, 1, V, 32)


def lp_bound(m: float) -> float:
    return 8 * U * max(abs(m), 16.0)


def prob_rel_bound(m: float, x_tok: float) -> float:
    return 8 * U * max(16.0, abs(m), abs(x_tok - m))


# ---------------------------------------------------------------------------------------------------------------- rule contexts
@dataclass(frozen=True)
class Ctx:
    """The opts struct of a launch: timestamp_begin comes from here, not from SpecialTokens.for_vocab."""
    V: int
    tag: str
    tb: int
    timestamps: bool
    eot: int
    no_timestamps: int
    no_speech: int
    suppress: Tuple[int, ...]
    begin_suppress: Tuple[int, ...]
    max_initial: Optional[int] = 50
    suppress_eot: bool = False

    def rules(self) -> R.Rules:
        return R.Rules(self.eot, self.no_timestamps, self.tb, self.suppress, self.begin_suppress, self.timestamps, self.max_initial,
                       self.suppress_eot)

    def text_tok(self) -> int:
        """a text token for histories: allowed everywhere, below eot"""
        return 0 if self.V == 7 else 5


def released_tb(V: int) -> int:
    return RELEASED_TB.get(V, 3 if V == 7 else V - 64)


def tb_modes(V: int) -> List[Tuple[str, int, bool]]:
    V4 = V & ~3
    out = [("released", released_tb(V), True)]
    if V > 49152 + 8:
        out.append(("tb49152", 49152, True))
    if V4 + 1 < V and V4 + 1 > 3:
        out.append(("tbtail", V4 + 1, True))
    out.append(("tblast", V - 1, True))
    out.append(("off", released_tb(V), False))
    return out


def make_ctx(V: int, tag: str, tb: int, timestamps: bool, max_initial: Optional[int] = 50, suppress_eot: bool = False,
             extra_suppress: Sequence[int] = ()) -> Ctx:
    if V == 7:
        eot, nots, nsp = 1, 2, 0
        sup = [0, V - 1]
        bsup = [eot]
    else:
        eot = min(50257, tb - 8)
        nots, nsp = tb - 1, tb - 2
        # chunk 0, chunk 11, the element below the timestamps, the last element
        sup = [3, 220, tb - 1, V - 1] + ([11 * 4096 + 17] if V > 11 * 4096 + 17 else [])
        bsup = [221, eot]
    sup = tuple(sorted(set(sup) | set(int(t) for t in extra_suppress)))
    return Ctx(V, tag, tb, timestamps, eot, nots, nsp, sup, tuple(bsup), max_initial, suppress_eot)


def histories(c: Ctx) -> Dict[str, List[int]]:
    t, tb, V = c.text_tok(), c.tb, c.V
    ts = min(tb + 2, V - 1)
    return {"empty": [], "text": [t], "odd": [t, ts], "pair": [t, ts, ts], "text_after_pair": [ts, ts, t],
            "odd_last": [t, V - 1], "pair_last": [V - 1, V - 1]}


# ---------------------------------------------------------------------------------------------------------------- rows
def normal_row(V: int, seed: int, scale: float = 1.0, offset: float = 0.0) -> np.ndarray:
    g = np.random.default_rng([V, seed]).standard_normal(V).astype(np.float32)
    return (g * np.float32(scale) + np.float32(offset)).astype(np.float32)


def separate(row: np.ndarray, hist: Sequence[int], c: Ctx) -> np.ndarray:
    """Construction step: when the greedy winner leads by less than 1/16 it is raised by 1/16, and a forced-timestamp margin
    closer to 0 than 1/16 is moved away by raising the best allowed timestamp by 1/4 (the margin then grows by at most that and
    at least its softmax share).  Deterministic; repeated until both hold."""
    row = row.copy()
    rules = c.rules()
    for _ in range(8):
        r = R.select_ref(row, hist, rules)
        if r.choice < 0:
            return row
        if c.timestamps and np.isfinite(r.margin) and abs(r.margin) < 1 / 16:
            s = R.apply_rules(R.torch.from_numpy(row), list(hist), rules, ts_prob_rule=False).numpy()
            best_ts = c.tb + int(np.argmax(s[c.tb:]))
            row[best_ts] += np.float32(0.25 if r.margin >= 0 else -0.25)
            continue
        if r.gap < 1 / 16:
            row[r.choice] += np.float32(0.0625) * max(1.0, abs(float(row[r.choice])) / 64)
            continue
        return row
    raise AssertionError("separate() did not converge")


def allowed_max(row: np.ndarray, hist: Sequence[int], c: Ctx) -> float:
    r = R.select_ref(row, hist, c.rules())
    return r.m if r.choice >= 0 else float(np.nanmax(row))


@dataclass
class Row:
    name: str
    row: np.ndarray
    hist: List[int]
    kind: str = "gap"          # "gap": winner leads by >= GAP; "tie": exact tie, `tie` = the two indices; "nan": partly NaN
    tie: Optional[Tuple[int, int]] = None
    margin: Optional[float] = None     # the float64 forced-timestamp margin the row was built for
    top: int = 1                       # the top `top` + 1 allowed values are separated by >= GAP or exact ties (top-k rows)
    planted: Optional[int] = None      # the index that must win (planted winners on allowed positions)


@dataclass
class RowSet:
    name: str
    ctx: Ctx
    rows: List[Row]
    _ref: Dict[Tuple, List[R.SelectRef]] = field(default_factory=dict)

    def matrix(self) -> np.ndarray:
        return np.stack([r.row for r in self.rows])

    def hist(self) -> np.ndarray:
        w = max(1, max(len(r.hist) for r in self.rows))
        h = np.full((len(self.rows), w), -1, dtype=np.int32)
        for i, r in enumerate(self.rows):
            h[i, :len(r.hist)] = r.hist
        return h

    def ref(self, k: int = 0, temperature: float = 0.0, seed: int = 0, position: int = 0, key_rows: Optional[Sequence[int]] = None,
            no_speech: bool = True) -> List[R.SelectRef]:
        key = (k, temperature, seed, position, tuple(key_rows) if key_rows is not None else None, no_speech)
        if key not in self._ref:
            rules = self.ctx.rules()
            self._ref[key] = [R.select_ref(r.row, r.hist, rules, self.ctx.no_speech if no_speech else -1, k, temperature, seed,
                                           i if key_rows is None else key_rows[i], position) for i, r in enumerate(self.rows)]
        return self._ref[key]


def chunk_indices(V: int, tb: int) -> List[int]:
    """element 0, the last element of a chunk and the first of the next, tb - 1 and tb, every tail position"""
    V4 = V & ~3
    idx = [0, 4095, 4096, 11 * 4096 + 4095, 12 * 4096, tb - 1, tb] + list(range(V4, V))
    return sorted(set(i for i in idx if 0 <= i < V))


def tie_pairs(c: Ctx) -> List[Tuple[str, int, int]]:
    """pairs of BODY indices that a one-text-token history leaves allowed in this context and that lie in one range (text): the
    same thread, two lanes, two waves, two chunks, chunk 0 against chunk 11.  Tail ties are tail_rowset's."""
    V = c.V
    if V == 7:      # one thread holds the whole body; in timestamp mode EOT is its only allowed text token
        return [] if c.timestamps else [("thread", 1, 2)]
    p = [("thread", 8, 9), ("lanes", 8, 12), ("waves", 8, 8 + 4 * 64), ("chunks", 8, 8 + 4096), ("far_chunks", 9, 9 + 11 * 4096)]
    top = min(V & ~3, c.tb if c.timestamps else V)
    return [(n, a, b) for n, a, b in p if b < top]


def hist_rowset(c: Ctx, variant: int) -> RowSet:
    """16 rows: every history kind against normal rows of every scale and offset (the combinations walk through the launches)"""
    H = histories(c)
    names = list(H)
    rows = []
    for i in range(16):
        hn = names[(i + variant) % len(names)]
        sc, off = SCALES[(i + variant) % 3], OFFSETS[(3 * i + variant) % 7]
        row = separate(normal_row(c.V, 100 * variant + i, sc, off), H[hn], c)
        rows.append(Row(f"{hn}-s{sc:g}-o{off:g}", row, H[hn]))
    return RowSet(f"hist{variant}", c, rows)


def plant_rowset(c: Ctx) -> RowSet:
    """a planted winner, 12 above everything allowed, at every index of chunk_indices; where the index is masked by the rules the
    row's own winner stands (separated like every other row)"""
    h = histories(c)["text"]
    rows = []
    for j, i in enumerate(chunk_indices(c.V, c.tb)[:16]):
        row = normal_row(c.V, 300 + j)
        row[i] = np.float32(allowed_max(row, h, c) + 12.0)
        rows.append(Row(f"plant{i}", separate(row, h, c), h))
    return RowSet("plant", c, rows)


def tie_rowset(c: Ctx) -> RowSet:
    """exact ties, bit-equal f32 values 12 above the rest at two indices (the pairs of tie_pairs), and in
    timestamp mode one text index against the only allowed timestamp at the value 0 over a row of negative logits: the
    forced-timestamp margin is then exactly 0 in every arithmetic (exp2(0) = 1, log(1) = 0), the rule stays off and the lower,
    text, index must win"""
    H = histories(c)
    rules = c.rules()
    rows = []
    for j, (n, a, b) in enumerate(tie_pairs(c)):
        h = H["text"]
        row = normal_row(c.V, 400 + j)
        s = R.apply_rules(R.torch.from_numpy(row), h, rules, ts_prob_rule=False).numpy()
        assert not np.isneginf(s[a]) and not np.isneginf(s[b]), (c.V, c.tag, n, a, b)   # built on allowed indices, never skipped
        row[a] = row[b] = np.float32(allowed_max(row, h, c) + 12.0)
        rows.append(Row(f"tie_{n}_{a}_{b}", row, h, "tie", (a, b)))
    if c.timestamps and c.tb <= c.V - 2 and c.eot < c.tb and c.V - 1 in c.suppress and not c.suppress_eot:
        h = [c.text_tok(), c.V - 2]     # allowed after this odd timestamp: text in [eot, tb) and V - 2 alone (V - 1 is suppressed)
        row = normal_row(c.V, 450, 1.0, -30.0)
        row[c.eot] = row[c.V - 2] = np.float32(0.0)
        rows.append(Row(f"tie_text_ts_{c.eot}_{c.V - 2}", row, h, "tie", (c.eot, c.V - 2), margin=0.0))
    return RowSet("tie", c, rows[:16])


def tail_rowset(c: Ctx) -> RowSet:
    """the V % 4 tail elements (held by threads 0 .. 2 in a register of their own) in a context whose suppress list leaves V - 1
    alone: an exact tie of a tail element against a body element of the same range held by another thread, an exact tie of two
    tail elements where two lie in one range, and a planted winner at every tail position"""
    V, V4 = c.V, c.V & ~3
    assert V4 < V
    c = dataclasses.replace(c, tag=c.tag + "-tail", suppress=tuple(t for t in c.suppress if t != V - 1))
    h = histories(c)["text"]
    s = R.apply_rules(R.torch.from_numpy(normal_row(V, 460)), h, c.rules(), ts_prob_rule=False).numpy()
    ok = ~np.isneginf(s)
    same = lambda a, b: not c.timestamps or ((a < c.tb) == (b < c.tb))    # noqa: E731
    tails = [i for i in range(V4, V) if ok[i]]
    assert tails, (V, c.tag)
    bodies = [int(b) for b in np.flatnonzero(ok[:V4])]
    cand = [(b, a) for a in tails for b in ([x for x in (8, c.tb + 1, 3, 1) if x in bodies] + bodies[:8] + bodies[-8:]) if same(a, b)]
    # (timestamp_begin = V - 1 on a one-element tail: the tail element is the only timestamp, its range has no body element)
    assert cand or (c.timestamps and c.tb >= V4), (V, c.tag, "no body element in the range of a tail element")
    other = [(b, a) for b, a in cand if (b % 4096) // 4 != a - V4]
    pairs = [("tail_body",) + (other[0] if other else cand[0])] if cand else []
    pairs += [("tail_lanes", a, b) for a in tails for b in tails if a < b and same(a, b)][:1]
    rows = []
    for j, (n, a, b) in enumerate(pairs):
        row = normal_row(V, 470 + j)
        row[a] = row[b] = np.float32(allowed_max(row, h, c) + 12.0)
        rows.append(Row(f"tie_{n}_{a}_{b}", row, h, "tie", (a, b)))
    for j, i in enumerate(tails):
        row = normal_row(V, 480 + j)
        row[i] = np.float32(allowed_max(row, h, c) + 12.0)
        rows.append(Row(f"plant_tail{i}", separate(row, h, c), h, planted=i))
    return RowSet("tail", c, rows)


def margin_rowset(c: Ctx) -> RowSet:
    """the timestamp range shifted by a constant so that the float64 margin is +d or -d (to the rounding of the shifted f32
    elements, asserted <= 1e-5), d in DELTAS; both winners lead their range by 1/2"""
    h = histories(c)["text"]
    rules = c.rules()
    rows = []
    for j, d in enumerate(DELTAS):
        for sign in (1.0, -1.0):
            row = normal_row(c.V, 500 + j)
            s = R.apply_rules(R.torch.from_numpy(row), h, rules, ts_prob_rule=False).numpy()
            row[int(np.argmax(s[:c.tb]))] += np.float32(0.5)
            row[c.tb + int(np.argmax(s[c.tb:]))] += np.float32(0.5)
            for _ in range(3):      # the shift, refined against the rounding of the shifted elements
                m0 = R.select_ref(row, h, rules).margin
                row[c.tb:] = (row[c.tb:].astype(np.float64) + (sign * d - m0)).astype(np.float32)
            rows.append(Row(f"margin{sign * d:+g}", row, h, "margin", margin=sign * d))
    return RowSet("margin", c, rows)


def nonfinite_rowset(c: Ctx) -> RowSet:
    """partly non-finite rows: NaN at allowed text / timestamp / tail positions (never chosen; every sum they enter is NaN), -inf
    elements (as masked), +inf at a suppressed id (masked away)"""
    H = histories(c)
    h = H["text"]
    V, tb = c.V, c.tb
    spots = {"nan_text": [c.eot] if V == 7 else [10, 4096 + 1, tb - 3], "nan_ts": [min(tb + 1, V - 1)], "nan_tail": [V - 1],
             "nan_both": [c.eot if V == 7 else 10, min(tb + 1, V - 1)]}
    rows = []
    for j, (n, idx) in enumerate(spots.items()):
        row = separate(normal_row(V, 600 + j), h, c)
        row[[i for i in idx if 0 <= i < V]] = np.nan
        rows.append(Row(n, row, h, "nan"))
    row = normal_row(V, 610)
    row[[i for i in (c.text_tok() + 1, min(tb + 1, V - 1), V - 2) if 0 <= i < V]] = -np.inf
    rows.append(Row("neg_inf", separate(row, h, c), h))
    row = separate(normal_row(V, 611), h, c)
    row[c.suppress[0]] = np.inf
    rows.append(Row("masked_pos_inf", row, h))
    return RowSet("nonfinite", c, rows)


def dead_ctx(V: int) -> Ctx:
    """rules that leave NOTHING after the odd timestamp V - 1: text below eot is masked by the timestamp rule, [eot, tb) and V - 1
    by the suppress list"""
    tb = released_tb(V)
    base = make_ctx(V, "dead", tb, True)
    return make_ctx(V, "dead", tb, True, extra_suppress=list(range(base.eot, tb)) + [V - 1])


def dead_rowset(V: int) -> RowSet:
    c = dead_ctx(V)
    H = histories(c)
    rows = [Row("masked", normal_row(V, 700), H["odd_last"]), Row("all_nan", np.full(V, np.nan, np.float32), H["text"]),
            Row("live", separate(normal_row(V, 701), H["text"], c), H["text"]), Row("all_neg_inf", np.full(V, -np.inf, np.float32), H["text"])]
    return RowSet("dead", c, rows)


def few_ctx(V: int) -> Ctx:
    """after the odd timestamp V - 2 only V - 2 and V - 1 are left: fewer than k candidates for k > 2"""
    tb = released_tb(V)
    base = make_ctx(V, "few", tb, True)
    c = make_ctx(V, "few", tb, True, extra_suppress=list(range(base.eot, tb)))
    return Ctx(V, "few", tb, True, c.eot, c.no_timestamps, c.no_speech, tuple(t for t in c.suppress if t != V - 1), c.begin_suppress)


def topk_rowset(c: Ctx) -> RowSet:
    """a ladder of 9 planted values (gaps 1, the rungs 3/4 and 6/7 exact ties) over the indices of chunk_indices and their
    neighbours: once over allowed text with the timestamps pushed down (rule off), once over timestamps (rule fires: no text id
    may come back), with and without history"""
    rules = c.rules()
    rows = []
    H = histories(c)
    for j, (hn, where) in enumerate((("text", "text"), ("text", "ts"), ("empty", "ts"), ("text_after_pair", "any"))):
        h = H[hn]
        row = normal_row(c.V, 800 + j)
        s = R.apply_rules(R.torch.from_numpy(row), h, rules, ts_prob_rule=False).numpy()
        ok = np.flatnonzero(~np.isneginf(s))
        tb = c.tb if c.timestamps else c.V
        pool = ok[ok < tb] if where == "text" else (ok[ok >= tb] if where == "ts" else ok)
        if pool.size == 0:
            continue
        pref = [i for i in chunk_indices(c.V, c.tb) + [i + 1 for i in chunk_indices(c.V, c.tb)] if i in set(pool.tolist())]
        rest = [int(i) for i in pool[np.linspace(0, pool.size - 1, min(pool.size, 12)).astype(int)] if i not in pref]
        idx = (pref + rest)[:9]
        top = float(s[ok].max())
        if where == "text" and c.timestamps:
            row[tb:] -= np.float32(40.0)            # no timestamp mass: the rule stays off
        vals = [top + 20 - r for r in range(9)]
        vals[4] = vals[3]; vals[7] = vals[6]
        for i, v in zip(idx, vals):
            row[i] = np.float32(v)
        rows.append(Row(f"ladder_{hn}_{where}", row, h, "ladder", top=min(len(idx), 9) - 1))
    return RowSet("topk", c, rows)


def few_rowset(V: int) -> RowSet:
    c = few_ctx(V)
    H = histories(c)
    h = [c.text_tok(), V - 2] if V > 7 else [0, V - 2]
    row = normal_row(V, 900)
    row[V - 1] = row[V - 2] + np.float32(1.0)
    return RowSet("few", c, [Row("two_left", row, h, "ladder", top=1)])


# ---------------------------------------------------------------------------------------------------------------- checks
def check_row(rs: RowSet, i: int) -> None:
    """the conditions a row was built for, against the float64 reference"""
    r, c = rs.rows[i], rs.ctx
    ref = R.select_ref(r.row, r.hist, c.rules(), c.no_speech, 9)
    tag = f"{c.V}/{c.tag}/{rs.name}/{r.name}"
    if r.margin is not None:
        assert abs(ref.margin - r.margin) <= 1e-5, (tag, ref.margin, r.margin)
        assert ref.forced == (r.margin > 0), tag
    elif c.timestamps and np.isfinite(ref.margin) and r.kind in ("gap", "tie"):
        assert abs(ref.margin) >= GAP, (tag, ref.margin)
    if r.kind == "gap":
        assert ref.choice < 0 or ref.gap >= GAP, (tag, ref.gap)
        assert r.planted is None or ref.choice == r.planted, (tag, ref.choice)
    elif r.kind == "margin":    # the text winner leads the timestamps by the margin itself (max <= logsumexp), its range by 1/2
        assert ref.gap >= min(abs(r.margin) - 1e-5, 0.25), (tag, ref.gap)
    elif r.kind == "tie":
        a, b = r.tie
        assert ref.choice == a and r.row[a].tobytes() == r.row[b].tobytes() and ref.gap == 0.0, (tag, ref.choice, ref.gap)
        assert ref.topk_id[1] == b and ref.topk_lp[0] == ref.topk_lp[1], tag
    elif r.kind == "nan":
        live = ~np.isnan(r.row)
        assert ref.choice >= 0 and live[ref.choice] and not np.isnan(ref.m), tag
    elif r.kind == "ladder":
        v = ref.topk_lp[:r.top + 1]
        d = -np.diff(v[np.isfinite(v)])
        assert np.all((d == 0) | (d >= GAP)), (tag, d)


def check_sampled(rs: RowSet, temperature: float, seed: int, position: int) -> None:
    for i, ref in enumerate(rs.ref(0, temperature, seed, position)):
        if ref.choice >= 0:
            assert ref.sample_gap >= GAP, (rs.ctx.V, rs.ctx.tag, rs.name, rs.rows[i].name, temperature, seed, ref.sample_gap)


@functools.lru_cache(maxsize=None)
def rowsets(V: int) -> Tuple[RowSet, ...]:
    """every row set of one vocabulary: the history and planted-winner sets for each timestamp_begin, ties, margins, non-finite
    rows, top-k ladders (max_initial and suppress_eot walk through the modes)"""
    out = []
    modes = tb_modes(V)
    if V in (51864, 53248):     # no tail and nothing new at the boundary: the released value and timestamps off
        modes = [m for m in modes if m[0] in ("released", "off")]
    for j, (tag, tb, ts) in enumerate(modes):
        mi = (50, None, 0)[j % 3]
        a = make_ctx(V, tag, tb, ts, mi, False)
        b = make_ctx(V, tag + "-noeot", tb, ts, (None, 0, 50)[j % 3], True)
        out += [hist_rowset(a, 0), hist_rowset(b, 1), plant_rowset(a), tie_rowset(a), topk_rowset(a)]
        if V & 3:
            out.append(tail_rowset(a))
        if ts:
            if tb < V - 1:
                out.append(margin_rowset(a))
            out.append(nonfinite_rowset(a))
    out.append(few_rowset(V))
    return tuple(r for r in out if r.rows)
