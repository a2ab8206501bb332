"""CPU: the float64 selection reference (oracle/whisper_ref.py select_ref), the case table (tests/select_cases.py) and the bounds of
tests/test_gpu_select_kernels.py, checked without a GPU:
  * select_ref against torch.log_softmax and apply_rules on the rows of tests/golden/rules.npz;
  * every condition the table's rows were built for (winner gaps, exact ties, forced-timestamp margins, sampled top-2 gaps);
  * a numpy model of the selection kernels' data layout and arithmetic - 13 chunks x 1024 threads x 4 elements, loaded clamped
    and unconditionally, with the tail on the first threads, the interval form of the rules, (max, lowest index) merges, f32 sums in thread, wave and 16-wave order with
    exactly rounded exp2 / log - which the table and the bounds ACCEPT, and which they REJECT with any one of nine defects
    switched on (DEFECTS below).  So the GPU test would notice each of those mistakes in a kernel."""
import os

import numpy as np
import pytest
import torch

import select_cases as S
from oracle import whisper_ref as R

torch.set_grad_enabled(False)
BIG = 0x7fffffff
LOG2E = np.float32(1.4426950408889634)
DEFECTS = ("tie_high", "tail_dropped", "tb_inclusive", "norm_text_only", "ts_floor_odd", "ns_processed", "topk_keeps_winner",
           "key_without_position", "last_ts_without_timestamps")
f32 = np.float32


def _tree(x):
    """wave-wide sum of 64 lanes as a butterfly: pairwise, in f32"""
    x = x.astype(np.float32)
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(np.float32)
    return x[..., 0]


def _block_sum(per_thread):
    """1024 per-thread partial sums -> wave sums (butterfly) -> thread 0 adds the 16 waves in order"""
    waves = _tree(per_thread.reshape(16, 64))
    t = f32(0)
    for w in waves:
        t = f32(t + w)
    return t


def _exp2(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp2(a.astype(np.float64)).astype(np.float32)


def _log(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(np.log(np.float64(x)))


def _best(vals, idx, high=False):
    """(max, lowest index among equals) over candidates; NaN and -inf are never taken (`v > a.v` from -inf)"""
    v = np.where(np.isnan(vals), -np.inf, vals)
    if v.size == 0 or not (v > -np.inf).any():
        return f32(-np.inf), BIG
    m = v.max()
    hit = idx[v == m]
    return f32(m), int(hit.max() if high else hit.min())


def kernel_model(row, hist, c: S.Ctx, k=0, temperature=0.0, seed=0, key_row=0, position=0, defect=None):
    """what select_body / beam_topk_kernel compute for one row, restated on the kernels' data layout"""
    row = np.asarray(row, np.float32)
    V, tb, n = c.V, c.tb, len(hist)
    V4 = V & ~3
    # ---- the rules as intervals (make_ranges / masked_mk)
    last, pen = (hist[-1] if n else -1), (hist[-2] if n > 1 else -1)
    ts_hist = [t for t in hist if t >= tb] if c.timestamps else []
    lts = ts_hist[-1] if ts_hist else -1
    last_is_ts, pen_is_ts = n >= 1 and last >= tb, n < 2 or pen >= tb
    odd = last_is_ts and not pen_is_ts
    ts_floor = ((lts if (odd and defect != "ts_floor_odd") else lts + 1) if lts >= 0 else 0)
    q_tb = tb if c.timestamps else BIG
    txt_lo = 0 if not c.timestamps else (BIG if n == 0 else (c.eot if odd else 0))
    ts_lo = BIG if (last_is_ts and pen_is_ts) else max(tb, ts_floor)
    ts_hi = tb + c.max_initial if (n == 0 and c.max_initial is not None) else BIG
    mk = np.zeros(V, np.uint8)
    mk[list(c.suppress)] |= 1
    mk[list(c.begin_suppress)] |= 2

    def masked_at(idx, byte):
        """masked_mk: the mask byte that was LOADED with the element, the interval tests on the element's own index"""
        in_txt, in_ts = (idx < q_tb) & (idx >= txt_lo), (idx >= q_tb) & (idx >= ts_lo) & (idx <= ts_hi)
        return ((byte & (3 if n == 0 else 1)) != 0) | (idx == (c.eot if c.suppress_eot else -1)) \
            | (idx == (c.no_timestamps if c.timestamps else -1)) | ~(in_txt | in_ts)

    s = np.where(masked_at(np.arange(V), mk), f32(-np.inf), row).astype(np.float32)     # the processed row, for the outputs
    # ---- load_row_regs: thread t requests 4 elements at min(4 t + 4096 k, V4 - 4) (never below 0) for EVERY chunk k = 0 .. 12 and
    # the tail element min(V4 + t, V - 1): clamped and unconditional.  A register is named by its own index 4 t + 4096 k + j; the
    # passes visit it only where the chunk start is below V4 (the tail: V4 + t < V), and there the clamp has moved nothing.
    t, j4 = np.arange(1024), np.arange(4)
    start = np.arange(13)[None, :] * 4096 + t[:, None] * 4
    load = np.maximum(np.minimum(start, V4 - 4), 0)
    own, src = (start[:, :, None] + j4).reshape(1024, 52), (load[:, :, None] + j4).reshape(1024, 52)
    rowp, mkp = np.concatenate([row, np.zeros(4, np.float32)]), np.concatenate([mk, np.zeros(4, np.uint8)])
    body = np.where(masked_at(own, mkp[src]), f32(-np.inf), rowp[src])
    body_held = np.repeat(start < V4, 4, axis=1)
    tail_own, tail_src = V4 + t, np.minimum(V4 + t, V - 1)
    tail = np.where(masked_at(tail_own, mk[tail_src]), f32(-np.inf), row[tail_src])
    tail_held = (tail_own < V) & (defect != "tail_dropped")
    held = np.concatenate([body_held, tail_held[:, None]], axis=1)
    own, src = np.concatenate([own, tail_own[:, None]], axis=1), np.concatenate([src, tail_src[:, None]], axis=1)
    assert np.array_equal(own[held], src[held])     # what is visited was loaded from its own place
    P = np.where(held, own, -1)
    vals = np.where(held, np.concatenate([body, tail[:, None]], axis=1), f32(-np.inf)).astype(np.float32)
    is_txt = (P <= q_tb) if defect == "tb_inclusive" else (P < q_tb)
    high = defect == "tie_high"
    mx_txt, i_txt = _best(vals[held & is_txt], P[held & is_txt], high)
    mx_ts, i_ts = _best(vals[held & ~is_txt], P[held & ~is_txt], high)
    mx_all = f32(max(mx_txt, mx_ts))
    mref = f32((f32(0) if mx_all == -np.inf else mx_all) * LOG2E)
    with np.errstate(invalid="ignore", over="ignore"):
        arg = (vals.astype(np.float64) * np.float64(LOG2E) - np.float64(mref)).astype(np.float32)    # fmaf: one rounding
    ex = np.where(held, _exp2(arg), f32(0)).astype(np.float32)
    acc = np.zeros((2, 1024), np.float32)
    for col in range(P.shape[1]):       # a thread adds its elements in index order, each to its range's sum
        acc[0] = (acc[0] + np.where(is_txt[:, col], ex[:, col], f32(0))).astype(np.float32)
        acc[1] = (acc[1] + np.where(~is_txt[:, col], ex[:, col], f32(0))).astype(np.float32)
    t0, t1 = _block_sum(acc[0]), _block_sum(acc[1])
    # ---- no-speech probability of the unprocessed row (strided pass from memory)
    src = s if defect == "ns_processed" else row
    out = {"masked": np.isneginf(s)}
    if c.no_speech >= 0:
        mx_raw = f32(np.nanmax(np.where(np.isnan(src), -np.inf, src)))
        pad = np.full(-(-V // 1024) * 1024, f32(-np.inf), np.float32)
        pad[:V] = src
        with np.errstate(invalid="ignore", over="ignore"):
            er = np.exp((pad - mx_raw).astype(np.float32).astype(np.float64)).astype(np.float32).reshape(-1, 1024)
        a = np.zeros(1024, np.float32)
        for j in range(er.shape[0]):
            a = (a + er[j]).astype(np.float32)
        t2 = _block_sum(a)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out["no_speech"] = f32(f32(np.exp(np.float64(f32(src[c.no_speech] - mx_raw)))) / t2)
    # ---- thread 0: the forced-timestamp rule, the log-normaliser, the choice
    with np.errstate(invalid="ignore", over="ignore"):
        force = bool(c.timestamps and t1 > 0 and f32(_log(t1) + mx_all) > mx_txt)
        if force:
            choice, cv, lse = i_ts, mx_ts, f32(_log(t1) + mx_all)
        else:
            pick_ts = mx_ts > mx_txt
            choice, cv = (i_ts, mx_ts) if pick_ts else (i_txt, mx_txt)
            lse = f32(_log(t0 if defect == "norm_text_only" else f32(t0 + t1)) + mx_all)
        live = choice != BIG
        if not live:
            choice, cv, lse = c.eot, f32(-np.inf), f32(0)
        out.update(forced=force, choice=choice, lp=f32(cv - lse))
        # ---- Gumbel-max pass
        if temperature > 0 and live:
            g = R.sample_gumbel(seed, key_row, 0 if defect == "key_without_position" else position, V)
            ok = held & ~np.isneginf(vals) & ~np.isnan(vals) & ~(force & (P < tb))
            z = (vals[ok] / f32(temperature)).astype(np.float32) + g[P[ok]]
            _, sc = _best(z.astype(np.float32), P[ok])
            if sc != BIG:
                choice = sc
                out.update(choice=sc, lp=f32(row[sc] - lse))
        # ---- candidates: k rounds of argmax over what is left
        if k:
            left = vals.copy()
            if force:
                left[is_txt] = -np.inf
            ids, lps = [], []
            for _ in range(k):
                v, w = _best(left[held], P[held])
                ids.append(-1 if w == BIG else w)
                lps.append(f32(-np.inf) if w == BIG else f32(v - lse))
                if defect != "topk_keeps_winner":
                    left[P == w] = -np.inf
            out.update(topk_id=np.array(ids), topk_lp=np.array(lps, np.float32))
    out["last_ts"] = choice if (choice >= tb and (c.timestamps or defect == "last_ts_without_timestamps")) else lts
    return out


def judge(rs, i, defect=None, ratios=None):
    """the checks of test_gpu_select_kernels on one row of the table, applied to the model; returns what failed"""
    r, c = rs.rows[i], rs.ctx
    bad = []
    ref = rs.ref(8)[i]
    got = kernel_model(r.row, r.hist, c, k=8, defect=defect)

    def close(what, g, w, bound):
        g, w = float(g), float(w)
        if not np.isfinite(w):
            if not ((np.isnan(g) and np.isnan(w)) or g == w):
                bad.append(what)
            return
        if ratios is not None:
            ratios[what] = max(ratios.get(what, 0.0), abs(g - w) / bound)
        if abs(g - w) > bound:
            bad.append(what)

    if not np.array_equal(got["masked"] | (got["forced"] & (np.arange(c.V) < c.tb)), ref.masked):
        bad.append("mask")
    want_choice, want_lp = (ref.choice, ref.lp) if ref.choice >= 0 else (c.eot, -np.inf)
    if got["choice"] != want_choice:
        bad.append("choice")
    close("lp", got["lp"], want_lp, S.lp_bound(ref.m if ref.choice >= 0 else 0.0))
    st = R.select_transition(R.select_history(r.hist, c.rules()), 3, want_choice, want_lp, c.rules(), S.MAX_NEW, 1 << 30)
    if got["last_ts"] != st.last_ts:
        bad.append("last_ts")
    if ref.no_speech is not None and np.isfinite(ref.no_speech) and ref.no_speech > 0:
        mr = float(np.nanmax(r.row))
        close("no_speech", got["no_speech"], ref.no_speech, S.prob_rel_bound(mr, float(r.row[c.no_speech])) * ref.no_speech)
    if not np.array_equal(got["topk_id"], ref.topk_id):
        bad.append("topk_id")
    else:
        for q in range(8):
            close("topk_lp", got["topk_lp"][q], ref.topk_lp[q], S.lp_bound(ref.m))
    if rs.name == "hist0" and ref.choice >= 0:
        for j, T in enumerate(S.TEMPERATURES):      # the launches of test_gpu_select_kernels.test_sampled: committed seeds, position 5
            seed, pos = S.SEEDS[(j + len(c.tag)) % len(S.SEEDS)], 5
            sref = rs.ref(0, T, seed, pos)[i]
            assert sref.sample_gap >= S.GAP, (c.V, c.tag, r.name, T, seed, sref.sample_gap)
            sg = kernel_model(r.row, r.hist, c, temperature=T, seed=seed, key_row=i, position=pos, defect=defect)
            if sg["choice"] != sref.sample_choice:
                bad.append("sample_choice")
            close("sample_lp", sg["lp"], sref.sample_lp, S.lp_bound(sref.m))
    return bad


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_select_ref_matches_log_softmax_and_apply_rules(golden_dir):
    g = np.load(os.path.join(golden_dir, "rules.npz"))
    V = g["rows"].shape[1]
    tb = V - 64
    for ts, key in ((True, "out_ts"), (False, "out_nots")):
        rules = R.Rules(tb - 8, tb - 1, tb, g["suppress"].tolist(), g["begin_suppress"].tolist(), ts)
        for row, hist, want in zip(g["rows"], g["hist"], g[key]):
            h = [int(t) for t in hist if t >= 0]
            ref = R.select_ref(row, h, rules, no_speech=tb - 2, k=5)
            np.testing.assert_array_equal(ref.masked, np.isneginf(want))            # the golden processed rows (HF code)
            s = R.apply_rules(torch.from_numpy(row), h, rules)
            np.testing.assert_array_equal(ref.masked, np.isneginf(s.numpy()))
            lsm = torch.log_softmax(s.double(), -1)
            assert ref.choice == int(want.argmax()) == int(lsm.argmax())
            assert abs(ref.lp - float(lsm[ref.choice])) < 1e-12 and abs(ref.lse - float(torch.logsumexp(s.double(), -1))) < 1e-12
            top = torch.topk(lsm, 5)
            np.testing.assert_array_equal(ref.topk_id, top.indices.numpy())
            np.testing.assert_allclose(ref.topk_lp, top.values.numpy(), atol=1e-12, rtol=0)
            raw = torch.softmax(torch.from_numpy(row).double(), -1)
            assert abs(ref.no_speech - float(raw[tb - 2])) < 1e-15
            if ts:
                m = []
                R.apply_rules(torch.from_numpy(row), h, rules, ts_prob_margin=m)
                assert ref.forced == (m[0] > 0) and (not np.isfinite(m[0]) or abs(ref.margin - m[0]) < 1e-4)


def test_select_transition_restates_the_state_update():
    rules = R.Rules(440, 447, 448)
    st = R.select_history([5, 450], rules)
    assert (st.n_sampled, st.last_tok, st.pen_tok, st.last_ts) == (2, 450, 5, 450)
    a = R.select_transition(st, 4, 451, -0.5, rules, 16, 3)
    assert (a.cur_tok, a.n_sampled, a.last_tok, a.pen_tok, a.last_ts, a.done, a.stored, a.sum_logprob) == (451, 3, 451, 450, 451, 1, (2, 451), -0.5)
    st.done = 1
    b = R.select_transition(st, 4, 451, -0.5, rules, 16, 3, rows_form=True)
    assert (b.cur_tok, b.n_sampled, b.done, b.newly_done, b.advanced, b.stored) == (440, 2, 1, False, False, None)
    c = R.select_transition(R.select_history([], rules), 1, 7, -1.0, rules, 16, 16, prompt=[1, 2, 3, 4], sot_index=1, want_no_speech=True)
    assert (c.cur_tok, c.n_sampled, c.captured_ns, c.chose) == (3, 0, True, False)
    off = R.Rules(440, 447, 448, timestamps=False)
    assert R.select_transition(R.select_history([450], off), 1, 451, 0.0, off, 16, 16).last_ts == -1


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("V", S.VOCABS)
def test_table_conditions_hold(V):
    sets = S.rowsets(V) + (S.dead_rowset(V),)
    assert all(1 <= len(rs.rows) <= S.MAX_BATCH for rs in sets)
    for rs in sets:
        for i in range(len(rs.rows)):
            S.check_row(rs, i)
        if rs.name == "hist0":
            for j, T in enumerate(S.TEMPERATURES):
                S.check_sampled(rs, T, S.SEEDS[(j + len(rs.ctx.tag)) % len(S.SEEDS)], 5)
    # every tie kind is present (a kind is left out only where the vocabulary cannot hold it)
    ties = {"_".join(r.name.split("_")[1:-2]) for rs in sets for r in rs.rows if r.kind == "tie"}
    want = {"text_ts"} | ({"thread", "lanes", "waves"} if V >= 512 else {"thread"}) | ({"chunks", "far_chunks"} if V > 12 * 4096 else set()) \
        | ({"tail_body"} if V & 3 else set()) | ({"tail_lanes"} if V & 3 >= 2 else set())
    assert want <= ties, (V, want - ties)
    for rs in sets:     # tail ties and tail plants in the released and the timestamps-off context of every vocabulary with a tail
        if rs.name == "tail" and rs.ctx.tag in ("released-tail", "off-tail"):
            assert any(r.name.startswith("tie_tail_body") for r in rs.rows) and any(r.planted is not None for r in rs.rows), (V, rs.ctx.tag)
    assert not (V & 3) or {rs.ctx.tag for rs in sets if rs.name == "tail"} >= {"released-tail", "off-tail"}
    names = {rs.name for rs in sets}
    assert {"hist0", "hist1", "plant", "tie", "topk", "few", "dead"} <= names
    d = S.dead_rowset(V).ref()
    assert [x.choice for x in d] == [-1, -1, d[2].choice, -1] and d[2].choice >= 0


MODEL_VOCABS = (7, 512, 51866)


@pytest.mark.parametrize("V", MODEL_VOCABS)
def test_table_accepts_the_kernel_model(V):
    """the layout model passes every check; its largest error / bound stays far from 1 (exact transcendentals)"""
    ratios = {}
    for rs in S.rowsets(V) + (S.dead_rowset(V),):
        for i in range(len(rs.rows)):
            assert judge(rs, i, None, ratios) == [], (V, rs.ctx.tag, rs.name, rs.rows[i].name)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 0.5, ratios


@pytest.mark.parametrize("defect", DEFECTS)
def test_table_rejects_a_defective_model(defect):
    """each defect is caught by at least one row of the table at the GPU test's bounds, at a Whisper vocabulary (51866: a tail of
    two elements, the released timestamp_begin inside chunk 12)"""
    caught = []
    for V in (51866,):
        for rs in S.rowsets(V):
            if defect == "tb_inclusive" and not rs.ctx.tag.startswith("tb49152"):
                continue        # this one must be seen where timestamp_begin is a chunk boundary: element tb opens chunk 12
            for i in range(len(rs.rows)):
                bad = judge(rs, i, defect)
                if bad:
                    caught.append((V, rs.ctx.tag, rs.name, rs.rows[i].name, bad))
                    break
            if len(caught) >= 3:
                break
        if len(caught) >= 3:
            break
    assert caught, defect
    print(defect, caught[:3])
