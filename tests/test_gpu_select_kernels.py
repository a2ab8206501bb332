"""GPU: the token-selection kernels of kernels_decode.hip - select_kernel<SAMPLE, false>, select_rows_kernel<SAMPLE>,
session_rows_select_kernel, beam_topk_kernel, token_logprob_kernel, token_prob_kernel - one launch at a time against the float64
reference (oracle/whisper_ref.py select_ref / select_transition), through the known-answer hook ttasr_select_probe (DESIGN.md
section 4.33).  Rows, rule contexts and the derived tolerances live in tests/select_cases.py; tests/test_select_reference_host.py
shows on the CPU that the table and the bounds see the defects they are there for.

Every launch: the signature names the instantiation; mask-dependent results (choice, candidate ids and their order) and every
integer state field are exact; log-probability increments, candidate values and token_logprob lie within 8 u max(|m|, 16) of the
reference, the no-speech probability and token_prob within 8 u max(16, |m|, |x_tok - m|) relative (a NaN where the reference is
NaN).  Engines: f32, 1 + 1 layers, one head, max_batch 16, one per vocabulary per module; no weights are loaded (the hook needs
none).  Largest error / bound per (form, quantity): printed by the last test, recorded in profiles/select_kernels.jsonl."""
import ctypes as C

import numpy as np
import pytest
import torch

import select_cases as S
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

RATIOS = {}     # (form, quantity) -> largest observed error / bound
POS = 3         # the position of the step launches


@pytest.fixture(scope="module")
def engines():
    from taiwan_tongues_asr_ce_amd.engine import Engine
    made = {}

    def get(V):
        if V not in made:
            made[V] = Engine(S.dims(V), COMPUTE_F32, S.MAX_BATCH)
        return made[V]
    yield get
    for e in made.values():
        e.close()


def make_opts(c: S.Ctx, sot_index: int = 0, max_new: int = S.MAX_NEW, no_speech: bool = True):
    o = _lib.GenOpts()
    sup, bsup = np.asarray(c.suppress, dtype=np.int32), np.asarray(c.begin_suppress, dtype=np.int32)
    o.max_new_tokens, o.eot, o.no_timestamps, o.timestamp_begin = max_new, c.eot, c.no_timestamps, c.tb
    o.no_speech, o.sot_index, o.timestamps = (c.no_speech if no_speech else -1), sot_index, int(c.timestamps)
    o.max_initial_timestamp_index = -1 if c.max_initial is None else c.max_initial
    o.suppress_eot, o.n_suppress, o.n_begin_suppress, o.check_interval = int(c.suppress_eot), len(sup), len(bsup), 1
    o.suppress, o.begin_suppress = sup.ctypes.data_as(C.POINTER(C.c_int32)), bsup.ctypes.data_as(C.POINTER(C.c_int32))
    o._keep = (sup, bsup)
    return o


def note(form, what, err, bound):
    RATIOS[(form, what)] = max(RATIOS.get((form, what), 0.0), float(err) / bound)


def close(form, what, got, want, bound, tag):
    """got within `bound` of the float64 `want`; non-finite values must agree exactly"""
    got, want = float(got), float(want)
    if not np.isfinite(want):
        assert (np.isnan(got) and np.isnan(want)) or got == want, (tag, form, what, got, want)
        return
    note(form, what, abs(got - want), bound)
    assert abs(got - want) <= bound, (tag, form, what, got, want, abs(got - want) / bound)


def close_prob(form, what, got, want, m, x_tok, tag):
    if not np.isfinite(want) or want == 0.0:
        close(form, what, got, want, 0.0, tag)
        return
    close(form, what, got, want, S.prob_rel_bound(m, x_tok) * want, tag)


def same_bits(a, b, tag):
    """equal bit for bit; NaNs need only be NaNs on both sides"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool), np.isnan(b) if b.dtype.kind == "f" else np.zeros(b.shape, bool)
    np.testing.assert_array_equal(na, nb, err_msg=tag)
    np.testing.assert_array_equal(a[~na].tobytes(), b[~nb].tobytes(), err_msg=tag)


def raw_max(row):
    return float(np.nanmax(row)) if not np.isnan(row).all() else float("nan")


def expect_rows(rs, refs, choices, lps, positions, sot_index, rows_form, done0=None, caps=None, sum0=None, prompt=None, plen=None):
    """the state after the launch, by select_transition"""
    rules = rs.ctx.rules()
    out = []
    for i, r in enumerate(rs.rows):
        st = R.select_history(r.hist, rules)
        st.done = int(done0[i]) if done0 is not None else 0
        st.sum_logprob = float(sum0[i]) if sum0 is not None else 0.0
        pr = None if prompt is None else list(prompt[i][:plen[i]])
        ch, lp = (choices[i], lps[i]) if choices[i] >= 0 else (rs.ctx.eot, -np.inf)
        out.append(R.select_transition(st, int(positions[i]), int(ch), float(lp), rules, S.MAX_NEW,
                                       int(caps[i]) if caps is not None else 1 << 30, pr, sot_index, rs.ctx.no_speech >= 0, rows_form))
    return out


def check_state(form, rs, res, exp, refs, n_done0, positions, tag, sum0=None):
    n = len(rs.rows)
    for i, (r, x) in enumerate(zip(rs.rows, exp)):
        t = f"{tag}/{r.name}"
        ints = dict(cur_tok=x.cur_tok, n_sampled=x.n_sampled, last_tok=x.last_tok, pen_tok=x.pen_tok, last_ts=x.last_ts, done=x.done)
        for k, v in ints.items():
            assert int(res[k][i]) == v, (t, k, int(res[k][i]), v)
        assert 0 <= int(res["cur_tok"][i]) < rs.ctx.V, t
        want = np.full(S.MAX_NEW, -1, dtype=np.int32)
        if x.stored:
            want[x.stored[0]] = x.stored[1]
        np.testing.assert_array_equal(res["out_tokens"][i], want, err_msg=t)
        s0 = float(sum0[i]) if sum0 is not None else 0.0
        if x.chose:
            # a chosen row: f32(sum + increment).  From a sum of 0 the add is exact and the bound is the increment's alone; a
            # non-zero sum rounds the add by at most u |sum|
            m = refs[i].m if refs[i].choice >= 0 else 0.0
            add = S.U * abs(x.sum_logprob) if (s0 != 0.0 and np.isfinite(x.sum_logprob)) else 0.0
            close(form, "lp", res["sum_logprob"][i], x.sum_logprob, S.lp_bound(m) + add, t)
        else:
            assert float(res["sum_logprob"][i]) == np.float32(s0), (t, "sum untouched")
        if x.captured_ns:
            mr = raw_max(r.row)
            close_prob(form, "no_speech", res["no_speech"][i], refs[i].no_speech, mr, float(r.row[rs.ctx.no_speech]), t)
        else:
            assert float(res["no_speech"][i]) == 0.0, (t, "no_speech untouched")
    assert int(res["n_done"][0]) == n_done0 + sum(x.newly_done for x in exp), (tag, "n_done")
    if form.startswith("step"):
        assert res["positions"].tolist() == [int(positions[0]) + 1, 0], (tag, "step advances once, ticket word 0", res["positions"])
    else:
        assert res["positions"].tolist() == [int(p) + int(x.advanced) for p, x in zip(positions, exp)], (tag, "live rows advance")


@pytest.mark.parametrize("V", S.VOCABS)
def test_step_greedy(engines, V):
    """select_kernel<false, false>: every row set; the history sets capture the no-speech probability (position = sot_index)"""
    e = engines(V)
    for rs in S.rowsets(V):
        n, tag = len(rs.rows), f"{V}/{rs.ctx.tag}/{rs.name}"
        sot = POS if rs.name.startswith("hist") else 0
        refs = rs.ref()
        res = e.select_probe("step", rs.matrix(), make_opts(rs.ctx, sot), rs.hist(), [POS])
        assert res["sig"] == f"select_kernel<false, false> grid {n * 1024}", res["sig"]
        exp = expect_rows(rs, refs, [r.choice for r in refs], [r.lp for r in refs], [POS] * n, sot, False)
        check_state("step", rs, res, exp, refs, 0, [POS], tag)


@pytest.mark.parametrize("V", S.VOCABS)
def test_rows_greedy(engines, V):
    """select_rows_kernel<false>: per-row positions (rows at sot_index = 2 capture the no-speech probability), finished rows are
    fed EOT with their state and position untouched, n_done counts on from its initial value"""
    e = engines(V)
    for rs in S.rowsets(V):
        n, tag = len(rs.rows), f"{V}/{rs.ctx.tag}/{rs.name}"
        pos = [1 + i % 3 for i in range(n)]
        done0 = [int(i % 5 == 4) for i in range(n)]
        sum0 = [np.float32(-1.5 * (i % 4)) for i in range(n)]
        refs = rs.ref()
        res = e.select_probe("rows", rs.matrix(), make_opts(rs.ctx, 2), rs.hist(), pos, done=done0, sum_logprob=sum0, n_done=sum(done0))
        assert res["sig"] == f"select_rows_kernel<false> grid {n * 1024}", res["sig"]
        exp = expect_rows(rs, refs, [r.choice for r in refs], [r.lp for r in refs], pos, 2, True, done0, sum0=sum0)
        check_state("rows", rs, res, exp, refs, sum(done0), pos, tag, sum0)


@pytest.mark.parametrize("V", S.VOCABS)
def test_session_equals_step(engines, V):
    """session_rows_select_kernel at (key row, position, temperature 0) returns the choice, the increment and the no-speech
    probability of select_kernel for that row, bit for bit; an entry that only captures returns choice -1"""
    e = engines(V)
    for rs in S.rowsets(V):
        n, tag = len(rs.rows), f"{V}/{rs.ctx.tag}/{rs.name}"
        opts = make_opts(rs.ctx, POS)
        st = e.select_probe("step", rs.matrix(), opts, rs.hist(), [POS])
        ent = [[i, POS, i, 3] for i in range(n)] + [[0, POS, 0, 2]]
        ent = ent[:S.MAX_BATCH]
        se = e.select_probe("session", rs.matrix(), opts, rs.hist(), entries=ent, entry_temp=[0.0] * len(ent), entry_seed=[0] * len(ent))
        assert se["sig"] == f"session_rows_select_kernel grid {len(ent) * 1024}", se["sig"]
        k = min(n, len(ent))
        same_bits(se["choice"][:k], st["cur_tok"][:k], tag)
        same_bits(se["lp"][:k], st["sum_logprob"][:k], tag)
        same_bits(se["no_speech"][:k], st["no_speech"][:k], tag)
        if len(ent) > n:
            assert se["choice"][n] == -1, tag
            same_bits(se["no_speech"][n:n + 1], st["no_speech"][:1], tag)


@pytest.mark.parametrize("V", S.VOCABS)
def test_sampled(engines, V):
    """select_kernel<true, false>, select_rows_kernel<true> and the session kernel at temperature > 0: the Gumbel-max choice of the
    reference (its perturbed top-2 gap is >= 1e-3 for the committed seeds), the increment within the bound, the three forms equal
    bit for bit; another position draws with another key"""
    e = engines(V)
    pos = 5
    for rs in S.rowsets(V):
        if rs.name != "hist0":
            continue
        n = len(rs.rows)
        for j, T in enumerate(S.TEMPERATURES):
            seed = S.SEEDS[(j + len(rs.ctx.tag)) % len(S.SEEDS)]
            tag = f"{V}/{rs.ctx.tag}/{rs.name}/T{T}/seed{seed}"
            S.check_sampled(rs, T, seed, pos)
            refs = rs.ref(0, T, seed, pos)
            opts = make_opts(rs.ctx, 0)
            st = e.select_probe("step", rs.matrix(), opts, rs.hist(), [pos], temperature=T, seed=seed)
            assert st["sig"] == f"select_kernel<true, false> grid {n * 1024}", st["sig"]
            exp = expect_rows(rs, refs, [r.sample_choice for r in refs], [r.sample_lp for r in refs], [pos] * n, 0, False)
            check_state("step_sampled", rs, st, exp, refs, 0, [pos], tag)
            ro = e.select_probe("rows", rs.matrix(), opts, rs.hist(), [pos] * n, temperature=T, seed=seed)
            assert ro["sig"] == f"select_rows_kernel<true> grid {n * 1024}", ro["sig"]
            se = e.select_probe("session", rs.matrix(), opts, rs.hist(), entries=[[i, pos, i, 1] for i in range(n)],
                                entry_temp=[T] * n, entry_seed=[seed] * n)
            for other, ch, lp in ((ro, ro["cur_tok"], ro["sum_logprob"]), (se, se["choice"], se["lp"])):
                same_bits(ch, st["cur_tok"], tag)
                same_bits(lp, st["sum_logprob"], tag)


@pytest.mark.parametrize("V", S.VOCABS)
def test_topk(engines, V):
    """beam_topk_kernel, k in {1, 2, 6, 8}: ids in reference order (value descending, id ascending among exact equals), no text id
    when the timestamp rule fires, -1 / -inf where fewer than k tokens are allowed, values within the bound; the no-speech output
    on and off"""
    e = engines(V)
    for rs in S.rowsets(V):
        if rs.name not in ("topk", "tie", "tail", "few", "hist0", "nonfinite", "margin", "plant"):
            continue
        n = len(rs.rows)
        refs = rs.ref(8)
        for k in S.TOPK_K:
            tag = f"{V}/{rs.ctx.tag}/{rs.name}/k{k}"
            want_ns = k in (2, 6)
            res = e.select_probe("topk", rs.matrix(), make_opts(rs.ctx, 0), rs.hist(), k=k, want_no_speech=want_ns)
            assert res["sig"] == f"beam_topk_kernel grid {n * 1024} k {k}", res["sig"]
            for i, (r, ref) in enumerate(zip(rs.rows, refs)):
                t = f"{tag}/{r.name}"
                np.testing.assert_array_equal(res["id"][i], ref.topk_id[:k], err_msg=t)
                if ref.forced:
                    assert all(j < 0 or j >= rs.ctx.tb for j in res["id"][i]), t
                for q in range(k):
                    close("topk", "lp", res["lp"][i, q], ref.topk_lp[q], S.lp_bound(ref.m), t)
                if want_ns:
                    close_prob("topk", "no_speech", res["no_speech"][i], ref.no_speech, raw_max(r.row), float(r.row[rs.ctx.no_speech]), t)


@pytest.mark.parametrize("V", S.VOCABS)
def test_token_logprob_and_prob(engines, V):
    """token_logprob_kernel and token_prob_kernel on the raw rows of the history sets (every scale and offset)"""
    e = engines(V)
    for rs in S.rowsets(V):
        if not rs.name.startswith("hist"):
            continue
        rows = rs.matrix().astype(np.float64)
        n = len(rows)
        lse = np.array([x.max() + np.log(np.exp(x - x.max()).sum()) for x in rows])
        picks = [0, V - 1, int(rows[2].argmax()) if n > 2 else 0, min(rs.ctx.tb, V - 1), V // 2]
        targets = [picks[i % len(picks)] if i != 2 else picks[2] for i in range(n)]
        tag = f"{V}/{rs.ctx.tag}/{rs.name}"
        res = e.select_probe("logprob", rs.matrix(), targets=targets)
        assert res["sig"] == f"token_logprob_kernel grid {n * 256}", res["sig"]
        for i in range(n):
            close("logprob", "lp", res["out"][i], rows[i, targets[i]] - lse[i], S.lp_bound(rows[i].max()), f"{tag}/{i}")
        tok = rs.ctx.no_speech
        res = e.select_probe("prob", rs.matrix(), token=tok)
        assert res["sig"] == f"token_prob_kernel grid {n * 256}", res["sig"]
        for i in range(n):
            close_prob("prob", "p", res["out"][i], np.exp(rows[i, tok] - lse[i]), rows[i].max(), rows[i, tok], f"{tag}/{i}")


@pytest.mark.parametrize("V", (512, 51865))
@pytest.mark.parametrize("form", ("step", "rows"))
@pytest.mark.parametrize("sot", (2, 0))
def test_state_update(engines, V, form, sot):
    """one launch over rows in every state: inside the prompt (fed the next prompt token; the no-speech probability is captured at
    sot_index = 2 on the forced row too; with sot_index = 0 that row leaves through the kernel's early exit), free, at its own budget, at the call's budget, already finished, choosing EOT"""
    e = engines(V)
    c = S.make_ctx(V, "state", S.released_tb(V), True)
    H = S.histories(c)
    t = c.text_tok()
    long_hist = [t] * (S.MAX_NEW - 1)
    rows, hists = [], [H["text"], H["text"], [t, t, t], long_hist, H["text"], H["text"], H["odd"], H["empty"]]
    for i, h in enumerate(hists):
        row = S.normal_row(V, 1000 + i)
        if i == 5:
            row[c.eot] = np.float32(S.allowed_max(row, h, c) + 12.0)     # the chosen EOT
        rows.append(S.Row(f"state{i}", S.separate(row, h, c), h))
    rs = S.RowSet("state", c, rows)
    n = len(rows)
    pos = 2
    prompt = np.full((n, 6), t, dtype=np.int32)
    prompt[0, :5] = [7, 8, 9, 10, 11]
    plen = [5, 3, 1, 2, 3, 1, 2, 3]
    caps = [1 << 30, 1 << 30, 4, 1 << 30, 1 << 30, 1 << 30, 1 << 30, 1 << 30]
    done0 = [0, 0, 0, 0, 1, 0, 0, 0]
    sum0 = [np.float32(v) for v in (0, -2.25, -1, -30.5, -7, 0, -0.5, 0)]
    refs = rs.ref()
    positions = [pos] if form == "step" else [pos] * n
    res = e.select_probe(form, rs.matrix(), make_opts(c, sot), rs.hist(), positions, prompt=prompt, prompt_len=plen, done=done0,
                         row_cap=caps, sum_logprob=sum0, n_done=3)
    exp = expect_rows(rs, refs, [r.choice for r in refs], [r.lp for r in refs], [pos] * n, sot, form == "rows", done0, caps, sum0, prompt, plen)
    assert exp[0].cur_tok == 10 and exp[0].n_sampled == 1 and exp[2].newly_done and exp[3].newly_done and exp[5].cur_tok == c.eot
    assert exp[4].cur_tok == c.eot and not exp[4].newly_done and exp[5].newly_done and not exp[1].newly_done
    check_state(form, rs, res, exp, refs, 3, positions, f"{V}/state/{form}/sot{sot}", sum0)


@pytest.mark.parametrize("V", S.VOCABS)
def test_unselectable_row_is_finished_with_eot(engines, V):
    """a row with nothing to select - every id masked by the rules, every logit NaN, every logit -inf - in the greedy, sampled,
    per-row and session forms: the token is EOT, the increment -inf, the row finished and counted; no id outside [0, V) comes
    back; the live row beside them is chosen as ever"""
    e = engines(V)
    rs = S.dead_rowset(V)
    c, n = rs.ctx, len(rs.rows)
    refs = rs.ref()
    assert [r.choice for r in refs][:2] == [-1, -1] and refs[2].choice >= 0 and refs[3].choice == -1
    for T, seed in ((0.0, 0), (1.0, S.SEEDS[0])):
        for form in ("step", "rows"):
            pos = [POS] if form == "step" else [POS] * n
            res = e.select_probe(form, rs.matrix(), make_opts(c, 0), rs.hist(), pos, temperature=T, seed=seed)
            for i in (0, 1, 3):
                k = len(rs.rows[i].hist)
                assert res["cur_tok"][i] == c.eot and res["last_tok"][i] == c.eot and res["out_tokens"][i, k] == c.eot, (form, T, i)
                assert res["done"][i] == 1 and res["n_sampled"][i] == k + 1 and res["sum_logprob"][i] == -np.inf, (form, T, i)
            assert res["n_done"][0] == 3 and res["done"][2] == 0 and 0 <= res["cur_tok"][2] < V
            assert np.isfinite(res["sum_logprob"][2])
            if T == 0.0:
                assert res["cur_tok"][2] == refs[2].choice
        se = e.select_probe("session", rs.matrix(), make_opts(c, 0), rs.hist(), entries=[[i, POS, i, 1] for i in range(n)],
                            entry_temp=[T] * n, entry_seed=[seed] * n)
        for i in (0, 1, 3):
            assert se["choice"][i] == c.eot and se["lp"][i] == -np.inf, (T, i)
        assert 0 <= se["choice"][2] < V and np.isfinite(se["lp"][2])


def test_report_ratios():
    """the largest error / bound per (form, quantity) of this run (recorded in profiles/select_kernels.jsonl and DESIGN.md 4.33)"""
    assert RATIOS, "runs after the other tests of this module"
    for (form, what), r in sorted(RATIOS.items()):
        print(f"select-kernel error / bound: {form:14s} {what:10s} {r:.3f}")
        assert r <= 1.0
