"""CPU: the references, the inputs and the tolerance of tests/test_gpu_self_attn_kernels.py, checked without a GPU.

  * the derived bound is not too tight: a plain np.float32 restatement of the kernels' arithmetic (per-slot online softmax in key
    order, the new key in slot 0, one merge by exp(m - M): self_attn_cases.f32_self_attention) stays inside 1 / 4 of the float32
    term on every input set the GPU tests use; the reference rounded to the engine type passes; every row's score span is <= 40,
    peaked rows hold >= 0.9 on their key, the sink row >= 0.6 on key 0;
  * the float64 reference agrees with the attention of oracle.whisper_ref's own decoder (the _attend of decoder_forward);
  * the inputs and the tolerance see the bugs they are there for: each named mutation of the reference is flagged by the GPU
    tests' own comparison (error_ratio / pool_mismatch) on at least one case of the GPU tests' own input sets;
  * the position list and the peaked keys cross the iteration and load-batch edges of both geometries, and the poison is where
    the GPU test says it is;
  * the header declares, and _lib.SYMBOLS lists, the hooks.
"""
import os
import re

import numpy as np
import pytest
import torch

import self_attn_cases as S
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.CASES_BY_NAME


# ---- the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,ct", S.ENGINES)
def test_float32_restatement_stays_inside_a_quarter_of_the_float32_term(H, ct):
    worst = 0.0
    for c in S.cases_of(ct):
        sc = S.scene(c, H, ct)
        ref = S.reference(sc)
        assert np.isfinite(ref["ref"]).all(), c.name              # the reference itself never reads poison
        assert ref["span"].max() <= 40, (c.name, ref["span"].max())
        peaked, sink = sc.tstar >= 0, np.zeros_like(sc.tstar, bool)
        sink[-1] = sc.tstar[-1] >= 0
        assert (ref["mass"][peaked & ~sink] >= 0.9).all() and (ref["mass0"][sink] >= 0.6).all(), c.name
        err = np.abs(S.restate(sc).astype(np.float64) - ref["ref"])
        assert (err <= ref["f32"] / 4).all(), (c.name, float((err / np.maximum(ref["f32"], 1e-300)).max()))
        worst = max(worst, float((err[ref["f32"] > 0] / ref["f32"][ref["f32"] > 0]).max()))
        ratio, where = S.error_ratio(S.rnd(ref["ref"].astype(np.float32), ct), ref)
        assert ratio <= 1, S.describe(sc, S.rnd(ref["ref"].astype(np.float32), ct), ref, where)
    print(f"H {H} {ct}: float32 restatement at most {worst:.4f} of the float32 term")


def test_reference_agrees_with_the_oracle_decoders_attention():
    sc = S.scene(CASES["rows-mix1"], 6, "bf16")
    rows = R.self_attn_ref(sc.q, sc.k, sc.v, S.launch_pool(sc), sc.pages, sc.pos)
    for r, (out, _, K, V) in enumerate(rows):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        got = R._attend(t(sc.q[r])[None, :, None, :], t(K)[None], t(V)[None]).numpy().reshape(6, 64)    # decoder_forward's call
        assert np.abs(got - out).max() <= 1e-12, r
    sc = S.scene(CASES["prefill-npos17"], 6, "f32")
    ref = S.reference(sc)["ref"]
    r0 = 0
    for n in sc.lens:                                             # the causal form: decoder_forward's mask over n new tokens
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[r0:r0 + n], dtype=np.float64)).permute(1, 0, 2)[None]
        mask = torch.triu(torch.full((n, n), R.NEG_INF, dtype=torch.float64), diagonal=1)
        got = R._attend(t(sc.q), t(sc.k), t(sc.v), mask).numpy().reshape(n, 6, 64)
        assert np.abs(got - ref[r0:r0 + n]).max() <= 1e-12
        r0 += n


# ---- mutations ------------------------------------------------------------------------------------------------------------------
def _attend(sc, edit=None, pages=None, pool=None, scale=1.0, den=1.0):
    """the reference with one thing wrong, rounded to the engine type: edit(K, V, row) -> (K, V) over the gathered keys"""
    pool = S.launch_pool(sc) if pool is None else pool
    q, k, v = (S.rnd(a * np.float32(scale), sc.ct) for a in (sc.q, sc.k, sc.v))
    rows = R.self_attn_ref(q, k, v, pool, sc.pages if pages is None else pages, sc.pos)
    out = np.empty((len(rows), sc.H, 64))
    for r, (o, _, K, V) in enumerate(rows):
        if edit is not None:
            K, V = edit(K, V, r)
            with np.errstate(invalid="ignore"):
                o, _ = R.cross_attn_ref(q[r], K, V)
        out[r] = o / den
    return S.rnd(out.astype(np.float32), sc.ct)


def _flagged(sc, out):
    return S.error_ratio(out, S.reference(sc))[0] > 1


def _drop(i):
    return lambda K, V, r: (np.delete(K, i, axis=1), np.delete(V, i, axis=1)) if K.shape[1] > i + 1 else (K, V)


def _v_shift(sc, d):
    def edit(K, V, r):
        p = int(sc.pos[r])
        if p == 0:
            return K, V
        _, Vp = R.self_history(S.launch_pool(sc), sc.pages[r], min(p + 1, S.N_CTX))
        V = V.copy()
        V[:, :p] = Vp[:, np.clip(np.arange(p) + d, 0, Vp.shape[1] - 1)]
        return K, V
    return edit


MUTATIONS = {
    "the new key left out": (("step-pos447", "step-pos1", "rows-mix0"), lambda sc: _attend(sc, lambda K, V, r: (K[:, :-1], V[:, :-1]) if K.shape[1] > 1 else (K, V))),
    "the last cached key dropped": (("step-pos447", "step-pos129", "rows-mix1"), lambda sc: _attend(sc, lambda K, V, r: _drop(K.shape[1] - 2)(K, V, r))),
    "key pos - 1 counted twice": (("step-pos447", "step-pos33", "rows-mix2"),
                                  lambda sc: _attend(sc, lambda K, V, r: (np.insert(K, -1, K[:, -2], axis=1), np.insert(V, -1, V[:, -2], axis=1)) if K.shape[1] > 1 else (K, V))),
    "V taken from slot (pos % 16) + 1": (("step-pos257", "rows-mix0"), lambda sc: _attend(sc, _v_shift(sc, 1))),
    "V taken from slot (pos % 16) - 1": (("step-pos257", "rows-mix0"), lambda sc: _attend(sc, _v_shift(sc, -1))),
    "K and V halves of a page swapped": (("step-pos65", "rows-mix2"),
                                         lambda sc: _attend(sc, lambda K, V, r: (np.concatenate([V[:, :-1], K[:, -1:]], 1), np.concatenate([K[:, :-1], V[:, -1:]], 1)))),
    "a row reading its neighbour's pages": (("step-pos129-row0-4", "step-pos447", "rows-mix1"), lambda sc: _attend(sc, pages=sc.pages[1:] + sc.pages[:1])),
    "the identity table used where a permuted one was set": (("step-pos257-permuted", "rows-mix0-permuted", "rows-row0-4-permuted"),
                                                             lambda sc: _attend(sc, pages=[tuple(S.identity_table()[sc.case.row0 + r]) for r in range(sc.case.n_rows)])),
    "the denominator counted LPR times": (("step-pos0", "step-pos447", "rows-mix0"), lambda sc: _attend(sc, den=S.LPR[sc.ct])),
    "one slab of four missing": (("step-pos128-slab4", "rows-mix1-slab4"), lambda sc: _attend(sc, scale=0.875)),
}


@pytest.mark.parametrize("ct", S.TYPES)
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_is_flagged(name, ct):
    names, mutate = MUTATIONS[name]
    hit = []
    for n in names:
        if ct not in CASES[n].types:
            continue
        sc = S.scene(CASES[n], 6, ct)
        assert not _flagged(sc, _attend(sc)), n                     # the harness itself: no mutation, no flag
        if _flagged(sc, mutate(sc)):
            hit.append(n)
    assert hit or all(ct not in CASES[n].types for n in names), (name, ct)
    assert len(hit) == sum(ct in CASES[n].types for n in names), (name, ct, hit)    # here: on every case listed


@pytest.mark.parametrize("ct", S.TYPES)
def test_first_key_of_the_second_load_batch_dropped_is_flagged(ct):
    b = S.batch(ct)
    assert b == {"f32": 64, "bf16": 128, "f16": 128}[ct]
    for n in ("step-pos447", "step-pos257", f"step-pos{b + 1}"):
        sc = S.scene(CASES[n], 6, ct)
        assert (sc.tstar == b).any() and (sc.tstar == b - 1).any(), n      # a row is peaked on either side of the edge
        assert _flagged(sc, _attend(sc, _drop(b))), (n, ct)


@pytest.mark.parametrize("ct", S.TYPES)
def test_stale_copy_on_write_page_is_flagged(ct):
    for n in ("step-beam", "rows-beam"):
        sc = S.scene(CASES[n], 6, ct)
        assert [len(p) // 2 for p in sc.copies] == [1, 5]
        for skip in ((0, 0), (1, 4)):                               # the only pair of the first list; the last pair of the second
            stale = {l: p.copy() for l, p in sc.pool.items()}
            for i, pairs in enumerate(sc.copies):
                keep = [x for j in range(0, len(pairs), 2) if (i, j // 2) != skip for x in pairs[j:j + 2]]
                for l in stale:
                    S.copy_pages(stale[l], keep)
            want = S.pool_after(sc, done=np.ones(S.MAX_BATCH, np.int32))
            assert all(S.pool_mismatch(stale[l], want[l]) for l in (0, 1)), (n, skip)           # seen in every layer's readback
            assert np.isfinite(_attend(sc, pool=stale[sc.case.layer])).all()                    # (stale values, not poison)
            assert _flagged(sc, _attend(sc, pool=stale[sc.case.layer])), (n, skip)              # and by the attention over it


@pytest.mark.parametrize("ct", S.TYPES)
def test_finished_row_appended_is_flagged(ct):
    for n in ("step-pos65-done", "rows-mix2-done", "rows-mix0-done-permuted"):
        sc = S.scene(CASES[n], 6, ct)
        flags = S.done_flags(sc.case.n_rows)
        assert flags.any() and not flags.all()
        bad = S.pool_mismatch(S.pool_after(sc)[sc.case.layer], S.pool_after(sc, done=flags)[sc.case.layer])
        assert bad, n


@pytest.mark.parametrize("ct", S.TYPES)
def test_causal_mask_off_by_one_is_flagged(ct):
    for n in ("prefill-npos2", "prefill-npos17", "prefill-npos129", "packed"):
        sc = S.scene(CASES[n], 6, ct)
        ref = S.reference(sc)
        for d in (1, -1):
            out, r0 = np.empty_like(ref["ref"]), 0
            for ln in sc.lens:
                K, V = (a[r0:r0 + ln].astype(np.float64).transpose(1, 0, 2) for a in (sc.k, sc.v))
                for t in range(ln):
                    e = min(max(t + 1 + d, 1), ln)
                    out[r0 + t] = R.cross_attn_ref(sc.q[r0 + t], K[:, :e], V[:, :e])[0]
                r0 += ln
            assert S.error_ratio(S.rnd(out.astype(np.float32), ct), ref)[0] > 1, (n, d)


# ---- coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", S.TYPES)
def test_positions_and_peaks_cross_the_edges_of_the_geometry(ct):
    it, b = S.slots(ct), S.batch(ct)
    assert (it, b) == ((16, 64) if ct == "f32" else (32, 128))
    step = {c.pos[0]: c for c in S.cases_of(ct) if c.form == "step" and c.table == "identity" and not c.n_slab and c.n_rows == S.MAX_BATCH and not c.done}
    assert set(step) == set(S.POSITIONS)
    for edge in (it, b, 16):
        assert {edge - 1, edge, edge + 1} <= set(step), edge
    rows_pos = {p for c in S.cases_of(ct) if c.form == "rows" for p in c.pos}
    assert set(S.POSITIONS) <= rows_pos
    assert any(abs(c.pos.index(0) - c.pos.index(447)) == 1 for c in S.cases_of(ct) if c.form == "rows" and 0 in c.pos and 447 in c.pos)
    peaks = set()
    for p in (257, 447):
        peaks |= set(S.scene(step[p], 6, ct).tstar.reshape(-1).tolist())
    assert {0, it - 1, it, b - 1, b, 2 * b - 1, 2 * b, 255, 256, 446, 447} <= peaks, sorted(peaks)
    sc = S.scene(step[447], 6, ct)
    assert 446 in sc.tstar and 447 in sc.tstar and 0 in sc.tstar      # last cached, new, first


@pytest.mark.parametrize("ct", S.TYPES)
def test_poison_is_everything_outside_the_logical_history(ct):
    for c in S.cases_of(ct):
        sc = S.scene(c, 6, ct)
        pool = sc.pool[c.layer]
        assert np.isnan(sc.pool[1 - c.layer]).all() or c.table == "beam", c.name
        owned = np.zeros((S.N_PAGES, 16), bool)
        if c.form in ("step", "rows") and c.table != "beam":
            for r, p in enumerate(sc.pos):
                t = np.arange(int(p))
                owned[np.asarray(sc.pages[r])[t // 16], t % 16] = True
        elif c.table == "beam":
            pool = S.launch_pool(sc)
            for r in range(c.n_rows):
                t = np.arange(S.BEAM_POS)
                owned[np.asarray(sc.pages[r])[t // 16], t % 16] = True
        fin = np.isfinite(pool)
        assert (fin == owned[:, None, None, :, None]).all(), c.name   # finite exactly on positions < pos of the rows' own pages
        assert same_nan_bits(pool)


def same_nan_bits(pool):
    return set(np.unique(pool.view(np.uint32)[np.isnan(pool)]).tolist()) <= {S.POISON["f32"]}


def test_packed_page_lists_are_not_contiguous_and_fit_the_lengths():
    assert [len(p) for p in S.PACKED_PAGES] == [-(-n // 16) for n in S.PACKED_LENS]
    flat = [p for pl in S.PACKED_PAGES for p in pl]
    assert len(set(flat)) == len(flat) and max(flat) < S.N_PAGES and min(flat) >= 0
    assert any(b - a != 1 for pl in S.PACKED_PAGES if len(pl) > 1 for a, b in zip(pl, pl[1:]))
    tab, pairs = S.beam_table()
    last = S.BEAM_POS // 16
    for grp in S.BEAM_GROUPS:
        assert all((tab[r, :last] == tab[grp[0], :last]).all() for r in grp)
        assert len({int(tab[r, last]) for r in grp}) == len(grp)


# ---- declarations ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_hooks():
    header = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    for fn in ("ttasr_self_kv_fill", "ttasr_self_kv_set", "ttasr_self_kv_get", "ttasr_self_attn_probe"):
        assert re.search(r"TTASR_API int %s\(" % fn, header), fn
        assert fn in _lib.SYMBOLS, fn
    assert "UNDEFINED until ttasr_decode_reset" in header
    from taiwan_tongues_asr_ce_amd.engine import Engine
    for i, form in enumerate(("STEP", "ROWS", "PREFILL", "PACKED", "COPY")):
        assert re.search(r"#define TTASR_SELF_%s %d\b" % (form, i), header) and Engine.SELF_FORMS[form.lower()] == i
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ttasr_self_attn_probe" in design and "self_attn_cases.py" in design
