"""Non-GPU: the inputs, bounds and case list of tests/test_gpu_enc_attn_kernels.py (tests/enc_attn_cases.py) do what they are there
for.

  1. The tolerance is not too tight: at every case's inputs a float64 emulation of the flash kernel's stated arithmetic - with the
     lazy reference maximum AND with the running maximum, both legal - stays under error / bound 1 in tier A and tier B, and a
     plain float32 restatement of enc_attn_simple_kernel stays under 1 in tier A.  The largest ratios are printed.
  2. The tolerance sees bugs: each of the listed mutations of the emulation exceeds 1 on at least one element of at least one case
     the GPU test runs.
  3. The case list obeys its caps, and the scenes hold the rows they promise (rising, offset, flat, peaked on the tile seams)."""
import numpy as np
import pytest

import enc_attn_cases as E

RATIOS = {}      # (what, type, tier) -> largest error / bound


def _note(what, ct, rs):
    for tier, r in rs.items():
        RATIOS[(what, ct, tier)] = max(RATIOS.get((what, ct, tier), 0.0), r)


def _geometries(form, arithmetic=None):
    seen = []
    for c in E.cases():
        g = (c.B, c.H, c.Tq, c.Tk)
        if c.form == form and (arithmetic is None or c.arithmetic == arithmetic) and g not in seen:
            seen.append(g)
    return seen


# ---- 3. the case list and the scenes ----------------------------------------------------------------------------------------------
def test_case_list_obeys_its_caps():
    cs = E.cases()
    assert len({c.name for c in cs}) == len(cs)
    for ct in E.TYPES:
        for var in E.VARIANTS[ct]:
            got = {(c.Tq, c.B, c.H) for c in cs if c.form == "self" and c.ct == ct and c.variant == var and c.Tq != E.FULL_T}
            assert got == {(T, B, H) for T in E.SELF_T for B, H in E.SELF_BH}, (ct, var)
        full = [c for c in cs if c.form == "self" and c.ct == ct and c.Tq == E.FULL_T]
        assert len(full) == 1 and full[0].B == 1
    assert {c.variant for c in cs if c.ct in E.TYPES16 and c.form == "self"} == {"qw2", "qw1", "plain"}
    assert {c.variant for c in cs if c.ct == "f32"} == {"plain", "default"}
    for ct in E.TYPES16:
        got = {(c.Tq, c.Tk, c.B) for c in cs if c.form == "cross" and c.ct == ct and (c.Tq, c.Tk) != E.CROSS_FULL}
        assert got == {(nq, Tk, B) for nq in E.CROSS_NQ for Tk in E.CROSS_TK for B in (1, 3)}
        assert len([c for c in cs if c.form == "cross" and c.ct == ct and (c.Tq, c.Tk) == E.CROSS_FULL]) == 1
    assert not [c for c in cs if c.form == "cross" and c.ct == "f32"]
    assert all(c.Tq <= 257 and c.Tk <= 257 for c in cs if c.Tq != E.FULL_T and (c.Tq, c.Tk) != E.CROSS_FULL)
    assert {(c.B * c.H) % 8 == 0 for c in cs if c.form == "self"} == {True, False}      # the XCD remap and the plain order
    assert {(c.B * c.H) % 8 == 0 for c in cs if c.form == "cross"} == {True, False}
    assert len({c.H for c in cs}) == len(E.HEADS) and max(c.B for c in cs) <= E.MAX_BATCH
    # both sides of the launcher's 32-row rule
    assert {c.Tq for c in cs if c.form == "cross" and c.arithmetic == "decode"} == {31}
    assert E.expected_signature(E.Case("cross", "bf16", "cross", 3, 3, 32, 20)) == "enc_attn_flash_kernel<unsigned short, true, 1> clips 3 rows 32"
    assert E.expected_signature(E.Case("self", "f16", "qw2", 2, 4, 257, 257)) == "enc_attn_flash_kernel<f16_t, false, 2> grid 4096"
    assert E.expected_signature(E.Case("self", "bf16", "qw1", 2, 4, 257, 257)) == "enc_attn_flash_kernel<unsigned short, false, 1> grid 6144"
    assert E.expected_signature(E.Case("self", "f32", "default", 1, 5, 20, 20)) == "enc_attn_simple_kernel<float> grid 2560"


@pytest.mark.parametrize("T", (20, 65, 150, 257))
def test_scene_holds_the_rows_it_promises(T):
    B, H = 2, 4
    sc = E.scene(B, H, T, T)
    kinds = [E.ROW_KINDS[i] for i in np.unique(sc.kind)]
    assert set(kinds) == set(E.ROW_KINDS), kinds
    # K and V of a head, and K of neighbouring heads, differ by a factor 2 or 4
    for b in range(B):
        for h in range(H - 1):
            assert E.amp_k(b, h) != E.amp_v(b, h) and E.amp_k(b, h) != E.amp_k(b, h + 1) and E.amp_v(b, h) != E.amp_k(b, h + 1) and \
                E.amp_v(b, h) != E.amp_v(b, h + 1)
    S = sc.Q.astype(np.float64) @ sc.K.astype(np.float64).transpose(0, 1, 3, 2)
    p = np.exp(S - S.max(-1, keepdims=True)); w = p / p.sum(-1, keepdims=True)
    peaked = sc.tstar >= 0
    assert (np.take_along_axis(w, np.maximum(sc.tstar, 0)[..., None], -1)[..., 0][peaked] >= 0.93).all()
    want = set(E.peak_frames(T))
    assert {0, T - 1, T - 2} <= want and all(f in want for m in range(64, T, 64) for f in (m - 1, m))
    assert set(sc.tstar[peaked].tolist()) == want, sorted(want - set(sc.tstar[peaked].tolist()))
    tm = E.tile_maxima(sc)
    rising = sc.kind == E.ROW_KINDS.index("rising")
    if tm.shape[-1] > 1:       # the tile maximum climbs by more than the lazy threshold at EVERY tile, the last one included
        assert (np.diff(tm[rising], axis=-1) > E.FA_THR).all()
    offset = sc.kind == E.ROW_KINDS.index("offset")
    assert (tm[offset].max(-1) < -150).all() and (tm[offset].min(-1) > -230).all()     # about -200 exp2 units, below -128
    flat = sc.kind == E.ROW_KINDS.index("flat")
    assert np.ptp(S[flat], axis=-1).max() == 0 and (S[flat] == 2).all()
    ref = E.references(sc, "bf16", "flash")["A"]["ref"]
    assert np.allclose(ref[flat], np.broadcast_to(sc.V.astype(np.float64).mean(2)[:, :, None], ref.shape)[flat], rtol=0, atol=1e-15)


# ---- 1. not too tight -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("self", "cross"))
@pytest.mark.parametrize("ct", E.TYPES16)
def test_flash_emulations_stay_inside_both_tiers(ct, form):
    worst = {}
    for g in _geometries(form, "flash"):
        sc = E.scene(g[0], g[1], g[2], g[3])
        refs = E.references(sc, ct, "flash")
        for lazy in (True, False):
            out = E.emulate_flash(sc, ct, lazy=lazy)
            assert np.isfinite(out).all(), (g, lazy)
            rs = E.ratios(out, refs)
            _note(f"{form} flash {'lazy' if lazy else 'running'}", ct, rs)
            for tier, r in rs.items():
                assert r <= 1.0, (g, ct, lazy, tier, r, E.worst_element(out, refs[tier]))
                key = ("full window" if g[3] == E.FULL_T else "T <= 257", tier)
                worst[key] = max(worst.get(key, 0.0), r)
    print(ct, form, {k: round(v, 3) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("ct", E.TYPES)
def test_plain_restatement_stays_inside_tier_a(ct):
    geoms = _geometries("self", "plain") if ct == "f32" else [g for g in _geometries("self", "plain") if g[2] != E.FULL_T]
    geoms = [g for g in geoms if any(c.ct == ct and (c.B, c.H, c.Tq, c.Tk) == g and c.arithmetic == "plain" for c in E.cases())]
    assert geoms
    for g in geoms:
        sc = E.scene(*g)
        refs = E.references(sc, ct, "plain")
        assert set(refs) == {"A"}
        out = E.emulate_plain(sc, ct)
        rs = E.ratios(out, refs)
        _note("self plain", ct, rs)
        assert rs["A"] <= 1.0, (g, ct, rs, E.worst_element(out, refs["A"]))
    if ct != "f32":            # the cross form below 32 rows per clip: the decode step's float32 kernels
        for g in _geometries("cross", "decode"):
            sc = E.scene(*g)
            refs = E.references(sc, ct, "decode")
            out = E.emulate_plain(sc, ct)
            rs = E.ratios(out, refs)
            _note("cross decode", ct, rs)
            assert rs["A"] <= 1.0, (g, ct, rs)


# ---- 2. sees bugs ---------------------------------------------------------------------------------------------------------------
MUT_GEOMS = ((2, 4, 20, 20), (3, 3, 65, 65), (1, 5, 129, 129), (2, 4, 150, 150), (1, 8, 257, 257), (3, 3, 33, 150))


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_every_mutation_is_flagged(mut):
    run_by_gpu = {(c.B, c.H, c.Tq, c.Tk) for c in E.cases() if c.arithmetic == "flash"}
    caught = []
    for g in MUT_GEOMS:
        assert g in run_by_gpu, g
        sc = E.scene(*g)
        for ct in E.TYPES16:
            refs = E.references(sc, ct, "flash")
            for lazy in (True, False):
                if not lazy and mut in ("move_o_not_l", "move_twice", "first_tile_rescale"):
                    continue           # bugs of the lazy form as the kernel has it
                rs = E.ratios(E.emulate_flash(sc, ct, lazy=lazy, mut=mut), refs)
                if rs["B"] > 1.0:
                    caught.append((g, ct, lazy, round(min(rs["A"], 1e9), 2), round(min(rs["B"], 1e9), 2)))
    print(mut, "flagged in", len(caught), "runs; first:", caught[:3])
    assert caught, mut
    assert any(a > 1.0 for *_, a, _b in caught), (mut, "tier A never flags it")


def test_one_dropped_key_of_a_diffuse_row_is_far_outside_tier_b():
    """the sensitivity the end-to-end thresholds (0.05 on the encoder output) do not have"""
    sc = E.scene(2, 4, 150, 150)
    for ct in E.TYPES16:
        refs = E.references(sc, ct, "flash")
        out = E.emulate_flash(sc, ct, mut="drop_key")
        err = np.abs(out.astype(np.float64) - refs["B"]["ref"])
        diffuse = sc.kind == E.ROW_KINDS.index("diffuse")
        r = (err / refs["B"]["bound"])[diffuse].max()
        print(ct, "one key of 150 dropped, diffuse rows: error / bound", round(float(r), 1), "largest error", float(err[diffuse].max()))
        assert r > 4 and err[diffuse].max() < 0.05


def test_zz_report_largest_ratios():
    for (what, ct, tier), r in sorted(RATIOS.items()):
        print(f"largest error / bound  {what:22s} {ct:5s} tier {tier}  {r:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
