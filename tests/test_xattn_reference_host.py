"""CPU: the references and the tolerance of tests/test_gpu_xattn_kernels.py, checked without a GPU.

  * oracle.whisper_ref.e4m3_encode / e4m3_decode (torch.float8_e4m3fn) against an independent brute-force nearest-code search
    over the 256-entry decode table, ties to the even code: every midpoint between adjacent finite codes, +-0, the subnormal
    range, 448;
  * the derived bound is not too tight: a plain np.float32 restatement of the kernels' arithmetic stays inside 1 / 4 of the
    float32 term on every input set the GPU tests use;
  * the inputs and the tolerance see the bugs they are there for: each named mutation of the reference is flagged by the GPU
    tests' own comparison on at least one case of the GPU tests' own input sets;
  * the header declares, and the library exports, the two known-answer hooks.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import xattn_cases as X
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_WINDOWS = X.WINDOWS + (X.FULL_WINDOW,)


# ---- e4m3 ---------------------------------------------------------------------------------------------------------------------
def _brute_force_encode(x):
    """nearest finite e4m3fn code of each float64 x by exhaustive search; exact ties go to the code with an even mantissa bit."""
    table = X.E4M3_TABLE
    finite = np.array([c for c in range(256) if not np.isnan(table[c])])
    out = np.empty(len(x), np.uint8)
    for i, v in enumerate(np.asarray(x, np.float64)):
        neg = np.signbit(v)
        cand = finite[(finite >= 128) == neg]                  # codes of the value's sign (-0.0 keeps its sign bit)
        dist = np.abs(table[cand] - v)
        best = cand[dist == dist.min()]
        assert 1 <= len(best) <= 2
        out[i] = best[0] if len(best) == 1 else best[best % 2 == 0][0]
    return out


def test_e4m3_reference_against_brute_force_nearest_code_search():
    t = X.E4M3_TABLE
    assert np.isnan(t[0x7f]) and np.isnan(t[0xff]) and np.isfinite(np.delete(t, [0x7f, 0xff])).all()
    assert t[0x7e] == 448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0] == 0 and np.signbit(t[0x80])
    # decode(encode(code value)) is the identity on every finite code
    finite = np.array([c for c in range(256) if c not in (0x7f, 0xff)], np.uint8)
    assert np.array_equal(R.e4m3_encode(t[finite].astype(np.float32)), finite)
    mids = X.E4M3_MIDPOINTS
    assert len(mids) == 126 and 17.0 in mids and 19.0 in mids and 2.0 ** -10 in mids
    g = np.random.Generator(np.random.Philox(key=5))
    eps = 2.0 ** -20
    probe = np.concatenate([
        mids, -mids, mids * (1 + eps), mids * (1 - eps), -mids * (1 + eps), -mids * (1 - eps),   # ties and both sides of them
        [0.0, -0.0, 448.0, -448.0, 447.9, 2.0 ** -9, 2.0 ** -10, 2.0 ** -11, -2.0 ** -10, 3 * 2.0 ** -10, 7.5 * 2.0 ** -9],
        g.uniform(-2.0 ** -6, 2.0 ** -6, 2000),                  # the subnormal range
        g.uniform(-448, 448, 2000), g.standard_normal(2000)]).astype(np.float32)
    assert np.array_equal(probe.astype(np.float64)[:252], np.concatenate([mids, -mids]))   # the ties survive float32
    got, want = R.e4m3_encode(probe), _brute_force_encode(probe.astype(np.float64))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(float(probe[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert R.e4m3_encode(np.array([17, 19, -17, -19], np.float32)).tolist() == [0x58, 0x5a, 0xd8, 0xda]   # 16, 20: the even codes
    assert R.e4m3_encode(np.array([0.0, -0.0], np.float32)).tolist() == [0x00, 0x80]


def test_quantiser_reference_on_the_block_kinds():
    """xkv_quant_ref on the blocks the GPU test places: the zero block gives scale 1 and codes 0; the outlier block lands in
    subnormals and zeros; the ties block's scaled values ARE e4m3 ties (inv is an exact power of two)."""
    for ct in X.TYPES:
        for T in (4, 30, 150):
            kinds = {k: X.quant_block(k, T, ct, seed=T + 3) for k in X.QUANT_KINDS}
            codes, sc = R.xkv_quant_ref(kinds["zero"])
            assert sc == 1.0 and not codes.any()
            codes, sc = R.xkv_quant_ref(kinds["outlier"])
            assert sc == np.float32(1000.0) * (np.float32(1) / np.float32(448))
            small = (codes & 0x7f) < 8                           # zero or subnormal
            assert small.sum() == codes.size - 1 and ((codes & 0x7f) == 0).any() and (((codes & 0x7f) > 0) & small).any()
            codes, sc = R.xkv_quant_ref(kinds["constant"])
            assert len(np.unique(codes)) == 1 and (codes.flat[0] & 0x7f) == 0x7e
            codes, sc = R.xkv_quant_ref(kinds["ties"])
            assert sc == np.float32(2.0 ** X.TIES_K)
            scaled = np.abs(kinds["ties"].astype(np.float64) / float(sc)).reshape(-1)
            on_tie = np.isin(scaled, X.E4M3_MIDPOINTS)
            assert on_tie.sum() >= scaled.size - 1 and set(X.E4M3_MIDPOINTS) <= set(scaled[on_tie]) or T == 4
            assert (R.e4m3_decode(codes).reshape(-1)[on_tie] != scaled[on_tie]).all() and (codes[..., :][on_tie.reshape(codes.shape)] % 2 == 0).all()
            codes, sc = R.xkv_quant_ref(kinds["negative"])
            assert (codes >= 0x80).all()
    seen = {X.quant_kind(b, h, w) for w in ALL_WINDOWS for b in range(3) for h in range(16)}
    assert seen == set(X.QUANT_KINDS)


# ---- the case table ----------------------------------------------------------------------------------------------------------
def test_case_table_covers_what_the_issue_names():
    for H in X.HEADS:
        names = [c.name for c in X.cases(H)]
        assert len(set(names)) == len(names)
    c20 = X.cases(20)
    assert {c.kv_div for c in c20 if c.form == "mq_fp8"} == {2, 3, 4, 5, 6, 7}
    assert {c.kv_div for c in c20 if c.form == "mq"} >= {2, 3, 4, 5, 6, 7, 8}
    assert {c.opt("xattn_mq_slices", 0) for c in c20 if c.form == "mq_fp8"} >= {0, 1, 3, 8}
    assert {c.n_slab for c in c20 if c.form == "fp8"} == {0, 1, 4} == {c.n_slab for c in c20 if c.form == "mq_fp8"}
    assert any(c.n_rows * c.H == 256 and c.form == "fp8" for c in X.cases(16))
    assert any(c.n_rows * c.H == 240 and c.fp8_mode and not c.reads_fp8 for c in c20)
    # slice shapes of the shared-clip e4m3 kernel at the full window: 13 x 2 one slice, 6 x 5 four, 2 x 7 eight
    by = {c.name: c for c in c20}
    for name, s in (("mqfp8-13x2", 1), ("mqfp8-6x5", 4), ("mqfp8-2x7", 8), ("mqfp8-6x5-slices3", 3)):
        assert X.expected_kernel(by[name], X.FULL_WINDOW, "bf16")[1] == s, name
    # the pipelined kernel: items on both sides of xattn_deep_items = 512, and the switch off
    pipe = [c for c in c20 if c.form == "pipe" and not c.done]
    assert {c.n_rows * 20 <= c.opt("xattn_deep_items", 512) for c in pipe} == {True, False}
    assert {c.opt("xattn_deep_items", 512) for c in pipe} == {0, 512} and {c.opt("xattn_nontemporal", 1) for c in pipe} == {0, 1}
    for H in X.HEADS:
        forms = {c.form for c in X.cases(H, X.FULL_WINDOW)}
        assert forms == ({c.form for c in X.cases(H)} if H == 20 else {"fp8"}), forms   # the full window: once per form
        assert all(c.n_rows <= X.MAX_BATCH and c.n_rows % c.kv_div == 0 for c in X.cases(H))
    for w in ALL_WINDOWS:
        f = X.peak_frames(w)
        assert f[0] == 0 and f[-1] == w - 1 and all(m - 1 in f and m in f for m in range(16, w, 16))


def _distinct(H, w):
    """the cases of (H, w) with distinct operands"""
    seen = {}
    for c in X.cases(H, w):
        seen.setdefault((c.layer, c.n_rows, c.kv_div, c.reads_fp8), c)
    return list(seen.values())


@pytest.mark.parametrize("H", X.HEADS)
def test_inputs_respect_the_bound_s_assumptions_and_the_bound_is_not_too_tight(H):
    """Per input set: |s - max s| <= 40 and sum |q| |k| <= 64 (what delta assumes), peaked items hold >= 0.9 of the mass, every
    peak frame of the window is visited, and the plain float32 restatement errs by at most 1 / 4 of the bound's float32 term."""
    worst = 0.0
    for w in ALL_WINDOWS:
        visited = set()
        for c in _distinct(H, w):
            o = X.operands(c, w)
            assert np.array_equal(X.rnd(o.q, "bf16"), o.q) and np.array_equal(X.rnd(o.q, "f16"), o.q)
            ref = X.reference(o.q, o.K, o.V, c.kv_div, "bf16")
            peaked = o.tstar >= 0
            assert ref["span"].max() <= 40 and ref["sqk"].max() <= 64, (c.name, w)
            assert ref["mass"][peaked].min() >= 0.9, (c.name, w, ref["mass"][peaked].min())
            assert c.n_rows == 1 or w <= 6 or ref["mass"][~peaked].max() < 0.9, (c.name, w)
            visited.update(o.tstar[peaked].tolist())
            if c.reads_fp8:
                out = X.f32_attention(o.q, R.e4m3_decode(o.codes[0]), R.e4m3_decode(o.codes[1]), c.kv_div, *o.scales)
            else:
                out = X.f32_attention(o.q, o.K, o.V, c.kv_div)
            err = np.abs(out.astype(np.float64) - ref["ref"])
            ok = err <= ref["f32"] / 4
            assert ok.all(), (c.name, w, float((err / np.maximum(ref["f32"], 1e-300)).max()))
            worst = max(worst, float((err[ref["f32"] > 0] / ref["f32"][ref["f32"] > 0]).max()))
        if w != X.FULL_WINDOW:
            assert visited == set(X.peak_frames(w)), (w, sorted(set(X.peak_frames(w)) - visited))
        else:
            assert {0, w - 1} <= visited and len(visited) >= 100
    print("H", H, "largest float32-restatement error / float32 term:", worst)


# ---- the mutations -----------------------------------------------------------------------------------------------------------
def _truncating_encode(x):
    """e4m3 by truncation toward zero instead of round-to-nearest-even"""
    pos = np.sort(X.E4M3_TABLE[:127])
    idx = np.searchsorted(pos, np.abs(x.astype(np.float64)), side="right") - 1
    order = np.argsort(X.E4M3_TABLE[:127])
    return (order[idx] | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def _attend(q, K, V, kv_div, weight=None):
    out = np.empty(q.shape, np.float64)
    for rows, k, v in X.gather(q, K, V, kv_div):
        s = np.einsum("rhc,htc->rht", q[rows].astype(np.float64), k)
        p = np.exp(s - s.max(-1, keepdims=True))
        if weight is not None:
            p = p * weight
        out[rows] = np.einsum("rht,htc->rhc", p / p.sum(-1, keepdims=True), v)
    return out


def _fp8_case(name, H=20):
    return next(c for c in X.cases(H) if c.name == name)


def _flagged(mutate, case_names, windows=(30, 66, 150)):
    """does the GPU tests' comparison flag `mutate(case, window, operands)` on at least one of the cases?  Also: the unmutated
    reference passes it with ratio 0."""
    hit = []
    for name in case_names:
        c = _fp8_case(name)
        for w in windows:
            o = X.operands(c, w)
            ref = X.reference(o.q, o.K, o.V, c.kv_div, "bf16")
            assert X.error_ratio(ref["ref"], ref) == 0.0
            ratio = X.error_ratio(mutate(c, w, o), ref)
            hit.append((name, w, ratio))
    assert any(r > 1 for _, _, r in hit), hit
    return hit


def test_mutation_truncating_quantiser_is_flagged():
    """the quantiser comparison is exact equality of codes: truncation differs on every block kind with a value off the grid"""
    for ct in X.TYPES:
        for w in (4, 30):
            blocks = X.quant_blocks(ct, w, 2, 20)
            codes, sc = R.xkv_quant_ref(blocks)
            inv = (np.float32(1) / sc)[..., None, None]
            trunc = _truncating_encode(blocks * inv)
            differs = (trunc != codes).reshape(2, 20, -1).any(-1)
            kinds = np.array([[X.quant_kind(b, h, w) for h in range(20)] for b in range(2)])
            assert differs[np.isin(kinds, ("ties", "heavy", "negative", "heavy2", "outlier"))].all()
            assert not differs[np.isin(kinds, ("zero", "constant"))].any()


def test_mutation_scales_swapped_or_shifted_are_flagged():
    def swapped(c, w, o):
        return _attend(o.q, X.dequant(o.codes[0], o.scales[1]), X.dequant(o.codes[1], o.scales[0]), c.kv_div)

    def neighbour(c, w, o):
        return _attend(o.q, X.dequant(o.codes[0], np.roll(o.scales[0], -1, axis=1)), X.dequant(o.codes[1], np.roll(o.scales[1], -1, axis=1)), c.kv_div)

    def neighbour_k_only(c, w, o):
        return _attend(o.q, X.dequant(o.codes[0], np.roll(o.scales[0], -1, axis=1)), o.V, c.kv_div)
    for m in (swapped, neighbour, neighbour_k_only):
        for name in ("fp8-rows13-slab0", "mqfp8-6x5"):
            assert all(r > 1 for _, _, r in _flagged(m, [name])), m.__name__


def test_mutation_dropped_last_frame_and_double_counted_seam_are_flagged():
    def drop_last(c, w, o):
        return _attend(o.q, o.K[:, :, :-1], o.V[:, :, :-1], c.kv_div)

    def seam_twice(c, w, o):
        weight = np.ones(w)
        weight[X.slice_plan(2, w)[1] if w > 64 else 32 if w > 32 else 16] = 2.0     # the first frame of the second slice
        return _attend(o.q, o.K, o.V, c.kv_div, weight)
    names = ["fp8-rows13-slab0", "mqfp8-6x5", "pipe-rows13-deep512-nt1-slab0", "split-rows3-slab0", "mq-6x5"]
    for m in (drop_last, seam_twice):
        assert all(r > 1 for _, _, r in _flagged(m, names)), m.__name__


def test_mutation_reversed_bytes_and_one_code_off_are_flagged():
    def reversed_bytes(c, w, o):
        kc = o.codes[0].reshape(o.codes[0].shape[:-1] + (16, 4))[..., ::-1].reshape(o.codes[0].shape)
        return _attend(o.q, X.dequant(kc, o.scales[0]), o.V, c.kv_div)

    def reversed_bytes_v(c, w, o):
        vc = o.codes[1].reshape(o.codes[1].shape[:-1] + (16, 4))[..., ::-1].reshape(o.codes[1].shape)
        return _attend(o.q, o.K, X.dequant(vc, o.scales[1]), c.kv_div)

    def one_code_off(c, w, o):
        """ONE V code, one step up, at the peaked frame of row 0 / head 0, in the channel with the largest value there"""
        vc = o.codes[1].copy()
        t = int(o.tstar[0, 0])
        ch = int(np.argmax(vc[0, 0, t] & 0x7f))
        vc[0, 0, t, ch] = int(vc[0, 0, t, ch]) + (1 if (vc[0, 0, t, ch] & 0x7f) < 0x7e else -1)
        return _attend(o.q, o.K, X.dequant(vc, o.scales[1]), c.kv_div)
    for m in (reversed_bytes, reversed_bytes_v, one_code_off):
        assert all(r > 1 for _, _, r in _flagged(m, ["fp8-rows13-slab0", "mqfp8-6x5"])), m.__name__


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_two_hooks():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"\b(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for fn in ("ttasr_get_cross_kv_fp8", "ttasr_cross_attn_probe"):
        assert fn in declared and fn in exported and fn in _lib.SYMBOLS, fn
    assert exported == set(_lib.SYMBOLS) == declared
