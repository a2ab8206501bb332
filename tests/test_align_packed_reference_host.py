"""CPU: the float64 reference and the derived bound of tests/align_packed_cases.py accept the kernels' arithmetic restated in
float32 and reject the bugs they are there for - a key past n_ctx leaking into a map, a row normalised with a stale reference,
item rows 128 / 129 swapped, a map of the wrong head - and the new C-ABI entries are declared, bound and documented."""
import os
import re

import numpy as np
import pytest

import align_packed_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (33, 224)             # an item of 33 rows, and a sequence of two items (128 + 96 rows)
SLOTS = X.seq_slots(len(LENS))
H = 6
ALL = list(range(H))


def _scene(ct, T, extra=0):
    K, V = X.synthetic_cache(ct, T + extra)
    q = X.make_q(K[:, :, :T], LENS, SLOTS, X.rounder(ct))
    return q, K, V


@pytest.mark.parametrize("ct", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("T", [20, 150])
def test_float32_arithmetic_is_inside_the_bound(ct, T):
    """The plain float32 evaluation is accepted at every engine type's bound (the f32 bound is the tightest), with room: the bound
    is not at the edge of what correct arithmetic gives."""
    q, K, V = _scene(ct, T)
    ref = X.reference(q, K, V, LENS, SLOTS, ct)
    out, maps = X.f32_attention(q, K, V, LENS, SLOTS)
    r_out, r_map = X.check(X.rounder(ct)(out), maps, ALL, ref)
    print(f"{ct} T={T}: float32 arithmetic at {r_out:.3f} (output) and {r_map:.3f} (maps) of the bound")
    assert r_out <= 1.0 and r_map <= 1.0
    np.testing.assert_allclose(ref["maps"].sum(-1), 1.0, atol=1e-12)


@pytest.mark.parametrize("ct", ["f32", "bf16", "f16"])
def test_reference_rejects_a_leaked_key(ct):
    """n_ctx = 20: the last (only) 64-key tile loads clamped keys; one of them (here: frame 20 of a longer cache) counted in the
    softmax sum changes every map row's normalisation."""
    q, K, V = _scene(ct, 20, extra=1)
    K[:, :, 20] = K[:, :, 19]                    # what a clamped load delivers: the last real key again
    ref = X.reference(q, K[:, :, :20], V[:, :, :20], LENS, SLOTS, ct)
    out, maps = X.f32_attention(q, K, V, LENS, SLOTS, n_ctx=20)
    assert X.check(out, maps, ALL, ref)[1] > 1.0
    good = X.f32_attention(q, K[:, :, :20], V[:, :, :20], LENS, SLOTS)
    assert X.check(X.rounder(ct)(good[0]), good[1], ALL, ref)[1] <= 1.0


@pytest.mark.parametrize("ct", ["f32", "bf16", "f16"])
def test_reference_rejects_a_stale_reference(ct):
    q, K, V = _scene(ct, 150)
    ref = X.reference(q, K, V, LENS, SLOTS, ct)
    out, maps = X.f32_attention(q, K, V, LENS, SLOTS, stale=True)
    assert X.check(out, maps, ALL, ref)[1] > 1.0


@pytest.mark.parametrize("ct", ["f32", "bf16", "f16"])
def test_reference_rejects_swapped_item_rows_and_a_wrong_head(ct):
    q, K, V = _scene(ct, 150)
    ref = X.reference(q, K, V, LENS, SLOTS, ct)
    out, maps = X.f32_attention(q, K, V, LENS, SLOTS)
    out = X.rounder(ct)(out)
    assert max(X.check(out, maps, ALL, ref)) <= 1.0
    a, b = LENS[0] + 128, LENS[0] + 129          # the last row of the second sequence's first item and the first row of its second
    sw_maps, sw_out = maps.copy(), out.copy()
    sw_maps[:, [a, b]] = sw_maps[:, [b, a]]
    sw_out[[a, b]] = sw_out[[b, a]]
    assert X.check(out, sw_maps, ALL, ref)[1] > 1.0 and X.check(sw_out, maps, ALL, ref)[0] > 1.0
    wrong = [1, 0, 2, 3, 4, 5]                   # heads 0 and 1 write each other's map
    assert X.check(out, maps, wrong, ref)[1] > 1.0
    one = [-1, -1, -1, 0, -1, -1]                # one selected head: its map is map 0
    assert X.check(out, maps[3:4], one, ref)[1] <= 1.0 and X.check(out, maps[2:3], one, ref)[1] > 1.0


def test_new_entries_are_declared_bound_and_documented():
    from taiwan_tongues_asr_ce_amd import _lib
    header = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    assert re.search(r"TTASR_API int ttasr_align_attn_probe\(", header) and "ttasr_align_attn_probe" in _lib.SYMBOLS
    assert '"align_packed" [0]' in header
    declared = set(re.findall(r"TTASR_API\s+[\w\s\*]+?\b(ttasr_\w+)\s*\(", header))
    assert declared == set(_lib.SYMBOLS)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "align_packed" in design and "ttasr_align_attn_probe" in design
