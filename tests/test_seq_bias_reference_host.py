"""Host: the numpy restatement of the sequence-bias processor (tests/seq_bias_cases.py reference) against HF Transformers'
SequenceBiasLogitsProcessor - always against the committed fixture tests/golden/seq_bias_hf.npz (tools/make_golden_seq_bias.py),
bit for bit, and against the live processor where transformers imports - and the proof that the case list sees the defects it
is there for: a restatement with one of them must differ from the fixture on the case built for it."""
import json
import os

import numpy as np
import pytest

import seq_bias_cases as S

V = S.GOLDEN_VOCAB


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "seq_bias_hf.npz"))
    return z, json.loads(str(z["cases"]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_holds_the_case_list(golden):
    z, record = golden
    cases = S.cases(V)
    assert [c.name for c in cases] == [r["name"] for r in record]
    for i, (c, r) in enumerate(zip(cases, record)):
        assert [[list(ids), b] for ids, b in c.table] == r["table"], c.name
        assert c.histories() == r["histories"], c.name
        assert np.array_equal(bits(c.logits(V)), bits(z[f"raw_{i}"])), c.name
    assert str(z["transformers"])


def test_restatement_equals_hf_fixture_bit_for_bit(golden):
    z, _ = golden
    for i, c in enumerate(S.cases(V)):
        got = S.reference(z[f"raw_{i}"], c.histories(), c.table)
        assert np.array_equal(bits(got), bits(z[f"out_{i}"])), c.name


def test_restatement_equals_live_hf():
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    for c in S.cases(V):
        raw = c.logits(V)
        proc = tf.SequenceBiasLogitsProcessor({tuple(ids): float(b) for ids, b in c.table})
        want = raw.copy()
        for r, h in enumerate(c.histories()):
            if h is not None:
                want[r] = proc(torch.tensor([h], dtype=torch.long).reshape(1, len(h)), torch.from_numpy(raw[r:r + 1].copy())).numpy()[0]
        assert np.array_equal(bits(S.reference(raw, c.histories(), c.table)), bits(want)), c.name


def _differs(golden, name, **mutation):
    z, _ = golden
    cases = S.cases(V)
    i = [c.name for c in cases].index(name)
    c = cases[i]
    histories = mutation.pop("histories", None) or c.histories()
    return not np.array_equal(bits(S.reference(z[f"raw_{i}"], histories, c.table, **mutation)), bits(z[f"out_{i}"]))


def test_cases_catch_a_wrong_summation_order(golden):
    """sequences that end in one token, all matching, summed backwards"""
    assert _differs(golden, "sum_two", order="reversed")
    assert _differs(golden, "sum_three", order="reversed")


def test_cases_catch_a_match_against_the_wrong_end(golden):
    assert _differs(golden, "wrong_end", end="head")


def test_cases_catch_an_ignored_prompt_boundary(golden):
    """a history that starts at the first sampled token, the prompt forgotten"""
    c = next(c for c in S.cases(V) if c.name == "straddle")
    sampled_only = [list(r.sampled) if c.chooses(r) else None for r in c.rows]
    assert _differs(golden, "straddle", histories=sampled_only)


def test_cases_catch_a_prefix_length_history_rule(golden):
    """HF skips a sequence LONGER than the history: L tokens need L history tokens, not L - 1 (DESIGN.md section 4.34 states HF's)"""
    assert _differs(golden, "history_shorter", min_hist="prefix")
    assert _differs(golden, "sixteen", min_hist="prefix")


def test_same_allows_only_the_signed_zero():
    raw = np.asarray([[-0.0, 1.0, -0.0]], dtype=np.float32)
    S.same(np.asarray([[-0.0, 1.0, 0.0]], np.float32), np.asarray([[0.0, 1.0, 0.0]], np.float32), raw)
    with pytest.raises(AssertionError):
        S.same(np.asarray([[-0.0, np.nextafter(np.float32(1), np.float32(2)), 0.0]], np.float32), np.asarray([[0.0, 1.0, 0.0]], np.float32), raw)
    with pytest.raises(AssertionError):
        S.same(np.asarray([[1.0, 1.0, 0.0]], np.float32), np.asarray([[0.0, 1.0, 0.0]], np.float32), raw)


def test_window_and_state_forms_carry_the_same_history():
    """what the two probe forms upload reads back as the case's histories, poison everywhere else"""
    for c in S.cases(V):
        hist, ln = S.window_form(c)
        st = S.state_form(c)
        for r, h in enumerate(c.histories()):
            if h is None:
                assert ln[r] == -1
                continue
            w = min(len(h), S.W)
            assert list(hist[r, S.W - w:]) == h[len(h) - w:] and (hist[r, :S.W - w] == S.POISON).all() and ln[r] == min(len(h), S.MAX_LEN)
            full = list(st["prompt"][r, :st["prompt_len"][r]]) + list(st["out_tokens"][r, :st["n_sampled"][r]])
            assert full == h, c.name
