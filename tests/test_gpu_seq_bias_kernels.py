"""GPU: the sequence-bias kernel (kernels_bias.hip seq_bias_kernel<STATE>) one launch at a time through the known-answer hook
ttasr_seq_bias_probe, against the numpy restatement of HF's SequenceBiasLogitsProcessor (tests/seq_bias_cases.py, pinned to HF by
tests/test_seq_bias_reference_host.py).  The kernel does the same float32 additions in the same order: equality is bit for bit,
with the one exception seq_bias_cases.same documents (an unbiased raw -0.0).  Both history forms, the released vocabularies
(51865 is the tiny preset's), every cap exactly full, poison behind every history's valid length.  Engines: f32, 1 + 1 layers,
no weights (the hook needs none)."""
import ctypes as C

import numpy as np
import pytest

import seq_bias_cases as S
from taiwan_tongues_asr_ce_amd import seq_bias
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def wanted():
    """the reference of every (vocabulary, case), computed once"""
    memo = {}

    def get(V, case):
        key = (V, case.name)
        if key not in memo:
            raw = case.logits(V)
            memo[key] = (raw, S.reference(raw, case.histories(), case.table))
            for a in memo[key]:
                a.flags.writeable = False
        return memo[key]
    return get


def probe(eng, form, case, raw):
    if form == "window":
        hist, ln = S.window_form(case)
        return eng.seq_bias_probe("window", raw, hist=hist, hist_len=ln)
    st = S.state_form(case)
    return eng.seq_bias_probe("state", raw, **st)


def test_tiny_preset_vocabulary_is_covered():
    assert PRESETS["tiny"].vocab in S.GPU_VOCABS


@pytest.mark.parametrize("form", ["window", "state"])
@pytest.mark.parametrize("V", S.GPU_VOCABS)
def test_kernel_equals_reference_bit_for_bit(engines, wanted, V, form):
    eng = engines(V)
    seen = set()
    for case in S.cases(V):
        raw, want = wanted(V, case)
        eng.set_sequence_bias(case.table)
        got, sig = probe(eng, form, case, raw)
        assert sig == f"seq_bias_kernel<{'true' if form == 'state' else 'false'}> grid {len(case.rows) * 256}", sig
        S.same(got, want, raw, (V, form, case.name))
        if case.name == "no_match":
            assert np.array_equal(got.view(np.uint32), raw.view(np.uint32))   # output identical to input
        if case.name == "special_values":
            assert np.isneginf(got[:, 5]).all() and np.isneginf(got[:, 17]).all() and np.isposinf(got[:, 40]).all()
        if case.name == "row_state":
            alone = [r for r, h in enumerate(case.histories()) if h is None]
            assert alone == [1, 2] and np.array_equal(got[alone].view(np.uint32), raw[alone].view(np.uint32))
            assert not np.array_equal(got[0], raw[0]) and not np.array_equal(got[3], raw[3])
        seen.add(case.name)
    eng.set_sequence_bias(None)
    assert {"caps_full", "caps_one_group", "sixteen", "straddle", "history_shorter", "sum_two", "sum_three", "edge_ids"} <= seen


def test_caps_full_really_fills_the_caps():
    for name, groups, entries in (("caps_full", S.MAX_GROUPS, S.MAX_ENTRIES), ("caps_one_group", S.MAX_GROUPS, S.MAX_ENTRIES)):
        case = next(c for c in S.cases(51865) if c.name == name)
        t = seq_bias.group_table(seq_bias.check_table(case.table, 51865))
        assert (len(t["groups"]), len(t["entries"])) == (groups, entries)


def test_state_form_without_a_prompt_reads_sampled_tokens_only(engines):
    eng = engines(51865)
    table = [((5, 9), 2.0), ((9,), 1.0)]
    eng.set_sequence_bias(table)
    raw = np.zeros((2, 51865), np.float32)
    out = np.full((2, S.MAX_NEW), S.POISON, np.int32)
    out[0, :2] = (3, 5)
    out[1, :1] = (5,)
    got, _ = eng.seq_bias_probe("state", raw, out_tokens=out, n_sampled=[2, 1], position=1)
    S.same(got, S.reference(raw, [[3, 5], [5]], table), raw)
    assert got[0, 9] == 3.0 and got[1, 9] == 1.0   # one history token is shorter than the two-token sequence
    eng.set_sequence_bias(None)


def _install_raw(eng, seqs):
    """ttasr_set_sequence_bias as the library sees it, past Engine.set_sequence_bias's own checks"""
    tokens = np.asarray([t for ids, _ in seqs for t in ids], np.int32)
    offsets = np.zeros(len(seqs) + 1, np.int32)
    np.cumsum([len(ids) for ids, _ in seqs], out=offsets[1:])
    bias = np.asarray([b for _, b in seqs], np.float32)
    i32p = C.POINTER(C.c_int32)
    rc = eng.lib.ttasr_set_sequence_bias(eng.h, len(seqs), tokens.ctypes.data_as(i32p), offsets.ctypes.data_as(i32p),
                                         bias.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, eng.lib.ttasr_last_error(eng.h).decode()


def test_library_refuses_what_breaks_a_cap_and_keeps_the_old_table(engines):
    V = 51865
    eng = engines(V)
    good = [((5, 9), 2.0)]
    eng.set_sequence_bias(good)
    raw = np.zeros((1, V), np.float32)
    hist = np.full((1, S.W), S.POISON, np.int32)
    hist[0, -2:] = (4, 5)
    for bad, word in (([(tuple(range(17)), 1.0)], "length"), ([((), 1.0)], "length"), ([((5,), float("nan"))], "finite"),
                      ([((5,), float("inf"))], "finite"), ([((V,), 1.0)], "vocabulary"), ([((-1, 2), 1.0)], "vocabulary"),
                      ([((5, 9), 1.0), ((5, 9), 2.0)], "repeats"),
                      ([((g,), 1.0) for g in range(S.MAX_GROUPS + 1)], "distinct last tokens"),
                      ([((1 + i % 4000, 1 + i // 4000, 7), 1.0) for i in range(S.MAX_ENTRIES + 1)], "at most")):
        rc, msg = _install_raw(eng, bad)
        assert rc != 0 and word in msg, (rc, msg)
        got, _ = eng.seq_bias_probe("window", raw, hist=hist, hist_len=[2])
        assert got[0, 9] == 2.0 and np.count_nonzero(got) == 1   # the table installed before is still the one in service
    eng.set_sequence_bias(None)
    with pytest.raises(Exception, match="no table"):
        eng.seq_bias_probe("window", raw, hist=hist, hist_len=[2])


def test_engine_refuses_before_the_library_is_called(engines):
    eng = engines(51865)
    for bad in ({(5,): float("nan")}, {tuple(range(17)): 1.0}, {(51865,): 1.0}, {(): 1.0}, {(1.5,): 1.0}, [((5,), 1.0), ((5,), 2.0)]):
        with pytest.raises(ValueError, match="sequence_bias"):
            eng.set_sequence_bias(bad)
