"""GPU: the encoder attention kernels against float64 references, through the known-answer hook ttasr_enc_attn_probe (DESIGN.md
section 4.36).  Inputs, case list, bounds and emulations live in tests/enc_attn_cases.py; tests/test_enc_attn_reference_host.py
shows on the CPU that the bounds pass every legal implementation of the stated arithmetic and flag the listed bugs.

  enc_attn_flash_kernel<T, false, 2 | 1>   self form, options flash_qw = 2 | 1, bf16 and fp16
  enc_attn_simple_kernel<T>                self form, option flash = 0 (bf16, fp16, f32) and the f32 engine's default
  enc_attn_flash_kernel<T, true, 1>        cross form from 32 rows per clip upward; 31 rows must take another kernel

Every case is ONE launch and asserts: the signature of what ran; the guard row behind the output intact and every element of the
NaN-filled output finite (every row is live); the output representable in the engine type; error / bound <= 1 per element in tier
A (softmax(q k) v in float64 on the given operands) and, for the flash kernel, tier B (float64 on the kernel's stated query
round_T(q log2 e)).  Identities of the kernel's per-query arithmetic, bit for bit: a batch item alone equals its rows in the
batch; flash_qw 1 equals flash_qw 2.

Engines: 1 encoder layer, 2 decoder layers, 8 / 4 / 3 / 5 heads, n_audio_ctx 1500, max_batch 3, created once per module.
Largest error / bound per (form, type): printed by the last test, recorded in DESIGN.md 4.36.

Measured on the MI355X (76 tests, 6.5 s), largest error / bound in tier A, tier B:
  self flash_qw 2 = 1    bf16 0.154, 0.496   fp16 0.150, 0.391
  self flash = 0         bf16 0.964          fp16 0.884          f32 0.009 (also with defaults)
  cross >= 32 rows       bf16 0.198, 0.570   fp16 0.299, 0.547
  cross 31 rows          bf16 0.975          fp16 0.918          (pipelined, shared-clip and frame-split kernels of the step)"""
import numpy as np
import pytest
import torch

import enc_attn_cases as E
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COMPUTE = {"bf16": COMPUTE_BF16, "f16": COMPUTE_F16, "f32": COMPUTE_F32}
RATIOS = {}     # (form / variant, type, tier) -> largest observed error / bound
REFS = {}       # (geometry, type, arithmetic) -> references, computed once


@pytest.fixture(scope="module")
def engines():
    from taiwan_tongues_asr_ce_amd.engine import Engine
    made = {}

    def get(H, ct):
        if (H, ct) not in made:
            e = Engine(E.dims(H), COMPUTE[ct], E.MAX_BATCH)
            e.load_weights(synth.state_dict(E.dims(H)).items())
            made[(H, ct)] = e
        return made[(H, ct)]
    yield get
    for e in made.values():
        e.close()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _refs(c):
    key = (c.B, c.H, c.Tq, c.Tk, c.ct, c.arithmetic)
    if key not in REFS:
        REFS[key] = E.references(E.scene(c.B, c.H, c.Tq, c.Tk), c.ct, c.arithmetic)
    return REFS[key]


def _launch(e, c, sc, items=None):
    """one launch of case c on the scene's batch items `items` (all of them by default): ([n][H][Tq][64], signature)"""
    for key, v in c.opts.items():
        e.set_option(key, v)
    sel = slice(None) if items is None else items
    sub = E.Scene(sc.Q[sel], sc.K[sel], sc.V[sel], sc.kind[sel], sc.tstar[sel])
    if c.form == "self":
        out, sig, guard = e.enc_attn_probe(qkv=E.qkv_of(sub))
    else:
        out, sig, guard = e.enc_attn_probe(q=E.q_rows_of(sub), k=sub.K, v=sub.V)
    assert guard, (c.name, sig, "the guard row behind the output was written")
    return np.ascontiguousarray(E.heads_of(out, c.H)), sig


def _run_case(e, c):
    sc = E.scene(c.B, c.H, c.Tq, c.Tk)
    out, sig = _launch(e, c, sc)
    assert E.sig_ok(sig, c), (c.name, sig, E.expected_signature(c))
    bad = np.argwhere(~np.isfinite(out))
    assert len(bad) == 0, (c.name, sig, f"{len(bad)} elements not written or not finite, first (b, h, query, channel) {bad[0].tolist()}")
    assert _same_bits(E.rnd_t(out, c.ct), out)
    refs = _refs(c)
    rs = E.ratios(out, refs)
    for tier, r in rs.items():
        k = c.group + (tier,)
        RATIOS[k] = max(RATIOS.get(k, 0.0), r)
    print(f"{c.name}: {sig} | error / bound " + " ".join(f"{t} {r:.3f}" for t, r in rs.items()))
    for tier, r in rs.items():
        assert r <= 1.0, (c.name, sig, f"tier {tier}", r, E.worst_element(out, refs[tier]))
    return out


def _cases(form, ct, key):
    return [c for c in E.cases() if c.form == form and c.ct == ct and (c.Tq if form == "self" else (c.Tq, c.Tk)) == key]


@pytest.mark.parametrize("T", E.SELF_T + (E.FULL_T,))
@pytest.mark.parametrize("ct", E.TYPES)
def test_self_form_against_the_float64_references(engines, ct, T):
    todo = _cases("self", ct, T)
    assert todo
    outs = {}
    try:
        for c in todo:
            outs[(c.variant, c.B, c.H)] = _run_case(engines(c.H, ct), c)
        for c in todo:
            sc = E.scene(c.B, c.H, c.Tq, c.Tk)
            if c.variant == "qw1":            # the kernel's comment: 64 and 32 queries per wave are bit-identical
                assert _same_bits(outs[("qw1", c.B, c.H)], outs[("qw2", c.B, c.H)]), (c.name, "flash_qw 1 and 2 differ")
            if c.arithmetic == "flash" and c.B > 1:     # a query's arithmetic does not depend on the batch around it
                for b in range(c.B):
                    alone, _ = _launch(engines(c.H, ct), c, sc, slice(b, b + 1))
                    assert _same_bits(alone[0], outs[(c.variant, c.B, c.H)][b]), (c.name, f"batch item {b} alone differs from its rows in the batch")
    finally:
        for H in {c.H for c in todo}:
            engines(H, ct).set_option("flash", 1); engines(H, ct).set_option("flash_qw", 2)


@pytest.mark.parametrize("nq,Tk", [(nq, Tk) for nq in E.CROSS_NQ for Tk in E.CROSS_TK] + [E.CROSS_FULL])
@pytest.mark.parametrize("ct", E.TYPES16)
def test_cross_form_and_the_32_row_rule(engines, ct, nq, Tk):
    todo = _cases("cross", ct, (nq, Tk))
    assert todo
    for c in todo:
        e = engines(c.H, ct)
        out = _run_case(e, c)
        if c.B > 1 and c.arithmetic == "flash":
            sc = E.scene(c.B, c.H, c.Tq, c.Tk)
            for b in range(c.B):
                alone, sig = _launch(e, c, sc, slice(b, b + 1))
                assert sig == f"enc_attn_flash_kernel<{E.sig_type(ct)}, true, 1> clips 1 rows {nq}"
                assert _same_bits(alone[0], out[b]), (c.name, f"clip {b} alone differs from its rows among {c.B} clips")


def test_refusals(engines):
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e, f = engines(4, "bf16"), engines(5, "f32")
    d = 4 * 64
    ok = np.zeros((2, 20, 3 * d), np.float32)
    out, sig, guard = e.enc_attn_probe(qkv=ok)
    assert guard and sig.startswith("enc_attn_flash_kernel<unsigned short, false, 2>") and not out.any()    # v = 0: the mean of zeros
    for shape in ((4, 20, 3 * d), (1, 1501, 3 * d)):       # more than max_batch items; T beyond n_audio_ctx
        with pytest.raises(TtasrError):
            e.enc_attn_probe(qkv=np.zeros(shape, np.float32))
    lib, h = e.lib, e.h
    buf = np.zeros(2 * 20 * d, np.float32)
    p = lambda a: a.ctypes.data
    assert lib.ttasr_enc_attn_probe(h, 0, 2, 0, p(ok), None, None, 0, p(buf), None, 0) < 0          # T = 0
    assert lib.ttasr_enc_attn_probe(h, 0, 2, 20, None, None, None, 0, p(buf), None, 0) < 0          # qkv NULL
    assert lib.ttasr_enc_attn_probe(h, 0, 2, 20, p(ok), None, None, 0, None, None, 0) < 0           # out NULL
    assert lib.ttasr_enc_attn_probe(h, 2, 2, 20, p(ok), None, None, 0, p(buf), None, 0) < 0         # form
    q, kv = np.zeros((2, 20, d), np.float32), np.zeros((2, 4, 30, 64), np.float32)
    assert lib.ttasr_enc_attn_probe(h, 1, 2, 20, p(q), None, p(kv), 30, p(buf), None, 0) < 0        # k NULL
    assert lib.ttasr_enc_attn_probe(h, 1, 2, 20, p(q), p(kv), p(kv), 0, p(buf), None, 0) < 0        # no frames
    assert lib.ttasr_enc_attn_probe(h, 1, 2, 20, p(q), p(kv), p(kv), 1501, p(buf), None, 0) < 0     # frames beyond n_audio_ctx
    assert lib.ttasr_enc_attn_probe(h, 1, 2, 449, p(q), p(kv), p(kv), 30, p(buf), None, 0) < 0      # rows beyond n_text_ctx
    assert lib.ttasr_enc_attn_probe(h, 1, 2, 20, p(q), p(kv), p(kv), 30, p(buf), None, 0) == 0
    with pytest.raises(TtasrError):                        # the cross form on the f32 engine
        f.enc_attn_probe(q=np.zeros((1, 40, 320), np.float32), k=np.zeros((1, 5, 30, 64), np.float32), v=np.zeros((1, 5, 30, 64), np.float32))
    out, sig, guard = f.enc_attn_probe(qkv=np.zeros((1, 20, 960), np.float32))
    assert guard and sig == "enc_attn_simple_kernel<float> grid 2560"
    with e.session(e.gen_opts(4, True), 4):
        with pytest.raises(TtasrError):                    # refused while a session is open
            e.enc_attn_probe(qkv=ok)
    e.enc_attn_probe(qkv=ok)


@pytest.mark.parametrize("ct", E.TYPES)
def test_encode_and_generate_are_bit_identical_before_and_after_a_probe_sequence(engines, ct):
    H = 3
    e = engines(H, ct)
    e.set_audio_ctx(30)
    try:
        st = e.special
        e.log_mel([synth.noise_clip(i, 30 * 320) for i in range(3)], want_output=False)
        prompt = [st.sot, st.lang_zh, st.transcribe]
        opts = e.gen_opts(12, True, suppress=[1, 2, 7, st.sot], begin_suppress=[5, st.eot], check_interval=1)

        def generate():
            r = e.generate([prompt] * 3, opts)
            return [list(t) for t in r.tokens], np.asarray(r.sum_logprob, np.float32).tobytes()
        enc = e.encode(3, want_output=True)
        before = generate()
        n = 0
        for c in E.cases():
            if c.ct == ct and c.H == H and (c.Tq, c.Tk) in ((65, 65), (160, 150)):
                _launch(e, c, E.scene(c.B, c.H, c.Tq, c.Tk))
                n += 1
        assert n >= (2 if ct == "f32" else 4)
        assert generate() == before                         # the resident cross-KV, the search state and the graphs
        assert _same_bits(e.encode(3, want_output=True), enc)   # the resident mel and the encoder's workspaces
        assert generate() == before
    finally:
        e.set_audio_ctx(0)
        e.set_option("flash", 1); e.set_option("flash_qw", 2)


def test_zz_report_largest_error_over_bound():
    """prints the table recorded in DESIGN.md section 4.36 (nothing to assert beyond the cases' own assertions)"""
    for (group, ct, tier), r in sorted(RATIOS.items()):
        print(f"largest error / bound  {group:20s} {ct:5s} tier {tier}  {r:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
