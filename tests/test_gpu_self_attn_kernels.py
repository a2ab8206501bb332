"""GPU: the decoder self-attention kernels over the paged KV pool - self_attn_decode_kernel<T, MODE 0|1|2|3, SLAB, IDENT>,
copy_pages_kernel, prefill_append_kernel, prefill_attend_kernel - one launch at a time against a float64 reference
(oracle/whisper_ref.py self_attn_ref / self_attn_causal_ref), through the known-answer hooks ttasr_self_kv_fill / _set / _get and
ttasr_self_attn_probe.  Inputs, case table and the derived tolerance live in tests/self_attn_cases.py;
tests/test_self_attn_reference_host.py shows on the CPU that they see the bugs they are there for.

Every case: both layers of the pool are filled with a NaN pattern of the engine type, the rows' histories [0, pos) are placed and
read back bit for bit, the named form is launched once, and then
  * the signature names the instantiation the case names;
  * |out - ref| <= the bound per output channel (a read outside a row's logical history is a non-finite output);
  * the case's layer is bit-identical to before except the one appended slot per live row, which holds round_T(k), round_T(v);
    the other layer is untouched;
  * identity table: the computed-page-id instantiation (IDENT) and the loaded-table one return the same bits;
  * finished rows: live rows bit-identical to the all-live run, finished rows 0, nothing appended for them;
  * beam table: made by the copy form from pair lists of 1 and 5 pairs - destination = source in every layer, everything else
    unchanged, an empty list launches nothing;
  * packed: a sequence alone returns the bits it returns inside the pass.
Engines: 1 encoder layer, 2 decoder layers, n_text_ctx 448, max_batch 8; f32, bf16, f16 at 6 heads and bf16 at 20 heads, created
once per module.  Largest error / bound per (form, type): printed by the last test, recorded in DESIGN.md 4.28."""
import numpy as np
import pytest
import torch

import self_attn_cases as S
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COMPUTE = {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
RATIOS = {}     # (form, type) -> largest observed error / bound
PARAMS = [pytest.param(H, ct, c, id=f"h{H}-{ct}-{c.name}") for H, ct in S.ENGINES for c in S.cases_of(ct)]


@pytest.fixture(scope="module")
def engines():
    from taiwan_tongues_asr_ce_amd.engine import Engine
    made = {}

    def get(H, ct):
        if (H, ct) not in made:
            e = Engine(S.dims(H), COMPUTE[ct], S.MAX_BATCH)
            e.load_weights(synth.state_dict(S.dims(H)).items())
            made[(H, ct)] = e
        return made[(H, ct)]
    yield get
    for e in made.values():
        e.close()


def _load_pool(e, ct, pools):
    """poison everywhere, then the finite positions [0, n) of every page that holds any; the readback must be the scene's bits"""
    e.self_kv_fill(-1, S.POISON[ct])
    for layer, pool in pools.items():
        n_fin = np.isfinite(pool[:, 0, 0, :, 0]).sum(axis=1)             # leading finite positions per page
        for n in np.unique(n_fin[n_fin > 0]):
            pages = np.nonzero(n_fin == n)[0]
            e.self_kv_set(layer, pages, np.nan_to_num(pool[pages]), int(n))
        bad = S.pool_mismatch(e.self_kv_get(layer), pool)
        assert not bad, ("placed pool differs from its readback at (page, K|V, head, position, channel)", layer, bad)


def _check_pool(e, sc, want, what):
    for layer in (0, 1):
        bad = S.pool_mismatch(e.self_kv_get(layer), want[layer])
        assert not bad, (f"{sc.case.name} ({sc.ct}, H {sc.H}) {what}: pool layer {layer} (case layer {sc.case.layer}) differs at "
                         f"(page, K|V, head, position, channel)", bad)


def _launch(e, sc, ident, done=None, feed=None):
    c = sc.case
    out, sig = e.self_attn_probe(c.form, c.layer, sc.feed() if feed is None else feed, sc.geom(), sc.aux(), identity_pages=ident, row0=c.row0, done=done)
    assert sig == S.expected_sig(c, sc.ct, sc.H, ident), (c.name, sig)
    return out.reshape(-1, sc.H, 64)


def _note(sc, ratio):
    key = (sc.case.form, sc.ct)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


@pytest.mark.parametrize("H,ct,c", PARAMS)
def test_case_against_the_float64_reference(engines, H, ct, c):
    e = engines(H, ct)
    sc = S.scene(c, H, ct)
    ref = S.reference(sc)
    _load_pool(e, ct, sc.pool)
    if sc.copies:       # the beam table: the children's own pages come from the copy form, pair lists of 1 and 5 pairs
        _, sig = e.self_attn_probe("copy", aux=[])
        assert sig == ""                                                  # nothing launched ...
        _check_pool(e, sc, sc.pool, "after an empty copy list")          # ... nothing changed
        for pairs in sc.copies:
            _, sig = e.self_attn_probe("copy", aux=pairs)
            assert sig == f"copy_pages_kernel<{S.SIG_TYPE[ct]}> grid {len(pairs) // 2 * 2 * 256}", sig
        _check_pool(e, sc, S.pool_after(sc, done=np.ones(c.n_rows, np.int32)), "after the copy-on-write lists")
    outs = []
    for i, ident in enumerate(c.ident):
        if i:
            _load_pool(e, ct, {l: S.launch_pool(sc) if l == c.layer else p for l, p in sc.pool.items()} if sc.copies else sc.pool)
        out = _launch(e, sc, ident)
        ratio, where = S.error_ratio(out, ref)
        print(f"{c.name} h{H} {ct} ident {int(ident)}: error / bound {ratio:.4f}")
        _note(sc, ratio)
        assert ratio <= 1, S.describe(sc, out, ref, where)
        _check_pool(e, sc, S.pool_after(sc), f"after the launch (identity_pages {int(ident)})")
        outs.append(out)
    if len(outs) == 2:
        assert S.same_bits(outs[0], outs[1]), f"{c.name}: computed page ids and the loaded identity table disagree"
    if c.done:
        flags = S.done_flags(c.n_rows)
        _load_pool(e, ct, sc.pool)
        out = _launch(e, sc, c.ident[0], done=flags)
        live = flags == 0
        assert S.same_bits(out[live], outs[0][live]), f"{c.name}: live rows differ from the all-live run"
        assert not out[~live].any(), f"{c.name}: a finished row wrote its output"
        _check_pool(e, sc, S.pool_after(sc, done=flags), "with finished rows")


@pytest.mark.parametrize("H,ct", S.ENGINES)
def test_packed_sequence_alone_returns_the_bits_it_returns_in_the_pass(engines, H, ct):
    e = engines(H, ct)
    c = next(x for x in S.cases() if x.form == "packed")
    sc = S.scene(c, H, ct)
    _load_pool(e, ct, sc.pool)
    whole = _launch(e, sc, False)
    r0 = 0
    for s, n in enumerate(sc.lens):
        e.self_kv_fill(-1, S.POISON[ct])
        out, _ = e.self_attn_probe("packed", c.layer, sc.qkv[r0:r0 + n], [n], list(sc.pages[s]))
        assert S.same_bits(out.reshape(n, H, 64), whole[r0:r0 + n]), f"sequence {s} of length {n} depends on its pass-mates"
        r0 += n


def test_refusals(engines):
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e, f = engines(6, "bf16"), engines(6, "f32")
    d = 6 * 64
    z = np.zeros((4, 3 * d), np.float32)
    e.self_attn_probe("step", 0, z, [5])
    bad = [dict(layer=2), dict(layer=-1), dict(geom=[448]), dict(geom=[-1]), dict(geom=[5, 5]), dict(row0=5), dict(row0=-1),
           dict(aux=[0] * 7), dict(aux=[224] * S.N_PAGES), dict(aux=[-1] * S.N_PAGES), dict(qkv=np.zeros((9, 3 * d), np.float32)),
           dict(qkv=np.zeros((5, 4, 3 * d), np.float32))]
    for kw in bad:
        args = dict(form="step", layer=0, qkv=z, geom=[5])
        args.update(kw)
        with pytest.raises(TtasrError):
            e.self_attn_probe(**args)
    with pytest.raises(TtasrError):                    # a position per row
        e.self_attn_probe("rows", 0, z, [5])
    with pytest.raises(TtasrError):                    # partial tiles on the f32 engine
        f.self_attn_probe("step", 0, np.zeros((2, 4, 3 * d), np.float32), [5])
    with pytest.raises(TtasrError):                    # n_seq x npos != rows
        e.self_attn_probe("prefill", 0, z, [3, 2])
    with pytest.raises(TtasrError):                    # more sequences than max_batch
        e.self_attn_probe("prefill", 0, np.zeros((9, 3 * d), np.float32), [9, 1])
    with pytest.raises(TtasrError):                    # more than 512 rows
        e.self_attn_probe("prefill", 0, np.zeros((520, 3 * d), np.float32), [8, 65])
    with pytest.raises(TtasrError):                    # page outside the pool
        e.self_attn_probe("packed", 0, z, [4], [S.N_PAGES])
    with pytest.raises(TtasrError):                    # two pages for 4 positions
        e.self_attn_probe("packed", 0, z, [4], [1, 2])
    with pytest.raises(TtasrError):                    # pairs: odd count, a page outside the pool, more than max_batch
        e.self_attn_probe("copy", aux=[1, 2, 3])
    with pytest.raises(TtasrError):
        e.self_attn_probe("copy", aux=[1, S.N_PAGES])
    with pytest.raises(TtasrError):
        e.self_attn_probe("copy", aux=list(range(18)))
    for call in (lambda: e.self_kv_fill(2, 0), lambda: e.self_kv_get(2), lambda: e.self_kv_get(0, [S.N_PAGES]),
                 lambda: e.self_kv_set(0, [0], np.zeros((1, 2, 6, 16, 64), np.float32), 17),
                 lambda: e.self_kv_set(0, [-1], np.zeros((1, 2, 6, 16, 64), np.float32), 1)):
        with pytest.raises(TtasrError):
            call()
    with e.session(e.gen_opts(4, True), 4):
        for call in (lambda: e.self_attn_probe("step", 0, z, [5]), lambda: e.self_kv_fill(0, 0), lambda: e.self_kv_get(0),
                     lambda: e.self_kv_set(0, [0], np.zeros((1, 2, 6, 16, 64), np.float32), 1), lambda: e.self_attn_probe("copy", aux=[0, 1])):
            with pytest.raises(TtasrError):            # refused while a session is open
                call()
    e.self_attn_probe("step", 0, z, [5])


@pytest.mark.parametrize("H,ct", S.ENGINES)
def test_generate_is_bit_identical_before_and_after_a_probe_sequence(engines, H, ct):
    e = engines(H, ct)
    st = e.special
    n = S.dims(H).n_frames * 160
    e.log_mel([synth.noise_clip(i, n) for i in range(3)])
    e.encode(3)
    prompt = [st.sot, st.lang_zh, st.transcribe]
    opts = e.gen_opts(24, True, suppress=[1, 2, 7, st.sot], begin_suppress=[5, st.eot], check_interval=1)

    def run():
        r = e.generate([prompt] * 3, opts)
        return [list(t) for t in r.tokens], np.asarray(r.sum_logprob, np.float32).tobytes()
    before = run()
    perm = S.CASES_BY_NAME["rows-mix0-permuted"]
    for c in (perm, S.CASES_BY_NAME["step-beam"], S.CASES_BY_NAME["packed"], S.CASES_BY_NAME["prefill-npos33-permuted"]):
        sc = S.scene(c, H, ct)
        _load_pool(e, ct, sc.pool)
        for pairs in sc.copies:
            e.self_attn_probe("copy", aux=pairs)
        _launch(e, sc, False)
    assert run() == before
    # the table is the identity again: the loaded-table instantiation on no table reads what the computed-page-id one reads
    sc = S.scene(S.CASES_BY_NAME["step-pos129-row0-4"], H, ct)
    _load_pool(e, ct, sc.pool)
    a = _launch(e, sc, True)
    _load_pool(e, ct, sc.pool)
    assert S.same_bits(a, _launch(e, sc, False))


def test_zz_report_largest_error_over_bound():
    for (form, ct), r in sorted(RATIOS.items()):
        print(f"self-attention {form:8s} {ct:5s} largest error / bound = {r:.4f}")
    assert all(r <= 1 for r in RATIOS.values())
