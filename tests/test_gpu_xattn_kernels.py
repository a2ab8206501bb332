"""GPU: the e4m3 cross-KV quantisers and every cross-attention kernel form of the decode step against plain references
(oracle/whisper_ref.py: xkv_quant_ref in float32 steps, cross_attn_ref in float64), through the known-answer hooks
ttasr_get_cross_kv_fp8 and ttasr_cross_attn_probe.  Inputs, case table and tolerance live in
tests/xattn_cases.py; tests/test_xattn_reference_host.py shows on the CPU that they see the bugs they are there for.

  (a) quantiser: codes and scales of every block kind, window and type equal xkv_quant_ref of the 16-bit readback, bit for bit
      (the build uses HIP's correctly rounded float32 division and one multiply: no tolerance), both layers, K and V;
  (b) session quantiser: the live slots of a greedy and a beam session equal the static encode's blocks of the same clip;
  (c) (d) attention: the probe's output against cross_attn_ref over what the form reads (codes x scale, or the 16-bit cache),
      inside the derived bound |out - ref| <= ulp_T(ref) / 2 (1 + 2^-6) + (2 delta + Tk 2^-24) max_t |V[t, c]|,
      delta = 65 2^-24 sum |q| |k|_max + 40 2^-23 + 2^-22 (xattn_cases.reference);
  (e) finished rows: live rows bit-identical to the all-live run, finished rows (per-row forms) and fully finished groups 0.
Every case asserts the signature of the kernel it names.  Before any comparison the 16-bit cache is read back and must equal what
was placed, bit for bit (identity / permutation k_proj and v_proj weights: xattn_cases.state_dict).

Engines: 1 encoder layer (never run except in (b)), 2 decoder layers, 20 and 16 heads, n_audio_ctx 1500, max_batch 32, bf16 and
fp16, created once per module.  Largest error / bound per kernel form: printed by the last test, recorded in DESIGN.md 4.17."""
import numpy as np
import pytest
import torch

import xattn_cases as X
from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COMPUTE = {"bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
RATIOS = {}     # (form, type) -> largest observed error / bound


def _new_engine(H, ct, max_batch=X.MAX_BATCH):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(X.dims(H), COMPUTE[ct], max_batch)
    e.load_weights(X.state_dict(H).items())
    return e


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(H, ct):
        if (H, ct) not in made:
            made[(H, ct)] = _new_engine(H, ct)
        return made[(H, ct)]
    yield get
    for e in made.values():
        e.close()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _place(e, blocks, fp8_mode):
    """blocks -> the cache, through ttasr_set_encoder_output; the 16-bit readback must be exactly what was placed"""
    e.set_option("xkv_fp8", fp8_mode)
    e.set_encoder_output(X.blocks_to_enc(blocks))
    B = blocks.shape[0]
    for layer in range(2):
        for which in range(2):
            assert _same_bits(e.cross_kv(layer, which, B), np.ascontiguousarray(X.cache_of(blocks, layer, which))), (layer, which)


def _check_fp8_copy(e, blocks):
    """the resident e4m3 copy == xkv_quant_ref of the (verified) 16-bit cache: codes and scales, both layers, K and V"""
    B = blocks.shape[0]
    for layer in range(2):
        for which in range(2):
            codes, sc = e.cross_kv_fp8(layer, which, B)
            want_codes, want_sc = R.xkv_quant_ref(np.ascontiguousarray(X.cache_of(blocks, layer, which)))
            bad = np.argwhere(sc.view(np.uint32) != want_sc.view(np.uint32))
            assert len(bad) == 0, ("scale", layer, which, bad[:4].tolist(), sc[tuple(bad[0])], want_sc[tuple(bad[0])])
            bad = np.argwhere(codes != want_codes)
            assert len(bad) == 0, ("codes", layer, which, len(bad), bad[:4].tolist(),
                                   [(int(codes[tuple(i)]), int(want_codes[tuple(i)])) for i in bad[:4]])


# ---- (a) the quantiser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", X.WINDOWS + (X.FULL_WINDOW,))
@pytest.mark.parametrize("ct", X.TYPES)
def test_quantiser_codes_and_scales_equal_the_float32_reference(engines, ct, window):
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e = engines(20, ct)
    e.set_audio_ctx(window)
    blocks = X.quant_blocks(ct, window, 3, 20)
    kinds = {X.quant_kind(b, h, window) for b in range(3) for h in range(20)}
    assert kinds == set(X.QUANT_KINDS)
    _place(e, blocks, 2)
    _check_fp8_copy(e, blocks)
    # a second encode with fewer clips: its slots hold the new clips' codes AND scales; the hook reads resident clips only
    again = X.quant_blocks(ct, window, 2, 20, salt=5)
    assert not np.array_equal(again, blocks[:2])
    _place(e, again, 2)
    _check_fp8_copy(e, again)
    with pytest.raises(TtasrError):
        e.cross_kv_fp8(0, 0, 3)


def test_hook_refusals(engines):
    from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
    e = engines(20, "bf16")
    e.set_audio_ctx(16)
    blocks = X.quant_blocks("bf16", 16, 2, 20)
    _place(e, blocks, 0)
    with pytest.raises(TtasrError):          # option off
        e.cross_kv_fp8(0, 0, 2)
    e.set_option("xkv_fp8", 2)
    with pytest.raises(TtasrError):          # no encode since the option was set
        e.cross_kv_fp8(0, 0, 2)
    _place(e, blocks, 2)
    e.cross_kv_fp8(1, 1, 2)
    for layer, which, B in ((2, 0, 2), (-1, 0, 2), (0, 2, 2), (0, 0, 0), (0, 0, 33)):
        with pytest.raises(TtasrError):
            e.cross_kv_fp8(layer, which, B)
    q = np.zeros((4, 1280), np.float32)
    for layer, kv_div in ((2, 1), (0, 3), (0, 0)):
        with pytest.raises(TtasrError):
            e.cross_attn_probe(layer, q, kv_div)
    with pytest.raises(TtasrError):          # 4 clips needed, 2 resident
        e.cross_attn_probe(0, q, 1)
    with pytest.raises(TtasrError):          # 5 partial tiles
        e.cross_attn_probe(0, np.zeros((5, 2, 1280), np.float32), 1)
    f = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    try:
        f.load_weights(synth.state_dict(PRESETS["micro"]).items())
        with pytest.raises(TtasrError):      # no resident encoder state
            f.cross_attn_probe(0, np.zeros((2, 128), np.float32), 1)
        f.set_encoder_output(np.zeros((2, 50, 128), np.float32))
        with pytest.raises(TtasrError):      # the f32 engine has no e4m3 copy
            f.cross_kv_fp8(0, 0, 2)
        out, sig = f.cross_attn_probe(0, np.zeros((2, 128), np.float32), 1)
        assert sig.startswith("cross_attn_decode_kernel<float") and np.isfinite(out).all()
    finally:
        f.close()


# ---- (b) the session's admission quantiser -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,beam", [("bf16", 0), ("f16", 2)], ids=["greedy-bf16", "beam2-f16"])
def test_session_slots_hold_the_static_encode_s_blocks(ct, beam):
    """xkv_fp8 = 2, window 30, real synthetic clips through the encoder.  Static: the clips in encodes of two, codes and scales read
    (and held to xkv_quant_ref of the 16-bit readback).  Session: after every poll the live slots - greedy row = slot, beam group
    = slot (ttasr_session_rows) - must hold their clip's static codes and scales; a slot is reused by a later clip."""
    window, n_clips = 30, 5
    slots = 2
    e = _new_engine(20, ct, max_batch=slots * max(beam, 1))
    try:
        e.set_option("xkv_fp8", 2)
        e.set_audio_ctx(window)
        kinds = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
        clips = [kinds[i % 3](40 + i, window * 320) for i in range(n_clips)]
        static = []
        for i in range(0, n_clips, slots):
            n = min(slots, n_clips - i)
            e.log_mel(clips[i:i + n], want_output=False)
            e.encode(n)
            per = {}
            for layer in range(2):
                for which in range(2):
                    codes, sc = e.cross_kv_fp8(layer, which, n)
                    want = R.xkv_quant_ref(e.cross_kv(layer, which, n))
                    assert _same_bits(codes, want[0]) and _same_bits(sc, want[1]), (i, layer, which)
                    per[(layer, which)] = (codes, sc)
            static += [{k: (v[0][j], v[1][j]) for k, v in per.items()} for j in range(n)]
        assert any(not _same_bits(static[0][(0, 0)][0], static[j][(0, 0)][0]) for j in range(1, n_clips))
        st = e.special
        prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
        opts = e.gen_opts(8, False, suppress_eot=True, check_interval=1, sot_index=0)
        caps = [2, 6, 3, 4, 2]
        held = [[] for _ in range(slots)]
        checked = 0
        with e.session(opts, len(prompt), beam=beam or 1, patience=1.0 if beam else None) as s:
            ids = s.submit(clips, [prompt] * n_clips, caps)
            while s.pending > 0:
                s.poll(max_steps=1)
                row_clip = s.rows()["clip"].tolist()
                live = {}
                for slot in range(slots):
                    cid = row_clip[slot * max(beam, 1)]
                    if cid >= 0:
                        live[slot] = ids.index(cid)
                        if not held[slot] or held[slot][-1] != live[slot]:
                            held[slot].append(live[slot])
                if not live:
                    continue
                for layer in range(2):
                    for which in range(2):
                        codes, sc = e.cross_kv_fp8(layer, which, slots)
                        for slot, j in live.items():
                            assert _same_bits(codes[slot], static[j][(layer, which)][0]), (slot, j, layer, which)
                            assert _same_bits(sc[slot], static[j][(layer, which)][1]), (slot, j, layer, which)
                            checked += 1
        assert sorted(sum(held, [])) == list(range(n_clips)), held      # every clip was seen live in a slot
        assert all(len(h) >= 2 for h in held), held                      # and every slot was reused
        assert checked >= 4 * n_clips
    finally:
        e.close()


# ---- (c) (d) (e) attention -----------------------------------------------------------------------------------------------------
def _run_case(e, c, window, ct):
    for key, default in X.DEFAULT_OPTS.items():
        e.set_option(key, c.opt(key, default))
    o = X.operands(c, window)
    qflat = o.q.reshape(c.n_rows, -1)
    feed = X.slab_parts(o.q, c.n_slab) if c.n_slab else qflat
    out, sig = e.cross_attn_probe(c.layer, feed, c.kv_div)
    assert X.sig_matches(sig, c, window, ct), (c.name, window, sig, X.expected_kernel(c, window, ct))
    ref = X.reference(o.q, o.K, o.V, c.kv_div, ct)
    assert ref["span"].max() <= 40 and ref["sqk"].max() <= 64                      # what the bound's delta assumes
    assert _same_bits(X.rnd(out, ct), out)
    ratio = X.error_ratio(out, ref)
    form = X.expected_kernel(c, window, ct)[0].split("<")[0] + ("+slab" if c.n_slab else "")
    RATIOS[(form, ct)] = max(RATIOS.get((form, ct), 0.0), ratio)
    print(f"{ct} H{c.H} w{window} {c.name}: {sig} | error / bound {ratio:.3f}")
    assert ratio <= 1.0, (c.name, window, ct, sig, ratio)
    if c.done:
        flags = X.done_flags(c)
        out2, sig2 = e.cross_attn_probe(c.layer, feed, c.kv_div, done=flags)
        assert sig2 == sig
        out, out2 = out.reshape(c.n_rows, c.H, 64), out2.reshape(c.n_rows, c.H, 64)
        live = flags == 0
        assert live.any() and (~live).any()
        assert _same_bits(out2[live], out[live]), (c.name, window)               # live rows: bit-identical to the all-live run
        assert np.abs(out[live]).max() > 0
        if c.done == "alt":
            assert not out2[~live].any(), (c.name, window)                       # per-row forms: finished rows come back 0
        else:
            assert not out2[:c.kv_div].any(), (c.name, window)                   # a fully finished group comes back 0


@pytest.mark.parametrize("window", X.WINDOWS + (X.FULL_WINDOW,))
@pytest.mark.parametrize("H", X.HEADS)
@pytest.mark.parametrize("ct", X.TYPES)
def test_attention_forms_against_the_float64_reference(engines, ct, H, window):
    e = engines(H, ct)
    e.set_audio_ctx(window)
    blocks = X.scene(H, window)
    todo = sorted(X.cases(H, window), key=lambda c: (c.fp8_mode, c.layer, c.n_rows, c.kv_div, c.reads_fp8))
    try:
        for mode in (0, 1, 2):
            group = [c for c in todo if c.fp8_mode == mode]
            if not group:
                continue
            _place(e, blocks, mode)
            if mode:
                _check_fp8_copy(e, blocks)
            for c in group:
                _run_case(e, c, window, ct)
    finally:
        for key, default in X.DEFAULT_OPTS.items():
            e.set_option(key, default)
        e.set_option("xkv_fp8", 0)
        X._operands.cache_clear()


def test_probe_leaves_search_state_and_graphs_alone(engines):
    """a generate call, a probe between, the same generate call: bit-identical results; and the step API's position survives"""
    e = engines(20, "bf16")
    e.set_audio_ctx(30)
    blocks = X.scene(20, 30)[:4]
    _place(e, blocks, 0)
    st = e.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(6, False, suppress_eot=True)
    a = e.generate([prompt] * 4, opts)
    e.decode_reset(4)
    l0 = e.decode_step([st.sot] * 4)
    q = np.ascontiguousarray(X.scene(20, 30)[:4, :, 0].reshape(4, -1))
    e.cross_attn_probe(0, q, 1, done=np.array([1, 0, 1, 0], np.int32))
    l1 = e.decode_step([st.lang_zh] * 4)
    e.decode_reset(4)
    assert _same_bits(e.decode_step([st.sot] * 4), l0)
    assert _same_bits(e.decode_step([st.lang_zh] * 4), l1)
    b = e.generate([prompt] * 4, opts)
    assert a.tokens == b.tokens and _same_bits(np.asarray(a.sum_logprob), np.asarray(b.sum_logprob))


def test_zz_report_largest_error_over_bound_per_form():
    """prints the table recorded in DESIGN.md section 4.17 / profiles/LAB_NOTEBOOK.md (nothing to assert beyond the cases' own
    assertions: every ratio is at most 1)"""
    for (form, ct), r in sorted(RATIOS.items()):
        print(f"largest error / bound  {form:34s} {ct:5s} {r:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
