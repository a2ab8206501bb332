"""CPU: the geometry sweep's table (tests/geometry_table.py) is accepted by ttasr_create as include/ttasr.h states its limits,
reaches every dispatch threshold it claims to reach from both sides, and its oracle side is affordable: the smallest, the
largest and the two published entries run through synth.state_dict and the oracle here and give finite logits."""
import time

import numpy as np
import pytest
import torch

from geometry_table import (PUBLISHED, ROW_BATCHES, TABLE, VOCAB_EDGES, WINDOWS, XATTN_BEAMS, XATTN_PAIRS, Case, oracle_weights,
                            reference)
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import PRESETS, SpecialTokens

torch.set_grad_enabled(False)


def test_ids_are_unique_and_spell_the_shape():
    ids = [c.id for c in TABLE]
    assert len(set(ids)) == len(ids)
    for c in TABLE:
        d = c.dims
        for part in (f"H{d.n_heads}d{d.d_model}f{d.ffn_dim}", f"V{d.vocab}", f"B{c.batch}", c.compute):
            assert part in c.id, (c.id, part)


@pytest.mark.parametrize("case", TABLE, ids=[c.id for c in TABLE])
def test_entry_is_inside_the_limits_of_the_header(case):
    """include/ttasr.h (ttasr_config, 'Geometry limits', ttasr_set_audio_ctx, ttasr_generate_beam) and ttasr_create's checks."""
    d = case.dims
    assert d.n_heads >= 1 and d.d_model == 64 * d.n_heads and d.d_model <= 1280
    assert d.ffn_dim >= 64 and d.ffn_dim % 64 == 0
    assert d.n_mels > 0 and d.n_mels % 8 == 0
    assert 2 <= d.vocab <= 53248
    assert 2 <= d.n_text_ctx <= 448
    assert d.n_audio_ctx >= 1 and d.enc_layers == 2 and d.dec_layers == 2
    assert case.compute in ("f32", "bf16", "f16")
    assert 1 <= case.batch <= 128
    if case.audio_ctx:
        assert 4 <= case.audio_ctx <= d.n_audio_ctx and case.audio_ctx % 2 == 0
    if case.beam:
        assert 1 <= case.beam <= 7 and case.batch % case.beam == 0
    # the decode steps of a case (prompt + two text tokens) fit the text context, and every token is in the vocabulary
    st = SpecialTokens.for_vocab(d.vocab)
    assert 6 <= d.n_text_ctx
    assert 0 < st.eot < st.timestamp_begin < d.vocab and max(220, 17 + 3 * 127) < d.vocab


def _of(axis):
    return [c for c in TABLE if c.axis == axis]


def test_published_widths_in_every_compute_type():
    assert (PUBLISHED[0].d_model, PUBLISHED[0].n_heads, PUBLISHED[0].ffn_dim) == (512, 8, 2048)
    assert (PUBLISHED[1].d_model, PUBLISHED[1].n_heads, PUBLISHED[1].ffn_dim) == (1024, 16, 4096)
    for dims, name in zip(PUBLISHED, ("base", "medium")):
        p = PRESETS[name]
        assert (dims.n_mels, dims.n_audio_ctx, dims.vocab, dims.n_text_ctx) == (p.n_mels, p.n_audio_ctx, p.vocab, p.n_text_ctx) == (80, 1500, 51865, 448)
        assert {c.compute for c in _of("published") if c.dims == dims} == {"f32", "bf16", "f16"}


def test_every_head_count_and_every_ffn_kind():
    heads = _of("heads")
    assert {c.dims.n_heads for c in heads if c.compute == "bf16"} == set(range(1, 21))
    for ct in ("f16", "f32"):
        assert {c.dims.n_heads for c in heads if c.compute == ct} == {4, 8, 12, 16, 20}
    for subset in (heads, [c for c in heads if c.compute == "f16"]):
        kinds = set()
        for c in subset:
            d, f = c.dims.d_model, c.dims.ffn_dim
            kinds.add("4d" if f == 4 * d else "64" if f == 64 else "5120" if f == 5120 else "odd" if (f // 64) % 2 == 1 else "?")
        assert kinds == {"4d", "64", "5120", "odd"}, kinds
    for c in heads:
        assert c.dims.n_audio_ctx % 64 != 0 and 64 < c.dims.n_audio_ctx < 128
        assert c.batch * c.dims.n_audio_ctx >= 256 and (c.batch * c.dims.n_audio_ctx) % 64 != 0   # the tiled encoder GEMMs, ragged
    # K / 64 of the decode GEMMs: every value 1 .. 20 (K = d) and the ffn values on top
    assert {c.dims.d_model // 64 for c in heads} == set(range(1, 21))


def test_every_row_group_and_the_vocabulary_kernels_batch_limit():
    rows = _of("rows")
    assert {(c.batch + 31) // 32 for c in rows} == {1, 2, 3, 4}
    widths = {c.dims.d_model for c in rows}
    assert len(widths) >= 3 and 1024 in widths
    for w in widths:
        assert {c.batch for c in rows if c.dims.d_model == w and c.compute == "bf16"} == set(ROW_BATCHES)
    assert {c.batch for c in rows if c.compute == "f16"} == set(ROW_BATCHES)
    assert {64, 65} <= set(ROW_BATCHES)                      # launch_gemm_vocab: B <= 64
    for c in rows:                                           # ... and every other precondition of that kernel holds
        assert c.dims.vocab >= 8192 and c.dims.d_model % 128 == 0 and c.dims.d_model // 128 <= 10 and c.dims.vocab % 5120 != 0
        assert c.dims.vocab % 32 != 0


def test_vocabulary_edges():
    vs = {c.dims.vocab for c in _of("vocab")}
    assert vs == set(VOCAB_EDGES) and {8191, 8192, 8193, 53248} <= vs
    assert sum(v % 5120 == 0 for v in vs) >= 2               # the 20-row layout
    for c in _of("vocab"):
        assert c.dims.d_model % 128 == 0                     # so that only N decides between the two vocabulary kernels
    for v in vs:
        assert {c.compute for c in _of("vocab") if c.dims.vocab == v} == {"f32", "bf16", "f16"}


def test_cross_attention_thresholds_from_both_sides():
    for axis, items in (("xattn", {c.batch * c.dims.n_heads for c in _of("xattn")}),
                        ("xattn-beam", {c.batch * c.dims.n_heads for c in _of("xattn-beam")})):
        for thr in (256, 512):
            assert thr - 1 in items and thr in items, (axis, thr, items)
            assert any(thr < i <= thr + 2 for i in items), (axis, thr, items)
    assert {(c.batch, c.dims.n_heads) for c in _of("xattn")} == set(XATTN_PAIRS)
    for B, H in XATTN_PAIRS:
        assert {c.compute for c in _of("xattn") if (c.batch, c.dims.n_heads) == (B, H)} == {"f32", "bf16", "f16"}
    assert {(c.n_clips, c.beam, c.dims.n_heads) for c in _of("xattn-beam")} == set(XATTN_BEAMS)
    assert all(c.compute == "f32" for c in _of("xattn-beam"))
    assert sum(c.beam >= 2 for c in _of("xattn-beam")) >= 5
    for c in _of("xattn") + _of("xattn-beam"):
        assert c.dims.n_audio_ctx >= 128                     # two 64-frame slices possible below 256 items


def test_mel_bins_text_contexts_and_windows():
    mt = _of("mel-text")
    assert {c.dims.n_mels for c in mt} == {8, 24, 80, 128}
    assert any(10 <= c.dims.n_text_ctx <= 99 for c in mt) and any(c.dims.n_text_ctx == 448 for c in mt)
    assert all(c.compute == "f32" for c in mt)
    win = _of("window")
    assert {c.audio_ctx for c in win} == set(WINDOWS) == {4, 62, 64, 66, 1498}
    for c in win:
        assert (c.dims.d_model, c.dims.n_heads, c.dims.n_audio_ctx) == (512, 8, 1500)
    for w in WINDOWS:
        assert {c.compute for c in win if c.audio_ctx == w} == {"bf16", "f16"}


def _cost(c: Case) -> int:
    return sum(int(np.prod(shape)) for _, shape, _ in synth.tensor_specs(c.dims)) + c.batch * c.window * c.dims.d_model


def test_oracle_side_runs_on_the_extremes_and_the_published_entries(capsys):
    """Also the affordability check of the sweep's CPU side: the elapsed time of each oracle run is printed (pytest -s)."""
    decode = [c for c in TABLE if not c.beam]
    picks = {min(decode, key=_cost).id: min(decode, key=_cost), max(decode, key=_cost).id: max(decode, key=_cost)}
    for dims in PUBLISHED:
        c = next(c for c in TABLE if c.axis == "published" and c.dims == dims and c.compute == "bf16")
        picks[c.id] = c
    assert len(picks) >= 3
    for cid, c in picks.items():
        t0 = time.perf_counter()
        sd = synth.state_dict(c.dims)
        W = oracle_weights(c, sd)
        ref = reference(c, W)
        dt = time.perf_counter() - t0
        with capsys.disabled():
            print(f"\n  oracle {cid}: {dt:.1f} s", end="")
        assert ref.mel.shape == (c.batch, c.dims.n_mels, 2 * c.window)
        assert ref.enc.shape == (c.batch, c.window, c.dims.d_model) and bool(torch.isfinite(ref.enc).all())
        assert len(ref.logits) == 6
        for lg in ref.logits:
            assert lg.shape == (c.batch, c.dims.vocab) and np.isfinite(lg).all()
        if c.compute in ("bf16", "f16") and c.axis != "published":
            # the sensitivity run differs from the plain one, by a 16-bit-sized amount
            from geometry_table import TORCH_DTYPE
            r2 = reference(c, W, round_activations=TORCH_DTYPE[c.compute])
            s = max(float(np.abs(a - b).max()) for a, b in zip(ref.logits, r2.logits))
            assert 0.0 < s < 0.5, s
