"""GPU: the swizzled cross-wave reduction buffer of the decode GEMMs changes where a partial sum waits in LDS, not what is added.

`dec_red_swizzle` = 1 stores the 16-byte chunk c of row b of a wave's 32 x 32 partial tile at chunk slot c ^ (b & 7) of that row
(conflict-free ds_write_b128), 0 keeps linear rows (kernels_skinny.hip, gemm_skinny_kernel / gemm_vocab_kernel).  The reader undoes
the XOR and adds the waves in the same fixed order, so step logits (ttasr_decode_step) and tokens must be EQUAL BIT FOR BIT with
either setting:
  - tiny width (K = 384 / 1536, vocabulary 51 865; 2 decoder layers and a 96-position audio context keep it quick - the GEMM
    shapes are the tiny model's) at 1, 20, 32, 33, 64, 97 and 128 rows: 1-4 row groups with ragged last groups, the looped and
    the straight-line forms, 4- and 8-wave workgroups, the persistent vocabulary kernel (<= 64 rows) and the generic one beyond;
  - one decoder layer at large-v3 width (d 1280, ffn 5120, vocabulary 51 866) at 32 rows: the 20-row narrow fc1 blocks, where
    chunk slots 5-7 of a row are written and never read;
  - the vocabulary GEMM's ragged last n-block (51 865 = 1620 * 32 + 25, 51 866 = 1620 * 32 + 26: `en + 3 >= N`);
  - beam search at 40 rows (8 clips x 5).
The encoder is not what this file is about: the cross-KV comes from seeded encoder rows."""
import numpy as np
import pytest
import torch

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, WhisperDims

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY_W = WhisperDims("tiny-width-a96", 80, 96, 384, 6, 1536, 1, 2, 51865, 32)
LARGE_W = WhisperDims("large-v3-width-1layer-a96", 128, 96, 1280, 20, 5120, 1, 1, 51866, 32)
MAX_B = 128
STEP_TOKENS = 5


def _engine(dims):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(dims, COMPUTE_BF16, MAX_B)
    e.load_weights(synth.state_dict(dims).items())
    g = np.random.Generator(np.random.Philox(key=dims.d_model + dims.n_audio_ctx))
    e.set_encoder_output(g.standard_normal((MAX_B, dims.n_audio_ctx, dims.d_model), dtype=np.float32))
    return e


@pytest.fixture(scope="module")
def tiny():
    e = _engine(TINY_W)
    yield e
    e.close()


@pytest.fixture(scope="module")
def large():
    e = _engine(LARGE_W)
    yield e
    e.close()


def _prompt(e):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def _both(e, B, n_new=6):
    """[(step logits of STEP_TOKENS positions, greedy tokens, sum_logprob)] for dec_red_swizzle = 1, 0 at B rows."""
    outs = []
    try:
        for on in (1, 0):
            e.set_option("dec_red_swizzle", on)
            e.decode_reset(B)
            lg = [e.decode_step([(7 + 13 * t + 29 * b) % 900 + 10 for b in range(B)]).copy() for t in range(STEP_TOKENS)]
            r = e.generate([_prompt(e)] * B, e.gen_opts(n_new, False, suppress_eot=True))
            outs.append((lg, r.tokens, r.sum_logprob.copy()))
    finally:
        e.set_option("dec_red_swizzle", 1)
    return outs


def _assert_identical(outs, what):
    (lg1, tok1, lp1), (lg0, tok0, lp0) = outs
    for t, (a, b) in enumerate(zip(lg1, lg0)):
        assert np.isfinite(a).all() and a.any(), (what, t)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, t, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    assert tok1 == tok0, what
    assert np.array_equal(lp1, lp0), what


@pytest.mark.parametrize("B", [1, 20, 32, 33, 64, 97, 128])
def test_tiny_width_logits_and_tokens_are_bit_identical(tiny, B):
    _assert_identical(_both(tiny, B), ("tiny", B))


def test_large_width_narrow_fc1_blocks_are_bit_identical_at_32_rows(large):
    _assert_identical(_both(large, 32), ("large", 32))


@pytest.mark.parametrize("which,B", [("tiny", 32), ("tiny", 64), ("tiny", 97), ("large", 32)])
def test_vocabulary_ragged_last_block_is_bit_identical(tiny, large, which, B):
    """The last n-block holds 25 (51 865) or 26 (51 866) columns: its last cell takes the column-by-column store.  Rows <= 64 run
    the persistent vocabulary kernel, 97 rows the generic kernel's ragged tail."""
    e = tiny if which == "tiny" else large
    V = e.dims.vocab
    assert V % 32 in (25, 26)
    (lg1, _, _), (lg0, _, _) = _both(e, B, n_new=1)
    tail = V - V % 32
    for a, b in zip(lg1, lg0):
        assert a.shape == (B, V)
        assert a[:, tail:].any() and np.isfinite(a[:, tail:]).all()
        assert np.array_equal(a[:, tail:].view(np.uint32), b[:, tail:].view(np.uint32)), (which, B)
        assert np.array_equal(a[:, tail - 32:tail].view(np.uint32), b[:, tail - 32:tail].view(np.uint32)), (which, B)


def test_beam_search_at_40_rows_gives_equal_tokens(tiny):
    e = tiny
    beams = []
    try:
        for on in (1, 0):
            e.set_option("dec_red_swizzle", on)
            r = e.generate_beam([_prompt(e)] * 8, 5, e.gen_opts(8, False))
            beams.append((r.tokens, r.sum_logprob.copy()))
    finally:
        e.set_option("dec_red_swizzle", 1)
    assert all(len(t) > 0 for t in beams[0][0])
    assert beams[0][0] == beams[1][0]
    assert np.array_equal(beams[0][1], beams[1][1])
