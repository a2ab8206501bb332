"""GPU: the decode-step kernels give the bits they gave before their argument lists were reordered.

The skinny GEMM, the row LayerNorm and the pipelined cross-attention of the decode chain take the values that their first load
batch needs as leading, preloaded arguments and fetch the rest under those loads (common.hpp sgpr_pin); self-attention and select
run between them on the same buffers.  That moves arguments, not arithmetic: every logit and every token must be what the parent commit produced.  tests/golden/decode_entry_crc.json holds the
CRC-32 of the step-API logits (f32 bytes of all 20 positions) and of the greedy tokens, recorded on the PARENT commit with
    TTASR_ENTRY_CRC_WRITE=1 (or =<path of the json to write>) python -m pytest tests/test_gpu_kernel_entry.py -m gpu
and the tests assert equality.

Shapes: 2 decoder layers, ffn = 4 d, vocab 1024, n_text_ctx 32, n_audio_ctx 96 (no multiple of 32; 1500 in one case), d = 128
and d = 1280; 20 positions (the KV page boundary at 16 is crossed); B in {1, 5, 32, 33, 128}; bf16, f16, f32.
K-split options (16-bit modes; the f32 mode runs the generic GEMMs and has no K split): the slab count the LayerNorm sees is the
slice count of the out-proj / fc2 GEMM, the largest divisor of K / 64 that the option allows - 0 (unsplit), 2, 4, 5, 8 (fc2), 10
(out-proj), 16 (fc2) at d = 1280 and 0, 2, 4, 8 at d = 128.  ONE slab cannot be reached through the engine (a GEMM is split into
>= 2 slices or not at all), so that LayerNorm bucket is covered only by its neighbours.  ksplit_qkv / ksplit_q = 1 turn the
slab forms of self- and cross-attention off, 2 and 4 turn them on.  dec_x_lds 0 and 1.
One ragged case (rows in the middle of the batch finish early: the live-row remap of the attention kernels) and one session case
(bf16, d = 128; per-row positions: prompts of different lengths, a second wave admitted into finished rows).
One f32 case per width is also held to the CPU oracle (logits within 1e-3, the f32 invariant of the suite; tokens through
oracle_checks.teacher_forced with tol 1e-3 / margin 2e-3), so a mis-wired argument fails even against a wrongly recorded fixture."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, WhisperDims

from oracle_checks import teacher_forced

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_entry_crc.json")
WRITE = os.environ.get("TTASR_ENTRY_CRC_WRITE", "")
COMPUTE = {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
N_POS, N_PROMPT, N_NEW = 20, 4, 16
MAX_B = 128
BATCHES = (1, 5, 32, 33, 128)
SUPPRESS, BEGIN_SUPPRESS = [1, 2, 7], [5]

# (name, {option: value}); the K-split options are ksplit_out / _q / _qkv / _fc2
OPTIONS = [
    ("auto", {}),
    ("unsplit", dict(ksplit_out=1, ksplit_q=1, ksplit_qkv=1, ksplit_fc2=1)),
    ("ks2", dict(ksplit_out=2, ksplit_q=2, ksplit_qkv=2, ksplit_fc2=2)),
    ("ks4", dict(ksplit_out=4, ksplit_q=4, ksplit_qkv=4, ksplit_fc2=4)),
    ("ks5", dict(ksplit_out=5, ksplit_fc2=5)),
    ("ks8", dict(ksplit_out=8, ksplit_fc2=8, ksplit_qkv=1)),
    ("ks16", dict(ksplit_out=16, ksplit_fc2=16, ksplit_q=1)),
    ("auto_nolds", dict(dec_x_lds=0)),
    ("ks4_nolds", dict(ksplit_out=4, ksplit_q=4, ksplit_qkv=4, ksplit_fc2=4, dec_x_lds=0)),
]
DEFAULTS = dict(ksplit_out=0, ksplit_q=0, ksplit_qkv=0, ksplit_fc2=0, dec_x_lds=1)


def _dims(d, audio_ctx=96):
    return WhisperDims(f"entry-d{d}-a{audio_ctx}", 80, audio_ctx, d, d // 64, 4 * d, 1, 2, 1024, 32)


@functools.lru_cache(maxsize=None)
def _weights(dims):
    return synth.state_dict(dims)


def _encoder_rows(dims, n):
    """Seeded encoder output [n][n_audio_ctx][d] (the encoder is not what this file is about)."""
    g = np.random.Generator(np.random.Philox(key=dims.d_model + dims.n_audio_ctx))
    return g.standard_normal((n, dims.n_audio_ctx, dims.d_model), dtype=np.float32)


def _engine(dims, compute):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(dims, COMPUTE[compute], MAX_B)
    e.load_weights(_weights(dims).items())
    return e


def _step_tokens(B):
    return [[(7 + 13 * t + 29 * b) % 900 + 10 for b in range(B)] for t in range(N_POS)]


def _prompt(st):
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def _opts(e, n_new=N_NEW, check_interval=1 << 20):
    return e.gen_opts(n_new, False, suppress=SUPPRESS + [e.special.sot], begin_suppress=BEGIN_SUPPRESS + [e.special.eot],
                      suppress_eot=True, check_interval=check_interval)


def _crc_tokens(rows):
    flat = np.asarray([len(r) for r in rows] + [t for r in rows for t in r], dtype=np.int32)
    return zlib.crc32(flat.tobytes())


def _run(e, B, opts=None):
    """(CRC of the step-API logits of N_POS positions, CRC of the greedy tokens, logits of every position, tokens) at B rows."""
    for k, v in {**DEFAULTS, **(opts or {})}.items():
        e.set_option(k, v)
    e.decode_reset(B)
    crc, logits = 0, []
    for toks in _step_tokens(B):
        lg = e.decode_step(toks)
        assert np.isfinite(lg).all()
        crc = zlib.crc32(np.ascontiguousarray(lg, dtype=np.float32).tobytes(), crc)
        logits.append(lg)
    res = e.generate([_prompt(e.special)] * B, _opts(e))
    assert all(len(t) == N_NEW for t in res.tokens)
    return crc, _crc_tokens(res.tokens), logits, res.tokens


class _Book:
    """The fixture: checked key by key, or (TTASR_ENTRY_CRC_WRITE) extended and written back."""

    def __init__(self):
        self.path = FIXTURE if WRITE in ("", "1") else WRITE
        self.data = {}
        if os.path.exists(self.path):
            with open(self.path) as f:
                self.data = json.load(f)

    def hold(self, key, value):
        if WRITE:
            self.data[key] = int(value)
            with open(self.path, "w") as f:
                json.dump(self.data, f, indent=0, sort_keys=True)
                f.write("\n")
            return
        assert key in self.data, f"{key}: not in {self.path} (record it on the parent commit)"
        assert int(value) == self.data[key], f"{key}: CRC-32 {int(value)} != recorded {self.data[key]}"


@pytest.fixture(scope="module")
def book():
    return _Book()


def _step_cases():
    """(d, compute, option set): every option set in the 16-bit modes; the f32 mode has no K split and no LDS tile."""
    return [(d, c, o) for d in (128, 1280) for c in ("bf16", "f16", "f32") for o in (OPTIONS if c != "f32" else OPTIONS[:1])]


@pytest.mark.parametrize("d,compute,option", _step_cases(), ids=[f"d{d}-{c}-{o[0]}" for d, c, o in _step_cases()])
def test_step_logits_and_greedy_tokens_are_the_parents(book, d, compute, option):
    """Every batch size at the automatic options, 5 and 33 rows at every other option set."""
    dims = _dims(d)
    name, opts = option
    e = _engine(dims, compute)
    try:
        e.set_encoder_output(_encoder_rows(dims, MAX_B))
        for B in (BATCHES if name == "auto" else (5, 33)):
            lc, tc, _, _ = _run(e, B, opts)
            print(f"d{d} {compute} B{B} {name}: logits {lc} tokens {tc}")
            book.hold(f"d{d}/{compute}/B{B}/{name}/logits", lc)
            book.hold(f"d{d}/{compute}/B{B}/{name}/tokens", tc)
    finally:
        e.close()


@pytest.mark.parametrize("compute", ["bf16", "f32"])
def test_full_audio_context(book, compute):
    dims = _dims(128, audio_ctx=1500)
    e = _engine(dims, compute)
    try:
        e.set_encoder_output(_encoder_rows(dims, 33))
        for B, (name, opts) in [(5, OPTIONS[0]), (33, OPTIONS[0]), (33, OPTIONS[3])]:
            lc, tc, _, _ = _run(e, B, opts)
            book.hold(f"d128a1500/{compute}/B{B}/{name}/logits", lc)
            book.hold(f"d128a1500/{compute}/B{B}/{name}/tokens", tc)
    finally:
        e.close()


@pytest.mark.parametrize("compute", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("d", [128, 1280])
def test_rows_that_finish_in_the_middle_of_the_batch(book, d, compute):
    dims = _dims(d)
    e = _engine(dims, compute)
    try:
        e.set_encoder_output(_encoder_rows(dims, MAX_B))
        for k, v in DEFAULTS.items():
            e.set_option(k, v)
        for B in (32, 33):
            caps = np.full(B, N_NEW, dtype=np.int32)
            caps[3:10] = 2
            caps[17] = 1
            caps[20:23] = 9
            res = e.generate([_prompt(e.special)] * B, _opts(e), row_max_new=caps)
            assert [len(t) for t in res.tokens] == caps.tolist()
            book.hold(f"d{d}/{compute}/B{B}/ragged/tokens", _crc_tokens(res.tokens))
            book.hold(f"d{d}/{compute}/B{B}/ragged/logprob", zlib.crc32(np.ascontiguousarray(res.sum_logprob, dtype=np.float32).tobytes()))
    finally:
        e.close()


def test_session_with_per_row_positions(book, compute="bf16"):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    d = 128
    dims = _dims(d)
    e = Engine(dims, COMPUTE[compute], 8)
    try:
        e.load_weights(_weights(dims).items())
        st = e.special
        n = 14                                           # more clips than rows: later clips are admitted into finished rows
        clips = [synth.noise_clip(40 + i, dims.n_frames * 160 - 37 * i) for i in range(n)]
        prompts = [_prompt(st)[:3 + (i % 2)] for i in range(n)]     # two prompt lengths: the rows' positions differ from the start
        caps = [3 + (5 * i) % (N_NEW - 2) for i in range(n)]
        with e.session(_opts(e, check_interval=1), max(len(p) for p in prompts)) as s:
            ids = s.submit(clips[:9], prompts[:9], caps[:9])
            got = s.poll()
            ids += s.submit(clips[9:], prompts[9:], caps[9:])
            got += s.drain()
        by_id = {r.id: r for r in got}
        rows = [by_id[i].tokens for i in ids]
        assert [len(r) for r in rows] == caps
        book.hold(f"d{d}/{compute}/session/tokens", _crc_tokens(rows))
        lp = np.asarray([by_id[i].sum_logprob for i in ids], dtype=np.float32)
        book.hold(f"d{d}/{compute}/session/logprob", zlib.crc32(lp.tobytes()))
    finally:
        e.close()


@pytest.mark.parametrize("d", [128, 1280])
def test_f32_against_the_oracle(d):
    dims = _dims(d)
    rd = R.Dims(**dims.as_dict())
    B = 5
    e = _engine(dims, "f32")
    try:
        enc = _encoder_rows(dims, MAX_B)
        e.set_encoder_output(enc)
        _, _, logits, tokens = _run(e, B)
        st = e.special
    finally:
        e.close()
    W = R.to_torch(_weights(dims))
    enc_ref = torch.from_numpy(enc[:B])
    xkv = R.cross_kv(enc_ref, W, rd)
    cache = R.SelfCache.empty(rd.dec_layers)
    worst = 0.0
    for toks, lg in zip(_step_tokens(B), logits):
        want = R.decoder_forward(torch.tensor(toks, dtype=torch.long)[:, None], cache, xkv, W, rd)[:, 0].numpy()
        worst = max(worst, float(np.abs(lg - want).max()))
    print(f"d{d}: worst f32 logit error {worst:.3g}")
    assert worst < 1e-3, worst
    rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin, suppress=SUPPRESS + [st.sot],
                    begin_suppress=BEGIN_SUPPRESS + [st.eot], timestamps=False)
    rules.suppress_eot = True
    g = teacher_forced(tokens, _prompt(st), enc_ref, W, rd, rules, tol=1e-3, margin=2e-3)
    assert g.n_steps == B * N_NEW and g.n_clear >= 0.6 * g.n_steps, g
