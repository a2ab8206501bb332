"""The geometry sweep's table (test infrastructure): ONE deterministic list of model shapes / batch sizes / windows that
tests/test_gpu_geometry_sweep.py runs on the GPU against the oracle and tests/test_geometry_table_host.py checks on the CPU
(limits of include/ttasr.h, coverage of the dispatch thresholds), plus the oracle side of a case.

Which kernel a launch becomes is arithmetic on the shape (kernels_skinny.hip launch_gemm_skinny / gemm_skinny_ksplit /
launch_gemm_vocab, engine_sched.hip gemm<T>, kernels_attn.hip launch_cross_attn_decode), so the axes are the quantities those
predicates read: head count (d = 64 H), ffn_dim, decode rows, vocabulary size, live (row, head) items, n_mels, windows.
Every model has 2 + 2 layers: the second layer's first LayerNorm is the consumer of the first layer's fc2 slabs."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import SpecialTokens, WhisperDims

SHORT_CTX = 94          # model window of the swept shapes: not a multiple of 64, so B * T has ragged last tiles
XATTN_CTX = 150         # cross-attention cases: two 64-frame slices stay possible below 256 items (cross_attn_splits)
SMALL_VOCAB = 531       # not a multiple of 32: the last n-block of the vocabulary projection is partial
ROWS_VOCAB = 8219       # >= 8192 (the persistent vocabulary kernel's range), last n-block partial
TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}


@dataclass(frozen=True)
class Case:
    axis: str
    dims: WhisperDims
    compute: str            # "f32" | "bf16" | "f16"
    batch: int              # rows of the decode batch
    beam: int = 0           # > 0: generate_beam over batch // beam clips (rows of a clip share its cross-KV)
    audio_ctx: int = 0      # > 0: ttasr_set_audio_ctx window on the model's n_audio_ctx positions

    @property
    def n_clips(self) -> int:
        return self.batch // self.beam if self.beam else self.batch

    @property
    def window(self) -> int:
        return self.audio_ctx or self.dims.n_audio_ctx

    @property
    def id(self) -> str:
        d = self.dims
        s = f"{self.axis}-H{d.n_heads}d{d.d_model}f{d.ffn_dim}-m{d.n_mels}-T{d.n_audio_ctx}-V{d.vocab}-t{d.n_text_ctx}-B{self.batch}"
        if self.beam:
            s += f"-beam{self.beam}"
        if self.audio_ctx:
            s += f"-w{self.audio_ctx}"
        return f"{s}-{self.compute}"


def _dims(H: int, ffn: int, *, mels: int = 80, T: int = SHORT_CTX, vocab: int = SMALL_VOCAB, text: int = 32) -> WhisperDims:
    return WhisperDims(f"sweep-h{H}", mels, T, 64 * H, H, ffn, 2, 2, vocab, text)


BASE2 = WhisperDims("base-2layer", 80, 1500, 512, 8, 2048, 2, 2, 51865)
MEDIUM2 = WhisperDims("medium-2layer", 80, 1500, 1024, 16, 4096, 2, 2, 51865)
PUBLISHED = (BASE2, MEDIUM2)


def head_axis_ffn(H: int) -> int:
    """ffn_dim of head count H: cycles through 4 d, an odd multiple of 64, 64 itself and 5120 (20-row layout on fc1); the shift
    by H // 4 makes every fourth head count (the fp16 / f32 subset) see all four kinds too."""
    return (4 * 64 * H, 64 * (2 * H + 1), 64, 5120)[(H + H // 4) % 4]


ROW_BATCHES = (1, 31, 32, 33, 64, 65, 96, 97, 128)
ROW_HEADS = (6, 8, 16)                                   # tiny, base, medium widths
VOCAB_EDGES = (8191, 8192, 8193, 10240, 51200, 53248)
XATTN_PAIRS = ((51, 5), (32, 8), (43, 6), (73, 7), (64, 8), (27, 19))      # (B, H): 255, 256, 258, 511, 512, 513 items
# the same products with rows that share a clip: (clips, beam, H).  258 = 43 x 6 has no beam in 2..7 dividing 43, so the
# product is kept with 3 heads; 73 is prime and 511 = 7 x 73 leaves only beam 1 (one row per clip: the shared-clip kernel
# does not apply, the beam bookkeeping still does)
XATTN_BEAMS = ((17, 3, 5), (8, 4, 8), (43, 2, 3), (73, 1, 7), (16, 4, 8), (9, 3, 19))
MEL_TEXT = ((8, 17), (24, 448), (80, 32), (128, 32))     # (n_mels, n_text_ctx)
WINDOWS = (4, 62, 64, 66, 1498)


def build_table() -> List[Case]:
    t: List[Case] = []
    for dims in PUBLISHED:
        for ct in ("f32", "bf16", "f16"):
            t.append(Case("published", dims, ct, 2))
    for H in range(1, 21):
        for ct in ("bf16", "f16", "f32"):
            if ct == "bf16" or H % 4 == 0:
                t.append(Case("heads", _dims(H, head_axis_ffn(H)), ct, 3))
    for H in ROW_HEADS:
        for B in ROW_BATCHES:
            for ct in ("bf16", "f16") if H == 16 else ("bf16",):
                t.append(Case("rows", _dims(H, 256 * H, vocab=ROWS_VOCAB), ct, B))
    for V in VOCAB_EDGES:
        for ct in ("bf16", "f16", "f32"):
            t.append(Case("vocab", _dims(2, 256, vocab=V), ct, 3))
    for B, H in XATTN_PAIRS:
        for ct in ("bf16", "f16", "f32"):
            t.append(Case("xattn", _dims(H, 256 * H, T=XATTN_CTX), ct, B))
    for A, beam, H in XATTN_BEAMS:
        t.append(Case("xattn-beam", _dims(H, 256 * H, T=XATTN_CTX), "f32", A * beam, beam=beam))
    for mels, text in MEL_TEXT:
        t.append(Case("mel-text", _dims(2, 256, mels=mels, text=text), "f32", 3))
    for w in WINDOWS:
        for ct in ("bf16", "f16"):
            t.append(Case("window", BASE2, ct, 2, audio_ctx=w))
    return t


TABLE: List[Case] = build_table()


# ---- the oracle side of a case --------------------------------------------------------------------------------------------
def clips_of(case: Case) -> List[np.ndarray]:
    n = case.window * 320
    return [synth.noise_clip(i, n) if i % 2 == 0 else synth.tonal_clip(i, n) for i in range(case.n_clips)]


def prompt_of(st: SpecialTokens) -> List[int]:
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def step_tokens(case: Case) -> List[List[int]]:
    """Tokens fed at each decode step, one per row: the prompt, then two text tokens that differ from row to row."""
    st = SpecialTokens.for_vocab(case.dims.vocab)
    B = case.batch
    steps = [[t] * B for t in prompt_of(st)]
    steps.append([(17 + 3 * b) % st.eot for b in range(B)])
    steps.append([(st.eot - 1 - 5 * b) % st.eot for b in range(B)])
    return steps


def oracle_weights(case: Case, sd: Dict[str, np.ndarray]):
    return R.to_torch(sd, round_bf16=case.compute == "bf16", round_f16=case.compute == "f16")


@dataclass
class Reference:
    mel: np.ndarray
    enc: torch.Tensor
    logits: List[np.ndarray]


def reference(case: Case, W, round_activations: Optional[torch.dtype] = None, clips=None, chunk: int = 4) -> Reference:
    """mel -> encoder -> per-step logits of `case` by the oracle on weights W.  round_activations: the 16-bit storage type whose
    rounding R.activation_rounding applies around every linear layer (the sensitivity run)."""
    d = case.dims
    rd = R.Dims(**d.as_dict())
    clips = clips_of(case) if clips is None else clips
    n = case.window * 320
    mel = np.stack([R.log_mel(c, d.n_mels, n_samples=n) for c in clips])
    with R.activation_rounding(round_activations):
        step = chunk if case.window > 400 else len(mel)
        enc = torch.cat([R.encoder_forward(torch.from_numpy(mel[i:i + step]), W, rd) for i in range(0, len(mel), step)], dim=0)
        xkv = R.cross_kv(enc, W, rd)
        cache = R.SelfCache.empty(rd.dec_layers)
        logits = [R.decoder_forward(torch.tensor(t, dtype=torch.long)[:, None], cache, xkv, W, rd)[:, 0].numpy()
                  for t in step_tokens(case)] if not case.beam else []
    return Reference(mel, enc, logits)
