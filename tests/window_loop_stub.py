"""TEST infrastructure: a scripted engine double for WhisperModel's host-side window loop (the style of _CtxEngine in
test_cabi_and_host.py).  It records every feature call - (seek, frames) per window, with the cut exactly as the loop passed
it - and answers every search with the tokens its script holds for the window that is resident; `patch_alignment` makes
alignment.find_alignment return the script's words for that window.  Never imported by the product."""
from __future__ import annotations

import types
from typing import Callable, Dict, List, Optional

import numpy as np

from taiwan_tongues_asr_ce_amd import alignment
from taiwan_tongues_asr_ce_amd.config import PRESETS, SpecialTokens
from taiwan_tongues_asr_ce_amd.engine import GenResult

DIMS = PRESETS["tiny"]
ST = SpecialTokens.for_vocab(DIMS.vocab)
W = DIMS.n_frames            # frames of the model's window (3000)
SILENT = dict(tokens=[ST.eot], lp=-50.0, ns=0.99)   # no_speech above and avg_logprob below their thresholds: the window is skipped


def ts(seconds: float) -> int:
    """The timestamp token of `seconds` into the window (20-ms units)."""
    return ST.timestamp_begin + int(round(seconds / 0.02))


def word(text: str, start: float, end: float, probability: float = 0.9, tokens: int = 1) -> dict:
    """One aligned word as alignment.find_alignment returns it (times relative to the window)."""
    return dict(word=text, tokens=[0] * tokens, start=start, end=end, probability=probability)


class ScriptEngine:
    """script(file_len, seek, frames) -> dict(tokens, lp (sum log-prob), ns, words (optional), sampled (optional: the answer of a
    sampled attempt)) or None for a silent window.  `calls` holds ("max", seeks), ("win", [(seek, frames given or None)]),
    ("prompt", file_len, seek, prompt) and ("opts", suppress) in order."""

    accepts_cut = True

    def __init__(self, dims, compute_type=0, max_batch=1, device=0):
        self.dims, self.special, self.max_batch = dims, SpecialTokens.for_vocab(dims.vocab), max_batch
        self.calls: List[tuple] = []
        self.script: Callable = lambda n, seek, frames: None
        self.resident: List[tuple] = []
        self.decoded: List[tuple] = []

    def load_weights(self, tensors):
        pass

    def close(self):
        pass

    def set_audio_ctx(self, n=0):
        pass

    def log_mel_windows(self, audio, seeks, floor_max=None, want_output=False, want_max=False, **kw):
        assert set(kw) <= ({"n_frames"} if self.accepts_cut else set()), kw
        files = [audio] * len(seeks) if isinstance(audio, np.ndarray) else list(audio)
        if want_max:
            self.calls.append(("max", [int(k) for k in seeks]))
            return None, np.zeros(len(seeks), np.float32)
        cut = kw.get("n_frames")
        assert cut is None or len(cut) == len(seeks)
        self.calls.append(("win", [(int(k), None if cut is None else int(cut[b])) for b, k in enumerate(seeks)]))
        left = [min(self.dims.n_frames, len(a) // 160 - int(k)) for a, k in zip(files, seeks)]
        self.resident = [(len(a), int(k), n if cut is None else min(n, int(cut[b]))) for b, (a, k, n) in enumerate(zip(files, seeks, left))]
        self.decoded.extend((k, n) for _, k, n in self.resident)
        return None, None

    def encode(self, B, want_output=False):
        assert B == len(self.resident)

    def gen_opts(self, max_new_tokens, timestamps, suppress=None, begin_suppress=None, suppress_eot=False, no_speech=True,
                 sot_index=0, max_initial_timestamp_index=50, check_interval=8):
        self.calls.append(("opts", None if suppress is None else list(suppress)))
        return types.SimpleNamespace(max_new_tokens=max_new_tokens)

    def _answer(self, prompts, sampled=False) -> GenResult:
        toks, lps, nss = [], [], []
        for b, p in enumerate(prompts):
            n, seek, frames = self.resident[b]
            self.calls.append(("prompt", n, seek, list(p)))
            r = self.script(n, seek, frames) or SILENT
            if sampled and "sampled" in r:
                r = r["sampled"]
            toks.append(list(r["tokens"])); lps.append(r.get("lp", -1.0)); nss.append(r.get("ns", 0.0))
        return GenResult(toks, np.asarray(lps, np.float32), np.asarray(nss, np.float32))

    def generate(self, prompts, opts):
        return self._answer(prompts)

    def generate_beam(self, prompts, beam, opts, patience=1.0, sot_index=None):
        return self._answer(prompts)

    def generate_sample(self, prompts, best_of, opts, temperature, seed=0):
        return self._answer(prompts, sampled=True)

    # what the tests read back
    def windows(self) -> List[tuple]:
        """(seek, frames decoded) of every window the loop asked features for, in order (lock step: one entry per row)."""
        return list(self.decoded)

    def asked(self) -> List[tuple]:
        """(seek, the cut as the loop passed it or None) of the same windows."""
        return [w for c in self.calls if c[0] == "win" for w in c[1]]

    def prompts(self, n: Optional[int] = None) -> List[tuple]:
        return [(c[2], c[3]) for c in self.calls if c[0] == "prompt" and (n is None or c[1] == n)]


class NoCutEngine(ScriptEngine):
    """The feature call as it was before the cut existed: a loop that passes n_frames to it fails."""
    accepts_cut = False


def make_model(script: Optional[Callable] = None, max_batch: int = 4, cls=ScriptEngine):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=max_batch, _engine_factory=cls)
    if script is not None:
        m.engine.script = script
    return m


def by_seek(table: Dict[int, dict]) -> Callable:
    """A script that answers by the window's seek alone; windows it does not name are silent."""
    return lambda n, seek, frames: table.get(seek)


def patch_alignment(monkeypatch) -> None:
    """alignment.find_alignment -> the words the engine's script holds for the resident window `clip`."""
    def find(engine, tokenizer, special, clip, text_tokens, num_frames, heads, *a, **k):
        n, seek, frames = engine.resident[clip]
        assert num_frames == frames
        r = engine.script(n, seek, frames) or {}
        return [dict(w, tokens=list(w["tokens"])) for w in r.get("words", [])]
    monkeypatch.setattr(alignment, "find_alignment", find)


def run(m, audio, **kw):
    """transcribe with the search that makes one engine call per window (greedy, no fallback ladder) -> (segments, info)."""
    opts = dict(language="zh", beam_size=1, temperature=0.0)
    opts.update(kw)
    segs, info = m.transcribe(audio, **opts)
    return list(segs), info
