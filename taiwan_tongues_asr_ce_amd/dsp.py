"""Audio optimisation ("dspMode" of the reference service's task API): the parameters of the device enhancement call
(Engine.enhance, ttasr_enhance: denoise, high-pass, level; length-preserving) and the mapping from the `dsp_mode` keyword of the
file-level surfaces.  The definition is this project's own - the product publishes none - and its effect on CER is unmeasured
(DESIGN.md section 4.35).  Off by default everywhere.

One rule on every surface: enhancement runs once, where the call's audio has become float32 mono 16 kHz and before a session
opens, and every consumer of that call - VAD, segmentation, speaker embedding, log-mel, alignment - sees the enhanced samples.
Live utterances (transcribe_stream, BatchedWhisperASR) are refused: they need a causal, stateful noise tracker, which is out of
scope."""
from __future__ import annotations

import math
from dataclasses import dataclass, fields, replace
from typing import Optional

DSP_DENOISE, DSP_HIGHPASS, DSP_LEVEL = 1, 2, 4   # TTASR_DSP_* of include/ttasr.h


@dataclass(frozen=True)
class DspParams:
    """What ttasr_enhance takes.  The defaults are the product's dspMode = 1: all three stages."""
    denoise: bool = True
    highpass: bool = True
    level: bool = True
    strength_db: float = 12.0                     # [0, 40]: the spectral gain never falls below 10^(-strength_db / 20)
    oversubtract: float = 3.0                     # (0, 16]: the noise floor is this many times the tracked minimum
    peak_target: float = 10.0 ** (-1.0 / 20.0)    # (0, 1]: the level stage brings the peak here (-1 dBFS) ...
    max_gain: float = 10.0                        # >= 1: ... with at most this gain

    @property
    def flags(self) -> int:
        return (DSP_DENOISE if self.denoise else 0) | (DSP_HIGHPASS if self.highpass else 0) | (DSP_LEVEL if self.level else 0)

    def check(self) -> "DspParams":
        """ValueError for what the library would refuse."""
        if self.flags == 0:
            raise ValueError("dsp_mode: at least one of denoise, highpass and level must be on (use dsp_mode=0 to turn the stage off)")
        for name in ("strength_db", "oversubtract", "peak_target", "max_gain"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"dsp_mode: {name} must be a finite number, got {v!r}")
        if not 0.0 <= self.strength_db <= 40.0:
            raise ValueError(f"dsp_mode: strength_db {self.strength_db} outside [0, 40]")
        if not 0.0 < self.oversubtract <= 16.0:
            raise ValueError(f"dsp_mode: oversubtract {self.oversubtract} outside (0, 16]")
        if not 0.0 < self.peak_target <= 1.0:
            raise ValueError(f"dsp_mode: peak_target {self.peak_target} outside (0, 1]")
        if self.max_gain < 1.0:
            raise ValueError(f"dsp_mode: max_gain {self.max_gain} is below 1")
        return self


def resolve(dsp_mode) -> Optional[DspParams]:
    """The `dsp_mode` keyword -> None (off) or checked DspParams.  None / 0 / False: off; 1 / True: all three stages (the product's
    1); a DspParams or a dict of its fields: taken as given."""
    if dsp_mode is None or dsp_mode is False or (isinstance(dsp_mode, int) and not isinstance(dsp_mode, bool) and dsp_mode == 0):
        return None
    if dsp_mode is True or (isinstance(dsp_mode, int) and dsp_mode == 1):
        return DspParams()
    if isinstance(dsp_mode, DspParams):
        return dsp_mode.check()
    if isinstance(dsp_mode, dict):
        known = {f.name for f in fields(DspParams)}
        unknown = sorted(set(dsp_mode) - known)
        if unknown:
            raise ValueError(f"dsp_mode: unknown field(s) {unknown}; DspParams has {sorted(known)}")
        return replace(DspParams(), **dsp_mode).check()
    raise ValueError(f"dsp_mode must be None, 0, 1, a DspParams or a dict of its fields, got {dsp_mode!r}")


def refuse_streaming(dsp_mode, what: str) -> None:
    """The live surfaces: ValueError before any device work when dsp_mode asks for enhancement."""
    if resolve(dsp_mode) is not None:
        raise ValueError(f"{what} does not take dsp_mode: a live utterance needs a causal, stateful noise tracker, which is out of "
                         "scope; the enhancement reads the whole recording (use it on the file-level surfaces)")
