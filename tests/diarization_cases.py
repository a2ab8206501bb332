"""TEST infrastructure: the signal, the networks and the parameters of the diarization pipeline's tests, and the float64 reference
of the whole pipeline - tests/pyannet_reference.py's probabilities, the masks, tests/xvector_reference.py's embeddings,
diarization.diarize_from - shared by the CPU test (which checks the conditions the GPU test rests on) and the GPU test (about six seconds of CPU, once
per process).

The networks carry synthetic weights, so neither is a detector of anything; the signal only has to make them move.  The seed of the
segmentation weights, ONSET and THRESHOLD are chosen so that the reference finds two speakers and none of its decisions lies
within the GPU tolerances of its threshold (test_diarization_host.py measures every margin named here):

* activity against the onset: 51 chunks x 293 frames x 3 local speakers are 44 829 decisions.  PROB_TOL, the tolerance of a
  probability, follows the rule of tests/xvector_cases.py: 16 x the distance of the float32 run of the segmentation reference
  from its float64 run on this signal (F32_PROB).  The probabilities of a network with random weights are spread in one broad
  hump, so 44 829 of them leave a gap of 2 PROB_TOL only out in its tail: ONSET = 0.647 stands in a gap of +- 1.5e-4, where
  0.9 % of the decisions are "active".  That is little speech, and enough for 47 usable embeddings and two clusters;
* cluster distance against the cut: THRESHOLD = 0.604 stands in the middle of the 0.125 wide gap between the last two merge
  heights of the tree (0.54 and 0.67), and the embeddings' tolerance (3.84e-4 of their largest entry) moves a distance between
  unit vectors by at most 7.3e-3;
* behind them: the nearest-centroid assignment, the rounding of the speaker count and the choice of the most active clusters
  have margins of their own, measured in the same test."""
from __future__ import annotations

import numpy as np

SR = 16000
SEG_SEED, SEG_CLASSES, SPK_SEED, SPK_DIM = 1, 3, 0, 192
ONSET, THRESHOLD, MIN_FRAMES = 0.647, 0.604, 10
F32_PROB = 9.0e-6              # measured on the CPU (8.91e-6), rounded up: float32 against float64 segmentation reference on the signal
PROB_TOL = 16 * F32_PROB


def voice(f0: float, seconds: float, seed: int, tilt: float) -> np.ndarray:
    """A harmonic complex: 24 harmonics of f0 with amplitudes h ** -tilt, a slow vibrato and a 4 Hz syllable envelope."""
    rng = np.random.default_rng([0xD1A, seed])
    t = np.arange(int(seconds * SR)) / SR
    phase = 2 * np.pi * f0 * (t + 0.003 * np.sin(2 * np.pi * 5.0 * t))
    x = sum((h ** -tilt) * np.sin(h * phase + rng.uniform(0, 2 * np.pi)) for h in range(1, 25) if h * f0 < 7000)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, 2 * np.pi))
    return 0.1 * x * env / np.abs(x).max()


def two_voice_signal() -> np.ndarray:
    """About 30 s: voice A (110 Hz) and voice B (210 Hz) alternating, 0.8 s of near-silence between the turns."""
    rng = np.random.default_rng(0xD1A2)
    parts = []
    for i, (who, dur) in enumerate(((0, 3.2), (1, 2.6), (0, 2.9), (1, 3.4), (0, 2.2), (1, 3.0), (0, 3.1), (1, 2.8))):
        parts.append(voice(110.0 if who == 0 else 210.0, dur, i, 1.0 if who == 0 else 1.6))
        parts.append(np.zeros(int(0.8 * SR)))
    x = np.concatenate(parts)
    return (x + 1e-4 * rng.standard_normal(len(x))).astype(np.float32)


def reference_pipeline():
    """The float64 reference of the pipeline on two_voice_signal(): dict(probs [K, 293, C], masks [K, C, 293], emb [K, C, D],
    turns as a float64 array [n, 3] of (start, end, speaker number)).  Computed once per process."""
    if not _REF:
        from pyannet_reference import cached_scores
        from xvector_reference import cached_embeddings
        from taiwan_tongues_asr_ce_amd import diarization
        sig = two_voice_signal()
        probs = cached_scores(SEG_SEED, "two voices", sig, classes=SEG_CLASSES)[1]
        masks = diarization.local_speaker_masks(probs, ONSET, min_frames=MIN_FRAMES)
        emb = cached_embeddings(SPK_SEED, SPK_DIM, "two voices", sig, masks)[0]
        turns = diarization.diarize_from(probs, emb, masks, len(sig), threshold=THRESHOLD, onset=ONSET)   # min_frames acts in the masks above
        _REF.update(probs=np.asarray(probs), masks=masks, emb=np.asarray(emb), turns=turns_array(turns))
    return _REF


_REF: dict = {}


def turns_array(turns) -> np.ndarray:
    return np.asarray([[t.start, t.end, int(str(t.speaker).split("_")[-1])] for t in turns], dtype=np.float64).reshape(-1, 3)
