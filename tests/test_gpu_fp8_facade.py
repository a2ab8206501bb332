"""GPU: `WhisperModel(cross_kv_fp8=True)` - the lock-step and the continuous form of transcribe_many both decode from the e4m3
cross-KV copy and agree file by file; the flag changes the scores of a model built without it.

The two forms agree under the conditions of the session's contract (include/ttasr.h): prompts forced through decode steps
(option prefill = 0) and exactly G = max_batch / beam files per lock-step pass."""
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import synth

pytestmark = pytest.mark.gpu


def test_transcribe_many_static_equals_continuous_and_differs_from_16bit():
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    kinds = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
    files = [kinds[i % 3](1900 + i)[: (6 + 2 * i) * 16000].astype(np.float32) for i in range(6)]
    kw = dict(language="zh", beam_size=5, temperature=0.0, max_new_tokens=12, no_speech_threshold=None, log_prob_threshold=None,
              compression_ratio_threshold=None)

    def run(model, **extra):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return [segs for segs, _ in model.transcribe_many(files, **kw, **extra)]
    m8 = WhisperModel("synthetic:large-v3-w2", compute_type="bfloat16", max_batch=30, cross_kv_fp8=True)
    try:
        m8.engine.set_option("prefill", 0)
        a = run(m8)
        b = run(m8, continuous=True)
        assert a == b
        assert sum(len(s) for s in a) > 0
    finally:
        m8.close()
    m16 = WhisperModel("synthetic:large-v3-w2", compute_type="bfloat16", max_batch=30)
    try:
        m16.engine.set_option("prefill", 0)
        c = run(m16)
    finally:
        m16.close()
    lp8 = [[s.avg_logprob for s in segs] for segs in a]
    lp16 = [[s.avg_logprob for s in segs] for segs in c]
    print("avg_logprob e4m3", lp8, "16-bit", lp16)
    assert lp8 != lp16
