"""GPU: the diarization pipeline on the device - segmentation network, masks on the host, speaker-embedding network, clustering
and reconstruction - on about 30 s of two synthetic voices: its turns are the turns of the same host pipeline fed the float64
references' probabilities and embeddings (tests/diarization_cases.py; test_diarization_host.py shows that the reference finds
two speakers and that none of its decisions lies within the tolerances of its threshold)."""
import numpy as np
import pytest

import diarization_cases as DC
import xvector_cases as XC
from taiwan_tongues_asr_ce_amd import diarization, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine
from taiwan_tongues_asr_ce_amd.model import WhisperModel

pytestmark = pytest.mark.gpu


def test_device_pipeline_gives_the_reference_pipelines_turns():
    ref = DC.reference_pipeline()
    sig = DC.two_voice_signal()
    e = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))
    e.load_segmentation(vad.synth_pyannet_weights(DC.SEG_SEED, DC.SEG_CLASSES))
    e.load_speaker_embedding(diarization.synth_xvector_weights(DC.SPK_SEED, DC.SPK_DIM))
    # the two device calls, by hand: every intermediate against its reference
    probs = e.segmentation_scores([sig], return_chunks=True)[1][0]
    p_err = float(np.abs(probs - ref["probs"]).max())
    masks = diarization.local_speaker_masks(probs, DC.ONSET, min_frames=DC.MIN_FRAMES)
    emb = e.speaker_embeddings([sig], [masks])[0]
    e_err = XC.rel(emb, ref["emb"]) if np.array_equal(masks, ref["masks"]) else float("nan")
    print(f"diarization: device probabilities vs float64 {p_err:.3e} (tolerance {DC.PROB_TOL:.2e}), embeddings {e_err:.3e} "
          f"(tolerance {XC.EMB_TOL:.2e}); {int((masks.sum(axis=2) > 0).sum())} masks with frames")
    assert p_err <= DC.PROB_TOL
    assert np.array_equal(masks, ref["masks"])
    assert e_err <= XC.EMB_TOL
    turns = diarization.diarize_from(probs, emb, masks, len(sig), threshold=DC.THRESHOLD, onset=DC.ONSET)
    assert np.array_equal(DC.turns_array(turns), ref["turns"])
    assert {t.speaker for t in turns} == {"SPEAKER_00", "SPEAKER_01"} and turns[0].speaker == "SPEAKER_00"
    # the same through the model's surface
    m = WhisperModel.__new__(WhisperModel)
    m.engine = e
    m._diarization = True
    assert m.diarize(sig, threshold=DC.THRESHOLD, onset=DC.ONSET, min_frames=DC.MIN_FRAMES) == turns
    one = m.diarize(sig, num_speakers=1, onset=DC.ONSET, min_frames=DC.MIN_FRAMES)
    assert {t.speaker for t in one} == {"SPEAKER_00"} and len(one) >= 1
    assert m.diarize(np.zeros(0, np.float32)) == []
    e.close()
