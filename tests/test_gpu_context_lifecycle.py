"""GPU: the life of a context's side resources (csrc/owned.hpp).  A fresh context touches every lazily created block, pinned twin,
event and the session's state once - VAD, float and wire streams, segmentation, ingest (PCM and FLAC), the alignment block
(allocated by the probe, regrown by the batched alignment, then read again by the probe), a beam session with prompt prefill and
language detection - and is closed; then a second context does the same in the same process.  Every call succeeds, the probe
reads the same bits from the regrown block, and the second context computes what the first did."""
import os

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, Session

pytestmark = pytest.mark.gpu

PD = PRESETS["micro"]
HEADS = [(0, 0), (1, 1)]


def _lifecycle(golden_dir):
    rng = np.random.default_rng(20)
    e = Engine(PD, COMPUTE_F32, 4)
    e.load_weights(synth.iter_weights(PD))
    st, d, H = e.special, PD.d_model, PD.n_heads
    out = {}
    # voice activity: the scratch block for one recording and the pinned staging; then the streams' table and wire pools
    e.load_vad(vad.synth_silero_weights())
    pcm513 = (rng.standard_normal(513) * 0.1).astype(np.float32)
    out["vad"] = e.vad_probs([pcm513])[0]
    assert out["vad"].shape == (2,) and np.all(np.isfinite(out["vad"]))
    sid = e.vad_stream_open()
    assert len(e.vad_stream_push([sid], [(rng.standard_normal(600) * 0.1).astype(np.float32)])[0]) == 1
    e.vad_stream_close(sid)
    sid = e.vad_stream_open((16000, 1, _lib.PCM_S16, None))
    s16 = (rng.standard_normal(600) * 3000).astype(np.int16)
    w_pcm, w_probs = e.vad_stream_push_wire([sid], [s16.tobytes()])
    assert len(w_pcm[0]) == 600 and len(w_probs[0]) == 1
    e.vad_stream_close(sid)
    # segmentation: one recording of one chunk
    e.load_segmentation(vad.synth_pyannet_weights())
    seg = e.segmentation_scores([(rng.standard_normal(80000) * 0.1).astype(np.float32)])[0]
    assert len(seg) == e.lib.ttasr_seg_frames(80000) and np.all(np.isfinite(seg))
    # ingest: the chunk slots and a tap table (8 kHz), then the FLAC scratch
    got = e.ingest([(rng.standard_normal(100) * 3000).astype(np.int16).tobytes()], [8000], [1], [_lib.PCM_S16])[0]
    assert len(got) == 200 and np.all(np.isfinite(got))
    flac = open(os.path.join(golden_dir, "flac_rfc9639_example1.flac"), "rb").read()
    info = _lib.flac_probe(flac)
    got = e.ingest([flac], [info.rate], [info.channels], [_lib.PCM_FLAC])[0]
    assert len(got) == e.lib.ttasr_ingest_len(info.rate, info.samples) and np.all(np.isfinite(got))
    # the alignment block: allocated by the probe, regrown by the batched alignment, read again by the probe
    e.log_mel([synth.noise_clip(0)[:PD.n_frames * 160], synth.tonal_clip(1)[:PD.n_frames * 160]], want_output=False)
    e.encode(2)
    q = rng.standard_normal((2, d)).astype(np.float32)
    head_pair = [0] + [-1] * (H - 1)
    out["probe"] = e.align_attn_probe(0, q, [2], [1], head_pair)
    seqs = [[st.sot, st.transcribe, st.no_timestamps, 7 + i, st.eot] for i in range(2)]
    r = e.align_batch([0, 1], seqs, [2, 2], [2 * PD.n_audio_ctx] * 2, HEADS)
    assert all(len(s) == 2 for s in r.start_frames) and all(np.all(np.isfinite(lp)) for lp in r.logprobs)
    again = e.align_attn_probe(0, q, [2], [1], head_pair)
    assert np.array_equal(again[0], out["probe"][0]) and np.array_equal(again[1], out["probe"][1])
    assert np.all(np.isfinite(out["probe"][0])) and np.allclose(out["probe"][1].sum(-1), 1.0, atol=1e-4)
    # a beam session with prompt prefill, armed for language detection: its pinned blocks, events and the beam exchange block
    tail = [st.transcribe, st.no_timestamps]
    clip = synth.burst_clip(2)[:PD.n_frames * 160]
    with e.session(e.gen_opts(4, False, suppress_eot=True, check_interval=1), 4, beam=2, patience=1.0, detect_language=True,
                   prefill=2) as s:
        ids = s.submit([clip], [[st.sot, Session.DETECT] + tail], [3])
        res = s.drain()
        assert [x.id for x in res] == ids and len(res[0].tokens) == 3 and res[0].language is not None
        ids = s.submit([clip], [[st.sot, e.language_span()[0]] + tail], [3])   # three prefillable positions: an admission pass
        res = s.drain()
        assert [x.id for x in res] == ids and len(res[0].tokens) == 3
    e.close()
    return out


def test_every_side_resource_twice_in_one_process(golden_dir):
    first = _lifecycle(golden_dir)
    second = _lifecycle(golden_dir)
    assert np.array_equal(first["vad"], second["vad"])
    assert np.array_equal(first["probe"][0], second["probe"][0]) and np.array_equal(first["probe"][1], second["probe"][1])
