"""CPU: the host side of the segmentation VAD - the C ABI's declarations, the weight table and its loader, the factory names and
the DevicePyannoteVAD backend on a fake engine."""
import asyncio
import os
import re

import numpy as np
import pytest

import pyannet_reference as R
from taiwan_tongues_asr_ce_amd import _lib, vad, vad_backends

SEG_SYMBOLS = ("ttasr_seg_load_tensor", "ttasr_seg_finalize", "ttasr_seg_classes", "ttasr_seg_chunks", "ttasr_seg_frames", "ttasr_seg_scores")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ttasr.h")


def test_symbols_are_declared_in_the_binding_and_the_header():
    hdr = open(HEADER).read()
    for s in SEG_SYMBOLS:
        assert s in _lib.SYMBOLS and re.search(r"TTASR_API \w+ " + s + r"\(", hdr), s
    assert f"#define TTASR_SEG_GROUP {_lib.SEG_GROUP}\n" in hdr and f"#define TTASR_SEG_CHUNK_FRAMES {_lib.SEG_CHUNK_FRAMES}\n" in hdr
    assert '"seg_lstm_rows"' in hdr and "UNPINNED" in hdr
    assert _lib.SEG_GROUP >= 10                                   # a group holds the chunks that can overlap its first frame


def test_chunk_and_frame_counts_of_the_library_are_the_reference_tables():
    lib = _lib.load()                                             # no context, no GPU call
    for n in (0, 1, 270, 271, 990, 991, 79999, 80000, 80001, 87999, 88000, 88001, 96000, 16000 * 3600, 1 << 40):
        assert lib.ttasr_seg_chunks(n) == R.n_chunks(n) and lib.ttasr_seg_frames(n) == R.n_frames(n), n
    for n in (-1, (1 << 40) + 1):
        assert lib.ttasr_seg_chunks(n) < 0 and lib.ttasr_seg_frames(n) < 0


def test_the_tensor_table():
    t = vad.PYANNET_TENSORS
    assert len(t) == 51 and t["lstm.weight_ih_l0_reverse"] == (512, 60) and t["lstm.weight_ih_l3"] == (512, 256)
    assert t["classifier.weight"] == ("C", 128) and t["sincnet.conv1d.0.filters"] == (80, 1, 251)
    for classes in (1, 3, 8):
        w = vad.synth_pyannet_weights(5, classes)
        assert list(w) == list(t) and all(a.dtype == np.float32 for a in w.values())
        assert w["classifier.weight"].shape == (classes, 128) and w["classifier.bias"].shape == (classes,)
    a, b = vad.synth_pyannet_weights(5), vad.synth_pyannet_weights(5)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["linear.0.weight"], vad.synth_pyannet_weights(6)["linear.0.weight"])
    with pytest.raises(ValueError):
        vad.synth_pyannet_weights(0, 9)
    assert (vad.SYNTH_PYANNET_GAIN, vad.SYNTH_PYANNET_BIAS) == (4.0, -1.0)


def test_load_pyannet_state_round_trips_an_npz_and_builds_the_filters(tmp_path):
    w = vad.synth_pyannet_weights(vad.SYNTH_PYANNET_SEED)
    path = tmp_path / "pyannet.npz"
    np.savez(path, **w, **{"unrelated.key": np.zeros(3)})
    got = vad.load_pyannet_state(str(path))
    assert list(got) == list(vad.PYANNET_TENSORS) and all(np.array_equal(got[k], w[k]) for k in w)
    # a checkpoint carries the cutoffs, not the filters, and may wrap its tensors in a "state_dict" level
    low, band = vad.mel_cutoffs()
    ckpt = {k: v for k, v in w.items() if k != "sincnet.conv1d.0.filters"}
    ckpt.update({vad.PYANNET_CUTOFFS[0]: low, vad.PYANNET_CUTOFFS[1]: band})
    got = vad.load_pyannet_state({"state_dict": ckpt, "epoch": 3})
    assert np.array_equal(got["sincnet.conv1d.0.filters"], w["sincnet.conv1d.0.filters"])
    torch = pytest.importorskip("torch")
    tpath = tmp_path / "pyannet.ckpt"
    torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in ckpt.items()}}, tpath)
    got = vad.load_pyannet_state(tpath)
    assert all(np.array_equal(got[k], w[k]) for k in w)


def test_load_pyannet_state_refuses_wrong_shapes_and_missing_tensors():
    w = vad.synth_pyannet_weights(vad.SYNTH_PYANNET_SEED)
    bad = dict(w)
    bad["lstm.weight_hh_l2"] = np.zeros((512, 127), np.float32)
    with pytest.raises(ValueError, match="lstm.weight_hh_l2"):
        vad.load_pyannet_state(bad)
    bad = dict(w)
    bad["classifier.bias"] = np.zeros(2, np.float32)              # the classifier's weight and bias disagree on C
    with pytest.raises(ValueError, match="classifier.bias"):
        vad.load_pyannet_state(bad)
    bad = dict(w)
    bad["classifier.weight"], bad["classifier.bias"] = np.zeros((9, 128), np.float32), np.zeros(9, np.float32)
    with pytest.raises(ValueError, match="classifier.weight"):
        vad.load_pyannet_state(bad)
    bad = dict(w)
    del bad["sincnet.conv1d.0.filters"]                           # neither the filters nor the cutoffs
    with pytest.raises(ValueError, match="filters"):
        vad.load_pyannet_state(bad)


# ---- the backend on a fake engine ----

class _FakeEngine:
    has_segmentation = True

    def __init__(self):
        self.calls, self.closed = [], False

    def segmentation_scores(self, audios):
        """0.9 over the frames whose centre sample is louder than 0.05, else 0.1."""
        self.calls.append([len(a) for a in audios])
        out = []
        for a in audios:
            centres = 495 + 270 * np.arange(R.n_frames(len(a)))
            out.append(np.where(np.abs(a[np.minimum(centres, len(a) - 1)]) > 0.05, 0.9, 0.1).astype(np.float32))
        return out

    def close(self):
        self.closed = True


class _Client:
    sampling_rate, samples_width = 16000, 2

    def __init__(self, cid, audio):
        self.client_id = cid
        self.scratch_buffer = bytearray((np.asarray(audio) * 32767).astype("<i2").tobytes())


def _burst(n, a, b):
    x = np.zeros(n, np.float32)
    x[a:b] = 0.5
    return x


def test_factory_names():
    eng = _FakeEngine()
    for name in ("pyannote", "mi355x_pyannote"):
        b = vad_backends.VADFactory.create_vad_pipeline(name, engine=eng, pyannote_args={"onset": 0.6})
        assert isinstance(b, vad_backends.DevicePyannoteVAD) and isinstance(b, vad_backends.VADInterface)
        assert b.args == dict(onset=0.6, offset=0.5, min_duration_on=0.3, min_duration_off=0.3)
    assert isinstance(vad_backends.VADFactory.create_vad_pipeline("silero", engine=type("E", (), {"has_vad": True})()), vad_backends.DeviceStreamVAD)
    with pytest.raises(ValueError):
        vad_backends.VADFactory.create_vad_pipeline("pyannote")   # neither weights nor an engine
    with pytest.raises(ValueError):
        vad_backends.VADFactory.create_vad_pipeline("pyannote", engine=type("E", (), {"has_segmentation": False})())
    with pytest.raises(ValueError, match="min_speech"):
        vad_backends.DevicePyannoteVAD(engine=eng, pyannote_args={"min_speech": 1})
    with pytest.raises(ValueError, match="unsupported"):
        vad_backends.VADFactory.create_vad_pipeline("webrtc")


def test_keywords_are_checked_and_ignored_ones_are_logged(caplog):
    eng = _FakeEngine()
    for bad in ({"onset": 0.6}, {"vad_parameters": {}}, {"model": "x"}):
        with pytest.raises(ValueError, match="unknown keywords"):
            vad_backends.DevicePyannoteVAD(engine=eng, **bad)
    with caplog.at_level("WARNING"):
        b = vad_backends.DevicePyannoteVAD(engine=eng, model_name="pyannote/segmentation", auth_token="t", device_index=0)
        assert b.engine is eng and "model_name" in caplog.text and "auth_token" in caplog.text
        caplog.clear()
        vad_backends.DevicePyannoteVAD(engine=eng, vad_model={"not": "read"})     # the engine's own network stays
        assert "ignores vad_model" in caplog.text


def test_concurrent_clients_share_one_call_and_get_seconds():
    eng = _FakeEngine()
    b = vad_backends.DevicePyannoteVAD(engine=eng, max_wait_ms=500.0)
    clients = [_Client("a", _burst(48000, 8000, 24000)), _Client("b", _burst(32000, 0, 32000)), _Client("c", _burst(16000, 0, 0))]

    async def run():
        for c in clients:                                        # the three are known: the batch waits for all of them
            b._clients.setdefault(c.client_id, object())
        first = await asyncio.gather(*[b.detect_activity(c) for c in clients])
        b.forget(clients[2])                                     # gone: the next batch waits for two
        second = await asyncio.gather(*[b.detect_activity(c) for c in clients[:2]], b.detect_activity(_Client("d", np.zeros(0))))
        return first, second

    first, second = asyncio.run(run())
    assert eng.calls[0] == [48000, 32000, 16000] and b.calls_run[0] == 3
    # client a: frames 28 ... 87 are loud (495 + 270 j in [8000, 24000)): opens at frame 28, closes at frame 88
    assert first[0] == [{"start": (495 + 270 * 28) / 16000.0, "end": (495 + 270 * 88) / 16000.0, "confidence": 1.0}]
    # client b: speech from the first frame to the last, clipped to the buffer
    assert 495 + 270 * (R.n_frames(32000) - 1) > 32000
    assert first[1] == [{"start": 495 / 16000.0, "end": 2.0, "confidence": 1.0}] and first[2] == []
    assert second[0] == first[0] and second[1] == first[1] and second[2] == []   # an empty buffer: [] without a device call
    assert sum(b.calls_run) == 5 and all(len(c) <= 3 for c in eng.calls)
    assert "c" not in b._clients
    b.close()
    assert not eng.closed                                         # a shared engine stays open


def test_a_failing_call_reaches_every_waiting_client():
    class Broken(_FakeEngine):
        def segmentation_scores(self, audios):
            raise RuntimeError("device lost")

    b = vad_backends.DevicePyannoteVAD(engine=Broken(), max_wait_ms=1.0)

    async def run():
        return await asyncio.gather(*[b.detect_activity(_Client(i, _burst(16000, 0, 8000))) for i in range(2)], return_exceptions=True)

    out = asyncio.run(run())
    assert all(isinstance(o, RuntimeError) for o in out) and b.calls_run == []
