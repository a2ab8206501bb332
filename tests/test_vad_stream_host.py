"""Host: vad.StreamingSpeechDetector and vad_backends (VADInterface, SimpleVAD, DeviceStreamVAD, VADFactory) on an engine
double.  The double implements Engine.vad_stream_open / _reset / _close / _push with the framing of include/ttasr.h on
vad_reference.SileroRef(float32).step: per stream (h, c), the last 64 evaluated samples and the pending samples; every complete
512-sample frame is evaluated in order, `finish` evaluates the zero-padded remainder and leaves the stream as reset."""
import asyncio
import zlib

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, vad, vad_backends
from taiwan_tongues_asr_ce_amd.asr import pcm16_bytes_to_float
from taiwan_tongues_asr_ce_amd.vad_backends import DeviceStreamVAD, SimpleVAD, VADFactory, VADInterface
from vad_reference import SileroRef, test_signal

SEED = vad.SYNTH_SILERO_SEED


class EngineDouble:
    has_vad = True

    def __init__(self):
        self.ref = SileroRef(vad.synth_silero_weights(SEED), np.float32)
        self.streams = {}
        self.pushes = []          # ids of every push
        self.resets = []
        self.closed = []

    @staticmethod
    def _zero():
        return {"state": np.zeros((2, 1, 128), np.float32), "ctx": np.zeros(64, np.float32), "pend": np.zeros(0, np.float32)}

    def vad_stream_open(self):
        sid = min(set(range(len(self.streams) + 1)) - set(self.streams))
        self.streams[sid] = self._zero()
        return sid

    def vad_stream_reset(self, sid):
        self.streams[sid] = self._zero()
        self.resets.append(sid)

    def vad_stream_close(self, sid):
        del self.streams[sid]
        self.closed.append(sid)

    def vad_stream_push(self, ids, audios, finish=None, return_logits=False):
        assert len(set(ids)) == len(ids) == len(audios) and not return_logits
        self.pushes.append(list(ids))
        out = []
        for k, (sid, a) in enumerate(zip(ids, audios)):
            st = self.streams[sid]
            x = np.concatenate([st["pend"], np.asarray(a, np.float32)])
            fin = bool(finish[k]) if finish is not None else False
            if fin and len(x) % 512:
                x = np.concatenate([x, np.zeros(512 - len(x) % 512, np.float32)])
            probs = []
            for f in range(len(x) // 512):
                frame = x[512 * f:512 * f + 512]
                p, st["state"] = self.ref.step(np.concatenate([st["ctx"], frame])[None, :], st["state"])
                st["state"] = st["state"].astype(np.float32)
                st["ctx"] = frame[-64:]
                probs.append(p)
            st["pend"] = x[len(x) // 512 * 512:]
            if fin:
                self.streams[sid] = self._zero()
            out.append(np.asarray(probs, dtype=np.float32))
        return out


class Client:
    def __init__(self, cid):
        self.client_id, self.scratch_buffer, self.sampling_rate, self.samples_width = cid, bytearray(), 16000, 2


def _s16(x):
    return (np.clip(x, -1, 1) * 32767).astype("<i2").tobytes()


@pytest.fixture(scope="module")
def world():
    """The double, a 4-s stretch of the test signal that starts 1 s before its first burst, and its offline probabilities."""
    eng = EngineDouble()
    sig = test_signal()
    start = int(np.flatnonzero(sig)[0]) - 16000
    audio = pcm16_bytes_to_float(_s16(sig[start:start + 4 * 16000]))
    probs = eng.ref.probs(audio).astype(np.float32)
    return eng, audio, probs


def _expect(world, n_samples, options):
    _, audio, probs = world
    k = n_samples // 512
    return vad.get_speech_timestamps(audio[:512 * k], options, lambda a: probs[:k])


def _seconds(chunks):
    return [{"start": c["start"] / 16000.0, "end": c["end"] / 16000.0, "confidence": 1.0} for c in chunks]


def test_streaming_speech_detector_equals_the_offline_rule_on_the_cut_buffer(world):
    eng, audio, _ = world
    det = vad.StreamingSpeechDetector(eng)
    o = vad.VadOptions(**vad_backends.DEFAULT_STREAM_VAD_OPTIONS)
    pos, seen = 0, set()
    for k in (12001, 0, 24003, 511, 513, 20000):
        det.feed(audio[pos:pos + k])
        pos += k
        got = det.segments(o)
        assert got == _expect(world, pos, o), pos
        assert det.n_samples == pos and len(det.probs) == pos // 512      # the partial frame waits until it fills
        seen.add(len(got))
    assert seen != {0}
    det.reset()
    assert det.n_samples == 0 and det.segments(o) == [] and eng.resets[-1] == det.stream_id
    det.feed(audio[:16000])
    assert det.segments(o) == _expect(world, 16000, o)
    sid = det.stream_id
    det.close()
    assert sid in eng.closed and sid not in eng.streams


def test_device_stream_vad_appends_resets_and_forgets(world):
    eng, audio, _ = world
    raw = _s16(audio)
    b = DeviceStreamVAD(engine=eng)
    o = b.options
    assert (o.threshold, o.min_speech_duration_ms, o.min_silence_duration_ms, o.speech_pad_ms) == (0.5, 300, 300, 0)
    c = Client("c1")
    r0 = len(eng.resets)

    async def scenario():
        closed = opened = 0
        for step in (24002, 48006, 24001, 30003):                          # odd byte counts: half a sample waits for its other half
            c.scratch_buffer += raw[len(c.scratch_buffer):len(c.scratch_buffer) + step]
            got = await b.detect_activity(c)
            n = len(c.scratch_buffer) // 2
            assert got == _seconds(_expect(world, n, o)), n
            if got and got[-1]["end"] < len(c.scratch_buffer) / 32000.0 - 0.1:
                closed += 1
            elif got:
                opened += 1
        assert closed >= 1 and opened >= 1, (closed, opened)
        st = b._streams["c1"]
        sid = st.detector.stream_id
        assert st.consumed == len(c.scratch_buffer) // 2 * 2 and st.crc == zlib.crc32(bytes(c.scratch_buffer[:st.consumed]))
        assert all(len(p) == 1 for p in eng.pushes[-4:]) and eng.resets[r0:] == []
        # a shorter buffer: the strategy cleared it after a transcription
        del c.scratch_buffer[:]
        c.scratch_buffer += raw[:20000]
        assert await b.detect_activity(c) == _seconds(_expect(world, 10000, o))
        assert eng.resets[r0:] == [sid]
        # as long as before, other content: found through the CRC of the consumed prefix
        del c.scratch_buffer[:]
        c.scratch_buffer += raw[32000:32000 + 20000 + 5000]
        got = await b.detect_activity(c)
        assert eng.resets[r0:] == [sid, sid]
        fresh = DeviceStreamVAD(engine=eng)
        c2 = Client("c2")
        c2.scratch_buffer += c.scratch_buffer
        assert got == await fresh.detect_activity(c2)
        fresh.forget(c2)
        b.forget(c)
        assert sid in eng.closed and "c1" not in b._streams
        b.forget(c)                                                        # unknown client: nothing to do

    n_closed = len(eng.closed)
    asyncio.run(scenario())
    assert len(eng.closed) == n_closed + 2
    b.close()


def test_concurrent_calls_share_one_push(world):
    eng, audio, _ = world
    raw = _s16(audio)
    b = DeviceStreamVAD(engine=eng, max_wait_ms=2.0)
    clients = [Client(i) for i in range(9)]
    for i, c in enumerate(clients):
        c.scratch_buffer += raw[2000 * i:2000 * i + 3000 + 1024 * i]

    async def scenario():
        got = await asyncio.gather(*(b.detect_activity(c) for c in clients[:8]))
        assert b.pushes_run == [8] and len(eng.pushes[-1]) == 8 and len(got) == 8
        await b.detect_activity(clients[8])                                # later: a push of its own
        assert b.pushes_run == [8, 1]
        clients[0].scratch_buffer += raw[:4000]
        await asyncio.gather(b.detect_activity(clients[0]), b.detect_activity(clients[0]))   # one stream: one row per push
        assert b.pushes_run == [8, 1, 1, 1]
        for c in clients:
            b.forget(c)

    asyncio.run(scenario())
    b.close()


def test_simple_vad():
    v = SimpleVAD()
    c = Client("s")
    assert isinstance(v, VADInterface) and v.min_duration == 0.1
    assert asyncio.run(v.detect_activity(c)) == []                         # empty
    c.scratch_buffer += bytes(3198)                                        # 0.0999 s
    assert asyncio.run(v.detect_activity(c)) == []                         # shorter than min_duration
    c.scratch_buffer += bytes(2)
    assert asyncio.run(v.detect_activity(c)) == [{"start": 0.0, "end": 0.1, "confidence": 1.0}]
    c.sampling_rate, c.samples_width = 8000, 4                             # the duration follows the client's format
    assert asyncio.run(SimpleVAD(min_duration=0.05).detect_activity(c))[0]["end"] == 3200 / 32000.0
    with pytest.raises(NotImplementedError):
        asyncio.run(VADInterface().detect_activity(c))


def test_vad_factory(world):
    eng = world[0]
    assert type(VADFactory.create_vad_pipeline("simple", min_duration=0.2)) is SimpleVAD
    assert VADFactory.create_vad_pipeline("simple", min_duration=0.2).min_duration == 0.2
    for name in ("silero", "mi355x_silero"):
        v = VADFactory.create_vad_pipeline(name, engine=eng, max_wait_ms=1.0, vad_parameters={"min_silence_duration_ms": 500})
        assert type(v) is DeviceStreamVAD and v.engine is eng and v.options.min_silence_duration_ms == 500 and v.options.threshold == 0.5
    for name in ("pyannote", "", None):
        with pytest.raises(ValueError):
            VADFactory.create_vad_pipeline(name)
    with pytest.raises(ValueError):
        DeviceStreamVAD()                                                  # neither weights nor an engine


def test_the_stream_symbols_are_declared():
    names = ("ttasr_vad_stream_open", "ttasr_vad_stream_reset", "ttasr_vad_stream_close", "ttasr_vad_stream_push")
    assert all(s in _lib.SYMBOLS for s in names)                           # the export test holds the library to SYMBOLS
    assert _lib.VAD_MAX_STREAMS == 1024
