"""CPU: the Python surfaces of wire streams - vad.WireFormat, vad.StreamingSpeechDetector(wire=), vad_backends.DeviceStreamVAD(wire=)
and the ASR adapters' wire= / audio_from= - against a fake engine whose vad_stream_push_wire IS the numpy stream of
tests/wire_stream_reference.py.  What the device computes is tests/test_gpu_wire_stream.py's business; here: which bytes reach which
call, the reset of a cleared buffer, what a client may declare, and that wire=None makes exactly the calls it always made."""
import asyncio

import numpy as np
import pytest

import wire_stream_reference as ws
from taiwan_tongues_asr_ce_amd import vad
from taiwan_tongues_asr_ce_amd.asr import MI355XWhisperASR, pcm16_bytes_to_float
from taiwan_tongues_asr_ce_amd.vad_backends import DEFAULT_STREAM_VAD_OPTIONS, DeviceStreamVAD, VADFactory

OPTIONS = vad.VadOptions(**DEFAULT_STREAM_VAD_OPTIONS)


def _frame_probs(x):
    """The fake network: a frame is speech when its mean level is high (whole 512-sample frames of x)."""
    n = len(x) // 512
    return (np.abs(x[:n * 512]).reshape(n, 512).mean(axis=1) > 0.05).astype(np.float32)


class FakeEngine:
    """Engine.vad_stream_* without a device; `calls` records every call a backend makes."""
    has_vad = True

    def __init__(self):
        self.calls, self.streams, self.next_id = [], {}, 0

    def vad_stream_open(self, wire=None):
        self.calls.append(("open", wire))
        sid, self.next_id = self.next_id, self.next_id + 1
        args = wire.wire_args() if hasattr(wire, "wire_args") else wire
        self.streams[sid] = dict(wire=None if wire is None else ws.Stream(args[0], args[1], args[2], args[3]), pend=np.zeros(0, np.float32))
        return sid

    def vad_stream_reset(self, sid):
        self.calls.append(("reset", sid))
        s = self.streams[sid]
        s["pend"] = np.zeros(0, np.float32)
        if s["wire"] is not None:
            s["wire"].reset()

    def vad_stream_close(self, sid):
        self.calls.append(("close", sid))
        del self.streams[sid]

    def _frames(self, s, x):
        x = np.concatenate([s["pend"], x])
        s["pend"] = x[len(x) // 512 * 512:]
        return _frame_probs(x)

    def vad_stream_push(self, ids, audios, finish=None, return_logits=False):
        self.calls.append(("push", list(ids), [np.array(a) for a in audios]))
        assert all(self.streams[i]["wire"] is None for i in ids)
        return [self._frames(self.streams[i], np.asarray(a, np.float32)) for i, a in zip(ids, audios)]

    def vad_stream_push_wire(self, ids, raws, finish=None, return_logits=False):
        self.calls.append(("push_wire", list(ids), [bytes(r) for r in raws]))
        pcm = [self.streams[i]["wire"].push(bytes(r), bool(finish and finish[k])) for k, (i, r) in enumerate(zip(ids, raws))]
        return pcm, [self._frames(self.streams[i], p) for i, p in zip(ids, pcm)]


class Client:
    def __init__(self, cid, rate=16000, width=2, **extra):
        self.client_id, self.scratch_buffer, self.sampling_rate, self.samples_width = cid, bytearray(), rate, width
        self.last_start_time = 0
        for k, v in extra.items():
            setattr(self, k, v)


def _ulaw_speech(n, seed):
    """mu-law bytes whose level switches between loud and near silence every 0.4 s (3200 frames at 8 kHz)."""
    rng = np.random.default_rng([0xFA4E, seed])
    loud = rng.integers(0, 256, size=n, dtype=np.uint8)
    quiet = rng.choice(np.array([0xFF, 0x7F, 0xFE, 0x7E], dtype=np.uint8), size=n)      # +-0 and +-8 of 32768
    on = (np.arange(n) // 3200 + seed) % 2 == 0
    return np.where(on, loud, quiet).astype(np.uint8).tobytes()


def _expect(raw, fmt):
    """(audio, segments in seconds) of a wire client whose stream consumed `raw`: the first K(F) samples of the whole."""
    rate, ch, code, pick = fmt.wire_args()
    frames = len(raw) // fmt.frame_bytes
    audio = ws.offline(rate, raw, code, ch, pick)[:ws.final(rate, frames)]
    probs = _frame_probs(audio)
    cut = np.zeros(len(probs) * 512, np.float32)
    chunks = vad.get_speech_timestamps(cut, OPTIONS, lambda a: probs)
    return audio, [{"start": c["start"] / 16000.0, "end": c["end"] / 16000.0, "confidence": 1.0} for c in chunks]


def _eq(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_wire_backend_pushes_raw_tails_and_resets_on_a_cleared_buffer():
    eng = FakeEngine()
    fmt = vad.WireFormat(8000, encoding="ulaw")
    backend = VADFactory.create_vad_pipeline("silero", engine=eng, wire=fmt)          # the keyword goes through the factory
    sig = [_ulaw_speech(40000, 1), _ulaw_speech(40000, 2)]
    clients = [Client("a", 8000, 1), Client("b", 8000, 1)]
    steps = (12001, 11999, 7, 12345)

    async def scenario():
        pos = [0, 0]
        voiced = 0
        for step in steps:
            for k, c in enumerate(clients):
                c.scratch_buffer += sig[k][pos[k]:pos[k] + step]
                pos[k] += step
            got = await asyncio.gather(*(backend.detect_activity(c) for c in clients))
            for c, g in zip(clients, got):
                audio, segs = _expect(bytes(c.scratch_buffer), fmt)
                assert g == segs and _eq(backend.audio(c), audio) and _eq(backend.audio(c, covering=bytes(c.scratch_buffer)), audio)
                voiced += len(g)
        assert voiced >= 4
        pushes = [c for c in eng.calls if c[0] == "push_wire"]
        assert len(pushes) == len(steps) and all(len(p[1]) == 2 for p in pushes)      # the two clients share every push
        assert [len(r) for p in pushes for r in p[2]] == [s for s in steps for _ in clients]   # the raw tail, cut nowhere
        assert not any(c[0] == "push" for c in eng.calls)
        # the strategy clears the buffer after a transcription; other audio arrives before the next call
        a = clients[0]
        assert backend.audio(a, covering=bytes(a.scratch_buffer)[:-1]) is None        # not the bytes the stream consumed
        a.scratch_buffer.clear()
        a.scratch_buffer += sig[1][5000:5000 + pos[0] + 3]
        got = await backend.detect_activity(a)
        audio, segs = _expect(bytes(a.scratch_buffer), fmt)
        assert got == segs and _eq(backend.audio(a), audio)
        assert ("reset", 0) in eng.calls
        backend.forget(a)
        assert backend.audio(a) is None and ("close", 0) in eng.calls

    asyncio.run(scenario())


def test_a_client_declares_its_format_and_bad_declarations_are_refused():
    f = vad.WireFormat.of_client
    assert f(Client("a", 8000, 1, encoding="ulaw")) == vad.WireFormat(8000, 1, "ulaw", None)
    assert f(Client("a", 8000, 2, channels=2, audio_channel="right")).wire_args() == (8000, 2, 1, 1)
    assert f(Client("a", 48000, 3)).wire_args() == (48000, 1, 2, -1)
    assert f(Client("a", 44100, 4, encoding="f32", channels=2, audio_channel="mix")).wire_args() == (44100, 2, 4, -1)
    assert f(Client("a")).wire_args() == (16000, 1, 1, -1)
    for bad in (Client("a", 8000, 1), Client("a", 8000, 2, encoding="ulaw"), Client("a", 8000, 2, encoding="ima4"),
                Client("a", 8000, 5), Client("a", 8000, 2, channels=9), Client("a", 8000, 2, channels=2, audio_channel=2),
                Client("a", 8000, 2, audio_channel="middle"), Client("a", 0, 2)):
        with pytest.raises(ValueError):
            f(bad)
    with pytest.raises(ValueError):
        vad.WireFormat(8000, encoding="ima4")
    with pytest.raises(ValueError):
        DeviceStreamVAD(engine=FakeEngine(), wire="server")
    assert vad.resolve_wire(None) is None

    eng = FakeEngine()
    backend = DeviceStreamVAD(engine=eng, wire="client")
    tel = Client("t", 8000, 1, encoding="alaw", channels=2, audio_channel="left")
    hifi = Client("h", 48000, 2)
    tel.scratch_buffer += np.random.default_rng(5).integers(0, 256, 9001, dtype=np.uint8).tobytes()
    hifi.scratch_buffer += ws.recording(48000, ws.S16, 1, 6001)

    async def scenario():
        await asyncio.gather(backend.detect_activity(tel), backend.detect_activity(hifi))
        with pytest.raises(ValueError):
            await backend.detect_activity(Client("u", 8000, 1))                       # ambiguous: no stream is opened for it
    asyncio.run(scenario())
    opened = [c[1].wire_args() for c in eng.calls if c[0] == "open"]
    assert sorted(opened) == [(8000, 2, 16, 0), (48000, 1, 1, -1)]
    assert _eq(backend.audio(tel), ws.offline(8000, bytes(tel.scratch_buffer), ws.ALAW, 2, 0)[:ws.final(8000, 4500)])
    assert _eq(backend.audio(hifi), ws.offline(48000, bytes(hifi.scratch_buffer), ws.S16, 1)[:ws.final(48000, 6001)])


def test_adapters_take_the_backends_audio_when_it_covers_the_buffer():
    eng = FakeEngine()
    fmt = vad.WireFormat(8000, channels=2, encoding="s16", audio_channel="right")
    backend = DeviceStreamVAD(engine=eng, wire=fmt)
    c = Client("a", 8000, 2, channels=2)
    raw = ws.recording(8000, ws.S16, 2, 5000)
    c.scratch_buffer += raw[:12002]
    asyncio.run(backend.detect_activity(c))

    def adapter(**kw):
        a = object.__new__(MI355XWhisperASR)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    with_backend = adapter(wire=fmt, audio_from=backend)
    want = ws.offline(8000, raw[:12000], ws.S16, 2, 1)[:ws.final(8000, 3000)]          # the final samples only: 6000 - 20
    assert len(want) == 5980 and _eq(with_backend.client_audio(c), want)
    host = fmt.to_16k(bytes(c.scratch_buffer))                                         # the host conversion and resampler
    assert len(host) == 6000 and host.dtype == np.float32
    assert np.abs(host[200:5900] - want[200:5900]).max() < 1e-3                         # the same audio, by another resampler
    c.scratch_buffer += raw[12002:12802]                                              # the buffer has grown past the stream
    assert _eq(with_backend.client_audio(c), fmt.to_16k(bytes(c.scratch_buffer)))
    assert _eq(adapter(wire=fmt, audio_from=None).client_audio(c), fmt.to_16k(bytes(c.scratch_buffer)))
    assert _eq(adapter(wire="client").client_audio(c), vad.WireFormat(8000, 2, "s16").to_16k(bytes(c.scratch_buffer)))   # as declared: the mean
    # wire=None (and an adapter built before the keyword existed): the s16 bytes at 16 kHz, as ever
    s16 = Client("p")
    s16.scratch_buffer += (np.arange(-300, 300, dtype="<i2") * 50).tobytes()
    for a in (adapter(wire=None, audio_from=backend), adapter()):
        assert _eq(a.client_audio(s16), pcm16_bytes_to_float(s16.scratch_buffer))
    # the picked channel of the host conversion is the picked channel
    assert _eq(fmt.to_mono(raw[:400]), (np.frombuffer(raw[:400], "<i2").reshape(-1, 2)[:, 1].astype(np.float32) / 32768.0))


def test_wire_none_makes_exactly_the_old_calls():
    eng = FakeEngine()
    backend = DeviceStreamVAD(engine=eng)
    c = Client("a")
    x = (np.random.default_rng(3).standard_normal(9000) * 3000).astype("<i2").tobytes()
    for n in (4001, 9000, 18000):
        c.scratch_buffer[:] = x[:n]
        asyncio.run(backend.detect_activity(c))
    assert [k[0] for k in eng.calls] == ["open", "push", "push", "push"] and eng.calls[0] == ("open", None)
    tails = [x[0:4000], x[4000:9000], x[9000:18000]]                                  # whole samples behind the consumed prefix
    for call, tail in zip(eng.calls[1:], tails):
        assert call[1] == [0] and len(call[2]) == 1 and _eq(call[2][0], pcm16_bytes_to_float(tail))
    assert backend.audio(c) is None                                                   # no wire stream: its caller has the audio
    det = vad.StreamingSpeechDetector(eng)
    with pytest.raises(ValueError):
        det.feed_bytes(b"\0\0")
    assert eng.calls[-1] == ("open", None)
    wired = vad.StreamingSpeechDetector(eng, wire=vad.WireFormat(8000, encoding="ulaw"))
    raw = _ulaw_speech(9000, 4)
    for piece in (raw[:1], raw[1:4000], raw[4000:]):
        wired.feed_bytes(piece)
    assert _eq(wired.audio, ws.offline(8000, raw, ws.ULAW, 1)[:ws.final(8000, 9000)]) and wired.n_samples == len(wired.audio)
    assert len(wired.probs) == len(wired.audio) // 512
    wired.feed_bytes(b"", finish=True)
    assert _eq(wired.audio, ws.offline(8000, raw, ws.ULAW, 1))
