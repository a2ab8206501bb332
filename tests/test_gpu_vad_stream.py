"""GPU: the stateful streaming VAD (ttasr_vad_stream_*, Engine.vad_stream_*, vad.StreamingSpeechDetector, vad_backends).

The contract is a bit contract: however a recording is cut into pushes, interleaved with other streams, ordered in a call or
grouped, the concatenated outputs of its stream equal the offline call (Engine.vad_probs) on the whole recording - `np.array_equal`
on float32, probabilities and logits - and without `finish` its first len // 512 values.  The offline call itself is held to
float64 by tests/test_gpu_vad.py; one split case here is held to the same reference at the same bounds (logits 1e-3,
probabilities 2.5e-4)."""
import asyncio
import ctypes as C

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError
from vad_reference import cached_probs, test_signal

pytestmark = pytest.mark.gpu

SEED = vad.SYNTH_SILERO_SEED
CHUNK = _lib.VAD_CHUNK_FRAMES
PIECES = (1, 511, 0, 512, 513, 63, 65, 1031)
LOGIT_TOL, PROB_TOL = 1e-3, 2.5e-4
E_INVALID = -1
_engines = {}


def _noise(n, seed):
    return (np.random.default_rng([0xA0D10, seed]).standard_normal(n) * 0.2).astype(np.float32)


def _long(n):
    """Noise whose level changes every 0.7 s (silence included), so the probabilities move."""
    rng = np.random.default_rng([0xA0D10, 77])
    level = np.repeat(rng.choice([0.0, 0.02, 0.1, 0.3], size=n // 11200 + 1), 11200)[:n]
    return (rng.standard_normal(n) * level).astype(np.float32)


def _engine(mode=COMPUTE_F32, max_batch=5):
    key = (mode, max_batch)
    if key not in _engines:
        e = Engine(PRESETS["micro"], mode, max_batch)
        e.load_weights(synth.iter_weights(PRESETS["micro"]))
        e.load_vad(vad.synth_silero_weights(SEED))
        _engines[key] = e
    return _engines[key]


def _offline(e, x):
    p, l = e.vad_probs([x], return_logits=True)
    return p[0], l[0]


def _cuts(n, pieces=PIECES):
    """Piece sizes cycling through `pieces`, cut to what is left of n samples."""
    out, i = [], 0
    while n > 0:
        k = min(pieces[i % len(pieces)], n)
        out.append(k)
        n -= k
        i += 1
    return out


def _feed(e, sid, x, finish, pieces=PIECES):
    """x through stream sid in pieces; checks every push's frame count; returns the concatenated (probs, logits)."""
    ps, ls, pos, pend = [], [], 0, 0
    cuts = _cuts(len(x), pieces)
    for j, k in enumerate(cuts):
        last = finish and j == len(cuts) - 1
        p, l = e.vad_stream_push([sid], [x[pos:pos + k]], finish=[last], return_logits=True)
        want = (pend + k) // 512 + (1 if last and (pend + k) % 512 else 0)
        assert len(p[0]) == want and len(l[0]) == want, (len(x), j, k)
        pend = (pend + k) % 512
        pos += k
        ps.append(p[0]); ls.append(l[0])
    return np.concatenate(ps), np.concatenate(ls)


def _same(got, want):
    return all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(got, want))


def _recordings():
    return [_noise(n, n) for n in (1, 511, 512, 513, 576, 1100)] + [test_signal()[: 512 * 40 + 7]]


# ---- 1. splits ----

def test_every_split_equals_the_offline_call():
    e = _engine()
    sid = e.vad_stream_open()
    for x in _recordings():
        want = _offline(e, x)
        assert _same(_feed(e, sid, x, finish=True), want), len(x)          # finish: the stream is as reset afterwards
        k = len(x) // 512
        got = _feed(e, sid, x, finish=False)
        assert len(got[0]) == k and _same(got, (want[0][:k], want[1][:k])), len(x)
        e.vad_stream_reset(sid)
    x = _recordings()[-1]
    p, l = _feed(e, sid, x, finish=True)
    want_p, want_l = cached_probs(SEED, ("signal-cut", len(x)), x)
    worst_l, worst_p = float(np.abs(l - want_l).max()), float(np.abs(p - want_p).max())
    print(f"vad stream, split test signal: device vs float64 logits {worst_l:.3e} probs {worst_p:.3e}")
    assert worst_l <= LOGIT_TOL and worst_p <= PROB_TOL
    e.vad_stream_close(sid)


# ---- 2. interleaving ----

def test_interleaved_streams_reset_and_an_offline_call_between_pushes():
    e = _engine()
    recs = [_noise(n, 100 + n) for n in (1100, 2000, 3333, 4096, 5000)]
    other = _noise(2777, 9)                                   # what stream 2 is fed after its reset
    want = [_offline(e, x) for x in recs]
    want_other = _offline(e, other)
    ids = [e.vad_stream_open() for _ in recs]
    pos = [0] * 5
    got = [([], []) for _ in recs]
    src = list(recs)

    def push(rows):
        """rows: (stream index, samples to take or None = the rest with finish), in the order of the call."""
        audios, fin = [], []
        for k, n in rows:
            take = len(src[k]) - pos[k] if n is None else n
            audios.append(src[k][pos[k]:pos[k] + take])
            fin.append(n is None)
            pos[k] += take
        p, l = e.vad_stream_push([ids[k] for k, _ in rows], audios, finish=fin, return_logits=True)
        for (k, _), pi, li in zip(rows, p, l):
            got[k][0].append(pi); got[k][1].append(li)

    push([(0, 300), (1, 513), (2, 1000), (3, 0), (4, 2048)])
    push([(4, 1), (2, 511), (0, 212)])                        # permuted, streams 1 and 3 absent
    e.vad_probs([_noise(1500, 3), _noise(700, 4)])            # an offline call between two pushes changes nothing
    push([(3, 4000), (1, 63), (0, 1)])
    e.vad_stream_reset(ids[2])                                # stream 2 starts over with another recording
    src[2], pos[2], got[2] = other, 0, ([], [])
    push([(2, 1031), (4, 1000), (1, None), (3, 0)])
    push([(0, None), (3, None), (2, 700)])
    push([(2, None), (4, None)])
    for k in range(5):
        w = want_other if k == 2 else want[k]
        assert _same((np.concatenate(got[k][0]), np.concatenate(got[k][1])), w), k
    for i in ids:
        e.vad_stream_close(i)


# ---- 3. more rows than max_batch ----

def test_twelve_streams_in_one_push_on_a_five_row_engine():
    e = _engine(COMPUTE_F32, 5)
    recs = [_noise(300 + 517 * i, 200 + i) for i in range(12)]
    ids = [e.vad_stream_open() for _ in recs]
    p, l = e.vad_stream_push(ids, recs, finish=[True] * 12, return_logits=True)   # three groups, the last one partial
    for x, pi, li in zip(recs, p, l):
        assert _same((pi, li), _offline(e, x)), len(x)
    for i in ids:
        e.vad_stream_close(i)


# ---- 4. the chunk loop ----

def test_a_push_longer_than_a_time_chunk():
    e = _engine()
    x = _long(100 + 512 * CHUNK + 513 + 40)
    sid = e.vad_stream_open()
    assert len(e.vad_stream_push([sid], [x[:100]])[0]) == 0                       # 100 samples pending
    p1, l1 = e.vad_stream_push([sid], [x[100:100 + 512 * CHUNK + 513]], return_logits=True)
    assert len(p1[0]) == CHUNK + 1                                                # two time chunks
    p2, l2 = e.vad_stream_push([sid], [x[100 + 512 * CHUNK + 513:]], finish=[True], return_logits=True)
    assert len(p2[0]) == 1
    want = _offline(e, x)
    assert _same((np.concatenate([p1[0], p2[0]]), np.concatenate([l1[0], l2[0]])), want)
    assert float(np.ptp(want[0])) > 0.3                                           # the values do move
    e.vad_stream_close(sid)


# ---- 5. finish and reuse ----

def test_finish_reuse_and_reopen():
    e = _engine()
    x = _noise(1024, 31)
    want = _offline(e, x)
    sid = e.vad_stream_open()
    p, l = e.vad_stream_push([sid], [x], finish=[True], return_logits=True)       # nothing pending: no extra value
    assert len(p[0]) == 2 and _same((p[0], l[0]), want)
    assert len(e.vad_stream_push([sid], [x[:0]], finish=[True])[0]) == 0
    again = e.vad_stream_push([sid], [x], finish=[True], return_logits=True)      # after finish: the same bits again
    assert _same((again[0][0], again[1][0]), want)
    e.vad_stream_push([sid], [x[:700]])                                           # leaves state and pending samples behind
    e.vad_stream_close(sid)
    sid2 = e.vad_stream_open()
    assert sid2 == sid                                                            # the lowest free id: the same one
    fresh = e.vad_stream_push([sid2], [x], finish=[True], return_logits=True)
    assert _same((fresh[0][0], fresh[1][0]), want)                                # ... with zero state
    e.vad_stream_close(sid2)
    with pytest.raises(TtasrError):
        e.vad_stream_close(sid2)


# ---- 6. compute modes ----

def test_compute_mode_does_not_change_a_bit():
    x = test_signal()[: 512 * 40 + 7]
    want = _offline(_engine(COMPUTE_F32), x)
    for mode in (COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16):
        e = _engine(mode)
        sid = e.vad_stream_open()
        assert _same(_feed(e, sid, x, finish=True), want), mode
        e.vad_stream_close(sid)


# ---- 7. isolation ----

def _generate(e):
    st = e.special
    opts = e.gen_opts(12, True, suppress=[1, 2, 7, st.sot], begin_suppress=[5, st.eot], check_interval=1)
    return e.generate([[st.sot, st.lang_zh, st.transcribe]] * 2, opts)


def test_generate_after_stream_pushes_is_bit_identical():
    e = _engine(COMPUTE_BF16)
    n = PRESETS["micro"].n_frames * 160
    clips = [synth.noise_clip(i, n) for i in range(2)]
    e.log_mel(clips, want_output=False)
    e.encode(2)
    a = _generate(e)
    e.log_mel(clips, want_output=False)
    e.encode(2)
    ids = [e.vad_stream_open(), e.vad_stream_open()]
    e.vad_stream_push(ids, [_noise(1100, 1), test_signal()[: 16000 * 3]])
    b = _generate(e)
    assert a.tokens == b.tokens and np.array_equal(a.sum_logprob, b.sum_logprob) and np.array_equal(a.no_speech_prob, b.no_speech_prob)
    e.vad_stream_push(ids[::-1], [_noise(600, 2), _noise(77, 3)], finish=[True, False])   # between two generates of one encoder state
    c = _generate(e)
    assert a.tokens == c.tokens and np.array_equal(a.sum_logprob, c.sum_logprob)
    for i in ids:
        e.vad_stream_close(i)


# ---- 8. inside an open session ----

def test_pushes_between_the_calls_of_an_open_session():
    e = _engine(COMPUTE_F32, 5)
    st = e.special
    n = PRESETS["micro"].n_frames * 160
    clips = [synth.noise_clip(40 + i, n) for i in range(7)]                       # more clips than rows: rows are refilled
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    caps = np.asarray([6, 16, 9, 12, 7, 14, 10], dtype=np.int32)
    opts = e.gen_opts(16, False, suppress_eot=True, check_interval=1)
    recs = [_noise(3000 + 700 * i, 300 + i) for i in range(3)]
    want = [_offline(e, x) for x in recs]                                         # computed before the session begins
    ids = [e.vad_stream_open() for _ in recs]

    def run(with_pushes):
        toks, pos, got, step, pushes = {}, [0] * 3, [([], []) for _ in recs], 0, 0
        with e.session(opts, len(prompt)) as s:
            cids = s.submit(clips, [prompt] * len(clips), caps)
            if with_pushes:
                with pytest.raises(TtasrError):
                    e.vad_stream_open()                                           # its first call allocates: refused in a session
            while s.pending > 0:
                for r in s.poll(max_steps=1):
                    toks[cids.index(r.id)] = r.tokens
                if with_pushes:
                    rows = [k for k in range(3) if pos[k] < len(recs[k]) and (step + k) % 3 != 2]   # streams come and go
                    if rows:
                        take = [min(257 + 300 * k, len(recs[k]) - pos[k]) for k in rows]
                        fin = [pos[k] + t == len(recs[k]) for k, t in zip(rows, take)]
                        p, l = e.vad_stream_push([ids[k] for k in rows], [recs[k][pos[k]:pos[k] + t] for k, t in zip(rows, take)],
                                                 finish=fin, return_logits=True)
                        pushes += 1
                        for k, t, pi, li in zip(rows, take, p, l):
                            pos[k] += t
                            got[k][0].append(pi); got[k][1].append(li)
                    step += 1
        return toks, pos, got, pushes

    plain, _, _, _ = run(False)
    toks, pos, got, pushes = run(True)
    assert pushes >= 5                                                            # pushes did run inside the session
    assert len(plain) == 7 and toks == plain                                      # every result's tokens, with and without pushes
    for k in range(3):                                                            # what the session left unfed goes in afterwards
        if pos[k] < len(recs[k]):
            p, l = e.vad_stream_push([ids[k]], [recs[k][pos[k]:]], finish=[True], return_logits=True)
            got[k][0].append(p[0]); got[k][1].append(l[0])
        assert _same((np.concatenate(got[k][0]), np.concatenate(got[k][1])), want[k]), k
    for i in ids:
        e.vad_stream_close(i)


# ---- 9. refusals ----

def _raw_push(e, ids, audios, finish=None, outs="auto", n=None, frames=True, null_pcm=False, ns=None):
    k = len(ids)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    idv = np.asarray(ids, dtype=np.int32)
    nsv = np.asarray([len(a) for a in audios] if ns is None else ns, dtype=np.int64)
    bufs = [np.zeros(len(a) // 512 + 2, np.float32) for a in audios]
    ptrs = (C.c_void_p * k)(*[None if null_pcm else a.ctypes.data for a in audios])
    optr = (C.c_void_p * k)(*[b.ctypes.data for b in bufs]) if outs == "auto" else outs
    fr = np.zeros(k, dtype=np.int32)
    fin = np.asarray(finish, dtype=np.int32).ctypes.data_as(i32p) if finish is not None else None
    return e.lib.ttasr_vad_stream_push(e.h, k if n is None else n, idv.ctypes.data_as(i32p), ptrs, nsv.ctypes.data_as(i64p), fin,
                                       optr, None, fr.ctypes.data_as(i32p) if frames else None)


def test_refusals_leave_every_stream_as_it_was():
    w = vad.synth_silero_weights(SEED)
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    sid = C.c_int32(-1)
    assert e.lib.ttasr_vad_stream_open(e.h, C.byref(sid)) == E_INVALID            # VAD weights not finalized
    assert _raw_push(e, [0], [_noise(600, 1)]) == E_INVALID
    e.load_vad(w)
    x = _noise(2000, 50)
    want = _engine().vad_probs([x], return_logits=True)
    want = (want[0][0], want[1][0])
    assert _raw_push(e, [0], [x]) == E_INVALID                                    # no stream is open: n above their number
    a, b = e.vad_stream_open(), e.vad_stream_open()
    piece = x[700:1300]
    null1 = (C.c_void_p * 1)(None)
    refusals = [
        lambda: _raw_push(e, [a], [piece], n=0),                                  # n < 1
        lambda: _raw_push(e, [a, b, a], [piece] * 3),                             # n above the number of open streams
        lambda: e.lib.ttasr_vad_stream_push(e.h, 1, None, None, None, None, None, None, None),   # NULL arrays
        lambda: _raw_push(e, [a], [piece], frames=False),                         # NULL out_frames
        lambda: _raw_push(e, [a], [piece], outs=None),                            # NULL out_probs array
        lambda: _raw_push(e, [7], [piece]),                                       # an id that is not open
        lambda: _raw_push(e, [-1], [piece]),
        lambda: _raw_push(e, [_lib.VAD_MAX_STREAMS], [piece]),
        lambda: _raw_push(e, [a, a], [piece, piece]),                             # the same id twice
        lambda: _raw_push(e, [a], [piece], ns=[-1]),                              # a negative length
        lambda: _raw_push(e, [a], [piece], null_pcm=True),                        # a NULL pcm with samples
        lambda: _raw_push(e, [a], [piece], outs=null1),                           # a NULL output row that would receive values
        lambda: _raw_push(e, [b, a], [piece[:10], piece], outs=(C.c_void_p * 2)(None, None)),
        lambda: e.lib.ttasr_vad_stream_reset(e.h, 9),
        lambda: e.lib.ttasr_vad_stream_close(e.h, 9),
    ]
    for k, refusal in enumerate(refusals):
        head = e.vad_stream_push([a], [x[:700]], return_logits=True)              # a half-fed stream: state and 188 pending samples
        assert refusal() == E_INVALID, k
        tail = e.vad_stream_push([a], [x[700:]], finish=[True], return_logits=True)   # ... completes to its offline bits
        assert _same((np.concatenate([head[0][0], tail[0][0]]), np.concatenate([head[1][0], tail[1][0]])), want), k
    assert _raw_push(e, [b], [piece[:10]], outs=null1) == 0                       # a row that receives no value may be NULL
    e.vad_stream_reset(b)
    ids = [a, b] + [e.vad_stream_open() for _ in range(_lib.VAD_MAX_STREAMS - 2)]
    assert sorted(ids) == list(range(_lib.VAD_MAX_STREAMS))
    assert e.lib.ttasr_vad_stream_open(e.h, C.byref(sid)) == E_INVALID            # beyond TTASR_VAD_MAX_STREAMS
    with pytest.raises(TtasrError):
        e.vad_stream_open()
    got = e.vad_stream_push([ids[-1], ids[500]], [x, x], finish=[True, True], return_logits=True)
    assert _same((got[0][0], got[1][0]), want) and _same((got[0][1], got[1][1]), want)
    for i in ids:
        e.vad_stream_close(i)
    assert _raw_push(e, [a], [piece]) == E_INVALID                                # closed
    e.close()


# ---- 10. the backend on the device ----

class _Client:
    def __init__(self, cid):
        self.client_id, self.scratch_buffer, self.sampling_rate, self.samples_width = cid, bytearray(), 16000, 2


def _s16(x):
    return (np.clip(x, -1, 1) * 32767).astype("<i2").tobytes()


def test_device_stream_vad_backend_follows_growing_scratch_buffers():
    from taiwan_tongues_asr_ce_amd.asr import pcm16_bytes_to_float
    from taiwan_tongues_asr_ce_amd.vad_backends import DEFAULT_STREAM_VAD_OPTIONS, VADFactory
    weights = vad.synth_silero_weights(SEED)
    backend = VADFactory.create_vad_pipeline("silero", vad_model=weights)
    ref = _engine()
    options = vad.VadOptions(**DEFAULT_STREAM_VAD_OPTIONS)
    sig = _s16(test_signal())
    offs = (0, 7 * 32000)                                     # the two clients hear different parts of the signal
    steps = (24002, 48006, 24002, 50002, 30002, 48002, 24006)
    clients = [_Client("a"), _Client("b")]

    def expect(c):
        audio = pcm16_bytes_to_float(bytes(c.scratch_buffer[: len(c.scratch_buffer) // 2 * 2]))
        cut = audio[: len(audio) // 512 * 512]
        probs = ref.vad_probs([cut])[0]
        chunks = vad.get_speech_timestamps(cut, options, lambda a: probs)
        return [{"start": ch["start"] / 16000.0, "end": ch["end"] / 16000.0, "confidence": 1.0} for ch in chunks]

    async def scenario():
        before = after = 0
        pos = list(offs)
        for step in steps:
            for k, c in enumerate(clients):
                c.scratch_buffer += sig[pos[k]:pos[k] + step]
                pos[k] += step
            got = await asyncio.gather(*(backend.detect_activity(c) for c in clients))
            for c, g in zip(clients, got):
                assert g == expect(c), (c.client_id, step)
                duration = len(c.scratch_buffer) / 32000.0
                if g and g[-1]["end"] < duration - 0.1:
                    before += 1
                elif g:
                    after += 1
        assert before >= 1 and after >= 1, (before, after)    # the trigger sees both a closed and an open last segment
        assert backend.pushes_run == [2] * len(steps)         # the two clients' calls share one push
        # the strategy clears the buffer after a transcription; other audio of at least the old length arrives before the next call
        old = len(clients[0].scratch_buffer)
        clients[0].scratch_buffer.clear()
        clients[0].scratch_buffer += sig[20 * 32000: 20 * 32000 + old + 4002]
        got = await backend.detect_activity(clients[0])
        assert got == expect(clients[0])
        fresh = VADFactory.create_vad_pipeline("mi355x_silero", engine=backend.engine)
        c2 = _Client("z")
        c2.scratch_buffer += clients[0].scratch_buffer
        assert got == await fresh.detect_activity(c2)         # ... and equals a fresh detection
        fresh.forget(c2)
        for c in clients:
            backend.forget(c)

    asyncio.run(scenario())
    backend.close()
