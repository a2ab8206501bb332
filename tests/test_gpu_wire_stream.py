"""GPU: wire streams (ttasr_vad_stream_open_wire / ttasr_vad_stream_push_wire, Engine.vad_stream_push_wire, DeviceStreamVAD(wire=)).

Every comparison is bit equality (`np.array_equal` on the uint32 views): an output's operands and their order depend on its index
alone, so however the bytes of a recording are cut into pushes, the concatenated PCM equals `Engine.ingest` of the whole recording
and the probabilities and logits equal `Engine.vad_probs` of that.  The cases and cuttings are those of
tests/wire_stream_reference.py."""
import asyncio
import ctypes as C

import numpy as np
import pytest

import wire_stream_reference as ws
from taiwan_tongues_asr_ce_amd import _lib, synth, vad
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError

pytestmark = pytest.mark.gpu

SEED = vad.SYNTH_SILERO_SEED
E_INVALID = -1
_engines = {}
_whole = {}


def _engine(max_batch=5):
    if max_batch not in _engines:
        e = Engine(PRESETS["micro"], COMPUTE_F32, max_batch)
        e.load_weights(synth.iter_weights(PRESETS["micro"]))
        e.load_vad(vad.synth_silero_weights(SEED))
        _engines[max_batch] = e
    return _engines[max_batch]


def _case(case):
    """(raw, pcm, probs, logits) of the whole recording through the offline calls, computed once per case."""
    if case not in _whole:
        rate, fmt, ch, pick, frames = case
        e = _engine()
        raw = ws.recording(rate, fmt, ch, frames)
        pcm = e.ingest([raw], [rate], [ch], [fmt], picks=[pick])[0]
        p, l = e.vad_probs([pcm], return_logits=True)
        _whole[case] = (raw, pcm, p[0], l[0])
    return _whole[case]


def _eq(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same(got, want):
    return all(_eq(a, b) for a, b in zip(got, want))


def _open(e, case):
    rate, fmt, ch, pick, _ = case
    return e.vad_stream_open(wire=(rate, ch, fmt, pick))


def _feed(e, sid, raw, cuts, finish=True):
    out, pos = ([], [], []), 0
    for j, k in enumerate(cuts):
        got = e.vad_stream_push_wire([sid], [raw[pos:pos + k]], finish=[finish and j == len(cuts) - 1], return_logits=True)
        pos += k
        for o, g in zip(out, got):
            o.append(g[0])
    assert pos == len(raw)
    return tuple(np.concatenate(o) for o in out)


def _cuttings(case):
    rate, fmt, ch, _, frames = case
    n = frames * ws.sample_bytes(fmt) * ch
    return [ws.fixed_cuts(rate, ch, fmt, n)] + [ws.random_cuts(n, seed) for seed in (1, 2, 3)]


_ids = lambda c: f"{c[0]}-{c[1]}-{c[2]}ch-pick{c[3]}"


# ---- 1. every cutting equals the offline calls ----

@pytest.mark.parametrize("case", ws.CASES, ids=_ids)
def test_every_cutting_equals_the_offline_calls(case):
    e = _engine()
    rate, fmt, ch, pick, frames = case
    raw, *want = _case(case)
    assert len(want[0]) == e.ingest_stream_len(rate, frames, True) == ws.final(rate, frames, True)
    sid = _open(e, case)
    for cuts in _cuttings(case):
        assert _same(_feed(e, sid, raw, cuts), want), cuts                        # finish: the stream is as reset afterwards
    # without finish: the first K(F) samples and the first K(F) // 512 values; a trailing byte that fills no frame stays pending
    K = e.ingest_stream_len(rate, frames)
    assert K == ws.final(rate, frames)
    extra = b"\x01" if ws.sample_bytes(fmt) * ch > 1 else b""
    cuts = _cuttings(case)[2]
    got = _feed(e, sid, raw + extra, cuts[:-1] + [cuts[-1] + len(extra)], finish=False)
    assert _same(got, (want[0][:K], want[1][:K // 512], want[2][:K // 512]))
    tail = e.vad_stream_push_wire([sid], [b""], finish=[True], return_logits=True)   # the rest, released by an empty finish
    assert _same([np.concatenate([g, t[0]]) for g, t in zip(got, tail)], want)
    e.vad_stream_close(sid)


# ---- 2. one call, three streams ----

def test_three_streams_of_different_formats_share_a_call_in_two_row_orders():
    e = _engine()
    cases = [ws.CASES[0], ws.CASES[4], ws.CASES[7]]                               # 8000 mu-law, 44100 s24 x 2, 192000 u8
    whole = [_case(c) for c in cases]
    ids = [_open(e, c) for c in cases]
    for order in ((0, 1, 2), (2, 0, 1)):
        cuts = [_cuttings(c)[1 + k] for k, c in enumerate(cases)]                 # seven pieces each, cut differently
        pos, got = [0] * 3, [([], [], []) for _ in cases]
        for j in range(7):
            rows = [k for k in order if not (j == 3 and k == 1)]                  # a stream sits out a call, and catches up
            take = [cuts[k][j] + (cuts[k][3] if j == 4 and k == 1 else 0) for k in rows]
            res = e.vad_stream_push_wire([ids[k] for k in rows], [whole[k][0][pos[k]:pos[k] + t] for k, t in zip(rows, take)],
                                         finish=[j == 6] * len(rows), return_logits=True)
            for r, (k, t) in enumerate(zip(rows, take)):
                pos[k] += t
                for o, g in zip(got[k], res):
                    o.append(g[r])
        for k in range(3):
            assert _same([np.concatenate(o) for o in got[k]], whole[k][1:]), (order, k)
    for i in ids:
        e.vad_stream_close(i)


# ---- 3. the internal chunk ----

@pytest.mark.parametrize("case", (ws.CASES[0], ws.CASES[3], ws.CASES[7]), ids=_ids)
def test_wire_chunk_does_not_change_a_bit(case):
    e = _engine()
    raw, *want = _case(case)
    sid = _open(e, case)
    H = ws.plan(case[0])[3]
    try:
        for chunk in (7, H + 3):
            e.set_option("wire_chunk", chunk)
            n = min(len(raw), 900 * ws.sample_bytes(case[1]) * case[2]) if chunk == 7 else len(raw)   # 7 frames a launch: a short piece
            got = _feed(e, sid, raw[:n], [n // 3, n - n // 3], finish=False)
            K = e.ingest_stream_len(case[0], n // (ws.sample_bytes(case[1]) * case[2]))
            assert _same(got, (want[0][:K], want[1][:K // 512], want[2][:K // 512])), chunk
            e.vad_stream_reset(sid)
    finally:
        e.set_option("wire_chunk", 0)
    e.vad_stream_close(sid)


def test_a_finish_whose_tail_exceeds_a_rows_share_of_the_pool_is_walked_without_new_frames():
    """256 rows at 16 Hz (up = 1000, down = 1, H = 20): a row's share of the result pool is 8 192 samples, so a chunk takes 8
    frames, and the 10 000 samples a finish releases behind the last frame come in two further chunks that bring no frames -
    they read the history the last frames left, and only the last of them carries the finish into the VAD."""
    e = _engine(64)
    rate, frames, rows = 16, 21, 256
    assert e.ingest_stream_len(rate, frames, True) - e.ingest_stream_len(rate, frames) == 10000 > (2 << 20) // rows
    recs = [np.random.default_rng([0x7A11, k]).integers(0, 256, frames, dtype=np.uint8).tobytes() for k in range(3)]
    pcm = e.ingest(recs, [rate] * 3, [1] * 3, [_lib.PCM_U8] * 3)
    p, l = e.vad_probs(pcm, return_logits=True)
    ids = [e.vad_stream_open(wire=(rate, 1, _lib.PCM_U8, -1)) for _ in range(rows)]
    head = e.vad_stream_push_wire(ids, [recs[k % 3][:5] for k in range(rows)], return_logits=True)
    tail = e.vad_stream_push_wire(ids, [recs[k % 3][5:] for k in range(rows)], finish=[True] * rows, return_logits=True)
    for k in range(rows):
        got = [np.concatenate([h[k], t[k]]) for h, t in zip(head, tail)]
        assert _same(got, (pcm[k % 3], p[k % 3], l[k % 3])), k
    for i in ids:
        e.vad_stream_close(i)


# ---- 4. reset, close, and float streams beside wire streams ----

def test_reset_close_and_float_streams_between_wire_pushes():
    e = _engine()
    case = ws.CASES[2]
    raw, *want = _case(case)
    sid = _open(e, case)
    e.vad_stream_push_wire([sid], [raw[:5001]])                                   # ends inside a sample
    e.vad_stream_reset(sid)
    assert _same(_feed(e, sid, raw, _cuttings(case)[1]), want)                    # a reset stream restarts cleanly
    x = want[0]                                                                   # any float32 PCM
    off = e.vad_probs([x], return_logits=True)
    fid = e.vad_stream_open()
    head = e.vad_stream_push([fid], [x[:1777]], return_logits=True)
    cuts = _cuttings(case)[2]
    mid = _feed(e, sid, raw, cuts[:4] + [sum(cuts[4:])])                          # wire pushes between the float stream's two
    tail = e.vad_stream_push([fid], [x[1777:]], finish=[True], return_logits=True)
    assert _same(mid, want)
    assert _same([np.concatenate([head[k][0], tail[k][0]]) for k in range(2)], [off[0][0], off[1][0]])
    with pytest.raises(TtasrError):
        e.vad_stream_push([sid], [x[:600]])                                       # a wire id in the float call
    with pytest.raises(TtasrError):
        e.vad_stream_push_wire([fid], [raw[:600]])                                # a float id in the wire call
    e.vad_stream_push_wire([sid], [raw[:4003]])
    e.vad_stream_close(sid)
    e.vad_stream_close(fid)
    again = e.vad_stream_open()                                                   # a closed wire id, reopened as a float stream
    assert again in (sid, fid)
    other = e.vad_stream_open()
    for i in (again, other):
        got = e.vad_stream_push([i], [x], finish=[True], return_logits=True)
        assert _same([got[0][0], got[1][0]], [off[0][0], off[1][0]])
        e.vad_stream_close(i)


# ---- 5. inside an open session ----

def test_a_wire_push_inside_an_open_session_leaves_its_tokens_alone():
    e = _engine()
    st = e.special
    n = PRESETS["micro"].n_frames * 160
    clips = [synth.noise_clip(60 + i, n) for i in range(6)]
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    caps = np.asarray([6, 14, 9, 12, 7, 10], dtype=np.int32)
    opts = e.gen_opts(14, False, suppress_eot=True, check_interval=1)
    case = ws.CASES[1]
    raw, *want = _case(case)
    sid = _open(e, case)
    cuts = ws.random_cuts(len(raw), 9, pieces=40)

    def run(with_pushes):
        toks, got, j = {}, ([], [], []), 0
        with e.session(opts, len(prompt)) as s:
            cids = s.submit(clips, [prompt] * len(clips), caps)
            if with_pushes:
                with pytest.raises(TtasrError):
                    e.vad_stream_open(wire=(8000, 1, _lib.PCM_ULAW, -1))          # an open may allocate: refused in a session
            while s.pending > 0:
                for r in s.poll(max_steps=1):
                    toks[cids.index(r.id)] = r.tokens
                if with_pushes and j < len(cuts) - 1:
                    res = e.vad_stream_push_wire([sid], [raw[sum(cuts[:j]):sum(cuts[:j + 1])]], return_logits=True)
                    j += 1
                    for o, g in zip(got, res):
                        o.append(g[0])
        return toks, got, j

    plain, _, _ = run(False)
    toks, got, j = run(True)
    assert j >= 5 and len(plain) == 6 and toks == plain
    res = e.vad_stream_push_wire([sid], [raw[sum(cuts[:j]):]], finish=[True], return_logits=True)
    assert _same([np.concatenate(o + [g[0]]) for o, g in zip(got, res)], want)
    e.vad_stream_close(sid)


# ---- 6. the backend on the device ----

class _Client:
    def __init__(self, cid):
        self.client_id, self.scratch_buffer, self.sampling_rate, self.samples_width, self.encoding = cid, bytearray(), 8000, 1, "ulaw"


def _ulaw_bytes(n, seed):
    """mu-law bytes that are loud for 0.4 s and near silence for 0.4 s, so the probabilities move"""
    rng = np.random.default_rng([0xFA4E, seed])
    quiet = rng.choice(np.array([0xFF, 0x7F, 0xFE, 0x7E], dtype=np.uint8), size=n)
    return np.where((np.arange(n) // 3200 + seed) % 2 == 0, rng.integers(0, 256, size=n, dtype=np.uint8), quiet).astype(np.uint8).tobytes()


def test_device_stream_vad_with_two_telephony_clients_end_to_end():
    from taiwan_tongues_asr_ce_amd.vad_backends import DEFAULT_STREAM_VAD_OPTIONS, VADFactory
    e = _engine()
    backend = VADFactory.create_vad_pipeline("mi355x_silero", engine=e, wire="client")
    options = vad.VadOptions(**DEFAULT_STREAM_VAD_OPTIONS)
    clients = [_Client("a"), _Client("b")]
    sig = [_ulaw_bytes(60000, 1), _ulaw_bytes(60000, 2)]
    steps = (12001, 12000, 11999, 12003)                                         # 1.5-s chunks at 8 kHz

    def expect(c):
        raw = bytes(c.scratch_buffer)
        audio = e.ingest([raw], [8000], [1], [_lib.PCM_ULAW])[0][:e.ingest_stream_len(8000, len(raw))]
        cut = audio[:len(audio) // 512 * 512]
        probs = e.vad_probs([cut])[0]
        chunks = vad.get_speech_timestamps(cut, options, lambda a: probs)
        return audio, [{"start": ch["start"] / 16000.0, "end": ch["end"] / 16000.0, "confidence": 1.0} for ch in chunks]

    async def scenario():
        pos = [0, 0]
        for step in steps:
            for k, c in enumerate(clients):
                c.scratch_buffer += sig[k][pos[k]:pos[k] + step]
                pos[k] += step
            got = await asyncio.gather(*(backend.detect_activity(c) for c in clients))
            for c, g in zip(clients, got):
                audio, segs = expect(c)
                assert g == segs and _eq(backend.audio(c, covering=bytes(c.scratch_buffer)), audio), (c.client_id, step)
        assert backend.pushes_run == [2] * len(steps)                            # the two clients share every push
        for c in clients:
            backend.forget(c)

    asyncio.run(scenario())
    backend.close()


# ---- 7. refusals ----

def _raw_push(e, ids, raws, n=None, nb="auto", cap="auto", got=True, pcm="auto", probs="auto", frames=True, null_raw=False):
    k = len(ids)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    idv = np.asarray(ids, dtype=np.int32)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in raws]
    nbv = np.asarray([len(b) for b in bufs] if nb == "auto" or nb is None else nb, dtype=np.int64)
    capv = np.asarray([4 * len(b) + 4096 for b in bufs] if cap == "auto" or cap is None else cap, dtype=np.int64)
    outs = [np.zeros(4 * len(b) + 4096, np.float32) for b in bufs]
    pr = [np.zeros(len(o) // 512 + 2, np.float32) for o in outs]
    ptrs = (C.c_void_p * k)(*[None if null_raw else b.ctypes.data for b in bufs])
    pptr = (C.c_void_p * k)(*[o.ctypes.data for o in outs]) if pcm == "auto" else pcm
    optr = (C.c_void_p * k)(*[p.ctypes.data for p in pr]) if probs == "auto" else probs
    ln, fr = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)
    return e.lib.ttasr_vad_stream_push_wire(e.h, k if n is None else n, idv.ctypes.data_as(i32p), ptrs,
                                            None if nb is None else nbv.ctypes.data_as(i64p), None, pptr,
                                            None if cap is None else capv.ctypes.data_as(i64p), ln.ctypes.data_as(i64p) if got else None,
                                            optr, None, fr.ctypes.data_as(i32p) if frames else None)


def test_refusals_leave_every_stream_as_it_was():
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    sid = C.c_int32(-1)
    assert e.lib.ttasr_vad_stream_open_wire(e.h, 8000, 1, _lib.PCM_ULAW, -1, C.byref(sid)) == E_INVALID   # VAD weights not finalized
    e.load_vad(vad.synth_silero_weights(SEED))
    case = ws.CASES[2]                                                            # 8000 s16 x 2
    raw, *want = _case(case)
    for args in ((8000, 1, _lib.PCM_IMA4, -1), (8000, 1, 9, -1), (8000, 0, _lib.PCM_S16, -1), (8000, 9, _lib.PCM_S16, -1),
                 (8000, 2, _lib.PCM_S16, 2), (8000, 2, _lib.PCM_S16, -2), (384000, 1, _lib.PCM_S16, -1), (0, 1, _lib.PCM_S16, -1)):
        assert e.lib.ttasr_vad_stream_open_wire(e.h, *args, C.byref(sid)) == E_INVALID, args
    assert e.lib.ttasr_vad_stream_open_wire(e.h, 8000, 1, _lib.PCM_S16, -1, None) == E_INVALID
    assert e.ingest_stream_len(384000, 10) < 0 and e.ingest_stream_len(16000 * 1024, 10) < 0 and e.ingest_stream_len(192000, 10) == 0
    assert _raw_push(e, [0], [raw[:800]]) == E_INVALID                            # no stream is open
    a, b, f = _open(e, case), _open(e, ws.CASES[0]), e.vad_stream_open()
    piece = raw[3001:6001]
    null1 = (C.c_void_p * 1)(None)
    refusals = [
        lambda: _raw_push(e, [a], [piece], n=0),
        lambda: _raw_push(e, [a, b, f, a], [piece] * 4),                          # n above the number of open streams
        lambda: e.lib.ttasr_vad_stream_push_wire(e.h, 1, None, None, None, None, None, None, None, None, None, None),
        lambda: _raw_push(e, [a], [piece], nb=None),                              # NULL n_bytes
        lambda: _raw_push(e, [a], [piece], got=False),                            # NULL out_pcm_len
        lambda: _raw_push(e, [a], [piece], frames=False),
        lambda: _raw_push(e, [a], [piece], probs=None),
        lambda: _raw_push(e, [a], [piece], probs=null1),                          # a NULL output row that would receive values
        lambda: _raw_push(e, [a], [piece], cap=[100]),                            # a capacity that is too small
        lambda: _raw_push(e, [a], [piece], cap=None),
        lambda: _raw_push(e, [f], [piece]),                                       # a float stream's id
        lambda: _raw_push(e, [b, f], [piece, piece]),
        lambda: _raw_push(e, [9], [piece]),                                       # an id that is not open
        lambda: _raw_push(e, [-1], [piece]),
        lambda: _raw_push(e, [a, a], [piece, piece]),                             # the same id twice
        lambda: _raw_push(e, [a], [piece], nb=[-1]),
        lambda: _raw_push(e, [a], [piece], null_raw=True),
        lambda: e.lib.ttasr_vad_stream_push(e.h, 1, (C.c_int32 * 1)(a), (C.c_void_p * 1)(want[0].ctypes.data), (C.c_int64 * 1)(600),
                                            None, (C.c_void_p * 1)(np.zeros(8, np.float32).ctypes.data), None, (C.c_int32 * 1)(0)),
    ]
    for k, refusal in enumerate(refusals):
        head = e.vad_stream_push_wire([a], [raw[:3001]], return_logits=True)      # a half-fed stream: history, a pending byte, VAD state
        assert refusal() == E_INVALID, k
        tail = e.vad_stream_push_wire([a], [raw[3001:]], finish=[True], return_logits=True)
        assert _same([np.concatenate([h[0], t[0]]) for h, t in zip(head, tail)], want), k
    assert _raw_push(e, [a], [piece], pcm=null1, cap=None) == 0                   # the samples need not be returned
    assert _raw_push(e, [a], [piece], pcm=None, cap=None) == 0
    for i in (a, b, f):
        e.vad_stream_close(i)
    assert _raw_push(e, [a], [piece]) == E_INVALID                                # closed
    e.close()
