"""GPU: FLAC recordings on the device (ttasr_ingest_wave with TTASR_PCM_FLAC; flac_decode_kernel in kernels_ingest.hip) against the
S16 / S32 path.

The contract (include/ttasr.h): for every accepted recording the output equals, bit for bit, ttasr_ingest_pcm fed the
left-justified integers of the stream as TTASR_PCM_S16 (bits <= 16) or TTASR_PCM_S32 - with a pick, fed that one channel as a
mono recording - whatever the chunk size, the other recordings of the call and its place in the call.  The integers come from the
case table of tests/flac_reference.py, whose writer never saw the decoder.  Every check is an equality of bytes.
The decode body the kernel runs is held clean under the sanitizers, on the host, by tests/test_flac_driver_host.py."""
import ctypes as C

import numpy as np
import pytest

import flac_reference as F
import ingest_reference as R
import telephony_reference as T
from taiwan_tongues_asr_ce_amd import _lib
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError

pytestmark = pytest.mark.gpu

E_INVALID = -1
_engines = {}
TABLE = tuple(n for n in sorted(F.CASES) if n != "largest_frame")          # (that one has a test of its own)


def _engine():
    """One micro context without weights, shared by the tests of this module: ingest needs none."""
    if "e" not in _engines:
        _engines["e"] = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    return _engines["e"]


def _pick_of(pick, ch):
    return {"mean": None, "first": 0, "last": ch - 1}[pick]


def _pcm_reference(e, items):
    """items: (integers [samples][channels], bits, rate, pick) -> ttasr_ingest_pcm of the left-justified integers, in one call"""
    raws, rates, chans, fmts = [], [], [], []
    for x, bits, rate, pick in items:
        x = x if pick is None or pick < 0 else x[:, pick:pick + 1]
        raws.append(np.ascontiguousarray(F.left_justified(x, bits)).tobytes())
        rates.append(rate), chans.append(x.shape[1]), fmts.append(R.S16 if bits <= 16 else R.S32)
    return e.ingest(raws, rates, chans, fmts)


def _flac_call(e, names, pick="mean", n_frames=None):
    cases = [F.case(n) for n in names]
    return e.ingest([c[0] for c in cases], [c[1] for c in cases], [c[3].shape[1] for c in cases], [F.FLAC] * len(cases),
                    picks=[_pick_of(pick, c[3].shape[1]) for c in cases], n_frames=n_frames)


def _items(names, pick="mean"):
    return [(F.case(n)[3], F.case(n)[2], F.case(n)[1], _pick_of(pick, F.case(n)[3].shape[1])) for n in names]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, i, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, i, int(np.flatnonzero(g != w)[0]))


@pytest.mark.parametrize("pick", ("mean", "first", "last"))
def test_the_case_table_equals_the_pcm_path(pick):
    e = _engine()
    got = _flac_call(e, TABLE, pick)
    _same(got, _pcm_reference(e, _items(TABLE, pick)), pick)
    assert [len(g) for g in got] == [R.n_out(F.case(n)[1], len(F.case(n)[3])) for n in TABLE]
    assert all(np.any(g != 0) for g in got)


def test_at_16000_the_outputs_are_the_integers():
    """16 kHz has no filter: a mono stream's outputs are v / 2^(bits - 1), a picked channel's too."""
    e = _engine()
    x12, x24 = F.case("escapes")[3], F.case("stereo_24bit")[3]
    got = _flac_call(e, ("escapes",))[0]
    assert got.tobytes() == (x12[:, 0].astype(np.float32) / np.float32(2048)).tobytes()
    got = _flac_call(e, ("stereo_24bit",), "last")[0]
    assert got.tobytes() == ((x24[:, 1] << 8).astype(np.float32) / np.float32(2147483648.0)).tobytes()


def test_the_largest_frame():
    """One frame of 65535 samples, verbatim and constant: one lane, 128 KiB of frame."""
    e = _engine()
    for pick in ("mean", "first"):
        _same(_flac_call(e, ("largest_frame",), pick), _pcm_reference(e, _items(("largest_frame",), pick)), pick)


@pytest.mark.parametrize("chunk", (300, 1000))
def test_chunk_edges_through_the_frame_table_change_no_bit(chunk):
    """ingest_chunk of a few hundred samples is rounded up to whole FLAC frames: chunks of one 576-sample frame, of nineteen
    16-sample frames, of the uneven frames of the variable stream - with the filter's halo reaching into the frames on both sides."""
    e = _engine()
    names = ("many_small", "variable", "stereo_16bit", "big_blocks", "partitions", "fixed_24bit_stereo", "odd_width_13", "tags", "ch8_12bit")
    whole = _flac_call(e, names)
    _same(whole, _pcm_reference(e, _items(names)), "whole")
    try:
        e.set_option("ingest_chunk", chunk)
        _same(_flac_call(e, names), whole, f"chunk {chunk}")
        _same(_flac_call(e, names, "last"), _pcm_reference(e, _items(names, "last")), f"chunk {chunk}, last channel")
    finally:
        e.set_option("ingest_chunk", 0)


def test_fewer_frames_than_held():
    e = _engine()
    names = ("variable", "stereo_16bit", "many_small", "lpc_24bit")
    counts = [len(F.case(n)[3]) - k for n, k in zip(names, (1, 577, 2239, 300))]
    got = _flac_call(e, names, n_frames=counts)
    want = _pcm_reference(e, [(x[:n], bits, rate, pick) for (x, bits, rate, pick), n in zip(_items(names), counts)])
    _same(got, want, "cut")
    try:
        e.set_option("ingest_chunk", 256)
        _same(_flac_call(e, names, n_frames=counts), want, "cut, chunk 256")
    finally:
        e.set_option("ingest_chunk", 0)
    assert len(_flac_call(e, ("variable",), n_frames=[0])[0]) == 0


def test_mixed_call_batch_independence_and_repeatability():
    e = _engine()
    ima_raw = T.ima_stream(5, 2, 512, 70)
    pcm = R.cached_case(44100, R.S16, 2, 3001)[0]
    fl = [F.case(n) for n in ("stereo_24bit", "variable", "lpc_16bit")]
    args = dict(raws=[fl[0][0], pcm, ima_raw, fl[1][0], fl[2][0]], rates=[fl[0][1], 44100, 8000, fl[1][1], fl[2][1]], channels=[2, 2, 2, 1, 2],
                formats=[F.FLAC, R.S16, T.IMA4, F.FLAC, F.FLAC], block_aligns=[0, 0, 512, 0, 0], picks=[1, None, 0, None, None],
                n_frames=[None] * 5)
    together = e.ingest(**args)
    _same(e.ingest(**args), together, "again")
    for i in (0, 3, 4):
        alone = e.ingest(**{k: v[i:i + 1] for k, v in args.items()})
        _same(alone, together[i:i + 1], f"recording {i} alone")
    _same(e.ingest([ima_raw], [8000], [2], [T.IMA4], block_aligns=[512], picks=[0]), together[2:3], "the IMA file alone")
    _same(e.ingest([pcm], [44100], [2], [R.S16]), together[1:2], "the PCM file through ttasr_ingest_pcm")
    rev = e.ingest(**{k: v[::-1] for k, v in args.items()})
    _same(rev[::-1], together, "reversed order")
    _same([together[0], together[3], together[4]],
          _pcm_reference(e, [(fl[0][3], 24, fl[0][1], 1), (fl[1][3], 16, fl[1][1], None), (fl[2][3], 16, fl[2][1], None)]), "the PCM path")


def test_tags_around_the_stream():
    """An ID3v2 tag, a padding block and an ID3v1 tail: the whole file goes in as read."""
    e = _engine()
    blob = F.case("tags")[0]
    assert blob[:3] == b"ID3" and blob[-128:-125] == b"TAG" and _lib.flac_probe(blob).first_frame == 456
    _same(_flac_call(e, ("tags",)), _pcm_reference(e, _items(("tags",))), "tags")


# ---- refusals ----

def _wave_call(e, raw, n_bytes, frames, rate, ch, fmt, pick, out, fn="ttasr_ingest_wave"):
    i32, i64 = (lambda v: np.asarray([v], dtype=np.int32)), (lambda v: np.asarray([v], dtype=np.int64))
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    ptr, optr = (C.c_void_p * 1)(raw.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    a = dict(nb=i64(n_bytes), fr=i64(frames), rate=i32(rate), ch=i32(ch), fmt=i32(fmt), ba=i32(0), pick=i32(pick))
    if fn == "ttasr_ingest_pcm":
        return e.lib.ttasr_ingest_pcm(e.h, 1, ptr, a["fr"].ctypes.data_as(i64p), a["rate"].ctypes.data_as(i32p), a["ch"].ctypes.data_as(i32p),
                                      a["fmt"].ctypes.data_as(i32p), optr)
    return e.lib.ttasr_ingest_wave(e.h, 1, ptr, a["nb"].ctypes.data_as(i64p), a["fr"].ctypes.data_as(i64p), a["rate"].ctypes.data_as(i32p),
                                   a["ch"].ctypes.data_as(i32p), a["fmt"].ctypes.data_as(i32p), a["ba"].ctypes.data_as(i32p),
                                   a["pick"].ctypes.data_as(i32p), optr)


def test_refusals_before_anything_is_enqueued_leave_the_context_usable():
    e = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    blob, rate, bits, x = F.case("stereo_16bit")
    raw = np.frombuffer(blob, dtype=np.uint8)
    want = e.ingest([blob], [rate], [2], [F.FLAC], picks=[1])[0]
    out = np.zeros(8192, dtype=np.float32)

    def refused(rc, message=None):
        assert rc == E_INVALID
        text = e.lib.ttasr_last_error(e.h).decode()
        assert text and (message is None or message in text), text
        assert e.ingest([blob], [rate], [2], [F.FLAC], picks=[1])[0].tobytes() == want.tobytes()      # a good call follows

    ok = dict(n_bytes=len(raw), frames=len(x), rate=rate, ch=2, fmt=F.FLAC, pick=-1)

    def call(buf=raw, **kw):
        a = dict(ok, **kw)
        return _wave_call(e, buf, a["n_bytes"], a["frames"], a["rate"], a["ch"], a["fmt"], a["pick"], out)

    assert call() == 0
    refused(call(rate=16000), "8000 Hz and 2 channels given as 16000 Hz")
    refused(call(ch=1), "given as 8000 Hz and 1 channels")
    refused(call(frames=len(x) + 1), "hold 2304")
    refused(call(pick=2)), refused(call(pick=-2))
    refused(call(n_bytes=len(raw) - 1), "CRC-16")                                  # the last frame is cut
    refused(call(fmt=19)), refused(call(fmt=33)), refused(call(fmt=31))            # 19 stays refused; 32 alone is FLAC
    refused(_wave_call(e, raw, len(raw), 10, rate, 2, F.FLAC, -1, out, "ttasr_ingest_pcm"))     # ttasr_ingest_pcm takes sample formats only
    for what, bad, message in F.refusals():
        buf = np.frombuffer(bad, dtype=np.uint8)
        refused(call(buf, n_bytes=len(buf), frames=1, rate=16000, ch=1), message)
    with pytest.raises(TtasrError, match="recording 0: FLAC: .*neither a frame nor an ID3v1 tag"):
        e.ingest([blob + b"junk!"], [rate], [2], [F.FLAC])                         # the facade raises with the library's message
    assert call(pick=0) == 0
    e.close()


def test_a_frame_that_fits_no_staging_slot_is_refused_before_anything_is_enqueued():
    """65535 samples at 800 Hz are 1 310 700 outputs, more than one result slot holds (2^20): the call is refused in the
    validation, with a good recording in front of it in the same call, and the next call is good."""
    e = _engine()
    good = _flac_call(e, ("variable",))
    x = np.full((65535, 1), 1234, dtype=np.int64)
    slow = F.encode(x, 800, 16, [65535], sub=lambda k, c: dict(kind="constant"))
    with pytest.raises(TtasrError, match=r"recording 1: FLAC frame 0 \(65535 samples at rate 800\) does not fit the staging slots"):
        e.ingest([F.case("variable")[0], slow], [44100, 800], [1, 1], [F.FLAC, F.FLAC])
    _same(_flac_call(e, ("variable",)), good, "the next call")
    assert len(e.ingest([slow], [800], [1], [F.FLAC], n_frames=[40000])[0]) == 800000       # what fits is taken


@pytest.mark.parametrize("kind", sorted(F.ILLEGAL))
def test_a_crc_valid_frame_with_illegal_content_fails_the_call_and_names_the_frame(kind):
    """The scan accepts these files (container, headers and CRCs are in order); the lane that decodes frame 1 finds the content
    illegal and says so in its status word.  The same bytes went through the same decode body under the sanitizers on the host."""
    e = _engine()
    good = _flac_call(e, ("variable",))
    bad = F.illegal(kind)
    with pytest.raises(TtasrError) as err:
        e.ingest([F.case("variable")[0], bad], [44100, 16000], [1, 1], [F.FLAC, F.FLAC])
    text = str(err.value)
    assert "(-1)" in text and "recording 1: FLAC frame 1: " in text and F.ILLEGAL[kind] in text, text
    _same(_flac_call(e, ("variable",)), good, "the next call")


def test_wire_streams_refuse_the_format():
    from taiwan_tongues_asr_ce_amd import vad
    e = Engine(PRESETS["micro"], COMPUTE_F32, 2)
    e.load_vad(vad.synth_silero_weights(3))
    sid = C.c_int32(-1)
    assert e.lib.ttasr_vad_stream_open_wire(e.h, 16000, 1, _lib.PCM_FLAC, -1, C.byref(sid)) == E_INVALID
    assert b"no stream format" in e.lib.ttasr_last_error(e.h)
    assert e.lib.ttasr_vad_stream_open_wire(e.h, 16000, 1, _lib.PCM_S16, -1, C.byref(sid)) == 0
    e.close()


# ---- the facade, tiny geometry ----

def test_facade_decode_audio_many_and_transcribe_many(tmp_path):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel, decode_audio
    names = ("stereo_24bit", "tags", "stereo_16bit")                          # 16 kHz, 16 kHz, 8 kHz
    paths = []
    for i, n in enumerate(names):
        paths.append(str(tmp_path / f"f{i}.flac"))
        open(paths[-1], "wb").write(F.case(n)[0])
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=4)
    try:
        got = m.decode_audio_many(paths)
        for p, g in zip(paths[:2], got):
            assert g.tobytes() == decode_audio(p).tobytes()                   # 16 kHz: bit-equal to the host path
        _same(got[2:], _pcm_reference(m.engine, _items(names[2:])), "8 kHz")
        right = m.decode_audio_many(paths, audio_channel="right")
        for p, g in zip(paths[:2], right):
            assert g.tobytes() == decode_audio(p, channel=1).tobytes()
        kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, max_new_tokens=8)
        host = m.transcribe_many(paths[:2], **kw)
        dev = m.transcribe_many(paths[:2], device_resample=True, **kw)
        for (segs, info), (hsegs, hinfo) in zip(dev, host):
            assert info.duration == hinfo.duration and [s.text for s in segs] == [s.text for s in hsegs]     # the same samples
    finally:
        m.close()
