"""GPU: coded WAVE data and the channel pick on the device (ttasr_ingest_wave, kernels_ingest.hip) against the S16 path.

The contract (include/ttasr.h): for every accepted recording the output equals, bit for bit, ttasr_ingest_pcm fed the decoded
int16 of the same data - with a pick, fed that one channel as a mono recording.  The int16 come from the plain-Python decoders of
tests/telephony_reference.py.  Every check here is an equality of bytes; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import ingest_reference as R
import telephony_reference as T
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine

pytestmark = pytest.mark.gpu

E_INVALID = -1
_engines = {}


def _engine():
    """One micro context without weights, shared by the tests of this module: ingest needs none."""
    if "e" not in _engines:
        _engines["e"] = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    return _engines["e"]


def _s16_reference(e, items):
    """items: (decoded int16 [frames][channels], rate, pick) -> what ttasr_ingest_pcm gives for each, in one call"""
    raws, rates, chans = [], [], []
    for x, rate, pick in items:
        x = x if pick is None or pick < 0 else x[:, pick:pick + 1]
        raws.append(np.ascontiguousarray(x).astype("<i2").tobytes())
        rates.append(rate)
        chans.append(x.shape[1])
    return e.ingest(raws, rates, chans, [R.S16] * len(items))


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, i, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, i, int(np.flatnonzero(g != w)[0]))


# ---- G.711 ----

@pytest.mark.parametrize("pick", ("mean", "first", "last"))
@pytest.mark.parametrize("fmt", (T.ULAW, T.ALAW), ids=("ulaw", "alaw"))
def test_g711_every_channel_count_rate_and_pick(fmt, pick):
    e = _engine()
    raws, rates, chans, picks, items = [], [], [], [], []
    for ch in T.G711_CHANNELS:
        for rate in T.G711_RATES:
            raw = T.random_bytes(T.G711_FRAMES * ch, 1000 * fmt + 10 * ch + rate % 7)
            p = {"mean": -1, "first": 0, "last": ch - 1}[pick]
            raws.append(raw), rates.append(rate), chans.append(ch), picks.append(p)
            items.append((T.decode(raw, fmt, ch), rate, p))
    got = e.ingest(raws, rates, chans, [fmt] * len(raws), picks=picks)
    _same(got, _s16_reference(e, items), (fmt, pick))
    assert any(np.any(g != 0) for g in got)


def test_g711_all_256_codes_at_16000_are_the_table():
    """At 16 kHz there is no filter: the outputs are the decoded samples / 32768 themselves."""
    codes = bytes(range(256))
    mu, a = _engine().ingest([codes, codes], [16000, 16000], [1, 1], [T.ULAW, T.ALAW])
    assert mu.tobytes() == (T.ULAW_TABLE.astype(np.float32) / 32768.0).tobytes()
    assert a.tobytes() == (T.ALAW_TABLE.astype(np.float32) / 32768.0).tobytes()


# ---- IMA ADPCM ----

_ima_cache = {}


def _ima_cases(block_align, ch):
    """Every frame count of the table for one block size: (raw, rate, frames, decoded int16), computed once."""
    key = (block_align, ch)
    if key not in _ima_cache:
        spb, out = T.ima_spb(block_align, ch), []
        for i, (frames, blocks, fact) in enumerate(T.ima_frame_counts(spb)):
            raw = T.ima_stream(blocks, ch, block_align, 100 * block_align + i, tail=(5 if i % 2 else 0))
            n = T.ima_frames(len(raw), ch, block_align, fact)
            assert n == frames
            out.append((raw, T.G711_RATES[(i + block_align // 36) % 4], n, T.ima_decode(raw, ch, block_align, n)))
        _ima_cache[key] = out
    return _ima_cache[key]


def _ima_call(e, cases, block_align, ch, pick=None):
    n = len(cases)
    return e.ingest([c[0] for c in cases], [c[1] for c in cases], [ch] * n, [T.IMA4] * n, block_aligns=[block_align] * n,
                    picks=None if pick is None else [pick] * n, n_frames=[c[2] for c in cases])


@pytest.mark.parametrize("block_align,ch", T.IMA_BLOCKS, ids=lambda v: str(v))
def test_ima_every_block_size_and_frame_count(block_align, ch):
    e = _engine()
    cases = _ima_cases(block_align, ch)
    for pick in (None,) + ((0, 1) if ch == 2 else ()):
        got = _ima_call(e, cases, block_align, ch, pick)
        _same(got, _s16_reference(e, [(c[3], c[1], pick) for c in cases]), (block_align, ch, pick))
    assert [len(g) for g in got] == [R.n_out(c[1], c[2]) for c in cases]


def test_ima_frame_count_defaults_to_the_whole_blocks():
    e = _engine()
    raw = T.ima_stream(3, 2, 72, 9, tail=71)
    got = e.ingest([raw], [8000], [2], [T.IMA4], block_aligns=[72])
    _same(got, _s16_reference(e, [(T.ima_decode(raw, 2, 72), 8000, None)]), "whole blocks")
    assert len(got[0]) == 2 * 195


@pytest.mark.parametrize("block_align,ch", ((36, 1), (72, 2), (256, 1)), ids=lambda v: str(v))
def test_ima_chunk_cuts_inside_blocks_change_no_bit(block_align, ch):
    """ingest_chunk = 100 frames: rounded up to whole blocks (130 frames of 65, one block of 505), so that the filter's halo and
    the cuts fall inside blocks."""
    e = _engine()
    spb = T.ima_spb(block_align, ch)
    raw = T.ima_stream(9, ch, block_align, 31)
    x = T.ima_decode(raw, ch, block_align)
    cases = [(raw, rate, n, x[:n]) for rate, n in ((8000, 9 * spb), (44100, 8 * spb + 3), (16000, 7 * spb + 1), (11025, 9 * spb - 1))]
    whole = _ima_call(e, cases, block_align, ch)
    _same(whole, _s16_reference(e, [(c[3], c[1], None) for c in cases]), "whole")
    try:
        e.set_option("ingest_chunk", 100)
        _same(_ima_call(e, cases, block_align, ch), whole, "chunk 100")
        if ch == 2:
            _same(_ima_call(e, cases, block_align, ch, 1), _s16_reference(e, [(c[3], c[1], 1) for c in cases]), "chunk 100, right")
    finally:
        e.set_option("ingest_chunk", 0)


def test_g711_chunk_boundaries_change_no_bit():
    e = _engine()
    raw = T.random_bytes(2 * 5003, 12)
    args = ([raw, raw], [8000, 44100], [2, 2], [T.ALAW, T.ULAW])
    whole = e.ingest(*args, picks=[1, -1])
    try:
        e.set_option("ingest_chunk", 601)
        _same(e.ingest(*args, picks=[1, -1]), whole, "chunk 601")
    finally:
        e.set_option("ingest_chunk", 0)
    _same(whole, _s16_reference(e, [(T.decode(raw, T.ALAW, 2), 8000, 1), (T.decode(raw, T.ULAW, 2), 44100, -1)]), "whole")


# ---- the call ----

def test_batch_independence_and_repeatability():
    e = _engine()
    ima = _ima_cases(512, 2)[4]
    mu = T.random_bytes(6 * 700, 40)
    pcm = R.cached_case(44100, R.S16, 2, 3001)[0]
    al = T.random_bytes(900, 41)
    args = dict(raws=[mu, pcm, ima[0], al], rates=[11025, 44100, ima[1], 8000], channels=[6, 2, 2, 1],
                formats=[T.ULAW, R.S16, T.IMA4, T.ALAW], block_aligns=[0, 0, 512, 0], picks=[5, None, 1, None],
                n_frames=[None, None, ima[2], None])
    together = e.ingest(**args)
    _same(e.ingest(**args), together, "again")
    alone = e.ingest([ima[0]], [ima[1]], [2], [T.IMA4], block_aligns=[512], picks=[1], n_frames=[ima[2]])
    _same(alone, together[2:3], "the 3rd of 4 alone")
    _same(e.ingest([pcm], [44100], [2], [R.S16]), together[1:2], "the PCM file through ttasr_ingest_pcm")
    rev = e.ingest(**{k: v[::-1] for k, v in args.items()})
    _same(rev[::-1], together, "reversed order")
    _same(together, _s16_reference(e, [(T.decode(mu, T.ULAW, 6), 11025, 5), (np.frombuffer(pcm, "<i2").reshape(-1, 2), 44100, None),
                                       (ima[3], ima[1], 1), (T.decode(al, T.ALAW, 1), 8000, None)]), "the S16 path")


def _wave_call(e, raw, n_bytes, frames, rate, ch, fmt, ba, pick, out, lib_fn="ttasr_ingest_wave"):
    i32, i64 = (lambda v: np.asarray([v], dtype=np.int32)), (lambda v: np.asarray([v], dtype=np.int64))
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    ptr, optr = (C.c_void_p * 1)(raw.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    a = dict(nb=i64(n_bytes), fr=i64(frames), rate=i32(rate), ch=i32(ch), fmt=i32(fmt), ba=i32(ba), pick=i32(pick))
    if lib_fn == "ttasr_ingest_pcm":
        return e.lib.ttasr_ingest_pcm(e.h, 1, ptr, a["fr"].ctypes.data_as(i64p), a["rate"].ctypes.data_as(i32p),
                                      a["ch"].ctypes.data_as(i32p), a["fmt"].ctypes.data_as(i32p), optr)
    return e.lib.ttasr_ingest_wave(e.h, 1, ptr, a["nb"].ctypes.data_as(i64p), a["fr"].ctypes.data_as(i64p), a["rate"].ctypes.data_as(i32p),
                                   a["ch"].ctypes.data_as(i32p), a["fmt"].ctypes.data_as(i32p), a["ba"].ctypes.data_as(i32p),
                                   a["pick"].ctypes.data_as(i32p), optr)


def test_refusals_leave_the_context_usable():
    e = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    raw = np.frombuffer(T.ima_stream(4, 2, 72, 50), dtype=np.uint8)          # 288 bytes: 4 stereo blocks, or 144 G.711 frames
    want = e.ingest([raw], [8000], [2], [T.IMA4], block_aligns=[72], picks=[1])[0]
    out = np.zeros(4096, dtype=np.float32)

    def refused(rc):
        assert rc == E_INVALID
        assert len(e.lib.ttasr_last_error(e.h)) > 0
        assert e.ingest([raw], [8000], [2], [T.IMA4], block_aligns=[72], picks=[1])[0].tobytes() == want.tobytes()

    ok = dict(n_bytes=288, frames=260, rate=8000, ch=2, fmt=T.IMA4, ba=72, pick=-1)

    def call(**kw):
        a = dict(ok, **kw)
        return _wave_call(e, raw, a["n_bytes"], a["frames"], a["rate"], a["ch"], a["fmt"], a["ba"], a["pick"], out)

    assert call() == 0
    refused(call(pick=2))                                  # a pick outside [-1, channels)
    refused(call(pick=-2))
    refused(call(fmt=T.ULAW, frames=144, pick=2))
    refused(call(ba=70))                                   # no multiple of 4 channels
    refused(call(ba=8, frames=1))                          # below 8 channels
    refused(call(ba=12, ch=2, frames=1))
    refused(call(ba=0))
    refused(call(frames=261))                              # more frames than the blocks hold
    refused(call(n_bytes=287))                             # ... than the bytes hold: 3 whole blocks
    refused(call(fmt=T.ULAW, frames=145))
    refused(call(fmt=R.S16, frames=73))
    refused(call(n_bytes=-1, frames=0))
    refused(call(fmt=6)), refused(call(fmt=19)), refused(call(fmt=-1))          # unknown format codes
    refused(call(rate=44056)), refused(call(ch=9, ba=72, frames=1)), refused(call(ch=0))
    for code in (6, T.ALAW, T.ULAW, T.IMA4):                # ttasr_ingest_pcm takes the six sample formats only
        refused(_wave_call(e, raw, 288, 10, 8000, 2, code, 72, -1, out, "ttasr_ingest_pcm"))
    assert call(fmt=T.ALAW, frames=144, pick=1) == 0
    e.close()


# ---- the facade, tiny geometry ----

def test_facade_decode_audio_many_and_transcribe_many(tmp_path):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel, decode_audio
    ima = T.ima_stream(40, 2, 512, 60)
    specs = ((T.ULAW, 2, 16000, T.random_bytes(2 * 16000, 61), 0, None), (T.IMA4, 2, 16000, ima, 512, 40 * 505 - 9),
             (T.ALAW, 1, 8000, T.random_bytes(8000, 62), 0, None))
    paths = []
    for i, (fmt, ch, rate, raw, ba, fact) in enumerate(specs):
        paths.append(str(tmp_path / f"f{i}.wav"))
        T.write_wav(paths[-1], raw, rate, ch, fmt, ba, fact=fact, extensible=(i == 0))
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=4)
    try:
        got = m.decode_audio_many(paths)
        for p, g in zip(paths[:2], got):
            assert g.tobytes() == decode_audio(p).tobytes()                # 16 kHz: bit-equal to the host path
        assert len(got[1]) == 40 * 505 - 9
        want = _s16_reference(m.engine, [(T.decode(specs[2][3], T.ALAW, 1), 8000, None)])
        assert got[2].tobytes() == want[0].tobytes()
        right = m.decode_audio_many(paths[:2], audio_channel="right")
        for p, g in zip(paths[:2], right):
            assert g.tobytes() == decode_audio(p, channel=1).tobytes()
        with pytest.raises(ValueError, match="1 channel"):
            m.decode_audio_many(paths, audio_channel="right")
        kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, max_new_tokens=8)
        host = m.transcribe_many(paths[:2], audio_channel="left", **kw)
        dev = m.transcribe_many(paths[:2], device_resample=True, audio_channel="left", **kw)
        assert len(dev) == len(host) == 2
        for (segs, info), (hsegs, hinfo) in zip(dev, host):
            assert info.duration == hinfo.duration and [s.text for s in segs] == [s.text for s in hsegs]   # the same samples
        with pytest.raises(ValueError, match="already mono"):
            m.transcribe(np.zeros(16000, np.float32), audio_channel="left", **kw)
    finally:
        m.close()
