"""GPU: file ingest on the device (ttasr_ingest_pcm, kernels_ingest.hip) against the float64 direct sum of
tests/ingest_reference.py, its bit-level contracts (rate 16000, chunking, batch independence), its index width, its refusals and
the facade (decode_audio_many, transcribe_many(device_resample=True)).

Bound (derived in ingest_reference.py, not measured): |y_dev - y_64| <= (T + C + 6) 2^-24 S_k per output.  Every check prints
its worst error / bound before it asserts."""
import ctypes as C

import numpy as np
import pytest

import ingest_reference as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
from taiwan_tongues_asr_ce_amd.engine import Engine, TtasrError

pytestmark = pytest.mark.gpu

E_INVALID = -1
_engines = {}


def _engine():
    """One micro context without weights, shared by the tests of this module: ingest needs none."""
    if "e" not in _engines:
        _engines["e"] = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    return _engines["e"]


def _inside(name, got, y, S, T, channels):
    """Asserts every output inside the bound; returns the worst error / bound."""
    assert got.dtype == np.float32 and got.shape == y.shape, (name, got.shape, y.shape)
    err, b = np.abs(got.astype(np.float64) - y), R.bound(S, T, channels)
    assert np.all(err[b == 0] == 0), name
    worst = float((err[b > 0] / b[b > 0]).max()) if np.any(b > 0) else 0.0
    print(f"ingest {name}: worst error / bound {worst:.3f} over {len(y)} outputs")
    assert worst <= 1.0, (name, worst)
    return worst


def _case_files(case):
    rate, fmt, ch = case
    return [R.cached_case(rate, fmt, ch, n) for n in R.lengths(rate)]


# ---- accuracy against float64 ----

@pytest.mark.parametrize("case", R.CASES + R.EXTREME_CASES, ids=lambda c: "r%d-f%d-c%d" % c)
def test_every_rate_format_and_channel_count(case):
    rate, fmt, ch = case
    files = _case_files(case)
    got = _engine().ingest([f[0] for f in files], [rate] * len(files), [ch] * len(files), [fmt] * len(files))
    for n, (raw, y, S, T), g in zip(R.lengths(rate), files, got):
        _inside(f"{case} n={n}", g, y, S, T, ch)


@pytest.mark.parametrize("fmt", range(6))
@pytest.mark.parametrize("ch", (1, 2))
def test_rate_16000_is_the_host_conversion_bit_for_bit(fmt, ch):
    raws = [R.signal(16000, n, ch, fmt, 3) for n in (1, 7, 4095, 4096, 4097, 9001)]
    got = _engine().ingest(raws, [16000] * len(raws), [ch] * len(raws), [fmt] * len(raws))
    for raw, g in zip(raws, got):
        assert g.tobytes() == R.host_convert(raw, fmt, ch).tobytes()


# ---- bit-level contracts ----

CHUNKED = ((44100, R.S16, 2), (48000, R.S24, 1), (11025, R.F32, 6), (192000, R.U8, 2), (16000, R.S16, 2))


def test_chunk_boundaries_change_no_bit():
    e = _engine()
    files = [(c, R.cached_case(c[0], c[1], c[2], 3 * 4099 + 17)) for c in CHUNKED]
    args = ([f[0] for _, f in files], [c[0] for c, _ in files], [c[2] for c, _ in files], [c[1] for c, _ in files])
    whole = e.ingest(*args)
    try:
        for chunk in (4099, 601):        # neither divisible by any `down`; 601 also puts several boundaries inside one tile
            e.set_option("ingest_chunk", chunk)
            parts = e.ingest(*args)
            for (c, (raw, y, S, T)), w, p in zip(files, whole, parts):
                assert p.tobytes() == w.tobytes(), (c, chunk)
                if c[0] != 16000:
                    _inside(f"{c} chunk {chunk}", p, y, S, T, c[2])
    finally:
        e.set_option("ingest_chunk", 0)


def test_batch_independence_and_repeatability():
    e = _engine()
    mix = [(8000, R.U8, 1, 5000), (96000, R.F64, 6, 7000), (44100, R.S16, 2, 30011), (16000, R.S32, 2, 4000), (22050, R.S24, 1, 9000)]
    raws = [R.cached_case(r, f, c, n)[0] for r, f, c, n in mix]
    args = (raws, [m[0] for m in mix], [m[2] for m in mix], [m[1] for m in mix])
    together = e.ingest(*args)
    again = e.ingest(*args)
    for a, b in zip(together, again):
        assert a.tobytes() == b.tobytes()
    alone = e.ingest([raws[2]], [mix[2][0]], [mix[2][2]], [mix[2][1]])[0]
    assert alone.tobytes() == together[2].tobytes()        # the 3rd of 5 mixed-rate files equals the file alone
    _, y, S, T = R.cached_case(*mix[2][:3], mix[2][3])
    _inside("3rd of 5", alone, y, S, T, mix[2][2])


def test_index_width_310_s_of_44100():
    """k * down passes 2^31 near the end of this recording (4 960 000 outputs x 441)."""
    rate, n = 44100, 310 * 44100
    rng = np.random.default_rng(0x310)
    raw = rng.integers(0, 256, size=n, dtype=np.uint8)
    got = _engine().ingest([raw], [rate], [1], [R.U8])[0]
    n_out = R.n_out(rate, n)
    assert len(got) == n_out and (n_out - 1) * 441 > 2 ** 31
    y, S, T = R.direct(rate, R.channels_f64(raw.tobytes(), R.U8, 1), n_out - 2000, n_out)
    _inside("310 s tail", got[-2000:], y, S, T, 1)


# ---- refusals ----

def _raw_call(e, raws, frames, rates, chans, fmts, outs):
    n = len(frames)
    i32p = C.POINTER(C.c_int32)
    f = np.asarray(frames, dtype=np.int64)
    r, c, m = (np.asarray(v, dtype=np.int32) for v in (rates, chans, fmts))
    ptrs = (C.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in raws])
    optr = (C.c_void_p * n)(*[o.ctypes.data if o is not None else None for o in outs])
    return e.lib.ttasr_ingest_pcm(e.h, n, ptrs, f.ctypes.data_as(C.POINTER(C.c_int64)), r.ctypes.data_as(i32p), c.ctypes.data_as(i32p),
                                  m.ctypes.data_as(i32p), optr)


def test_refusals_leave_the_context_usable():
    e = Engine(PRESETS["micro"], COMPUTE_F32, 4)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))      # only the open session below needs weights
    raw = np.frombuffer(R.cached_case(48000, R.S16, 2, 3000)[0], dtype=np.uint8)
    want = e.ingest([raw], [48000], [2], [R.S16])[0]
    out = np.zeros_like(want)

    def refused(rc):
        assert rc == E_INVALID
        assert len(e.lib.ttasr_last_error(e.h)) > 0
        assert e.ingest([raw], [48000], [2], [R.S16])[0].tobytes() == want.tobytes()     # a valid call afterwards succeeds

    refused(_raw_call(e, [raw], [3000], [44056], [2], [R.S16], [out]))      # a rate outside the accepted ratios
    refused(_raw_call(e, [raw], [3000], [48000], [0], [R.S16], [out]))      # 0 channels
    refused(_raw_call(e, [raw], [1000], [48000], [9], [R.U8], [out]))       # 9 channels
    refused(_raw_call(e, [raw], [3000], [48000], [2], [6], [out]))          # a bad format code
    refused(_raw_call(e, [raw], [3000], [48000], [2], [-1], [out]))
    refused(_raw_call(e, [None], [3000], [48000], [2], [R.S16], [out]))     # a NULL row with frames
    refused(_raw_call(e, [raw], [3000], [48000], [2], [R.S16], [None]))
    refused(_raw_call(e, [raw, raw], [3000, -1], [48000, 48000], [2, 2], [R.S16, R.S16], [out, out]))   # the 2nd row is bad: nothing ran
    with pytest.raises(TtasrError):
        e.ingest([raw], [44056], [2], [R.S16])
    assert not e.ingest_accepts(44056) and e.ingest_accepts(44100)
    with e.session(e.gen_opts(4, True), 4):
        assert _raw_call(e, [raw], [3000], [48000], [2], [R.S16], [out]) == E_INVALID      # an open session
        assert len(e.lib.ttasr_last_error(e.h)) > 0
    assert e.ingest([raw], [48000], [2], [R.S16])[0].tobytes() == want.tobytes()
    assert _raw_call(e, [None], [0], [48000], [2], [R.S16], [None]) == 0                   # an empty recording is legal
    e.close()


# ---- the facade, tiny geometry ----

def test_facade_decode_audio_many_and_transcribe_many(tmp_path):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel, decode_audio
    specs = ((48000, R.S16, 2, 48000 * 2 + 11), (44100, R.S24, 1, 44100 * 2 + 5), (16000, R.S16, 1, 16000 * 2 + 3))
    paths = []
    for i, (rate, fmt, ch, n) in enumerate(specs):
        paths.append(str(tmp_path / f"f{i}.wav"))
        R.write_wav(paths[-1], R.cached_case(rate, fmt, ch, n)[0], rate, ch, fmt, extensible=(i == 1))
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=4)
    try:
        extra = np.zeros(5, np.float32)
        got = m.decode_audio_many(paths + [extra])
        assert got[3] is extra or np.array_equal(got[3], extra)                # arrays pass through
        for (rate, fmt, ch, n), g in zip(specs[:2], got):
            _, y, S, T = R.cached_case(rate, fmt, ch, n)
            _inside(f"facade {rate}", g, y, S, T, ch)
        assert got[2].tobytes() == decode_audio(paths[2]).tobytes()            # 16 kHz: bit-equal to the host path
        kw = dict(language="zh", beam_size=2, temperature=0.0, log_prob_threshold=None, max_new_tokens=8)
        host = m.transcribe_many(paths, **kw)
        dev = m.transcribe_many(paths, device_resample=True, **kw)
        assert len(dev) == len(host) == len(paths)
        for (segs, info), (_, hinfo) in zip(dev, host):
            assert isinstance(segs, list) and info.duration == hinfo.duration
        segs, info = m.transcribe(paths[0], device_resample=True, **kw)
        assert info.duration == host[0][1].duration
    finally:
        m.close()
