"""CPU: the context-free entry points of the file ingest (ttasr_ingest_len, ttasr_ingest_filter: the library loads without a
GPU), model.read_audio_raw on WAVE files of every sample format, and decode_audio's outputs on those files, which this feature
must not change."""
import ctypes as C
import zlib

import numpy as np
import pytest

import ingest_reference as R
from taiwan_tongues_asr_ce_amd import _lib, model

# (format, channels, WAVE_FORMAT_EXTENSIBLE, crc32 of decode_audio's float32 output): 1 000 frames of R.signal(16000, ..., seed 7)
# at 16 kHz.  The checksums were recorded from decode_audio of the commit BEFORE the device ingest existed.
FILES = (
    (R.U8, 1, False, 0xc300fce4), (R.S16, 2, False, 0x049ff8e5), (R.S24, 1, False, 0x225f6a60), (R.S32, 2, False, 0x1b69fe4e),
    (R.F32, 1, False, 0xa6dace3c), (R.F64, 2, False, 0xbe5854a3), (R.S16, 6, True, 0xd7779b26), (R.S24, 2, True, 0x5512d8bd),
    (R.F32, 6, True, 0xea5f7ddc), (R.S16, 1, False, 0x84b27fd6), (R.S16, 6, False, 0xd7779b26),
)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_format_codes_match_the_header():
    assert (_lib.PCM_U8, _lib.PCM_S16, _lib.PCM_S24, _lib.PCM_S32, _lib.PCM_F32, _lib.PCM_F64) == (R.U8, R.S16, R.S24, R.S32, R.F32, R.F64)
    assert _lib.PCM_BYTES == R.BYTES


def test_ingest_len(lib):
    for rate in R.RATES + (16000,) + tuple(c[0] for c in R.EXTREME_CASES):
        for n in (0, 1, 2, 7, 159, 160, 441, 44100, 2 ** 31 + 5, 13_671_000):
            assert lib.ttasr_ingest_len(rate, n) == R.n_out(rate, n), (rate, n)
    for rate in (44056, 0, -16000, 16000 * 1025, 15999):
        assert not R.accepted(rate)
        assert lib.ttasr_ingest_len(rate, 100) < 0, rate
    assert lib.ttasr_ingest_len(48000, -1) < 0


@pytest.mark.parametrize("rate", R.RATES + tuple(c[0] for c in R.EXTREME_CASES))
def test_ingest_filter_is_the_float64_design(lib, rate):
    R_ = R.ratio(rate)[2]
    N = lib.ttasr_ingest_filter(rate, None, 0)
    assert N == 20 * R_ + 1
    got = np.full(N + 3, 7.0, dtype=np.float32)
    assert lib.ttasr_ingest_filter(rate, got.ctypes.data_as(C.POINTER(C.c_float)), N) == N
    assert np.all(got[N:] == 7.0)                      # nothing behind the taps is written
    short = np.full(8, 7.0, dtype=np.float32)
    assert lib.ttasr_ingest_filter(rate, short.ctypes.data_as(C.POINTER(C.c_float)), 5) == N
    assert np.all(short[:5] == got[:5]) and np.all(short[5:] == 7.0)
    h = R.design(rate)
    ulp = np.spacing(np.abs(h).astype(np.float32)).astype(np.float64)
    assert float((np.abs(got[:N].astype(np.float64) - h) / ulp).max()) <= 1.0
    assert abs(float(got[:N].astype(np.float64).sum()) - R.ratio(rate)[0]) < 1e-4     # DC gain = up


def test_ingest_filter_refusals(lib):
    assert lib.ttasr_ingest_filter(16000, None, 0) == 0     # no filter at the target rate
    for rate in (44056, 0, 16000 * 1025):
        assert lib.ttasr_ingest_filter(rate, None, 0) < 0


@pytest.mark.parametrize("fmt,ch,ext,crc", FILES, ids=lambda v: str(v))
def test_read_audio_raw_and_decode_audio_unchanged(tmp_path, fmt, ch, ext, crc):
    raw = R.signal(16000, 1000, ch, fmt, 7)
    path = str(tmp_path / "a.wav")
    R.write_wav(path, raw, 16000, ch, fmt, ext)
    want = model.decode_audio(path)
    assert want.dtype == np.float32 and want.shape == (1000,)
    assert zlib.crc32(want.tobytes()) == crc
    samples, rate, channels, code = model.read_audio_raw(path)
    assert bytes(samples) == raw and (rate, channels, code) == (16000, ch, fmt)
    assert R.host_convert(samples, code, channels).tobytes() == want.tobytes()


@pytest.mark.parametrize("rate,fmt,ch", ((48000, R.S16, 2), (44100, R.S24, 1), (8000, R.U8, 1)))
def test_decode_audio_resampled_files_unchanged(tmp_path, rate, fmt, ch):
    """At other rates decode_audio is its conversion followed by scipy's resample_poly in float64, as before."""
    from scipy.signal import resample_poly
    raw = R.signal(rate, 1000, ch, fmt, 7)
    path = str(tmp_path / "a.wav")
    R.write_wav(path, raw, rate, ch, fmt)
    up, down = R.ratio(rate)[:2]
    want = resample_poly(R.host_convert(raw, fmt, ch), up, down).astype(np.float32)
    assert model.decode_audio(path).tobytes() == want.tobytes()
    samples, r, c, code = model.read_audio_raw(path)
    assert bytes(samples) == raw and (r, c, code) == (rate, ch, fmt)


def test_read_audio_raw_other_containers(tmp_path):
    """Without soundfile (or for bytes it does not take) the caller is told to use decode_audio."""
    path = tmp_path / "a.flac"
    path.write_bytes(b"not audio")
    assert model.read_audio_raw(str(path)) is None


def test_decode_audio_many_without_and_with_an_ingesting_engine(tmp_path):
    """An engine without `ingest` (the oracle seam) sends every path through decode_audio; one with it gets every accepted file in
    ONE call and the files it does not take go through decode_audio."""
    paths = []
    for i, (rate, fmt, ch) in enumerate(((48000, R.S16, 2), (44056, R.S16, 1), (16000, R.S24, 1))):
        paths.append(str(tmp_path / f"f{i}.wav"))
        R.write_wav(paths[-1], R.signal(rate, 500, ch, fmt, i), rate, ch, fmt)
    m = model.WhisperModel.__new__(model.WhisperModel)
    m.engine = object()
    arr = np.arange(4, dtype=np.float32)
    plain = m.decode_audio_many(paths + [arr])
    for p, a in zip(paths, plain):
        assert a.tobytes() == model.decode_audio(p).tobytes()
    assert plain[3] is arr or np.array_equal(plain[3], arr)

    class Ingesting:
        calls = []

        def ingest_accepts(self, rate):
            return R.accepted(rate)

        def ingest(self, raws, rates, channels, formats):
            self.calls.append((list(rates), list(channels), list(formats)))
            return [np.full(R.n_out(r, len(bytes(b)) // (R.BYTES[f] * c)), 0.5, np.float32) for b, r, c, f in zip(raws, rates, channels, formats)]

    m.engine = Ingesting()
    got = m.decode_audio_many(paths)
    assert Ingesting.calls == [([48000, 16000], [2, 1], [R.S16, R.S24])]
    assert got[0].shape == (R.n_out(48000, 500),) and np.all(got[0] == 0.5) and got[2].shape == (500,)
    assert got[1].tobytes() == model.decode_audio(paths[1]).tobytes()      # 44 056 Hz: the host path


def test_batch_cli_has_the_flag():
    from taiwan_tongues_asr_ce_amd import batch_cli
    assert batch_cli.build_parser().parse_args(["folder", "--device-resample"]).device_resample is True
    assert batch_cli.build_parser().parse_args(["folder"]).device_resample is False
