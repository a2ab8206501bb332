"""CPU: the native FLAC reader through the built library (ttasr_flac_probe / ttasr_flac_frames / ttasr_flac_decode: no GPU) and
through audio_io, against the plain-Python reference of tests/flac_reference.py.  Everything is an equality of integers or bytes."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import flac_reference as F
import ingest_reference as R
from taiwan_tongues_asr_ce_amd import _lib, audio_io, batch_cli, model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac_rfc9639_example1.flac")


def test_the_code_and_the_symbols():
    assert _lib.PCM_FLAC == F.FLAC == 32
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "ttasr.h")).read()
    assert "#define TTASR_PCM_FLAC 32" in hdr
    for name in ("ttasr_flac_probe", "ttasr_flac_frames", "ttasr_flac_decode"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_probe_frames_and_decode_equal_the_reference(name):
    blob, rate, bits, x = F.case(name)
    d = F.read(blob)
    info = _lib.flac_probe(blob)
    assert (info.rate, info.channels, info.bits, info.samples) == (rate, x.shape[1], bits, len(x))
    assert (info.frames, info.max_blocksize, info.first_frame) == (len(d.frames), d.max_bs, d.first_frame)
    assert info.has_md5 and not info.total_disagrees
    assert [tuple(r) for r in _lib.flac_frames(blob).tolist()] == d.frames
    got, _ = _lib.flac_decode(blob)
    assert got.dtype == np.int32 and np.array_equal(got, d.samples) and np.array_equal(got, x)


def test_known_answer():
    blob = open(GOLDEN, "rb").read()
    info = _lib.flac_probe(blob)
    assert tuple(info) == (44100, 2, 16, 1, 1, 1, 42, 1)
    assert _lib.flac_frames(blob).tolist() == [[42, 15, 0]]
    assert _lib.flac_decode(blob)[0].tolist() == [[25588, 10416]]
    c = audio_io.read_audio_coded(GOLDEN)
    assert (c.rate, c.channels, c.format, c.block_align, c.n_frames) == (44100, 2, _lib.PCM_FLAC, 0, 1) and c.samples == blob
    assert audio_io.decode_coded(c).tolist() == [np.float32((25588 / 32768 + 10416 / 32768) / 2)]     # its MD5 holds


def test_frames_hook_capacity_and_null_arguments():
    lib = _lib.load()
    blob, _, _, x = F.case("many_small")
    b = np.frombuffer(blob, dtype=np.uint8)
    table = np.full((5, 3), -7, dtype=np.int64)
    why = C.create_string_buffer(200)
    assert lib.ttasr_flac_frames(b.ctypes.data, len(b), table.ctypes.data_as(C.POINTER(C.c_int64)), 4, why, 200) == 140
    assert table[:4].tolist() == [list(f) for f in F.read(blob).frames[:4]] and table[4].tolist() == [-7] * 3
    assert lib.ttasr_flac_frames(b.ctypes.data, len(b), None, 0, None, 0) == 140
    assert lib.ttasr_flac_frames(None, 10, None, 0, why, 200) < 0 and b"NULL" in why.value
    out = np.zeros((10, 2), dtype=np.int32)
    assert lib.ttasr_flac_decode(b.ctypes.data, len(b), out.ctypes.data_as(C.POINTER(C.c_int32)), 10, why, 200) < 0
    assert b"2240 samples" in why.value and not out.any()               # an output that is too small is not written
    assert lib.ttasr_flac_probe(b.ctypes.data, len(b), None, why, 200) != 0


# ---- refusals ----

@pytest.mark.parametrize("what,blob,message", list(F.refusals()), ids=[r[0] for r in F.refusals()])
def test_refusals_say_which_rule(what, blob, message):
    with pytest.raises(ValueError) as e:
        _lib.flac_probe(blob)
    assert message in str(e.value), str(e.value)
    for fn in (_lib.flac_frames, _lib.flac_decode):
        with pytest.raises(ValueError):
            fn(blob)
    with pytest.raises(F.FlacError):
        F.read(blob)                          # the reference refuses it too


def test_what_is_not_refused():
    good = F.three()
    assert _lib.flac_probe(F.stream_of(F.three(numbers=(70000, 70001, 70002)))).samples == 96         # the first frame may start anywhere
    assert _lib.flac_probe(F.write_stream(good, 16000, 1, 16, 0)).total_disagrees is False      # total 0 = unknown
    short = F.write_stream(good[:2], 16000, 1, 16, 96)
    info = _lib.flac_probe(short)
    assert info.samples == 64 and info.total_disagrees and not info.has_md5                      # the samples held, not the claim
    assert _lib.flac_probe(F.stream_of([])).samples == 0 and _lib.flac_decode(F.stream_of([]))[0].shape == (0, 1)
    assert _lib.flac_probe(F.stream_of(good, id3v1=True)).samples == 96


def test_truncation_at_every_byte():
    """Every prefix of a small file is refused or decodes a whole-frame prefix of the samples."""
    blob, _, _, x = F.case("rate_codes")
    ends = {42: 0}                            # the byte behind the metadata: no frame, no sample
    ends.update({off + size: first + 100 for off, size, first in F.read(blob).frames})
    decoded = 0
    for n in range(len(blob)):
        try:
            got, info = _lib.flac_decode(blob[:n])
        except ValueError:
            assert n not in ends, n
            continue
        assert n in ends, n
        assert info.samples == len(got) == ends[n] and np.array_equal(got, x[:len(got)])
        decoded += 1
    assert decoded == 3                       # the bare metadata, one frame, two frames


@pytest.mark.parametrize("kind", sorted(F.ILLEGAL))
def test_crc_valid_frames_with_illegal_content(kind):
    blob = F.illegal(kind)
    info = _lib.flac_probe(blob)              # the container and the CRCs are in order
    assert (info.samples, info.frames) == (96, 3)
    with pytest.raises(ValueError) as e:
        _lib.flac_decode(blob)
    assert "frame 1 at byte" in str(e.value) and F.ILLEGAL[kind] in str(e.value), str(e.value)


# ---- audio_io ----

def _wav_of(path, x, rate, bits):
    lj = F.left_justified(x, bits)
    R.write_wav(path, lj.astype("<i2" if bits <= 16 else "<i4").tobytes(), rate, x.shape[1], R.S16 if bits <= 16 else R.S32)


@pytest.mark.parametrize("name", ("stereo_16bit", "stereo_24bit", "ch8_12bit", "odd_width_13", "fixed_8bit_mono", "ch3_20bit", "tags"))
def test_decode_audio_equals_the_wave_file_of_the_same_integers(tmp_path, name):
    blob, rate, bits, x = F.case(name)
    flac, wav = str(tmp_path / "a.flac"), str(tmp_path / "a.wav")
    open(flac, "wb").write(blob)
    _wav_of(wav, x, rate, bits)
    assert model.decode_audio(flac).tobytes() == model.decode_audio(wav).tobytes()              # 16 kHz or resampled
    last = x.shape[1] - 1
    assert model.decode_audio(flac, channel=last).tobytes() == model.decode_audio(wav, channel=last).tobytes()
    with pytest.raises(ValueError, match="channel"):
        model.decode_audio(flac, channel=x.shape[1])
    c = model.read_audio_coded(flac)
    assert (bytes(c.samples), c.rate, c.channels, c.format, c.block_align, c.n_frames) == (blob, rate, x.shape[1], _lib.PCM_FLAC, 0, len(x))
    assert model.read_audio_raw(flac) is None
    v, b = audio_io.flac_to_int(c)
    assert b == bits and np.array_equal(v, x)


def test_flac_is_found_by_content_and_other_bytes_still_go_on(tmp_path):
    blob, rate, bits, x = F.case("escapes")
    odd = str(tmp_path / "a.mp3")             # whatever the name says
    open(odd, "wb").write(blob)
    assert model.read_audio_coded(odd).format == _lib.PCM_FLAC
    tagged = str(tmp_path / "b.flac")
    open(tagged, "wb").write(F.case("tags")[0])
    assert model.read_audio_coded(tagged).n_frames == 768
    junk = tmp_path / "c.flac"
    junk.write_bytes(b"not audio")
    assert model.read_audio_coded(str(junk)) is None and model.read_audio_coded(str(tmp_path / "missing.flac")) is None
    id3_only = tmp_path / "d.mp3"
    id3_only.write_bytes(b"ID3\x04\x00\x00\x00\x00\x00\x04abcd\xff\xfb\x90\x00")
    assert model.read_audio_coded(str(id3_only)) is None
    bad = str(tmp_path / "e.flac")
    open(bad, "wb").write(blob[:-1])
    for fn in (model.read_audio_coded, model.decode_audio):
        with pytest.raises(ValueError, match="CRC-16"):
            fn(bad)


def test_md5_is_checked(tmp_path):
    blob, rate, bits, x = F.case("escapes")
    wrong = bytearray(blob)
    wrong[4 + 4 + 18] ^= 1                    # the first byte of STREAMINFO's MD5
    path = str(tmp_path / "a.flac")
    open(path, "wb").write(bytes(wrong))
    c = model.read_audio_coded(path)          # the probe does not decode
    with pytest.raises(ValueError, match="MD5"):
        audio_io.decode_coded(c)
    with pytest.raises(ValueError, match="MD5"):
        model.decode_audio(path)
    assert audio_io.decode_coded(c, verify_md5=False).tobytes() == audio_io.decode_coded(model.CodedAudio(blob, *c[1:])).tobytes()
    none = F.encode(x, rate, bits, [192] * 3, md5=False)
    assert not _lib.flac_probe(none).has_md5
    assert audio_io.decode_coded(model.CodedAudio(none, *c[1:])).shape == (576,)


def test_decode_audio_many_hands_flac_to_an_ingesting_engine(tmp_path):
    specs = ("stereo_16bit", "lpc_24bit", "rate_codes")
    paths = []
    for i, name in enumerate(specs):
        paths.append(str(tmp_path / f"f{i}.flac"))
        open(paths[-1], "wb").write(F.case(name)[0])
    wav = str(tmp_path / "g.wav")
    R.write_wav(wav, R.signal(48000, 300, 2, R.S16, 3), 48000, 2, R.S16)
    m = model.WhisperModel.__new__(model.WhisperModel)
    m.engine = object()
    for p, a in zip(paths, m.decode_audio_many(paths)):
        assert a.tobytes() == model.decode_audio(p).tobytes()                  # no ingest: the host path

    class Ingesting:
        calls = []

        def ingest_accepts(self, rate):
            return R.accepted(rate)

        def ingest(self, raws, rates, channels, formats, block_aligns=None, picks=None, n_frames=None):
            self.calls.append((list(rates), list(channels), list(formats), list(block_aligns), list(picks), list(n_frames)))
            assert [bytes(r) for r in raws[:3]] == [F.case(n)[0] for n in specs]
            return [np.full(R.n_out(r, n), 0.25, np.float32) for r, n in zip(rates, n_frames)]

    m.engine = Ingesting()
    got = m.decode_audio_many(paths + [wav], audio_channel=None)
    assert Ingesting.calls == [([8000, 44100, 11000, 48000], [2, 2, 1, 2], [F.FLAC] * 3 + [R.S16], [0, 0, 0, 4], [None] * 4, [2304, 768, 300, 300])]
    assert [len(g) for g in got] == [R.n_out(8000, 2304), R.n_out(44100, 768), R.n_out(11000, 300), 100]


def test_batch_cli_folder_with_a_flac_file(tmp_path, monkeypatch):
    class Seg:
        def __init__(self, text):
            self.text = text

    class Model:
        calls = []

        def transcribe(self, audio, **kw):
            self.calls.append(len(audio))
            return iter([Seg(f"長{len(audio)}")]), object()

    monkeypatch.chdir(tmp_path)
    folder = tmp_path / "audio"
    folder.mkdir()
    blob, rate, bits, x = F.case("stereo_24bit")               # 2304 samples at 16 kHz
    (folder / "a.flac").write_bytes(blob)
    (folder / "c.flac").write_bytes(blob[:-3])                 # a damaged one is that file's error
    with wave.open(str(folder / "b.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(np.zeros(500, dtype="<i2").tobytes())
    assert "*.flac" in batch_cli.AUDIO_PATTERNS
    final = batch_cli.process_audio_folder(str(folder), model=Model(), log=lambda *_: None)
    a, b, c = final["detailed_results"]
    assert Model.calls == [2304, 500]
    assert (a["audio_file"], a["asr_result"]) == ("a.flac", "長2304") and "error" not in a
    assert c["asr_result"] is None and "CRC-16" in c["error"]
