"""CPU: the host audio reader (decode_audio, read_audio_coded, read_audio_raw, WireFormat.to_mono / to_16k, pcm16_bytes_to_float)
against tests/golden/audio_io_parent.json, the CRC32 and length of everything the commit BEFORE the reader moved into audio_io
returned for a seeded corpus of RIFF/WAVE files and wire buffers.  The reference is that commit, never the code under test:

    python tests/test_audio_io_host.py > tests/golden/audio_io_parent.json      (run at that commit)

Also: the three cases in which the single RIFF parser differs on purpose from the stdlib `wave` reader it replaced, and two bit
depths whose handling changed for files that were not read before; and that audio_io imports without the model
layer."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":          # run as a script to record the table: the package is one folder up
    sys.path.insert(0, os.path.dirname(HERE))

import ingest_reference as R  # noqa: E402
import telephony_reference as T  # noqa: E402
from taiwan_tongues_asr_ce_amd import asr, model, vad  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "audio_io_parent.json")
RATES = (8000, 11025, 16000, 44100, 48000)


def _crc(x):
    b = x if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x).tobytes()
    return [zlib.crc32(b), len(x)]


def _with_list_chunk(path):
    """Puts a `LIST` chunk of odd size (and its pad byte) in front of the file's `data` chunk."""
    with open(path, "rb") as f:
        blob = f.read()
    at = blob.index(b"data")
    blob = blob[:at] + b"LIST" + struct.pack("<I", 11) + b"INFOISFT\0ab" + b"\0" + blob[at:]
    with open(path, "wb") as f:
        f.write(blob[:4] + struct.pack("<I", len(blob) - 8) + blob[8:])


def _set_data_size(path, size):
    with open(path, "rb") as f:
        blob = f.read()
    at = blob.index(b"data")
    with open(path, "wb") as f:
        f.write(blob[:at + 4] + struct.pack("<I", size) + blob[at + 8:])


def write_corpus(folder):
    """The seeded files -> [(name, path, channels)], in a fixed order."""
    out = []

    def add(name, channels, writer, *args, **kw):
        path = os.path.join(str(folder), name + ".wav")
        writer(path, *args, **kw)
        out.append((name, path, channels))
        return path

    i = 0
    for fmt in range(6):                                   # the six PCM formats x channels x plain / EXTENSIBLE, the rates in turn
        for ch in (1, 2, 3):
            for ext in (False, True):
                rate, frames = RATES[i % 5], 257 + 13 * i
                add(f"pcm_f{fmt}_c{ch}_{'ext' if ext else 'plain'}_{rate}", ch, R.write_wav, R.signal(rate, frames, ch, fmt, i), rate, ch,
                    fmt, extensible=ext)
                i += 1
    for fmt in (T.ALAW, T.ULAW):                           # G.711
        for ch in (1, 2):
            for ext in (False, True):
                rate = RATES[i % 5]
                add(f"g711_{fmt}_c{ch}_{'ext' if ext else 'plain'}_{rate}", ch, T.write_wav, T.random_bytes((301 + i) * ch, i), rate, ch,
                    fmt, extensible=ext)
                i += 1
    for ba, ch in ((36, 1), (72, 2), (256, 1), (512, 2)):  # IMA ADPCM: two block sizes, mono and stereo; without `fact`, with a
        spb = T.ima_spb(ba, ch)                            # `fact` smaller than the blocks hold, and with one that is larger
        for fact, ext in ((None, False), (2 * spb + 5, False), (2 * spb + 5, True), (9 * spb, False)):
            rate = RATES[i % 5]
            add(f"ima_b{ba}_c{ch}_fact{fact}_{'ext' if ext else 'plain'}_{rate}", ch, T.write_wav, T.ima_stream(3, ch, ba, i, tail=5), rate,
                ch, T.IMA4, ba, fact=fact, extensible=ext)
            i += 1
    # a LIST chunk before data; an odd-sized data chunk with its pad byte; a trailing partial frame
    _with_list_chunk(add("list_s16_c2", 2, R.write_wav, R.signal(44100, 311, 2, R.S16, 900), 44100, 2, R.S16))
    _with_list_chunk(add("list_f32_c1_ext", 1, R.write_wav, R.signal(48000, 299, 1, R.F32, 901), 48000, 1, R.F32, extensible=True))
    _with_list_chunk(add("list_ulaw_c2", 2, T.write_wav, T.random_bytes(402, 902), 8000, 2, T.ULAW))
    add("odd_u8_c1", 1, R.write_wav, R.signal(11025, 301, 1, R.U8, 903), 11025, 1, R.U8)
    add("odd_s24_c1", 1, R.write_wav, R.signal(8000, 303, 1, R.S24, 904), 8000, 1, R.S24)
    add("odd_alaw_c1", 1, T.write_wav, T.random_bytes(333, 905), 8000, 1, T.ALAW)
    add("partial_s16_c2", 2, R.write_wav, R.signal(16000, 280, 2, R.S16, 906) + b"\x01\x02\x03", 16000, 2, R.S16)
    add("partial_s32_c2", 2, R.write_wav, R.signal(48000, 270, 2, R.S32, 907) + b"\x01\x02\x03\x04\x05", 48000, 2, R.S32)
    add("partial_f64_c3_ext", 3, R.write_wav, R.signal(44100, 260, 3, R.F64, 908) + b"\x07" * 11, 44100, 3, R.F64, extensible=True)
    add("partial_ulaw_c2", 2, T.write_wav, T.random_bytes(2 * 300 + 1, 909), 11025, 2, T.ULAW)
    return out


def wire_cases():
    """[(name, WireFormat, raw)]: every wire encoding x channels, the mean and a pick, the rates in turn, a partial frame at the end"""
    out, i = [], 0
    for enc, (code, width) in vad.WIRE_ENCODINGS.items():
        for ch, pick in ((1, None), (2, None), (2, "right"), (3, None), (3, 1)):
            rate, frames = RATES[i % 5], 263 + 7 * i
            raw = T.random_bytes(frames * ch, 1000 + i) if code >= 16 else R.signal(rate, frames, ch, code, 1000 + i)
            out.append((f"{enc}_c{ch}_pick{pick}_{rate}", vad.WireFormat(rate, ch, enc, pick), raw + b"\x55" * (width * ch - 1)))
            i += 1
    return out


def record(folder):
    """What the reader returns for the corpus -> {name: {what: [crc32, length] or the fields}}"""
    table = {}
    for name, path, ch in write_corpus(folder):
        c = model.read_audio_coded(path)
        r = model.read_audio_raw(path)
        row = {"decode": _crc(model.decode_audio(path)),
               "coded": _crc(bytes(c.samples)) + [int(v) for v in c[1:]],
               "raw": None if r is None else _crc(bytes(r[0])) + [int(v) for v in r[1:]]}
        for k in range(ch):
            row[f"channel{k}"] = _crc(model.decode_audio(path, channel=k))
        table["file:" + name] = row
    for name, w, raw in wire_cases():
        table["wire:" + name] = {"to_mono": _crc(w.to_mono(raw)), "to_16k": _crc(w.to_16k(raw))}
    table["pcm16_bytes_to_float"] = _crc(asr.pcm16_bytes_to_float(R.signal(16000, 777, 1, R.S16, 2000)))
    return table


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    return record(tmp_path_factory.mktemp("audio_io"))


def test_the_corpus_covers_what_it_should(got):
    names = [k for k in got if k.startswith("file:")]
    assert len(names) == 36 + 8 + 16 + 10 and len([k for k in got if k.startswith("wire:")]) == 40
    assert {int(n.rsplit("_", 1)[1]) for n in names if n.startswith(("file:pcm", "file:g711", "file:ima"))} == set(RATES)


def test_every_output_is_the_parent_commits(got):
    with open(GOLDEN, "r", encoding="utf-8") as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


# ---- where the single parser differs, on purpose, from the stdlib reader it replaced ----

def _s16_stereo(tmp_path, name, extra=b""):
    raw = R.signal(16000, 200, 2, R.S16, 3000)
    path = str(tmp_path / name)
    R.write_wav(path, raw + extra, 16000, 2, R.S16)
    return path, (np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0).reshape(-1, 2).mean(axis=1)


def test_a_data_size_of_zero_means_the_rest_of_the_file(tmp_path):
    path, want = _s16_stereo(tmp_path, "zero.wav")
    _set_data_size(path, 0)
    assert model.decode_audio(path).tobytes() == want.tobytes()
    assert model.read_audio_coded(path).n_frames == 200 == len(model.read_audio_raw(path)[0]) // 4


def test_a_data_size_beyond_the_file_is_trimmed_to_whole_frames(tmp_path):
    path, want = _s16_stereo(tmp_path, "long.wav", extra=b"\x01")      # one byte of a further frame, and the pad byte after it
    _set_data_size(path, 5000)
    assert model.decode_audio(path).tobytes() == want.tobytes()
    assert model.read_audio_coded(path).n_frames == 200 == len(model.read_audio_raw(path)[0]) // 4


def test_a_file_shorter_than_a_riff_header_is_a_value_error(tmp_path):
    path = str(tmp_path / "short.wav")
    with open(path, "wb") as f:
        f.write(b"RIFF\x04\0")            # the stdlib reader ended in EOFError inside the chunk header
    for fn in (model.decode_audio, model.read_audio_coded, model.read_audio_raw):
        with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
            fn(path)


def _odd_depth(path, bits, extensible=False):
    """Integer PCM, mono, 16 kHz, with a bit depth that fills its bytes only in part (or more than four of them)."""
    width = (bits + 7) // 8
    raw = R.signal(16000, 150, 1, R.S16, 3100) if width == 2 else bytes(150 * width)
    R.write_wav(path, raw, 16000, 1, R.S16, extensible=extensible)
    with open(path, "rb") as f:
        blob = bytearray(f.read())
    blob[32:36] = struct.pack("<HH", width, bits)           # block_align and bits per sample of the fmt chunk
    with open(path, "wb") as f:
        f.write(bytes(blob))
    return raw


def test_twelve_bit_samples_sit_in_two_bytes_plain_or_extensible(tmp_path):
    """The plain file read so through the stdlib reader; the EXTENSIBLE one was refused ("unsupported WAVE format tag 1, 12 bits")
    and now reads the same way."""
    for ext in (False, True):
        path = str(tmp_path / f"twelve{int(ext)}.wav")
        raw = _odd_depth(path, 12, ext)
        want = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
        assert model.decode_audio(path).tobytes() == want.tobytes()
        assert model.read_audio_raw(path) == (raw, 16000, 1, R.S16)
        assert model.read_audio_coded(path)[3:] == (R.S16, 2, 150)


def test_integer_samples_wider_than_four_bytes_are_refused_by_every_reader(tmp_path):
    """read_audio_raw / read_audio_coded returned None for these and decode_audio raised "unsupported sample width 5"."""
    path = str(tmp_path / "forty.wav")
    _odd_depth(path, 40)
    for fn in (model.decode_audio, model.read_audio_coded, model.read_audio_raw):
        with pytest.raises(ValueError, match="unsupported WAVE format tag 1, 40 bits"):
            fn(path)


def test_audio_io_imports_without_the_model_layer():
    code = ("import sys; import taiwan_tongues_asr_ce_amd.audio_io as a; p = 'taiwan_tongues_asr_ce_amd.'; "
            "bad = [m for m in ('model', 'vad', 'engine') if p + m in sys.modules]; assert not bad, bad; "
            "assert a.decode_audio and a.read_audio_coded and a.read_audio_raw and a.CodedAudio and a.parse_audio_channel")
    done = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        print(json.dumps(record(d), indent=0, sort_keys=True))
