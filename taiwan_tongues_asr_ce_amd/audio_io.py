"""Audio input on the host: the one RIFF/WAVE parser, the native FLAC reader (the library's ttasr_flac_* functions), the one
bytes -> float32 sample conversion (the definition that csrc/kernels_ingest.hip and include/ttasr.h restate for the device),
the one host resampler, and the readers built from them -
`read_audio_coded` / `read_audio_raw` for the device ingest (Engine.ingest) and `decode_audio` for the host path.  Nothing here
needs the model layer, the engine or a GPU."""
from __future__ import annotations

import struct
from math import gcd
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from .config import SAMPLE_RATE

WAVE_PCM, WAVE_FLOAT, WAVE_ALAW, WAVE_ULAW, WAVE_IMA_ADPCM = 1, 3, 6, 7, 0x11      # the format tags this reader takes
# (format tag, bytes per sample) -> the _lib.PCM_* code of the samples
_PCM_FORMATS = {(WAVE_PCM, 1): _lib.PCM_U8, (WAVE_PCM, 2): _lib.PCM_S16, (WAVE_PCM, 3): _lib.PCM_S24, (WAVE_PCM, 4): _lib.PCM_S32,
                (WAVE_FLOAT, 4): _lib.PCM_F32, (WAVE_FLOAT, 8): _lib.PCM_F64}

_IMA_INDEX = np.array([-1, -1, -1, -1, 2, 4, 6, 8], dtype=np.int32)
_IMA_STEP = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
    11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], dtype=np.int32)


def _pick_channel(path: str, channel: Optional[int], n_ch: int) -> Optional[int]:
    if channel is None:
        return None
    if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)) or not 0 <= channel < n_ch:
        raise ValueError(f"{path}: channel {channel!r} asked of a file with {n_ch} channel{'s' if n_ch != 1 else ''} "
                         f"(0 ... {n_ch - 1}, or None for their mean)")
    return int(channel)


def parse_audio_channel(value) -> Optional[int]:
    """The `audio_channel` option in its spellings -> None (the mean of the channels) or a channel index from 0: None / "mix" /
    "left" / "right" / an index.  The reference's service field audioChannel maps as 0 -> "mix", 1 -> "left", 2 -> "right"."""
    if value is None or value == "mix":
        return None
    if value in ("left", "right"):
        return 0 if value == "left" else 1
    if isinstance(value, str) and value.isdigit():
        return int(value)
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool) and value >= 0:
        return int(value)
    raise ValueError(f"audio_channel {value!r}: expected None, 'mix', 'left', 'right' or a channel index from 0")


def _g711_table(mu_law: bool) -> np.ndarray:
    """The 256 int16 values of a G.711 law, from the formulas of include/ttasr.h."""
    b = np.arange(256, dtype=np.int32)
    if mu_law:
        u = ~b & 0xFF
        v = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
        return np.where(u & 0x80, -v, v).astype(np.int16)
    a = b ^ 0x55
    e, v = (a >> 4) & 7, ((a & 15) << 4) + 8
    v = np.where(e >= 1, (v + 0x100) << np.maximum(e - 1, 0), v)
    return np.where(a & 0x80, v, -v).astype(np.int16)


def _ima_decode(data: bytes, n_ch: int, block_align: int, n_frames: int) -> np.ndarray:
    """IMA ADPCM blocks -> int16 [n_frames][n_ch] (include/ttasr.h has the definition): every block and channel at once, one
    loop over the samples of a block."""
    per = block_align // n_ch - 4                        # data bytes of one channel in a block
    spb, blocks = 1 + 2 * per, len(data) // block_align
    b = np.frombuffer(data, dtype=np.uint8, count=blocks * block_align).reshape(blocks, block_align)
    head = b[:, :4 * n_ch].reshape(blocks, n_ch, 4).astype(np.int32)
    pred = ((head[..., 0] | (head[..., 1] << 8)) ^ 0x8000) - 0x8000
    index = np.minimum(head[..., 2], 88)
    body = b[:, 4 * n_ch:].reshape(blocks, per // 4, n_ch, 4).transpose(0, 2, 1, 3).reshape(blocks, n_ch, per)
    nib = np.empty((blocks, n_ch, 2 * per), dtype=np.int32)
    nib[..., 0::2], nib[..., 1::2] = body & 15, body >> 4          # low nibble first
    out = np.empty((blocks, spb, n_ch), dtype=np.int16)
    out[:, 0] = pred
    for k in range(spb - 1):
        n, step = nib[..., k], _IMA_STEP[index]
        d = (step >> 3) + np.where(n & 4, step, 0) + np.where(n & 2, step >> 1, 0) + np.where(n & 1, step >> 2, 0)
        pred = np.clip(np.where(n & 8, pred - d, pred + d), -32768, 32767)
        index = np.clip(index + _IMA_INDEX[n & 7], 0, 88)
        out[:, k + 1] = pred
    return out.reshape(blocks * spb, n_ch)[:n_frames]


def samples_to_float(raw, fmt: int, channels: int = 1) -> np.ndarray:
    """Interleaved little-endian samples of one of the six PCM_* sample formats or a G.711 law -> float32 [frames], or
    [frames][channels] for more than one channel: the integer formats scaled by a power of two, 32-bit integers and doubles
    rounded to float32, G.711 through the int16 it stands for."""
    if fmt in (_lib.PCM_ALAW, _lib.PCM_ULAW):
        x = _g711_table(fmt == _lib.PCM_ULAW)[np.frombuffer(raw, dtype=np.uint8)].astype(np.float32) / 32768.0
    elif fmt == _lib.PCM_U8:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif fmt == _lib.PCM_S16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif fmt == _lib.PCM_S24:      # little endian: sign-extend through the top byte of an int32
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        x = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8 >> 8).astype(np.float32) / 8388608.0
    elif fmt == _lib.PCM_S32:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif fmt in (_lib.PCM_F32, _lib.PCM_F64):
        x = np.frombuffer(raw, dtype="<f4" if fmt == _lib.PCM_F32 else "<f8").astype(np.float32)
    else:
        raise ValueError(f"sample format {fmt} is none of the PCM_* sample formats or G.711 laws")
    return x if channels == 1 else x.reshape(-1, channels)


def downmix(x: np.ndarray, channel: Optional[int]) -> np.ndarray:
    """float32 [frames] or [frames][channels] -> [frames]: the float32 mean of the channels, or one of them."""
    if x.ndim == 1:
        return x
    return x.mean(axis=1) if channel is None else x[:, channel]


def resample(x: np.ndarray, rate: int, sampling_rate: int = SAMPLE_RATE) -> np.ndarray:
    """Mono samples at `rate` -> contiguous float32 at `sampling_rate`: scipy's polyphase resampler over the whole array."""
    if rate != sampling_rate:
        from scipy.signal import resample_poly
        g = gcd(rate, sampling_rate)
        x = resample_poly(x, sampling_rate // g, rate // g)
    return np.ascontiguousarray(x, dtype=np.float32)


class CodedAudio(NamedTuple):
    """What Engine.ingest needs of one file: the data bytes as the file has them, format = the _lib.PCM_* code (the six sample
    formats, PCM_ALAW, PCM_ULAW, PCM_IMA4), block_align = bytes per frame, or per block for IMA, n_frames = the frames the bytes
    hold (IMA: what `fact` says when that is less).  A FLAC file is format PCM_FLAC: samples = the whole file as read (tags and
    metadata included), block_align = 0, n_frames = the samples per channel its frames hold."""
    samples: bytes
    rate: int
    channels: int
    format: int
    block_align: int
    n_frames: int


def _parse_riff(path: str):
    """(tag, channels, rate, bits, block_align, data bytes, `fact` sample count or None) of a RIFF/WAVE file; EXTENSIBLE resolved
    to its sub-format."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data, fact = 12, None, None, None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"fact" and len(body) >= 4:
            fact = struct.unpack("<I", body[:4])[0]
        elif cid == b"data":
            data = body            # (a streamed file's size field of 0 / 0xFFFFFFFF: the slice is whatever is there)
            if size in (0, 0xFFFFFFFF):
                data = blob[pos + 8:]
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None or len(fmt) < 16:
        raise ValueError(f"{path}: RIFF/WAVE without fmt / data chunk")
    tag, n_ch, sr, _, block_align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]          # first two bytes of the sub-format GUID
    return tag, n_ch, sr, bits, block_align, data, fact


def _id3v2_size(head: bytes) -> int:
    """Bytes of the ID3v2 tag that the first ten bytes of a file announce, header and footer included; 0: no such tag."""
    if len(head) < 10 or head[:3] != b"ID3":
        return 0
    return 10 + ((head[6] & 0x7F) << 21 | (head[7] & 0x7F) << 14 | (head[8] & 0x7F) << 7 | (head[9] & 0x7F)) + (10 if head[5] & 0x10 else 0)


def _flac_marker(blob: bytes) -> int:
    """Byte offset of the "fLaC" marker of a file that begins with it, or with an ID3v2 tag followed by it; -1: not FLAC."""
    pos = _id3v2_size(blob[:10])
    return pos if blob[pos:pos + 4] == b"fLaC" else -1


def _read_flac(path: str) -> Optional[CodedAudio]:
    """CodedAudio of a file whose content is FLAC; None for a missing file or other bytes; ValueError for damaged FLAC.  Only a
    file that has the marker is read whole: of a tagged file of another kind, the ten bytes of the tag's header and four behind
    the tag."""
    try:
        with open(path, "rb") as f:
            pos = _id3v2_size(f.read(10))
            f.seek(pos)
            if f.read(4) != b"fLaC":
                return None
            f.seek(0)
            blob = f.read()
    except OSError:
        return None
    try:
        info = _lib.flac_probe(blob)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    return CodedAudio(blob, info.rate, info.channels, _lib.PCM_FLAC, 0, info.samples)


def flac_to_int(c: CodedAudio, verify_md5: bool = True):
    """A PCM_FLAC CodedAudio -> (int32 [frames][channels] plain integers, bits per sample), decoded by the library on the host.
    verify_md5: when STREAMINFO carries an MD5 it is checked against the decoded samples (interleaved, little-endian signed
    numbers of ceil(bits / 8) bytes); a mismatch is a ValueError."""
    blob = c.samples if isinstance(c.samples, (bytes, bytearray)) else bytes(c.samples)
    x, info = _lib.flac_decode(blob)
    if verify_md5 and info.has_md5:
        import hashlib
        at = _flac_marker(blob) + 8 + 18            # the marker, STREAMINFO's block header, the 18 bytes in front of its MD5
        width = (info.bits + 7) // 8
        le = x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width]
        if hashlib.md5(np.ascontiguousarray(le).tobytes()).digest() != bytes(blob[at:at + 16]):
            raise ValueError("FLAC: the MD5 of the decoded samples is not the one in STREAMINFO")
    return x[:c.n_frames], info.bits


def read_audio_coded(path: str) -> Optional[CodedAudio]:
    """Path -> CodedAudio for the device ingest.  A file whose content is FLAC (it begins with "fLaC", or with an ID3v2 tag
    followed by it): the whole file, format PCM_FLAC, needing no decoder library; ValueError when it is damaged or unsupported.
    RIFF/WAVE (format tag 1, 3, 6, 7, 0x11, or EXTENSIBLE with one of them as its
    sub-format): the data bytes untouched, cut to whole frames.  Other containers: through soundfile when it imports, at the file's
    own rate, as a float32 array [frames][channels] (format PCM_F32); None without soundfile or for a container it does not take
    (decode_audio tries the other decoders)."""
    if not path.lower().endswith((".wav", ".wave")):
        c = _read_flac(path)
        if c is not None:
            return c
        try:
            import soundfile as sf  # type: ignore
            x, sr = sf.read(path, dtype="float32", always_2d=True)
        except Exception:
            return None
        return CodedAudio(np.ascontiguousarray(x), int(sr), int(x.shape[1]), _lib.PCM_F32, 4 * int(x.shape[1]), len(x))
    tag, n_ch, sr, bits, block_align, data, fact = _parse_riff(path)
    if tag in (WAVE_ALAW, WAVE_ULAW, WAVE_IMA_ADPCM):
        if n_ch < 1:
            raise ValueError(f"{path}: {n_ch} channels")
        if tag != WAVE_IMA_ADPCM:
            if bits != 8:
                raise ValueError(f"{path}: G.711 with {bits} bits per sample")
            n = len(data) // n_ch
            return CodedAudio(data[:n * n_ch], sr, n_ch, _lib.PCM_ALAW if tag == WAVE_ALAW else _lib.PCM_ULAW, n_ch, n)
        if bits != 4 or block_align < 8 * n_ch or block_align % (4 * n_ch):
            raise ValueError(f"{path}: IMA ADPCM with {bits} bits per sample in blocks of {block_align} bytes for {n_ch} channels")
        held = len(data) // block_align * (1 + 2 * (block_align // n_ch - 4))
        return CodedAudio(data, sr, n_ch, _lib.PCM_IMA4, block_align, fact if fact is not None and fact <= held else held)
    width = (bits + 7) // 8            # integer samples sit in whole bytes (12 bits in 2); float ones are 32 or 64 bits
    fmt = _PCM_FORMATS.get((tag, width))
    if fmt is None or n_ch < 1 or (tag == WAVE_FLOAT and bits != 8 * width):
        raise ValueError(f"{path}: unsupported WAVE format tag {tag}, {bits} bits")
    n = len(data) // (width * n_ch)
    return CodedAudio(data[:n * width * n_ch], sr, n_ch, fmt, width * n_ch, n)


def read_audio_raw(path: str):
    """read_audio_coded as the (samples, rate, channels, format) tuple of Engine.ingest's plain form, or None when the file has
    to go through decode_audio or is a coded one (G.711, IMA ADPCM)."""
    c = read_audio_coded(path)
    return None if c is None or c.format >= _lib.PCM_ALAW else c[:4]


def decode_coded(c: CodedAudio, channel: Optional[int] = None, verify_md5: bool = True) -> np.ndarray:
    """CodedAudio -> mono float32 at the file's own rate, on the host: the mean of the channels, or one of them.  FLAC is decoded by
    the library (ttasr_flac_decode) to integers v, which become v / 2^(bits - 1) exactly as the left-justified int16 / int32 do;
    verify_md5 checks the stream's MD5 when it carries one (ValueError on a mismatch)."""
    if c.format == _lib.PCM_FLAC:
        v, bits = flac_to_int(c, verify_md5)
        if bits <= 16:
            x = (v << (16 - bits)).astype(np.float32) / 32768.0
        else:
            x = (v << (32 - bits)).astype(np.float32) / 2147483648.0
        x = x.reshape(-1) if c.channels == 1 else x
    elif c.format == _lib.PCM_IMA4:
        x = _ima_decode(c.samples, c.channels, c.block_align, c.n_frames).astype(np.float32) / 32768.0
        x = x.reshape(-1) if c.channels == 1 else x
    else:
        x = samples_to_float(c.samples, c.format, c.channels)
    return downmix(x, channel)


def decode_audio(path: str, sampling_rate: int = SAMPLE_RATE, channel: Optional[int] = None) -> np.ndarray:
    """Path -> mono float32 @16 kHz.  RIFF/WAV (integer and float PCM, G.711 A-law / mu-law, IMA ADPCM) needs nothing beside
    numpy and, for another rate, scipy; a file whose content is FLAC is decoded natively by the library, whatever its name, and
    needs nothing else either (its MD5 is checked when it carries one); other containers go through soundfile / librosa / PyAV when the host has one (the reference
    decodes with librosa / PyAV: asr_core.py:156, faster-whisper decode_audio).  channel=None averages the channels; an index takes
    that channel alone."""
    if not path.lower().endswith((".wav", ".wave")):
        fl = _read_flac(path)
        if fl is not None:
            return resample(decode_coded(fl, _pick_channel(path, channel, fl.channels)), fl.rate, sampling_rate)
        # compressed containers (asr_core.py:118 also globs mp3/flac/m4a/aac): use whichever decoder the host has —
        # none is installed in the build image, so these branches are unexercised here and the error below is what
        # the folder tool records per file
        try:
            import soundfile as sf  # type: ignore
            x, sr = sf.read(path, dtype="float32", always_2d=True)
        except ImportError:
            x = None
        except Exception:
            x = None  # format not handled by libsndfile: try the next decoder
        if x is not None:
            c = _pick_channel(path, channel, x.shape[1])
            return resample(x.mean(axis=1) if c is None else x[:, c], sr, sampling_rate)
        if channel is not None:
            raise RuntimeError(f"{path}: picking a channel of this container needs soundfile; RIFF/WAV needs nothing")
        try:
            import librosa  # type: ignore
            x, _ = librosa.load(path, sr=sampling_rate, mono=True)
            return np.ascontiguousarray(x, dtype=np.float32)
        except ImportError:
            pass
        try:
            import av  # type: ignore
            with av.open(path) as container:
                resampler = av.audio.resampler.AudioResampler(format="s16", layout="mono", rate=sampling_rate)
                chunks = [f.to_ndarray().reshape(-1) for frame in container.decode(audio=0) for f in resampler.resample(frame)]
            return (np.concatenate(chunks).astype(np.float32) / 32768.0) if chunks else np.zeros(0, np.float32)
        except ImportError:
            raise RuntimeError(f"{path}: no decoder for this container (install soundfile, librosa or av); RIFF/WAV needs none")
    c = read_audio_coded(path)
    return resample(decode_coded(c, _pick_channel(path, channel, c.channels)), c.rate, sampling_rate)
