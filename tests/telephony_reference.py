"""The telephony codecs of include/ttasr.h ("coded WAVE files and the channel pick") written out in plain Python / numpy, a
RIFF writer for their files, and the case table of the tests.  Everything here is integer arithmetic: the checks that use it are
bit-for-bit equalities.

Inputs are seeded random bytes: every byte string is a legal G.711 stream, and every block of random bytes is a legal IMA ADPCM
block (a header step index above 88 is read as 88), so no encoder is needed."""
import struct

import numpy as np

ALAW, ULAW, IMA4 = 16, 17, 18          # TTASR_PCM_ALAW / _ULAW / _IMA4
S16 = 1                                # TTASR_PCM_S16
TAGS = {ALAW: 6, ULAW: 7, IMA4: 0x11}  # WAVE format tags

IMA_INDEX = (-1, -1, -1, -1, 2, 4, 6, 8)
IMA_STEP = (
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
    11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767)
assert len(IMA_STEP) == 89


# ---- G.711 ----

def ulaw_sample(b):
    u = ~b & 0xFF
    e, m = (u >> 4) & 7, u & 15
    v = (((m << 3) + 0x84) << e) - 0x84
    return -v if u & 0x80 else v


def alaw_sample(b):
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    v = (m << 4) + 8
    if e >= 1:
        v = (v + 0x100) << (e - 1)
    return v if a & 0x80 else -v


ULAW_TABLE = np.array([ulaw_sample(b) for b in range(256)], dtype=np.int16)
ALAW_TABLE = np.array([alaw_sample(b) for b in range(256)], dtype=np.int16)


def g711_decode(raw, fmt, channels):
    """bytes -> int16 [frames][channels]"""
    table = ULAW_TABLE if fmt == ULAW else ALAW_TABLE
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    return table[b[:len(b) - len(b) % channels]].reshape(-1, channels)


# ---- IMA ADPCM ----

def ima_nibble(n, pred, index, low_first=True, clamp_index=True, keep_eighth=True):
    """One nibble: (predictor, index) -> (predictor, index).  The keyword switches exist for the tests that show the reference
    catches what it is there for; the defaults are the definition."""
    step = IMA_STEP[index]
    d = step >> 3 if keep_eighth else 0
    if n & 4:
        d += step
    if n & 2:
        d += step >> 1
    if n & 1:
        d += step >> 2
    pred = pred - d if n & 8 else pred + d
    pred = max(-32768, min(32767, pred))
    index += IMA_INDEX[n & 7]
    if clamp_index:
        index = max(0, min(88, index))
    else:
        index = index % 89          # "a missing clamp" that still cannot index outside the table
    return pred, index


def ima_spb(block_align, channels):
    return 1 + 2 * (block_align // channels - 4)


def ima_decode(raw, channels, block_align, n_frames=None, low_first=True, clamp_index=True, keep_eighth=True, group=4):
    """bytes -> int16 [frames][channels]: whole blocks only, cut to n_frames when given.  One Python loop over everything: slow and
    plain on purpose."""
    raw = bytes(raw)
    spb = ima_spb(block_align, channels)
    blocks = len(raw) // block_align
    out = np.zeros((blocks * spb, channels), dtype=np.int16)
    for b in range(blocks):
        blk = raw[b * block_align:(b + 1) * block_align]
        for c in range(channels):
            pred, index = struct.unpack("<hB", blk[4 * c:4 * c + 3])
            index = min(index, 88)
            f = b * spb
            out[f, c] = pred
            f += 1
            per_channel = block_align // channels - 4           # data bytes of this channel
            for k in range(per_channel):
                g, r = divmod(k, group)
                byte = blk[4 * channels + g * group * channels + group * c + r]
                nibbles = (byte & 15, byte >> 4) if low_first else (byte >> 4, byte & 15)
                for n in nibbles:
                    pred, index = ima_nibble(n, pred, index, clamp_index=clamp_index, keep_eighth=keep_eighth)
                    out[f, c] = pred
                    f += 1
    return out if n_frames is None else out[:n_frames]


def ima_frames(n_bytes, channels, block_align, fact=None):
    held = n_bytes // block_align * ima_spb(block_align, channels)
    return fact if fact is not None and fact <= held else held


# ---- files ----

def decode(raw, fmt, channels, block_align=0, n_frames=None):
    """int16 [frames][channels] of a stream in any of the three codes"""
    if fmt == IMA4:
        return ima_decode(raw, channels, block_align, n_frames)
    x = g711_decode(raw, fmt, channels)
    return x if n_frames is None else x[:n_frames]


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def ima_stream(blocks, channels, block_align, seed, tail=0):
    """`blocks` random blocks and `tail` bytes that fill no block.  Random header bytes put a step index above 88 into about two
    blocks of three; the first block's first channel gets index 200 whatever the seed."""
    raw = bytearray(random_bytes(blocks * block_align + tail, seed))
    if blocks:
        raw[2] = 200
    return bytes(raw)


def write_wav(path, raw, rate, channels, fmt, block_align=0, fact=None, extensible=False):
    """A RIFF/WAVE file around a coded stream: tag 6 / 7 / 0x11, or extensible=True 0xFFFE with that tag as its sub-format; fact =
    the sample count of a `fact` chunk (None: no such chunk)."""
    tag = TAGS[fmt]
    if fmt == IMA4:
        spb = ima_spb(block_align, channels)
        body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block_align // spb, block_align, 4)
        extra = struct.pack("<H", spb)
    else:
        body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels, channels, 8)
        extra = b""
    if extensible:
        body += struct.pack("<HHIH", 22, 4 if fmt == IMA4 else 8, 0, tag) + bytes.fromhex("000000001000800000AA00389B71")
    else:
        body += struct.pack("<H", len(extra)) + extra
    data = bytes(raw)
    chunks = b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body + b"\0" * (len(body) & 1)
    if fact is not None:
        chunks += b"fact" + struct.pack("<II", 4, fact)
    chunks += b"data" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks)


# ---- the case table ----

G711_CHANNELS = (1, 2, 6)
G711_RATES = (8000, 11025, 16000, 44100)
G711_FRAMES = 1531                      # odd, and several tiles of the slow rates' outputs

# (block_align, channels): 36 mono = 65 samples a block, 256 mono = 505
IMA_BLOCKS = ((36, 1), (72, 2), (256, 1), (512, 2), (2048, 1))


def ima_frame_counts(spb):
    """(frames, blocks in the file, fact): the last entry has more blocks than its fact chunk says"""
    return ((1, 1, 1), (spb - 1, 1, spb - 1), (spb, 1, None), (spb + 1, 2, spb + 1), (3 * spb + 7, 4, 3 * spb + 7),
            (2 * spb + 5, 5, 2 * spb + 5))
