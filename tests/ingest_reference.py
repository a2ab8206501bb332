"""Float64 restatement of the device file ingest (include/ttasr.h, ttasr_ingest_*), numpy only: the filter design, the direct sum
with the quantities its error bound is made of, a plain float32 emulation of that sum, the seeded inputs and the case table.

Bound (derived, not measured): |y_dev - y_64| <= (T + C + 6) 2^-24 S_k with S_k = sum_i |h[t]| mean_c |x_c[i]|, T the taps per
output (ceil(N / up)) and C the channels.  With u = 2^-24 (the unit roundoff of float32) the device's roundings cost, to first order
and relative to S_k: the conversion of a sample u (only s32 and f64 round at all); the C - 1 channel additions and the division
C u; a tap rounded to float32, allowed 1 ulp, 2 u; the products u in all (each is relative to its own term, and the terms sum to at
most S_k); the T - 1 accumulations (T - 1) u (every partial sum is at most S_k); the store nothing (the accumulator is the result).
That is (T + C + 3) u S_k; three more units cover the second-order terms and a fused multiply-add's different split."""
from math import gcd

import numpy as np

TARGET = 16000
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
U8, S16, S24, S32, F32, F64 = range(6)
BYTES = (1, 2, 3, 4, 4, 8)
MAX_R = 1024
# the library's tile rule (csrc/ingest.hpp, engine_ingest.hip ingest_plan): restated so that tests can sit on tile boundaries
THREADS, SPAN, SPAN_MAX, MAX_TILE = 256, 8192, 36864, 4096


def ratio(rate):
    """(up, down, R, half, N) of a rate."""
    g = gcd(rate, TARGET)
    up, down = TARGET // g, rate // g
    R = max(up, down)
    return up, down, R, 10 * R, 20 * R + 1


def accepted(rate):
    return rate >= 1 and ratio(rate)[2] <= MAX_R


def n_out(rate, n):
    up, down = ratio(rate)[:2]
    return -(-n * up // down)


def taps_per_output(rate):
    up, _, _, _, N = ratio(rate)
    return -(-N // up)


def span(rate, tile):
    up, down, _, half, _ = ratio(rate)
    return tile * down // up + 2 * half // up + 2


def tile_for(rate):
    for t in range(MAX_TILE, THREADS - 1, -THREADS):
        if span(rate, t) <= SPAN:
            return t
    t = THREADS
    while t > 1 and span(rate, t) > SPAN_MAX:
        t -= 1
    return t


def design(rate):
    """h[0..N) in float64: firwin(N, 1 / R, window=("kaiser", 5.0)) * up, written out."""
    up, _, R, half, N = ratio(rate)
    m = np.arange(N, dtype=np.float64)
    w = np.sinc((m - half) / R) / R * np.kaiser(N, 5.0)
    return up * w / w.sum()


def channels_f64(raw, fmt, channels):
    """The samples of a raw interleaved buffer as float64 [n_frames][channels], scaled to [-1, 1), exactly."""
    b = np.frombuffer(raw, dtype=np.uint8)
    if fmt == U8:
        x = (b.astype(np.float64) - 128.0) / 128.0
    elif fmt == S16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0
    elif fmt == S24:
        t = b.reshape(-1, 3).astype(np.int32)
        x = ((t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)) << 8 >> 8).astype(np.float64) / 8388608.0
    elif fmt == S32:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    elif fmt == F32:
        x = np.frombuffer(raw, dtype="<f4").astype(np.float64)
    else:
        x = np.frombuffer(raw, dtype="<f8").astype(np.float64)
    return x.reshape(-1, channels)


def host_convert(raw, fmt, channels):
    """decode_audio's conversion and downmix (model.py), float32: what the device gives at rate 16000, bit for bit."""
    if fmt == U8:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif fmt == S16:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif fmt == S24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        x = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8 >> 8).astype(np.float32) / 8388608.0
    elif fmt == S32:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        x = np.frombuffer(raw, dtype="<f4" if fmt == F32 else "<f8").astype(np.float32)
    if channels > 1:
        x = x.reshape(-1, channels).mean(axis=1)
    return np.ascontiguousarray(x, dtype=np.float32)


def _index(rate, n_frames, k_lo, k_hi, tap_shift=0):
    """Per output k in [k_lo, k_hi) and tap slot j: the tap index t, the frame i and whether the pair takes part."""
    up, down, _, half, _ = ratio(rate)
    L = taps_per_output(rate)
    k = np.arange(k_lo, k_hi, dtype=np.int64)[:, None]
    j = np.arange(L - 1, -1, -1, dtype=np.int64)[None, :]      # descending j = ascending i
    a = k * down + half
    ih, p = a // up, a % up
    t, i = p + j * up + tap_shift, ih - j
    ok = (t >= 0) & (t <= 2 * half) & (i >= 0) & (i < n_frames)
    return np.where(ok, t, 0), np.where(ok, i, 0), ok


def direct(rate, x, k_lo=0, k_hi=None, h=None, tap_shift=0):
    """The direct sum in float64 for outputs [k_lo, k_hi): (y, S, T).  x: float64 [n_frames][channels]."""
    n = len(x)
    k_hi = n_out(rate, n) if k_hi is None else k_hi
    h = design(rate) if h is None else h
    t, i, ok = _index(rate, n, k_lo, k_hi, tap_shift)
    mono, mag = x.mean(axis=1), np.abs(x).mean(axis=1)
    hh = np.where(ok, h[t], 0.0)
    return (hh * mono[i]).sum(axis=1), (np.abs(hh) * mag[i]).sum(axis=1), taps_per_output(rate)


def emulate_f32(rate, raw, fmt, channels, k_lo=0, k_hi=None):
    """The same sum in plain float32: converted samples, float32 taps, every product and every accumulation rounded, i ascending."""
    mono = host_convert(raw, fmt, channels)
    n = len(mono)
    k_hi = n_out(rate, n) if k_hi is None else k_hi
    h = design(rate).astype(np.float32)
    t, i, ok = _index(rate, n, k_lo, k_hi)
    acc = np.zeros(k_hi - k_lo, dtype=np.float32)
    for c in range(t.shape[1]):
        acc = np.where(ok[:, c], (acc + (mono[i[:, c]] * h[t[:, c]]).astype(np.float32)).astype(np.float32), acc)
    return acc


def bound(S, T, channels):
    return (T + channels + 6) * 2.0 ** -24 * S


def signal(rate, n_frames, channels, fmt, seed):
    """Raw interleaved bytes of a seeded recording: Gaussian noise at -15 dBFS per channel, a tone at 7.9 kHz and one at 0.45 rate
    where that lies above 8 kHz (the filter must remove it: it may alias nowhere), quantised to the format."""
    rng = np.random.default_rng([0x1A6E57, seed, rate, channels, fmt])
    x = rng.standard_normal((n_frames, channels)) * 10.0 ** (-15 / 20)
    tt = np.arange(n_frames, dtype=np.float64)[:, None] / rate
    if 7900.0 < rate / 2:
        x += 0.1 * np.sin(2 * np.pi * 7900.0 * tt + np.arange(channels)[None, :])
    if 0.45 * rate > 8000.0:
        x += 0.1 * np.sin(2 * np.pi * 0.45 * rate * tt + 0.5)
    x = np.clip(x, -1.0, 1.0 - 2.0 ** -7)
    if fmt == U8:
        return (np.round(x * 128.0) + 128).astype(np.uint8).tobytes()
    if fmt == S16:
        return np.round(x * 32768.0).astype("<i2").tobytes()
    if fmt == S24:
        v = np.round(x * 8388608.0).astype(np.int32).reshape(-1)
        return np.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], axis=1).astype(np.uint8).tobytes()
    if fmt == S32:
        return np.round(x * 2147483648.0).astype("<i4").tobytes()
    return x.astype("<f4" if fmt == F32 else "<f8").tobytes()


def lengths(rate):
    """Input lengths of a case: 1, 7, one frame short of a tile of outputs, the tile, one more, about three tiles."""
    up, down = ratio(rate)[:2]
    nt = max(tile_for(rate) * down // up, 9)
    return (1, 7, nt - 1, nt, nt + 1, 3 * nt + 5)


# (rate, format, channels): every rate twice, every format four times, channels 1, 2 and 6 eight times each
CASES = tuple((r, (i + 3 * v) % 6, (1, 2, 6)[(i + v) % 3]) for i, r in enumerate(RATES) for v in (0, 1))
# ratios that take the large LDS budget with a short tile (16 384 000 Hz: up 1, down 1024, tile 15) and the largest up (15 984 Hz:
# up 1000, down 999)
EXTREME_CASES = ((16000 * 1024, S16, 1), (15984, F32, 2))


_cache = {}


def cached_case(rate, fmt, channels, n_frames, seed=0):
    """(raw, y, S, T) of one seeded recording, computed once per process and shared by the tests that need it."""
    key = (rate, fmt, channels, n_frames, seed)
    if key not in _cache:
        raw = signal(rate, n_frames, channels, fmt, seed)
        _cache[key] = (raw,) + direct(rate, channels_f64(raw, fmt, channels))
    return _cache[key]


def write_wav(path, raw, rate, channels, fmt, extensible=False):
    """A RIFF/WAVE file around raw interleaved samples: format tag 1 (integer PCM), 3 (IEEE float) or, extensible=True, 0xFFFE
    with that tag as its sub-format."""
    import struct
    bits, tag = 8 * BYTES[fmt], 3 if fmt in (F32, F64) else 1
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    if extensible:
        body += struct.pack("<HHIH", 22, bits, 0, tag) + bytes.fromhex("000000001000800000AA00389B71")
    data = bytes(raw)
    chunks = b"WAVE" + b"fmt " + struct.pack("<I", len(body)) + body + b"data" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks)
