"""File ingest: the host path of audio_io.decode_audio against one Engine.ingest call (kernels_ingest.hip), on 32 in-memory
recordings of 60 s at 44.1 and 48 kHz, 2-channel int16 and mono int16.

  host     decode_audio's conversion path on the sample bytes, one thread, file by file: int16 -> float32 / 32768, the channel
           mean, scipy.signal.resample_poly, float32.  One pass over the 32 recordings after a warm-up on the first; the time is
           the sum.
  device   ONE Engine.ingest call over the 32 recordings, host bytes in to host float32 out (the call ends in a stream
           synchronise): 2 warm-up calls, median / min / max of --repeats calls.
  phases   one more call under option ingest_timing = 1, which waits after every copy and kernel and reports the host-clock sums:
           staging copies on the host (into the pinned slots and out of them), uploads, kernels, downloads.  The waits cost the
           overlap the timed calls have, so the four do not add up to the device figure.
Nothing is asserted.  One JSON object on stdout and in --out.

    python tools/ingest_bench.py [--files 32] [--seconds 60] [--repeats 5] [--out profiles/ingest_bench.json]

--codec ulaw | alaw | ima4 (may be given several times) measures telephony files instead: 8 kHz, mono and 2-channel, G.711 bytes or
IMA ADPCM blocks of 256 bytes per channel (505 samples), random bytes.  The host path is then audio_io.decode_audio's from the data
bytes on - the G.711 table or the numpy IMA decoder, / 32768, the channel mean, resample_poly - and the device path the same one
Engine.ingest call (ttasr_ingest_wave).  The result goes to profiles/ingest_bench_codecs.json.

    python tools/ingest_bench.py --codec ulaw --codec alaw --codec ima4

--codec flac measures FLAC files: ONE recording of --seconds (default 600) at 44.1 kHz, 16 bits, in frames of 4096 samples with
order-2 fixed predictors and one Rice parameter per subframe - written here by a numpy encoder and checked against
ttasr_flac_decode before anything is timed - fed --files (default 8) times in one call, as 2 channels and as 1.  Beside the usual
figures the workload reports the same audio as S16 through the unchanged device path, the host path (ttasr_flac_decode, the MD5
check, / 32768, the channel mean, resample_poly) with its decode and scan (ttasr_flac_probe: the CRC pass) shares, and the
compression ratio.  The result goes to profiles/ingest_bench_flac.json.

    python tools/ingest_bench.py --codec flac
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = 2150.0   # audio-s/s of the engine's greedy headline workload (README.md)


def host_ingest(raw: np.ndarray, rate: int, channels: int) -> np.ndarray:
    """audio_io.decode_audio from the sample bytes on, for 16-bit PCM."""
    from taiwan_tongues_asr_ce_amd import _lib, audio_io
    return audio_io.resample(audio_io.downmix(audio_io.samples_to_float(raw, _lib.PCM_S16, channels), None), rate)


def host_ingest_coded(raw: bytes, rate: int, channels: int, codec: str, block_align: int) -> np.ndarray:
    """audio_io.decode_audio from the data bytes on, for a coded file."""
    from taiwan_tongues_asr_ce_amd import _lib, audio_io
    code = {"ulaw": _lib.PCM_ULAW, "alaw": _lib.PCM_ALAW, "ima4": _lib.PCM_IMA4}[codec]
    held = len(raw) // block_align * (1 + 2 * (block_align // channels - 4)) if codec == "ima4" else len(raw) // channels
    return audio_io.resample(audio_io.decode_coded(audio_io.CodedAudio(raw, rate, channels, code, block_align, held)), rate)


def _bits(v: int, n: int) -> np.ndarray:
    return np.array([(v >> (n - 1 - j)) & 1 for j in range(n)], dtype=np.uint8)


def _coded_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for n in range(2, 8):
        if v < 1 << (7 - n + 6 * (n - 1)):
            return bytes([((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(n - 2, -1, -1)])
    raise ValueError(v)


def flac_encode(x: np.ndarray, rate: int, blocksize: int = 4096) -> bytes:
    """int16 [frames][channels] -> a FLAC file (fixed blocking, independent channels, order-2 fixed predictors, one 5-bit Rice
    parameter per subframe, MD5 in STREAMINFO), fast enough for ten minutes of audio: numpy per subframe, and the CRC-16 of all
    frames at once, column by column (frames padded with zero bytes in FRONT, which a CRC with init 0 does not see)."""
    import hashlib
    n, ch = x.shape
    rate_code = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}[rate]
    bodies = []
    for k, a in enumerate(range(0, n, blocksize)):
        bs = min(blocksize, n - a)
        code = {256 << j: 8 + j for j in range(8)}.get(bs, 7)
        head = bytearray([0xFF, 0xF8, (code << 4) | rate_code, ((ch - 1) << 4) | (4 << 1)]) + _coded_number(k)
        if code == 7:
            head += (bs - 1).to_bytes(2, "big")
        c8 = 0
        for b in head:
            c8 ^= b
            for _ in range(8):
                c8 = ((c8 << 1) ^ 0x07) & 0xFF if c8 & 0x80 else (c8 << 1) & 0xFF
        parts = []
        for c in range(ch):
            s = x[a:a + bs, c].astype(np.int64)
            if bs < 3:                                    # verbatim
                parts += [_bits(0x02, 8)] + [_bits(int(v) & 0xFFFF, 16) for v in s]
                continue
            res = s[2:] - 2 * s[1:-1] + s[:-2]
            u = np.where(res >= 0, res << 1, ((-res) << 1) - 1)
            kk = min(max(int(np.log2(u.mean() + 1.0)), 0), 30)
            q = u >> kk
            length = q + 1 + kk
            off = np.cumsum(length) - length
            bits = np.zeros(int(length.sum()), dtype=np.uint8)
            bits[off + q] = 1
            for j in range(kk):
                bits[off + q + 1 + j] = (u >> (kk - 1 - j)) & 1
            parts += [_bits(0x14, 8), _bits(int(s[0]) & 0xFFFF, 16), _bits(int(s[1]) & 0xFFFF, 16), _bits(1, 2), _bits(0, 4), _bits(kk, 5), bits]
        bodies.append(bytes(head) + bytes([c8]) + np.packbits(np.concatenate(parts)).tobytes())
    table = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        table[i] = c
    width = max(len(b) for b in bodies)
    rows = np.zeros((len(bodies), width), dtype=np.uint8)
    for r, b in zip(rows, bodies):
        r[width - len(b):] = np.frombuffer(b, dtype=np.uint8)
    crc = np.zeros(len(bodies), dtype=np.uint32)
    for j in range(width):
        crc = ((crc << 8) & 0xFFFF) ^ table[(crc >> 8) ^ rows[:, j]]
    info = blocksize.to_bytes(2, "big") * 2 + bytes(6) + ((rate << 44) | ((ch - 1) << 41) | (15 << 36) | n).to_bytes(8, "big")
    info += hashlib.md5(np.ascontiguousarray(x).astype("<i2").tobytes()).digest()
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info + b"".join(b + int(c).to_bytes(2, "big") for b, c in zip(bodies, crc))


def flac_signal(n: int, channels: int, rate: int) -> np.ndarray:
    """Something a predictor can work on: a few drifting tones and a little noise, int16 [n][channels]."""
    rng = np.random.default_rng([0xF1AC, n, channels])
    t = np.arange(n, dtype=np.float64) / rate
    x = np.zeros((n, channels))
    for c in range(channels):
        for f, a in ((220.0 + 13 * c, 3000.0), (1370.0 + 7 * c, 1200.0), (4100.0, 400.0)):
            x[:, c] += a * np.sin(2 * np.pi * f * t * (1.0 + 0.02 * np.sin(0.3 * t)) + c)
        x[:, c] += rng.normal(0.0, 60.0, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def bench_flac(eng, args, res):
    from taiwan_tongues_asr_ce_amd import _lib, audio_io
    rate = 44100
    res["format"] = "FLAC, 16 bits, frames of 4096 samples, order-2 fixed predictors"
    for channels in (2, 1):
        n = int(args.seconds * rate)
        x = flac_signal(n, channels, rate)
        t = time.perf_counter()
        blob = flac_encode(x, rate)
        encode_s = time.perf_counter() - t
        got, info = _lib.flac_decode(blob)
        assert np.array_equal(got, x) and info.has_md5, "the benchmark's encoder and the library disagree"
        raws, pcm = [blob] * args.files, [x] * args.files
        # (n_frames as audio_io.read_audio_coded reports it: the call scans each file once, inside the library)
        call = lambda: eng.ingest(raws, [rate] * args.files, [channels] * args.files, [_lib.PCM_FLAC] * args.files,  # noqa: E731
                                  n_frames=[n] * args.files)
        call_s16 = lambda: eng.ingest(pcm, [rate] * args.files, [channels] * args.files, [_lib.PCM_S16] * args.files)  # noqa: E731
        audio_s = args.files * n / rate
        coded = audio_io.CodedAudio(blob, rate, channels, _lib.PCM_FLAC, 0, n)
        t = time.perf_counter()
        _lib.flac_probe(blob)
        scan_s = time.perf_counter() - t
        t = time.perf_counter()
        _lib.flac_decode(blob)
        decode_s = time.perf_counter() - t
        t = time.perf_counter()
        host = audio_io.resample(audio_io.decode_coded(coded), rate)
        host_s = time.perf_counter() - t
        times = {}
        for name, fn in (("flac", call), ("s16", call_s16)):
            for _ in range(2):
                dev = fn()
            xs = []
            for _ in range(args.repeats):
                t = time.perf_counter()
                fn()
                xs.append(time.perf_counter() - t)
            times[name] = xs
            if name == "flac":
                flac_out = dev
            else:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(flac_out, dev)), "FLAC and S16 outputs differ"
        eng.set_option("ingest_timing", 1)
        call()
        ph = eng.phase_ms()
        eng.set_option("ingest_timing", 0)
        dev_s, s16_s = statistics.median(times["flac"]), statistics.median(times["s16"])
        diff = float(np.abs(flac_out[0].astype(np.float64) - host).max())
        res["workloads"][f"{rate} Hz x {channels} ch flac"] = {
            "audio_s": round(audio_s, 1), "files": args.files, "flac_mb_per_file": round(len(blob) / 1e6, 2),
            "compression": round(len(blob) / x.nbytes, 3), "flac_frames_per_file": info.frames, "encode_s_numpy": round(encode_s, 2),
            "host_s_per_file": round(host_s, 4), "host_audio_s_per_s": round(n / rate / host_s, 1),
            "host_flac_decode_s_per_file": round(decode_s, 4), "host_scan_s_per_file": round(scan_s, 5),
            "host_scan_mb_per_s": round(len(blob) / 1e6 / scan_s, 1),
            "device_median_s": round(dev_s, 5), "device_min_s": round(min(times["flac"]), 5), "device_max_s": round(max(times["flac"]), 5),
            "device_audio_s_per_s": round(audio_s / dev_s, 1),
            "device_s16_median_s": round(s16_s, 5), "device_s16_audio_s_per_s": round(audio_s / s16_s, 1),
            "flac_over_s16_time": round(dev_s / s16_s, 3), "device_over_host": round(host_s * args.files / dev_s, 2),
            "device_exceeds_headline": bool(audio_s / dev_s > HEADLINE), "outputs_bit_equal_to_s16_path": True,
            "phases_serialised_ms": {"staging_copies_host": round(ph["mel"], 2), "h2d": round(ph["encoder"], 2),
                                     "kernel": round(ph["cross_kv"], 2), "d2h": round(ph["decode"], 2)},
            "max_abs_diff_device_vs_host": float(f"{diff:.3e}")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codec", action="append", choices=("ulaw", "alaw", "ima4", "flac"), default=None)
    ap.add_argument("--files", type=int, default=None)
    ap.add_argument("--seconds", type=float, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only_flac = args.codec == ["flac"]
    if args.files is None:
        args.files = 8 if only_flac else 32
    if args.seconds is None:
        args.seconds = 600.0 if only_flac else 60.0
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ingest_bench_flac.json" if only_flac else
                                "ingest_bench_codecs.json" if args.codec else "ingest_bench.json")
    from taiwan_tongues_asr_ce_amd import _lib
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    eng = Engine(PRESETS["micro"], COMPUTE_F32, 4)       # ingest needs no weights
    res = {"tool": "tools/ingest_bench.py", "files": args.files, "seconds_per_file": args.seconds, "format": "int16",
           "headline_greedy_audio_s_per_s": HEADLINE, "workloads": {}}
    if args.codec:
        res["format"] = "G.711 / IMA ADPCM, random bytes"
    if args.codec and "flac" in args.codec:
        bench_flac(eng, args, res)
    for codec, rate in [(c, 8000) for c in args.codec if c != "flac"] if args.codec else [(None, 44100), (None, 48000)]:
        for channels in (2, 1):
            n = int(args.seconds * rate)
            rng = np.random.default_rng([0x16E57, rate, channels])
            if codec is None:
                raws = [rng.integers(-6000, 6000, size=n * channels, dtype=np.int16) for _ in range(args.files)]
                host_fn = lambda r: host_ingest(r, rate, channels)  # noqa: E731
                call = lambda: eng.ingest(raws, [rate] * len(raws), [channels] * len(raws), [_lib.PCM_S16] * len(raws))  # noqa: E731
            else:
                ba = 256 * channels
                if codec == "ima4":
                    n = n // 505 * 505                      # whole blocks
                    size = n // 505 * ba
                else:
                    size = n * channels
                raws = [rng.integers(0, 256, size=size, dtype=np.uint8) for _ in range(args.files)]
                code = {"ulaw": _lib.PCM_ULAW, "alaw": _lib.PCM_ALAW, "ima4": _lib.PCM_IMA4}[codec]
                host_fn = lambda r: host_ingest_coded(r.tobytes(), rate, channels, codec, ba)  # noqa: E731
                call = lambda: eng.ingest(raws, [rate] * len(raws), [channels] * len(raws), [code] * len(raws),  # noqa: E731
                                          block_aligns=[ba] * len(raws))
            audio_s = args.files * n / rate
            host_fn(raws[0])
            t = time.perf_counter()
            host = [host_fn(r) for r in raws]
            host_s = time.perf_counter() - t
            for _ in range(2):
                dev = call()
            xs = []
            for _ in range(args.repeats):
                t = time.perf_counter()
                call()
                xs.append(time.perf_counter() - t)
            dev_s = statistics.median(xs)
            eng.set_option("ingest_timing", 1)
            call()
            ph = eng.phase_ms()
            eng.set_option("ingest_timing", 0)
            diff = max(float(np.abs(d.astype(np.float64) - h).max()) for d, h in zip(dev, host))
            res["workloads"][f"{rate} Hz x {channels} ch" + (f" {codec}" if codec else "")] = {
                "audio_s": round(audio_s, 1), "raw_mb": round(sum(r.nbytes for r in raws) / 1e6, 1),
                "host_s": round(host_s, 4), "host_audio_s_per_s": round(audio_s / host_s, 1),
                "device_median_s": round(dev_s, 5), "device_min_s": round(min(xs), 5), "device_max_s": round(max(xs), 5),
                "device_audio_s_per_s": round(audio_s / dev_s, 1), "device_over_host": round(host_s / dev_s, 2),
                "device_exceeds_headline": bool(audio_s / dev_s > HEADLINE),
                "phases_serialised_ms": {"staging_copies_host": round(ph["mel"], 2), "h2d": round(ph["encoder"], 2),
                                         "kernel": round(ph["cross_kv"], 2), "d2h": round(ph["decode"], 2)},
                "max_abs_diff_device_vs_host": float(f"{diff:.3e}")}
            del raws, host, dev
    eng.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
