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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codec", action="append", choices=("ulaw", "alaw", "ima4"), default=None)
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ingest_bench_codecs.json" if args.codec else "ingest_bench.json")
    from taiwan_tongues_asr_ce_amd import _lib
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    eng = Engine(PRESETS["micro"], COMPUTE_F32, 4)       # ingest needs no weights
    res = {"tool": "tools/ingest_bench.py", "files": args.files, "seconds_per_file": args.seconds, "format": "int16",
           "headline_greedy_audio_s_per_s": HEADLINE, "workloads": {}}
    if args.codec:
        res["format"] = "G.711 / IMA ADPCM, random bytes"
    for codec, rate in [(c, 8000) for c in args.codec] if args.codec else [(None, 44100), (None, 48000)]:
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
