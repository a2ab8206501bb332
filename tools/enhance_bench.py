#!/usr/bin/env python3
"""What the audio enhancement call costs: Engine.enhance with all three stages over one synthetic hour
and over 64 recordings of 30 s, each as ONE call, host memory to host memory (uploads, kernels, downloads), wall clock, the
median of the repeats with the smallest and largest beside it, after one warm-up call that allocates the context's block.
Reported: seconds, audio seconds per second, and the bytes per second the call achieved against the 8 bytes per sample it must
move (4 up, 4 down).  Results must be bit-identical from repeat to repeat (asserted).

    python tools/enhance_bench.py [--repeats 5] [--out profiles/enhance.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def signal(n: int, seed: int):
    """Harmonic bursts in white noise (the test signals' recipe), float32."""
    import numpy as np
    t = np.arange(n, dtype=np.float64) / 16000.0
    tone = sum(np.sin(2 * np.pi * 140.0 * h * t + h) / h for h in range(1, 7))
    return (0.15 * ((t % 0.5) < 0.25) * tone + 0.02 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance.json"))
    args = ap.parse_args()
    import numpy as np
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine

    e = Engine(PRESETS["micro"], COMPUTE_F32, 1)
    loads = {"one_hour": [signal(3600 * 16000, 1)], "64_x_30_s": [signal(30 * 16000, 10 + i) for i in range(64)]}
    out = {"engine": "micro, float32 (the call needs no weights)", "stages": "denoise + highpass + level, default parameters",
           "repeats": args.repeats, "unit": "wall-clock seconds of one Engine.enhance call, host memory to host memory: median [min, max]",
           "bytes_per_sample_the_call_must_move": 8, "results": {}}
    for name, audios in loads.items():
        samples = sum(len(a) for a in audios)
        e.enhance(audios)   # warm-up: the block, the code objects
        secs, crc = [], None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            z = e.enhance(audios)
            secs.append(time.perf_counter() - t0)
            c = zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in z))
            assert crc in (None, c), (name, "results differ between repeats")
            crc = c
        med = statistics.median(secs)
        out["results"][name] = {
            "recordings": len(audios), "samples": samples, "audio_seconds": samples / 16000.0,
            "seconds": {"median": round(med, 5), "min": round(min(secs), 5), "max": round(max(secs), 5)},
            "audio_s_per_s": round(samples / 16000.0 / med, 1),
            "achieved_GB_per_s_of_the_8_B_per_sample": round(8.0 * samples / med / 1e9, 3),
            "result_crc32": crc}
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
