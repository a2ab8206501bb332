"""Word alignment: the one-clip path against the batched device path, in one process on the same sequences.

Workload: large-v3 geometry (synthetic weights), bf16, 24 resident clips, 10 alignment heads, one teacher-forced sequence per
clip with a seeded 40 ... 120 text tokens.
  (A) the one-clip path: per clip Engine.align (maps to the host) + alignment.token_start_times (numpy + host DTW);
  (B) one Engine.align_batch call (pass, post-processing and DTW on the device; start frames and log-probs to the host).
Both are timed as wall time per clip over --repeats runs after a warm-up; median and range are reported.
  session: a refill_bench-shaped greedy session (4-token prompt, seeded budgets), wall time and decode steps with hold mode +
  Session.align after every poll against the same session with hold off.
One JSON line per measurement on stdout and, with --out, appended to that file.

    python tools/align_bench.py [--model large-v3] [--clips 24] [--repeats 7] [--session-clips 96] [--out profiles/align_batch.jsonl]
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

from taiwan_tongues_asr_ce_amd import alignment, synth  # noqa: E402
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, PRESETS  # noqa: E402
from taiwan_tongues_asr_ce_amd.engine import Engine  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--clips", type=int, default=24)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--session-clips", type=int, default=96)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dims = PRESETS[args.model]
    eng = Engine(dims, COMPUTE_BF16, args.batch)
    eng.load_weights(synth.iter_weights(dims))
    st = eng.special
    n = args.clips
    heads = alignment.default_alignment_heads(dims.dec_layers, dims.n_heads, limit=10)
    rng = np.random.Generator(np.random.Philox(key=args.seed))
    lens = rng.integers(40, 121, size=n)
    seqs = [[st.sot, st.lang_zh, st.transcribe, st.no_timestamps] + rng.integers(300, 20000, size=int(k)).tolist() + [st.eot] for k in lens]
    clips = [synth.noise_clip(i) for i in range(n)]
    eng.log_mel(clips, want_output=False)
    eng.encode(n)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def path_a():
        out = []
        for c in range(n):
            w, _ = eng.align(c, seqs[c], heads)
            out.append(alignment.token_start_times(w, 3, len(seqs[c]) - 1, 3000))
        return out

    def path_b():
        return eng.align_batch(list(range(n)), seqs, [3] * n, [3000] * n, heads).start_frames

    a0, b0 = path_a(), path_b()      # warm-up (first-touch allocations, the scratch of the batched pass)
    agree = float(np.mean([np.mean(np.round(x * 50).astype(int) == y) for x, y in zip(a0, b0)]))
    ta, tb = [], []
    for _ in range(args.repeats):    # interleaved, so that drift hits both alike
        t0 = time.perf_counter(); path_a(); ta.append((time.perf_counter() - t0) * 1e3 / n)
        t0 = time.perf_counter(); path_b(); tb.append((time.perf_counter() - t0) * 1e3 / n)
    emit({"bench": "align", "model": args.model, "clips": n, "heads": len(heads), "text_tokens": [int(lens.min()), int(lens.max())],
          "one_clip_ms_per_clip": spread(ta), "batch_ms_per_clip": spread(tb),
          "speedup_median": round(statistics.median(ta) / statistics.median(tb), 2), "equal_start_frames": round(agree, 4)})

    # the session: hold + align after every poll against hold off
    N = args.session_clips
    sclips = [synth.noise_clip(100 + i) for i in range(N)]
    caps = rng.integers(32, 129, size=N).astype(np.int32)
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = eng.gen_opts(128, timestamps=False, suppress_eot=True)

    def session(hold):
        t0 = time.perf_counter()
        with eng.session(opts, len(prompt)) as s:
            if hold:
                s.hold()
            ids = s.submit(sclips, [prompt] * N, caps)
            where = {cid: i for i, cid in enumerate(ids)}
            while s.pending > 0:
                got = s.poll()
                if hold and got:
                    s.align([r.id for r in got], [prompt + [t for t in r.tokens if t < st.eot] + [st.eot] for r in got],
                            [3] * len(got), [3000] * len(got), heads)
            steps = int(s.stats()["steps"])
        return time.perf_counter() - t0, steps

    session(False); session(True)    # warm-up
    for hold in (False, True, False, True):
        wall, steps = session(hold)
        emit({"bench": "session", "model": args.model, "clips": N, "hold_and_align": hold, "wall_s": round(wall, 3), "decode_steps": steps})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
