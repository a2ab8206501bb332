#!/usr/bin/env python3
"""What the sequence-bias launch costs: the greedy 32-row decode step and the 5 x 8-row beam position
of one engine context in three states - no table, a table of 64 entries, a table with every cap full (4096 groups, 8192 entries) -
alternated round by round in ONE process, after a warm-up round that captures every step graph.  Every bias is 0.0, so all three
states must produce the same tokens (asserted): only the launch differs.  Times are the decode phase between device events
(Engine.phase_ms) over the steps of the call, the median over the rounds, with the smallest and largest round beside it.

    python tools/seq_bias_bench.py [--model large-v3] [--rounds 5] [--out profiles/seq_bias.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables(vocab: int):
    import numpy as np
    rng = np.random.default_rng(5)
    ids = rng.permutation(np.arange(1000, 40000))[:4096 + 64].tolist()
    small = {(ids[4096 + i], ids[i]): 0.0 for i in range(64)}
    full = {}
    for g in range(4096):
        full[(ids[g],)] = 0.0
        full[(ids[(g + 1) % 4096], ids[g])] = 0.0
        full[(ids[(g + 7) % 4096], ids[(g + 3) % 4096], ids[g])] = 0.0
    return {"none": None, "entries_64": small, "full": full}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_bias.json"))
    args = ap.parse_args()
    import numpy as np
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine

    dims = PRESETS[args.model]
    e = Engine(dims, COMPUTE_BF16, 40)
    e.load_weights(synth.iter_weights(dims))
    st = e.special
    e.log_mel([synth.noise_clip(b) for b in range(32)], want_output=False)
    e.encode(32)
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(args.new_tokens, False, suppress_eot=True)
    steps = len(prompt) - 1 + args.new_tokens
    states = tables(dims.vocab)
    runs = {"greedy_32_rows": lambda: e.generate([prompt] * 32, opts), "beam_5x8_rows": lambda: e.generate_beam([prompt] * 8, 5, opts)}
    ms = {r: {s: [] for s in states} for r in runs}
    tokens = {}
    for rnd in range(args.rounds + 1):               # round 0 warms up: graph capture, code objects
        for s, table in states.items():
            e.set_sequence_bias(table)
            for r, run in runs.items():
                res = run()
                crc = zlib.crc32(np.asarray(res.tokens, dtype=np.int32).tobytes())
                assert tokens.setdefault(r, crc) == crc, (r, s, "tokens differ between the states")
                if rnd:
                    ms[r][s].append(e.phase_ms()["decode"] / steps)
    e.set_sequence_bias(None)
    out = {"model": args.model, "compute": "bf16", "rounds": args.rounds, "new_tokens": args.new_tokens, "steps_per_call": steps,
           "unit": "ms of the decode phase per step (device events), median [min, max] over the rounds",
           "tokens_identical_in_all_states": True, "token_crc32": tokens, "results": {}}
    for r in runs:
        out["results"][r] = {s: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for s, v in ms[r].items()}
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
