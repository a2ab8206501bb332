"""Language detection: the device call against the step-level path it replaces, in one process on the same resident clips.

Workload: large-v3 geometry (synthetic weights), bf16, 32 resident clips (log-mel and encoder run once, outside the timed part).
  (A) the step-level path: Engine.decode_reset + Engine.decode_step([sot] * B) with the [B][51 866] logits copied to the host +
      the numpy softmax over the language span (what WhisperModel.detect_language did, for all B rows at once);
  (B) one Engine.detect_language(B) call (ttasr_detect_language: the same decoder pass ending in the language head; indices and
      probabilities to the host).
Both are wall times around calls that end in a stream synchronise, taken alternately (A, B, A, B, ...) over --repeats rounds
after a warm-up of both; median, minimum and maximum are reported, together with the largest difference of the span logits of
the two paths and whether the winners agree.  No threshold is asserted.  One JSON object on stdout and, with --out, in that file.

    python tools/lang_bench.py [--model large-v3] [--clips 32] [--repeats 50] [--out profiles/lang_detect.json]

--session: language=None through a continuous-batching session.  64 clips (--session-clips) through 32 rows (--clips), seeded
token budgets 32 ... 128, check_interval 8:
  (before)  detection before the session - static passes of 32 clips (log-mel, encoder, Engine.detect_language), then an unarmed
            session whose prompts carry the languages found (what transcribe_stream(language=None) does by default);
  (inside)  an armed session (Engine.session(detect_language=True)) whose prompts carry the placeholder: one more decode step
            per clip, no encoder pass beforehand;
  (given)   the unarmed session alone with the languages given: what a session cost before detection existed, to be set beside
            tools/refill_bench.py of the previous revision.
The three are wall times around whole runs, taken alternately over --repeats rounds after a warm-up of each; median, minimum and
maximum are reported, with whether (inside) returns (before)'s languages and tokens.  Nothing is asserted.

    python tools/lang_bench.py --session [--repeats 5] [--out profiles/lang_detect_session.json]
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

from taiwan_tongues_asr_ce_amd import synth  # noqa: E402
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS  # noqa: E402
from taiwan_tongues_asr_ce_amd.engine import Engine  # noqa: E402

KINDS = (synth.noise_clip, synth.tonal_clip, synth.burst_clip, synth.noise_clip)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--compute", default="bf16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--session", action="store_true", help="detection before a session against detection inside it")
    ap.add_argument("--session-clips", type=int, default=64)
    args = ap.parse_args()
    if args.session:
        return main_session(args)
    dims = PRESETS[args.model]
    B = args.clips
    eng = Engine(dims, {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}[args.compute], B)
    eng.load_weights(synth.iter_weights(dims))
    sot = eng.special.sot
    begin, n_lang = eng.language_span()
    eng.log_mel([KINDS[i % 4](i) for i in range(B)], want_output=False)
    eng.encode(B)

    def path_a():
        eng.decode_reset(B)
        ll = eng.decode_step([sot] * B)[:, begin:begin + n_lang].astype(np.float64)
        p = np.exp(ll - ll.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        return p.argmax(axis=1), p, ll

    def path_b(want_logits=False):
        return eng.detect_language(B, want_logits=want_logits)

    for _ in range(3):               # warm-up: the step graph of (A), first launches of both
        ia, pa, la = path_a()
        ib, pb, lb = path_b(True)
    ta, tb = [], []
    for _ in range(args.repeats):    # alternating, so that drift and neighbours hit both alike
        t0 = time.perf_counter(); path_a(); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); path_b(); tb.append((time.perf_counter() - t0) * 1e3)
    out = {"bench": "lang_detect", "model": args.model, "compute": args.compute, "clips": B, "n_lang": n_lang,
           "step_path_ms": spread(ta), "detect_call_ms": spread(tb),
           "ratio_of_medians": round(statistics.median(ta) / statistics.median(tb), 3),
           "span_logits_max_abs_diff": float(np.abs(lb - la).max()), "prob_max_abs_diff": float(np.abs(pb - pa).max()),
           "winners_equal": bool(np.array_equal(ia, ib)),
           "method": "host wall time around calls that end in a stream synchronise; both paths warmed, then alternated; the "
                     "encoder state is resident and outside the timed part"}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main_session(args):
    from taiwan_tongues_asr_ce_amd.engine import Session
    dims = PRESETS[args.model]
    B, N = args.clips, args.session_clips
    eng = Engine(dims, {"f32": COMPUTE_F32, "bf16": COMPUTE_BF16, "f16": COMPUTE_F16}[args.compute], B)
    eng.load_weights(synth.iter_weights(dims))
    st = eng.special
    begin, n_lang = eng.language_span()
    tail = [st.transcribe, st.no_timestamps]
    opts = eng.gen_opts(128, timestamps=False, suppress_eot=True, check_interval=8)
    clips = [KINDS[i % 4](i) for i in range(N)]
    caps = np.random.Generator(np.random.Philox(key=6)).integers(32, 129, size=N).astype(np.int32)

    def run_session(prompts, armed):
        langs, toks = [None] * N, [None] * N
        with eng.session(opts, 4, detect_language=armed) as s:
            ids = s.submit(clips, prompts, caps)
            where = {cid: i for i, cid in enumerate(ids)}
            for r in s.drain():
                langs[where[r.id]], toks[where[r.id]] = r.language, r.tokens
            stats = s.stats()
        return langs, toks, stats

    def before():
        langs = []
        for i in range(0, N, B):
            chunk = clips[i:i + B]
            eng.log_mel(chunk, want_output=False)
            eng.encode(len(chunk))
            langs += eng.detect_language(len(chunk))[0].tolist()
        _, toks, stats = run_session([[st.sot, begin + l] + tail for l in langs], False)
        return langs, toks, stats

    def inside():
        return run_session([[st.sot, Session.DETECT] + tail] * N, True)

    found = before()[0]                      # warm-up of every path: graph captures, first-touch allocations
    inside()

    def given():
        return run_session([[st.sot, begin + l] + tail for l in found], False)
    given()
    t = {"before": [], "inside": [], "given": []}
    last = {}
    for _ in range(args.repeats):            # alternating, so that drift and neighbours hit all three alike
        for name, fn in (("before", before), ("inside", inside), ("given", given)):
            t0 = time.perf_counter()
            last[name] = fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"bench": "lang_detect_session", "model": args.model, "compute": args.compute, "rows": B, "clips": N, "n_lang": n_lang,
           "detect_before_session_ms": spread(t["before"]), "detect_inside_session_ms": spread(t["inside"]),
           "unarmed_session_languages_given_ms": spread(t["given"]),
           "saving_ms_per_clip": round((med["before"] - med["inside"]) / N, 3),
           "inside_over_given": round(med["inside"] / med["given"], 4),
           "decode_steps": {k: int(last[k][2]["steps"]) for k in last},
           "encode_ms_session": {k: round(last[k][2]["encode_ms"], 1) for k in last},
           "languages_equal": last["inside"][0] == last["before"][0], "tokens_equal": last["inside"][1] == last["before"][1],
           "method": "host wall time around whole runs (every run ends in the session's last synchronise); each path warmed, "
                     "then alternated"}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
