"""ONE long recording: transcribe()'s window-by-window loop against the batched pipeline, in one process on the same audio.

Workload: large-v3 geometry (synthetic weights), bf16, max_batch 30, beam 5, one 600-s recording of noise bursts between digital
silences (the signal of tools/vad_bench.py), the VAD network with synthetic weights on the device.  The EOT row of the token
embedding is scaled (--eot-boost, as longform_bench.py) so that searches end at spread lengths.  Three forms:
  a  transcribe(vad_filter=True, condition_on_previous_text=False, without_timestamps=True): 30-s windows of the filtered audio in order
  b  BatchedInferencePipeline, retry_held=False: a failing group is released and submitted again (one encoder pass per attempt)
  c  BatchedInferencePipeline, retry_held=True: a failing group is retried on its held cross-KV (Session.retry)
and two regimes: the reference's default thresholds and ladder (on synthetic weights almost every attempt falls back), and
thresholds off with temperature 0.  Per form and regime, after --warmups runs, the median of --repeats runs with their spread:
audio-s/s (wall, VAD included), encoder and decode GPU ms, clips encoded, attempts, retries and mean live rows per decode step
(forms b and c, from ttasr_session_stats).  VAD ms is the device network over the recording, timed on its own.

    python tools/onefile_bench.py [--seconds 600] [--max-new 224] [--repeats 5] [--warmups 2] [--regime off|ref|both] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from longform_bench import make_engine_class  # noqa: E402
from vad_bench import bursts  # noqa: E402
from taiwan_tongues_asr_ce_amd import BatchedInferencePipeline, vad  # noqa: E402
from taiwan_tongues_asr_ce_amd.model import WhisperModel  # noqa: E402


def counting_engine_class(boost, counters):
    base = make_engine_class(boost, counters)

    class OneFileEngine(base):
        def encode(self, B, *a, **kw):
            counters["clips_encoded"] += B
            return super().encode(B, *a, **kw)
    return OneFileEngine


def run_form(model, counters, audio, form, kw):
    for k in ("encode_ms", "decode_ms", "steps", "attempts", "clips_encoded"):
        counters[k] = 0
    counters["on_session"] = lambda sess: None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        if form == "a":
            segs, info = model.transcribe(audio, vad_filter=True, condition_on_previous_text=False, **kw)
        else:
            segs, info = BatchedInferencePipeline(model).transcribe(audio, vad_filter=True, retry_held=form == "c", **kw)
        segs = list(segs)
        dt = time.perf_counter() - t0
    m = {"wall_s": dt, "audio_s_per_s": len(audio) / 16000.0 / dt, "segments": len(segs)}
    if form == "a":
        m.update(encode_ms=counters["encode_ms"], decode_ms=counters["decode_ms"], clips_encoded=counters["clips_encoded"],
                 attempts=counters["attempts"], retries=0)
    else:
        st = info.session
        m.update(encode_ms=st["encode_ms"], decode_ms=st["decode_ms"], clips_encoded=int(st["clips_encoded"]),
                 attempts=sum(len(c["attempts"]) for c in info.chunks), retries=int(st["retries"]), groups=len(info.chunks),
                 mean_live_rows_per_step=st["live_row_steps"] / max(1.0, st["steps"]), decode_steps=int(st["steps"]))
    return segs, m


def measure(model, counters, audio, form, kw, warmups, repeats):
    for _ in range(warmups):
        run_form(model, counters, audio, form, kw)
    runs = [run_form(model, counters, audio, form, kw) for _ in range(repeats)]
    segs = runs[0][0]
    assert all(s == segs for s, _ in runs), "a form must return the same segments in every run"
    rate = [m["audio_s_per_s"] for _, m in runs]
    out = {k: (round(statistics.median(m[k] for _, m in runs), 2) if isinstance(runs[0][1][k], float) else runs[0][1][k])
           for k in runs[0][1]}
    out["audio_s_per_s_min"], out["audio_s_per_s_max"] = round(min(rate), 2), round(max(rate), 2)
    return segs, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--max-new", type=int, default=224, help="max_new_tokens of every window / group (the reference's 448 // 2)")
    ap.add_argument("--eot-boost", type=float, default=8.0)
    ap.add_argument("--max-batch", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--regime", default="both", choices=["off", "ref", "both"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    counters = {k: 0 for k in ("encode_ms", "decode_ms", "steps", "attempts", "clips_encoded")}
    model = WhisperModel(f"synthetic:{args.model}", device="cuda", compute_type="bfloat16", max_batch=args.max_batch, pipeline_depth=1,
                         vad_model=vad.synth_silero_weights(), _engine_factory=counting_engine_class(args.eot_boost, counters))
    audio = bursts(1000, args.seconds)
    vad_ms = []
    for _ in range(args.warmups + args.repeats):
        t0 = time.perf_counter()
        model.vad_speech_probs([audio])
        vad_ms.append((time.perf_counter() - t0) * 1e3)
    base = dict(language="zh", beam_size=5, without_timestamps=True, max_new_tokens=args.max_new)
    regimes = {"reference_defaults": dict(base),   # ladder 0.0 ... 1.0, best_of 5, thresholds 2.4 / -1.0 / 0.6
               "thresholds_off": dict(base, temperature=0.0, no_speech_threshold=None, log_prob_threshold=None,
                                      compression_ratio_threshold=None)}
    want = {"off": ["thresholds_off"], "ref": ["reference_defaults"], "both": ["reference_defaults", "thresholds_off"]}[args.regime]
    line = {"metric": "onefile_audio_s_per_s", "model": args.model, "compute": "bf16", "max_batch": args.max_batch, "beam": 5,
            "eot_boost": args.eot_boost, "max_new_tokens": args.max_new, "audio_s": round(len(audio) / 16000.0, 1),
            "warmups": args.warmups, "repeats": args.repeats, "vad_ms": round(statistics.median(vad_ms[args.warmups:]), 2)}
    for name in want:
        res, segs = {}, {}
        for form in "abc":
            segs[form], res[form] = measure(model, counters, audio, form, regimes[name], args.warmups, args.repeats)
        res["b_c_identical"] = segs["b"] == segs["c"]
        res["c_encodes_one_clip_per_group"] = res["c"]["clips_encoded"] == res["c"]["groups"]
        res["pipeline_over_transcribe"] = round(res["c"]["audio_s_per_s"] / res["a"]["audio_s_per_s"], 3)
        res["retry_over_resubmit"] = round(res["c"]["audio_s_per_s"] / res["b"]["audio_s_per_s"], 3)
        line[name] = res
        print(json.dumps({name: res}), file=sys.stderr, flush=True)
    model.close()
    out = json.dumps(line)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
