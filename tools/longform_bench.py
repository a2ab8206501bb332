"""Long-form folder job: lock-step transcribe_many against transcribe_many(continuous=True), in one process on the same files.

Workload: large-v3 geometry (synthetic weights), bf16, max_batch 30, beam 5, a synthetic folder of files of 45 ... 240 s.  The EOT
row of the token embedding is scaled (--eot-boost, as refill_bench.py --beam) so that windows end at spread lengths.  Two regimes:
  thresholds off   no_speech / log-prob / compression thresholds None, temperature 0 only: the refill alone;
  reference        the reference job's defaults (temperature ladder 0.0 ... 1.0, best_of 5, thresholds 2.4 / -1.0 / 0.6).  On
                   synthetic weights almost every window falls back, so attempts per window are reported; fewer files
                   (--fallback-files) keep the lock-step run's serial tail within a few minutes.
For each regime and each form: audio-s/s (wall), encoder and decode GPU ms, decode steps and mean live rows per step (the
continuous form's from ttasr_session_stats; the lock-step form's decode steps are the beam positions of its passes plus prompt +
sampled length of its single-window fallback attempts, and its live rows are not reported), windows and attempts, and whether the
two forms returned identical segments (they need not: the lock-step form gives a pass one budget and decodes temperature 0 with
beam search even at beam 1, the continuous form runs transcribe()'s per-file algorithm).

    python tools/longform_bench.py [--files 24] [--fallback-files 8] [--max-new 224] [--regime off|ref|both] [--out FILE]

--word-timestamps [--retry-held {0,1}] (profiles/continuous_words.json) measures the continuous form only,
in both regimes: without words (the form above), with words through the packed alignment pass, with words through the padded
pass (a switch of this tool: the engine's option is forced to 0), with the other value of retry_held, and retry_held=True
without words.  Alignment ms is the host time inside Session.align, which returns with its results on the host.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from taiwan_tongues_asr_ce_amd import synth  # noqa: E402
from taiwan_tongues_asr_ce_amd.engine import Engine  # noqa: E402
from taiwan_tongues_asr_ce_amd.model import WhisperModel  # noqa: E402


def folder(n, seed=0):
    """n files of 45 ... 240 s built from the synthetic 30-s clip kinds."""
    kinds = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sec = int(rng.integers(45, 241))
        parts, have, k = [], 0, 0
        while have < sec * 16000:
            c = kinds[(i + k) % 3](1000 * seed + 50 * i + k)
            parts.append(c)
            have += len(c)
            k += 1
        out.append(np.concatenate(parts)[: sec * 16000].astype(np.float32))
    return out


def make_engine_class(boost, counters):
    class BenchEngine(Engine):
        """Engine with the EOT embedding row scaled and the lock-step path's GPU phases and calls counted."""

        def load_weights(self, tensors):
            def scaled():
                for name, w in tensors:
                    if name == "model.decoder.embed_tokens.weight":
                        w = np.array(w, copy=True)
                        w[self.special.eot] *= boost
                    yield name, w
            return super().load_weights(scaled())

        def log_mel_windows(self, *a, **kw):
            r = super().log_mel_windows(*a, **kw)
            if not kw.get("want_max"):
                counters["encode_ms"] += self.phase_ms()["mel"]
            return r

        def encode(self, B, *a, **kw):
            r = super().encode(B, *a, **kw)
            ph = self.phase_ms()
            counters["encode_ms"] += ph["encoder"] + ph["cross_kv"]
            return r

        def generate_beam(self, prompts, beam, opts, *a, **kw):
            r = super().generate_beam(prompts, beam, opts, *a, **kw)
            counters["decode_ms"] += self.phase_ms()["decode"]
            counters["steps"] += int(self.beam_profile()["positions"])
            counters["attempts"] += len(prompts)
            return r

        def generate_sample(self, prompts, best_of, opts, *a, **kw):
            r = super().generate_sample(prompts, best_of, opts, *a, **kw)
            counters["decode_ms"] += self.phase_ms()["decode"]
            counters["steps"] += len(prompts[0]) - 1 + max(len(t) for t in r.tokens)
            counters["attempts"] += len(prompts)
            return r

        def session(self, *a, **kw):
            s = super().session(*a, **kw)
            counters["on_session"](s)
            return s

        def set_option(self, key, value):
            # bench-only switch: the words run through the PADDED alignment pass (what ttasr_session_align does with the option off)
            if key == "align_packed" and counters.get("force_padded"):
                value = 0
            super().set_option(key, value)
    return BenchEngine


def run(model, counters, files, kw, continuous, session_prefill=0, words=False, retry_held=None, padded=False):
    for k in ("encode_ms", "decode_ms", "steps", "attempts", "align_ms", "align_calls", "align_clips"):
        counters[k] = 0
    counters["force_padded"] = bool(padded)
    stats = {}
    if words or retry_held is not None:
        kw = dict(kw, word_timestamps=bool(words), retry_held=retry_held)

    def on_session(sess):   # the session's statistics are read just before it ends
        close, align = sess.close, sess.align

        def timed_align(ids, *a, **k):   # Session.align returns with its results on the host: the host clock covers the pass
            t0 = time.perf_counter()
            r = align(ids, *a, **k)
            counters["align_ms"] += (time.perf_counter() - t0) * 1e3
            counters["align_calls"] += 1
            counters["align_clips"] += len(ids)
            return r
        sess.align = timed_align

        def close_with_stats():
            if sess.open:
                stats.update(sess.stats())
            close()
        sess.close = close_with_stats
    counters["on_session"] = on_session
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        if session_prefill:
            kw = dict(kw, session_prefill=session_prefill)
        out = model.transcribe_many(files, continuous=continuous, **kw)
        dt = time.perf_counter() - t0
    audio_s = sum(len(f) for f in files) / 16000.0
    segs = [s for s, _ in out]
    windows = sum(len({seg.seek for seg in fs}) for fs in segs)
    m = {"wall_s": round(dt, 2), "audio_s_per_s": round(audio_s / dt, 1), "segments": sum(len(s) for s in segs),
         "windows_with_segments": windows}
    if continuous:
        m.update({"encode_ms": round(stats["encode_ms"], 1), "decode_ms": round(stats["decode_ms"], 1),
                  "decode_steps": int(stats["steps"]), "attempts": int(stats["clips_encoded"]),
                  "mean_live_rows_per_step": round(stats["live_row_steps"] / max(1.0, stats["steps"]), 2),
                  "encoder_passes": int(stats["encodes"])})
        if words or retry_held is not None:
            m.update({"word_timestamps": bool(words), "retry_held": retry_held, "align_pass": "padded" if padded else "packed",
                      "align_ms": round(counters["align_ms"], 1), "align_calls": counters["align_calls"],
                      "align_clips": counters["align_clips"], "words": sum(len(seg.words or []) for fs in segs for seg in fs)})
        if session_prefill:   # the admission passes of option session_prefill
            m.update({"session_prefill": int(session_prefill), "prefill_passes": int(stats["prefill_passes"]),
                      "prefill_clips": int(stats["prefill_clips"]), "prefill_positions": int(stats["prefill_positions"]),
                      "prefill_ms": round(stats["prefill_ms"], 1)})
    else:
        m.update({"encode_ms": round(counters["encode_ms"], 1), "decode_ms": round(counters["decode_ms"], 1),
                  "decode_steps": counters["steps"], "attempts": counters["attempts"]})
    m["temperatures_used"] = sorted({seg.temperature for fs in segs for seg in fs})
    return segs, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--fallback-files", type=int, default=8)
    ap.add_argument("--max-new", type=int, default=224, help="max_new_tokens of every window (the reference's 448 // 2)")
    ap.add_argument("--eot-boost", type=float, default=8.0)
    ap.add_argument("--max-batch", type=int, default=30)
    ap.add_argument("--regime", default="both", choices=["off", "ref", "both"],
                    help="off: thresholds off only; ref: reference defaults only (on --fallback-files files)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--xkv-fp8", type=int, default=0, choices=[0, 1, 2],
                    help="option xkv_fp8: 0 the 16-bit cross-KV cache, 1 the e4m3 copy for unshared static rows only, 2 wherever a "
                         "kernel for it exists (shared rows, sessions)")
    ap.add_argument("--session-prefill", type=int, default=0, metavar="N",
                    help="also run the continuous form with transcribe_many(session_prefill=N): prompts of at least N prefillable "
                         "positions come from an admission pass of the session instead of forced decode steps")
    ap.add_argument("--word-timestamps", action="store_true",
                    help="measure transcribe_many(continuous=True, word_timestamps=True) instead: the continuous form without words, "
                         "words with the packed alignment pass, words with the padded pass (a bench-only switch), and --retry-held")
    ap.add_argument("--retry-held", type=int, default=1, choices=[0, 1],
                    help="with --word-timestamps: the value of retry_held for the words runs; the other value is measured as well")
    args = ap.parse_args()
    counters = {}
    model = WhisperModel(f"synthetic:{args.model}", device="cuda", compute_type="bfloat16", max_batch=args.max_batch,
                         pipeline_depth=1, cross_kv_fp8=args.xkv_fp8 == 2,
                         _engine_factory=make_engine_class(args.eot_boost, counters))
    if args.xkv_fp8 == 1:
        model.engine.set_option("xkv_fp8", 1)   # the continuous runs are refused in this mode
    base = dict(language="zh", beam_size=5, condition_on_previous_text=True, max_new_tokens=args.max_new)
    off = dict(base, temperature=0.0, no_speech_threshold=None, log_prob_threshold=None, compression_ratio_threshold=None)
    ref = dict(base)   # the reference defaults: ladder 0.0 ... 1.0, best_of 5, thresholds 2.4 / -1.0 / 0.6
    files = folder(args.files)
    # warm-up: graph captures and first-touch allocations of both forms
    warm = [f[: 16000 * 45] for f in files[:2]]
    for cont in (False, True):
        run(model, counters, warm, dict(off, max_new_tokens=16), cont)
    if args.session_prefill:
        run(model, counters, warm, dict(off, max_new_tokens=16), True, args.session_prefill)
    line = {"metric": "longform_audio_s_per_s", "model": args.model, "compute": "bf16", "xkv_fp8": args.xkv_fp8, "max_batch": args.max_batch, "beam": 5,
            "eot_boost": args.eot_boost, "max_new_tokens": args.max_new, "files": args.files,
            "audio_s": round(sum(len(f) for f in files) / 16000.0, 1)}
    if args.word_timestamps:
        def strip(fs):   # what must not change when words are added
            return [[(g.id, g.seek, g.tokens, g.temperature, g.avg_logprob, g.no_speech_prob) for g in f] for f in fs]
        run(model, counters, warm, dict(off, max_new_tokens=16), True, words=True)
        line["metric"] = "continuous_words_audio_s_per_s"
        rh = bool(args.retry_held)
        for name, fl, kw in (("thresholds_off", files, off), ("reference_defaults", files[: args.fallback_files], ref)):
            if args.regime not in ("both", {"thresholds_off": "off", "reference_defaults": "ref"}[name]):
                continue
            s0, m0 = run(model, counters, fl, kw, True)
            s1, m1 = run(model, counters, fl, kw, True, words=True, retry_held=rh)
            s2, m2 = run(model, counters, fl, kw, True, words=True, retry_held=rh, padded=True)
            s3, m3 = run(model, counters, fl, kw, True, words=True, retry_held=not rh)
            s4, m4 = run(model, counters, fl, kw, True, retry_held=True)
            line[name] = {"files": len(fl), "audio_s": round(sum(len(f) for f in fl) / 16000.0, 1), "continuous": m0,
                          "words_packed": m1, "words_padded": m2, "words_packed_other_retry_held": m3, "no_words_retry_held": m4,
                          "ratio_words_packed_over_continuous": round(m1["audio_s_per_s"] / m0["audio_s_per_s"], 3),
                          "ratio_packed_over_padded": round(m1["audio_s_per_s"] / m2["audio_s_per_s"], 3),
                          "segments_identical_to_continuous": [int(strip(x) == strip(s0)) for x in (s1, s2, s3, s4)],
                          "word_starts_equal_packed_vs_padded": [
                              int(sum(a.start == b.start for f, g in zip(s1, s2) for x, y in zip(f, g) for a, b in zip(x.words or [], y.words or []))),
                              int(sum(len(x.words or []) for f in s1 for x in f))]}
            print(json.dumps(line[name]), file=sys.stderr, flush=True)
    elif args.regime in ("off", "both"):
        sa, a = run(model, counters, files, off, False)
        sb, b = run(model, counters, files, off, True)
        line["thresholds_off"] = {"lock_step": a, "continuous": b, "ratio": round(b["audio_s_per_s"] / a["audio_s_per_s"], 3),
                                  "files_identical": int(sum(x == y for x, y in zip(sa, sb)))}
        if args.session_prefill:
            sp, pm = run(model, counters, files, off, True, args.session_prefill)
            line["thresholds_off"].update({"continuous_prefill": pm, "ratio_prefill_over_continuous": round(pm["audio_s_per_s"] / b["audio_s_per_s"], 3),
                                           "files_identical_prefill": int(sum(x == y for x, y in zip(sb, sp)))})
        print(json.dumps(line["thresholds_off"]), file=sys.stderr, flush=True)
    if not args.word_timestamps and args.regime in ("ref", "both"):
        ff = files[: args.fallback_files]
        sc, c = run(model, counters, ff, ref, False)
        sd, d = run(model, counters, ff, ref, True)
        n_win = max(1, sum(-(-len(f) // 480000) for f in ff))   # at least one window per 30 s (seeks may advance less)
        for m in (c, d):
            m["attempts_per_30s_window"] = round(m["attempts"] / n_win, 2)
        line["reference_defaults"] = {"files": len(ff), "audio_s": round(sum(len(f) for f in ff) / 16000.0, 1),
                                      "lock_step": c, "continuous": d,
                                      "ratio": round(d["audio_s_per_s"] / c["audio_s_per_s"], 3),
                                      "files_identical": int(sum(x == y for x, y in zip(sc, sd)))}
        if args.session_prefill:
            sp, pm = run(model, counters, ff, ref, True, args.session_prefill)
            pm["attempts_per_30s_window"] = round(pm["attempts"] / n_win, 2)
            line["reference_defaults"].update({"continuous_prefill": pm,
                                               "ratio_prefill_over_continuous": round(pm["audio_s_per_s"] / d["audio_s_per_s"], 3),
                                               "files_identical_prefill": int(sum(x == y for x, y in zip(sd, sp)))})
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
