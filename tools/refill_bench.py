"""Continuous batching against the static path, in one process on the same clips and budgets.

Workload: large-v3 geometry (synthetic weights), bf16, 256 synthetic 30-s clips, 4-token prompt, seeded per-clip token budgets
uniform in 32 ... 128 (synthetic weights emit no meaningful EOT: the budgets are the lengths).
  (a) static: batches of 32 clips through log-mel, encoder and ttasr_generate_capped (what bench.py side.ragged times);
  (b) the session (ttasr_session_*) with option refill_overlap = 0 (the default): the next clips are encoded between two step runs;
  (c) the session with refill_overlap = 1 (opt-in, a second stream): the next clips are encoded while the decode steps run.
Prints one JSON line: audio-s/s, encoder / decode GPU ms, mean live rows per decode step, b/a and c/a, and whether every clip's
tokens agree across the three runs.

    python tools/refill_bench.py [--clips 256] [--model large-v3] [--check-interval 8] [--out profiles/refill_bench.json]

--beam K: the beam-search form.  max_batch 30 (the streaming default, 6 groups of 5), 120 synthetic clips of 10 ... 30 s; the EOT
row of the token embedding is scaled (--eot-boost) so that hypotheses finish at spread positions (the length histogram is printed).
  (a) static: lock-step ttasr_generate_beam passes of G = max_batch / K clips (prefill = 0 and enc_gemm = 3, the session's forms);
  (b) the beam session (ttasr_session_begin_beam), refill_overlap = 0;  (c) the same with refill_overlap = 1.
    python tools/refill_bench.py --beam 5 [--clips 120] [--eot-boost 8] [--out profiles/refill_beam_bench.json]

--prev-tokens P[,P...] with --session-prefill N[,N...]: the threshold sweep of option session_prefill.  Only
the session runs (refill_overlap = 0), once per (P, N): every clip carries a previous-text prompt of P random tokens in front of the
sot sequence, and clips with at least N prefillable positions get them from an admission pass (N = 0: forced through decode
steps).  One JSON line per pair - audio-s/s, steps, live rows per step, decode / encoder ms, the four prefill statistics and whether
the tokens equal the N = 0 run - appended to --out.  With --beam K the same through the beam session.
    python tools/refill_bench.py --clips 64 --prev-tokens 8,16,32,64,128,223 --session-prefill 0,1,8,16,32,64 [--beam 5] \
        --out profiles/session_prefill_threshold.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from taiwan_tongues_asr_ce_amd import synth  # noqa: E402
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, PRESETS  # noqa: E402
from taiwan_tongues_asr_ce_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--check-interval", type=int, default=8)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--only-overlap", action="store_true", help="time (c) alone (for a kernel trace of the session)")
    ap.add_argument("--no-graph", action="store_true",
                    help="option graph = 0 (decode steps launched one by one): for rocprofv3, which crashes inside hipGraph capture")
    ap.add_argument("--beam", type=int, default=0, help="beam width: compare static beam passes with the beam session")
    ap.add_argument("--eot-boost", type=float, default=8.0, help="--beam: scale of the EOT embedding row (synthetic weights)")
    ap.add_argument("--xkv-fp8", type=int, default=0, choices=[0, 1, 2],
                    help="option xkv_fp8: 0 the 16-bit cross-KV cache, 1 the e4m3 copy for unshared static rows only, 2 wherever a "
                         "kernel for it exists (shared rows, sessions)")
    ap.add_argument("--prev-tokens", default=None, help="comma list: previous-text tokens in front of the sot sequence (the session_prefill sweep)")
    ap.add_argument("--session-prefill", default="0", help="comma list of option session_prefill values for the sweep")
    args = ap.parse_args()
    if args.prev_tokens is not None:
        return main_prefill_sweep(args)
    if args.beam:
        return main_beam(args)
    dims = PRESETS[args.model]
    B, N = args.batch, args.clips
    eng = Engine(dims, COMPUTE_BF16, B)
    eng.load_weights(synth.iter_weights(dims))
    if args.xkv_fp8:
        eng.set_option("xkv_fp8", args.xkv_fp8)   # 1: the session calls are refused
    if args.no_graph:
        eng.set_option("graph", 0)
    st = eng.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = eng.gen_opts(args.new_tokens, timestamps=False, suppress_eot=True, check_interval=args.check_interval)
    clips = [synth.noise_clip(i) for i in range(N)]
    caps = np.random.Generator(np.random.Philox(key=args.seed)).integers(32, args.new_tokens + 1, size=N).astype(np.int32)
    audio_s = 30.0 * N

    def static():
        toks, enc_ms, dec_ms, steps = [], 0.0, 0.0, 0
        for i in range(0, N, B):
            chunk = clips[i:i + B]
            eng.log_mel(chunk, want_output=False)
            eng.encode(len(chunk))
            toks += eng.generate([prompt] * len(chunk), opts, row_max_new=caps[i:i + B]).tokens
            ph = eng.phase_ms()
            enc_ms += ph["mel"] + ph["encoder"] + ph["cross_kv"]
            dec_ms += ph["decode"]
            steps += int(caps[i:i + B].max())
        live = float(caps.sum()) / steps     # sampling steps (the prompt is prefilled in one pass)
        return toks, {"encode_ms": round(enc_ms, 1), "decode_ms": round(dec_ms, 1), "decode_steps": steps,
                      "mean_live_rows_per_step": round(live, 2)}

    def session():
        out = [None] * N
        with eng.session(opts, len(prompt)) as s:
            ids = s.submit(clips, [prompt] * N, caps)
            where = {cid: i for i, cid in enumerate(ids)}
            for r in s.drain():
                out[where[r.id]] = r.tokens
            stt = s.stats()
        return out, {"encode_ms": round(stt["encode_ms"], 1), "decode_ms": round(stt["decode_ms"], 1), "decode_steps": int(stt["steps"]),
                     "polls": int(stt["polls"]), "encoder_passes": int(stt["encodes"]),
                     "mean_live_rows_per_step": round(stt["live_row_steps"] / max(1.0, stt["steps"]), 2)}

    def timed(fn):
        t0 = time.perf_counter()
        toks, m = fn()
        dt = time.perf_counter() - t0
        m.update({"wall_s": round(dt, 3), "audio_s_per_s": round(audio_s / dt, 1)})
        return toks, m

    # warm-up: graph captures and first-touch allocations of every path (the session's staging buffer included)
    keep = clips, caps, N
    clips, caps, N = clips[:B + 4], caps[:B + 4], B + 4
    static()
    eng.set_option("refill_overlap", 0)
    session()
    eng.set_option("refill_overlap", 1)
    session()
    clips, caps, N = keep

    if args.only_overlap:
        _, c = timed(session)
        print(json.dumps({"metric": "refill_audio_s_per_s", "model": args.model, "clips": N, "session_overlap": c}))
        eng.close()
        return
    ta, a = timed(static)
    eng.set_option("refill_overlap", 0)
    tb, b = timed(session)
    eng.set_option("refill_overlap", 1)
    tc, c = timed(session)
    line = {
        "metric": "refill_audio_s_per_s", "model": args.model, "compute": "bf16", "xkv_fp8": args.xkv_fp8, "clips": N, "batch": B,
        "budgets": {"lo": 32, "hi": args.new_tokens, "seed": args.seed, "mean": round(float(caps.mean()), 1)},
        "check_interval": args.check_interval, "prompt_tokens": len(prompt),
        "static": a, "session_sync": b, "session_overlap": c,
        "ratio_b_over_a": round(b["audio_s_per_s"] / a["audio_s_per_s"], 3),
        "ratio_c_over_a": round(c["audio_s_per_s"] / a["audio_s_per_s"], 3),
        "clips_equal_b_c": int(sum(x == y for x, y in zip(tb, tc))),
        "clips_equal_a_c": int(sum(x == y for x, y in zip(ta, tc))),
        "note": "b and c must agree on every clip (every session encoder pass runs the same GEMM family, so a clip's bits do "
                "not depend on how clips were grouped into passes); (a) prefills the prompt in one pass where the session "
                "forces it through decode steps, so a/c token equality holds only where those two prompt paths agree",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    eng.close()


def main_prefill_sweep(args):
    dims = PRESETS[args.model]
    K = args.beam
    B = (30 if args.batch == 32 else args.batch) if K else args.batch
    N = args.clips
    new_tokens = args.new_tokens if args.new_tokens != 128 else 96
    eng = Engine(dims, COMPUTE_BF16, B)
    eng.load_weights(synth.iter_weights(dims))
    if args.no_graph:
        eng.set_option("graph", 0)
    st = eng.special
    opts = eng.gen_opts(new_tokens, timestamps=False, suppress_eot=True, no_speech=False, check_interval=args.check_interval)
    clips = [synth.noise_clip(i) for i in range(N)]
    caps = np.random.Generator(np.random.Philox(key=args.seed)).integers(32, new_tokens + 1, size=N).astype(np.int32)
    rng = np.random.default_rng(args.seed)
    lines = []

    def run(prompts, n_pre):
        out = [None] * N
        t0 = time.perf_counter()
        with (eng.session(opts, len(prompts[0]), beam=K, prefill=n_pre) if K else eng.session(opts, len(prompts[0]), prefill=n_pre)) as s:
            ids = s.submit(clips, prompts, caps)
            where = {cid: i for i, cid in enumerate(ids)}
            for r in s.drain():
                out[where[r.id]] = r.tokens
            stt = s.stats()
        dt = time.perf_counter() - t0
        return out, stt, dt

    for P in [int(v) for v in args.prev_tokens.split(",")]:
        prompts = [[st.sot_prev] + rng.integers(300, 20000, size=P).tolist() + [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
                   for _ in range(N)]
        base = None
        for n_pre in [int(v) for v in args.session_prefill.split(",")]:
            run(prompts[:B + 2] + prompts[:N - B - 2], n_pre)              # warm-up: graphs, the pass's workspace
            toks, stt, dt = run(prompts, n_pre)
            if n_pre == 0:
                base = toks
            line = {"metric": "session_prefill_threshold", "model": args.model, "compute": "bf16", "beam": K, "max_batch": B, "clips": N,
                    "prev_tokens": P, "prompt_tokens": len(prompts[0]), "session_prefill": n_pre,
                    "audio_s_per_s": round(30.0 * N / dt, 1), "wall_s": round(dt, 3), "decode_steps": int(stt["steps"]),
                    "mean_live_rows_per_step": round(stt["live_row_steps"] / max(1.0, stt["steps"]), 2),
                    "decode_ms": round(stt["decode_ms"], 1), "encode_ms": round(stt["encode_ms"], 1),
                    "prefill_passes": int(stt["prefill_passes"]), "prefill_clips": int(stt["prefill_clips"]),
                    "prefill_positions": int(stt["prefill_positions"]), "prefill_ms": round(stt["prefill_ms"], 2),
                    "clips_equal_forced": None if base is None else int(sum(x == y for x, y in zip(toks, base)))}
            print(json.dumps(line), flush=True)
            lines.append(line)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
    eng.close()


def main_beam(args):
    dims = PRESETS[args.model]
    K = args.beam
    B = 30 if args.batch == 32 else args.batch      # --batch keeps its greedy default of 32; the beam form's default is 30
    G = B // K
    N = args.clips if args.clips != 256 else 120
    N = max(G, N - N % G)                            # whole static passes
    new_tokens = args.new_tokens if args.new_tokens != 128 else 96
    eng = Engine(dims, COMPUTE_BF16, B)
    st = eng.special

    def weights():
        for name, w in synth.iter_weights(dims):
            if name == "model.decoder.embed_tokens.weight":
                w = w.copy()
                w[st.eot] *= args.eot_boost
            yield name, w
    eng.load_weights(weights())
    if args.xkv_fp8:
        eng.set_option("xkv_fp8", args.xkv_fp8)   # 1: the session calls are refused (and a static beam reads the 16-bit cache)
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = eng.gen_opts(new_tokens, timestamps=False)
    clips_all = [synth.noise_clip(i)[: 16000 * (10 + (7 * i) % 21)] for i in range(N)]
    audio_s_all = sum(len(c) for c in clips_all) / 16000.0
    clips = clips_all

    def static():
        toks, enc_ms, dec_ms, steps = [], 0.0, 0.0, 0
        eng.set_option("prefill", 0)
        eng.set_option("enc_gemm", 3)
        for i in range(0, len(clips), G):
            chunk = clips[i:i + G]
            eng.log_mel(chunk, want_output=False)
            eng.encode(len(chunk))
            toks += eng.generate_beam([prompt] * len(chunk), K, opts).tokens
            ph = eng.phase_ms()
            enc_ms += ph["mel"] + ph["encoder"] + ph["cross_kv"]
            dec_ms += ph["decode"]
            steps += int(eng.beam_profile()["positions"])
        eng.set_option("prefill", 1)
        eng.set_option("enc_gemm", 0)
        return toks, {"encode_ms": round(enc_ms, 1), "decode_ms": round(dec_ms, 1), "decode_steps": steps}

    def session():
        out = [None] * len(clips)
        with eng.session(opts, len(prompt), beam=K) as s:
            ids = s.submit(clips, [prompt] * len(clips))
            where = {cid: i for i, cid in enumerate(ids)}
            for r in s.drain():
                out[where[r.id]] = r.tokens
            stt = s.stats()
        return out, {"encode_ms": round(stt["encode_ms"], 1), "decode_ms": round(stt["decode_ms"], 1), "decode_steps": int(stt["steps"]),
                     "encoder_passes": int(stt["encodes"]), "live_row_steps": int(stt["live_row_steps"]),
                     "mean_live_rows_per_step": round(stt["live_row_steps"] / max(1.0, stt["steps"]), 2)}

    def timed(fn):
        t0 = time.perf_counter()
        toks, m = fn()
        dt = time.perf_counter() - t0
        audio_s = sum(len(c) for c in clips) / 16000.0
        m.update({"wall_s": round(dt, 3), "audio_s_per_s": round(audio_s / dt, 1),
                  "ms_per_step": round(m["decode_ms"] / max(1, m["decode_steps"]), 3)})
        return toks, m

    # warm-up: graph captures and first-touch allocations of every path
    clips = clips_all[:2 * G]
    static()
    for ov in (0, 1):
        eng.set_option("refill_overlap", ov)
        session()
    clips = clips_all
    ta, a = timed(static)
    eng.set_option("refill_overlap", 0)
    tb, b = timed(session)
    eng.set_option("refill_overlap", 1)
    tc, c = timed(session)
    eng.set_option("refill_overlap", 0)
    # every clip takes the same number of steps in both forms (same decisions), so the static pass's live row-steps are the session's
    a["mean_live_rows_per_step"] = round(b["live_row_steps"] / max(1, a["decode_steps"]), 2)
    lens = [len(t) for t in tb]
    hist = {}
    for n in lens:
        k = f"{(n // 8) * 8}-{(n // 8) * 8 + 7}"
        hist[k] = hist.get(k, 0) + 1
    print("token-length histogram:", dict(sorted(hist.items(), key=lambda kv: int(kv[0].split("-")[0]))), file=sys.stderr)
    line = {
        "metric": "refill_beam_audio_s_per_s", "model": args.model, "compute": "bf16", "xkv_fp8": args.xkv_fp8, "beam": K, "max_batch": B, "groups": G,
        "clips": N, "audio_s": round(audio_s_all, 1), "eot_boost": args.eot_boost, "max_new_tokens": new_tokens,
        "prompt_tokens": len(prompt), "length_histogram": hist, "mean_tokens": round(float(np.mean(lens)), 1),
        "static": a, "session_sync": b, "session_overlap": c,
        "ratio_b_over_a": round(b["audio_s_per_s"] / a["audio_s_per_s"], 3),
        "ratio_c_over_a": round(c["audio_s_per_s"] / a["audio_s_per_s"], 3),
        "clips_equal_a_b": int(sum(x == y for x, y in zip(ta, tb))),
        "clips_equal_a_c": int(sum(x == y for x, y in zip(ta, tc))),
        "all_clips_agree": all(x == y == z for x, y, z in zip(ta, tb, tc)),
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    eng.close()


if __name__ == "__main__":
    main()
