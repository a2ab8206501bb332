#!/usr/bin/env python3
"""Headline benchmark: audio-seconds transcribed per wall-second, whisper-large-v3 geometry, greedy,
30-s clips, batch 32 per GPU (BASELINE.json metric / configs[2]); data-parallel over N GPUs (configs[3]).

One "step" = the whole hot path over one batch of synthetic clips, timed as SURVEY.md section 8(d) defines the metric:
PCM f32 resident in PINNED HOST memory -> token ids on the host (H2D copy + log-mel -> encoder -> cross-KV -> 4-token prompt
+ 128 greedy tokens, EOT suppressed so every run decodes the same length).  The same K steps with the PCM already resident in
HBM are timed right after and reported beside it (`config.hbm_resident`; 0.3-0.4 % faster).  Weights are seeded synthetic tensors of the named geometry (no
checkpoint exists offline).  Launch: `python bench.py` (1 GPU), `python bench.py --gpus N` (spawns its own N rank
processes) or `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`.
Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def cpu_baseline(dims, n_new: int, budget_layers: int = 2, budget_steps: int = 6):
    """Time the CPU oracle (oracle/whisper_ref.py, a port of the reference's HF path) on a bounded sample
    of the same workload: ONE 30-s clip, full log-mel + conv stem, `budget_layers` of the encoder layers,
    cross-KV + `budget_steps` decode steps of `budget_layers` decoder layers, all at large-v3 width; the
    per-layer / per-step times are scaled to the full depth and token count.  Returns audio-s/s."""
    import torch
    from oracle import whisper_ref as R
    from taiwan_tongues_asr_ce_amd import synth
    torch.set_grad_enabled(False)
    # oversubscribing small ops with hundreds of threads is pathologically slow in torch: use at most 32
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    L = budget_layers
    sub = R.Dims(dims.n_mels, dims.n_audio_ctx, dims.d_model, dims.n_heads, dims.ffn_dim, L, L, dims.vocab, dims.n_text_ctx)
    want = set()
    for name, shape, kind in synth.tensor_specs(dims):
        parts = name.split(".")
        if "layers" in parts and int(parts[parts.index("layers") + 1]) >= L:
            continue
        want.add((name, shape, kind))
    W = {n: torch.from_numpy(synth.make_tensor(n, s, k)) for n, s, k in want}
    clip = synth.noise_clip(0)
    t0 = time.perf_counter()
    mel = torch.from_numpy(R.log_mel(clip, dims.n_mels))[None]
    t_mel = time.perf_counter() - t0
    R.encoder_stem(mel, W)  # warm-up (thread pool, allocator), then time
    t0 = time.perf_counter()
    x = R.encoder_stem(mel, W)
    t_stem = time.perf_counter() - t0
    R.encoder_layer(x, W, "model.encoder.layers.0", dims.n_heads)  # warm-up
    t0 = time.perf_counter()
    for i in range(L):
        x = R.encoder_layer(x, W, f"model.encoder.layers.{i}", dims.n_heads)
    t_layer = (time.perf_counter() - t0) / L
    enc = R._ln(x, W["model.encoder.layer_norm.weight"], W["model.encoder.layer_norm.bias"])
    R.cross_kv(enc, W, sub)  # warm-up
    t0 = time.perf_counter()
    xkv = R.cross_kv(enc, W, sub)
    t_xkv = (time.perf_counter() - t0) / L
    cache = R.SelfCache.empty(L)
    R.decoder_forward(torch.tensor([[1]]), cache, xkv, W, sub)  # warm
    t0 = time.perf_counter()
    for s in range(budget_steps):
        R.decoder_forward(torch.tensor([[s + 2]]), cache, xkv, W, sub)
    t_step_L = (time.perf_counter() - t0) / budget_steps
    # a step = L decoder layers + the vocabulary projection; separate the two by timing the projection
    h = torch.randn(1, dims.d_model)
    t0 = time.perf_counter()
    for _ in range(3):
        h @ W["model.decoder.embed_tokens.weight"].t()
    t_vocab = (time.perf_counter() - t0) / 3
    t_dec_layer = max(t_step_L - t_vocab, 0.0) / L
    n_steps = 4 + n_new - 1
    total = (t_mel + t_stem + dims.enc_layers * t_layer + dims.dec_layers * t_xkv
             + n_steps * (dims.dec_layers * t_dec_layer + t_vocab))
    return {"value": round(30.0 / total, 4), "unit": "audio-s/s", "cores": cores, "kind": "port",
            "sample": (f"EXTRAPOLATED from a bounded sample (cpu_baseline.value is the complete run): oracle/whisper_ref.py (torch CPU f32, {cores} threads), 1 clip of the same workload: log-mel + "
                       f"stem + {L}/{dims.enc_layers} encoder layers, cross-KV and {budget_steps} decode steps of "
                       f"{L}/{dims.dec_layers} decoder layers at large-v3 width, scaled linearly to full depth and "
                       f"{n_steps} steps; est. {total:.1f} s per 30-s clip. The reference's own CPU path "
                       f"(CTranslate2 int8, api/file_asr.py:188) is not installable offline")}


def cpu_baseline_full(dims, n_new: int):
    """ONE complete run of the CPU oracle on the headline workload at B = 1: full large-v3 depth,
    one 30-s clip, 4-token prompt + n_new greedy tokens with EOT suppressed.  Minutes of host time: run once with
    `python bench.py --cpu-full` on the GPU box and cached under profiles/ (the default run reads the cache)."""
    import torch
    from oracle import whisper_ref as R
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import SpecialTokens
    from taiwan_tongues_asr_ce_amd.engine import default_suppress
    torch.set_grad_enabled(False)
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    rd = R.Dims(**dims.as_dict())
    W = R.to_torch(synth.state_dict(dims))
    st = SpecialTokens.for_vocab(dims.vocab)
    clip = synth.noise_clip(0)
    t0 = time.perf_counter()
    mel = torch.from_numpy(R.log_mel(clip, dims.n_mels))[None]
    enc = R.encoder_forward(mel, W, rd)
    t_enc = time.perf_counter() - t0
    rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                    suppress=default_suppress(st, rd.vocab) + [st.eot], begin_suppress=[220, st.eot], timestamps=False)
    ref = R.greedy_decode(enc, [st.sot, st.lang_zh, st.transcribe, st.no_timestamps], W, rd, rules, n_new)
    total = time.perf_counter() - t0
    return {"value": round(30.0 / total, 4), "unit": "audio-s/s", "cores": cores, "kind": "port", "seconds": round(total, 1),
            "encoder_seconds": round(t_enc, 1), "tokens": len(ref.tokens[0]), "cpu": _cpu_model(),
            "sample": f"oracle/whisper_ref.py (a port of the reference's HF path), ONE COMPLETE run executed live: 1 clip x 30 s of the workload, "
                      f"all {dims.enc_layers}+{dims.dec_layers} layers, 4-token prompt + {n_new} greedy tokens (EOT suppressed), torch "
                      f"CPU f32, {cores} threads; {total:.1f} s of host time.  The reference's own CPU path (CTranslate2 int8, "
                      f"api/file_asr.py:188) is not installable offline"}


def cpu_baseline_matrix(n_new: int, budget_s: float = 40.0):
    """SURVEY.md section 8(d)'s small rows: the CPU oracle end to end (log-mel -> encoder -> cross-KV -> 4-token prompt + n_new
    greedy tokens, EOT suppressed) on the tiny and small geometries at B = 1 and B = 8, complete runs (no extrapolation).
    Rows are taken in order of cost and the loop stops once `budget_s` of host time is spent (skipped rows are listed)."""
    import torch
    from oracle import whisper_ref as R
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import PRESETS, SpecialTokens
    from taiwan_tongues_asr_ce_amd.engine import default_suppress
    torch.set_grad_enabled(False)
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    rows, spent, t_b1 = [], 0.0, {}
    for name, B in (("tiny", 1), ("tiny", 8), ("small", 1), ("small", 8)):
        predicted = t_b1.get(name, 0.0) * B * 0.85          # a batch of B costs about B x the single clip on these host cores
        if spent + predicted > budget_s:
            rows.append({"model": name, "batch": B, "skipped": f"predicted {predicted:.0f} s: over the host-time budget "
                                                               f"({budget_s:.0f} s) of the default run; see profiles/ for a full run"})
            continue
        dims = PRESETS[name]
        rd = R.Dims(**dims.as_dict())
        W = R.to_torch(synth.state_dict(dims))
        st = SpecialTokens.for_vocab(dims.vocab)
        clips = [synth.noise_clip(b) for b in range(B)]
        rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                        suppress=default_suppress(st, rd.vocab) + [st.eot], begin_suppress=[220, st.eot], timestamps=False)
        t0 = time.perf_counter()
        res = R.transcribe_tokens(clips, W, rd, [st.sot, st.lang_zh, st.transcribe, st.no_timestamps], rules, n_new)
        dt = time.perf_counter() - t0
        spent += dt
        if B == 1:
            t_b1[name] = dt
        assert all(len(t) == n_new for t in res.tokens)
        rows.append({"model": name, "batch": B, "seconds": round(dt, 2), "audio_s_per_s": round(B * 30.0 / dt, 2)})
    return {"cores": cores, "kind": "port", "new_tokens": n_new, "rows": rows}


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def xattn_traffic_from_profile(xp: dict, sig: str, B: int):
    """(traffic bytes per launch | None, note): the committed PMC profile of the dominant kernel is used ONLY when it was taken on
    the kernel signature (name, template arguments, grid) this run launched - otherwise null plus the reason, never a stale number."""
    sigs = xp.get("signatures") or []
    if sig and sig in sigs:
        return (round(xp["traffic_bytes_per_32row_launch"] * B / 32.0),
                f"profiles/xattn_pmc.json, taken on `{sig}` = the kernel this run launched (static: separate rocprofv3 --pmc passes, "
                f"not re-measured by this run)")
    return None, (f"stale profile: profiles/xattn_pmc.json was taken on {sigs or [xp.get('kernel')]}, this run launched `{sig}` - "
                  f"re-run the --pmc passes (tools/gpu_session.sh)")


def pmc_busy_from_profile(kernels: dict, sigs, flops):
    """(flop-weighted MFMA-busy fraction | None, note) of the kernels with signatures `sigs` from a committed *_pmc.json; None when
    any of them has no entry taken on exactly that signature."""
    fr = []
    for sig in sigs:
        hit = [v["mfma_busy_frac"] for v in kernels.values() if sig and sig in v.get("signatures", []) and "mfma_busy_frac" in v]
        if not hit:
            return None, (f"stale profile: no entry taken on `{sig}` (the encoder GEMM kernels this run launched: {list(sigs)}) - "
                          f"re-run the --pmc passes (tools/gpu_session.sh)")
        fr.append(hit[0])
    return round(sum(flops) / sum(f / b for f, b in zip(flops, fr)), 4), None


def _self_launch(n: int, cmd=None) -> int:
    """`python bench.py --gpus N` from a bare shell (no torchrun environment): this parent process touches no GPU - it
    only spawns the N rank processes (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set exactly as
    torch.distributed.run would) and relays rank 0's JSON line.  Nothing is exec'ed over an initialised GPU process.
    `cmd` (tests): the rank command line instead of this script's own."""
    import socket
    import subprocess
    import torch
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if torch.cuda.device_count() < n:   # device_count() does not initialise the GPU
        # fewer devices than ranks: the ranks share GPUs and talk over gloo (RCCL refuses two ranks per device).
        # Plumbing check only - the line then says so in config.parallelism
        env["TTASR_DIST_BACKEND"] = "gloo"
    procs = [subprocess.Popen(cmd or [sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL) for r in range(n)]
    # rank 0's stdout is drained on a thread so that the parent can watch every child: when ANY rank dies, the others - which
    # would otherwise sit in a collective until its timeout - are ended (by their exact PIDs) and the launch fails at once
    import threading
    out0 = []
    rd = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    failed = None
    while any(p.poll() is None for p in procs):
        bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad:
            failed = bad[0]
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            break
        time.sleep(0.2)
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(timeout=30))
        except subprocess.TimeoutExpired:
            p.kill()
            rcs.append(p.wait())
    rd.join(5)
    if failed is not None:
        print(f"bench.py --gpus {n}: rank {failed[0]} exited with code {failed[1]}; the other ranks were stopped", file=sys.stderr, flush=True)
        return abs(failed[1]) or 1
    for line in (out0[0].decode() if out0 else "").splitlines():   # rank 0 prints the ONE JSON line; library chatter is not relayed
        if line.startswith("{"):
            print(line, flush=True)
    return max(abs(rc) for rc in rcs)


def _host_greedy_prefix(eng, B, prompt, tokens, n_check, suppress, begin_suppress, eot):
    """Recompute the first n_check greedy choices of every row through the STEP API (ttasr_decode_step: raw logits to the
    host, rules + first-maximum argmax applied here in numpy) on the cross-KV the last timed step left resident,
    teacher-forced on the tokens the timed step produced.  The step API feeds the prompt token by token while generate()
    prefills it in one batched pass (other GEMM tiles: the last bits of the cached keys differ), so a disagreement is only
    accepted where the recomputed top-2 margin is within bf16 rounding distance of a tie.
    -> (positions compared, positions that agree, largest margin at a disagreement)."""
    eng.decode_reset(B)
    logits = None
    for t in prompt:
        logits = eng.decode_step([t] * B)
    sup = np.asarray(sorted(set(suppress) | {eot}), dtype=np.int64)     # benchmark mode: EOT suppressed
    bsup = np.asarray(begin_suppress, dtype=np.int64)
    agree, worst = 0, 0.0
    for i in range(n_check):
        lg = logits.copy()
        lg[:, sup] = -np.inf
        if i == 0:
            lg[:, bsup] = -np.inf
        mine = lg.argmax(axis=1)
        for b in range(B):
            if mine[b] == tokens[b, i]:
                agree += 1
            else:
                worst = max(worst, float(lg[b, mine[b]] - lg[b, tokens[b, i]]))
        if i + 1 < n_check:
            logits = eng.decode_step(tokens[:, i].tolist())
    return B * n_check, agree, worst


def _step_api_margins(eng, B, prompt, tokens, suppress, begin_suppress, eot):
    """Teacher-force the engine on `tokens` [B][n] through the STEP API and return, for every row and position, the margin of the
    chosen token over the best OTHER allowed token of the processed logits (float32 [B][n]; > 0 where the token is the argmax) and
    that other token (int32 [B][n]).  Run on the f32 parity engine (`--compute f32 --dump-tokens`) this is the evidence behind
    "a 16-bit engine leaves the f32 sequence only at a near-tie": profiles/bench_tokens_f32_margins.npy / _runner_up.npy."""
    n = tokens.shape[1]
    eng.decode_reset(B)
    logits = None
    for t in prompt:
        logits = eng.decode_step([t] * B)
    sup = np.asarray(sorted(set(suppress) | {eot}), dtype=np.int64)
    bsup = np.asarray(begin_suppress, dtype=np.int64)
    margin = np.zeros((B, n), dtype=np.float32)
    other = np.zeros((B, n), dtype=np.int32)
    rows = np.arange(B)
    for i in range(n):
        lg = logits.copy()
        lg[:, sup] = -np.inf
        if i == 0:
            lg[:, bsup] = -np.inf
        chosen = lg[rows, tokens[:, i]].copy()
        lg[rows, tokens[:, i]] = -np.inf
        other[:, i] = lg.argmax(axis=1)
        margin[:, i] = chosen - lg[rows, other[:, i]]
        if i + 1 < n:
            logits = eng.decode_step(tokens[:, i].tolist())
    return margin, other


def token_agreement(mine: np.ndarray, ref_file: str, model: str, clips: str):
    """Agreement of `mine` (int32 [B][n] greedy tokens of this run) with the committed tokens of another engine on this very
    workload (profiles/<ref_file>, [32][128], written by `bench.py --compute ... --dump-tokens`).  Greedy decoding is not
    teacher-forced, so once a row diverges the rest of it is a different sentence: reported are the rows that never diverge, each
    row's first divergent position, the equal-prefix fraction of all tokens and - when the reference is the f32 parity engine,
    whose per-position top-2 margins are committed beside its tokens - the F32 ENGINE'S OWN MARGIN at every first divergence and
    whether the 16-bit engine took the f32 runner-up (the checkable form of "it flipped a near-tie")."""
    B, n = mine.shape
    try:
        ref = np.load(os.path.join(ROOT, "profiles", ref_file))
    except Exception:
        return None
    if not (model == "large-v3" and clips == "noise" and ref.shape[0] >= B and ref.shape[1] >= n):
        return None
    neq = mine != ref[:B, :n]
    first = np.where(neq.any(axis=1), neq.argmax(axis=1), n)
    out = {"rows_identical": int((first == n).sum()), "rows": int(B),
           "equal_prefix_fraction": round(float(first.sum()) / (B * n), 4),
           "first_divergence_per_row": [int(x) for x in first],
           "source": f"profiles/{ref_file} (same clips / weights / prompt)"}
    stem = ref_file[:-4]
    try:
        mg = np.load(os.path.join(ROOT, "profiles", stem + "_margins.npy"))
        ru = np.load(os.path.join(ROOT, "profiles", stem + "_runner_up.npy"))
        div = [{"row": int(r), "position": int(first[r]), "ref_engine_top2_margin": round(float(mg[r, first[r]]), 5),
                "took_ref_runner_up": bool(ru[r, first[r]] == mine[r, first[r]])} for r in range(B) if first[r] < n]
        out["divergences"] = div
        out["largest_ref_margin_at_a_divergence"] = max((d["ref_engine_top2_margin"] for d in div), default=0.0)
        out["ref_margin_percentiles_all_positions"] = {q: round(float(np.percentile(mg[:B, :n], q)), 4) for q in (1, 5, 25, 50)}
        out["margins_source"] = f"profiles/{stem}_margins.npy (the reference engine's own processed top-2 margin at every position, step API)"
    except Exception:
        out["divergences"] = None
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict, limit: int = DUMP_LIMIT_BYTES) -> dict:
    """Write every array as float64 `out_dir/<name>.npy` so that two builds can be compared output for output.  An array whose
    share of `limit` is too small for it keeps a fixed, seeded sample of its rows (the same rows in every run).
    -> {name: {"shape": written shape, "rows_of": original row count}}."""
    os.makedirs(out_dir, exist_ok=True)
    share = limit // max(1, len(arrays))
    written = {}
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        rows = a.shape[0]
        row_bytes = max(1, a[:1].nbytes)
        if a.nbytes > share:
            keep = np.sort(np.random.Generator(np.random.Philox(key=0)).choice(rows, size=max(1, share // row_bytes), replace=False))
            a = a[keep]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
        written[name] = {"shape": list(a.shape), "rows_of": rows}
    return written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--compute", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--more-in-flight", action="store_true",
                    help="also report the 2-context side measurement (off by default so that a rocprofv3 run of the plain "
                         "command sees only single-context launches)")
    ap.add_argument("--validate", action="store_true",
                    help="multi-GPU validation mode: every rank decodes the same probe clip and the first-step logits are "
                         "gathered and compared (proves the RCCL weight broadcast)")
    ap.add_argument("--contexts", type=int, default=1,
                    help="opt-in serving configuration: this many independent engine contexts per GPU, each running the "
                         "whole step on its own batch of --batch clips from its own host thread (clips in flight per GPU "
                         "= contexts x batch; the latency-bound decode chains of one context fill the gaps of the other)")
    ap.add_argument("--cpu-full", action="store_true",
                    help="run ONE full large-v3 B = 1 pass of the CPU oracle (minutes) and cache it as profiles/cpu_baseline_full.json")
    ap.add_argument("--write-crc", action="store_true", help="record the token checksum of this run as the expected one")
    ap.add_argument("--xkv-fp8", action="store_true",
                    help="opt-in serving mode (NOT the headline): OCP e4m3 copy of the cross-KV cache read by the decode step's "
                         "cross-attention (ttasr_set_option xkv_fp8); the line's dtype says so and output_check reports the token "
                         "agreement with the bf16 and the f32 engines")
    ap.add_argument("--dump-tokens", default=None, help="save rank 0's int32 [B][new_tokens] token ids of the last timed step as .npy")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (the token ids of every rank's clips, "
                         "-1 = padding) as DIR/tokens.npy in float64; inputs are seeded, so runs with the same arguments compare "
                         "output for output")
    ap.add_argument("--no-side", action="store_true",
                    help="skip the side modes of the default run (fp16 engine, fp8 cross-KV cache, two contexts in flight): a "
                         "rocprofv3 run then sees only the headline configuration's launches")
    ap.add_argument("--side-steps", type=int, default=4, help="timed steps of every side mode")
    ap.add_argument("--option", action="append", default=[],
                    help="key=value passed to ttasr_set_option on every engine before its weights are loaded (A/B runs; the line "
                         "records them in config.options)")
    ap.add_argument("--clips", default="noise", choices=["noise", "tonal"],
                    help="synthetic clip set of the timed steps (SURVEY.md 8d: 0.1 N(0,1) noise; the tonal set - five sines - is "
                         "also measured as a side number by the default run)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_self_launch(args.gpus))

    import torch
    import torch.distributed as dist
    from taiwan_tongues_asr_ce_amd import synth
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd import dist as _dist_mod
    from taiwan_tongues_asr_ce_amd.dist import barrier as dist_barrier, broadcast_weights, gather_tokens, init_process_group
    from taiwan_tongues_asr_ce_amd.engine import Engine

    rank, world, local = init_process_group()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    local = local % max(torch.cuda.device_count(), 1)   # ranks > devices only in the shared-GPU plumbing smoke test
    torch.cuda.set_device(local)
    grp = dist.is_initialized()     # several ranks, or ONE rank with TTASR_DIST_FORCE=1 (the RCCL code paths on a 1-GPU box)
    transport = dist.get_backend() if grp else None
    dims = PRESETS[args.model]
    B = args.batch
    C_ = max(1, args.contexts)
    compute = {"bf16": COMPUTE_BF16, "f16": COMPUTE_F16, "f32": COMPUTE_F32}[args.compute]
    engines = [Engine(dims, compute, B, device=local) for _ in range(C_)]
    eng = engines[0]
    for kv in args.option:
        k_, v_ = kv.split("=", 1)
        for e_ in engines:
            e_.set_option(k_, int(v_))
    if args.xkv_fp8:
        if args.compute == "f32":
            raise SystemExit("--xkv-fp8 needs a 16-bit engine")
        for e_ in engines:
            e_.set_option("xkv_fp8", 1)
    t_load = time.perf_counter()
    for e_ in engines:
        if grp and os.environ.get("TTASR_BENCH_LOCAL_WEIGHTS") is None:
            # north_star: rank 0 owns the checkpoint, the others receive it over RCCL (xGMI broadcast, 256 MB buckets)
            broadcast_weights(e_, dims, src_iter=synth.iter_weights(dims) if rank == 0 else None, device=local)
        else:
            e_.load_weights(synth.iter_weights(dims))
    t_load = time.perf_counter() - t_load

    # synthetic clips: rank r owns clips [r*B, (r+1)*B) of the global batch (weak scaling)
    make_clip = synth.noise_clip if args.clips == "noise" else synth.tonal_clip
    pcm = torch.empty((B, 480000), dtype=torch.float32, device=f"cuda:{local}")
    for b in range(B):
        pcm[b] = torch.from_numpy(make_clip(rank * B + b)).to(pcm.device)
    ns = [480000] * B
    torch.cuda.synchronize()    # the engine reads pcm on its own (non-blocking) stream
    st = eng.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = eng.gen_opts(args.new_tokens, timestamps=False, suppress_eot=True, no_speech=True, check_interval=1 << 20)

    # the timed region starts with the PCM f32 in PINNED HOST memory and ends with the token ids on the host
    pcm_host = pcm.cpu().pin_memory()

    def one_pass_hbm(e_):
        e_.log_mel_device(pcm.data_ptr(), 480000, ns)
        e_.encode(B)
        return e_.generate([prompt] * B, opts).tokens

    def one_pass(e_):
        e_.log_mel_host_ptr(pcm_host.data_ptr(), 480000, ns)      # includes the H2D copy on the context's stream
        e_.encode(B)
        return e_.generate([prompt] * B, opts).tokens

    def local_pass(one):
        """This rank's batch(es) through the hot path; no collective."""
        if C_ == 1:
            return one(eng)
        # --contexts N: one step = every context passes its own batch, concurrently (ctypes releases the GIL)
        import threading
        out, errs = [None] * C_, []

        def run(i):
            try:
                out[i] = one(engines[i])
            except Exception as ex:
                errs.append(ex)
        th = [threading.Thread(target=run, args=(i,)) for i in range(C_)]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()
        if errs:
            raise errs[0]
        return [t for o in out for t in o]

    def step():
        return gather_tokens(local_pass(one_pass), args.new_tokens, device=local)

    for _ in range(args.warmup):
        step()
    phases, per_step = [], []
    if grp:
        dist_barrier(local)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        toks = step()                       # generate() returns host tokens: the step ends synchronised
        per_step.append(time.perf_counter() - ts)
        phases.append(eng.phase_ms())
    torch.cuda.synchronize()
    if grp:
        dist_barrier(local)
    dt = time.perf_counter() - t0
    rank_ms = None
    if grp:
        cdev = "cpu" if dist.get_backend() == "gloo" else f"cuda:{local}"
        t = torch.tensor([dt], dtype=torch.float64, device=cdev)
        every = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(every, t)                         # every rank's own clock around its K steps
        rank_ms = [float(x.item()) / args.steps * 1e3 for x in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert toks.shape == (world * B * C_, args.new_tokens)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, {"tokens": toks})

    logits_spread = None
    if args.validate or grp:
        from taiwan_tongues_asr_ce_amd.dist import gather_logits
        eng.log_mel([synth.noise_clip(0)], want_output=False)        # the SAME clip on every rank
        eng.encode(1)
        eng.decode_reset(1)
        all_lg = gather_logits(eng.decode_step([st.sot]), device=local)
        logits_spread = float(np.abs(all_lg - all_lg[0:1]).max())
        # every rank loaded the same broadcast bits and no kernel uses float atomics: the spread is expected to be exactly 0
        if logits_spread > (2e-2 if args.compute != "f32" else 1e-4):
            raise SystemExit(f"validation failed: first-step logits differ across ranks by {logits_spread}")

    # The same K steps with the PCM already resident in HBM (the timed region minus the H2D copy of 61 MB per batch): a side
    # number on every rank's own clock, reported by rank 0 (max over ranks is not taken: it is not `value`)
    hbm_ms = None
    if rank == 0:
        local_pass(one_pass_hbm)
        ts = time.perf_counter()
        for _ in range(args.steps):
            local_pass(one_pass_hbm)
        hbm_ms = (time.perf_counter() - ts) / args.steps * 1e3

    # What ties the timed work to correct output (rank 0): (i) a replay of the step must be bit-identical (no float atomics);
    # (ii) the first choices of EVERY row of the last timed step are recomputed through a different route - the step API
    # hands raw logits to the host, the rules and the first-maximum argmax run in numpy, teacher-forced on the step's own
    # tokens - and must agree except within rounding distance of a tie; (iii) a CRC-32 of all B x new_tokens token ids against the value recorded for this
    # configuration in profiles/bench_tokens_crc.json (a tripwire for skipped work / changed arithmetic; rewritten with
    # --write-crc when a kernel change legitimately alters the last bits).  Logit-level parity of the same kernels
    # against the oracle is the job of tests/ (test_gpu_full_size.py at this geometry).
    check = None
    if rank == 0 and C_ == 1:
        import zlib
        n_chk = min(8, args.new_tokens)
        mine = np.asarray(toks[:B], dtype=np.int32)
        again = one_pass(eng)            # also restores this rank's resident state after the validation probe
        replay_equal = all(list(mine[b, :len(t)]) == list(t) for b, t in enumerate(again))
        n_cmp, n_agree, worst = _host_greedy_prefix(eng, B, prompt, mine, n_chk, [opts.suppress[i] for i in range(opts.n_suppress)],
                                                    [opts.begin_suppress[i] for i in range(opts.n_begin_suppress)], st.eot)
        crc = zlib.crc32(np.ascontiguousarray(mine).tobytes()) & 0xFFFFFFFF
        if args.dump_tokens:
            np.save(args.dump_tokens, np.ascontiguousarray(mine))
        key = f"{args.model}/b{B}/n{args.new_tokens}/{args.compute}" + ("+xkv_fp8" if args.xkv_fp8 else "")
        crc_path = os.path.join(ROOT, "profiles", "bench_tokens_crc.json")
        try:
            with open(crc_path) as f:
                known = json.load(f)
        except Exception:
            known = {}
        if args.write_crc:
            known[key] = crc
            with open(crc_path, "w") as f:
                json.dump(known, f, indent=1, sort_keys=True)
        # (iv) agreement with the f32 PARITY engine's tokens on this very workload (north_star: token-for-token at greedy decode):
        # profiles/bench_tokens_f32.npy is the [32][128] output of `bench.py --compute f32 --dump-tokens` (the f32 engine is the
        # one that meets the 1e-3 / token-exact gate against the oracle at this geometry, tests/test_gpu_full_size.py), with its
        # per-position top-2 margins beside it: see token_agreement().
        def agreement(ref_file):
            return token_agreement(mine, ref_file, args.model, args.clips)
        if args.dump_tokens:     # the reference engine's own margins (step API, teacher-forced on its own tokens)
            mg, ru = _step_api_margins(eng, B, prompt, mine, [opts.suppress[i] for i in range(opts.n_suppress)],
                                       [opts.begin_suppress[i] for i in range(opts.n_begin_suppress)], st.eot)
            stem = args.dump_tokens[:-4] if args.dump_tokens.endswith(".npy") else args.dump_tokens
            np.save(stem + "_margins.npy", mg)
            np.save(stem + "_runner_up.npy", ru)
        vs_f32 = agreement("bench_tokens_f32.npy")
        vs_bf16 = agreement("bench_tokens_bf16.npy") if (args.xkv_fp8 or args.compute != "bf16") else None
        tol = {"bf16": 0.05, "f16": 0.0125, "f32": 1e-3}[args.compute]
        check = {"replay_bit_identical": bool(replay_equal), "prefix_choices_recomputed_via_step_api": n_cmp,
                 "prefix_choices_equal": n_agree, "largest_margin_at_a_disagreement": round(worst, 5), "margin_tolerance": tol,
                 "tokens_crc32": crc, "expected_crc32": known.get(key), "crc_match": (known.get(key) == crc) if key in known else None,
                 "vs_f32_parity_tokens": vs_f32, "vs_bf16_engine_tokens": vs_bf16}
        if worst > tol or n_agree < 0.9 * n_cmp or not replay_equal:
            raise SystemExit(f"output check failed: {check}")
        # the recomputation moved the decode state: rebuild the step's state for the kernel measurements below
        one_pass(eng)

    if rank == 0:
        esz = 2 if args.compute != "f32" else 4
        # roofline of the dominant kernel: decoder cross-attention (HBM-bound), measured live with hipEvents
        # on the engine's own stream (ttasr_bench_kernel), state = the cross-KV left by the last step.
        k = eng.bench_kernel("xattn", B, iters=50)
        achieved = k["bytes"] / (k["ms"] * 1e-3) / 1e9
        # HBM traffic per launch from the PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, collected separately
        # and committed as profiles/xattn_pmc.json; gfx950 x2 FETCH_SIZE correction applied there)
        # ... and only when that profile describes the kernel THIS run launches: the library reports the signature of what
        # ttasr_bench_kernel launched (kernel name, template arguments, grid), the profile lists the signatures it was taken on;
        # a kernel change without a PMC refresh yields traffic = null plus the reason, never a stale number
        traffic, traffic_note = None, None
        try:
            with open(os.path.join(ROOT, "profiles", "xattn_pmc.json")) as f:
                traffic, traffic_note = xattn_traffic_from_profile(json.load(f), k.get("signature"), B)
        except Exception as ex:
            traffic_note = f"profiles/xattn_pmc.json unreadable: {ex}"
        roof = {"kernel": (k.get("signature") or "cross_attn_decode_kernel").split("<")[0], "kernel_signature": k.get("signature"),
                "bound": "hbm", "achieved": round(achieved, 1), "peak": 8000.0,
                "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "traffic": traffic,
                "traffic_source": traffic_note,
                "avg_launch_us": round(k["ms"] * 1e3, 2), "bytes_per_launch": k["bytes"]}
        # encoder GEMMs (the four shapes of one layer), flop-weighted: total flops / total time.
        # (i) IN SITU: one extra untimed pass of the real encoder schedule with a hipEvent after
        # every launch (option enc_kernel_timing, ttasr_encoder_kernel_ms) - each GEMM runs between its real neighbours, at the
        # clock the sustained phase holds.  This is `mfma.frac`.
        R_ = B * dims.n_audio_ctx
        d_, f_, T_ = dims.d_model, dims.ffn_dim, dims.n_audio_ctx
        cls_flops = {"qkv": 2.0 * R_ * 3 * d_ * d_ * dims.enc_layers, "out_proj": 2.0 * R_ * d_ * d_ * dims.enc_layers,
                     "fc1": 2.0 * R_ * d_ * f_ * dims.enc_layers, "fc2": 2.0 * R_ * d_ * f_ * dims.enc_layers,
                     "attention": 4.0 * B * T_ * T_ * d_ * dims.enc_layers,
                     "conv": B * (2.0 * 2 * T_ * d_ * 3 * dims.n_mels + 2.0 * T_ * d_ * 3 * d_),
                     "cross_kv": 2.0 * R_ * 2 * d_ * d_ * dims.dec_layers}
        eng.set_option("enc_kernel_timing", 1)
        eng.log_mel_device(pcm.data_ptr(), 480000, ns)
        eng.encode(B)
        eng.encode(B)                       # the second pass is the measured one (events already created)
        km = eng.encoder_kernel_ms()
        eng.set_option("enc_kernel_timing", 0)
        gemm_cls = ("qkv", "out_proj", "fc1", "fc2")
        insitu_tf = sum(cls_flops[k_] for k_ in gemm_cls) / (sum(km[k_] for k_ in gemm_cls) * 1e-3) / 1e12
        insitu = {k_: {"ms": round(km[k_], 3), "tflops": round(cls_flops[k_] / (km[k_] * 1e-3) / 1e12, 1) if k_ in cls_flops and km[k_] > 0 else None}
                  for k_ in km}
        # (ii) isolated relaunch loops of the same four kernels (round-2 figure, kept for comparison: 30 back-to-back launches
        # of ONE kernel right after a clock-recovery pass read higher than the sustained phase)
        names = ("enc_gemm_qkv", "enc_gemm_out", "enc_gemm_fc1", "enc_gemm_fc2")
        for n in names:
            eng.bench_kernel(n, B, iters=10)
        gs = [eng.bench_kernel(n, B, iters=30) for n in names]
        enc_tf = sum(x["flops"] for x in gs) / (sum(x["ms"] for x in gs) * 1e-3) / 1e12
        # matrix-pipe occupancy of the same four kernels from the committed PMC pass (clock-independent; static, like traffic)
        pmc_busy, pmc_file, pmc_note = None, None, None
        try:
            pmc_file = next(f_ for f_ in ("r6_pmc.json", "r5_pmc.json", "r4_pmc.json", "r3_pmc.json", "r2_pmc.json") if os.path.exists(os.path.join(ROOT, "profiles", f_)))
            with open(os.path.join(ROOT, "profiles", pmc_file)) as f:
                pmc_busy, pmc_note = pmc_busy_from_profile(json.load(f)["kernels"], [x.get("signature") for x in gs], [x["flops"] for x in gs])
        except Exception as ex:
            pmc_note = f"PMC profile unreadable: {ex}"
        ph = {kk: round(float(np.mean([p[kk] for p in phases])), 2) for kk in phases[0]}
        # phase-level fractions.  Decode: SURVEY.md 8(d)'s algorithmic bytes per step at the mean
        # position - decoder weights (every decoder-layer matrix + the tied embedding, read once per step for the whole batch)
        # + the cross-KV of every row + the self-KV read so far + the logits written - over the measured time per step.
        n_steps = len(prompt) + args.new_tokens - 1
        t_mean = (n_steps - 1) / 2.0
        dec_w = dims.dec_layers * (8 * d_ * d_ + 2 * d_ * f_) + dims.vocab * d_
        step_bytes = (dec_w * esz + B * dims.dec_layers * 2 * T_ * d_ * esz + B * dims.dec_layers * 2 * d_ * esz * t_mean
                      + B * dims.vocab * 4)
        ms_step = ph["decode"] / n_steps
        roof["decode_phase"] = {"bytes_per_step": round(step_bytes), "steps": n_steps, "ms_per_step": round(ms_step, 4),
                                "achieved_GBps": round(step_bytes / (ms_step * 1e-3) / 1e9, 1),
                                "frac_of_8TBps": round(step_bytes / (ms_step * 1e-3) / 8e12, 4),
                                "floor_ms_at_8TBps": round(step_bytes / 8e12 * 1e3, 4)}
        enc_phase_flops = sum(v for k_, v in cls_flops.items() if k_ != "cross_kv")
        out = {
            "metric": "audio-sec/s (RTF) whisper-large-v3 greedy, 30 s clips, batch 32; 1/2/4/8 GPU",
            "value": round(world * C_ * B * 30.0 * args.steps / dt, 2), "unit": "audio-s/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.compute + (" + fp8 (e4m3) cross-KV cache: opt-in serving mode, not the headline configuration" if args.xkv_fp8 else ""),
            "data": "synthetic",
            "config": {"workload": f"whisper-{args.model} geometry (random-init seeded weights), " + (f"{C_} concurrent contexts x " if C_ > 1 else "") + f"{B} x 30 s 16 kHz synthetic "
                                   f"clips per GPU in pinned host memory, H2D + log-mel + encoder + cross-KV + 4-token prompt + "
                                   f"{args.new_tokens} greedy tokens (EOT suppressed), {args.compute}",
                       "clips_per_gpu": B * C_, "contexts_per_gpu": C_, "new_tokens": args.new_tokens, "options": args.option or None,
                       "transport": transport,
                       "parallelism": f"dp{world}" + (f" x {C_} contexts" if C_ > 1 else "") +
                                      (" (ranks share GPUs over gloo: plumbing check, not a scaling number)"
                                       if world > torch.cuda.device_count() else ""),
                       "host_binding": (_dist_mod.HOST_BINDING or None) if world > 1 else None,
                       "rank_logits_spread": logits_spread,
                       "rank_ms_per_step": None if rank_ms is None else {"min": round(min(rank_ms), 2), "max": round(max(rank_ms), 2),
                                                                          "per_rank": [round(x, 2) for x in rank_ms]},
                       "phase_ms": ph, "median_ms_per_step": round(float(np.median(per_step)) * 1e3, 2),
                       "timed_region": "PCM f32 in pinned host memory -> token ids on the host (SURVEY.md 8(d)); H2D copy included",
                       "hbm_resident": {"ms_per_step": round(hbm_ms, 2), "steps": args.steps,
                                        "audio_s_per_s": round(C_ * B * 30.0 / (hbm_ms * 1e-3), 2),
                                        "note": "same steps with the PCM already in HBM (no H2D copy); side number, this rank's clock"},
                       "weight_load_s": round(t_load, 1)},
            "roofline": roof,
            "mfma": {"kernel": "encoder layer GEMMs (qkv, out-proj, fc1, fc2; flop-weighted), timed IN SITU: one pass of the real "
                               "encoder schedule with a hipEvent after every launch", "achieved_tflops": round(insitu_tf, 1),
                     "peak_tflops": 2500.0, "frac": round(insitu_tf / 2500.0, 4),
                     "in_situ_by_class": insitu,
                     "encoder_phase_frac": round(enc_phase_flops / (ph["encoder"] * 1e-3) / 2.5e15, 4),
                     "cross_kv_phase_frac": round(cls_flops["cross_kv"] / (ph["cross_kv"] * 1e-3) / 2.5e15, 4),
                     "isolated_relaunch_tflops": round(enc_tf, 1), "isolated_relaunch_frac": round(enc_tf / 2500.0, 4),
                     "pmc_mfma_busy_frac": pmc_busy,
                     "pmc_source": f"profiles/{pmc_file} (static; entries matched by kernel signature)" if pmc_busy is not None else pmc_note},
        }
        if world == 1 and C_ == 1 and args.clips == "noise":
            # SURVEY.md 8(d)'s tonal variant (five sines: exercises the per-clip max - 8 clamp of the log-mel): the same step on
            # the other clip set, a side number (the weights are random, so the content changes the front end, not the decode)
            for b in range(B):
                pcm[b] = torch.from_numpy(synth.tonal_clip(rank * B + b)).to(pcm.device)
            pcm_host.copy_(pcm)
            torch.cuda.synchronize()
            one_pass(eng)
            tt = []
            for _ in range(3):
                ts = time.perf_counter()
                one_pass(eng)
                tt.append(time.perf_counter() - ts)
            out["config"]["tonal_clips"] = {"ms_per_step": round(float(np.median(tt)) * 1e3, 2),
                                            "audio_s_per_s": round(B * 30.0 / float(np.median(tt)), 1), "steps": 3}
        if check is not None:
            out["output_check"] = check
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "dtype": "float64", "arrays": dumped}
        if world == 1 and C_ == 1 and (args.more_in_flight or not args.no_side):
            # Side modes, NEVER `value` (measured by the default run, under the driver's clock).  Each is
            # the same step (pinned host PCM -> tokens) for `--side-steps` timed passes after one warm-up:
            #   more_in_flight : a second independent bf16 context passes its own batch of B clips concurrently (2 x B clips in
            #                    flight; one context's latency-bound decode chain leaves most of the chip idle);
            #   xkv_fp8        : opt-in e4m3 copy of the cross-KV cache read by the decode step's cross-attention;
            #   f16            : the fp16 engine - the reference's own GPU type (asr_core.py:141, api/config.py:12) and the 16-bit
            #                    mode whose greedy tokens equal the f32 parity engine's on this workload.
            import threading
            side, n2 = {}, max(1, args.side_steps)
            for b in range(B):                                   # back to the headline clip set (the tonal side number changed it)
                pcm[b] = torch.from_numpy(make_clip(rank * B + b)).to(pcm.device)
            pcm_host.copy_(pcm)
            torch.cuda.synchronize()

            def timed(fn, clips_in_flight):
                fn()
                ts_ = time.perf_counter()
                for _ in range(n2):
                    last = fn()
                dt_ = (time.perf_counter() - ts_) / n2
                return last, {"value": round(clips_in_flight * 30.0 / dt_, 2), "unit": "audio-s/s", "ms_per_step": round(dt_ * 1e3, 2),
                              "steps": n2}

            def tok_array(rows):
                return np.asarray([list(t) + [0] * (args.new_tokens - len(t)) for t in rows], dtype=np.int32)
            if not args.no_side:
                # ragged: the headline workload with a token budget PER ROW (seeded, uniform 32 ... new_tokens; the longest row keeps
                # the full length) - what natural stopping looks like to the kernels ("with fixed N_dec and with natural
                # EOT"; synthetic weights emit no meaningful EOT, so the lengths are stated: ttasr_generate_capped).  Finished rows
                # leave the decode step's attention kernels (round 6); `static_batch` = the same budgets with option ragged_exit = 0,
                # i.e. the static batch of rounds 1-5 where every row streams its cross-KV until the last one ends.
                lo_ = min(32, args.new_tokens)
                caps = np.random.Generator(np.random.Philox(key=6)).integers(lo_, args.new_tokens + 1, size=B).astype(np.int32)
                caps[int(caps.argmax())] = args.new_tokens

                def ragged_pass():
                    eng.log_mel_host_ptr(pcm_host.data_ptr(), 480000, ns)
                    eng.encode(B)
                    return eng.generate([prompt] * B, opts, row_max_new=caps).tokens
                tr, m = timed(ragged_pass, B)
                ph_r = eng.phase_ms()
                eng.set_option("ragged_exit", 0)
                ts_, m_static = timed(ragged_pass, B)
                ph_s = eng.phase_ms()
                eng.set_option("ragged_exit", 1)
                L_, H_, T_ = dims.dec_layers, dims.n_heads, dims.n_audio_ctx
                per_row_step = L_ * H_ * 2 * T_ * 128                      # cross-KV bytes one live row streams per decode step (16-bit)
                waste = L_ * H_ * 256 * 3 * 16                             # a finished row still requests its first K batch (3 rows x 16 B per lane)
                steps_run = int(caps.max())
                streamed = float(caps.astype(np.int64).sum()) * per_row_step + float((steps_run - caps.astype(np.int64)).sum()) * waste
                m.update({
                    "row_budgets": {"min": int(caps.min()), "max": int(caps.max()), "mean": round(float(caps.mean()), 1), "seed": 6},
                    "tokens_generated": int(caps.sum()), "tokens_fixed_length": int(B * args.new_tokens),
                    "decode_ms": round(ph_r["decode"], 2), "decode_ms_fixed_length": round(statistics.median([p_["decode"] for p_ in phases]), 2),
                    "decode_ms_static_batch_same_budgets": round(ph_s["decode"], 2), "static_batch_audio_s_per_s": m_static["value"],
                    "decode_ratio_vs_fixed_length": round(ph_r["decode"] / statistics.median([p_["decode"] for p_ in phases]), 4),
                    "cross_kv_bytes_streamed": streamed, "cross_kv_bytes_static_batch": float(B) * steps_run * per_row_step,
                    "rows_equal_headline_prefix": int(sum(list(tr[r]) == [int(v_) for v_ in toks[r][:caps[r]]] for r in range(B))),
                    "rows_equal_static_batch": int(sum(list(tr[r]) == list(ts_[r]) for r in range(B))),
                    "note": "same 32 x 30 s of audio; a row is finished at its budget (ttasr_generate_capped) and leaves the attention "
                            "kernels; every row must equal the headline row cut at its budget (rows_equal_headline_prefix = B)"})
                side["ragged"] = m
            e2 = Engine(dims, compute, B, device=local)
            e2.load_weights(synth.iter_weights(dims))
            engines.append(e2)

            def both():
                th = [threading.Thread(target=one_pass, args=(e_,)) for e_ in (eng, e2)]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
            _, m = timed(both, 2 * B)
            m.update({"contexts_per_gpu": 2, "clips_in_flight_per_gpu": 2 * B, "dtype": args.compute,
                      "note": "opt-in serving configuration; the headline value is one context, one batch in flight"})
            side["more_in_flight"] = m
            out["more_in_flight"] = {"contexts_per_gpu": 2, "clips_in_flight_per_gpu": 2 * B, "steps": n2, "audio_s_per_s": m["value"],
                                     "note": "side measurement; the headline value above is one context, one batch in flight"}
            if not args.no_side and args.compute != "f32" and not args.xkv_fp8:
                e2.set_option("xkv_fp8", 1)
                t8, m = timed(lambda: one_pass(e2), B)
                t8 = tok_array(t8)
                m.update({"dtype": args.compute + " + e4m3 cross-KV cache", "phase_ms": {k_: round(v_, 2) for k_, v_ in e2.phase_ms().items()},
                          "vs_f32_parity_tokens": token_agreement(t8, "bench_tokens_f32.npy", args.model, args.clips),
                          "vs_headline_tokens_rows_identical": int((t8 == np.asarray(toks[:B], dtype=np.int32)).all(axis=1).sum()),
                          "note": "opt-in serving mode (ttasr_set_option xkv_fp8), never the headline"})
                side["xkv_fp8"] = m
            e2.close()
            engines.remove(e2)
            if not args.no_side and args.compute == "bf16" and not args.xkv_fp8:
                e3 = Engine(dims, COMPUTE_F16, B, device=local)
                e3.load_weights(synth.iter_weights(dims))
                engines.append(e3)
                t16, m = timed(lambda: one_pass(e3), B)
                t16 = tok_array(t16)
                import zlib
                m.update({"dtype": "f16", "phase_ms": {k_: round(v_, 2) for k_, v_ in e3.phase_ms().items()}, "tokens_crc32": zlib.crc32(np.ascontiguousarray(t16).tobytes()) & 0xFFFFFFFF,
                          "vs_f32_parity_tokens": token_agreement(t16, "bench_tokens_f32.npy", args.model, args.clips),
                          "note": "compute_type float16 = the reference's GPU setting (asr_core.py:141); same kernels templated on the storage type"})
                side["f16"] = m
                e3.close()
                engines.remove(e3)
            if not args.no_side and args.compute == "bf16" and not args.xkv_fp8 and args.model == "large-v3":
                # folder: the reference's folder tool (asr_core.py:151: one file at a time) on 48 synthetic recordings of 60 s, beam 5,
                # <= 64 tokens per 30-s window, through WhisperModel - groups of 24 files in lock step (120 decode rows: what the
                # folder tool's default context carries), ONE group at a time (pipeline_depth 1) against TWO groups in flight on two
                # engine contexts that share one copy of the weights (pipeline_depth 2: round 6).  Same groups -> identical results;
                # audio-s/s = 2 880 s of audio / wall time.  (12 files in groups of 6 - 30 rows - measured 595 -> 892: profiles/.)
                for e_ in list(engines):          # the model below builds its own contexts: release the bench engine's 20 GB first
                    e_.close()
                engines.clear()
                import warnings
                from taiwan_tongues_asr_ce_amd.model import WhisperModel
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    wm = WhisperModel(f"synthetic:{args.model}", device="cuda", device_index=local, compute_type="bfloat16", max_batch=120,
                                      pipeline_depth=2)
                    files = [np.concatenate([synth.tonal_clip(2 * i), synth.noise_clip(2 * i + 1)]) for i in range(48)]
                    groups = [files[:24], files[24:]]
                    kwf = dict(language="zh", beam_size=5, temperature=0.0, log_prob_threshold=None, max_new_tokens=64)
                    wm.transcribe_groups(groups, pipeline_depth=2, **kwf)             # warm-up: both lanes, graphs
                    res, wall = {}, {}
                    for depth in (1, 2, 1, 2):
                        ts_ = time.perf_counter()
                        r_ = wm.transcribe_groups(groups, pipeline_depth=depth, **kwf)
                        wall[depth] = min(wall.get(depth, 1e9), time.perf_counter() - ts_)
                        res[depth] = [[(sg.start, sg.end, tuple(sg.tokens)) for sg in segs] for g_ in r_ for segs, _ in g_]
                    side["folder"] = {
                        "workload": "48 x 60 s synthetic recordings, beam 5, <= 64 tokens per window, 24 files (120 decode rows) in lock step per group",
                        "serial_audio_s_per_s": round(2880.0 / wall[1], 1), "pipelined_audio_s_per_s": round(2880.0 / wall[2], 1),
                        "serial_s": round(wall[1], 3), "pipelined_s": round(wall[2], 3), "speed_up": round(wall[1] / wall[2], 3),
                        "results_identical": res[1] == res[2], "engine_contexts": len(wm._lanes),
                        "second_context_shares_weights": bool(wm._lanes[1].shares_weights),
                        "note": "WhisperModel(..., pipeline_depth=2).transcribe_groups / batch_cli --pipeline-depth 2 (ttasr_create_shared)"}
                    wm.close()
            out["side"] = side
        if world == 1 and not args.no_cpu_baseline:
            # cpu_baseline.value = ONE COMPLETE run of the CPU oracle on one clip of the workload, executed live on this box's host
            # cores (VERDICT round 4, next #2e); the per-layer extrapolation of earlier rounds is kept as `extrapolated_sample`
            full_path = os.path.join(ROOT, "profiles", "cpu_baseline_full.json")
            if args.model == "large-v3" or args.cpu_full:
                full = cpu_baseline_full(dims, args.new_tokens)
                out["cpu_baseline"] = full
                if args.cpu_full:
                    with open(full_path, "w") as f:
                        json.dump(full, f, indent=1)
                ext = cpu_baseline(dims, args.new_tokens)
                out["cpu_baseline"]["extrapolated_sample"] = {"value": ext["value"], "sample": ext["sample"]}
                try:   # an earlier complete run on another box's host (history)
                    with open(full_path) as f:
                        prev = json.load(f)
                    out["cpu_baseline"]["earlier_full_run"] = {k_: prev[k_] for k_ in ("value", "seconds", "cores", "cpu") if k_ in prev}
                except Exception:
                    pass
            else:
                out["cpu_baseline"] = cpu_baseline(dims, args.new_tokens)
            if args.model == "large-v3":   # the tiny / small rows of SURVEY.md 8(d), complete runs, bounded host time
                out["cpu_baseline"]["matrix"] = cpu_baseline_matrix(args.new_tokens, budget_s=25.0)
        if world > 1:   # a multi-rank line must say how the ranks talked and prove they hold the same weights
            assert transport is not None and logits_spread is not None and rank_ms is not None and len(rank_ms) == world, \
                (transport, logits_spread, rank_ms)
        line = json.dumps(out)
    for e_ in engines:
        e_.close()
    if grp:
        dist_barrier(local)
        dist.destroy_process_group()
    if rank == 0:
        # the result is the LAST line this process writes: RCCL prints its version banner through C stdio, which is block-buffered
        # on a pipe and would otherwise land after the result at exit
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
        print(line, flush=True)


if __name__ == "__main__":
    main()
