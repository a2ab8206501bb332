"""Speaker diarization on the device - where the time goes.  Micro geometry, float32, synthetic weights
(vad.synth_pyannet_weights, diarization.synth_xvector_weights): the networks are exercised, nobody is recognised.

  timing     one synthetic hour and 64 x 30 s (tools/vad_bench.py's bursts): the segmentation call, the mask step, the embedding
             call (Engine.speaker_embeddings, 3 masks per chunk) and the host clustering + reconstruction, each timed on its
             own: 1 warm-up, median / min / max of --repeats, and audio-s/s of the embedding call and of the whole pipeline.
  tdnn       the five TDNN blocks are 775.3 MMAC per chunk; their achieved TF/s against the 157 TF f32 peak comes from the
             kernel split of a trace (--kernel-stats), as does every kernel's share.
  host       the float32 torch restatement of the embedding network (front end, TDNN blocks, pooling of 3 masks, Linear) on 16
             host threads over one group of 16 chunks.
Nothing is asserted.  One JSON object on stdout and, with --out, in that file.  --hour-only: two embedding calls on the hour
and nothing else (the command a kernel trace is taken of; --kernel-stats FILE merges that trace's statistics CSV).

    python tools/diar_bench.py [--repeats 5] [--kernel-stats stats.csv] [--out profiles/diarization.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from taiwan_tongues_asr_ce_amd import _lib, diarization, synth, vad  # noqa: E402
from vad_bench import bursts, timed  # noqa: E402

TDNN_MAC = sum(f * cin * k * cout for f, (cin, cout, k, _) in zip((289, 285, 279, 279, 279), diarization.TDNN_BLOCKS))
F32_PEAK_TF = 157.0
ONSET = 0.35   # of the synthetic segmentation weights: about half of the frames are somebody's


def kernel_split(path: str, chunks: int) -> dict:
    """The spk_* and seg_* rows of a kernel trace's statistics CSV (Name, Calls, TotalDurationNs), and the TDNN blocks' TF/s."""
    import csv
    import re
    with open(path) as f:
        rows = [(re.search(r"(spk|seg)_\w+(<[^>]*>)?", r["Name"]), r) for r in csv.DictReader(f)]
    rows = [(m.group(0), r) for m, r in rows if m]
    total = sum(float(r["TotalDurationNs"]) for _, r in rows) or 1.0
    out = {name: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                  "share": round(float(r["TotalDurationNs"]) / total, 4)} for name, r in rows}
    tdnn_ns = sum(float(r["TotalDurationNs"]) for name, r in rows if name.startswith("spk_gemm_kernel<0") or name.startswith("spk_gemm_kernel<1"))
    if tdnn_ns:
        out["tdnn_blocks"] = {"chunks": chunks, "flop": 2.0 * TDNN_MAC * chunks, "total_ms": round(tdnn_ns / 1e6, 3),
                              "tf_per_s": round(2.0 * TDNN_MAC * chunks / tdnn_ns / 1e3, 2),
                              "of_f32_peak": round(2.0 * TDNN_MAC * chunks / tdnn_ns / 1e3 / F32_PEAK_TF, 4)}
    return out


def torch_restatement(weights, audio80000: np.ndarray, masks: np.ndarray, chunks: int, repeats: int) -> dict:
    """The embedding network in torch float32 operators on 16 threads: `chunks` chunks as one batch, 3 masks each."""
    import torch
    import torch.nn.functional as F
    torch.set_grad_enabled(False)
    torch.set_num_threads(16)
    w = {k: torch.from_numpy(v) for k, v in weights.items()}
    x0 = torch.from_numpy(np.tile(audio80000[None, None], (chunks, 1, 1)))
    m = torch.from_numpy(np.tile(masks[None], (chunks, 1, 1)))                  # [chunks, 3, 293]
    lrelu = lambda v: F.leaky_relu(v, 0.01)   # noqa: E731

    def run():
        x = F.instance_norm(x0, weight=w["sincnet.wav_norm1d.weight"], bias=w["sincnet.wav_norm1d.bias"], eps=1e-5)
        x = F.max_pool1d(torch.abs(F.conv1d(x, w["sincnet.conv1d.0.filters"], stride=10)), 3)
        x = lrelu(F.instance_norm(x, weight=w["sincnet.norm1d.0.weight"], bias=w["sincnet.norm1d.0.bias"], eps=1e-5))
        for i in (1, 2):
            x = F.max_pool1d(F.conv1d(x, w[f"sincnet.conv1d.{i}.weight"], w[f"sincnet.conv1d.{i}.bias"]), 3)
            x = lrelu(F.instance_norm(x, weight=w[f"sincnet.norm1d.{i}.weight"], bias=w[f"sincnet.norm1d.{i}.bias"], eps=1e-5))
        for l, (_, _, _, dil) in enumerate(diarization.TDNN_BLOCKS):
            x = lrelu(F.conv1d(x, w[f"tdnns.{3 * l}.weight"], w[f"tdnns.{3 * l}.bias"], dilation=dil))
            x = F.batch_norm(x, w[f"tdnns.{3 * l + 2}.running_mean"], w[f"tdnns.{3 * l + 2}.running_var"],
                             w[f"tdnns.{3 * l + 2}.weight"], w[f"tdnns.{3 * l + 2}.bias"], training=False, eps=1e-5)
        wr = F.interpolate(m, size=x.shape[2], mode="nearest")[:, :, None, :]   # [chunks, 3, 1, 279]
        v1, v2 = wr.sum(dim=3), (wr * wr).sum(dim=3)
        mean = (wr * x[:, None]).sum(dim=3) / v1
        var = (wr * (x[:, None] - mean[..., None]) ** 2).sum(dim=3) / (v1 - v2 / v1 + 1e-8)
        return F.linear(torch.cat([mean, torch.sqrt(var)], dim=2), w["embedding.weight"], w["embedding.bias"])

    t = timed(run, repeats, warm=1)
    t.update(chunks=chunks, threads=16, ms_per_chunk=round(1e3 * t["median_s"] / chunks, 3))
    return t


def bench(repeats: int, hour_only: bool, kernel_stats) -> dict:
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(PRESETS["micro"], COMPUTE_F32, 64)
    e.load_weights(synth.iter_weights(PRESETS["micro"]))
    e.load_segmentation(vad.synth_pyannet_weights(vad.SYNTH_PYANNET_SEED, 3))
    xw = diarization.synth_xvector_weights()
    e.load_speaker_embedding(xw)
    hour = bursts(1, 3600.0)
    res = {"tool": "tools/diar_bench.py", "weights": "vad.synth_pyannet_weights(), diarization.synth_xvector_weights()",
           "engine": "micro geometry, float32, max_batch 64", "group_chunks": _lib.SPK_GROUP, "masks_per_chunk": 3,
           "tdnn_mmac_per_chunk": round(TDNN_MAC / 1e6, 1), "onset": ONSET}
    if hour_only:
        probs = e.segmentation_scores([hour], return_chunks=True)[1]
        masks = [diarization.local_speaker_masks(probs[0], ONSET)]
        for _ in range(2):
            e.speaker_embeddings([hour], masks)
        e.close()
        return {"hour_only": True, "chunks": int(masks[0].shape[0])}
    res["timing"] = {}
    for name, audios in (("1 x 3600 s", [hour]), ("64 x 30 s", [bursts(100 + i, 30.0) for i in range(64)])):
        audio_s = sum(len(a) for a in audios) / 16000.0
        probs = e.segmentation_scores(audios, return_chunks=True)[1]
        masks = [diarization.local_speaker_masks(p, ONSET) for p in probs]
        emb = e.speaker_embeddings(audios, masks)
        row = {"audio_s": audio_s, "chunks": int(sum(len(p) for p in probs)),
               "masks_with_frames": int(sum((m.sum(axis=2) > 0).sum() for m in masks)),
               "segmentation": timed(lambda: e.segmentation_scores(audios, return_chunks=True), repeats, warm=1),
               "masks_host": timed(lambda: [diarization.local_speaker_masks(p, ONSET) for p in probs], repeats, warm=1),
               "embedding": timed(lambda: e.speaker_embeddings(audios, masks), repeats, warm=1)}
        t0 = time.perf_counter()
        turns = [diarization.diarize_from(p, x, m, len(a), onset=ONSET) for p, x, m, a in zip(probs, emb, masks, audios)]
        row["clustering_and_reconstruction_host"] = {"one_run_s": round(time.perf_counter() - t0, 4),
                                                     "speakers": [len({t.speaker for t in ts}) for ts in turns][:8]}
        total = (row["segmentation"]["median_s"] + row["masks_host"]["median_s"] + row["embedding"]["median_s"]
                 + row["clustering_and_reconstruction_host"]["one_run_s"])
        row["embedding_audio_s_per_s"] = round(audio_s / row["embedding"]["median_s"], 1)
        row["embedding_tdnn_tf_per_s_of_wall"] = round(2.0 * TDNN_MAC * row["chunks"] / row["embedding"]["median_s"] / 1e12, 2)
        row["pipeline_audio_s_per_s"] = round(audio_s / total, 1)
        res["timing"][name] = row
    chunk = bursts(7, 5.0)
    res["torch_float32_16_threads"] = torch_restatement(xw, chunk, diarization.local_speaker_masks(
        np.random.default_rng(0).uniform(0, 1, (1, 293, 3)), 0.5)[0], _lib.SPK_GROUP, min(repeats, 3))
    if kernel_stats:
        res["kernel_split_of_two_hour_calls"] = kernel_split(kernel_stats, 2 * res["timing"]["1 x 3600 s"]["chunks"])
    e.close()
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hour-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="a kernel trace's statistics CSV of --hour-only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    text = json.dumps(bench(args.repeats, args.hour_only, args.kernel_stats), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
