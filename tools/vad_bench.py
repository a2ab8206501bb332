"""Device VAD (Engine.vad_probs: the Silero-v5-shaped network of kernels_vad.hip) - throughput, what it replaces, its share of a
folder group, and its accuracy cases.  Synthetic weights (vad.synth_silero_weights), large-v3 geometry for the group.

  timing     Engine.vad_probs on 1, 24 and 120 recordings of 60 s and on one of 3600 s: wall time around the call (it ends in
             a stream synchronise and includes staging the host PCM), 2 warm-up calls, median / min / max of --repeats calls,
             and audio-s/s from the median.
  reference  the float32 numpy restatement (tests/vad_reference.py) driven frame by frame through vad.silero_speech_prob_fn on
             this host, on 60 s: the Python loop the device call replaces.
  share      WhisperModel.transcribe_many(24 recordings of 60 s, beam 5, <= 64 tokens per window, vad_filter=True) - the folder
             tool's default group - and the vad_probs call over the same 24 recordings inside it.
  accuracy   the cases of tests/test_gpu_vad.py: largest distance of the device's logits / probabilities from the float64
             reference and, beside it, of the float32 reference from float64.
Nothing is asserted.  One JSON object on stdout and, with --out, in that file.  --hour-only: three calls on the 3600-s recording
and nothing else (the command a kernel trace is taken of).

  --stream   the stateful streaming VAD instead (Engine.vad_stream_push), on the context a DeviceStreamVAD backend owns (micro
             geometry, max_batch 64): for 1, 64, 256 and 1024 open streams the wall time of ONE push of 24 000 samples (the
             server's 1.5-s chunk) per stream and of one push of 512 samples (one frame) per stream, and beside each the
             stateless alternative - Engine.vad_probs over the accumulated 3-s buffers of the same streams, what a server
             without streams runs at every chunk.  2 warm-ups, median / min / max of --repeats.  Records, not gates.

  --stream --wire ulaw8k|s16x2_8k|s16_48k   wire streams (Engine.vad_stream_push_wire): one push of 64 streams x 1.5-s pieces in
             that wire format, in ms per push, beside the same pieces converted and resampled on the host and then pushed as
             16 kHz floats, and beside the file kernel run per row (Engine.ingest) and then pushed.  --trace-pushes N: N wire
             pushes and nothing else (the command a kernel trace counts launches of).

  --pyannote   the PyanNet-shaped segmentation network instead (Engine.segmentation_scores, kernels_seg.hip), micro geometry,
             float32, max_batch 64, synthetic weights: audio-s/s on one synthetic hour and on 64 x 30 s; every recurrence form
             (option seg_lstm_rows = 1, 2, 4 chunks per workgroup) on recordings of 1, 8, 64 and 7 000 chunks; the latency of
             DevicePyannoteVAD.detect_activity for 1, 8 and 64 concurrent clients with 3-s buffers; and beside them the float32
             torch restatement of the network on 16 host threads over one group of 64 chunks.  --kernel-stats FILE merges the
             per-kernel split of a kernel trace's statistics CSV (taken of --pyannote --hour-only: three calls on the hour).

    python tools/vad_bench.py --pyannote [--repeats 5] [--kernel-stats stats.csv] [--out profiles/pyannote_vad.json]
    python tools/vad_bench.py [--model large-v3] [--repeats 7] [--out profiles/vad_device.json]
    python tools/vad_bench.py --stream [--repeats 7] [--out profiles/vad_stream.json]
    python tools/vad_bench.py --stream --wire ulaw8k [--repeats 7] [--out profiles/wire_stream.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from taiwan_tongues_asr_ce_amd import vad  # noqa: E402

HEADLINE = 2150.0   # audio-s/s of the engine's headline workload (README.md)


def bursts(seed: int, total_s: float) -> np.ndarray:
    """Noise bursts of 1-3 s between digital silences of 2.5-4 s (the shape of the suite's test signal), cut to total_s."""
    rng = np.random.default_rng([0xBE7C4, seed])
    parts, n = [], 0
    while n < total_s * 16000:
        gap, burst = int(rng.uniform(2.5, 4.0) * 16000), int(rng.uniform(1.0, 3.0) * 16000)
        parts += [np.zeros(gap, np.float32), (rng.standard_normal(burst) * rng.uniform(0.08, 0.25)).astype(np.float32)]
        n += gap + burst
    return np.concatenate(parts)[: int(total_s * 16000)]


def timed(fn, repeats: int, warm: int = 2):
    for _ in range(warm):
        fn()
    xs = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t)
    return {"median_s": round(statistics.median(xs), 5), "min_s": round(min(xs), 5), "max_s": round(max(xs), 5), "runs": len(xs)}


def accuracy(engine) -> dict:
    import test_gpu_vad as T
    from vad_reference import cached_probs, test_signal
    sig, long = test_signal(), T._long()
    C = T.CHUNK
    cases = {"n=1 short lengths": [([T._noise(n, n)], [("noise", n)]) for n in T.LENGTHS],
             "n=5 mixed": [([T._noise(n, n) for n in lens], [("noise", n) for n in lens]) for lens in T.MIXED],
             "40-s test signal": [([sig], ["signal"])],
             "chunk boundary": [([long[:n] for n in (512 * C - 1, 512 * C, 512 * C + 1, 512 * (2 * C + 3))],
                                 [("long", n) for n in (512 * C - 1, 512 * C, 512 * C + 1, 512 * (2 * C + 3))])]}
    out = {}
    for name, calls in cases.items():
        w = dict(device_logit=0.0, device_prob=0.0, float32_ref_logit=0.0, float32_ref_prob=0.0)
        for audios, keys in calls:
            p, l = engine.vad_probs(audios, return_logits=True)
            for a, k, pi, li in zip(audios, keys, p, l):
                p64, l64 = cached_probs(T.SEED, k, a)
                p32, l32 = cached_probs(T.SEED, k, a, np.float32)
                w["device_logit"] = max(w["device_logit"], float(np.abs(li - l64).max()))
                w["device_prob"] = max(w["device_prob"], float(np.abs(pi - p64).max()))
                w["float32_ref_logit"] = max(w["float32_ref_logit"], float(np.abs(l32 - l64).max()))
                w["float32_ref_prob"] = max(w["float32_ref_prob"], float(np.abs(p32 - p64).max()))
        out[name] = {k: float(f"{v:.3e}") for k, v in w.items()}
    return out


def stream_bench(repeats: int) -> dict:
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(PRESETS["micro"], COMPUTE_F32, 64)
    e.load_vad(vad.synth_silero_weights())
    res = {"tool": "tools/vad_bench.py --stream", "weights": "vad.synth_silero_weights()", "engine": "micro geometry, float32, max_batch 64",
           "chunk_samples": 24000, "frame_samples": 512, "stateless_buffer_samples": 48000, "streams": {}}
    base = bursts(2000, 40.0)
    for n in (1, 64, 256, 1024):
        buffers = [np.ascontiguousarray(base[(997 * i) % (len(base) - 48000):][:48000]) for i in range(n)]
        chunks = [b[24000:] for b in buffers]
        frames = [b[:512] for b in buffers]
        ids = [e.vad_stream_open() for _ in range(n)]
        e.vad_stream_push(ids, [b[:24000] for b in buffers])          # the streams hold the first half of their buffers
        row = {"push_24000": timed(lambda: e.vad_stream_push(ids, chunks), repeats),
               "push_512": timed(lambda: e.vad_stream_push(ids, frames), repeats),
               "stateless_vad_probs_48000": timed(lambda: e.vad_probs(buffers), repeats)}
        row["push_24000"]["frames_per_stream"] = 46.875
        row["push_24000"]["x_faster_than_stateless"] = round(row["stateless_vad_probs_48000"]["median_s"] / row["push_24000"]["median_s"], 2)
        row["push_512"]["x_faster_than_stateless"] = round(row["stateless_vad_probs_48000"]["median_s"] / row["push_512"]["median_s"], 2)
        row["push_24000"]["us_per_stream"] = round(1e6 * row["push_24000"]["median_s"] / n, 1)
        row["push_512"]["us_per_stream"] = round(1e6 * row["push_512"]["median_s"] / n, 1)
        res["streams"][str(n)] = row
        for i in ids:
            e.vad_stream_close(i)
    e.close()
    return res


WIRES = {"ulaw8k": dict(rate=8000, channels=1, encoding="ulaw"), "s16x2_8k": dict(rate=8000, channels=2, encoding="s16"),
         "s16_48k": dict(rate=48000, channels=1, encoding="s16")}


def wire_pieces(fmt, n: int, seconds: float):
    """n pieces of `seconds` in the wire format, cut from the burst signal resampled by plain interpolation (a bench input)."""
    base = bursts(3000, 40.0)
    frames = int(seconds * fmt.rate)
    out = []
    for i in range(n):
        at = (997 * i) % (len(base) - int(seconds * 16000) - 1)
        x = np.interp(np.arange(frames) * (16000.0 / fmt.rate), np.arange(int(seconds * 16000) + 1), base[at:at + int(seconds * 16000) + 1])
        s16 = np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)
        if fmt.encoding == "ulaw":   # G.711 mu-law encoder (bench input only): sign, segment of the biased magnitude, four mantissa bits
            mag = np.minimum(np.abs(s16.astype(np.int32)), 32635) + 0x84
            seg = np.floor(np.log2(mag)).astype(np.int32) - 7
            raw = (~(np.where(s16 < 0, 0x80, 0) | (seg << 4) | ((mag >> (seg + 3)) & 15)) & 0xFF).astype(np.uint8).tobytes()
        else:
            raw = np.repeat(s16[:, None], fmt.channels, axis=1).astype("<i2").tobytes()
        out.append(raw)
    return out


def wire_bench(repeats: int, wire: str, n: int = 64, seconds: float = 1.5, trace_pushes: int = 0) -> dict:
    """--stream --wire: ONE Engine.vad_stream_push_wire of n streams x 1.5-s pieces, and beside it the two ways without it - the
    pieces converted and resampled on the host (vad.WireFormat.to_16k: scipy's resample_poly per piece, which is NOT cut-invariant:
    every piece gets edge transients) and then Engine.vad_stream_push, and the pieces through Engine.ingest (the file kernel: one
    launch per row, not cut-invariant either) and then Engine.vad_stream_push."""
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    fmt = vad.WireFormat(**WIRES[wire])
    e = Engine(PRESETS["micro"], COMPUTE_F32, 64)
    e.load_vad(vad.synth_silero_weights())
    pieces = wire_pieces(fmt, n, seconds)
    wids = [e.vad_stream_open(wire=fmt) for _ in range(n)]
    fids = [e.vad_stream_open() for _ in range(n)]
    if trace_pushes:
        for _ in range(trace_pushes):
            e.vad_stream_push_wire(wids, pieces)
        e.close()
        return {"wire_pushes": trace_pushes, "rows": n}
    rate, ch, code, pick = fmt.wire_args()

    def host_path():
        e.vad_stream_push(fids, [fmt.to_16k(p) for p in pieces])

    def per_row_path():
        e.vad_stream_push(fids, e.ingest(pieces, [rate] * n, [ch] * n, [code] * n, picks=[pick] * n))

    res = {"tool": f"tools/vad_bench.py --stream --wire {wire}", "weights": "vad.synth_silero_weights()",
           "engine": "micro geometry, float32, max_batch 64", "wire": WIRES[wire], "streams": n, "piece_seconds": seconds,
           "piece_bytes": len(pieces[0]),
           "push_wire": timed(lambda: e.vad_stream_push_wire(wids, pieces), repeats),
           "host_convert_resample_then_push": timed(host_path, repeats),
           "per_row_ingest_kernel_then_push": timed(per_row_path, repeats),
           "vad_stream_push_of_16k_float_alone": None,
           "note": "the two alternatives resample every piece on its own: their results carry edge transients at every cut"}
    ready = [fmt.to_16k(p) for p in pieces]
    res["vad_stream_push_of_16k_float_alone"] = timed(lambda: e.vad_stream_push(fids, ready), repeats)
    for k in ("push_wire", "host_convert_resample_then_push", "per_row_ingest_kernel_then_push", "vad_stream_push_of_16k_float_alone"):
        res[k]["ms_per_push"] = round(1e3 * res[k]["median_s"], 3)
    e.close()
    return res


def torch_pyannet_float32(weights, threads: int = 16):
    """The float32 torch restatement of the network: fn(x [chunks, 80000]) -> probabilities [chunks, 293, C] on `threads` host threads."""
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(threads)
    w = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in weights.items()}
    lstm = torch.nn.LSTM(60, 128, num_layers=4, bidirectional=True, batch_first=True)
    lstm.load_state_dict({k[5:]: v for k, v in w.items() if k.startswith("lstm.")})

    def fn(x):
        with torch.no_grad():
            y = torch.from_numpy(x)[:, None, :]
            y = F.instance_norm(y, weight=w["sincnet.wav_norm1d.weight"], bias=w["sincnet.wav_norm1d.bias"], eps=1e-5)
            y = torch.abs(F.conv1d(y, w["sincnet.conv1d.0.filters"], stride=10))
            for i in range(3):
                if i:
                    y = F.conv1d(y, w[f"sincnet.conv1d.{i}.weight"], w[f"sincnet.conv1d.{i}.bias"])
                y = F.leaky_relu(F.instance_norm(F.max_pool1d(y, 3, 3), weight=w[f"sincnet.norm1d.{i}.weight"],
                                                 bias=w[f"sincnet.norm1d.{i}.bias"], eps=1e-5))
            y = lstm(y.transpose(1, 2))[0]
            for i in range(2):
                y = F.leaky_relu(F.linear(y, w[f"linear.{i}.weight"], w[f"linear.{i}.bias"]))
            return torch.sigmoid(F.linear(y, w["classifier.weight"], w["classifier.bias"])).numpy()
    return fn


def kernel_split(path: str) -> dict:
    """The seg_* rows of a kernel trace's statistics CSV (Name, Calls, TotalDurationNs): calls, total ms and share per kernel."""
    import csv
    import re
    with open(path) as f:
        rows = [(re.search(r"seg_\w+(<[^>]*>)?", r["Name"]), r) for r in csv.DictReader(f)]
    rows = [(m.group(0), r) for m, r in rows if m]
    total = sum(float(r["TotalDurationNs"]) for _, r in rows) or 1.0
    return {name: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                   "share": round(float(r["TotalDurationNs"]) / total, 4)} for name, r in rows}


def pyannote_bench(repeats: int, hour_only: bool, kernel_stats) -> dict:
    import asyncio

    from taiwan_tongues_asr_ce_amd import _lib, vad_backends
    from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
    from taiwan_tongues_asr_ce_amd.engine import Engine
    weights = vad.synth_pyannet_weights()
    e = Engine(PRESETS["micro"], COMPUTE_F32, 64)
    e.load_segmentation(weights)
    hour = bursts(3000, 3600.0)
    if hour_only:
        for _ in range(3):
            e.segmentation_scores([hour])
        return {"hour_only_calls": 3, "chunks_per_call": int(e.lib.ttasr_seg_chunks(len(hour)))}
    res = {"tool": "tools/vad_bench.py --pyannote", "weights": "vad.synth_pyannet_weights()", "engine": "micro geometry, float32, max_batch 64",
           "group_chunks": _lib.SEG_GROUP, "timing": {}, "recurrence_forms": {}, "detect_activity_3s_buffers": {}}
    clips = [bursts(3100 + i, 30.0) for i in range(64)]
    for name, audios in (("1 x 3600 s", [hour]), ("64 x 30 s", clips)):
        t = timed(lambda: e.segmentation_scores(audios), repeats)
        secs = sum(len(a) for a in audios) / 16000.0
        t.update(audio_s=secs, chunks=int(sum(e.lib.ttasr_seg_chunks(len(a)) for a in audios)), audio_s_per_s=round(secs / t["median_s"], 1))
        res["timing"][name] = t
    for chunks in (1, 8, 64, 7000):
        x = hour[:80000 + 8000 * (chunks - 1)]
        row = {}
        for rows in (1, 2, 4):
            e.set_option("seg_lstm_rows", rows)
            t = timed(lambda: e.segmentation_scores([x]), repeats)
            row[f"rows_{rows}"] = dict(t, ms_per_chunk=round(1e3 * t["median_s"] / chunks, 4))
        e.set_option("seg_lstm_rows", 0)
        row["fastest"] = min(("rows_1", "rows_2", "rows_4"), key=lambda k: row[k]["median_s"])
        res["recurrence_forms"][str(chunks)] = row

    class Client:
        sampling_rate, samples_width = 16000, 2

        def __init__(self, cid, audio):
            self.client_id, self.scratch_buffer = cid, bytearray((np.clip(audio, -1, 1) * 32767).astype("<i2").tobytes())

    for n in (1, 8, 64):
        backend = vad_backends.DevicePyannoteVAD(engine=e, max_wait_ms=2.0)
        clients = [Client(i, hour[(99991 * i) % (len(hour) - 48000):][:48000]) for i in range(n)]

        async def once():
            return await asyncio.gather(*[backend.detect_activity(c) for c in clients])

        loop = asyncio.new_event_loop()
        t = timed(lambda: loop.run_until_complete(once()), repeats)
        t["device_calls"] = sorted(set(backend.calls_run))
        t["ms_per_client"] = round(1e3 * t["median_s"] / n, 3)
        res["detect_activity_3s_buffers"][str(n)] = t
        backend.close()
        loop.close()
    fn = torch_pyannet_float32(weights, 16)
    group = np.stack([hour[8000 * k:8000 * k + 80000] for k in range(64)])
    t = timed(lambda: fn(group), 3, warm=1)
    t.update(chunks=64, host_threads=16, ms_per_chunk=round(1e3 * t["median_s"] / 64, 3), audio_s_per_s_of_a_long_recording=round(64 * 0.5 / t["median_s"], 1))
    res["torch_float32_restatement_64_chunks"] = t
    got = e.segmentation_scores([hour[:80000 + 8000 * 63]], return_chunks=True)[1][0]
    res["device_vs_torch_float32_max_abs_probability"] = float(f"{np.abs(got - fn(group)).max():.3e}")
    if kernel_stats:
        res["kernel_split_of_three_hour_calls"] = kernel_split(kernel_stats)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--compute", default="bfloat16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hour-only", action="store_true")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--wire", choices=sorted(WIRES), default=None, help="with --stream: wire streams in this format")
    ap.add_argument("--trace-pushes", type=int, default=0, help="with --stream --wire: this many pushes and nothing else (the command a kernel trace is taken of)")
    ap.add_argument("--pyannote", action="store_true", help="the segmentation network (Engine.segmentation_scores)")
    ap.add_argument("--kernel-stats", default=None, help="with --pyannote: a kernel trace's statistics CSV of --pyannote --hour-only")
    args = ap.parse_args()
    if args.pyannote:
        text = json.dumps(pyannote_bench(args.repeats, args.hour_only, args.kernel_stats), indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.stream:
        res = wire_bench(args.repeats, args.wire, trace_pushes=args.trace_pushes) if args.wire else stream_bench(args.repeats)
        text = json.dumps(res, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    warnings.simplefilter("ignore")
    weights = vad.synth_silero_weights()
    hour = bursts(1000, 3600.0)
    if args.hour_only:
        from taiwan_tongues_asr_ce_amd.config import COMPUTE_F32, PRESETS
        from taiwan_tongues_asr_ce_amd.engine import Engine
        e = Engine(PRESETS["micro"], COMPUTE_F32, 1)
        e.load_vad(weights)
        for _ in range(3):
            e.vad_probs([hour])
        print(json.dumps({"hour_only_calls": 3, "frames_per_call": -(-len(hour) // 512)}))
        return
    m = WhisperModel(f"synthetic:{args.model}", device="cuda", compute_type=args.compute, max_batch=120, vad_model=weights)
    eng = m.engine
    files = [bursts(i, 60.0) for i in range(120)]
    res = {"tool": "tools/vad_bench.py", "model": args.model, "compute_type": args.compute, "weights": "vad.synth_silero_weights()",
           "chunk_frames": 1024, "timing": {}}
    for name, audios in (("1 x 60 s", files[:1]), ("24 x 60 s", files[:24]), ("120 x 60 s", files), ("1 x 3600 s", [hour])):
        t = timed(lambda: eng.vad_probs(audios), args.repeats)
        secs = sum(len(a) for a in audios) / 16000.0
        t["audio_s"] = secs
        t["audio_s_per_s"] = round(secs / t["median_s"], 1)
        t["x_headline_2150"] = round(t["audio_s_per_s"] / HEADLINE, 1)
        res["timing"][name] = t
    from vad_reference import SileroRef
    ref = SileroRef(weights, np.float32)
    fn = vad.silero_speech_prob_fn(lambda frame, state: ref.step(frame, state))
    t = timed(lambda: fn(files[0]), 3, warm=1)
    t["audio_s_per_s"] = round(60.0 / t["median_s"], 1)
    res["reference_float32_numpy_frame_by_frame_60s"] = t
    kw = dict(language="zh", beam_size=5, temperature=0.0, log_prob_threshold=None, max_new_tokens=64)
    group = files[:24]
    m.transcribe_many(group, vad_filter=True, **kw)                     # warm-up: graphs, scratch
    t_many = timed(lambda: m.transcribe_many(group, vad_filter=True, **kw), 3, warm=0)
    t_plain = timed(lambda: m.transcribe_many(group, **kw), 3, warm=1)
    t_vad = res["timing"]["24 x 60 s"]["median_s"]
    kept = sum(info.duration_after_vad for _, info in m.transcribe_many(group, vad_filter=True, **kw)) / (24 * 60.0)
    res["share_of_a_24_file_group"] = {
        "transcribe_many_vad_filter_s": t_many, "vad_probs_s": t_vad, "vad_share": round(t_vad / t_many["median_s"], 4),
        "transcribe_many_without_vad_s": t_plain, "audio_kept_by_vad": round(kept, 3),
        "group_audio_s_per_s_with_vad": round(24 * 60.0 / t_many["median_s"], 1),
        "group_audio_s_per_s_without_vad": round(24 * 60.0 / t_plain["median_s"], 1)}
    res["accuracy_vs_float64"] = accuracy(eng)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    m.close()


if __name__ == "__main__":
    main()
