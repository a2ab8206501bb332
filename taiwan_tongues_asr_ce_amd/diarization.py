"""Speaker diarization on top of the two device networks: the PyanNet-shaped segmentation network gives, per 5-s chunk, the
activity of up to C local speakers (Engine.segmentation_scores(return_chunks=True)); the XVectorSincNet-shaped network gives
one embedding per (chunk, local speaker) (Engine.speaker_embeddings); everything between and behind them is here, on the
host, in numpy and scipy: the masks, the clustering, the reconstruction of "who spoke when", the speaker of a segment or word,
and the SRT writer of the speaker-labelled subtitle.

UNPINNED against pyannote.audio and the published pyannote/embedding checkpoint: neither exists offline, so the tensor names
and shapes (XVECTOR_TENSORS), the pooling and the pipeline's rules are restated from memory, and the device network is held
to the float64 restatement of tests/xvector_reference.py on synthetic weights (include/ttasr.h ttasr_spk_*)."""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import vad

FRAMES, POOL_FRAMES, STATS = vad.PYANNET_FRAMES, 279, 3000
MAX_MASKS, MAX_DIM = 8, 512
# block: (cin, cout, kernel, dilation); the state-dict index of block l's Conv1d is 3 l, of its BatchNorm1d 3 l + 2
TDNN_BLOCKS = ((60, 512, 5, 1), (512, 512, 3, 2), (512, 512, 3, 3), (512, 512, 1, 1), (512, 1500, 1, 1))


def _xvector_table() -> Dict[str, tuple]:
    t: Dict[str, tuple] = {k: v for k, v in vad.PYANNET_TENSORS.items() if k.startswith("sincnet.")}
    for l, (cin, cout, k, _) in enumerate(TDNN_BLOCKS):
        t[f"tdnns.{3 * l}.weight"], t[f"tdnns.{3 * l}.bias"] = (cout, cin, k), (cout,)
        for part in ("weight", "bias", "running_mean", "running_var"):
            t[f"tdnns.{3 * l + 2}.{part}"] = (cout,)
    t["embedding.weight"], t["embedding.bias"] = ("D", STATS), ("D",)
    return t


XVECTOR_TENSORS: Dict[str, tuple] = _xvector_table()   # 45 tensors; "D" = the embedding's dimension, 1 ... 512
SYNTH_XVECTOR_SEED = 0


def synth_xvector_weights(seed: int = SYNTH_XVECTOR_SEED, dim: int = 192) -> Dict[str, np.ndarray]:
    """Seeded synthetic weights in the shapes of XVECTOR_TENSORS (float32): the filters are sinc_filters of the mel-spaced
    initial cutoffs, every matrix is drawn N(0, 1 / sqrt(fan_in)) so that activations stay O(1) through the five blocks, the
    BatchNorms' running means are drawn around 0.2 and their running variances in [0.5, 1.5] (never 0 and 1: an error in the
    normalisation shows), the other vectors are small.  Deterministic per (seed, dim).  NOT a speaker model: a stand-in that
    exercises the network."""
    if not 1 <= int(dim) <= MAX_DIM:
        raise ValueError(f"dim {dim} outside 1 ... {MAX_DIM}")
    rng = np.random.default_rng([0x5BEA4E7, int(seed)])
    out: Dict[str, np.ndarray] = {}
    for name, shape in XVECTOR_TENSORS.items():
        shape = tuple(int(dim) if d == "D" else d for d in shape)
        if name == "sincnet.conv1d.0.filters":
            w = vad.sinc_filters(*vad.mel_cutoffs())
        elif name.endswith("running_mean"):
            w = 0.2 + 0.3 * rng.standard_normal(shape)
        elif name.endswith("running_var"):
            w = rng.uniform(0.5, 1.5, shape)
        elif "norm1d" in name or (name.startswith("tdnns.") and len(shape) == 1 and int(name.split(".")[1]) % 3 == 2):
            w = (1.0 + 0.1 * rng.standard_normal(shape)) if name.endswith("weight") else 0.1 * rng.standard_normal(shape)
        elif name.endswith("weight"):
            w = rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
        else:
            w = rng.standard_normal(shape) * 0.05
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def load_xvector_state(path_or_mapping) -> Dict[str, np.ndarray]:
    """The tensors of XVECTOR_TENSORS as float32 arrays, from a mapping (state dict; torch tensors or arrays), an `.npz` file, or
    - when torch imports - a torch file, with an optional "state_dict" level (a Lightning checkpoint).  The filters come from
    "sincnet.conv1d.0.filters" when the source has it, else from the cutoffs vad.PYANNET_CUTOFFS through vad.sinc_filters.  Keys
    outside the table (num_batches_tracked among them) are ignored; a missing tensor or a wrong shape raises ValueError."""
    src = path_or_mapping
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        path = os.fspath(src)
        if str(path).lower().endswith(".npz"):
            with np.load(path) as z:
                src = {k: z[k] for k in z.files}
        else:
            try:
                import torch
            except ImportError as e:
                raise RuntimeError(f"{path}: reading a torch checkpoint needs torch; convert it to .npz") from e
            src = torch.load(path, map_location="cpu", weights_only=True)
    src = dict(src)
    if "state_dict" in src and hasattr(src["state_dict"], "items"):
        src = dict(src["state_dict"])
    to_np = lambda v: np.asarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else v)   # noqa: E731
    out: Dict[str, np.ndarray] = {}
    if "sincnet.conv1d.0.filters" not in src and all(k in src for k in vad.PYANNET_CUTOFFS):
        out["sincnet.conv1d.0.filters"] = vad.sinc_filters(*(to_np(src[k]) for k in vad.PYANNET_CUTOFFS))
    dim = None
    for name, shape in XVECTOR_TENSORS.items():
        if name not in src:
            continue
        a = np.ascontiguousarray(to_np(src[name]), dtype=np.float32)
        if "D" in shape:
            if a.ndim != len(shape) or not 1 <= a.shape[0] <= MAX_DIM or (dim is not None and a.shape[0] != dim):
                raise ValueError(f"speaker-embedding tensor {name}: shape {a.shape}, expected {shape} with one D in 1 ... {MAX_DIM}")
            dim = a.shape[0]
            shape = tuple(dim if d == "D" else d for d in shape)
        if a.shape != shape:
            raise ValueError(f"speaker-embedding tensor {name}: shape {a.shape}, expected {shape}")
        out[name] = a
    missing = [n for n in XVECTOR_TENSORS if n not in out]
    if missing:
        raise ValueError(f"speaker-embedding state is missing {missing}")
    return {n: out[n] for n in XVECTOR_TENSORS}


# ---- masks ---------------------------------------------------------------------------------------------------------------

def local_speaker_masks(chunk_probs, onset: float = 0.5, exclude_overlap: bool = True, min_frames: int = 10) -> np.ndarray:
    """chunk_probs [K, 293, C] -> float32 [K, C, 293] binary frame weights, one mask per local speaker: 1 on the frames where its
    probability is >= onset.  exclude_overlap: the frames where two or more speakers are active are removed; a speaker that
    keeps fewer than min_frames frames that way gets its overlapped frames back (its whole activity)."""
    p = np.asarray(chunk_probs)
    if p.ndim != 3 or p.shape[1] != FRAMES:
        raise ValueError(f"chunk probabilities of shape {p.shape}, expected (K, {FRAMES}, C)")
    active = p >= onset                                            # [K, 293, C]
    masks = active
    if exclude_overlap:
        clean = active & (active.sum(axis=2, keepdims=True) < 2)
        few = clean.sum(axis=1, keepdims=True) < int(min_frames)   # [K, 1, C]
        masks = np.where(few, active, clean)
    return np.ascontiguousarray(masks.transpose(0, 2, 1), dtype=np.float32)


# ---- clustering ----------------------------------------------------------------------------------------------------------

def cluster_embeddings(emb, valid, threshold: float, num_speakers: Optional[int] = None, min_cluster_size: int = 2,
                       max_train: int = 2000) -> Tuple[np.ndarray, np.ndarray]:
    """emb [..., D] embeddings and valid [...] = the clean frames behind each (0: not to be used) -> (labels [...] int64, -1 for
    the rows that are skipped, centroids [n_clusters, D] of unit vectors' means).  Rows with a NaN or with valid <= 0 are
    skipped.  The others are unit-normalised; the at most max_train of them with the most clean frames (ties: the earlier row)
    are clustered by centroid-linkage agglomerative clustering (scipy.cluster.hierarchy.linkage(method="centroid")) and the
    tree is cut at distance `threshold` - or, with num_speakers, into that many clusters (fewer when there are fewer rows).
    Without num_speakers, clusters of fewer than min_cluster_size rows are folded into the nearest cluster of at least that
    size (cosine distance between centroids; when no cluster is that large, the largest one - the earliest of them - is the
    only one kept).  Clusters are numbered in the order of their first training row.  Every usable row is then given the
    cluster of the nearest centroid by cosine distance (ties: the lower number).  Deterministic: no random state anywhere."""
    from scipy.cluster.hierarchy import fcluster, linkage
    e = np.asarray(emb, dtype=np.float64)
    lead = e.shape[:-1]
    e = e.reshape(-1, e.shape[-1])
    v = np.asarray(valid, dtype=np.float64).reshape(-1)
    if v.shape[0] != e.shape[0]:
        raise ValueError(f"{e.shape[0]} embeddings and {v.shape[0]} validity entries")
    norm = np.sqrt((e * e).sum(axis=1))
    usable = np.isfinite(e).all(axis=1) & (v > 0) & (norm > 0)
    labels = np.full(e.shape[0], -1, dtype=np.int64)
    idx = np.flatnonzero(usable)
    if len(idx) == 0:
        return labels.reshape(lead), np.zeros((0, e.shape[1]))
    unit = e[idx] / norm[idx, None]
    train = np.sort(np.argsort(-v[idx], kind="stable")[:max(1, int(max_train))])   # rows of `unit`, in their own order
    x = unit[train]
    if len(x) == 1:
        raw = np.ones(1, dtype=np.int64)
    else:
        tree = linkage(x, method="centroid", metric="euclidean")
        if num_speakers is not None:
            # the tree's merges in their order until that many clusters are left: centroid linkage is not monotonic (the centroid
            # of two orthogonal unit vectors is nearer to a third than they were to each other), which fcluster's "maxclust"
            # cannot cut at every count
            want = max(1, min(int(num_speakers), len(x)))
            raw = np.arange(len(x), dtype=np.int64)          # the node every row belongs to: itself, then the merges' nodes
            for i, (a, b) in enumerate(tree[:len(x) - want, :2].astype(np.int64)):
                raw[(raw == a) | (raw == b)] = len(x) + i
        else:
            raw = fcluster(tree, float(threshold), criterion="distance")
    _, first = np.unique(raw, return_index=True)
    order = {raw[i]: n for n, i in enumerate(np.sort(first))}
    lab = np.asarray([order[r] for r in raw], dtype=np.int64)
    cents = np.stack([x[lab == q].mean(axis=0) for q in range(len(order))])
    if num_speakers is None and len(cents) > 1:
        sizes = np.bincount(lab, minlength=len(cents))
        large = np.flatnonzero(sizes >= int(min_cluster_size))
        if len(large) == 0:
            large = np.asarray([int(np.argmax(sizes))])
        if len(large) < len(cents):
            lc = cents[large]
            for q in range(len(cents)):
                if q not in large:
                    lab[lab == q] = large[int(np.argmax(_cosine(cents[q][None], lc)[0]))]
            keep = {int(q): n for n, q in enumerate(large)}
            lab = np.asarray([keep[int(q)] for q in lab], dtype=np.int64)
            cents = np.stack([x[lab == q].mean(axis=0) for q in range(len(large))])
    labels[idx] = np.argmax(_cosine(unit, cents), axis=1)
    return labels.reshape(lead), cents


def _cosine(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Cosine similarity of every row of a with every row of b."""
    an = a / np.maximum(np.sqrt((a * a).sum(axis=1, keepdims=True)), 1e-30)
    bn = b / np.maximum(np.sqrt((b * b).sum(axis=1, keepdims=True)), 1e-30)
    return an @ bn.T


# ---- reconstruction ------------------------------------------------------------------------------------------------------

class Turn(NamedTuple):
    start: float
    end: float
    speaker: object   # the cluster's number (reconstruct) or its "SPEAKER_xx" label (WhisperModel.diarize)


def _chunk_start_frame(k: int) -> int:
    return (vad.PYANNET_STEP * k + 135) // vad.PYANNET_FRAME_STEP


def n_frames(n_samples: int, n_chunks: int) -> int:
    """F(n) of include/ttasr.h: the frames of a recording of n samples with K chunks."""
    return 0 if n_chunks == 0 else min(-(-int(n_samples) // vad.PYANNET_FRAME_STEP), _chunk_start_frame(n_chunks - 1) + FRAMES)


def speaker_activations(chunk_probs, labels, n_samples: int, onset: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """chunk_probs [K, 293, C], labels [K, C] (-1: a local speaker without a cluster) -> (activations [F, n_clusters],
    speaker count [F] before rounding).  Per chunk and cluster: the maximum over the local speakers given to the cluster (0
    when there is none); the chunks are overlap-added with the segmentation network's Hamming window on its frame grid
    (chunk k's frame f lands on recording frame (8000 k + 135) // 270 + f; a weighted mean, chunks ascending).  The speaker
    count of a chunk frame is the number of local speakers with probability >= onset, aggregated in the same way."""
    p = np.asarray(chunk_probs, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    k_n = p.shape[0]
    n_clusters = int(lab.max()) + 1 if lab.size and lab.max() >= 0 else 0
    f_n = n_frames(n_samples, k_n)
    win = np.hamming(FRAMES).astype(np.float32).astype(np.float64)
    act = np.zeros((f_n, n_clusters))
    cnt = np.zeros(f_n)
    den = np.zeros(f_n)
    for k in range(k_n):
        s = _chunk_start_frame(k)
        m = min(FRAMES, f_n - s)
        if m <= 0:
            continue
        per = np.zeros((FRAMES, n_clusters))
        for c in range(p.shape[2]):
            if lab[k, c] >= 0:
                per[:, lab[k, c]] = np.maximum(per[:, lab[k, c]], p[k, :, c])
        act[s:s + m] += win[:m, None] * per[:m]
        cnt[s:s + m] += win[:m] * (p[k, :m] >= onset).sum(axis=1)
        den[s:s + m] += win[:m]
    den = np.maximum(den, 1e-30)
    return act / den[:, None], cnt / den


def reconstruct(chunk_probs, labels, n_samples: int, onset: float = 0.5, min_duration_on: float = 0.0,
                min_duration_off: float = 0.0) -> List[Turn]:
    """Who spoke when: speaker_activations, then per frame the `count` clusters with the largest activation are active, count =
    the aggregated speaker count rounded half up and capped at the number of clusters (ties: the lower cluster number).
    Frame j stands at t_j = (495 + 270 j) / 16 000 s; a turn opens at the first active frame of a cluster and closes at its
    first inactive frame (at the last frame when still open).  Per cluster, turns whose gap is <= min_duration_off are merged
    (min_duration_off > 0 only) and turns shorter than min_duration_on are dropped; the turns are clipped to the recording and
    returned in order of (start, cluster)."""
    act, cnt = speaker_activations(chunk_probs, labels, n_samples, onset)
    f_n, n_clusters = act.shape
    count = np.minimum(np.floor(cnt + 0.5).astype(np.int64), n_clusters)
    rank = np.argsort(-act, axis=1, kind="stable")
    active = np.zeros((f_n, n_clusters), dtype=bool)
    for j in range(f_n):
        active[j, rank[j, :count[j]]] = True
    at = lambda j: (vad.PYANNET_FRAME_CENTRE + vad.PYANNET_FRAME_STEP * j) / float(vad.SAMPLING_RATE)   # noqa: E731
    dur = n_samples / float(vad.SAMPLING_RATE)
    turns: List[Turn] = []
    for c in range(n_clusters):
        segs, start = [], None
        for j in range(f_n):
            if active[j, c] and start is None:
                start = at(j)
            elif not active[j, c] and start is not None:
                segs.append([start, at(j)])
                start = None
        if start is not None:
            segs.append([start, at(f_n - 1)])
        merged: List[List[float]] = []
        for s in segs:
            if merged and min_duration_off > 0 and s[0] - merged[-1][1] <= min_duration_off:
                merged[-1][1] = s[1]
            else:
                merged.append(s)
        for a, b in merged:
            a, b = max(a, 0.0), min(b, dur)
            if b > a and b - a >= min_duration_on:
                turns.append(Turn(a, b, c))
    turns.sort(key=lambda t: (t.start, t.speaker))
    return turns


def label_turns(turns: Sequence[Turn]) -> List[Turn]:
    """Cluster numbers -> "SPEAKER_00", "SPEAKER_01", ... in the order of first appearance."""
    names: Dict[object, str] = {}
    out = []
    for t in turns:
        names.setdefault(t.speaker, f"SPEAKER_{len(names):02d}")
        out.append(Turn(t.start, t.end, names[t.speaker]))
    return out


def assign_speakers(items, turns: Sequence[Turn]) -> list:
    """The speaker of every item - anything with .start and .end in seconds (Segment, Word), or a (start, end) pair: the one
    whose turns overlap it longest (ties: the speaker that appears first in `turns`); None without any overlap."""
    out = []
    for it in items:
        a, b = (it.start, it.end) if hasattr(it, "start") else (it[0], it[1])
        total: Dict[object, float] = {}
        for t in turns:
            o = min(b, t.end) - max(a, t.start)
            if o > 0:
                total[t.speaker] = total.get(t.speaker, 0.0) + o
        out.append(max(total, key=lambda s: total[s]) if total else None)   # max keeps the first of equal totals
    return out


# ---- the pipeline --------------------------------------------------------------------------------------------------------

DEFAULT_THRESHOLD = 0.7   # centroid distance between unit vectors at which the tree is cut (UNPINNED; a tuning value)


def diarize_from(chunk_probs, embeddings, masks, n_samples: int, threshold: float = DEFAULT_THRESHOLD,
                 num_speakers: Optional[int] = None, onset: float = 0.5, min_cluster_size: int = 2, max_train: int = 2000,
                 min_duration_on: float = 0.0, min_duration_off: float = 0.0) -> List[Turn]:
    """The host half of the pipeline behind the two networks: chunk probabilities [K, 293, C], the embeddings [K, C, D] of the
    masks [K, C, 293] -> labelled turns.  A local speaker that is never active, or whose embedding is NaN, belongs to no
    cluster."""
    masks = np.asarray(masks)
    labels, _ = cluster_embeddings(embeddings, masks.sum(axis=2), threshold, num_speakers, min_cluster_size, max_train)
    return label_turns(reconstruct(chunk_probs, labels, n_samples, onset, min_duration_on, min_duration_off))


def diarize(engine, audio: np.ndarray, **kw) -> List[Turn]:
    """One recording (mono float32 @16 kHz) through the pipeline on `engine`, which holds both networks: two device calls - the
    segmentation, then the embeddings - with the mask step on the host between them.  Keywords: diarize_from's, and
    exclude_overlap / min_frames of local_speaker_masks."""
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    mk = {k: kw.pop(k) for k in ("exclude_overlap", "min_frames") if k in kw}
    _, probs, _ = engine.segmentation_scores([audio], return_chunks=True)
    if probs[0].shape[0] == 0:
        return []
    masks = local_speaker_masks(probs[0], kw.get("onset", 0.5), **mk)
    emb = engine.speaker_embeddings([audio], [masks])[0]
    return diarize_from(probs[0], emb, masks, len(audio), **kw)


# ---- the speaker-labelled subtitle -----------------------------------------------------------------------------------------

def srt_timestamp(seconds: float) -> str:
    """hh:mm:ss,mmm as the reference service writes it (api/file_asr.py:482-514): the time is rounded to whole milliseconds FIRST
    (Python's round of seconds x 1000) and split afterwards, so 59.9996 s carries into the minute; None and negative times are
    0; hours grow past 99 without a limit."""
    ms = int(round(max(float(seconds or 0.0), 0.0) * 1000))
    s, ms = divmod(ms, 1000)
    m, s = divmod(s, 60)
    h, m = divmod(m, 60)
    return f"{h:02d}:{m:02d}:{s:02d},{ms:03d}"


def dia_srt(cues: Sequence[Tuple[float, float, Optional[str], str]]) -> str:
    """(start, end, speaker, text) cues -> the SRT text of the DIA subtitle: the index, "start --> end", the text prefixed with
    "SPEAKER_xx: " (nothing for a cue without a speaker), an empty line.  The reference service's conventions: line breaks inside
    a text become spaces and the text is stripped; every line ends CRLF.  Write the result in binary or with newline="": the
    reference's own writer opens its file with newline="\\r\\n" AND writes "\\r\\n", which doubles the CR on disk; its comment
    asks for CRLF, and CRLF is what this gives."""
    lines = []
    for i, (a, b, who, text) in enumerate(cues, 1):
        text = (text or "").replace("\r", " ").replace("\n", " ").strip()
        lines += [str(i), f"{srt_timestamp(a)} --> {srt_timestamp(b)}", (f"{who}: " if who else "") + text, ""]
    return "\r\n".join(lines) + ("\r\n" if lines else "")
