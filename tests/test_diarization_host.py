"""CPU: the host side of speaker diarization - the C ABI's declarations, the masks, the clustering, the reconstruction and turn
rules against a loop-written restatement, the speaker of a segment, the SRT conventions against the reference service's
recorded output, the folder tool's --diarize on a stub model, and the conditions the GPU pipeline test rests on."""
import ctypes as C
import json
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import diarization_cases as DC
from taiwan_tongues_asr_ce_amd import _lib, batch_cli, diarization as D
from taiwan_tongues_asr_ce_amd.model import Segment, WhisperModel, Word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPK_SYMBOLS = ("ttasr_spk_load_tensor", "ttasr_spk_finalize", "ttasr_spk_dim", "ttasr_spk_embed")


# ---- ABI ----

def test_header_map_binding_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "ttasr.h"), encoding="utf-8").read()
    for s in SPK_SYMBOLS:
        assert s in _lib.SYMBOLS and re.search(r"TTASR_API \w+ " + s + r"\(", hdr), s
    assert "global: ttasr_*;" in open(os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc", "ttasr.map")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {s for s in SPK_SYMBOLS} <= {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, value in (("TTASR_SPK_GROUP", _lib.SPK_GROUP), ("TTASR_SPK_MAX_MASKS", _lib.SPK_MAX_MASKS),
                        ("TTASR_SPK_MAX_DIM", _lib.SPK_MAX_DIM), ("TTASR_SPK_STATS", _lib.SPK_STATS)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert "UNPINNED against the published pyannote/embedding checkpoint" in hdr
    assert (D.MAX_MASKS, D.MAX_DIM, D.STATS) == (_lib.SPK_MAX_MASKS, _lib.SPK_MAX_DIM, _lib.SPK_STATS)


def test_a_null_context_is_refused_without_a_crash():
    lib = _lib.load()
    one = np.zeros(1, np.float32)
    dims = (C.c_int64 * 1)(1)
    assert lib.ttasr_spk_load_tensor(None, b"embedding.bias", one.ctypes.data, dims, 1) == -1
    assert lib.ttasr_spk_finalize(None) == -1 and lib.ttasr_spk_dim(None) == -1
    ptr = (C.c_void_p * 1)(one.ctypes.data)
    ns = (C.c_int64 * 1)(1)
    assert lib.ttasr_spk_embed(None, 1, ptr, ns, 1, ptr, ptr, None) == -1


# ---- masks ----

def _probs(k=1, c=3):
    return np.zeros((k, 293, c))


def test_masks_exclude_overlap_and_fall_back_below_min_frames():
    p = _probs()
    p[0, 10:60, 0] = 0.9            # speaker 0: 50 frames, 20 of them under speaker 1
    p[0, 40:70, 1] = 0.5            # speaker 1: 30 frames (>= onset counts), 20 overlapped + 10 clean
    p[0, 45:50, 2] = 0.7            # speaker 2: 5 frames, all overlapped
    p[0, 100:103, 2] = 0.499        # below the onset
    m = D.local_speaker_masks(p, onset=0.5, min_frames=10)
    assert m.shape == (1, 3, 293) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0}
    assert np.flatnonzero(m[0, 0]).tolist() == list(range(10, 40))
    assert np.flatnonzero(m[0, 1]).tolist() == list(range(60, 70))                          # exactly min_frames stay: no fallback
    assert np.flatnonzero(m[0, 2]).tolist() == list(range(45, 50))                          # none would stay: its whole activity
    m11 = D.local_speaker_masks(p, onset=0.5, min_frames=11)
    assert np.flatnonzero(m11[0, 1]).tolist() == list(range(40, 70))                        # one frame short: the fallback
    keep = D.local_speaker_masks(p, onset=0.5, exclude_overlap=False)
    assert np.array_equal(keep.transpose(0, 2, 1), (p >= 0.5).astype(np.float32))
    assert not D.local_speaker_masks(_probs(2), 0.5).any()
    with pytest.raises(ValueError):
        D.local_speaker_masks(np.zeros((1, 292, 3)))


# ---- clustering ----

def _directions(n_per=12, dim=16, noise=0.05, seed=0, scales=True):
    rng = np.random.default_rng(seed)
    base = np.linalg.qr(rng.standard_normal((dim, dim)))[0][:3]
    truth = np.repeat(np.arange(3), n_per)
    rng.shuffle(truth)
    x = base[truth] + noise * rng.standard_normal((len(truth), dim))
    if scales:
        x *= rng.uniform(0.2, 5.0, (len(truth), 1))               # the length of an embedding says nothing
    return x, truth


def _same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def test_three_separated_directions_are_recovered_and_nan_rows_ignored():
    x, truth = _directions()
    labels, cents = D.cluster_embeddings(x, np.full(len(x), 30), threshold=0.7)
    assert cents.shape == (3, 16) and _same_partition(labels, truth)
    assert labels[0] == 0 and sorted(set(labels.tolist())) == [0, 1, 2]                      # numbered by first appearance
    y = x.copy().reshape(6, 6, 16)
    y[1, 2] = np.nan
    y[4, 0, 3] = np.inf
    valid = np.full((6, 6), 30)
    valid[5, 5] = 0                                                                        # a local speaker that never spoke
    l2, _ = D.cluster_embeddings(y, valid, threshold=0.7)
    assert l2.shape == (6, 6) and l2[1, 2] == l2[4, 0] == l2[5, 5] == -1
    keep = l2.reshape(-1) >= 0
    assert keep.sum() == 33 and _same_partition(l2.reshape(-1)[keep], truth[keep])
    assert np.array_equal(l2, D.cluster_embeddings(y, valid, threshold=0.7)[0])             # deterministic
    empty, c0 = D.cluster_embeddings(np.full((2, 4), np.nan), np.ones(2), 0.7)
    assert empty.tolist() == [-1, -1] and c0.shape == (0, 4)


def test_num_speakers_forces_the_count_and_one_speaker_is_one_cluster():
    x, truth = _directions()
    for n in (1, 2, 3, 5):
        labels, cents = D.cluster_embeddings(x, np.full(len(x), 30), threshold=0.7, num_speakers=n)
        assert len(cents) == n and len(set(labels.tolist())) == n
    one = _directions(seed=3)[0][_directions(seed=3)[1] == 0]
    labels, cents = D.cluster_embeddings(one, np.full(len(one), 5), threshold=0.7)
    assert len(cents) == 1 and not labels.any()
    labels, cents = D.cluster_embeddings(one[:1], [5], threshold=0.7)                        # a single embedding
    assert labels.tolist() == [0] and len(cents) == 1
    assert len(D.cluster_embeddings(one[:1], [5], threshold=0.7, num_speakers=4)[1]) == 1     # fewer rows than speakers


def test_small_clusters_fold_into_the_nearest_large_one():
    x, truth = _directions(n_per=10, noise=0.02)
    stray = x[truth == 1][:1] * 0 + (x[truth == 1][0] / np.linalg.norm(x[truth == 1][0]) + 0.9 * x[truth == 2][0] / np.linalg.norm(x[truth == 2][0]))
    y = np.concatenate([x, stray])
    labels, cents = D.cluster_embeddings(y, np.full(len(y), 30), threshold=0.35, min_cluster_size=1)
    assert len(cents) == 4 and np.sum(labels == labels[-1]) == 1                             # on its own without the rule ...
    labels, cents = D.cluster_embeddings(y, np.full(len(y), 30), threshold=0.35, min_cluster_size=2)
    assert len(cents) == 3 and labels[-1] == labels[:-1][truth == 1][0]                      # ... with it: in the nearer of the two


def test_max_train_takes_the_rows_with_the_most_clean_frames_deterministically():
    x, truth = _directions(n_per=20)
    valid = np.arange(len(x)) % 7 + 1
    a = D.cluster_embeddings(x, valid, threshold=0.7, max_train=15)
    b = D.cluster_embeddings(x, valid, threshold=0.7, max_train=15)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert _same_partition(a[0], truth)                                                    # every row is assigned, trained on or not
    # the training rows: most clean frames first, ties by order - the centroids are those of that subset alone
    train = np.sort(np.argsort(-valid, kind="stable")[:15])
    assert valid[train].min() >= 6 and set(np.flatnonzero(valid == 7)) <= set(train)
    c, _ = D.cluster_embeddings(x[train], valid[train], threshold=0.7), None
    assert np.allclose(a[1], c[1])


# ---- reconstruction and turn rules ----

def _loop_reconstruct(probs, labels, n, onset, on, off):
    """The rules of diarization.reconstruct, frame by frame in plain loops."""
    K, C_ = probs.shape[0], probs.shape[2]
    n_cl = max([l for row in labels for l in row] + [-1]) + 1
    F = 0 if K == 0 else min(-(-n // 270), (8000 * (K - 1) + 135) // 270 + 293)
    win = [float(np.float32(0.54 - 0.46 * np.cos(2 * np.pi * f / 292))) for f in range(293)]
    turns = []
    state = [None] * n_cl
    segs = [[] for _ in range(n_cl)]
    for j in range(F):
        num, cnt, den = [0.0] * n_cl, 0.0, 0.0
        for k in range(K):
            f = j - (8000 * k + 135) // 270
            if 0 <= f < 293:
                for q in range(n_cl):
                    best = 0.0
                    for c in range(C_):
                        if labels[k][c] == q:
                            best = max(best, probs[k, f, c])
                    num[q] += win[f] * best
                cnt += win[f] * sum(1 for c in range(C_) if probs[k, f, c] >= onset)
                den += win[f]
        count = min(int(np.floor(cnt / den + 0.5)), n_cl)
        order = sorted(range(n_cl), key=lambda q: (-num[q] / den, q))[:count]
        t = (495 + 270 * j) / 16000.0
        for q in range(n_cl):
            if q in order and state[q] is None:
                state[q] = t
            elif q not in order and state[q] is not None:
                segs[q].append([state[q], t])
                state[q] = None
    for q in range(n_cl):
        if state[q] is not None:
            segs[q].append([state[q], (495 + 270 * (F - 1)) / 16000.0])
        merged = []
        for s in segs[q]:
            if merged and off > 0 and s[0] - merged[-1][1] <= off:
                merged[-1][1] = s[1]
            else:
                merged.append(s)
        for a, b in merged:
            a, b = max(a, 0.0), min(b, n / 16000.0)
            if b > a and b - a >= on:
                turns.append((a, b, q))
    return sorted(turns, key=lambda t: (t[0], t[2]))


def _random_case(seed, k_n, n):
    rng = np.random.default_rng(seed)
    t = np.arange(293)[None, :, None]
    probs = 0.5 + 0.5 * np.sin(2 * np.pi * (t / rng.uniform(40, 200, (k_n, 1, 3)) + rng.uniform(0, 1, (k_n, 1, 3))))
    probs = np.clip(probs + 0.05 * rng.standard_normal(probs.shape), 0, 1)
    labels = rng.integers(-1, 3, (k_n, 3))
    return probs, labels, n


@pytest.mark.parametrize("seed,k_n,n,on,off", [(0, 1, 40000, 0.0, 0.0), (1, 1, 80000, 0.1, 0.0), (2, 3, 96000, 0.0, 0.2),
                                               (3, 4, 99000, 0.25, 0.3), (4, 12, 80000 + 88000, 0.5, 0.5)])
def test_reconstruct_equals_the_loop_written_reference(seed, k_n, n, on, off):
    probs, labels, n = _random_case(seed, k_n, n)
    got = D.reconstruct(probs, labels, n, 0.5, on, off)
    want = _loop_reconstruct(probs, labels.tolist(), n, 0.5, on, off)
    assert len(got) == len(want) and len(got) >= 1
    for g, w in zip(got, want):
        assert g.speaker == w[2] and abs(g.start - w[0]) < 1e-9 and abs(g.end - w[1]) < 1e-9


def test_turn_rules_on_a_hand_made_case():
    p = _probs(1, 2)
    p[0, 10:50, 0] = 0.9                                         # speaker 0 alone, then both, then speaker 1 alone
    p[0, 40:90, 1] = 0.8
    p[0, 100:102, 0] = 0.9                                       # a blip of two frames, 10 frames after its last turn
    at = lambda j: (495 + 270 * j) / 16000.0                     # noqa: E731
    turns = D.reconstruct(p, [[0, 1]], 80000, 0.5)
    assert [(t.speaker, t.start, t.end) for t in turns] == [(0, at(10), at(50)), (1, at(40), at(90)), (0, at(100), at(102))]
    assert [t.speaker for t in D.reconstruct(p, [[0, 1]], 80000, 0.5, min_duration_on=0.1)] == [0, 1]
    filled = D.reconstruct(p, [[0, 1]], 80000, 0.5, min_duration_off=1.0)
    assert [(t.speaker, t.start, t.end) for t in filled] == [(0, at(10), at(102)), (1, at(40), at(90))]
    assert D.reconstruct(p, [[0, 0]], 80000, 0.5)[0][:2] == (at(10), at(90))                 # one cluster: count 2 is capped at 1
    assert D.reconstruct(p, [[-1, -1]], 80000, 0.5) == [] and D.reconstruct(_probs(0, 2), np.zeros((0, 2), int), 0) == []
    named = D.label_turns([D.Turn(0, 1, 7), D.Turn(1, 2, 3), D.Turn(2, 3, 7)])
    assert [t.speaker for t in named] == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_00"]


# ---- the speaker of a segment ----

def test_assign_speakers_largest_overlap_wins_and_none_without_overlap():
    turns = [D.Turn(0.0, 2.0, "SPEAKER_00"), D.Turn(2.0, 5.0, "SPEAKER_01"), D.Turn(6.0, 6.5, "SPEAKER_00")]
    seg = lambda a, b: Segment(0, 0, a, b, "x", [], 0.0, 0.0, 0.0, 0.0, None)   # noqa: E731
    items = [seg(0.5, 1.5), seg(1.0, 4.0), seg(1.5, 2.4), seg(5.0, 6.0), seg(5.9, 6.2), seg(1.0, 3.0), Word(4.9, 6.6, "w", 1.0), (7.0, 8.0)]
    assert D.assign_speakers(items, turns) == ["SPEAKER_00", "SPEAKER_01", "SPEAKER_00", None, "SPEAKER_00", "SPEAKER_00", "SPEAKER_00", None]
    assert D.assign_speakers([seg(0, 1)], []) == [None] and D.assign_speakers([], turns) == []
    assert Segment._fields == ("id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio",
                               "no_speech_prob", "words") and Word._fields == ("start", "end", "word", "probability")


# ---- SRT ----

def test_srt_follows_the_reference_services_recorded_output():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "srt_timestamps.json"), encoding="utf-8"))
    assert len(golden["timestamps"]) >= 20
    for t, want in golden["timestamps"]:
        assert D.srt_timestamp(t) == want, t
    assert D.srt_timestamp(59.9996) == "00:01:00,000" and D.srt_timestamp(3599.9996) == "01:00:00,000"     # the millisecond carry
    text = D.dia_srt([(0.0, 1.5, "SPEAKER_00", " 你好\n世界 "), (1.5, 59.9996, None, "ok"), (60.0, 61.0, "SPEAKER_01", "")])
    assert text == ("1\r\n00:00:00,000 --> 00:00:01,500\r\nSPEAKER_00: 你好 世界\r\n\r\n"
                    "2\r\n00:00:01,500 --> 00:01:00,000\r\nok\r\n\r\n"
                    "3\r\n00:01:00,000 --> 00:01:01,000\r\nSPEAKER_01: \r\n\r\n")
    assert "\n" not in text.replace("\r\n", "") and D.dia_srt([]) == ""


# ---- the folder tool ----

class _Seg:
    def __init__(self, text, start, end):
        self.text, self.start, self.end = text, start, end


class _Model:
    has_diarization = False

    def __init__(self):
        self.diarized, self.loaded = [], None

    def transcribe(self, audio, **kw):
        return iter([_Seg("今天", 0.0, 1.0), _Seg("天氣", 1.0, 2.5), _Seg("好", 9.0, 9.5)]), object()

    def load_diarization(self, seg, spk):
        self.loaded, self.has_diarization = (seg, spk), True

    def diarize(self, audio, num_speakers=None):
        self.diarized.append((len(audio), num_speakers))
        return [D.Turn(0.0, 1.2, "SPEAKER_00"), D.Turn(1.2, 3.0, "SPEAKER_01")]


def _wav(path, n=1600):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)   # noqa: E702
        w.writeframes(np.zeros(n, dtype="<i2").tobytes())


def test_batch_cli_diarize_writes_the_dia_srt_and_changes_nothing_else(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain, dia = tmp_path / "plain", tmp_path / "dia"
    for folder in (plain, dia):
        folder.mkdir()
        _wav(folder / "a.wav")
        _wav(folder / "b.wav", 3200)
    m0, m1 = _Model(), _Model()
    r0 = batch_cli.process_audio_folder(str(plain), model=m0, log=lambda *_: None, group_files=1, output_json=str(tmp_path / "p.json"))
    r1 = batch_cli.process_audio_folder(str(dia), model=m1, log=lambda *_: None, group_files=1, output_json=str(tmp_path / "d.json"),
                                        diarize=True, seg_model="seg.npz", spk_model="spk.npz", num_speakers=2)
    assert r0 == r1 and (tmp_path / "p.json").read_bytes() == (tmp_path / "d.json").read_bytes()
    assert sorted(os.listdir(plain)) == ["a.wav", "a_asr.txt", "b.wav", "b_asr.txt"] and not m0.diarized and m0.loaded is None
    assert sorted(os.listdir(dia)) == ["a.wav", "a_asr.txt", "a_dia.srt", "b.wav", "b_asr.txt", "b_dia.srt"]
    for n in ("a_asr.txt", "b_asr.txt"):
        assert (plain / n).read_bytes() == (dia / n).read_bytes()
    assert m1.loaded == ("seg.npz", "spk.npz") and m1.diarized == [(1600, 2), (3200, 2)]
    assert (dia / "a_dia.srt").read_bytes().decode("utf-8") == (
        "1\r\n00:00:00,000 --> 00:00:01,000\r\nSPEAKER_00: 今天\r\n\r\n2\r\n00:00:01,000 --> 00:00:02,500\r\nSPEAKER_01: 天氣\r\n\r\n"
        "3\r\n00:00:09,000 --> 00:00:09,500\r\n好\r\n\r\n")
    with pytest.raises(ValueError, match="seg_model"):
        batch_cli.process_audio_folder(str(plain), model=_Model(), log=lambda *_: None, diarize=True)
    # the command line: the flag needs both models, and the models need the flag
    assert batch_cli.main([str(plain), "--diarize"]) == 1 and batch_cli.main([str(plain), "--seg-model", "x"]) == 1
    args = batch_cli.build_parser().parse_args([str(plain), "--diarize", "--seg-model", "s", "--spk-model", "k", "--num-speakers", "3"])
    assert (args.diarize, args.seg_model, args.spk_model, args.num_speakers) == (True, "s", "k", 3)
    assert batch_cli.build_parser().parse_args([str(plain)]).diarize is False


# ---- the pipeline on the reference, and the conditions of the GPU test ----

def test_reference_pipeline_finds_two_speakers_and_no_decision_is_near_its_threshold():
    from pyannet_reference import cached_scores
    from scipy.cluster.hierarchy import linkage
    import xvector_cases as XC
    ref = DC.reference_pipeline()
    sig = DC.two_voice_signal()
    probs, emb, masks = ref["probs"], ref["emb"], ref["masks"]
    assert 29.0 < len(sig) / 16000 < 31.0 and probs.shape == (51, 293, 3)
    # what float32 costs the segmentation reference on this signal, and the tolerance that follows
    p32 = cached_scores(DC.SEG_SEED, "two voices", sig, np.float32, classes=DC.SEG_CLASSES)[1]
    f32 = float(np.abs(p32 - probs).max())
    margin = float(np.abs(probs - DC.ONSET).min())
    print(f"segmentation float32 vs float64 on the signal {f32:.3e} (recorded {DC.F32_PROB:.1e}); tolerance {DC.PROB_TOL:.2e}; "
          f"nearest probability to the onset {margin:.3e}; active {float((probs >= DC.ONSET).mean()):.4f}")
    assert DC.F32_PROB / 4 <= f32 <= DC.F32_PROB * 1.1 and DC.PROB_TOL == 16 * DC.F32_PROB
    assert margin > DC.PROB_TOL
    # the cut: no merge height within what the embeddings' tolerance can move a distance between unit vectors
    ok = ~np.isnan(emb).any(axis=2)
    assert np.array_equal(ok, masks.sum(axis=2) > 0) or ok.sum() <= (masks.sum(axis=2) > 0).sum()
    norm = np.linalg.norm(emb[ok], axis=1)
    unit = emb[ok] / norm[:, None]
    move = 4 * XC.EMB_TOL * np.abs(emb[ok]).max() * np.sqrt(emb.shape[2]) / norm.min()   # both ends of a distance, every entry off by the tolerance, twice over
    heights = linkage(unit, method="centroid")[:, 2]
    gap = float(np.abs(heights - DC.THRESHOLD).min())
    print(f"{ok.sum()} usable embeddings; a distance moves by at most {move:.3e}; nearest merge height to the cut {gap:.3e}")
    assert gap > move
    labels, cents = D.cluster_embeddings(emb, masks.sum(axis=2), DC.THRESHOLD)
    assert len(cents) == 2 and np.bincount(labels[labels >= 0]).min() >= 2
    sims = np.stack([unit @ (c / np.linalg.norm(c)) for c in cents], axis=1)
    assert float(np.abs(sims[:, 0] - sims[:, 1]).min()) > move                             # the nearest centroid is clearly nearer
    act, cnt = D.speaker_activations(probs, labels, len(sig), DC.ONSET)
    assert float(np.abs(cnt - (np.floor(cnt) + 0.5)).min()) > 1e-3                           # the count is a mean of integers: it moves only when a decision flips
    one = np.floor(cnt + 0.5) == 1
    assert one.any() and float(np.abs(act[one, 0] - act[one, 1]).min()) > 2 * DC.PROB_TOL   # who is the most active is clear
    turns = ref["turns"]
    assert len(turns) >= 3 and set(turns[:, 2]) == {0.0, 1.0}                                # two speakers are found


def test_whisper_model_diarize_is_two_engine_calls_with_the_masks_between():
    ref = DC.reference_pipeline()
    sig = DC.two_voice_signal()
    calls = []

    class _Engine:
        has_segmentation = has_speaker_embedding = True

        def segmentation_scores(self, audios, return_chunks=False):
            calls.append(("seg", len(audios[0]), return_chunks))
            return [None], [ref["probs"].astype(np.float32)], [None]

        def speaker_embeddings(self, audios, weights):
            calls.append(("spk", len(audios[0]), weights[0].copy()))
            return [ref["emb"].astype(np.float32)]

    m = WhisperModel.__new__(WhisperModel)
    m.engine = _Engine()
    with pytest.raises(RuntimeError, match="load_diarization"):
        m.diarize(sig)
    m._diarization = True
    turns = m.diarize(sig, threshold=DC.THRESHOLD, onset=DC.ONSET, min_frames=DC.MIN_FRAMES)
    assert [c[0] for c in calls] == ["seg", "spk"] and calls[0][2] is True and np.array_equal(calls[1][2], ref["masks"])
    assert np.array_equal(DC.turns_array(turns), ref["turns"]) and turns[0].speaker == "SPEAKER_00"
    assert {t.speaker for t in turns} == {"SPEAKER_00", "SPEAKER_01"}
    forced = m.diarize(sig, num_speakers=1, onset=DC.ONSET)
    assert {t.speaker for t in forced} == {"SPEAKER_00"}
    m.transcribe = lambda audio, **kw: (iter([Segment(0, 0, turns[0].start, turns[0].end, "a", [], 0, 0, 0, 0, None),
                                              Segment(1, 0, 1000.0, 1001.0, "b", [], 0, 0, 0, 0, None)]), "info")
    pairs, info = m.transcribe_diarized(sig, diarization_options=dict(threshold=DC.THRESHOLD, onset=DC.ONSET, min_frames=DC.MIN_FRAMES))
    assert info == "info" and [(s.text, who) for s, who in pairs] == [("a", "SPEAKER_00"), ("b", None)]
