"""Writes tests/golden/seq_bias_hf.npz: the cases of tests/seq_bias_cases.py at a 64-id vocabulary, fed row by row through HF
Transformers' own SequenceBiasLogitsProcessor on the CPU.  Per case i the raw logits `raw_i` and the processed rows `out_i`
(float32 [rows][64]); `cases` holds, as JSON, every case's name, table (in order) and histories (null: a row the launch leaves
alone, copied through unchanged); `transformers` the version that produced the file.

    python tools/make_golden_seq_bias.py          # needs torch and transformers; no GPU
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seq_bias_cases as S  # noqa: E402


def hf_rows(raw: np.ndarray, histories, table) -> np.ndarray:
    import torch
    from transformers import SequenceBiasLogitsProcessor
    proc = SequenceBiasLogitsProcessor({tuple(ids): float(b) for ids, b in table})
    out = raw.copy()
    for r, hist in enumerate(histories):
        if hist is None:
            continue
        ids = torch.tensor([list(hist)], dtype=torch.long).reshape(1, len(hist))
        out[r] = proc(ids, torch.from_numpy(raw[r:r + 1].copy())).numpy()[0]
    return out


def main() -> int:
    import transformers
    arrays, record = {}, []
    for i, case in enumerate(S.cases(S.GOLDEN_VOCAB)):
        raw = case.logits(S.GOLDEN_VOCAB)
        arrays[f"raw_{i}"], arrays[f"out_{i}"] = raw, hf_rows(raw, case.histories(), case.table)
        record.append(dict(name=case.name, table=[[list(ids), b] for ids, b in case.table], histories=case.histories()))
    path = os.path.join(ROOT, "tests", "golden", "seq_bias_hf.npz")
    np.savez_compressed(path, cases=np.asarray(json.dumps(record)), transformers=np.asarray(transformers.__version__), **arrays)
    print(path, os.path.getsize(path), "bytes,", len(record), "cases, transformers", transformers.__version__)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
