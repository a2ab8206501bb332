"""Keyword biasing on the host: the sequence-bias table of Engine.set_sequence_bias (ttasr_set_sequence_bias; DESIGN.md section
4.34) - its checks, the flat form the library takes, the grouped form the library builds from it - and the expansion of
`prompt_words` into such a table.  The definition is HF Transformers' SequenceBiasLogitsProcessor."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

MAX_LEN = 16          # tokens of one sequence (kSeqBiasMaxLen of csrc/seq_bias.hpp)
WINDOW = MAX_LEN - 1  # history tokens a match can look at
MAX_GROUPS = 4096     # distinct last tokens
MAX_ENTRIES = 8192    # sequences longer than one token
DEFAULT_BOOST = 2.0   # prompt_word_boost: a starting value nobody has measured (no trained checkpoint is available offline)

Table = List[Tuple[Tuple[int, ...], float]]

LOCK_STEP_ONLY = ("{what}: sequence_bias / prompt_words are not available in a continuous-batching session (the session's kernels "
                  "do not apply the table); use the lock-step form, transcribe_many(..., continuous=False)")


def refuse_in_session(what: str, sequence_bias=None, prompt_words=None) -> None:
    """The ValueError of every continuous surface for a sequence_bias / prompt_words that is given; raised before any device work."""
    if sequence_bias or split_prompt_words(prompt_words):
        raise ValueError(LOCK_STEP_ONLY.format(what=what))


def check_table(mapping: Union[Mapping, Iterable], vocab: int) -> Table:
    """{tuple of ids: bias} (or an iterable of (ids, bias)) -> [(ids, bias)] in the mapping's order, every cap of the library
    checked first: ValueError names the sequence that is refused."""
    items = list(mapping.items()) if isinstance(mapping, Mapping) else [tuple(kv) for kv in mapping]
    out: Table = []
    seen, last = set(), set()
    n_long = 0
    for key, bias in items:
        try:
            ids = tuple(int(t) for t in key)
            ok = all(int(t) == t for t in key)
        except (TypeError, ValueError):
            raise ValueError(f"sequence_bias: key {key!r} is not a tuple of token ids") from None
        if not ok:
            raise ValueError(f"sequence_bias: key {key!r} is not a tuple of token ids")
        if not 1 <= len(ids) <= MAX_LEN:
            raise ValueError(f"sequence_bias: {ids!r} has {len(ids)} tokens, outside [1, {MAX_LEN}]")
        for t in ids:
            if not 0 <= t < vocab:
                raise ValueError(f"sequence_bias: id {t} of {ids!r} is outside the vocabulary [0, {vocab})")
        try:
            b = float(bias)
        except (TypeError, ValueError):
            raise ValueError(f"sequence_bias: the bias of {ids!r} is not a number: {bias!r}") from None
        if not math.isfinite(b) or abs(b) > float(np.finfo(np.float32).max):
            raise ValueError(f"sequence_bias: the bias of {ids!r} is not finite in float32: {bias!r}")
        if ids in seen:
            raise ValueError(f"sequence_bias: {ids!r} is listed twice")
        seen.add(ids)
        last.add(ids[-1])
        n_long += len(ids) > 1
        out.append((ids, b))
    if len(last) > MAX_GROUPS:
        raise ValueError(f"sequence_bias: {len(last)} distinct last tokens, at most {MAX_GROUPS}")
    if n_long > MAX_ENTRIES:
        raise ValueError(f"sequence_bias: {n_long} sequences longer than one token, at most {MAX_ENTRIES}")
    return out


def flatten(table: Table) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> tokens int32 [sum of lengths], offsets int32 [n + 1], biases float32 [n]: the arguments of ttasr_set_sequence_bias."""
    tokens = np.asarray([t for ids, _ in table for t in ids], dtype=np.int32)
    offsets = np.zeros(len(table) + 1, dtype=np.int32)
    np.cumsum([len(ids) for ids, _ in table], out=offsets[1:])
    return tokens, offsets, np.asarray([b for _, b in table], dtype=np.float32)


def group_table(table: Table) -> Dict[str, list]:
    """The layout the library builds (csrc/seq_bias.hpp seq_bias_build), for tests and tools: groups (token, length-1 bias or None,
    first entry, entries) in the order their tokens first appear, entries (bias, prefix length, prefix offset) in table order
    inside a group, and the flat prefix tokens."""
    order: List[int] = []
    len1: Dict[int, Optional[float]] = {}
    members: Dict[int, List[Tuple[Tuple[int, ...], float]]] = {}
    for ids, b in table:
        t = ids[-1]
        if t not in members:
            order.append(t); len1[t] = None; members[t] = []
        if len(ids) == 1:
            len1[t] = b
        else:
            members[t].append((ids, b))
    groups, entries, prefix = [], [], []
    for t in order:
        groups.append((t, len1[t], len(entries), len(members[t])))
        for ids, b in members[t]:
            entries.append((b, len(ids) - 1, len(prefix)))
            prefix.extend(ids[:-1])
    return dict(groups=groups, entries=entries, prefix=prefix)


def split_prompt_words(prompt_words: Union[None, str, Sequence[str]]) -> List[str]:
    """A comma-separated string (ASCII or full-width commas) or a list -> the phrases, stripped, empty ones dropped, in order."""
    if prompt_words is None:
        return []
    if isinstance(prompt_words, str):
        prompt_words = prompt_words.replace("，", ",").replace("、", ",").split(",")
    return [w.strip() for w in prompt_words if isinstance(w, str) and w.strip()]


def expand_prompt_words(prompt_words, boost: float, encode: Callable[[str], Sequence[int]]) -> Dict[Tuple[int, ...], float]:
    """Every phrase p is tokenised as p and, where that differs, as " " + p; of each tokenisation every prefix of two or more
    tokens becomes a sequence with bias `boost`, and its first token alone one with boost / 2 (the first token of a name is weak
    evidence on its own).  A tokenisation longer than 16 tokens contributes its first 16.  A key that arises twice keeps the
    larger bias."""
    boost = float(boost)
    if not math.isfinite(boost):
        raise ValueError(f"prompt_word_boost={boost!r}: a finite number")
    out: Dict[Tuple[int, ...], float] = {}

    def put(key, b):
        out[key] = max(out[key], b) if key in out else b

    for p in split_prompt_words(prompt_words):
        forms = [tuple(int(t) for t in encode(p))]
        spaced = tuple(int(t) for t in encode(" " + p))
        if spaced != forms[0]:
            forms.append(spaced)
        for ids in forms:
            ids = ids[:MAX_LEN]
            if not ids:
                continue
            put(ids[:1], boost / 2)
            for k in range(2, len(ids) + 1):
                put(ids[:k], boost)
    return out


def resolve(sequence_bias, prompt_words, boost, encode, vocab: int) -> Optional[Table]:
    """The table of one call from its options (None: no table): sequence_bias first, in its order, then what prompt_words adds; a
    key both name keeps the larger bias."""
    merged: Dict[Tuple[int, ...], float] = {}
    if sequence_bias:
        merged.update(check_table(sequence_bias, vocab))
    if split_prompt_words(prompt_words):
        for key, b in expand_prompt_words(prompt_words, DEFAULT_BOOST if boost is None else boost, encode).items():
            merged[key] = max(merged[key], b) if key in merged else b
    return check_table(merged, vocab) if merged else None
