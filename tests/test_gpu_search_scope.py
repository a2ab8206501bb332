"""GPU: a search cannot leave its context half-configured, and two decode shapes never share a step graph.

What picks the kernels of a decode step is one value - the context's `KernelOpts` plus the `StepShape` (rows per clip, identity
or loaded page tables, static or per-row positions) that a `SearchScope` installs for one search and restores on every exit.
The captured step graphs are keyed on that value, so searches of different shapes interleaved on ONE context must give, bit for
bit, what each gives as the only search of a fresh context; and a search that is refused or ends in an error must leave the
defaults behind: live rows, no copy in flight.

Geometry: the `tiny` preset, bf16, synthetic weights, noise clips; 12 new tokens, EOT allowed."""
import ctypes as C

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import _lib, synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, PRESETS

pytestmark = pytest.mark.gpu

DIMS = PRESETS["tiny"]
N_NEW = 12
E_INVALID = -1   # include/ttasr.h TTASR_E_INVALID


@pytest.fixture(scope="module")
def world():
    return dict(synth.state_dict(DIMS)), [synth.noise_clip(500 + i) for i in range(6)]


def _engine(sd, max_batch):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, COMPUTE_BF16, max_batch)
    e.load_weights(sd.items())
    return e


def _prompt(e):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def _encode(e, clips):
    e.log_mel(clips, want_output=False)
    e.encode(len(clips))


def _result(r):
    return r.tokens, np.asarray(r.sum_logprob, np.float32).copy(), np.asarray(r.no_speech_prob, np.float32).copy()


def _session(e, clips, **kw):
    prompt = _prompt(e)
    with e.session(e.gen_opts(N_NEW, False), len(prompt), **kw) as s:
        ids = s.submit(clips, [prompt] * len(clips))
        got = {r.id: r for r in s.drain()}
    rs = [got[i] for i in ids]
    return [r.tokens for r in rs], np.asarray([r.sum_logprob for r in rs], np.float32), np.asarray([r.no_speech_prob for r in rs], np.float32)


def _greedy6(e, clips):
    _encode(e, clips)
    return _result(e.generate([_prompt(e)] * 6, e.gen_opts(N_NEW, False)))


def _beam(e, clips):
    _encode(e, clips[:2])
    return _result(e.generate_beam([_prompt(e)] * 2, 3, e.gen_opts(N_NEW, False)))


def _sample(e, clips):
    _encode(e, clips[:2])
    return _result(e.generate_sample([_prompt(e)] * 2, 3, e.gen_opts(N_NEW, False), 0.4, seed=7))


CALLS = [("generate 6 rows", _greedy6), ("generate_beam 2 x 3", _beam), ("generate_sample 2 x 3", _sample),
         ("greedy session", lambda e, clips: _session(e, clips)), ("beam session", lambda e, clips: _session(e, clips, beam=3)),
         ("generate 6 rows again", _greedy6)]


def test_interleaved_shapes_on_one_context_equal_each_alone(world):
    """Six searches of five different step shapes, in order, on one engine: each equals the same call as the only search of a
    fresh engine (tokens, sum_logprob, no_speech_prob, bit for bit).  Two shapes that compared equal in the graph key would
    replay each other's kernels here."""
    sd, clips = world
    shared = _engine(sd, 6)
    for name, call in CALLS:
        got = call(shared, clips)
        fresh = _engine(sd, 6)
        want = call(fresh, clips)
        fresh.close()
        assert got[0] == want[0], name
        assert np.array_equal(got[1], want[1]), (name, got[1], want[1])
        assert np.array_equal(got[2], want[2]), (name, got[2], want[2])
    shared.close()


def _generate_raw(lib, e, B, caps=None):
    """ttasr_generate / ttasr_generate_capped through the bare C ABI: (return code, tokens, lengths, sum_logprob, no_speech)."""
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    prompt = _prompt(e)
    pr = np.ascontiguousarray([prompt] * B, dtype=np.int32)
    pl = np.full(B, len(prompt), dtype=np.int32)
    opts = e.gen_opts(N_NEW, False)
    toks, lens = np.zeros((B, N_NEW), np.int32), np.zeros(B, np.int32)
    lp, ns = np.zeros(B, np.float32), np.zeros(B, np.float32)
    tail = (toks.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p))
    head = (e.h, B, pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p), len(prompt), C.byref(opts))
    if caps is None:
        rc = lib.ttasr_generate(*head, *tail)
    else:
        cp = np.ascontiguousarray(caps, dtype=np.int32)
        rc = lib.ttasr_generate_capped(*head, cp.ctypes.data_as(i32p), *tail)
    return rc, toks, lens, lp, ns


def test_refused_budget_leaves_nothing_behind(world):
    """ttasr_generate_capped with one budget of 0 is refused before anything is uploaded or enqueued; the ttasr_generate that
    follows equals a fresh engine's.  Engine.generate checks the range itself and never reaches the library."""
    sd, clips = world
    lib = _lib.load()
    e, fresh = _engine(sd, 4), _engine(sd, 4)
    _encode(e, clips[:4])
    _encode(fresh, clips[:4])
    rc = _generate_raw(lib, e, 4, caps=[N_NEW, 0, N_NEW, N_NEW])[0]
    assert rc == E_INVALID
    assert b"row_max_new[1]=0" in lib.ttasr_last_error(e.h)
    got, want = _generate_raw(lib, e, 4), _generate_raw(lib, fresh, 4)
    assert got[0] == 0 and want[0] == 0
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a, b), (a, b)

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")
    real, e.lib = e.lib, NoLibrary()
    try:
        for bad in ([0, 4, 4, 4], [4, 4, 4, N_NEW + 1], [-1, 1, 1, 1]):
            with pytest.raises(ValueError):
                e.generate([_prompt(e)] * 4, e.gen_opts(N_NEW, False), row_max_new=bad)
    finally:
        e.lib = real
    e.close(); fresh.close()


def test_search_that_ends_in_an_error_leaves_live_rows(world):
    """Beam search with every vocabulary id suppressed stops with the library's own "no live candidate" refusal (a host-side
    return in the middle of the search, no device fault).  The step-level calls that follow see four live rows at the default
    shape: their logits equal a fresh engine's."""
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    sd, clips = world
    e, fresh = _engine(sd, 4), _engine(sd, 4)
    _encode(e, clips[:4])
    _encode(fresh, clips[:4])
    opts = e.gen_opts(N_NEW, False, suppress=list(range(DIMS.vocab)))
    with pytest.raises(TtasrError, match="no live candidate"):
        e.generate_beam([_prompt(e)] * 2, 2, opts)
    tok = [e.special.sot] * 4
    e.decode_reset(4)
    fresh.decode_reset(4)
    got, want = e.decode_step(tok), fresh.decode_step(tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want), np.abs(got - want).max(axis=1)
    e.close(); fresh.close()
