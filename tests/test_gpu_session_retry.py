"""GPU: ttasr_session_retry / Session.retry - a new search on a held clip, with no encoder work.

A retried clip must equal, bit for bit (tokens, sum_logprob, no_speech), the same audio submitted afresh with the retry's
parameters: a window clip against a fresh Session.submit_windows, a clip that came through Session.submit against a fresh
Session.submit (it keeps its own mel, and that call's parameters are temperature 0, rows = beam, sot index = opts.sot_index).
The retries must enqueue no encoder work: encodes, clips_encoded and encode_ms of Session.stats() stay where they were.

Geometry: preset tiny, synthetic weights, max_batch 6, beam 2 (3 groups), five clips of 2-8 s of seeded noise with different
budgets, so that groups are refilled and a long clip is still live while its neighbours are retried."""
import ctypes as C

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu

DIMS = PRESETS["tiny"]
B, BEAM = 6, 2
N_NEW = 24
SECONDS = (2, 8, 3, 5, 4)
BUDGETS = (6, 24, 8, 10, 7)     # clip 1 outlives the others' first attempts and retries
PLAIN = 4                        # this clip goes in through Session.submit
LONG = 1
T_RETRY = 0.4


def _clips():
    return [synth.noise_clip(700 + i, 16000 * s) for i, s in enumerate(SECONDS)]


def _engine(compute, fp8=0):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, compute, B)
    e.load_weights(synth.state_dict(DIMS).items())
    if fp8:
        e.set_option("xkv_fp8", fp8)
    return e


def _prompt(e, n_prev):
    st = e.special
    prev = [st.sot_prev] + [1000 + 37 * j for j in range(n_prev)] if n_prev else []
    return prev + [st.sot, st.lang_zh, st.transcribe, st.no_timestamps], len(prev)


def _key(r):
    return r.tokens, np.float32(r.sum_logprob).tobytes(), np.float32(r.no_speech_prob).tobytes()


def _seed(i):
    return 9000 + 17 * i


def _fresh(e, opts, prompt, sot, prefill, clips, which, temperature):
    """One session without hold mode: the window clips `which` at `temperature` (rows 2, their seeds and budgets); with
    temperature None the PLAIN clip alone through Session.submit."""
    with e.session(opts, 32, beam=BEAM, patience=1.0, prefill=prefill) as s:
        if temperature is None:
            ids = s.submit([clips[PLAIN]], [prompt], [BUDGETS[PLAIN]])
        else:
            ids = s.submit_windows([clips[i] for i in which], [0] * len(which), [prompt] * len(which), [sot] * len(which),
                                   max_new=[BUDGETS[i] for i in which], temperature=[temperature] * len(which),
                                   rows=[BEAM] * len(which), seed=[_seed(i) for i in which])
        got = {r.id: r for r in s.drain()}
    return [_key(got[i]) for i in ids]


CASES = [pytest.param(COMPUTE_F32, 0, 0, 0, id="f32"), pytest.param(COMPUTE_BF16, 0, 0, 0, id="bf16"),
         pytest.param(COMPUTE_BF16, 2, 4, 12, id="bf16-xkv_fp8-prefill4")]


@pytest.mark.parametrize("compute,fp8,prefill,n_prev", CASES)
def test_retried_clips_equal_fresh_submissions_and_encode_nothing(compute, fp8, prefill, n_prev):
    e = _engine(compute, fp8)
    try:
        clips = _clips()
        prompt, sot = _prompt(e, n_prev)
        opts = e.gen_opts(N_NEW, timestamps=False, sot_index=sot)
        windows = [i for i in range(5) if i != PLAIN]
        # the references: fresh sessions with the retry's parameters, and the long clip alone
        want_t0 = dict(zip(windows, _fresh(e, opts, prompt, sot, prefill, clips, windows, 0.0)))
        want_hot = dict(zip(windows, _fresh(e, opts, prompt, sot, prefill, clips, windows, T_RETRY)))
        want_plain, = _fresh(e, opts, prompt, sot, prefill, clips, [PLAIN], None)
        solo, = _fresh(e, opts, prompt, sot, prefill, clips, [LONG], 0.0)
        assert want_t0[LONG] == solo
        assert any(want_hot[i] != want_t0[i] for i in windows)      # the sampled attempt is another search

        with e.session(opts, 32, beam=BEAM, patience=1.0, prefill=prefill) as s:
            s.hold()
            where, attempt = {}, {}
            for i in range(5):
                if i == PLAIN:
                    cid, = s.submit([clips[i]], [prompt], [BUDGETS[i]])
                else:
                    cid, = s.submit_windows([clips[i]], [0], [prompt], [sot], max_new=[BUDGETS[i]], rows=[BEAM], seed=[_seed(i)])
                where[cid], attempt[cid] = i, 0
            got = {i: [] for i in range(5)}
            long_live_during_retry = False
            retries = 0
            while s.pending > 0:
                done = s.poll()
                assert done, "session idle with clips unfinished"
                for r in done:
                    i, k = where.pop(r.id), attempt.pop(r.id)
                    got[i].append(_key(r))
                    if k == 2:
                        s.release([r.id])
                        continue
                    # attempt 1: the sampled retry; attempt 2: the first attempt's own parameters again
                    before = s.stats()
                    temp = T_RETRY if k == 0 else 0.0
                    new, = s.retry([r.id], [prompt], [sot], max_new=[BUDGETS[i]], temperature=[temp], rows=[BEAM], seed=[_seed(i)])
                    after = s.stats()
                    retries += 1
                    assert new != r.id and new not in where
                    for name in ("encodes", "clips_encoded", "encode_ms"):
                        assert after[name] == before[name], name
                    rows = s.rows()
                    assert new in rows["clip"] and r.id not in rows["clip"]
                    if i != LONG and any(c in where and where[c] == LONG and attempt[c] == 0 for c in rows["clip"]):
                        long_live_during_retry = True
                    where[new], attempt[new] = i, k + 1
            stats = s.stats()
        assert retries == 10 and stats["clips_encoded"] == 5
        assert long_live_during_retry
        for i in windows:
            assert got[i][0] == want_t0[i], ("first attempt", i)
            assert got[i][1] == want_hot[i], ("retry at 0.4", i)
            assert got[i][2] == want_t0[i], ("retry with the first attempt's parameters", i)
        # the plain clip: its own mel stays in its slot through a sampled retry; its own parameters reproduce a fresh submit
        assert got[PLAIN][0] == want_plain and got[PLAIN][2] == want_plain
        assert got[PLAIN][1] != want_plain
        if prefill:
            assert stats["prefill_clips"] == 15     # every admission and every retry applied the rule to the 17-token prompt
    finally:
        e.close()


def test_retry_refusals_leave_the_clips_held_and_the_session_usable():
    from taiwan_tongues_asr_ce_amd.engine import Session, TtasrError
    e = _engine(COMPUTE_F32)
    try:
        clips = _clips()
        prompt, sot = _prompt(e, 0)
        opts = e.gen_opts(N_NEW, timestamps=False, sot_index=sot)
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        i64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

        def raw(ids, pr=None, rows=BEAM, budget=6):
            """ttasr_session_retry itself, past the checks of Session.retry."""
            n = len(ids)
            a = np.asarray(ids, np.int64)
            p = np.zeros((n, 32), np.int32)
            pr = prompt if pr is None else pr
            p[:, :len(pr)] = pr
            pl, so = np.full(n, len(pr), np.int32), np.full(n, sot, np.int32)
            caps, rw, sd = np.full(n, budget, np.int32), np.full(n, rows, np.int32), np.zeros(n, np.uint32)
            return e.lib.ttasr_session_retry(e.h, n, i64p(a), i32p(p), i32p(pl), i32p(so), i32p(caps), None, i32p(rw),
                                             sd.ctypes.data_as(C.POINTER(C.c_uint32)), None)

        with e.session(opts, 32, beam=BEAM, patience=1.0, detect_language=True) as s:
            first, = s.submit_windows([clips[0]], [0], [prompt], [sot], max_new=[6])
            r, = s.drain()
            assert raw([first]) == -1                       # hold mode off (and the clip is gone)
            s.hold()
            a, b = s.submit_windows([clips[0], clips[2]], [0, 0], [prompt] * 2, [sot] * 2, max_new=[6, 6])
            live, = s.submit_windows([clips[1]], [0], [prompt], [sot], max_new=[N_NEW])
            done = {}
            while a not in done or b not in done:
                done.update({r.id: r for r in s.poll()})
            assert live not in done
            assert raw([live]) == -1                        # not held: still decoding
            assert raw([first]) == -1 and raw([12345]) == -1   # released long ago / unknown
            assert raw([a, a]) == -1                        # listed twice
            detect = list(prompt)
            detect[sot + 1] = Session.DETECT
            assert raw([a], pr=detect) == -1                # the placeholder
            assert raw([a], rows=0) == -1 and raw([a], rows=BEAM + 1) == -1
            assert raw([a], budget=0) == -1 and raw([a], budget=N_NEW + 1) == -1
            assert raw([a, b], rows=0) == -1                # nothing changed for either
            rows = s.rows()["clip"]
            assert a in rows and b in rows
            with pytest.raises(ValueError):
                s.retry([a], [detect], [sot])
            # the held clips are still there: one is retried, one released, and the session drains
            new, = s.retry([a], [prompt], [sot], max_new=[6])
            s.release([b])
            with pytest.raises(TtasrError):
                s.release([a])                              # its id stopped being held
            rest = {r.id: r for r in s.drain()}
            assert _key(rest[new]) == _key(done[a]) and live in rest
            s.release([new, live])
        with e.session(opts, 32) as s:                      # a greedy session refuses the call
            s.hold()
            cid, = s.submit([clips[0]], [prompt], [6])
            s.drain()
            assert raw([cid]) == -1
            with pytest.raises(ValueError):
                s.retry([cid], [prompt], [sot])
            s.release([cid])
    finally:
        e.close()
