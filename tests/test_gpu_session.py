"""GPU: the continuous-batching session (ttasr_session_*, Engine.session, WhisperModel.transcribe_stream).

Clips submitted to a session take free rows of a max_batch-row decode batch and hand their row to the next clip when they finish.
The batch always runs at max_batch rows, every row carries its own position, and a row's computation does not depend on its
neighbours, so a clip decoded in a session must equal - bit for bit: tokens, sum_logprob, no_speech - the same clip decoded in a
static batch of max_batch rows (ttasr_generate_capped with option prefill = 0, i.e. prompts forced through ordinary steps).
That rests on the encoder giving a clip the same bits whatever number of clips shares its pass (the session encodes the clips
it admits in small batches, and in overlap mode that number depends on GPU timing).  In f32 the encoder is batch-invariant as
it is.  In bf16 / fp16 the automatic GEMM dispatch (engine_sched.hip gemm()) goes by tile count and picks the 256 x 128
gemm_bf16_v2 for a few clips, which rounds differently from the 256 x 256 family (v3 / persistent v4 / v5, bit-identical to
each other) that 32 clips get; the session's passes therefore always run the 256 x 256 family.
test_encoder_output_does_not_depend_on_the_batch holds both facts.

Geometry: the benchmark's width (large-v3-w2: d 1280, 20 heads, 2 + 2 layers), max_batch 32, 64 clips with seeded budgets 32 ... 128
(synthetic weights never emit a meaningful EOT: suppress_eot, the lengths are the budgets)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import whisper_ref as R
from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, COMPUTE_F32, PRESETS

from oracle_checks import encode_chunked, teacher_forced_causal

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DIMS = PRESETS["large-v3-w2"]
B = 32
N_CLIPS = 64
N_NEW = 128
GRADED = (0, 9, 18, 27, 36, 45, 54, 63)


def _caps(n=N_CLIPS, seed=11, lo=32, hi=N_NEW):
    return np.random.Generator(np.random.Philox(key=seed)).integers(lo, hi + 1, size=n).astype(np.int32)


def _clips(n):
    kinds = (synth.noise_clip, synth.tonal_clip, synth.noise_clip, synth.burst_clip)   # the clip kinds of test_gpu_ragged.py
    return [kinds[i % 4](300 + i) for i in range(n)]


def _engine(compute, sd):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, compute, B)
    e.load_weights(sd.items())
    return e


def _prompt(e, ts=False):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe] + ([] if ts else [st.no_timestamps])


def _opts(e, ts=False):
    return e.gen_opts(N_NEW, ts, suppress_eot=True, check_interval=8)


def _static(e, clips, caps, prompt, opts):
    """Static batches of B clips through ttasr_generate_capped, prompts forced through decode steps (prefill = 0)."""
    e.set_option("prefill", 0)
    toks, lp, ns = [], [], []
    for i in range(0, len(clips), B):
        chunk = clips[i:i + B]
        e.log_mel(chunk, want_output=False)
        e.encode(len(chunk))
        r = e.generate([prompt] * len(chunk), opts, row_max_new=caps[i:i + B])
        toks += r.tokens
        lp += list(r.sum_logprob)
        ns += list(r.no_speech_prob)
    e.set_option("prefill", 1)
    return toks, np.asarray(lp, dtype=np.float32), np.asarray(ns, dtype=np.float32)


def _session(e, clips, caps, prompt, opts, waves=1):
    """All clips through one session; returns results in input order (+ the session's statistics)."""
    n = len(clips)
    toks, lp, ns = [None] * n, np.zeros(n, np.float32), np.zeros(n, np.float32)
    with e.session(opts, len(prompt)) as s:
        cut = n if waves == 1 else n // 2
        ids = s.submit(clips[:cut], [prompt] * cut, caps[:cut])
        got = []
        if waves > 1:
            got += s.poll()                                   # the first poll runs before the second wave exists
            assert got, "a poll returns once at least one clip finished"
            ids += s.submit(clips[cut:], [prompt] * (n - cut), caps[cut:])
        got += s.drain()
        stats = s.stats()
        stats["rows"] = s.rows()
    where = {cid: i for i, cid in enumerate(ids)}
    assert len(got) == n and sorted(where[r.id] for r in got) == list(range(n))
    for r in got:
        i = where[r.id]
        toks[i], lp[i], ns[i] = r.tokens, r.sum_logprob, r.no_speech_prob
    return toks, lp, ns, stats


@pytest.fixture(scope="module")
def world():
    sd = synth.state_dict(DIMS)
    clips = _clips(N_CLIPS)
    return sd, clips, _caps()


def _same(a, b):
    ta, la, na = a[:3]
    tb, lb, nb = b[:3]
    assert len(ta) == len(tb)
    for i in range(len(ta)):
        assert ta[i] == tb[i], (i, len(ta[i]), len(tb[i]))
    assert np.array_equal(la, lb), np.flatnonzero(la != lb)
    assert np.array_equal(na, nb), np.flatnonzero(na != nb)


@pytest.mark.parametrize("compute,tol,margin", [(COMPUTE_F32, 1e-3, 2e-3), (COMPUTE_BF16, 0.15, 0.16), (COMPUTE_F16, 0.15, 0.16)],
                         ids=["f32", "bf16", "f16"])
def test_session_is_bit_identical_to_the_static_batch_and_graded(world, compute, tol, margin):
    sd, clips, caps = world
    e = _engine(compute, sd)
    prompt, opts = _prompt(e), _opts(e)
    ses = _session(e, clips, caps, prompt, opts)
    assert [len(t) for t in ses[0]] == caps.tolist() and np.isfinite(ses[1]).all()
    _same(ses, _static(e, clips, caps, prompt, opts))
    stats = ses[3]
    assert stats["clips_encoded"] == N_CLIPS and stats["live_row_steps"] == sum(len(prompt) - 1 + int(c) for c in caps)
    # refilled rows keep the batch busy (two static batches of 32 would be ~63 % occupied by these budgets)
    assert stats["live_row_steps"] > 0.5 * stats["steps"] * B, stats
    # the oracle grades 8 of the clips (one causal pass each: their lengths differ)
    rd = R.Dims(**DIMS.as_dict())
    W = R.to_torch(sd, round_bf16=compute == COMPUTE_BF16, round_f16=compute == COMPUTE_F16)
    enc_ref = encode_chunked(np.stack([R.log_mel(clips[i], DIMS.n_mels) for i in GRADED]), W, rd)
    st = e.special
    rules = R.Rules(eot=st.eot, no_timestamps=st.no_timestamps, timestamp_begin=st.timestamp_begin,
                    suppress=[opts.suppress[i] for i in range(opts.n_suppress)], begin_suppress=[220, st.eot], timestamps=False)
    rules.suppress_eot = True
    n_steps = n_clear = 0
    for k, i in enumerate(GRADED):
        g = teacher_forced_causal([ses[0][i]], prompt, enc_ref[k:k + 1], W, rd, rules, tol=tol, margin=margin, rows_per_pass=1)
        n_steps += g.n_steps
        n_clear += g.n_clear
    assert n_steps == int(sum(caps[i] for i in GRADED))
    assert n_clear >= 0.6 * n_steps, (n_clear, n_steps)
    e.close()


@pytest.mark.parametrize("compute", [COMPUTE_F32, COMPUTE_BF16], ids=["f32", "bf16"])
def test_overlap_submission_waves_and_a_nearly_empty_batch(world, compute):
    sd, clips, caps = world
    e = _engine(compute, sd)
    prompt, opts = _prompt(e), _opts(e)
    sync = _session(e, clips, caps, prompt, opts)            # the default: encode between two step runs on the one stream
    # refill_overlap 1: the encode runs on a second stream, the grouping of clips into encoder passes follows GPU timing - same bits
    e.set_option("refill_overlap", 1)
    over = _session(e, clips, caps, prompt, opts)
    again = _session(e, clips, caps, prompt, opts)
    e.set_option("refill_overlap", 0)
    _same(over, sync)
    _same(again, sync)
    # two waves: the second half is submitted after the first poll returned
    _same(_session(e, clips, caps, prompt, opts, waves=2), sync)
    # 5 clips in 32 rows: the 5 clips are what they are in the full runs, and the 27 other rows stay idle
    few = _session(e, clips[:5], caps[:5], prompt, opts)
    _same(few, ([sync[0][i] for i in range(5)], sync[1][:5], sync[2][:5]))
    st5 = few[3]
    assert st5["encodes"] == 1 and st5["clips_encoded"] == 5
    interval = 8
    longest = len(prompt) - 1 + int(caps[:5].max())
    assert st5["steps"] <= -(-longest // interval) * interval
    assert st5["live_row_steps"] == sum(len(prompt) - 1 + int(c) for c in caps[:5])
    rows = st5["rows"]
    assert (rows["clip"] == -1).all() and (rows["done"] == 1).all()           # every clip returned, every row free again
    # the admitted rows froze after their last token; the idle rows never left position 0 (a finished or free row neither
    # appends to its KV pages nor advances: kernels_attn.hip self_attn_decode_kernel leaves before the append)
    assert rows["row_pos"][:5].tolist() == [len(prompt) - 1 + int(c) for c in caps[:5]]
    assert (rows["row_pos"][5:] == 0).all()
    e.close()


def test_timestamp_mode_session(world):
    sd, clips, caps = world
    e = _engine(COMPUTE_BF16, sd)
    prompt, opts = _prompt(e, ts=True), _opts(e, ts=True)
    ref = _static(e, clips[:B], caps[:B], prompt, opts)
    ses = _session(e, clips[:B], caps[:B], prompt, opts)
    _same(ses, ref)
    assert any(t >= e.special.timestamp_begin for toks in ses[0] for t in toks)
    e.close()


@pytest.mark.parametrize("compute", [COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16], ids=["f32", "bf16", "f16"])
def test_encoder_output_does_not_depend_on_the_batch(world, compute):
    """The property the session rests on: a clip's encoder output at batch 3 equals its output at batch 32 (automatic dispatch,
    what a static batch of 32 gets).  f32: as it is.  16 bits: with the encoder GEMMs held to the 256 x 256 family (option
    enc_gemm = 3, what every session pass runs); the automatic dispatch at batch 3 takes gemm_bf16_v2 for some GEMMs and
    then differs in rounding only."""
    sd, clips, _ = world
    e = _engine(compute, sd)
    e.log_mel(clips[:B], want_output=False)
    wide = e.encode(B, want_output=True)
    e.log_mel(clips[:3], want_output=False)
    narrow = e.encode(3, want_output=True)
    if compute == COMPUTE_F32:
        assert np.array_equal(narrow, wide[:3])
    else:
        assert np.abs(narrow - wide[:3]).max() <= 0.02 * np.abs(wide[:3]).max()
        e.set_option("enc_gemm", 3)
        e.log_mel(clips[:3], want_output=False)
        fixed = e.encode(3, want_output=True)
        e.set_option("enc_gemm", 0)
        assert np.array_equal(fixed, wide[:3])
    e.close()


def test_refusals_leave_the_context_usable(world):
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    sd, clips, caps = world
    e = _engine(COMPUTE_BF16, sd)
    prompt, opts = _prompt(e), _opts(e)
    with pytest.raises(TtasrError):
        e.session(opts, len(prompt), temperature=0.5)
    e.set_option("xkv_fp8", 1)
    with pytest.raises(TtasrError):
        e.session(opts, len(prompt))
    e.set_option("xkv_fp8", 0)
    with e.session(opts, len(prompt)) as s:
        lib, h = e.lib, e.h
        pcm = np.ascontiguousarray(clips[0], dtype=np.float32)
        ptrs = (ctypes.c_void_p * 1)(pcm.ctypes.data)
        ns = np.asarray([len(pcm)], dtype=np.int64)
        pr = np.asarray([prompt], dtype=np.int32)
        pl = np.asarray([len(prompt)], dtype=np.int32)
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        for bad in (0, N_NEW + 1):                              # budgets outside [1, max_new_tokens], straight to the library
            cap = np.asarray([bad], dtype=np.int32)
            assert lib.ttasr_session_submit(h, 1, ptrs, ns.ctypes.data_as(i64p), pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p),
                                            cap.ctypes.data_as(i32p), None) == -1
        long_ns = np.asarray([30 * 16000 + 1], dtype=np.int64)   # longer than one window
        cap = np.asarray([8], dtype=np.int32)
        assert lib.ttasr_session_submit(h, 1, ptrs, long_ns.ctypes.data_as(i64p), pr.ctypes.data_as(i32p), pl.ctypes.data_as(i32p),
                                        cap.ctypes.data_as(i32p), None) == -1
        with pytest.raises(TtasrError):                          # every other search / encode call waits for the session's end
            e.generate([prompt], opts)
        with pytest.raises(TtasrError):
            e.encode(1)
        with pytest.raises(TtasrError):
            e.decode_step([prompt[0]])
        with pytest.raises(TtasrError):
            e.align(0, prompt + [1, 2], [(0, 0)])
        assert s.submit(clips[:2], [prompt] * 2, caps[:2]) == [0, 1]   # the refused calls changed nothing
        assert len(s.drain()) == 2
    # after the session a static generate returns what a fresh engine returns
    e.log_mel(clips[:B], want_output=False)
    e.encode(B)
    got = e.generate([prompt] * B, opts, row_max_new=caps[:B])
    f = _engine(COMPUTE_BF16, sd)
    f.log_mel(clips[:B], want_output=False)
    f.encode(B)
    want = f.generate([prompt] * B, opts, row_max_new=caps[:B])
    assert got.tokens == want.tokens and np.array_equal(got.sum_logprob, want.sum_logprob)
    f.close()
    e.close()


def test_transcribe_stream_is_transcribe_batch_for_full_batches():
    """WhisperModel.transcribe_stream keeps transcribe_batch's contract (token ids per clip, input order) for any number of
    clips; with full static batches and prompts forced through decode steps the two give the same tokens (natural EOT here)."""
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=8)
    n = m.n_window
    clips = [(synth.noise_clip, synth.tonal_clip, synth.burst_clip)[i % 3](500 + i, n - 977 * i) for i in range(24)]
    m.engine.set_option("prefill", 0)
    want = m.transcribe_batch(clips, max_new_tokens=48)
    m.engine.set_option("prefill", 1)
    got = m.transcribe_stream(clips, max_new_tokens=48)
    assert got == want
    short = m.transcribe_stream(clips[:3], max_new_tokens=48, row_max_new=[1, 5, 48])
    assert [len(t) <= c for t, c in zip(short, (1, 5, 48))] == [True] * 3
    assert short[2] == want[2]
    assert m.transcribe_stream([]) == []
