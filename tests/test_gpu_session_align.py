"""GPU: word alignment inside a continuous-batching session (`ttasr_session_hold / _align / _release`) and the facade on top of
it and of `ttasr_align_batch` (`transcribe_windows`, `transcribe_stream`, `BatchedWhisperASR` with word_timestamps=True)."""
import asyncio
import ctypes as C
import warnings

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F32, PRESETS

pytestmark = pytest.mark.gpu

HEADS = [(3, 0), (3, 5), (2, 1), (1, 4)]


def _pool(n):
    makers = (synth.noise_clip, synth.tonal_clip, synth.burst_clip)
    return [makers[i % 3](i)[: (4 + i % 5) * 16000] for i in range(n)]


def _engine(compute, max_batch):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    pd = PRESETS["tiny"]
    e = Engine(pd, compute, max_batch)
    e.load_weights(synth.iter_weights(pd))
    return e


def _seq(st, toks):
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps] + [t for t in toks if t < st.eot] + [st.eot]


def _run_session(e, clips, caps, beam, hold):
    """-> {clip index: (tokens, sum_logprob, no_speech)}, and with hold the start frames / log-probs of every aligned clip."""
    st = e.special
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(24, timestamps=False, sot_index=0)
    res, aligned = {}, {}
    with (e.session(opts, len(prompt), beam=beam) if beam > 1 else e.session(opts, len(prompt))) as s:
        if hold:
            s.hold()
        ids = s.submit(clips, [prompt] * len(clips), caps)
        where = {cid: i for i, cid in enumerate(ids)}
        while s.pending > 0:
            got = s.poll()
            assert got
            for r in got:
                res[where[r.id]] = (r.tokens, r.sum_logprob, r.no_speech_prob)
            if hold:
                a = s.align([r.id for r in got], [_seq(st, r.tokens) for r in got], [3] * len(got),
                            [len(clips[where[r.id]]) // 160 for r in got], HEADS)
                for k, r in enumerate(got):
                    aligned[where[r.id]] = (a.start_frames[k], a.logprobs[k])
    return res, aligned


@pytest.mark.parametrize("compute", [COMPUTE_F32, COMPUTE_BF16])
@pytest.mark.parametrize("beam", [1, 2])
def test_hold_changes_no_live_row(compute, beam):
    """6. 3x as many clips as groups, seeded budgets, hold on and Session.align after every poll: tokens, sum_logprob and
    no_speech of every clip bit-identical to the same session with hold off."""
    e = _engine(compute, 4)
    groups = 4 // beam
    clips = _pool(3 * groups + 1)
    caps = np.random.default_rng(17).integers(3, 24, size=len(clips)).tolist()
    plain, _ = _run_session(e, clips, caps, beam, hold=False)
    held, aligned = _run_session(e, clips, caps, beam, hold=True)
    assert sorted(plain) == sorted(held) == list(range(len(clips))) and sorted(aligned) == sorted(held)
    for i in plain:
        assert plain[i][0] == held[i][0], i
        assert np.float32(plain[i][1]).tobytes() == np.float32(held[i][1]).tobytes(), i
        assert np.float32(plain[i][2]).tobytes() == np.float32(held[i][2]).tobytes(), i
        n_text = len([t for t in held[i][0] if t < e.special.eot])
        assert len(aligned[i][0]) == n_text + 1 and len(aligned[i][1]) == n_text + 4
        assert np.all(np.diff(aligned[i][0]) >= 0) and np.all(np.isfinite(aligned[i][1]))
    e.close()


@pytest.mark.parametrize("compute", [COMPUTE_F32, COMPUTE_BF16])
@pytest.mark.parametrize("beam", [1, 2])
def test_session_alignment_equals_static_alignment(compute, beam):
    """7. the clips one poll returned together: start frames identical and log-probs bit-identical to ttasr_align_batch over
    the same sequences in the same order after a static pass of G clips with prefill = 0 (16-bit: enc_gemm = 3)."""
    e = _engine(compute, 4)
    st = e.special
    G = 4 // beam
    clips = _pool(G)
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(20, timestamps=False, sot_index=0)
    with (e.session(opts, len(prompt), beam=beam) if beam > 1 else e.session(opts, len(prompt))) as s:
        s.hold()
        ids = s.submit(clips, [prompt] * G, [9] * G)           # equal budgets: the clips finish in the same poll
        got = []
        while s.pending > 0:
            got += s.poll()
        assert len(got) == G
        rows = s.rows()
        unit = {int(rows["clip"][g * max(beam, 1)]): g for g in range(G)}
        seqs = [_seq(st, r.tokens) for r in got]
        frames = [len(clips[ids.index(r.id)]) // 160 for r in got]
        a = s.align([r.id for r in got], seqs, [3] * G, frames, HEADS, debug=True)
    e.set_option("prefill", 0)
    if compute != COMPUTE_F32:
        e.set_option("enc_gemm", 3)
    # static slot of a clip = the unit it held in the session
    static = [None] * G
    for r in got:
        static[unit[r.id]] = clips[ids.index(r.id)]
    e.log_mel(static, want_output=False)
    e.encode(G)
    b = e.align_batch([unit[r.id] for r in got], seqs, [3] * G, frames, HEADS, debug=True)
    for k in range(G):
        np.testing.assert_array_equal(a.start_frames[k], b.start_frames[k])
        assert a.logprobs[k].tobytes() == b.logprobs[k].tobytes(), k
        assert a.costs[k].tobytes() == b.costs[k].tobytes(), k
    e.close()


@pytest.mark.parametrize("beam", [1, 2])
def test_units_are_held_and_released(beam):
    """8. a held clip's id stays on its rows until align or release; with every unit held and clips queued a poll returns nothing
    with stats['queued'] > 0, after release the queue drains; refusals change nothing; session_end with held clips succeeds."""
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    e = _engine(COMPUTE_F32, 4)
    st = e.special
    G = 4 // beam
    clips = _pool(2 * G + 1)
    prompt = [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]
    opts = e.gen_opts(12, timestamps=False, sot_index=0)
    e.set_option("refill_overlap", 1)
    with (e.session(opts, len(prompt), beam=beam) if beam > 1 else e.session(opts, len(prompt))) as s:
        with pytest.raises(TtasrError):
            s.hold()                                       # the pass would race the overlapped encode: refused
    e.set_option("refill_overlap", 0)
    with (e.session(opts, len(prompt), beam=beam) if beam > 1 else e.session(opts, len(prompt))) as s:
        with pytest.raises(ValueError):
            s.release([0])                                 # hold off (checked in Python)
        assert e.lib.ttasr_session_release(e.h, 1, np.zeros(1, np.int64).ctypes.data_as(C.POINTER(C.c_int64))) == -1
        s.hold()
        ids = s.submit(clips, [prompt] * len(clips), [6] * len(clips))
        got = []
        while len(got) < G:
            got += s.poll()
        held = [r.id for r in got]
        rows = s.rows()
        assert sorted(set(int(c) for c in rows["clip"][: G * beam])) == sorted(held) and np.all(rows["done"] == 1)
        assert s.poll() == [] and s.stats()["queued"] > 0   # nothing can start: every unit is held
        with pytest.raises(TtasrError):
            s.release([ids[-1]])                           # queued, not held
        with pytest.raises(TtasrError):
            s.align([12345], [_seq(st, [400])], [3], [3000], HEADS)
        with pytest.raises(ValueError):
            s.release([held[0], held[0]])
        assert sorted(set(int(c) for c in s.rows()["clip"][: G * beam])) == sorted(held)
        s.release(held[:1])
        assert held[0] not in set(int(c) for c in s.rows()["clip"])
        a = s.align(held[1:], [_seq(st, r.tokens) for r in got[1:]], [3] * (G - 1), [3000] * (G - 1), HEADS) if G > 1 else None
        assert a is None or len(a.start_frames) == G - 1
        assert all(int(c) not in held for c in s.rows()["clip"])
        rest = []
        while len(rest) < G:
            rest += s.poll()
        assert all(r.id not in held for r in rest)
        s.release([r.id for r in rest])
        last = []
        while s.pending > 0:
            last += s.poll()
        assert len(last) == 1                               # left held: session_end releases it
    e.log_mel(clips[:2], want_output=False)
    e.encode(2)
    assert len(e.generate([prompt[:3]] * 2, e.gen_opts(4, True)).tokens) == 2
    e.close()


def _check_words(words, text, seconds):
    assert "".join(w["word"] for w in words) == text
    starts = [w["start"] for w in words]
    assert starts == sorted(starts)
    assert all(0.0 <= w["start"] <= w["end"] <= seconds + 1e-6 for w in words)
    assert all(0.0 <= w["probability"] <= 1.0 for w in words)


@pytest.mark.parametrize("beam", [1, 2])
def test_facade_words(beam):
    """9. transcribe_windows and transcribe_stream with word_timestamps=True: words monotone, inside the clip, joining to the
    text; text and tokens identical to the same call without words."""
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:tiny", device="cuda", compute_type="float32", max_batch=4)
    clips = _pool(5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = m.transcribe_windows(clips, beam_size=beam, max_new_tokens=20)
        full = m.transcribe_windows(clips, beam_size=beam, max_new_tokens=20, word_timestamps=True)
        short = m.transcribe_windows(clips[:2], beam_size=beam, max_new_tokens=20, word_timestamps=True, audio_ctx="auto")
        toks = m.transcribe_stream(clips, beam_size=beam, max_new_tokens=20)
        both = m.transcribe_stream(clips, beam_size=beam, max_new_tokens=20, word_timestamps=True)
    assert [(t, e) for t, e, _ in full] == plain and any(w for _, _, w in full)
    for c, (text, _, words) in zip(clips, full):
        _check_words(words, text, len(c) / 16000.0)
    for c, (text, _, words) in zip(clips, short):
        _check_words(words, text, len(c) / 16000.0)
    assert [t for t, _ in both] == toks
    for c, (t, words) in zip(clips, both):
        _check_words(words, m.tokenizer.decode([x for x in t if x < m.special.eot]), len(c) / 16000.0)
    m.engine.close()


class _Client:
    def __init__(self, audio, last_start):
        self.scratch_buffer = (np.clip(audio, -1, 1) * 32767).astype(np.int16).tobytes()
        self.last_start_time = last_start


@pytest.mark.parametrize("continuous", [False, True])
def test_streaming_backend_words(continuous):
    """9. BatchedWhisperASR(word_timestamps=True): non-empty words offset by last_start_time, duration = the last word's end;
    with the flag off "words" == []."""
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    clips = _pool(3)

    async def run(asr):
        try:
            return await asyncio.gather(*[asr.transcribe(_Client(c, 100.0 * (i + 1))) for i, c in enumerate(clips)])
        finally:
            await asr.aclose()

    kw = dict(model_path="synthetic:tiny", compute_type="float32", beam_size=2, max_clips=3, max_new_tokens=16, max_wait_ms=3000.0,
              continuous=continuous)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        on = asyncio.run(run(BatchedWhisperASR(word_timestamps=True, **kw)))
        off = asyncio.run(run(BatchedWhisperASR(**kw)))
    assert any(r is not None for r in on)
    for i, (a, b) in enumerate(zip(on, off)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a["text"] == b["text"] and b["words"] == [] and len(a["words"]) > 0
        assert set(a["words"][0]) == {"word", "start", "end", "probability"}
        base = 100.0 * (i + 1)
        assert all(base <= w["start"] <= w["end"] <= base + 30.0 for w in a["words"])
        assert abs(a["duration"] - (a["words"][-1]["end"] - base)) < 1e-9
