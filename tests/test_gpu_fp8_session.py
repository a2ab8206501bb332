"""GPU: option xkv_fp8 = 2 in continuous-batching sessions.  A session encodes into its staging cross-KV and quantises each
admitted clip from staging slot j straight into its live slot (xkv_quant_slots_kernel); the block and its scales must be those a
static ttasr_encode builds, in the slot the rows read.  So, with the option at 2 on both sides, the sessions' contracts hold
unchanged: a greedy clip equals the same clip of a static ttasr_generate_capped pass of max_batch rows (prefill = 0), a beam clip
the same clip of ttasr_generate_beam over exactly G clips (prefill = 0, enc_gemm = 3), a sampled window slot 0 of a
ttasr_generate_sample pass - bit for bit.  A block or a scale written to the wrong slot breaks that.

Preset large-v3-w2 (20 heads, 2 + 2 layers), budgets <= 12 tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, PRESETS, SpecialTokens

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DIMS = PRESETS["large-v3-w2"]
BEAM = 5
HEADS = [(1, 0), (1, 5), (0, 1), (1, 4)]


def _clips(n, seed=300):
    kinds = (synth.noise_clip, synth.tonal_clip, synth.noise_clip, synth.burst_clip)
    return [kinds[i % 4](seed + i) for i in range(n)]


def _state(boost):
    sd = dict(synth.state_dict(DIMS))
    if boost:
        st = SpecialTokens.for_vocab(DIMS.vocab)
        e = sd["model.decoder.embed_tokens.weight"].copy()
        e[st.eot] *= boost
        sd["model.decoder.embed_tokens.weight"] = e
    return sd


@pytest.fixture(scope="module")
def plain():
    return _state(0.0)


@pytest.fixture(scope="module")
def boosted():
    return _state(5.0)


def _engine(sd, max_batch, fp8):
    from taiwan_tongues_asr_ce_amd.engine import Engine
    e = Engine(DIMS, COMPUTE_BF16, max_batch)
    e.load_weights(sd.items())
    if fp8:
        e.set_option("xkv_fp8", fp8)
    return e


def _prompt(e):
    st = e.special
    return [st.sot, st.lang_zh, st.transcribe, st.no_timestamps]


def _f32(v):
    return np.float32(v).tobytes()


def test_greedy_session_equals_the_static_mode2_pass(plain):
    """max_batch 16, 40 clips with budgets 2..12 (24 clips cannot refill 16 rows: 16 are first fills), drawn so that every row is
    refilled at least once; the clips behind the first 16 go into whichever rows end first, from staging slots (their order in
    the encoder pass that brought them) that are not those rows - both facts are asserted from ttasr_session_rows."""
    B, N = 16, 40
    clips = _clips(N)
    caps = np.random.Generator(np.random.Philox(key=21)).integers(2, 13, size=N).astype(np.int32)
    assert caps.min() == 2 and caps.max() == 12
    e = _engine(plain, B, 2)
    try:
        prompt = _prompt(e)
        opts = e.gen_opts(12, False, suppress_eot=True, check_interval=2)

        def session(watch=False):
            held = [[] for _ in range(B)]                       # the clip ids every row has held, in order
            moved = 0                                           # refilled clips whose row is not their staging slot
            with e.session(opts, len(prompt)) as s:
                ids = s.submit(clips, [prompt] * N, caps)
                got = {}
                while s.pending > 0:
                    for r in s.poll(max_steps=2 if watch else 1 << 30):
                        got[r.id] = r
                    if watch:
                        new = {}
                        for row, cid in enumerate(s.rows()["clip"].tolist()):
                            if cid >= 0 and (not held[row] or held[row][-1] != cid):
                                held[row].append(cid)
                                new[cid] = row
                        # clips are encoded and admitted in submission order: a pass's staging slots are the ranks of its ids
                        if min(new, default=0) >= B:
                            moved += sum(row != j for j, (cid, row) in enumerate(sorted(new.items())))
                assert s.stats()["encodes"] >= 2
            if watch:
                assert all(len(h) >= 2 for h in held), [len(h) for h in held]      # every row was refilled
                assert moved > 0                                                  # live slot != staging slot was exercised
            return [got[i] for i in ids]
        ses = session(watch=True)
        # static passes of exactly 16 rows (the second padded with the first clips), prompts forced through decode steps
        pad = list(range(N)) + list(range(-N % B))
        e.set_option("prefill", 0)
        static = []
        for i in range(0, len(pad), B):
            idx = pad[i:i + B]
            e.log_mel([clips[j] for j in idx], want_output=False)
            e.encode(B)
            r = e.generate([prompt] * B, opts, row_max_new=caps[idx])
            static += [(r.tokens[k], r.sum_logprob[k], r.no_speech_prob[k]) for k in range(B)]
        e.set_option("prefill", 1)
        for i in range(N):
            assert len(ses[i].tokens) == caps[i]
            assert ses[i].tokens == static[i][0], i
            assert _f32(ses[i].sum_logprob) == _f32(static[i][1]) and _f32(ses[i].no_speech_prob) == _f32(static[i][2]), i
        e.set_option("xkv_fp8", 0)
        ses16 = session()
        assert any(_f32(a.sum_logprob) != _f32(b.sum_logprob) for a, b in zip(ses, ses16)), "the session did not read the e4m3 copy"
    finally:
        e.close()


def _beam_static(e, clips, prompts, opts, G):
    e.set_option("prefill", 0)
    e.set_option("enc_gemm", 3)
    out = []
    try:
        for i in range(0, len(clips), G):
            e.log_mel(clips[i:i + G], want_output=False)
            e.encode(G)
            r = e.generate_beam(prompts[i:i + G], BEAM, opts)
            out += [(r.tokens[k], r.sum_logprob[k], r.no_speech_prob[k]) for k in range(G)]
    finally:
        e.set_option("prefill", 1)
        e.set_option("enc_gemm", 0)
    return out


def test_beam_session_and_a_sampled_window_equal_their_static_passes(boosted):
    """max_batch 30, beam 5 (G = 6), 10 clips: four groups are refilled.  One window clip of a 40-s file decoded as 5 sampled rows."""
    B, G, N = 30, 6, 10
    clips = _clips(N, seed=900)
    file = np.concatenate([synth.tonal_clip(950), synth.noise_clip(951)[:160000]]).astype(np.float32)
    e = _engine(boosted, B, 2)
    try:
        prompt = _prompt(e)
        opts = e.gen_opts(12, False, sot_index=0)
        _, mx = e.log_mel_windows(file, [0, 3000], want_max=True)
        floor = float(np.max(mx))
        with e.session(opts, len(prompt), beam=BEAM) as s:
            ids = s.submit(clips, [prompt] * N)
            wid, = s.submit_windows([file], [3000], [prompt], [0], floor_max=[floor], temperature=[0.4], rows=[BEAM], seed=[77])
            got = {r.id: r for r in s.drain()}
            assert s.stats()["encodes"] >= 2
        pad = clips + clips[:2 * G - N]
        static = _beam_static(e, pad, [prompt] * len(pad), opts, G)
        lens = set()
        for i in range(N):
            r = got[ids[i]]
            lens.add(len(r.tokens))
            assert r.tokens == static[i][0], i
            assert _f32(r.sum_logprob) == _f32(static[i][1]) and _f32(r.no_speech_prob) == _f32(static[i][2]), i
        assert len(lens) > 1, lens                               # groups ended at different positions: mid-flight hand-overs
        e.set_option("prefill", 0)
        e.set_option("enc_gemm", 3)
        e.log_mel_windows([file] * G, [3000] * G, floor_max=[floor] * G)
        e.encode(G)
        r = e.generate_sample([prompt] * G, BEAM, opts, 0.4, seed=77)
        w = got[wid]
        assert w.tokens == r.tokens[0]
        assert _f32(w.sum_logprob) == _f32(r.sum_logprob[0]) and _f32(w.no_speech_prob) == _f32(r.no_speech_prob[0])
    finally:
        e.close()


def test_hold_and_align_do_not_depend_on_the_mode(boosted):
    """Alignment reads the 16-bit block of the held clip's live slot: the same start frames, log-probabilities and cost matrices
    as an option-0 session aligning the same token sequences."""
    B, G = 30, 6
    clips = [c[: (8 + 3 * i) * 16000] for i, c in enumerate(_clips(G, seed=1100))]
    frames = [len(c) // 160 for c in clips]

    def run(mode, seqs):
        e = _engine(boosted, B, mode)
        try:
            st = e.special
            prompt = _prompt(e)
            opts = e.gen_opts(9, False, sot_index=0, suppress_eot=True)
            with e.session(opts, len(prompt), beam=BEAM) as s:
                s.hold()
                ids = s.submit(clips, [prompt] * G)
                got = {r.id: r for r in s.drain()}
                if seqs is None:
                    seqs = [prompt + [t for t in got[i].tokens if t < st.eot] + [st.eot] for i in ids]
                a = s.align(ids, seqs, [3] * G, frames, HEADS, debug=True)
            return seqs, a
        finally:
            e.close()
    seqs, a8 = run(2, None)
    _, a16 = run(0, seqs)
    for k in range(G):
        np.testing.assert_array_equal(a8.start_frames[k], a16.start_frames[k])
        assert a8.logprobs[k].tobytes() == a16.logprobs[k].tobytes(), k
        assert a8.costs[k].tobytes() == a16.costs[k].tobytes(), k


def test_refusals_and_the_end_of_a_session(plain):
    from taiwan_tongues_asr_ce_amd import _lib
    from taiwan_tongues_asr_ce_amd.engine import TtasrError
    B = 16
    clips = _clips(B, seed=1300)
    e = _engine(plain, B, 1)
    fresh = _engine(plain, B, 2)
    try:
        lib = _lib.load()
        prompt = _prompt(e)
        opts = e.gen_opts(6, False, suppress_eot=True)
        # mode 1 is still refused by both begin calls, and the context stays usable
        assert lib.ttasr_session_begin(e.h, C.byref(opts), len(prompt), C.c_float(0.0)) != 0
        assert lib.ttasr_session_begin_beam(e.h, C.byref(opts), len(prompt), BEAM, C.c_float(1.0)) != 0
        e.set_option("xkv_fp8", 2)
        e.log_mel(clips, want_output=False)
        e.encode(B)
        before = e.generate([prompt] * B, opts)
        with e.session(opts, len(prompt)) as s:
            s.submit(clips[:3], [prompt] * 3)
            assert len(s.drain()) == 3
        # the session leaves no resident encoder state, the e4m3 copy included
        with pytest.raises(TtasrError):
            e.generate([prompt] * B, opts)
        e.log_mel(clips, want_output=False)
        e.encode(B)
        after = e.generate([prompt] * B, opts)
        fresh.log_mel(clips, want_output=False)
        fresh.encode(B)
        ref = fresh.generate([prompt] * B, opts)
        for r in (before, after):
            assert r.tokens == ref.tokens and np.array_equal(r.sum_logprob, ref.sum_logprob)
            assert np.array_equal(r.no_speech_prob, ref.no_speech_prob)
    finally:
        e.close(); fresh.close()
