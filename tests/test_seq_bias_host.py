"""Host: keyword biasing above the library (taiwan_tongues_asr_ce_amd/seq_bias.py and the surfaces that take sequence_bias /
prompt_words) - the table's checks and grouped layout, the prompt_words expansion, the refusal on every continuous surface
before a session opens, the table cleared when a call ends (on exceptions too) and installed on every lane of a pipelined
run.  No GPU: the engines are the scripted doubles of tests/window_loop_stub.py with a recording set_sequence_bias."""
import math
import threading

import numpy as np
import pytest

import seq_bias_cases as S
import window_loop_stub as stub
from taiwan_tongues_asr_ce_amd import batch_cli, seq_bias

V = stub.DIMS.vocab


class BiasEngine(stub.ScriptEngine):
    """records every set_sequence_bias with the thread that made it; lanes are made with share_weights_with"""
    log = []          # (engine id, table or None, thread name): shared by the lanes of one test
    opened = []       # sessions asked for

    def __init__(self, dims, compute_type=0, max_batch=1, device=0, share_weights_with=None):
        super().__init__(dims, compute_type, max_batch, device)
        self.installed = None

    def set_sequence_bias(self, mapping=None):
        self.installed = None if not mapping else list(mapping)
        BiasEngine.log.append((id(self), self.installed, threading.current_thread().name))

    def session(self, *a, **k):
        BiasEngine.opened.append((a, k))
        raise AssertionError("a session was opened")

    def _answer(self, prompts, sampled=False):
        self.calls.append(("bias", self.installed))
        return super()._answer(prompts, sampled)


@pytest.fixture
def model():
    BiasEngine.log, BiasEngine.opened = [], []
    m = stub.make_model(lambda n, seek, frames: dict(tokens=[stub.ts(0.0), 400, 401, stub.ts(2.0), stub.ST.eot], lp=-1.0), cls=BiasEngine)
    yield m
    m.close()


AUDIO = np.zeros(16000 * 3, np.float32)
TABLE = {(5, 9): 2.0, (9,): 1.0, (7, 5, 9): -1.0}


# ---- the table --------------------------------------------------------------------------------------------------------------
def test_check_table_keeps_order_and_flattens():
    t = seq_bias.check_table(TABLE, V)
    assert t == [((5, 9), 2.0), ((9,), 1.0), ((7, 5, 9), -1.0)]
    tokens, offsets, biases = seq_bias.flatten(t)
    assert tokens.tolist() == [5, 9, 9, 7, 5, 9] and offsets.tolist() == [0, 2, 3, 6] and biases.tolist() == [2.0, 1.0, -1.0]
    assert tokens.dtype == np.int32 and offsets.dtype == np.int32 and biases.dtype == np.float32


def test_grouping_is_stable():
    t = seq_bias.check_table([((1, 9), 1.0), ((2, 8), 2.0), ((3, 9), 3.0), ((8,), 4.0), ((4, 5, 9), 5.0), ((6, 8), 6.0)], V)
    g = seq_bias.group_table(t)
    assert g["groups"] == [(9, None, 0, 3), (8, 4.0, 3, 2)]          # groups in order of first appearance, entries contiguous
    assert g["entries"] == [(1.0, 1, 0), (3.0, 1, 1), (5.0, 2, 2), (2.0, 1, 4), (6.0, 1, 5)]   # table order inside a group
    assert g["prefix"] == [1, 3, 4, 5, 2, 6]
    # the grouped table gives the reference's sums: same cases, same answers
    for c in S.cases(64):
        gt = seq_bias.group_table(seq_bias.check_table(c.table, 64))
        raw = c.logits(64)
        got = raw.copy()
        for r, h in enumerate(c.histories()):
            if h is None:
                continue
            for tok, one, first, n in gt["groups"]:
                total, applies = np.float32(0), one is not None
                if applies:
                    total = np.float32(total + np.float32(one))
                for b, plen, off in gt["entries"][first:first + n]:
                    if len(h) >= plen + 1 and h[len(h) - plen:] == gt["prefix"][off:off + plen]:
                        total, applies = np.float32(total + np.float32(b)), True
                if applies:
                    got[r, tok] = np.float32(raw[r, tok] + total)
        S.same(got, S.reference(raw, c.histories(), c.table), raw, c.name)


@pytest.mark.parametrize("bad, word", [
    ({tuple(range(17)): 1.0}, "outside \\[1, 16\\]"), ({(): 1.0}, "outside \\[1, 16\\]"), ({(5,): math.nan}, "not finite"),
    ({(5,): math.inf}, "not finite"), ({(5,): 1e39}, "not finite"), ({(V,): 1.0}, "outside the vocabulary"),
    ({(-1, 3): 1.0}, "outside the vocabulary"), ([((5, 6), 1.0), ((5, 6), 2.0)], "listed twice"), ({(1.5,): 1.0}, "token ids"),
    ({"ab": 1.0}, "token ids"), ({(5,): "x"}, "not a number"),
    ({(g,): 1.0 for g in range(seq_bias.MAX_GROUPS + 1)}, "distinct last tokens"),
    ({(1 + i % 4000, 1 + i // 4000, 7): 1.0 for i in range(seq_bias.MAX_ENTRIES + 1)}, "longer than one token"),
])
def test_check_table_refuses(bad, word):
    with pytest.raises(ValueError, match=word):
        seq_bias.check_table(bad, V)


def test_caps_exactly_full_are_accepted():
    full = [((g,), 1.0) for g in range(seq_bias.MAX_GROUPS)] + [((1 + i % 4000, 1 + i // 4000, 7), 1.0) for i in range(seq_bias.MAX_ENTRIES)]
    assert len(seq_bias.check_table(full, V)) == seq_bias.MAX_GROUPS + seq_bias.MAX_ENTRIES
    assert len(seq_bias.check_table({tuple(range(16)): 1.0}, V)) == 1
    assert (seq_bias.MAX_LEN, seq_bias.WINDOW, seq_bias.MAX_GROUPS, seq_bias.MAX_ENTRIES) == (S.MAX_LEN, S.W, S.MAX_GROUPS, S.MAX_ENTRIES)


# ---- prompt_words -------------------------------------------------------------------------------------------------------------
def test_prompt_words_expansion():
    enc = {"ab": [10, 11, 12], " ab": [20, 11, 12], "c": [30], " c": [30], "d": [10, 11], " d": [40]}
    t = seq_bias.expand_prompt_words("ab, c,,d", 3.0, lambda s: enc[s])
    assert t == {(10,): 1.5, (10, 11): 3.0, (10, 11, 12): 3.0, (20,): 1.5, (20, 11): 3.0, (20, 11, 12): 3.0, (30,): 1.5, (40,): 1.5}
    assert seq_bias.split_prompt_words("王小明，台北、 高雄 ,") == ["王小明", "台北", "高雄"]
    assert seq_bias.split_prompt_words(["a ", "", "b"]) == ["a", "b"] and seq_bias.split_prompt_words(None) == []
    # a key that arises twice keeps the larger bias: (10,) from "x" at boost / 2 and (10, 11) from both
    enc2 = {"x": [10, 11], " x": [10, 11], "y": [10], " y": [10]}
    assert seq_bias.expand_prompt_words(["x", "y"], 2.0, lambda s: enc2[s]) == {(10,): 1.0, (10, 11): 2.0}
    # a tokenisation longer than 16 tokens contributes its first 16
    long = seq_bias.expand_prompt_words("z", 2.0, lambda s: list(range(1, 21)))
    assert max(len(k) for k in long) == 16 and len(long) == 16
    with pytest.raises(ValueError, match="finite"):
        seq_bias.expand_prompt_words("x", math.inf, lambda s: [1])


def test_resolve_merges_and_keeps_the_larger(model):
    enc = model.tokenizer.encode
    word = "台北"
    ids = tuple(enc(word))
    t = dict(seq_bias.resolve({ids[:1]: 5.0, (3, 4): 1.0}, word, None, enc, V))
    assert t[ids[:1]] == 5.0 and t[(3, 4)] == 1.0                     # the given bias is larger than boost / 2
    assert all(b == seq_bias.DEFAULT_BOOST for k, b in t.items() if len(k) > 1 and k != (3, 4))
    assert seq_bias.resolve(None, None, None, enc, V) is None and seq_bias.resolve({}, " , ", None, enc, V) is None
    assert seq_bias.DEFAULT_BOOST == 2.0


# ---- the surfaces ---------------------------------------------------------------------------------------------------------------
def test_transcribe_installs_while_segments_are_produced_and_clears(model):
    segs, _ = model.transcribe(AUDIO, language="zh", beam_size=1, temperature=0.0, sequence_bias=TABLE)
    assert BiasEngine.log == []
    assert [s.text for s in segs] != []
    eng = model.engine
    want = seq_bias.check_table(TABLE, V)
    assert [c[1] for c in eng.calls if c[0] == "bias"] == [want]          # the search ran with the table installed
    assert [t for _, t, _ in BiasEngine.log] == [want, None] and eng.installed is None


def test_prompt_words_are_tokenised_once_and_do_not_touch_the_prompt(model, monkeypatch):
    n = {"enc": 0}
    real = model.tokenizer.encode

    def counting(s, *a, **k):
        n["enc"] += 1
        return real(s, *a, **k)
    monkeypatch.setattr(model.tokenizer, "encode", counting)
    segs, _ = model.transcribe(np.zeros(16000 * 65, np.float32), language="zh", beam_size=1, temperature=0.0, prompt_words="台北,高雄",
                               prompt_word_boost=4.0, condition_on_previous_text=False)
    list(segs)
    assert n["enc"] == 4                                                   # two phrases, each with and without the space
    eng = model.engine
    assert len(eng.prompts()) == 3 and all(p == eng.prompts()[0][1] for _, p in eng.prompts())   # three windows, one plain prompt
    assert len([t for _, t, _ in BiasEngine.log if t]) == 1 and BiasEngine.log[-1][1] is None
    assert max(b for _, b in BiasEngine.log[0][1]) == 4.0


def test_table_is_cleared_when_the_call_raises(model):
    def boom(n, seek, frames):
        raise RuntimeError("search failed")
    model.engine.script = boom
    segs, _ = model.transcribe(AUDIO, language="zh", beam_size=1, temperature=0.0, sequence_bias=TABLE)
    with pytest.raises(RuntimeError, match="search failed"):
        list(segs)
    assert [t is None for _, t, _ in BiasEngine.log] == [False, True] and model.engine.installed is None
    BiasEngine.log = []
    with pytest.raises(RuntimeError, match="search failed"):
        model.transcribe_many([AUDIO], language="zh", beam_size=1, temperature=0.0, prompt_words="台北")
    assert [t is None for _, t, _ in BiasEngine.log] == [False, True] and model.engine.installed is None
    # a generator that is dropped half way clears too
    model.engine.script = lambda n, seek, frames: dict(tokens=[stub.ts(0.0), 400, stub.ts(2.0), 401, stub.ts(4.0), stub.ST.eot], lp=-1.0)
    BiasEngine.log = []
    segs, _ = model.transcribe(AUDIO, language="zh", beam_size=1, temperature=0.0, sequence_bias=TABLE)
    next(iter(segs))
    segs.close()
    assert model.engine.installed is None and BiasEngine.log[-1][1] is None


def test_a_refused_table_reaches_no_engine(model):
    with pytest.raises(ValueError, match="not finite"):
        model.transcribe(AUDIO, language="zh", sequence_bias={(5,): math.nan})
    with pytest.raises(ValueError, match="outside the vocabulary"):
        model.transcribe_many([AUDIO], language="zh", sequence_bias={(V,): 1.0})
    assert BiasEngine.log == [] and model.engine.calls == []


def test_continuous_surfaces_refuse_before_a_session_opens(model):
    for call in (lambda: model.transcribe_many([AUDIO], language="zh", continuous=True, prompt_words="台北"),
                 lambda: model.transcribe_many([AUDIO], language="zh", continuous=True, sequence_bias=TABLE),
                 lambda: model.transcribe_groups([[AUDIO]], continuous=True, language="zh", prompt_words="台北"),
                 lambda: model.transcribe_stream([AUDIO], prompt_words="台北"),
                 lambda: model.transcribe_stream([AUDIO], sequence_bias=TABLE),
                 lambda: model.transcribe_batched(AUDIO, prompt_words="台北"),
                 lambda: model.transcribe_batched(AUDIO, sequence_bias=TABLE)):
        with pytest.raises(ValueError, match="lock-step form"):
            call()
    assert BiasEngine.opened == [] and BiasEngine.log == [] and model.engine.calls == []
    from taiwan_tongues_asr_ce_amd.streaming import BatchedWhisperASR
    with pytest.raises(ValueError, match="lock-step form"):
        BatchedWhisperASR(continuous=True, prompt_words="台北", model_path="synthetic:tiny")
    with pytest.raises(ValueError, match="lock-step form"):
        batch_cli.process_audio_folder(".", continuous=True, prompt_words="台北", model=model)
    with pytest.raises(ValueError, match="lock-step form"):
        batch_cli.process_audio_folder(".", batched=True, prompt_words="台北", model=model)


def test_batch_cli_flags(tmp_path, capsys):
    assert batch_cli.main([str(tmp_path), "--prompt-words", "a,b", "--continuous"]) == 1
    assert "--prompt-words" in capsys.readouterr().out
    assert batch_cli.main([str(tmp_path), "--prompt-words", "a,b", "--batched"]) == 1
    assert batch_cli.main([str(tmp_path), "--prompt-word-boost", "3"]) == 1
    args = batch_cli.build_parser().parse_args([str(tmp_path), "--prompt-words", "王小明,台北", "--prompt-word-boost", "3.5"])
    assert args.prompt_words == "王小明,台北" and args.prompt_word_boost == 3.5


def test_every_lane_installs_the_table(model):
    model.pipeline_depth = 2
    groups = [[AUDIO], [AUDIO], [AUDIO], [AUDIO]]
    # both workers take a group: the first search of each waits until the other has one too
    both, met = threading.Barrier(2), set()

    def script(n, seek, frames):
        me = threading.current_thread().name
        if me not in met:
            met.add(me)
            both.wait(timeout=30)
        return dict(tokens=[stub.ts(0.0), 400, 401, stub.ts(2.0), stub.ST.eot], lp=-1.0)
    for i in range(2):
        model._lane(i).script = script
    out = model.transcribe_groups(groups, pipeline_depth=2, language="zh", beam_size=1, temperature=0.0, prompt_words="台北",
                                  prompt_word_boost=3.0)
    assert len(out) == 4 and all(len(o) == 1 for o in out)
    want = seq_bias.resolve(None, "台北", 3.0, model.tokenizer.encode, V)
    engines = {e for e, _, _ in BiasEngine.log}
    assert len(engines) == 2 == len(model._lanes)                            # both lanes installed it ...
    for lane in model._lanes:
        mine = [t for e, t, _ in BiasEngine.log if e == id(lane)]
        assert mine and mine[0::2] == [want] * (len(mine) // 2) and all(t is None for t in mine[1::2])   # ... and cleared it per group
        assert lane.installed is None
        assert all(c[1] == want for c in lane.calls if c[0] == "bias")        # every search of every lane ran with it
    threads = {th for _, _, th in BiasEngine.log}
    assert threads == {"ttasr-lane0", "ttasr-lane1"}


def test_asr_adapter_passes_prompt_words_to_transcribe_path(monkeypatch):
    from taiwan_tongues_asr_ce_amd.asr import MI355XWhisperASR
    a = MI355XWhisperASR.__new__(MI355XWhisperASR)
    seen = {}

    class Pipe:
        def transcribe(self, path, **kw):
            seen.update(kw)
            return [], None
    a.asr_pipeline, a.default_transcribe_kwargs, a.device_resample, a.batched, a.audio_channel = Pipe(), {}, False, False, None
    a.bias_options = {"prompt_words": "台北", "prompt_word_boost": 3.0}
    a.transcribe_path("x.wav")
    assert seen["prompt_words"] == "台北" and seen["prompt_word_boost"] == 3.0
    a.transcribe_path("x.wav", prompt_words="高雄")
    assert seen["prompt_words"] == "高雄"
