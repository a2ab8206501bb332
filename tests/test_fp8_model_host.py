"""Host surface of the e4m3 cross-KV mode (no GPU): `WhisperModel(cross_kv_fp8=True)` sets engine option xkv_fp8 = 2 on lane 0
before anything is encoded and on every lane `_lane()` creates later, refuses the float32 compute type, and `batch_cli` has
the `--xkv-fp8` switch."""
import pytest

from taiwan_tongues_asr_ce_amd import batch_cli
from taiwan_tongues_asr_ce_amd.config import SpecialTokens


class _Engine:
    """Engine double: records the calls a WhisperModel makes on an engine context, in order."""
    made = []

    def __init__(self, dims, compute_type, max_batch, device=0, share_weights_with=None):
        self.calls = []
        self.owner = share_weights_with
        self.special = SpecialTokens.for_vocab(dims.vocab)
        _Engine.made.append(self)

    def load_weights(self, tensors):
        self.calls.append(("load_weights",))

    def set_option(self, key, value):
        self.calls.append(("set_option", key, value))

    def encode(self, B, want_output=False):
        self.calls.append(("encode", B))

    def close(self):
        self.calls.append(("close",))


@pytest.fixture(autouse=True)
def _fresh():
    _Engine.made = []


def _model(**kw):
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    return WhisperModel("synthetic:micro", compute_type=kw.pop("compute_type", "bfloat16"), max_batch=10, pipeline_depth=2,
                        _engine_factory=_Engine, **kw)


def test_flag_sets_mode_two_on_lane_zero_before_any_encode():
    m = _model(cross_kv_fp8=True)
    lane0, = _Engine.made
    assert m.cross_kv_fp8 is True
    assert lane0.calls == [("load_weights",), ("set_option", "xkv_fp8", 2)]
    m.close()


def test_flag_is_replayed_on_lanes_created_later():
    m = _model(cross_kv_fp8=True)
    lane1 = m._lane(1)
    assert lane1 is _Engine.made[1] and lane1.owner is _Engine.made[0]
    assert lane1.calls == [("set_option", "xkv_fp8", 2)]
    assert m._lane(1) is lane1 and lane1.calls == [("set_option", "xkv_fp8", 2)]      # set once per lane
    m.close()


def test_without_the_flag_no_option_is_set():
    m = _model()
    m._lane(1)
    assert m.cross_kv_fp8 is False
    assert all(c[0] != "set_option" for e in _Engine.made for c in e.calls)
    m.close()


@pytest.mark.parametrize("compute_type", ["float32", "fp32"])
def test_float32_model_refuses_the_flag(compute_type):
    with pytest.raises(ValueError, match="cross_kv_fp8"):
        _model(cross_kv_fp8=True, compute_type=compute_type)
    assert _Engine.made == []                                   # refused before an engine exists


def test_an_engine_without_options_ignores_the_flag():
    class _NoOptions:
        def __init__(self, dims, compute_type, max_batch, device=0):
            self.special = SpecialTokens.for_vocab(dims.vocab)

        def load_weights(self, tensors):
            pass

        def close(self):
            pass
    from taiwan_tongues_asr_ce_amd.model import WhisperModel
    m = WhisperModel("synthetic:micro", compute_type="bfloat16", max_batch=2, cross_kv_fp8=True, _engine_factory=_NoOptions)
    assert m.cross_kv_fp8 is True
    m.close()


def test_batch_cli_parser_accepts_the_switch():
    ap = batch_cli.build_parser()
    assert ap.parse_args(["folder"]).xkv_fp8 is False
    assert ap.parse_args(["folder", "--xkv-fp8"]).xkv_fp8 is True


def test_batch_cli_summary_names_the_cache_only_when_it_is_the_e4m3_copy(tmp_path, monkeypatch):
    import struct
    import wave
    monkeypatch.chdir(tmp_path)
    folder = tmp_path / "audio"
    folder.mkdir()
    with wave.open(str(folder / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(struct.pack("<1600h", *([0] * 1600)))

    class _Seg:
        text = "x"

    class _Model:
        def __init__(self, fp8):
            self.cross_kv_fp8 = fp8

        def transcribe(self, audio, **kw):
            return iter([_Seg()]), None
    off = batch_cli.process_audio_folder(str(folder), model=_Model(False), log=lambda *_: None)
    on = batch_cli.process_audio_folder(str(folder), model=_Model(True), log=lambda *_: None)
    assert "cross_kv_cache" not in off["summary"]
    assert on["summary"]["cross_kv_cache"] == "fp8_e4m3"
