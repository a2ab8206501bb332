"""MI355X-native Whisper inference hot path behind the reference's WhisperModel.transcribe surface."""
from .config import PRESETS, WhisperDims, DecodeOptions, SpecialTokens, COMPUTE_F32, COMPUTE_BF16, COMPUTE_F16  # noqa: F401


def __getattr__(name):
    # BatchedInferencePipeline lives in .batched, which imports the model layer: loaded on first use, so that importing the
    # package stays as light as before
    if name == "BatchedInferencePipeline":
        from .batched import BatchedInferencePipeline
        return BatchedInferencePipeline
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
