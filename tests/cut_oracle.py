"""TEST infrastructure: tests/oracle_engine.py's engine with the cut form of the window feature call
(Engine.log_mel_windows(n_frames=...)): window b is pad_or_trim(features[:, seek:seek + n_frames[b]]) of the oracle's whole-file
features.  tests/test_clip_timestamps_host.py holds it to a reference written there; tests/test_gpu_clip_options.py drives the
window loop with it beside the HIP engine.  Never imported by the product."""
from oracle_engine import OracleEngine


class CutOracle(OracleEngine):
    def log_mel_windows(self, audio, seeks, floor_max=None, want_output=False, want_max=False, n_frames=None):
        out = super().log_mel_windows(audio, seeks, floor_max, want_output, want_max)
        if n_frames is not None:
            assert len(n_frames) == len(seeks) and min(n_frames) >= 1
            for b, n in enumerate(n_frames):
                self.mel[b, :, int(n):] = 0.0          # the frames behind the cut: 0 in feature space
        return out
