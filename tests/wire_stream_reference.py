"""A wire stream (include/ttasr.h, "wire streams") restated in numpy: ONE recording that arrives as bytes in pieces and leaves as
float32 mono 16 kHz, with the pending bytes, the mono history and K(F) written out.  Built on tests/ingest_reference.py (the
conversion, the filter design, the plain float32 sum) and tests/telephony_reference.py (the two G.711 laws); it shares no code
with the package.

The three keyword switches of `Stream` plant the bugs the case list is there to catch (history dropped at a cut, history short by
`short_history` frames, K(F) off by one); the defaults are the definition.  A history one frame short loses frame F - H.  Where up
divides 2 half that frame only ever meets the tap h[2 half], the sinc's zero, and no float32 bit can show its loss; at 44100 (up
160, 2 half = 8820, H = 55) it meets the taps 8800 ... 8820 at the cuts `exposing_cut` finds, and `fixed_cuts` carries one."""
import numpy as np

import ingest_reference as ref
import telephony_reference as tel

U8, S16, S24, S32, F32, F64 = range(6)
ALAW, ULAW, IMA4 = tel.ALAW, tel.ULAW, tel.IMA4

# (rate, format, channels, pick, frames): 0.3 - 1.2 s each - several output tiles (256 ... 1024 outputs) and several VAD frames
CASES = (
    (8000, ULAW, 1, -1, 4807),      # telephony: one party
    (8000, ALAW, 2, 1, 4099),       # ... one party per channel, the second picked
    (8000, S16, 2, -1, 3001),       # the mean of two channels
    (48000, S16, 1, -1, 14407),     # up == 1
    (44100, S24, 2, 0, 13231),      # 6-byte frames of 3-byte samples: cuts inside a sample
    (11025, F32, 1, -1, 3313),      # up = 640
    (16000, S16, 3, -1, 5003),      # no filter, 6-byte frames
    (192000, U8, 1, -1, 57607),     # H = 240
)


def sample_bytes(fmt):
    return 1 if fmt in (ALAW, ULAW) else ref.BYTES[fmt]


def plan(rate):
    """(up, down, half, H) of a stream rate; half = 0 and H = 0 at 16000 (no filter)."""
    up, down, _, half, _ = ref.ratio(rate)
    if rate == ref.TARGET:
        half = 0
    return up, down, half, 2 * half // up


def stream_rate(rate):
    return ref.accepted(rate) and plan(rate)[3] <= 255


def final(rate, n_frames, finished=False, shift=0):
    """K(F) = max(0, ceil((F up - half) / down)); finished: n_out(F) = ceil(F up / down)."""
    up, down, half, _ = plan(rate)
    if finished:
        return -(-n_frames * up // down)
    return max(0, -(-(n_frames * up - half) // down) + shift)


def final_brute(rate, n_frames):
    """K(F) counted: the outputs from 0 on whose every tap inside [0, 2 half] sits on a frame below F."""
    if rate == ref.TARGET:
        return n_frames
    up, down = plan(rate)[:2]
    k_hi = n_frames * up // down + 2
    t, i, ok = ref._index(rate, 1 << 60, 0, k_hi)
    last = np.where(ok, i, -1).max(axis=1)          # the last frame output k reads
    done = last < n_frames
    return int(k_hi if done.all() else np.argmin(done))


def mono_equivalent(raw, fmt, channels, pick):
    """(raw', fmt', channels') of a PCM recording that ttasr_ingest_pcm turns into the same mono: G.711 decoded to int16, a
    picked channel taken out as a mono recording."""
    raw = bytes(raw)
    if fmt in (ALAW, ULAW):
        x = tel.g711_decode(raw, fmt, channels)
        if pick >= 0:
            x, channels = x[:, pick:pick + 1], 1
        return np.ascontiguousarray(x).astype("<i2").tobytes(), S16, channels
    if pick >= 0 and channels > 1:
        w = ref.BYTES[fmt]
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, channels, w)
        return np.ascontiguousarray(b[:, pick, :]).tobytes(), fmt, 1
    return raw, fmt, channels


def mono(raw, fmt, channels, pick):
    return ref.host_convert(*mono_equivalent(raw, fmt, channels, pick))


def offline(rate, raw, fmt, channels, pick=-1):
    """The whole recording at once: ingest_reference.emulate_f32, or the converted samples at 16000."""
    fb = sample_bytes(fmt) * channels
    raw = bytes(raw)[:len(raw) // fb * fb]
    if rate == ref.TARGET:
        return mono(raw, fmt, channels, pick)
    return ref.emulate_f32(rate, *mono_equivalent(raw, fmt, channels, pick))


class Stream:
    def __init__(self, rate, channels, fmt, pick=-1, drop_history=False, short_history=0, k_shift=0):
        assert stream_rate(rate) and fmt != IMA4
        self.rate, self.channels, self.fmt, self.pick = rate, channels, fmt, pick
        self.up, self.down, self.half, self.H = plan(rate)
        self.fb = sample_bytes(fmt) * channels
        self.taps = ref.design(rate).astype(np.float32) if rate != ref.TARGET else None
        self.drop_history, self.short_history, self.k_shift = drop_history, short_history, k_shift
        self.reset()

    def reset(self):
        self.pending = b""
        self.hist = np.zeros(self.H, dtype=np.float32)      # mono[F - H .. F), zeros below frame 0
        self.F = self.K = 0

    def push(self, data, finish=False):
        """The float32 samples that become final."""
        buf = self.pending + bytes(data)
        whole = len(buf) // self.fb * self.fb
        new = mono(buf[:whole], self.fmt, self.channels, self.pick)
        self.pending = buf[whole:]
        F0, F1 = self.F, self.F + len(new)
        k_lo = self.K
        k_hi = final(self.rate, F1, True) if finish else max(final(self.rate, F1, shift=self.k_shift), k_lo)
        hist = np.zeros(self.H, dtype=np.float32) if self.drop_history and len(new) else self.hist
        keep = self.H - self.short_history
        local = np.concatenate([hist, new])                 # frame i at local[i - (F0 - H)]
        if self.taps is None:
            out = local[k_lo - (F0 - self.H):k_hi - (F0 - self.H)].copy()
        else:
            t, i, ok = ref._index(self.rate, F1, k_lo, k_hi)
            at = i - (F0 - self.H)
            seen = ok & (at >= self.H - keep if F0 else at >= 0)
            x = np.where(seen, local[np.clip(at, 0, len(local) - 1)], np.float32(0)).astype(np.float32)   # H >= 20: never empty
            out = np.zeros(k_hi - k_lo, dtype=np.float32)
            for c in range(t.shape[1]):
                out = np.where(ok[:, c], (out + (x[:, c] * self.taps[t[:, c]]).astype(np.float32)).astype(np.float32), out)
        self.hist = local[len(local) - self.H:] if self.H else local[:0]
        self.F, self.K = F1, k_hi
        if finish:
            self.reset()
        return out


def oldest_frame_slack(rate):
    """2 half - H up: how far the tap that frame F - H meets may lie below 2 half.  0 where up divides 2 half (every upsampling
    rate and up == 1): frame F - H then only ever meets h[2 half], the sinc's zero (about 1e-18 in floating point), and its loss
    changes no float32 bit.  Above 0 (44100: 20) the frame meets real taps at some cuts - see exposing_cut."""
    up, _, half, H = plan(rate)
    return 2 * half - H * up


def exposing_cut(rate, after):
    """The first frame count F > after at which the first non-final output, k = K(F), reads frame F - H: its tap index there is
    2 half - slack + d with d = K(F) down - (F up - half), which is a tap of the filter when d <= slack.  None where slack is 0."""
    up, down, half, _ = plan(rate)
    slack = oldest_frame_slack(rate)
    if slack == 0:
        return None
    F = after + 1
    while final(rate, F) * down - (F * up - half) > slack or final(rate, F) == 0:
        F += 1
    return F


def fixed_cuts(rate, channels, fmt, n_bytes):
    """Piece sizes in bytes: 0, 1, a frame less one byte, H - 1, H and H + 1 frames, where the rate has one a piece that ends on
    an exposing cut (exposing_cut: the next push reads the oldest history frame through a real tap), the rest."""
    fb, H = sample_bytes(fmt) * channels, plan(rate)[3]
    cuts = [0, 1, fb - 1, max(H - 1, 0) * fb, H * fb, (H + 1) * fb]
    F = exposing_cut(rate, sum(cuts) // fb)
    if F is not None:
        cuts.append(F * fb - sum(cuts))
    left = n_bytes - sum(cuts)
    assert left > 0
    return cuts + [left]


def random_cuts(n_bytes, seed, pieces=7):
    rng = np.random.default_rng([0x57AEA3, seed, n_bytes])
    at = np.sort(rng.integers(0, n_bytes + 1, size=pieces - 1))
    return [int(v) for v in np.diff(np.concatenate([[0], at, [n_bytes]]))]


def recording(rate, fmt, channels, frames, seed=0):
    if fmt in (ALAW, ULAW):
        return tel.random_bytes(frames * channels, [0xC0DEC, seed, rate, fmt])
    return ref.signal(rate, frames, channels, fmt, seed)


def feed(stream, raw, cuts, finish=True):
    out, pos = [], 0
    for j, k in enumerate(cuts):
        out.append(stream.push(raw[pos:pos + k], finish and j == len(cuts) - 1))
        pos += k
    assert pos == len(raw)
    return np.concatenate(out)
