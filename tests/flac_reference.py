"""FLAC in plain Python, written from the stream definition of include/ttasr.h (RFC 9639): a reader and an INDEPENDENT writer, and
the case table that the host and GPU tests of the native decoder share.

The writer chooses everything a real encoder chooses - per subframe the kind, the predictor order, LPC precision / shift /
coefficients, the partition order, the Rice method, escape partitions (n = 0 included) and wasted bits; per frame the stereo code,
the blocksize (and the code that carries it) and the blocking strategy - and can write illegal content under valid CRCs (kind
"raw").  The reader decodes frame after frame (it finds a frame's end by decoding it, not by scanning for a CRC) and takes mutant
switches, one per classic mistake; tests/test_flac_reference_host.py holds the case table to killing every one of them.  Sample
arithmetic is exact Python integers: nothing wraps."""
import hashlib
import struct

import numpy as np

FLAC = 32                               # TTASR_PCM_FLAC
MUTANTS = ("zigzag_sign", "part0_full", "no_side_bit", "no_wasted_shift", "midside_lowbit", "lpc_logical_shift", "lpc_32bit",
           "bs_code_no_plus1", "crc16_reflected", "one_byte_number")
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BITS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
BS_CODES = dict([(192, 1)] + [(576 << k, 2 + k) for k in range(4)] + [(256 << k, 8 + k) for k in range(8)])


class FlacError(ValueError):
    pass


def crc8(data) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def _crc16_reflected(data) -> int:      # the mutant: polynomial 0xA001, LSB first
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ 0xA001 if c & 1 else c >> 1
    return ((c & 0xFF) << 8) | (c >> 8)


def left_justified(x: np.ndarray, bits: int) -> np.ndarray:
    """The integers of a `bits`-wide stream as the decoder stores them: int16 v << (16 - bits), or int32 v << (32 - bits)."""
    x = np.asarray(x, dtype=np.int64)
    return (x << (16 - bits)).astype(np.int16) if bits <= 16 else (x << (32 - bits)).astype(np.int32)


def md5_of(x: np.ndarray, bits: int) -> bytes:
    width = (bits + 7) // 8
    le = np.ascontiguousarray(np.asarray(x, dtype=np.int64).astype("<i8")).view(np.uint8).reshape(-1, 8)[:, :width]
    return hashlib.md5(np.ascontiguousarray(le).tobytes()).digest()


# ---- the writer ----

class _W:
    def __init__(self):
        self.parts = []

    def u(self, v, n):
        if n:
            assert 0 <= v < (1 << n), (v, n)
            self.parts.append(format(v, "0%db" % n))

    def s(self, v, n):
        if n:
            assert -(1 << (n - 1)) <= v < (1 << (n - 1)), (v, n)
            self.parts.append(format(v & ((1 << n) - 1), "0%db" % n))

    def unary(self, q):
        self.parts.append("0" * q + "1")

    def bytes(self) -> bytes:
        t = "".join(self.parts)
        t += "0" * (-len(t) % 8)
        return int(t, 2).to_bytes(len(t) // 8, "big") if t else b""


def coded_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for n in range(2, 8):
        if v < 1 << (7 - n + 6 * (n - 1)):
            lead = ((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))
            return bytes([lead] + [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(n - 2, -1, -1)])
    raise ValueError(v)


_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def _write_residual(w, res, bs, order, part_order, method, escapes):
    w.u(method, 2)
    w.u(part_order, 4)
    pb = 5 if method else 4
    esc = (1 << pb) - 1
    at = 0
    for part in range(1 << part_order):
        count = (bs >> part_order) - (order if part == 0 else 0)
        vals = res[at:at + count]
        at += count
        if part in escapes:
            n = max([0] + [(v if v >= 0 else ~v).bit_length() + 1 for v in vals if v != 0])
            w.u(esc, pb)
            w.u(n, 5)
            for v in vals:
                w.s(v, n)
            continue
        us = [(v << 1) if v >= 0 else ((-v) << 1) - 1 for v in vals]
        k = min(max(max(us + [0]).bit_length() - 2, 0), esc - 1)
        w.u(k, pb)
        for u in us:
            w.unary(u >> k)
            w.u(u & ((1 << k) - 1), k)
    assert at == len(res)


def _write_subframe(w, s, width, spec):
    """s: the channel's integers of `width` bits.  spec: kind constant | verbatim | fixed | lpc | raw, order, precision, shift, coefs,
    part_order, method, escapes, wasted; raw: type (the six type bits) and payload [(value, bits), ...] written behind the
    wasted-bits field."""
    kind, wasted = spec.get("kind", "verbatim"), spec.get("wasted", 0)
    s = [int(v) for v in s]
    bs = len(s)
    if wasted:
        assert all(v & ((1 << wasted) - 1) == 0 for v in s)
        s = [v >> wasted for v in s]
    wd = width - wasted
    order = spec.get("order", 0)
    tbits = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order, "raw": spec.get("type", 0)}[kind]
    w.u(0, 1)
    w.u(tbits, 6)
    w.u(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "raw":
        for v, n in spec["payload"]:
            w.u(v, n)
    elif kind == "constant":
        assert all(v == s[0] for v in s)
        w.s(s[0], wd)
    elif kind == "verbatim":
        for v in s:
            w.s(v, wd)
    else:
        for v in s[:order]:
            w.s(v, wd)
        if kind == "fixed":
            co, shift = _FIXED[order], 0
        else:
            co, shift, prec = spec["coefs"], spec["shift"], spec["precision"]
            w.u(prec - 1, 4)
            w.s(shift, 5)
            for cf in co:
                w.s(cf, prec)
        res = [s[i] - (sum(cf * s[i - 1 - j] for j, cf in enumerate(co)) >> shift) for i in range(order, bs)]
        _write_residual(w, res, bs, order, spec.get("part_order", 0), spec.get("method", 0), spec.get("escapes", ()))


def encode_frame(x, rate, bits, number, variable=False, stereo=0, subs=None, bs_code=None, rate_code=None, bits_code=None) -> bytes:
    """x: int [blocksize][channels].  stereo: 0 independent, 8 left/side, 9 side/right, 10 mid/side.  subs: one subframe spec per
    channel.  bs_code / rate_code / bits_code force a header code (6, 7: the blocksize follows; 12, 13, 14: the rate follows;
    0: take it from STREAMINFO)."""
    x = np.asarray(x, dtype=np.int64)
    bs, ch = x.shape
    subs = subs or [{}] * ch
    if bs_code is None:
        bs_code = BS_CODES.get(bs, 6 if bs <= 256 else 7)
    if rate_code is None:
        rate_code = RATE_CODES.get(rate, 0)
    if bits_code is None:
        bits_code = BITS_CODES.get(bits, 0)
    head = bytearray([0xFF, 0xF8 | (1 if variable else 0), (bs_code << 4) | rate_code, ((stereo if stereo else ch - 1) << 4) | (bits_code << 1)])
    head += coded_number(number)
    if bs_code in (6, 7):
        head += (bs - 1).to_bytes(bs_code - 5, "big")
    if rate_code == 12:
        head += bytes([rate // 1000])
    elif rate_code in (13, 14):
        head += (rate if rate_code == 13 else rate // 10).to_bytes(2, "big")
    head.append(crc8(head))
    cols, widths = [x[:, c].tolist() for c in range(ch)], [bits] * ch
    if stereo:
        l, r = cols
        side = [a - b for a, b in zip(l, r)]
        if stereo == 8:
            cols, widths = [l, side], [bits, bits + 1]
        elif stereo == 9:
            cols, widths = [side, r], [bits + 1, bits]
        else:
            cols, widths = [[(a + b) >> 1 for a, b in zip(l, r)], side], [bits, bits + 1]
    w = _W()
    for col, wd, spec in zip(cols, widths, subs):
        _write_subframe(w, col, wd, spec)
    body = bytes(head) + w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def write_stream(frames, rate, channels, bits, total, md5=None, min_bs=16, max_bs=65535, id3v2=0, padding=None, id3v1=False,
                 seektable=False) -> bytes:
    """The file: optional ID3v2 tag of `id3v2` payload bytes, fLaC, STREAMINFO, optional SEEKTABLE-typed and PADDING blocks, the
    frames, an optional ID3v1 tag."""
    out = bytearray()
    if id3v2:
        out += b"ID3\x04\x00\x00" + bytes([(id3v2 >> 21) & 0x7F, (id3v2 >> 14) & 0x7F, (id3v2 >> 7) & 0x7F, id3v2 & 0x7F]) + b"\x55" * id3v2
    out += b"fLaC"
    info = struct.pack(">HH", min_bs, max_bs) + b"\0\0\0\0\0\0"
    info += ((rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total).to_bytes(8, "big") + (md5 or b"\0" * 16)
    blocks = [(0, info)]
    if seektable:
        blocks.append((3, b"\xff" * 18))
    if padding is not None:
        blocks.append((1, b"\0" * padding))
    for k, (t, body) in enumerate(blocks):
        out += bytes([t | (0x80 if k + 1 == len(blocks) else 0)]) + len(body).to_bytes(3, "big") + body
    for f in frames:
        out += f
    if id3v1:
        out += b"TAG" + b"\x20" * 125
    return bytes(out)


def encode(x, rate, bits, blocksizes, variable=False, start=0, stereo=0, sub=None, md5=True, total=None, frame_kw=None, **stream_kw):
    """x int [samples][channels] -> file bytes.  blocksizes: the blocksize of every frame (their sum = len(x)); stereo: a code, or
    a function of the frame index; sub(frame, channel) -> subframe spec; frame_kw(frame) -> extra encode_frame arguments."""
    x = np.asarray(x, dtype=np.int64)
    assert sum(blocksizes) == len(x)
    frames, at = [], 0
    for k, bs in enumerate(blocksizes):
        number = start + at if variable else start + k
        st = stereo(k) if callable(stereo) else stereo
        frames.append(encode_frame(x[at:at + bs], rate, bits, number, variable, st, [sub(k, c) if sub else {} for c in range(x.shape[1])],
                                   **(frame_kw(k) if frame_kw else {})))
        at += bs
    return write_stream(frames, rate, x.shape[1], bits, len(x) if total is None else total, md5_of(x, bits) if md5 else None, **stream_kw)


# ---- the reader ----

class _R:
    def __init__(self, data: bytes, pos: int):
        self.d, self.pos = data, pos * 8

    def u(self, n: int) -> int:
        if n == 0:
            return 0
        a, b = self.pos >> 3, (self.pos + n + 7) >> 3
        if b > len(self.d):
            raise FlacError("ran past the end")
        v = int.from_bytes(self.d[a:b], "big") >> (b * 8 - self.pos - n)
        self.pos += n
        return v & ((1 << n) - 1)

    def s(self, n: int) -> int:
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        q = 0
        while True:
            left = len(self.d) * 8 - self.pos
            if left <= 0:
                raise FlacError("ran past the end")
            n = min(left, 32)
            v = self.u(n)
            if v:
                z = n - v.bit_length()
                self.pos -= n - z - 1
                return q + z
            q += n


def _read_number(d, pos, one_byte):
    b = d[pos]
    if b < 0x80 or one_byte:
        return b, 1
    n = 8 - (b ^ 0xFF).bit_length()            # leading ones
    if n < 2 or n > 7:
        raise FlacError("invalid coded number")
    v = b & (0x7F >> n)
    for k in range(1, n):
        if d[pos + k] & 0xC0 != 0x80:
            raise FlacError("invalid coded number")
        v = (v << 6) | (d[pos + k] & 0x3F)
    return v, n


def _read_header(d, pos, end, mut):
    if pos + 6 > end or d[pos] != 0xFF or d[pos + 1] & 0xFE != 0xF8:
        raise FlacError(f"no frame header at byte {pos}")
    variable = d[pos + 1] & 1
    bsc, rc, cc, sc = d[pos + 2] >> 4, d[pos + 2] & 15, d[pos + 3] >> 4, (d[pos + 3] >> 1) & 7
    if d[pos + 3] & 1 or bsc == 0 or rc == 15 or cc > 10 or sc == 3:
        raise FlacError(f"reserved code in the frame header at byte {pos}")
    number, n = _read_number(d, pos + 4, mut.get("one_byte_number"))
    at = pos + 4 + n
    plus = 0 if mut.get("bs_code_no_plus1") else 1
    if bsc == 1:
        bs = 192
    elif bsc <= 5:
        bs = 576 << (bsc - 2)
    elif bsc == 6:
        bs, at = d[at] + plus, at + 1
    elif bsc == 7:
        bs, at = int.from_bytes(d[at:at + 2], "big") + plus, at + 2
    else:
        bs = 256 << (bsc - 8)
    rate = {v: k for k, v in RATE_CODES.items()}.get(rc, 0)
    if rc == 12:
        rate, at = d[at] * 1000, at + 1
    elif rc in (13, 14):
        rate, at = int.from_bytes(d[at:at + 2], "big") * (1 if rc == 13 else 10), at + 2
    if at >= end or crc8(d[pos:at]) != d[at]:
        raise FlacError(f"broken CRC-8 in the frame header at byte {pos}")
    bits = {0: 0, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}[sc]
    return dict(variable=variable, bs=bs, rate=rate, channels=cc + 1 if cc < 8 else 2, stereo=cc if cc >= 8 else 0, bits=bits,
                number=number, len=at + 1 - pos)


def _read_residual(r, bs, order, mut):
    method = r.u(2)
    if method > 1:
        raise FlacError("reserved residual method")
    P = r.u(4)
    if bs % (1 << P) or (bs >> P) < order:
        raise FlacError("bad partition")
    pb = 5 if method else 4
    out = []
    for part in range(1 << P):
        count = (bs >> P) - (order if part == 0 and not mut.get("part0_full") else 0)
        k = r.u(pb)
        if k == (1 << pb) - 1:
            n = r.u(5)
            out += [r.s(n) for _ in range(count)]
            continue
        for _ in range(count):
            u = (r.unary() << k) | r.u(k)
            out.append(-(u >> 1) if mut.get("zigzag_sign") and u & 1 else (u >> 1) ^ -(u & 1))
    return out[:bs - order]


def _read_subframe(r, bs, width, mut):
    if r.u(1):
        raise FlacError("reserved subframe padding bit")
    t = r.u(6)
    wasted = r.unary() + 1 if r.u(1) else 0
    wd = width - wasted
    if wd < 1:
        raise FlacError("wasted bits leave no width")
    if t == 0:
        s = [r.s(wd)] * bs
    elif t == 1:
        s = [r.s(wd) for _ in range(bs)]
    elif 8 <= t <= 12 or t >= 32:
        order = t - 8 if t < 32 else t - 31
        if order > bs:
            raise FlacError("bad partition: order above the blocksize")
        s = [r.s(wd) for _ in range(order)]
        if t < 32:
            co, shift = _FIXED[order], 0
        else:
            prec = r.u(4) + 1
            if prec == 16:
                raise FlacError("bad precision")
            shift = r.s(5)
            if shift < 0:
                raise FlacError("bad shift")
            co = [r.s(prec) for _ in range(order)]
        for e in _read_residual(r, bs, order, mut):
            acc = sum(cf * s[-1 - j] for j, cf in enumerate(co))
            if t >= 32 and mut.get("lpc_32bit"):
                acc = ((acc + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
            if t >= 32 and mut.get("lpc_logical_shift"):
                acc &= (1 << 64) - 1
            s.append(e + (acc >> shift))
    else:
        raise FlacError("reserved subframe type")
    return s if mut.get("no_wasted_shift") else [v << wasted for v in s]


class Decoded:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def read(blob: bytes, **mut) -> Decoded:
    """File bytes -> Decoded(rate, channels, bits, samples int64 [n][channels], frames [(byte offset, byte length, first sample)],
    max_bs, first_frame, total (STREAMINFO's claim), md5 (None: absent, else whether it matches)).  FlacError for everything the
    stream definition refuses.  **mut: the mutant switches (MUTANTS)."""
    assert set(mut) <= set(MUTANTS)
    d, pos = bytes(blob), 0
    if d[:3] == b"ID3" and len(d) >= 10:
        pos = 10 + ((d[6] & 0x7F) << 21 | (d[7] & 0x7F) << 14 | (d[8] & 0x7F) << 7 | (d[9] & 0x7F)) + (10 if d[5] & 0x10 else 0)
    if d[pos:pos + 4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos += 4
    info, last = None, False
    while not last:
        if pos + 4 > len(d):
            raise FlacError("cut inside the metadata")
        t, size, last = d[pos] & 0x7F, int.from_bytes(d[pos + 1:pos + 4], "big"), bool(d[pos] & 0x80)
        if t == 127 or (info is None) != (t == 0) or pos + 4 + size > len(d) or (t == 0 and size != 34):
            raise FlacError("invalid metadata")
        if t == 0:
            info = d[pos + 4:pos + 38]
        pos += 4 + size
    v = int.from_bytes(info[10:18], "big")
    rate, channels, bits, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if not 4 <= bits <= 24:
        raise FlacError(f"{bits} bits per sample")
    end = len(d)
    if end - 128 >= pos and d[end - 128:end - 125] == b"TAG":
        end -= 128
    first_frame, frames, cols, prev = pos, [], [[] for _ in range(channels)], None
    n = 0
    while pos < end:
        h = _read_header(d, pos, end, mut)
        if (h["rate"] and h["rate"] != rate) or h["channels"] != channels or (h["bits"] and h["bits"] != bits):
            raise FlacError(f"the frame at byte {pos} differs from STREAMINFO")
        if not 1 <= h["bs"] <= 65535:
            raise FlacError("blocksize")
        if prev is not None and (h["variable"] != prev["variable"] or
                                 h["number"] != (prev["number"] + prev["bs"] if prev["variable"] else prev["number"] + 1)):
            raise FlacError(f"the coded number of the frame at byte {pos} does not continue")
        r = _R(d[:end], pos + h["len"])
        sub = []
        for c in range(channels):
            side = (h["stereo"], c) in ((8, 1), (9, 0), (10, 1)) and not mut.get("no_side_bit")
            sub.append(_read_subframe(r, h["bs"], bits + (1 if side else 0), mut))
        if r.u(-r.pos % 8):
            raise FlacError("padding bits are set")
        q = r.pos >> 3
        if q + 2 > end:
            raise FlacError("ran past the end")
        crc = _crc16_reflected(d[pos:q]) if mut.get("crc16_reflected") else crc16(d[pos:q])
        if crc != int.from_bytes(d[q:q + 2], "big"):
            raise FlacError(f"broken CRC-16 in the frame at byte {pos}")
        if h["stereo"] == 8:
            sub[1] = [a - b for a, b in zip(sub[0], sub[1])]
        elif h["stereo"] == 9:
            sub[0] = [a + b for a, b in zip(sub[0], sub[1])]
        elif h["stereo"] == 10:
            m = [(a << 1) | (0 if mut.get("midside_lowbit") else b & 1) for a, b in zip(sub[0], sub[1])]
            sub = [[(a + b) >> 1 for a, b in zip(m, sub[1])], [(a - b) >> 1 for a, b in zip(m, sub[1])]]
        for c in range(channels):
            cols[c] += sub[c]
        frames.append((pos, q + 2 - pos, n))
        n += h["bs"]
        pos, prev = q + 2, h
    if n > 1 << 40:
        raise FlacError("more than 2^40 samples")
    x = np.array(cols, dtype=np.int64).T.reshape(n, channels)
    md5 = None if info[18:34] == b"\0" * 16 else md5_of(x, bits) == info[18:34]
    return Decoded(rate=rate, channels=channels, bits=bits, samples=x, frames=frames, first_frame=first_frame, total=total, md5=md5,
                   max_bs=max([0] + [b[2] - a[2] for a, b in zip(frames, frames[1:])] + ([n - frames[-1][2]] if frames else [])))


# ---- the case table ----

def signal(n, ch, bits, seed, smooth=True):
    """Deterministic integers of `bits` bits [n][ch]: a random walk (what predictors like) or white noise over the whole range."""
    rng = np.random.default_rng([0xF1AC, seed, n, ch, bits])
    lim = 1 << (bits - 1)
    if not smooth:
        return rng.integers(-lim, lim, size=(n, ch), dtype=np.int64)
    step = rng.integers(-(lim >> 4) - 1, (lim >> 4) + 2, size=(n, ch), dtype=np.int64)
    return np.clip(np.cumsum(step, axis=0), -lim, lim - 1)


def _lpc_spec(order, seed, **kw):
    rng = np.random.default_rng([0x1BC, order, seed])
    coefs = [int(v) for v in rng.integers(-(1 << 14), 1 << 14, size=order)]
    coefs[0] = -(1 << 14) if seed % 2 else coefs[0]             # negative sums
    return dict(kind="lpc", order=order, precision=15, shift=14, coefs=coefs, **kw)


def _split(n, bs):
    return [bs] * (n // bs) + ([n % bs] if n % bs else [])


_cache = {}


def case(name):
    """(file bytes, rate, bits, expected int64 [samples][channels]) of a named case, built once."""
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def _c_fixed_orders(bits, ch, rate):
    def build():
        x = signal(5 * 255, ch, bits, bits)
        sub = lambda k, c: dict(kind="fixed", order=k, method=(k + c) & 1)  # noqa: E731
        return encode(x, rate, bits, [255] * 5, sub=sub), rate, bits, x
    return build


def _c_partitions():
    x = signal(4 * 256 + 16 + 17, 2, 16, 3)
    def sub(k, c):  # noqa: E306
        if k < 4:
            return dict(kind="fixed", order=(k + 1 + c) % 5, part_order=k, method=c, escapes=((1,) if k == 2 else ()))
        return dict(kind="fixed", order=2, part_order=(2 if k == 4 else 0), method=1)
    return encode(x, 8000, 16, [256] * 4 + [16, 17], sub=sub), 8000, 16, x


def _c_escapes():
    x = signal(3 * 192, 1, 12, 5)
    x[192:192 + 96] = x[192]                       # a flat stretch: residual zero, escape with n = 0
    sub = lambda k, c: dict(kind="fixed", order=1, part_order=1, method=k & 1, escapes=(0, 1) if k else (1,))  # noqa: E731
    return encode(x, 16000, 12, [192] * 3, sub=sub), 16000, 12, x


def _c_lpc(bits, rate, orders, bs):
    def build():
        x = signal(bs * len(orders), 2, bits, 7 + bits, smooth=False)
        sub = lambda k, c: _lpc_spec(orders[k], k + c, part_order=(k % 3 if bs % 4 == 0 and (bs >> 2) >= orders[k] else 0), method=1)  # noqa: E731
        return encode(x, rate, bits, [bs] * len(orders), sub=sub, stereo=lambda k: 0), rate, bits, x
    return build


def _c_stereo(bits, rate):
    def build():
        n = 4 * 576
        x = signal(n, 2, bits, 11) >> 1
        d = np.clip(signal(n, 1, bits - 3, 12)[:, 0], -(1 << (bits - 4)) + 1, (1 << (bits - 4)) - 1)
        x[:, 1] = x[:, 0] - 4 * d                                               # left - right has two wasted bits
        def sub(k, c):  # noqa: E306
            if k % 4 == 0:
                return dict(kind="verbatim")
            side = (k % 4, c) in ((1, 1), (2, 0), (3, 1))
            return dict(kind="fixed", order=2, part_order=2, wasted=2) if side else dict(kind="fixed", order=1, method=1)
        return encode(x, rate, bits, [576] * 4, stereo=lambda k: (0, 8, 9, 10)[k % 4], sub=sub), rate, bits, x
    return build


def _c_variable():
    sizes = [17, 1000, 16, 255, 1, 192, 300]
    x = signal(sum(sizes), 1, 16, 13)
    sub = lambda k, c: dict(kind="fixed", order=min(k % 5, sizes[k] - 1 if sizes[k] < 5 else 4))  # noqa: E731
    return encode(x, 44100, 16, sizes, variable=True, start=100, sub=sub, frame_kw=lambda k: dict(bs_code=7 if k == 1 else None)), 44100, 16, x


def _c_many_small():
    x = signal(140 * 16, 2, 8, 17)
    sub = lambda k, c: dict(kind="fixed", order=1 + (k & 1), method=c)  # noqa: E731
    return encode(x, 8000, 8, [16] * 140, sub=sub, stereo=lambda k: 10 if k % 3 == 0 else 0), 8000, 8, x


def _c_channels(ch, bits, rate, bs):
    def build():
        x = signal(2 * bs + 5, ch, bits, 19 + ch)
        x[:, ch - 1] = x[0, ch - 1]                  # a constant channel
        sub = lambda k, c: dict(kind="constant") if c == ch - 1 else dict(kind="fixed", order=c % 5, wasted=0)  # noqa: E731
        return encode(x, rate, bits, [bs, bs, 5], sub=sub), rate, bits, x
    return build


def _c_odd_width():
    x = signal(1000 + 4096, 2, 13, 23)
    sub = lambda k, c: dict(kind="fixed", order=3, part_order=3, method=1)  # noqa: E731
    return encode(x, 22050, 13, [1000, 4096], sub=sub, stereo=lambda k: 10), 22050, 13, x


def _c_big_blocks():
    x = signal(4608 + 4096, 1, 20, 29)
    sub = lambda k, c: dict(kind="fixed", order=4, part_order=2 + k)  # noqa: E731
    return encode(x, 44100, 20, [4608, 4096], sub=sub), 44100, 20, x


def _c_largest_frame():
    x = signal(65535, 2, 16, 31, smooth=False)
    x[:, 1] = -12345
    sub = lambda k, c: dict(kind="constant") if c else dict(kind="verbatim")  # noqa: E731
    return encode(x, 16000, 16, [65535], sub=sub), 16000, 16, x


def _c_tags():
    x = signal(3 * 256, 2, 16, 37)
    sub = lambda k, c: dict(kind="fixed", order=2, part_order=1)  # noqa: E731
    return encode(x, 16000, 16, [256] * 3, sub=sub, id3v2=301, padding=77, id3v1=True, seektable=True), 16000, 16, x


def _c_rate_codes():
    x = signal(3 * 100, 1, 16, 41)
    return encode(x, 11000, 16, [100] * 3, sub=lambda k, c: dict(kind="fixed", order=1), frame_kw=lambda k: dict(rate_code=(12, 13, 14)[k], bits_code=0)), 11000, 16, x


def _c_wasted_verbatim():
    x = signal(2 * 64, 1, 24, 43) & ~0xFF
    return encode(x, 48000, 24, [64, 64], sub=lambda k, c: dict(kind="verbatim" if k else "fixed", order=0, wasted=8)), 48000, 24, x


def _c_decoy(kind):
    """Three verbatim frames.  Inside one of them stands, behind two bytes that make the CRC-16 of the frame so far zero, what a scan
    can take for the next frame: in the last frame a sync code whose header CRC-8 fails ("sync_in_last"), in the middle frame a
    whole valid header - frame 0's own seven bytes, so its number does not continue - ("header_in_middle").  Neither is a frame end: no valid
    continuing header begins there."""
    def build():
        x = signal(3 * 32, 1, 16, 53)
        frame = lambda k: encode_frame(x[32 * k:32 * k + 32], 16000, 16, k, subs=[dict(kind="verbatim")])  # noqa: E731
        k, decoy = (2, b"\xff\xf8") if kind == "sync_in_last" else (1, frame(0)[:8])
        at = 32 * k + 4                                           # the sample that becomes the CRC-16; the decoy follows it
        x[at + 1:at + 1 + len(decoy) // 2, 0] = np.frombuffer(decoy, dtype=">i2")
        x[at, 0] = 0
        head = frame(k)[:-2 - 2 * (32 - 4)]                       # header, subframe header and samples 0 .. 3 of the frame
        x[at, 0] = np.frombuffer(crc16(head).to_bytes(2, "big"), dtype=">i2")[0]
        blob = write_stream([frame(0), frame(1), frame(2)], 16000, 1, 16, 96, md5_of(x, 16))
        body = frame(k)
        assert crc16(body[:len(head) + 2]) == 0 and body[len(head) + 2:len(head) + 2 + len(decoy)] == decoy
        return blob, 16000, 16, x
    return build


CASES = {
    "fixed_8bit_mono": _c_fixed_orders(8, 1, 8000),
    "fixed_16bit_3ch": _c_fixed_orders(16, 3, 16000),
    "fixed_24bit_stereo": _c_fixed_orders(24, 2, 44100),
    "partitions": _c_partitions,
    "escapes": _c_escapes,
    "lpc_16bit": _c_lpc(16, 16000, (1, 7, 32), 192),
    "lpc_24bit": _c_lpc(24, 44100, (1, 7, 32), 256),
    "stereo_16bit": _c_stereo(16, 8000),
    "stereo_24bit": _c_stereo(24, 16000),
    "variable": _c_variable,
    "many_small": _c_many_small,
    "ch8_12bit": _c_channels(8, 12, 16000, 17),
    "ch3_20bit": _c_channels(3, 20, 44100, 576),
    "odd_width_13": _c_odd_width,
    "big_blocks": _c_big_blocks,
    "largest_frame": _c_largest_frame,
    "tags": _c_tags,
    "rate_codes": _c_rate_codes,
    "wasted_verbatim": _c_wasted_verbatim,
    "decoy_sync_in_last": _c_decoy("sync_in_last"),
    "decoy_header_in_middle": _c_decoy("header_in_middle"),
}

KNOWN_ANSWER_HEX = ("664c614380000022100010000000 0f00000f0ac442f0000000013e84b41807dc6903 07586a3dad1a2e0f"
                    "fff8691800 00bf 0358fd03128b aa9a").replace(" ", "")
# (RFC 9639's first example: 44100 Hz, 2 channels, 16 bits, one frame of one sample, samples 25588 and 10416)


# ---- CRC-valid frames with illegal content (one small mono 16-bit file each; frame 1 of 3 is the bad one) ----

def illegal(kind: str) -> bytes:
    x = signal(3 * 32, 1, 16, 47)
    good = lambda k: encode_frame(x[32 * k:32 * k + 32], 16000, 16, k, subs=[dict(kind="fixed", order=1)])  # noqa: E731
    payload = {
        "reserved_type": dict(kind="raw", type=0b000010, payload=[(0, 64)]),
        "reserved_type_13": dict(kind="raw", type=13, payload=[(0, 64)]),
        "precision_1111": dict(kind="raw", type=32, payload=[(5, 16), (15, 4), (3, 5), (1, 8)]),
        "negative_shift": dict(kind="raw", type=32, payload=[(5, 16), (7, 4), (0b11111, 5), (1, 8)]),
        "unary_to_the_end": dict(kind="raw", type=9, payload=[(5, 16), (0, 2), (0, 4), (3, 4), (0, 200)]),
        "partition_not_dividing": dict(kind="raw", type=9, payload=[(5, 16), (0, 2), (6, 4), (0, 40)]),
        "partition_below_order": dict(kind="raw", type=12, payload=[(5, 16)] * 4 + [(0, 2), (4, 4), (0, 40)]),
        "residual_method_2": dict(kind="raw", type=9, payload=[(5, 16), (2, 2), (0, 40)]),
        "trailing_bytes_in_frame": dict(kind="raw", type=0, payload=[(5, 16), (0, 24)]),
        "padding_bit_set": dict(kind="raw", type=8, payload=[(0, 2), (0, 4), (0, 4)] + [(1, 1)] * 32 + [(1, 6)]),
    }[kind]
    bad = encode_frame(x[32:64], 16000, 16, 1, subs=[payload])
    return write_stream([good(0), bad, good(2)], 16000, 1, 16, 96)


ILLEGAL = {"reserved_type": "reserved", "reserved_type_13": "reserved", "precision_1111": "precision", "negative_shift": "shift",
           "unary_to_the_end": "past the end", "partition_not_dividing": "partition", "partition_below_order": "partition",
           "residual_method_2": "reserved", "trailing_bytes_in_frame": "end before", "padding_bit_set": "reserved"}


# ---- refused streams ----

def patched(frame: bytes, fn) -> bytes:
    """The frame with fn(header bytearray) applied and both CRCs made good again."""
    h = _read_header(frame, 0, len(frame), {})
    head = bytearray(frame[:h["len"] - 1])
    fn(head)
    head.append(crc8(head))
    body = bytes(head) + frame[h["len"]:-2]
    return body + crc16(body).to_bytes(2, "big")


def three(rate=16000, bits=16, ch=1, numbers=(0, 1, 2), variable=False, **kw):
    x = signal(96, ch, bits, 51)
    return [encode_frame(x[32 * k:32 * k + 32], rate, bits, numbers[k], variable, subs=[dict(kind="fixed", order=1)] * ch, **kw) for k in range(3)]


def stream_of(frames, rate=16000, ch=1, bits=16, **kw):
    return write_stream(frames, rate, ch, bits, 96, **kw)


def _set(i, v):
    def fn(head):
        head[i] = v
    return fn


def refusals():
    """(what, file bytes, a piece of the library's message) for every stream the definition refuses."""
    good = three()
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x40]) + b[i + 1:]  # noqa: E731
    yield "32 bits in STREAMINFO", write_stream(good, 16000, 1, 32, 96), "32 bits per sample"
    yield "25 bits in STREAMINFO", write_stream(good, 16000, 1, 25, 96), "25 bits per sample"
    yield "frame 0 at another rate", stream_of(three(rate=8000)), "frame 0 at byte 42: its rate differs"
    yield "frame 2 at another rate", stream_of(good[:2] + three(rate=8000)[2:]), "frame 2 at byte 167: its rate differs"
    yield "another channel count", stream_of(good[:1] + three(ch=2)[1:]), "frame 1 at byte 105: its channel count differs"
    yield "another width", stream_of(good[:2] + three(bits=8)[2:]), "its sample width differs"
    yield "32-bit frame", stream_of([patched(good[0], lambda h: _set(3, h[3] | 0x0E)(h))] + good[1:]), "32 bits per sample"
    yield "reserved blocksize code", stream_of([patched(good[0], lambda h: (_set(2, h[2] & 0x0F)(h), h.__delitem__(5)))] + good[1:]), "reserved blocksize code"
    yield "invalid rate code", stream_of([patched(good[0], lambda h: _set(2, h[2] | 0x0F)(h))] + good[1:]), "invalid rate code"
    yield "reserved channel code", stream_of([patched(good[0], lambda h: _set(3, (h[3] & 0x0F) | 0xB0)(h))] + good[1:]), "reserved channel code"
    yield "reserved sample-size code", stream_of([patched(good[0], lambda h: _set(3, (h[3] & 0xF1) | 0x06)(h))] + good[1:]), "reserved sample-size code"
    yield "reserved bit", stream_of([patched(good[0], lambda h: _set(3, h[3] | 1)(h))] + good[1:]), "reserved bit"
    yield "reserved code in a later frame", stream_of(good[:1] + [patched(good[1], lambda h: _set(3, h[3] | 1)(h))] + good[2:]), "frame 1 at byte 105: reserved bit"
    yield "broken CRC-8 of frame 0", stream_of([flip(good[0], 2)] + good[1:]), "frame 0 at byte 42: broken header CRC-8"
    yield "broken CRC-8 of frame 1", stream_of([good[0], flip(good[1], 4)] + good[2:]), "frame 1 at byte 105: broken header CRC-8"
    yield "broken CRC-16 of frame 1", stream_of([good[0], flip(good[1], len(good[1]) - 1), good[2]]), "frame 1 at byte 105: no end where its CRC-16 holds"
    yield "damage inside frame 2", stream_of(good[:2] + [flip(good[2], 20)]), "frame 2 at byte 167: no end where its CRC-16 holds"
    yield "fixed blocking skips a number", stream_of(three(numbers=(0, 1, 3))), "its coded number 3 does not continue 1 (fixed"
    yield "variable blocking repeats a number", stream_of(three(numbers=(500, 532, 532), variable=True)), "its coded number 532 does not continue 532 (variable"
    yield "the strategy changes", stream_of(good[:2] + three(numbers=(0, 1, 64), variable=True)[2:]), "does not continue"
    yield "bytes behind the last frame", stream_of(good) + b"junk!", "5 bytes behind frame 2 (from byte 229) are neither a frame nor an ID3v1 tag"
    yield "a short tag behind the last frame", stream_of(good) + b"TAG" + b" " * 100, "103 bytes behind frame 2"
    yield "metadata type 127", b"fLaC" + bytes([127, 0, 0, 34]) + bytes(34) + b"".join(good), "type 127"
    yield "STREAMINFO is not first", b"fLaC" + bytes([1, 0, 0, 2, 0, 0]) + stream_of(good)[4:], "STREAMINFO must be the first"
    yield "STREAMINFO of another size", b"fLaC" + bytes([0x80, 0, 0, 33]) + bytes(33), "33 bytes instead of 34"
    yield "cut inside the metadata", stream_of(good)[:30], "cut inside the metadata"
    yield "an ID3 tag that runs past the file", b"ID3\x04\x00\x00\x00\x00\x7f\x7f" + stream_of(good), "no fLaC marker"
