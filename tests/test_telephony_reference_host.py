"""CPU: the reference decoders of tests/telephony_reference.py against the stdlib's audioop where it exists, and proof that the
reference tells the right decoder from the wrong ones it is there to catch."""
import struct

import numpy as np
import pytest

import telephony_reference as T


def test_g711_every_code_against_audioop():
    audioop = pytest.importorskip("audioop")
    codes = bytes(range(256))
    assert np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2").tolist() == T.ULAW_TABLE.tolist()
    assert np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2").tolist() == T.ALAW_TABLE.tolist()


def test_g711_ranges_and_symmetry():
    assert (int(T.ULAW_TABLE.min()), int(T.ULAW_TABLE.max())) == (-32124, 32124)
    assert (int(T.ALAW_TABLE.min()), int(T.ALAW_TABLE.max())) == (-32256, 32256)
    assert T.ulaw_sample(0xFF) == 0 and T.ulaw_sample(0x7F) == 0 and T.ulaw_sample(0x00) == -32124
    assert T.alaw_sample(0xD5) == 8 and T.alaw_sample(0x55) == -8
    assert len(set(T.ALAW_TABLE.tolist())) == 256 and len(set(T.ULAW_TABLE.tolist())) == 255      # mu-law has two zeros


def test_ima_nibble_rule_against_audioop():
    """audioop.adpcm2lin reads the high nibble of a byte first: the streams are compared with their nibbles swapped."""
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(0x1A)
    for _ in range(50):
        n = int(rng.integers(1, 200))
        data = rng.integers(0, 256, size=n, dtype=np.uint8)
        pred, index = int(rng.integers(-32768, 32768)), int(rng.integers(0, 89))
        swapped = bytes(((b & 15) << 4 | b >> 4) for b in data.tolist())
        want = np.frombuffer(audioop.adpcm2lin(swapped, 2, (pred, index))[0], dtype="<i2")
        got = []
        for b in data.tolist():
            for nib in (b & 15, b >> 4):
                pred, index = T.ima_nibble(nib, pred, index)
                got.append(pred)
        assert got == want.tolist()


def test_ima_block_layout_mono_by_hand():
    """One 12-byte mono block: header (100, index 3), then two groups.  The first samples are worked out by hand from the rule."""
    blk = struct.pack("<hBB", 100, 3, 0) + bytes([0x07, 0x80, 0, 0, 0, 0, 0, 0])
    x = T.ima_decode(blk, 1, 12)
    assert x.shape == (17, 1)
    # nibble 7 at step 10: d = 1 + 10 + 5 + 2 = 18 -> 118, index 3 + 8 = 11; nibble 0 at step 21: d = 2 -> 120, index 10;
    # nibble 0 at step 19: d = 2 -> 122, index 9; nibble 8 at step 17: d = 2, minus -> 120
    assert x[:5, 0].tolist() == [100, 118, 120, 122, 120]


def test_ima_stereo_groups_interleave_by_four_bytes():
    left = T.random_bytes(16, 1)
    right = T.random_bytes(16, 2)
    head_l, head_r = struct.pack("<hBB", -5, 40, 0), struct.pack("<hBB", 7000, 88, 0)
    stereo = head_l + head_r + b"".join(left[g:g + 4] + right[g:g + 4] for g in range(0, 16, 4))
    x = T.ima_decode(stereo, 2, 40)
    assert x.shape == (33, 2)
    assert x[:, 0].tolist() == T.ima_decode(head_l + left, 1, 20)[:, 0].tolist()
    assert x[:, 1].tolist() == T.ima_decode(head_r + right, 1, 20)[:, 0].tolist()


def test_header_index_above_88_reads_as_88():
    body = T.random_bytes(32, 3)
    a = T.ima_decode(struct.pack("<hBB", 11, 200, 0) + body, 1, 36)
    b = T.ima_decode(struct.pack("<hBB", 11, 88, 0) + body, 1, 36)
    assert a.tolist() == b.tolist()


@pytest.mark.parametrize("wrong", (dict(low_first=False), dict(clamp_index=False), dict(keep_eighth=False)))
def test_reference_differs_from_the_wrong_decoders_mono(wrong):
    raw = T.ima_stream(4, 1, 256, 5)
    assert not np.array_equal(T.ima_decode(raw, 1, 256), T.ima_decode(raw, 1, 256, **wrong))


def test_reference_differs_from_one_byte_stereo_groups():
    raw = T.ima_stream(4, 2, 72, 6)
    good, bad = T.ima_decode(raw, 2, 72), T.ima_decode(raw, 2, 72, group=1)
    assert good.shape == bad.shape and not np.array_equal(good, bad)
    assert np.array_equal(good[::65], bad[::65])          # the block headers are read alike: the data layout differs


def test_frame_count_rule():
    assert T.ima_spb(36, 1) == 65 and T.ima_spb(72, 2) == 65 and T.ima_spb(256, 1) == 505 and T.ima_spb(512, 2) == 505
    assert T.ima_frames(3 * 36 + 35, 1, 36) == 195                    # trailing bytes fill no block
    assert T.ima_frames(3 * 36, 1, 36, fact=100) == 100
    assert T.ima_frames(3 * 36, 1, 36, fact=196) == 195               # a fact beyond the blocks is not believed
