"""CPU: the plain-Python FLAC reference of the tests (tests/flac_reference.py) against itself.  The writer and the reader were
written independently from the stream definition, so a round trip checks both; the known answer of RFC 9639 checks the reader
against the outside world; and every mutant switch of the reader - one per classic decoder mistake - has to change the outcome
of at least one case of the table, or the table would not notice that mistake in the native decoder either."""
import os

import numpy as np
import pytest

import flac_reference as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac_rfc9639_example1.flac")


def test_known_answer_of_rfc_9639():
    blob = open(GOLDEN, "rb").read()
    assert blob == bytes.fromhex(F.KNOWN_ANSWER_HEX) and len(blob) == 57
    d = F.read(blob)
    assert (d.rate, d.channels, d.bits) == (44100, 2, 16)
    assert d.samples.tolist() == [[25588, 10416]] and d.frames == [(42, 15, 0)] and d.md5 is True
    assert blob[42 + 6] == 0xbf == F.crc8(blob[42:48])                   # the header CRC-8
    assert blob[-2:] == b"\xaa\x9a" and F.crc16(blob[42:-2]) == 0xaa9a   # the frame CRC-16


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_round_trip(name):
    blob, rate, bits, x = F.case(name)
    d = F.read(blob)
    assert (d.rate, d.channels, d.bits, d.total) == (rate, x.shape[1], bits, len(x))
    assert np.array_equal(d.samples, x) and d.md5 is True
    assert -(1 << (bits - 1)) <= int(x.min()) and int(x.max()) < 1 << (bits - 1)


def _outcome(blob, **mut):
    try:
        return F.read(blob, **mut).samples.tobytes()
    except F.FlacError as e:
        return "error: " + str(e)[:20]
    except (IndexError, AssertionError, OverflowError, ValueError) as e:           # a mutant may walk off the data
        return "crash: " + type(e).__name__


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_the_case_table_kills_every_mutant(mutant):
    killed = [name for name in F.CASES if name != "largest_frame" and _outcome(F.case(name)[0], **{mutant: True}) != _outcome(F.case(name)[0])]
    assert killed, mutant


def test_the_writer_covers_what_the_issue_lists():
    """The table holds every blocksize, width, channel count and stereo code the GPU test needs."""
    sizes, widths, chans = set(), set(), set()
    for name in F.CASES:
        blob, rate, bits, x = F.case(name)
        d = F.read(blob)
        firsts = [f[2] for f in d.frames] + [len(x)]
        sizes |= {b - a for a, b in zip(firsts, firsts[1:])}
        widths.add(bits)
        chans.add(x.shape[1])
    assert {1, 16, 17, 192, 255, 256, 576, 1000, 4096, 4608, 65535} <= sizes
    assert {8, 12, 13, 16, 20, 24} <= widths and {1, 2, 3, 8} <= chans


def test_illegal_frames_keep_valid_crcs():
    """The files with illegal content differ from a good file in frame 1 only, and their CRCs hold: the reader gets as far as
    the content."""
    for kind in F.ILLEGAL:
        blob = F.illegal(kind)
        with pytest.raises(F.FlacError) as e:
            F.read(blob)
        assert "CRC-8" not in str(e.value), kind
