"""CPU: the C ABI of wire streams - the header, the library's exports and _lib.SYMBOLS agree on the three new names, and
ttasr_ingest_stream_len (no context, no GPU) is the K(F) / n_out(F) of tests/wire_stream_reference.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import wire_stream_reference as ws
from taiwan_tongues_asr_ce_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ttasr_ingest_stream_len", "ttasr_vad_stream_open_wire", "ttasr_vad_stream_push_wire")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_exports_and_symbols_agree_on_the_three_names(lib):
    hdr = open(os.path.join(ROOT, "include", "ttasr.h")).read()
    declared = set(re.findall(r"TTASR_API\s+\w+\s+(ttasr_[a-z_0-9]+)\s*\(", hdr))
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert name in declared and name in defined and name in _lib.SYMBOLS, name
        assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None
    assert lib.ttasr_ingest_stream_len.restype is ctypes.c_int64
    assert '"wire_chunk"' in hdr


def test_stream_len_is_the_reference_count(lib):
    rates = ws.ref.RATES + (16000, 15984, 16)
    for rate in rates:
        assert ws.stream_rate(rate), rate
        for F in list(range(0, 300)) + [511, 512, 4807, 57607, 10 ** 9, 1 << 40]:
            assert lib.ttasr_ingest_stream_len(rate, F, 0) == ws.final(rate, F), (rate, F)
            assert lib.ttasr_ingest_stream_len(rate, F, 1) == ws.final(rate, F, True) == lib.ttasr_ingest_len(rate, F), (rate, F)
    assert [lib.ttasr_ingest_stream_len(16000, F, 0) for F in (0, 1, 513)] == [0, 1, 513]


def test_stream_len_refuses_what_the_stream_path_does_not_take(lib):
    assert lib.ttasr_ingest_len(384000, 10) >= 0 and lib.ttasr_ingest_stream_len(384000, 10, 0) < 0      # H = 480: file ingest only
    assert lib.ttasr_ingest_len(16000 * 1024, 10) >= 0 and lib.ttasr_ingest_stream_len(16000 * 1024, 10, 1) < 0
    for rate in (0, -8000, 16000 * 1025, 16001 * 3):                                                     # no ingest rate at all
        assert lib.ttasr_ingest_len(rate, 10) < 0 and lib.ttasr_ingest_stream_len(rate, 10, 0) < 0, rate
    assert lib.ttasr_ingest_stream_len(8000, -1, 0) < 0 and lib.ttasr_ingest_stream_len(8000, (1 << 40) + 1, 0) < 0
    assert lib.ttasr_ingest_stream_len(192000, 10, 0) == 0 and ws.plan(192000)[3] == 240                 # the largest listed rate
    # the wire calls need a context: a NULL one is refused, not dereferenced
    sid = ctypes.c_int32(-1)
    assert lib.ttasr_vad_stream_open_wire(None, 8000, 1, _lib.PCM_ULAW, -1, ctypes.byref(sid)) == -1
    assert lib.ttasr_vad_stream_push_wire(None, 1, None, None, None, None, None, None, None, None, None, None) == -1
