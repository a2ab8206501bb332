"""CPU: the FLAC decode body (csrc/flac.hpp) under the address and undefined-behaviour sanitizers, as its own program.
tests/flac_host_driver.cpp is compiled as plain C++ - host code only, the sanitizer flags given to the host side alone - with the Makefile's compiler and run: the
embedded damaged and truncated files, every frame with every byte damaged, every prefix of every frame and random bytes behind
valid headers go through the very decode_frame() the device runs with one lane per FLAC frame, on heap blocks of exactly the size
it may touch.  The GPU tests of the kernel rest on this being clean."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc")


def _hipcc():
    default = re.search(r"^HIPCC \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)


def test_decode_body_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "flac_host_driver")
    cc = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                         "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                         "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "flac_host_driver.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "flac driver ok" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert run.stdout.count("whole-frame prefixes ok") == 19

