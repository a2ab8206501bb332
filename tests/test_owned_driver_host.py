"""CPU: the owner types of csrc/owned.hpp under the address and undefined-behaviour sanitizers, as their own program.
tests/owned_driver.cpp is compiled as plain C++ - no HIP runtime: the header takes its memory from a policy - with the Makefile's
compiler and run.  Its malloc-backed policy counts live allocations, records the order of quiesce / release / alloc and fails an
allocation on request, so the paths a GPU test cannot reach without starving the device - a block that cannot be allocated on
first use or on regrow - are checked here: empty block, error return, and the next call allocates."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc")


def _hipcc():
    default = re.search(r"^HIPCC \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)


def test_owner_types_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "owned_driver")
    cc = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                         "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
                         "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "owned_driver.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "owned driver ok" in run.stdout and "0 live" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr
