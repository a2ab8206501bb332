"""The page book of both beam searches (csrc/beam_pages.hpp) under seeded random schedules, on the host: the GPU suite cannot see
a book-keeping mistake, because results do not depend on page ids and a leaked page only shows many steps later.
tests/beam_pages_driver.cpp is compiled as plain C++ with the Makefile's compiler and run; after every operation it checks that
the reference counts equal the table's, that the free list is exactly the unreferenced pages in descending order, that a write
page is private and a split leaves one pair whose source is still referenced, that a pool of rows x pages_per_seq pages never
reports empty, and that a pool that is too small is reported as such instead of crashing."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc")


def _hipcc():
    default = re.search(r"^HIPCC \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)


def test_page_book_holds_its_invariants_under_random_schedules(tmp_path):
    exe = str(tmp_path / "beam_pages_driver")
    cc = subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "beam_pages_driver.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("steps ok") == 8 and "exhaustion ok" in run.stdout


def test_the_book_lives_in_one_place():
    """The searches keep no page book of their own: reference counts appear in beam_pages.hpp only, and the session reports an
    empty pool as an error instead of asserting."""
    for name in os.listdir(CSRC):
        text = open(os.path.join(CSRC, name), errors="replace").read() if name.endswith((".hip", ".hpp")) else ""
        assert name == "beam_pages.hpp" or "refcnt" not in text, name
        assert "bpin" not in text, name
    assert "assert(" not in open(os.path.join(CSRC, "engine_refill.hip")).read()
