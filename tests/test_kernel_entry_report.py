"""Non-GPU: the headline decode kernels issue their first vector load without waiting for a kernel-argument fetch.

tools/kernel_entry_report.py compiles the kernel files to gfx950 assembly (hipcc only, no GPU) and reports, per kernel, the
argument dwords that arrive preloaded and whether an s_waitcnt on lgkmcnt stands between entry and the first vector memory
instruction.  The instantiations below are the ones the benchmark's greedy step launches (large-v3, 32 rows, bf16).
kernels_skinny.hip takes about a minute to compile; the two files are compiled once for the module.  Skipped without hipcc."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_entry_report", os.path.join(ROOT, "tools", "kernel_entry_report.py"))
ker = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ker)

HEADLINE = {
    "kernels_misc": ["layernorm_rows_kernel<unsigned short, 4, false>", "layernorm_rows_kernel<unsigned short, 8, false>"],
    "kernels_skinny": ["gemm_skinny_kernel<unsigned short, 4, 1, 4, true, true>", "gemm_skinny_kernel<unsigned short, 4, 1, 5, true, true>",
                       "gemm_skinny_kernel<unsigned short, 4, 1, 10, true, true>", "gemm_skinny_kernel<unsigned short, 8, 1, 10, true, true>",
                       "gemm_vocab_kernel<unsigned short, 1, true>"],
    "kernels_attn": ["cross_attn_pipe_kernel<unsigned short, true, true, 3>"],
}


def _hipcc():
    path = ker.hipcc()
    return path if os.path.exists(path) else shutil.which("hipcc")


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if not _hipcc():
        pytest.skip("hipcc is not installed")
    os.environ.setdefault("HIPCC", _hipcc())
    got = ker.report(files=tuple(HEADLINE), keep=str(tmp_path_factory.mktemp("asm")))
    return {(r["file"], r["pretty"]): r for r in got}


@pytest.mark.parametrize("file,kernel", [(f, k) for f, ks in HEADLINE.items() for k in ks])
def test_first_vector_load_waits_for_no_argument_fetch(rows, file, kernel):
    r = rows.get((file, kernel))
    assert r is not None, f"{kernel}: not in {file}.hip's assembly ({sorted(k for f, k in rows if f == file)[:8]} ...)"
    assert r["wait"] == "no", r
    assert r["loads_before"] <= 1 and r["preload"] >= 12, r
