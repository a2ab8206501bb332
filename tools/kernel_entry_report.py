"""How every kernel of the decode chain ENTERS (CPU only: needs hipcc, no GPU).

Compiles kernels_skinny / _misc / _attn / _decode.hip to gfx950 assembly with the Makefile's flags (CXXFLAGS + PRELOAD) and
prints, per kernel:
  kernarg   bytes of the kernel-argument segment
  preload   argument dwords that arrive preloaded in SGPRs (.amdhsa_user_sgpr_kernarg_preload_length)
  s_loads   scalar loads from the kernarg segment issued after the compatibility prologue, up to the first vector memory
            instruction / in the whole kernel
  wait      whether an s_waitcnt that waits on lgkmcnt stands between the kernel's entry and its first vector memory
            instruction ("yes": every wave pays a scalar round trip before its first address exists)
Usage:  python tools/kernel_entry_report.py [--only REGEX] [--files kernels_misc ...] [--keep-asm DIR | --asm-dir DIR]
The non-GPU test tests/test_kernel_entry_report.py asserts wait == "no" for the headline instantiations."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taiwan_tongues_asr_ce_amd", "csrc")
FILES = ("kernels_skinny", "kernels_misc", "kernels_attn", "kernels_decode")
VMEM = re.compile(r"^\s*(global_|buffer_|flat_|scratch_)(load|store|atomic)")
SLOAD_KERNARG = re.compile(r"^\s*s_load_dword\w*\s+\S+\s+s\[0:1\]")
WAIT_LGKM = re.compile(r"^\s*s_waitcnt\b.*lgkmcnt\(\d+\)")


def make_var(name):
    """Value of a `NAME ?= value` line of the Makefile."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(rf"{name}\s*\?=\s*(.*)", line)
            if m:
                return m.group(1).strip()
    raise KeyError(name)


def hipcc():
    return os.environ.get("HIPCC") or make_var("HIPCC")


def flags():
    cxx = make_var("CXXFLAGS").replace("$(ARCH)", make_var("ARCH")).replace("$(EXTRA)", "")
    return cxx.split() + make_var("PRELOAD").split()


def compile_asm(name, out_dir):
    out = os.path.join(out_dir, name + ".s")
    cmd = [hipcc()] + flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=os.path.dirname(hipcc()) + os.pathsep + "/opt/rocm/llvm/bin" + os.pathsep + os.environ.get("PATH", "")) \
        or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def parse(asm_path):
    """[{name, kernarg, preload, loads_before, loads_total, wait}] for every kernel of one assembly file."""
    with open(asm_path) as f:
        lines = f.read().splitlines()
    desc = {}
    cur = None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = desc.setdefault(m.group(1), {})
            continue
        if cur is not None:
            m = re.match(r"\s*\.amdhsa_(kernarg_size|user_sgpr_kernarg_preload_length)\s+(\d+)", ln)
            if m:
                cur[m.group(1)] = int(m.group(2))
            elif ".end_amdhsa_kernel" in ln:
                cur = None
    out = []
    for name, dsc in desc.items():
        try:
            start = lines.index(next(l for l in lines if l.startswith(name + ":")))
        except StopIteration:
            continue
        body = []
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            body.append(ln)
        # the compatibility prologue (firmware without preload) loads the preloaded dwords itself and branches over the padding:
        # the kernel proper starts behind the `.p2align 8` that follows that branch
        first = 0
        if dsc.get("user_sgpr_kernarg_preload_length", 0):
            for i, ln in enumerate(body[:40]):
                if re.match(r"\s*\.p2align\s+8", ln):
                    first = i + 1
                    break
        loads_before = loads_total = 0
        wait = False
        seen_vmem = False
        for ln in body[first:]:
            if SLOAD_KERNARG.match(ln):
                loads_total += 1
                if not seen_vmem:
                    loads_before += 1
            if not seen_vmem:
                if WAIT_LGKM.match(ln):
                    wait = True
                if VMEM.match(ln):
                    seen_vmem = True
        out.append(dict(name=name, kernarg=dsc.get("kernarg_size", -1), preload=dsc.get("user_sgpr_kernarg_preload_length", 0),
                        loads_before=loads_before, loads_total=loads_total, wait=("yes" if wait else "no") if seen_vmem else "-"))
    return out


def report(files=FILES, only=None, keep=None, asm_dir=None):
    """asm_dir: read <file>.s from there instead of compiling (the assembly of another commit, kept with --keep-asm)."""
    tmp = keep or tempfile.mkdtemp(prefix="ttasr_entry_")
    os.makedirs(tmp, exist_ok=True)
    rows = []
    try:
        with ThreadPoolExecutor(max_workers=4) as pool:   # the compiler runs in child processes: one thread per file
            asm = list(pool.map(lambda f: os.path.join(asm_dir, f + ".s") if asm_dir else compile_asm(f, tmp), files))
        for f, path in zip(files, asm):
            for r in parse(path):
                r["file"] = f
                rows.append(r)
    finally:
        if not keep:
            shutil.rmtree(tmp, ignore_errors=True)
    names = demangle([r["name"] for r in rows])
    for r in rows:
        r["pretty"] = re.sub(r"^void |\(.*$", "", names[r["name"]])
    if only:
        rows = [r for r in rows if re.search(only, r["pretty"])]
    return sorted(rows, key=lambda r: (r["file"], r["pretty"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", nargs="*", default=list(FILES))
    ap.add_argument("--only", default=None, help="regular expression on the demangled kernel name")
    ap.add_argument("--keep-asm", default=None, metavar="DIR")
    ap.add_argument("--asm-dir", default=None, metavar="DIR", help="parse DIR/<file>.s (written by --keep-asm) instead of compiling")
    a = ap.parse_args()
    rows = report(a.files, a.only, a.keep_asm, a.asm_dir)
    print(f"{'file':15s} {'kernarg':>7s} {'preload':>7s} {'s_loads':>9s} {'wait':>4s}  kernel")
    for r in rows:
        print(f"{r['file']:15s} {r['kernarg']:7d} {r['preload']:7d} {r['loads_before']:4d}/{r['loads_total']:<4d} {r['wait']:>4s}  {r['pretty']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
