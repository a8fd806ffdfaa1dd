#!/usr/bin/env python3
"""Is the device code of two builds the same?  For every object of two csrc/obj directories: the embedded gfx950 code
object (.hip_fatbin section -> clang-offload-bundler), then sha256 of its .text, sha256 of its .rodata (the kernel
descriptors) and the sorted list of kernel symbols.  Whole code objects are NOT compared: each embeds a compilation-unit
id derived from the source text.  The check for a host-only change (needs no GPU).

    python tools/code_identity.py PARENT_OBJ_DIR BRANCH_OBJ_DIR > profiles/<name>_code_identity.txt

Exit status 1 if any unit differs.
"""
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def unit(obj, tmp):
    """-> (sha256 .text, sha256 .rodata, [kernel symbols]); a unit without device code: ('-', '-', [])"""
    fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return "-", "-", []
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    if os.path.getsize(co) == 0:
        return "-", "-", []
    sums = []
    for sec in (".text", ".rodata"):
        out = os.path.join(tmp, "sec")
        if os.path.exists(out):
            os.remove(out)
        run(f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={sec}", co, out)
        sums.append(hashlib.sha256(open(out, "rb").read()).hexdigest() if os.path.exists(out) else "-")
    kernels = sorted(line.split()[-1][:-3] for line in run(f"{LLVM}/llvm-objdump", "--syms", co).splitlines()
                     if line.endswith(".kd"))   # (every kernel has a descriptor symbol <name>.kd)
    return sums[0], sums[1], kernels


def main(parent, branch):
    names = sorted({f for d in (parent, branch) for f in os.listdir(d) if f.endswith(".o")})
    differ = 0
    print(f"{'unit':24s} {'kernels':>7s}  {'.text sha256':16s}  {'.rodata sha256':16s}  parent == branch (.text / .rodata / kernel symbols)")
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            sides = []
            for d in (parent, branch):
                path = os.path.join(d, name)
                sides.append(unit(path, tmp) if os.path.exists(path) else None)
            a, b = sides
            if a is None or b is None:
                differ += 1
                print(f"{name:24s} only in the {'branch' if a is None else 'parent'} build: DIFFERENT")
                continue
            same = [a[i] == b[i] for i in range(3)]
            differ += not all(same)
            verdict = " / ".join("same" if s else "DIFFERENT" for s in same)
            print(f"{name:24s} {len(b[2]):7d}  {b[0][:16]:16s}  {b[1][:16]:16s}  {verdict}")
            if not same[2]:
                for k in sorted(set(a[2]) ^ set(b[2])):
                    print(f"    {'parent only' if k in a[2] else 'branch only'}: {k}")
    print(f"{len(names)} translation units, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
