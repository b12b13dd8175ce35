#!/usr/bin/env python3
"""Are the kernels of two builds of one .hip file the same code?  (CPU only.)

usage: cmp_kernels.py PARENT.out NEW.out
  the linked gfx950 code objects that `make isa` leaves in build/isa/
  (rt_kernel-hip-amdgcn-amd-amdhsa-gfx950.out) of two checkouts.

Disassembles both with llvm-objdump and compares the instruction text kernel
by kernel, addresses aside (a kernel added to the file moves every other one,
renumbers the assembly's labels and renames the generated __hip_cuid, so the
.s files themselves never compare equal).  Prints the kernels that differ or
went missing, then one line of totals; exit status 1 if any did.
"""
import os
import re
import subprocess
import sys

OBJDUMP = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def funcs(path):
    txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        out[cur].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:.*$", "", line).strip())  # (the address comment)
    return out


def main():
    a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
    same = diff = 0
    for k in sorted(a):
        if k not in b:
            print("MISSING in new:", k)
            diff += 1
        elif a[k] != b[k]:
            n = sum(1 for x, y in zip(a[k], b[k]) if x != y) + abs(len(a[k]) - len(b[k]))
            print("DIFFERS:", k, "-", n, "of", len(a[k]), "lines")
            diff += 1
        else:
            same += 1
    print("identical: %d, different: %d, only in new: %s" % (same, diff, sorted(set(b) - set(a))))
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
