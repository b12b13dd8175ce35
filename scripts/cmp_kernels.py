#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  (CPU only.)

usage: cmp_kernels.py PARENT.out NEW.out
       cmp_kernels.py PARENT.out [PARENT.out ...] -- NEW.out [NEW.out ...]
  the linked gfx950 code objects that `make isa` leaves in build/isa/
  (<unit>-hip-amdgcn-amd-amdhsa-gfx950.out) of two checkouts; a set on either
  side when one checkout keeps in several translation units what the other
  keeps in one.

Disassembles them with llvm-objdump and compares the instruction text kernel
by kernel, matched by name over the union of each side, addresses aside (a
kernel added to a file moves every other one, renumbers the assembly's labels
and renames the generated __hip_cuid, so the .s files themselves never
compare equal).  A kernel of the parent that is missing from the new set, or
that either set holds twice, fails.  Two differences are allowed, both of
addresses only, and counted:
  1. trailing `s_nop 0` / `...` lines behind a function's last instruction
     (the assembler's padding, which depends on what follows the function);
  2. the 32-bit literals of the s_add_u32 / s_addc_u32 pair that directly
     follows a pc read (s_getpc_b64) of the same register pair: the
     pc-relative distance to a variable of the code object.
Everything else compares exactly: other literals, any register, any opcode,
any order.  Prints the kernels that differ, went missing or are doubled, then
one line of totals; exit status 1 if any did.
"""
import os
import re
import subprocess
import sys

OBJDUMP = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def parse(txt):
    """llvm-objdump -d text -> {function: [instruction lines, address comments removed]}"""
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


def funcs(path):
    return parse(subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout)


def union(sets):
    """Several code objects' functions as one -> ({function: lines}, the names held more than once)"""
    out, doubled = {}, set()
    for s in sets:
        for k, v in s.items():
            if k in out:
                doubled.add(k)
            out[k] = v
    return out, doubled


def unpadded(lines):
    n = len(lines)
    while n and lines[n - 1] in ("s_nop 0", "..."):
        n -= 1
    return lines[:n]


def _pc_literal(lines, i):
    """Line i with its literal blanked if it is the s_add_u32 or the s_addc_u32 behind a pc read, else None."""
    m = re.match(r"^(s_add_u32|s_addc_u32) s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$", lines[i])
    if not m or m.group(2) != m.group(3):
        return None
    lo = int(m.group(2))
    if m.group(1) == "s_addc_u32":  # the pair's high half: behind the low half's add
        lo -= 1
        i -= 1
        if i < 0 or not re.match(r"^s_add_u32 s%d, s%d, (0x[0-9a-f]+|-?\d+)$" % (lo, lo), lines[i]):
            return None
    if i < 1 or lines[i - 1] != "s_getpc_b64 s[%d:%d]" % (lo, lo + 1):
        return None
    return "%s s%s, s%s" % m.group(1, 2, 3)


def compare(a, b):
    """Two functions' lines -> (the same code?, pc-relative literals that differ, trailing padding differs?)"""
    ua, ub = unpadded(a), unpadded(b)
    padding = len(a) - len(ua) != len(b) - len(ub)
    if len(ua) != len(ub):
        return False, 0, padding
    literals = 0
    for i, (x, y) in enumerate(zip(ua, ub)):
        if x == y:
            continue
        px = _pc_literal(ua, i)
        if px is None or px != _pc_literal(ub, i):
            return False, literals, padding
        literals += 1
    return True, literals, padding


def compare_sets(parents, news, out=sys.stdout):
    """Lists of {function: lines} -> the number of parent functions that differ, are missing or doubled."""
    a, da = union(parents)
    b, db = union(news)
    same = bad = literals = padded = 0
    for k in sorted(da):
        print("TWICE in parent:", k, file=out)
        bad += 1
    for k in sorted(db):
        print("TWICE in new:", k, file=out)
        bad += 1
    for k in sorted(a):
        if k in da or k in db:
            continue
        if k not in b:
            print("MISSING in new:", k, file=out)
            bad += 1
            continue
        ok, lit, pad = compare(a[k], b[k])
        if not ok:
            ua, ub = unpadded(a[k]), unpadded(b[k])
            n = sum(1 for x, y in zip(ua, ub) if x != y) + abs(len(ua) - len(ub))
            print("DIFFERS:", k, "-", n, "of", len(ua), "lines", file=out)
            bad += 1
            continue
        same += 1
        literals += lit
        padded += pad
        if lit:
            print("pc-relative literals:", k, "-", lit, file=out)
    print("identical: %d, different: %d, only in new: %s; allowed: %d pc-relative literals, %d functions' trailing padding"
          % (same, bad, sorted(set(b) - set(a)), literals, padded), file=out)
    return bad


def main(argv):
    if "--" in argv:
        i = argv.index("--")
        parents, news = argv[:i], argv[i + 1:]
    else:
        parents, news = argv[:1], argv[1:]
    if not parents or not news or ("--" not in argv and len(argv) != 2):
        sys.exit(__doc__)
    return 1 if compare_sets([funcs(p) for p in parents], [funcs(p) for p in news]) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
