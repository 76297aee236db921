#!/usr/bin/env python3
"""Does a source-only change leave the compiled gfx950 code alone?  Compares two builds of the library (the parent commit's and the working tree's):
every device function's instruction text (addresses, encodings and trailing comments stripped), every kernel's register / scratch / LDS figures
(the code objects' metadata notes) and the exported symbols.  Needs no GPU.  Exit status 1 if anything differs.  --lds-offsets: a change that moves
members of an LDS structure may change the offset immediates of LDS instructions, and nothing else.

    tools/ab_build_base.sh HEAD && python tools/codegen_diff.py ab/base.so radae_amd/libradehip.so [--show N] [--lds-offsets]
"""
import difflib
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_spill_exec import LLVM, SYM, disassemble


def functions(lib, lds_offsets=False):
    """-> {symbol: [instruction text]} over all code objects of the library"""
    out, cur = {}, None
    for line in disassemble(lib).split("\n"):
        m = SYM.match(line)
        if m:
            cur = out.setdefault(m.group(2), [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            ins = " ".join(line.split("//")[0].split())
            cur.append(re.sub(r"offset([01]?):\d+", r"offset\1:*", ins) if lds_offsets and ins.startswith("ds_") else ins)
    for ins in out.values():          # the padding up to the next function's alignment is not the function's
        while ins and ins[-1] in ("s_nop 0", "s_code_end"):
            ins.pop()
    return out


def resources(lib):
    """-> the lines 'kernel vgpr .. spill .. scratch .. static-lds ..' that tools/kernel_resources.py prints, sorted"""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_resources.py"), lib], check=True, capture_output=True, text=True)
    return sorted(" ".join(l.split()) for l in r.stdout.splitlines() if l.strip())


def exported(lib):
    r = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", lib], check=True, capture_output=True, text=True)
    rows = [l.split() for l in r.stdout.splitlines()]
    return sorted(f[7] for f in rows if len(f) == 8 and f[0].rstrip(":").isdigit() and f[6] != "UND")


def main():
    a, b = sys.argv[1], sys.argv[2]
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 0
    bad = 0
    fa, fb = functions(a, "--lds-offsets" in sys.argv), functions(b, "--lds-offsets" in sys.argv)
    for s in sorted(set(fa) | set(fb)):
        if fa.get(s) == fb.get(s):
            continue
        bad += 1
        d = [l for l in difflib.unified_diff(fa.get(s, []), fb.get(s, []), lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print(f"{s}: {len(fa.get(s, []))} -> {len(fb.get(s, []))} instructions, {len(d)} differing lines")
        for l in d[:show]:
            print("   ", l)
    ra, rb = resources(a), resources(b)
    if ra != rb:
        bad += 1
        for l in difflib.unified_diff(ra, rb, a, b, lineterm="", n=0):
            print("resources:", l)
    ea, eb = exported(a), exported(b)
    if ea != eb:
        bad += 1
        print("exported symbols: only in", a, sorted(set(ea) - set(eb)), "only in", b, sorted(set(eb) - set(ea)))
    print(f"{len(fa)} / {len(fb)} device functions, {len(ra)} / {len(rb)} kernels, {len(ea)} / {len(eb)} exported symbols: {'IDENTICAL' if not bad else f'{bad} difference(s)'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
