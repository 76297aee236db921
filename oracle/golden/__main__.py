"""python -m oracle.golden [names...]: regenerate the fixtures of tests/golden/ (all of them without names) in dependency order, each generator in an
interpreter of its own, so that none sees what another patched or drew.  --check regenerates into a temporary directory and compares with the committed files."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

from . import reference
from .registry import BY_NAME, GENERATORS, ordered

REPO = reference.REPO


def compare(new, old):
    """'identical', 'same arrays' (an .npz whose members agree in key, dtype, shape and bytes: only the container differs) or 'DIFFERENT (where)'."""
    if not os.path.exists(old):
        return "DIFFERENT (not in the tree)"
    if open(new, "rb").read() == open(old, "rb").read():
        return "identical"
    if not new.endswith(".npz"):
        return "DIFFERENT (bytes)"
    a, b = np.load(new), np.load(old)
    for ka, kb in zip(a.files, b.files):
        if ka != kb or a[ka].dtype != b[kb].dtype or a[ka].shape != b[kb].shape or a[ka].tobytes() != b[kb].tobytes():
            return f"DIFFERENT ({ka})"
    if len(a.files) != len(b.files):
        return f"DIFFERENT ({(a.files + b.files)[min(len(a.files), len(b.files))]})"
    return "same arrays"


def run(g, ref, dst, check):
    """One generator in a child interpreter.  Its needs come from `dst` where they all are there already, else from the tree; under --check from the tree alone."""
    for d in ("tests/golden", "weights"):
        os.makedirs(os.path.join(dst, d), exist_ok=True)
    src = dst if not check and all(os.path.exists(os.path.join(dst, n)) for n in g.needs) else REPO
    r = subprocess.run([sys.executable, "-m", "oracle.golden", g.name, "--reference", ref, "--out", dst, "--in-process", src], cwd=REPO,
                       capture_output=check, text=True)
    if r.returncode:
        sys.exit(f"{r.stdout or ''}{r.stderr or ''}oracle.golden: generator {g.name} failed")


def main():
    ap = argparse.ArgumentParser(prog="python -m oracle.golden", description=__doc__)
    ap.add_argument("names", nargs="*", metavar="name", help="generators to run (see --list); all of them if none is given")
    ap.add_argument("--reference", metavar="DIR", help="the reference project's directory; else $RADAE_REFERENCE, else /root/reference")
    ap.add_argument("--list", action="store_true", help="print generator, outputs and needs, and stop")
    ap.add_argument("--out", metavar="DIR", default=REPO, help="write DIR/tests/golden/... instead of into the tree")
    ap.add_argument("--check", action="store_true", help="regenerate into a temporary directory and compare with the committed files")
    ap.add_argument("--in-process", metavar="SRC", help=argparse.SUPPRESS)      # the child: run the one named generator here, needs read from SRC
    args = ap.parse_args()
    if args.list:
        for g in GENERATORS:
            print(f"{g.name}\n  writes " + "\n         ".join(g.outputs) + ("\n  needs  " + "\n         ".join(g.needs) if g.needs else ""))
        return
    unknown = [n for n in args.names if n not in BY_NAME]
    if unknown:
        ap.error(f"no such generator: {' '.join(unknown)} (see --list)")
    ref = reference.find(args.reference)
    if args.in_process:
        return BY_NAME[args.names[0]].run(args.in_process, args.out)
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for g in ordered(args.names):
            run(g, ref, tmp if args.check else os.path.abspath(args.out), args.check)
            for o in g.outputs if args.check else ():
                verdict = compare(os.path.join(tmp, o), os.path.join(REPO, o))
                bad += verdict.startswith("DIFFERENT")
                print(f"{o}: {verdict}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
