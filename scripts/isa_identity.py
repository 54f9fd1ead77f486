#!/usr/bin/env python3
"""Same machine code?  Compares the gfx950 assembly listings of the three constitutive translation units of a git revision with the working tree's.

usage: scripts/isa_identity.py REV [--voce-only]

REV's exaconstit_amd/csrc and include are exported with `git archive` into a temporary directory; both sides are compiled with
`hipcc -S --cuda-device-only` and the FLAGS + MODEL_FLAGS their own Makefile gives (`make -pn`), at most 6 compilers at a time.  No GPU is needed.
Per unit the result is `identical` or the first differing kernel symbol and line; exit status 0 only if all three are identical.
--voce-only leaves the Kocks-Mecking instantiations out (-DEXA_VARIANT_VOCE_ONLY: a quarter of the time, for work in progress).

Compare listings, not objects: the bundled object files differ in their wrapper even where the code is the same.  One symbol of a listing is no code and
is masked: __hip_cuid_<hash>, a one-byte marker named after a hash of the source file's PATH, which differs between the two directories by construction.
"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ["model_kernels", "model_kernels_aos", "model_kernels_p2"]
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def make_vars(csrc):
    """HIPCC and the expanded FLAGS + MODEL_FLAGS from the Makefile's own data base"""
    db = subprocess.run(["make", "-pn", "-C", csrc, "TUNE="], capture_output=True, text=True).stdout
    var = {m.group(1): m.group(2) for m in re.finditer(r"^([A-Za-z_]+) [:?]?= ?(.*)$", db, re.M)}
    def expand(v):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), v)
    return expand(var["HIPCC"]), (expand(var["FLAGS"]) + " " + expand(var["MODEL_FLAGS"])).split()


def listing(job):
    csrc, unit, out, extra = job
    hipcc, flags = make_vars(csrc)
    subprocess.run([hipcc] + flags + extra + ["-S", "--cuda-device-only", unit + ".hip", "-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return out


def compare(a, b):
    """None if the listings agree, else (kernel symbol, line number, line counts)"""
    la, lb = open(a).read().split("\n"), open(b).read().split("\n")
    sym = "(before the first symbol)"
    for i, (x, y) in enumerate(zip(la, lb)):
        if CUID.sub("__hip_cuid", x) != CUID.sub("__hip_cuid", y): return sym, i + 1, len(la) - 1, len(lb) - 1
        m = re.match(r"^(\w+):", x)
        if m: sym = m.group(1)
    return None if len(la) == len(lb) else (sym, min(len(la), len(lb)), len(la) - 1, len(lb) - 1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1: sys.exit(__doc__)
    rev, extra = args[0], (["-DEXA_VARIANT_VOCE_ONLY"] if "--voce-only" in sys.argv else [])
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, "exaconstit_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        sides = {"rev": os.path.join(tmp, "exaconstit_amd", "csrc"), "tree": os.path.join(ROOT, "exaconstit_amd", "csrc")}
        jobs = [(csrc, u, os.path.join(tmp, "%s_%s.s" % (u, side)), extra) for side, csrc in sides.items() for u in UNITS]
        with ThreadPoolExecutor(max_workers=6) as pool: list(pool.map(listing, jobs))
        print("%s against the working tree%s (listings of hipcc -S --cuda-device-only, __hip_cuid_<path hash> masked)" % (rev, ", Voce instantiations only" if extra else ""))
        bad = 0
        for u in UNITS:
            a, b = os.path.join(tmp, u + "_rev.s"), os.path.join(tmp, u + "_tree.s")
            d = compare(a, b)
            if d is None: print("%-18s identical   %d lines both" % (u, len(open(a).read().split("\n")) - 1))
            else: bad += 1; print("%-18s DIFFERS     first at line %d, in %s   (%d against %d lines)" % (u, d[1], d[0], d[2], d[3]))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
