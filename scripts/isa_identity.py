#!/usr/bin/env python3
"""Same machine code?  Compares the gfx950 assembly listings of translation units of a git revision with the working tree's, symbol by symbol.

usage: scripts/isa_identity.py REV [--voce-only] [--units=UNIT[,UNIT...]]

REV's exaconstit_amd/csrc and include are exported with `git archive` into a temporary directory; both sides are compiled with
`hipcc -S --cuda-device-only` and the flags their own Makefile gives (`make -pn`: FLAGS, and MODEL_FLAGS for the constitutive units), at most 6
compilers at a time.  No GPU is needed.  --units names the units (file names under csrc without .hip); the default is the three constitutive ones.
A listing is cut into its symbols - a function from its section line to the resource comments behind it, together with its entry in the kernel
metadata - plus what stands before the first and behind the last function.  Per unit the result is `identical`, or the symbols that differ (with the
first differing line) and the symbols that only one side has: a removed kernel shows as `only in REV`, not as a difference in its neighbour.
Exit status 0 only if every symbol present on both sides is identical.
--voce-only leaves the Kocks-Mecking instantiations out (-DEXA_VARIANT_VOCE_ONLY: a quarter of the time, for work in progress).

Compare listings, not objects: the bundled object files differ in their wrapper even where the code is the same.  Masked, because they are no code:
__hip_cuid_<hash>, a one-byte marker named after a hash of the source file's PATH, which differs between the two directories by construction, and the
running number of the function in its local labels and loop comments (.LBB<n>_<m>, .Lfunc_end<n>, Header=BB<n>_<m>), which shifts behind a
removed function - and with it the padding in front of a block label's loop comment, which the assembly printer aligns to a column: a label whose
function number gains a digit (functions ADDED in front of it) gets one space less.
"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ["model_kernels", "model_kernels_aos", "model_kernels_p2"]
MODEL_UNITS = set(UNITS)
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
FN_LABEL = re.compile(r"\.L(func_begin|func_end|[A-Za-z]+)\d+(_\d+)?\b")
LOOP_NOTE = re.compile(r"\bBB\d+(_\d+)\b")      # the block names in the loop comments ("in Loop: Header=BB<n>_<m>")
LABEL_PAD = re.compile(r"^(\.L\w+:)\s+;")      # block label, padding, loop comment
BEGIN = re.compile(r"-- Begin function (\S+)")


def make_vars(csrc, unit):
    """HIPCC and the expanded flags of the unit from the Makefile's own data base"""
    db = subprocess.run(["make", "-pn", "-C", csrc, "TUNE="], capture_output=True, text=True).stdout
    var = {m.group(1): m.group(2) for m in re.finditer(r"^([A-Za-z_]+) [:?]?= ?(.*)$", db, re.M)}
    def expand(v):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), "")), v)
    return expand(var["HIPCC"]), (expand(var["FLAGS"]) + (" " + expand(var["MODEL_FLAGS"]) if unit in MODEL_UNITS else "")).split()


def listing(job):
    csrc, unit, out, extra = job
    hipcc, flags = make_vars(csrc, unit)
    subprocess.run([hipcc] + flags + extra + ["-S", "--cuda-device-only", unit + ".hip", "-o", out], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return out


def mask(line):
    return LABEL_PAD.sub(r"\1 ;", LOOP_NOTE.sub(r"BB\1", FN_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), CUID.sub("__hip_cuid", line))))


def symbols(path):
    """{symbol: masked lines} of a listing, in order; '(header)' and '(trailer)' hold what belongs to no function"""
    lines = [mask(l) for l in open(path).read().split("\n")]
    meta = lines.index("\t.amdgpu_metadata") if "\t.amdgpu_metadata" in lines else len(lines)
    starts = []
    for i, l in enumerate(lines[:meta]):
        m = BEGIN.search(l)
        if m: starts.append((i - 1 if i > 0 and lines[i - 1].startswith("\t.section") else i, m.group(1)))
    fill = [i for i, l in enumerate(lines[:meta]) if l.startswith("\t.p2alignl")]      # (the padding behind the last function opens the trailer)
    end = (fill[-1] - 1 if lines[fill[-1] - 1] == "\t.text" else fill[-1]) if fill and starts and fill[-1] > starts[-1][0] else meta
    out = {"(header)": lines[:starts[0][0]] if starts else lines[:end]}
    for k, (i, name) in enumerate(starts):
        out.setdefault(name, []).extend(lines[i:starts[k + 1][0] if k + 1 < len(starts) else end])
    out["(trailer)"] = lines[end:meta]
    # kernel metadata: one YAML entry per kernel, '  - ' at the start of its first line
    entry, rest = [], []
    def flush():
        name = next((l.split(":", 1)[1].strip() for l in entry if l.startswith("    .name:")), None)
        if name: out.setdefault(name, []).extend(entry)
        else: rest.extend(entry)
    for l in lines[meta:]:
        if l.startswith("  - ") or not l.startswith("    "): flush(); entry = []
        entry.append(l)
    flush()
    out["(trailer)"] += rest
    return out


def compare(a, b):
    """(symbols that differ: [(symbol, first differing line of the symbol)], only in a, only in b, number of symbols on both sides)"""
    sa, sb = symbols(a), symbols(b)
    diff = []
    for name in sa:
        if name in sb and sa[name] != sb[name]:
            n = next((i for i, (x, y) in enumerate(zip(sa[name], sb[name])) if x != y), min(len(sa[name]), len(sb[name])))
            diff.append((name, n + 1))
    return diff, [n for n in sa if n not in sb], [n for n in sb if n not in sa], sum(n in sb for n in sa)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1: sys.exit(__doc__)
    rev, extra = args[0], (["-DEXA_VARIANT_VOCE_ONLY"] if "--voce-only" in sys.argv else [])
    units = next((a.split("=", 1)[1].split(",") for a in sys.argv[1:] if a.startswith("--units=")), UNITS)
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, "exaconstit_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        sides = {"rev": os.path.join(tmp, "exaconstit_amd", "csrc"), "tree": os.path.join(ROOT, "exaconstit_amd", "csrc")}
        jobs = [(csrc, u, os.path.join(tmp, "%s_%s.s" % (u, side)), extra) for side, csrc in sides.items() for u in units]
        with ThreadPoolExecutor(max_workers=6) as pool: list(pool.map(listing, jobs))
        print("%s against the working tree%s (listings of hipcc -S --cuda-device-only, symbol by symbol; __hip_cuid_<path hash> and the function numbers of local labels masked)"
              % (rev, ", Voce instantiations only" if extra else ""))
        bad = 0
        for u in units:
            diff, only_rev, only_tree, both = compare(os.path.join(tmp, u + "_rev.s"), os.path.join(tmp, u + "_tree.s"))
            bad += len(diff)
            print("%-18s %s   %d symbols on both sides%s" % (u, "DIFFERS  " if diff else "identical", both, "" if not diff else ", %d differ" % len(diff)))
            for name, n in diff: print("   differs      %s   (first at line %d of the symbol)" % (name, n))
            for name in only_rev: print("   only in REV  %s" % name)
            for name in only_tree: print("   only in tree %s" % name)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
