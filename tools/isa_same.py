"""Do two builds hold the same machine code?  Compares two directories of listings written by tools/check_lds_flat.py --keep:
every function's instructions and every kernel's .amdhsa_* block (registers, LDS, scratch ...), function by function.
Functions are paired by symbol, not by file, so one that moved to another translation unit still meets its counterpart;
a symbol that several listings of a directory define (the stream walk is compiled five times) is told apart by the first
kernel of its listing.  Comments are dropped and local labels (.LBB<i>_<j>, .Lfunc_*, .LJTI ...) renumbered per function in
order of appearance.  Prints the symbols that differ or have no counterpart; exit code 1 if there are any.
  python tools/isa_same.py DIR_A DIR_B"""
import glob
import os
import re
import sys
from collections import Counter


def functions(path):
    """{symbol: [normalised lines]} of one listing, kernels' descriptor blocks appended to their code; and its kernels in order"""
    fns, kernels, cur, labels = {}, [], None, {}
    for line in open(path):
        t = line.split(";")[0].strip()
        if not t:
            continue
        m = re.match(r"\.type\s+(\S+),@function", t)
        k = re.match(r"\.amdhsa_kernel\s+(\S+)", t)
        if m or k:
            cur, labels = fns.setdefault((m or k).group(1), []), {}
            if k:
                kernels.append(k.group(1))
            continue
        if cur is None or (t.startswith(".") and not t.startswith((".L", ".amdhsa_"))):
            cur = None if t.startswith((".size", ".end_amdhsa_kernel")) else cur      # other directives: alignment, sections
            continue
        cur.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), " ".join(t.split())))
    return fns, kernels


def build(d):
    files = [functions(p) for p in sorted(glob.glob(os.path.join(d, "*.s")))]
    shared = {s for s, n in Counter(s for fns, _ in files for s in fns).items() if n > 1}
    return {s + (" [with %s]" % kernels[0] if s in shared else ""): body for fns, kernels in files for s, body in fns.items()}


def main():
    a, b = build(sys.argv[1]), build(sys.argv[2])
    bad = ["only in %s: %s" % (sys.argv[1 + (s in b)], s) for s in sorted(set(a) ^ set(b))]
    for s in sorted(set(a) & set(b)):
        if a[s] != b[s]:
            i = next((i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y), min(len(a[s]), len(b[s])))
            bad.append("differs: %s (%d / %d lines, first at %d: %r / %r)" % (s, len(a[s]), len(b[s]), i, a[s][i:i + 1], b[s][i:i + 1]))
    print("\n".join(bad) if bad else "isa_same: %d functions, all the same" % len(a))
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
