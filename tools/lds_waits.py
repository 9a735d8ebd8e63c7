"""Where a kernel waits for LDS: for a unit of hmp3_amd/csrc/hx_units.tab, compiled to assembly with the table's flags (as
tools/check_lds_flat.py does; hipcc cross-compiles without a GPU), the sequence of LDS reads, LDS writes, waits on lgkmcnt
and branches of every function and of every loop the compiler marks in it.  A line loop that is meant to have all its
reads in flight together shows as one block "RRRRRRRR:"; one the compiler split by a run-time guard shows as sibling
blocks "RR:" "RR:" "RR:", each paying the LDS round trip on its own.
  R  ds_read*        W  ds_write*      A  other ds_* (atomics, swizzles, bpermute)
  :  s_waitcnt with lgkmcnt(0)         .  s_waitcnt with lgkmcnt(n > 0)
  b  branch          c  call           |  basic block boundary
"siblings": basic blocks that hold nothing of LDS but their own reads and the full wait that ends them ("RR:", ":RR:b")
and have a neighbour of that shape next to them in the listing (blocks without LDS instructions or waits in between do not
count as separation).  It reads ds_* and s_waitcnt mnemonics only: scalar loads that share lgkmcnt are not shown.
  python tools/lds_waits.py UNIT [UNIT ...] [--functions REGEX] [--keep DIR | --from DIR]
(--keep DIR leaves the listings in DIR; --from DIR reads DIR/<unit>.s, listings kept by an earlier run, without compiling)"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_lds_flat import BASE, HIPCC, SRC, UNITS

LABEL = re.compile(r"^([_A-Za-z.$][\w.$]*):")
INLOOP = re.compile(r";\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r";\s+=>\s*This (?:Inner )?Loop Header: Depth=(\d+)")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def classify(t):
    op = t.split()[0]
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "R"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "W"
    if op.startswith("ds_"):
        return "A"
    if op == "s_waitcnt":
        m = LGKM.search(t)
        if m:
            return ":" if int(m.group(1)) == 0 else "."
        return ""
    if op.startswith("s_cbranch") or op == "s_branch":
        return "b"
    if op.startswith("s_swappc") or op.startswith("s_setpc"):
        return "c"
    return ""


def parse(path):
    """[(function, [(block label, loop header or None, depth, sequence)])] in listing order"""
    funcs = []
    blocks = None
    cur = None
    for line in open(path):
        m = LABEL.match(line)
        if m:
            name = m.group(1)
            if name.startswith(".L"):
                if blocks is None or not name.startswith(".LBB"):
                    continue
                loop = INLOOP.search(line)
                cur = [name[2:], loop.group(1) if loop else None, int(loop.group(2)) if loop else 0, ""]
                blocks.append(cur)
            else:
                blocks = []
                funcs.append((name, blocks))
                cur = ["entry", None, 0, ""]
                blocks.append(cur)
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            cur = blocks = None
            continue
        if t.startswith(";"):
            fall = re.match(r";\s*%bb\.(\d+):", t)           # a block entered by falling through has no label
            if fall:
                cur = ["bb." + fall.group(1), None, 0, ""]
                blocks.append(cur)
            h = HEADER.search(t)
            loop = INLOOP.search(t)
            if h and not cur[3]:
                cur[1], cur[2] = cur[0], int(h.group(1))
            elif loop and not cur[3] and cur[1] is None:
                cur[1], cur[2] = loop.group(1), int(loop.group(2))
            continue
        if not t or t.startswith("."):
            continue
        cur[3] += classify(t)
    return funcs


READ_WAIT = re.compile(r"^[b.:]*(R+):[:.]*[bc]*$")


def siblings(blocks):
    """number of blocks of shape "own reads, then a full wait" that stand next to another of that shape"""
    shapes = []
    for label, loop, depth, seq in blocks:
        if not seq.strip("bc"):
            continue            # nothing of LDS in it: no separation
        m = READ_WAIT.match(seq)
        shapes.append(len(m.group(1)) if m else 0)
    n = 0
    for i, s in enumerate(shapes):
        if s and ((i > 0 and shapes[i - 1]) or (i + 1 < len(shapes) and shapes[i + 1])):
            n += 1
    return n


def wrap(s, width=116, indent="      "):
    return "\n".join(indent + s[i:i + width] for i in range(0, len(s), width)) if s else indent + "-"


def report(unit, path, want):
    funcs = parse(path)
    names = subprocess.run(["c++filt"], input="\n".join(f for f, b in funcs), capture_output=True, text=True).stdout.split("\n")
    print("== %s" % unit)
    for (mangled, blocks), dem in zip(funcs, names):
        name = dem.split("(")[0]
        if want and not want.search(name):
            continue
        whole = "".join(seq for l, h, d, seq in blocks)
        if not re.search("[RWA]", whole):
            continue
        print("%s: reads %d writes %d other-ds %d full-waits %d counted-waits %d branches %d siblings %d" % (
            name, whole.count("R"), whole.count("W"), whole.count("A"), whole.count(":"), whole.count("."), whole.count("b"), siblings(blocks)))
        # the function's blocks outside any loop, then loop by loop (innermost header), in listing order
        groups, order = {}, []
        for b in blocks:
            key = (b[1], b[2])
            if key not in groups:
                groups[key] = []
                order.append(key)
            groups[key].append(b)
        for key in order:
            seq = "|".join(b[3] for b in groups[key] if b[3])
            if not re.search("[RWA:.]", seq):
                continue
            head = "  straight-line" if key[0] is None else "  loop %s depth %d" % key
            print("%s: siblings %d" % (head, siblings(groups[key])))
            print(wrap(seq))


def main():
    args = sys.argv[1:]
    keep = want = have = None
    if "--keep" in args:
        keep = args[args.index("--keep") + 1]
        del args[args.index("--keep"):args.index("--keep") + 2]
    if "--from" in args:
        have = args[args.index("--from") + 1]
        del args[args.index("--from"):args.index("--from") + 2]
    if "--functions" in args:
        want = re.compile(args[args.index("--functions") + 1])
        del args[args.index("--functions"):args.index("--functions") + 2]
    table = {name: flags for name, group, flags in UNITS}
    if not args or any(u not in table for u in args):
        raise SystemExit(__doc__ + "\nunits: " + " ".join(table))
    if have:
        for unit in args:
            report(unit, os.path.join(have, unit + ".s"), want)
        return
    tmp = keep or tempfile.mkdtemp(prefix="hxwaits.")
    os.makedirs(tmp, exist_ok=True)
    procs = []
    for unit in args:
        out = os.path.join(tmp, unit + ".s")
        procs.append((unit, out, subprocess.Popen([HIPCC] + BASE + table[unit] + [unit + ".hip", "-o", out], cwd=SRC, stderr=subprocess.PIPE)))
    for unit, out, p in procs:
        err = p.communicate()[1].decode()
        if p.returncode != 0:
            print(err[-2000:], file=sys.stderr)
            raise SystemExit("lds_waits: %s did not compile" % unit)
        report(unit, out, want)


if __name__ == "__main__":
    main()
