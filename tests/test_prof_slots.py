"""The stream walk's profile slots (enum HxProf, hx_types.h) are the one table the kernels and the profile tools share."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "hmp3_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import prof_slots  # noqa: E402

TOOLS = ("gpu_prof.py", "gpu_prof_bench.py", "gpu_prof_overlap.py", "prof_outlier.py")


def test_slots_are_unique_and_fit_the_profile_block():
    m = prof_slots.members()
    assert len(m) > 40
    values = [v for _, v in m]
    assert len(set(values)) == len(values), "two members share a slot"
    assert all(0 <= v < 64 for v in values)
    names = prof_slots.slots()
    assert len(set(names.values())) == len(names)
    assert names[31] == "total" and prof_slots.slot("n_sweeps_helper") == 45


def test_every_slot_the_kernels_book_is_an_enum_member():
    members = {m for m, _ in prof_slots.members()}
    used = set()
    for f in sorted(os.listdir(SRC)):
        if not f.endswith((".hip", ".inc", ".h")):
            continue
        src = open(os.path.join(SRC, f)).read()
        for macro in re.finditer(r"\bPROF(?:_ACC|_CNT)?\(\s*([^,)]+)", src):
            used.add((f, macro.group(1).strip()))
        for idx in re.finditer(r"\bL\.prof\[([^\]]+)\]", src):
            used.add((f, idx.group(1).strip()))
    # (the macros' own parameter and the block's clear / copy-out by lane are not slots)
    used = {(f, u) for f, u in used if u not in ("id", "(id)", "threadIdx.x", "LANE")}
    assert len(used) > 40
    bad = sorted((f, u) for f, u in used if u not in members)
    assert not bad, "profile slots that are not HxProf members: %s" % bad


def test_the_profile_tools_carry_no_name_table_of_their_own():
    for t in TOOLS:
        src = open(os.path.join(ROOT, "tools", t)).read()
        assert "import prof_slots" in src, t
        assert not re.search(r"\{\s*\d+\s*:\s*[\"']", src), "%s has a literal slot -> name table" % t
        assert not re.search(r"\[:,\s*\d+\]", src), "%s reads a profile slot by number" % t
