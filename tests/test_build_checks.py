"""Build checks that need no GPU: hipcc cross-compiles the kernels for gfx950 and the listings are read."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "hmp3_amd", "csrc")


def checked_units():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lds_flat.py"), "--print-flags"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    return {l.split()[1]: l.split()[2:] for l in r.stdout.strip().splitlines()}


def test_no_flat_instruction_touches_lds_in_any_kernel():
    """the kernels' wave-local LDS hand-overs order DS instructions only (no s_waitcnt): a generic pointer into LDS in an
    out-of-line function would compile to FLAT accesses, which that order does not cover (tools/check_lds_flat.py)"""
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc on this host")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lds_flat.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok (13 translation units)" in r.stdout


def test_flat_check_compiles_with_the_flags_of_the_build_script():
    """tools/check_lds_flat.py and hmp3_amd/build.sh both take units and flags from hmp3_amd/csrc/hx_units.tab: the optimisation
    level, scheduler strategy and MachineLICM switch of every translation unit must be the measured ones"""
    units = checked_units()
    ilp, nolicm = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"], ["-mllvm", "-disable-machine-licm"]
    for u in ("hx_alloc", "hx_alloc_slim", "hx_alloc_lsf", "hx_alloc1", "hx_alloc1_lsf"):
        assert units[u + ".hip"] == ["-O2"] + ilp + nolicm, u
    for u in ("hx_polyphase", "hx_src"):
        assert units[u + ".hip"] == ["-O3", "-fno-slp-vectorize"] + nolicm, u
    for u in ("hx_spec", "hx_prep"):
        assert units[u + ".hip"] == ["-O3", "-fno-slp-vectorize"] + ilp, u
    assert units["hx_pack.hip"] == ["-O3"]
    sh = open(os.path.join(ROOT, "hmp3_amd", "build.sh")).read()
    assert "hx_units.tab" in sh and not re.search(r"\bhx_\w+\.(hip|cpp|inc)\b", sh), "build.sh names a unit of its own"
    assert '${HX_ALLOC_OPT:--O2}' in sh and 'ALLOC_SCHED="${HX_ALLOC_SCHED-$ILP}"' in sh and 'NOLICM="${HX_NOLICM--mllvm -disable-machine-licm}"' in sh and "${HX_OPT:--O3}" in sh


def test_every_kernel_file_is_under_the_flat_check():
    """every source that defines a __global__ function is compiled by tools/check_lds_flat.py, as a unit or through #include:
    a new kernel file cannot stay outside the check"""
    reached, todo = set(), list(checked_units())
    while todo:
        f = todo.pop()
        if f not in reached and os.path.exists(os.path.join(SRC, f)):
            reached.add(f)
            todo += re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(SRC, f)).read(), re.M)
    kernels = {f for f in os.listdir(SRC) if re.search(r"\b__global__\b", open(os.path.join(SRC, f), errors="replace").read())}
    assert kernels and kernels <= reached, sorted(kernels - reached)
