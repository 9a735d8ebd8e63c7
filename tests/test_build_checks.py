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


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """tools/check_lds_flat.py run once, its listings kept: (the finished process, the directory of <unit>.s files)"""
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc on this host")
    d = str(tmp_path_factory.mktemp("listings"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lds_flat.py"), "--keep", d], capture_output=True, text=True, timeout=600)
    return r, d


def test_no_flat_instruction_touches_lds_in_any_kernel(listings):
    """the kernels' wave-local LDS hand-overs order DS instructions only (no s_waitcnt): a generic pointer into LDS in an
    out-of-line function would compile to FLAT accesses, which that order does not cover (tools/check_lds_flat.py)"""
    r = listings[0]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok (18 translation units)" in r.stdout      # (the five stream-walk units twice: the walk, and its twin with the test tap)


def test_every_kernel_keeps_fp32_denormals(listings):
    """The product is byte-identical to the reference on float input down to subnormal samples (the DC blocker's tail after
    digital silence is subnormal for seconds), so no kernel may flush them.  Every kernel descriptor (.amdhsa_kernel block) of
    the listings says `.amdhsa_float_denorm_mode_32 3`: the FLOAT_DENORM_MODE field of the wave's MODE register for
    single precision, 3 = flush neither source nor destination denormals ("preserve"; 0 flushes both).  The same holds for
    `.amdhsa_float_denorm_mode_16_64 3` (the double-precision noise terms).  A descriptor without the directive would take
    the assembler's default, so its absence fails too.  And the build's flags hold no switch that flushes or relaxes
    floating point: they are taken from hmp3_amd/build.sh and hx_units.tab alone."""
    r, d = listings
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    kernels = 0
    for unit in checked_units():
        text = open(os.path.join(d, unit[:-4] + ".s")).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
            kernels += 1
            for directive in (".amdhsa_float_denorm_mode_32", ".amdhsa_float_denorm_mode_16_64"):
                v = re.findall(r"^\s*" + re.escape(directive) + r"\s+(\S+)\s*$", m.group(2), re.M)
                assert v == ["3"], (unit, m.group(1), directive, v)
        assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == len(re.findall(r"^\s*\.end_amdhsa_kernel", text, re.M))
    # every __global__ function of the sources has a descriptor that was read (templates may add more)
    src = "".join(open(os.path.join(SRC, f), errors="replace").read() for f in os.listdir(SRC) if f.endswith((".hip", ".inc")))
    assert kernels >= len(re.findall(r"^\s*(?:template\s*<[^>]*>\s*)?__global__\b", src, re.M)) > 0, kernels


FLUSH_OR_FAST = re.compile(r"(?<![\w-])-(?:ffast-math|Ofast|ffp-model=fast|funsafe-math-optimizations|fapprox-func|ffinite-math-only|fassociative-math"
                           r"|freciprocal-math|fno-signed-zeros|fno-honor-(?:nans|infinities)|f(?:gpu|cuda)-flush-denormals-to-zero"
                           r"|f(?:gpu|cuda)-approx-transcendentals|fdenormal-fp-math(?:-f32)?=|mdaz-ftz|cl-denorms-are-zero|cl-fast-relaxed-math"
                           r"|cl-unsafe-math-optimizations|munsafe-fp-atomics|fno-hip-fp32-correctly-rounded-divide-sqrt)")


def test_build_flags_hold_no_flush_or_fast_math_switch():
    """hmp3_amd/build.sh and hx_units.tab, the two places compiler flags come from: no switch that flushes denormals or
    licenses value-changing floating-point rewrites, in any spelling clang knows for HIP; -fno-fast-math and
    -ffp-contract=off stay on every hipcc line"""
    assert FLUSH_OR_FAST.search("hipcc -O3 -ffast-math x") and FLUSH_OR_FAST.search("-fgpu-flush-denormals-to-zero")
    assert FLUSH_OR_FAST.search("-fdenormal-fp-math-f32=preserve-sign") and not FLUSH_OR_FAST.search("-O3 -fno-fast-math -ffp-contract=off")
    for f in (os.path.join(ROOT, "hmp3_amd", "build.sh"), os.path.join(SRC, "hx_units.tab")):
        code = "\n".join(l.split("#")[0] if l.lstrip().startswith("#") else l for l in open(f).read().splitlines())
        assert not FLUSH_OR_FAST.search(code), (f, FLUSH_OR_FAST.search(code).group(0))
    sh = open(os.path.join(ROOT, "hmp3_amd", "build.sh")).read()
    flags = re.search(r'^FLAGS="(.*)"$', sh, re.M).group(1)
    assert "-fno-fast-math" in flags.split() and "-ffp-contract=off" in flags.split()
    # the listings above are compiled with the same two switches
    tool = open(os.path.join(ROOT, "tools", "check_lds_flat.py")).read()
    assert '"-ffp-contract=off", "-fno-fast-math"' in tool and not FLUSH_OR_FAST.search(tool)


def test_flat_check_compiles_with_the_flags_of_the_build_script():
    """tools/check_lds_flat.py and hmp3_amd/build.sh both take units and flags from hmp3_amd/csrc/hx_units.tab: the optimisation
    level, scheduler strategy and MachineLICM switch of every translation unit must be the measured ones"""
    units = checked_units()
    ilp, nolicm = ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"], ["-mllvm", "-disable-machine-licm"]
    for u in ("hx_alloc", "hx_alloc_slim", "hx_alloc_lsf", "hx_alloc1", "hx_alloc1_lsf"):
        assert units[u + ".hip"] == ["-O2"] + ilp + nolicm, u
        # (its twin with the test tap in the stream walk's place: built as the unit is)
        assert units[u.replace("hx_alloc", "hx_count") + ".hip"] == units[u + ".hip"], u
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
