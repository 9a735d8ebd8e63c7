"""The stream walk's line loops - sweep_load / sweep_run (gain search), isf2_run (inverse_sf2), quant_lines (every copy of the
quantiser, requant_count<0> and <1>) - process all their lines in one basic block whatever the class's run width
(hx_alloc.hip, "No guard on the class's run width").  Byte identity against the CPU oracle through the C ABI, on batches small
enough for a few seconds that still reach every one of those loops: every sample rate (their scalefactor band tables give
the run widths the host produces), two reduced band counts, both directions of the CBR rate loop (counted on the oracle
before the bytes are compared), the strict-sum fallback, and mono (no helper wave).  Run with: python -m pytest tests -m gpu"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import ROOT
from hmp3_amd import api
from line_loop_cases import BATCHES, F, STREAMS, batch_pcm, encode_two_calls
from oracle import oracle as O

pytestmark = pytest.mark.gpu
MPEG1_RATES = ("44k", "48k", "32k")
STAT_INCREASE, STAT_DECREASE = 1, 4                         # hxo_rate_stats: granules that entered increase_bits / decrease_bits


@functools.lru_cache(maxsize=None)
def reference(name, mono=False):
    """(the batch's PCM, the oracle's bytes per stream, the oracle's rate-loop counters over the batch): computed once,
    shared by the two kernel builds and the tests"""
    kw = dict(BATCHES[name], mode=3) if mono else BATCHES[name]
    pcm = batch_pcm(kw, mono)
    stats = (C.c_longlong * 8).in_dll(O.lib(), "hxo_rate_stats")
    before = list(stats)
    want = []
    for s in range(pcm.shape[0]):
        enc = O.OracleEncoder(O.default_control(**kw))
        want.append(b"".join(enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152]) for f in range(F)))
    return pcm, want, [stats[i] - before[i] for i in range(8)]


def run_width(kw):
    w = np.zeros(1, np.int32)
    assert api.lib().hx_debug_host_table(C.byref(api.default_control(**kw)), b"run_w", w.ctypes.data, 4) == 4
    return int(w[0])


def test_the_batches_cover_the_run_widths_the_host_produces():
    """The kernels run all RUNW_MAX / 2 pairs whatever the width (no path per width), so: at least three different widths
    among the batches, each an even value in 2 .. 10."""
    widths = {name: run_width(kw) for name, kw in BATCHES.items()}
    print("run_w per batch:", widths)
    assert all(w in (2, 4, 6, 8, 10) for w in widths.values()), widths
    assert len(set(widths.values())) >= 3, widths


@pytest.mark.parametrize("name", [n for n in BATCHES if not n.startswith("lsf")])
def test_line_loops_byte_identical_to_oracle(name):
    kw = BATCHES[name]
    pcm, want, stats = reference(name)
    print("%s: run_w %d, oracle granules entering increase_bits %d, decrease_bits %d" % (name, run_width(kw), stats[STAT_INCREASE], stats[STAT_DECREASE]))
    if name in MPEG1_RATES:     # the rate loop is really entered: both copies of requant_count run
        assert stats[STAT_INCREASE] >= 10 and stats[STAT_DECREASE] >= 6, stats
    got = encode_two_calls(kw, pcm)
    for s in range(len(want)):
        assert got[s] == want[s], "stream %d (seed %d, rho %.1f)" % ((s,) + STREAMS[s])


@pytest.mark.parametrize("name", [n for n in BATCHES if n.startswith("lsf")])
def test_line_loops_lsf_byte_identical_to_oracle(name):
    """k_alloc_lsf: the MPEG-2 rates' band tables"""
    kw = BATCHES[name]
    pcm, want, stats = reference(name)
    print("%s: run_w %d" % (name, run_width(kw)))
    got = encode_two_calls(kw, pcm)
    for s in range(len(want)):
        assert got[s] == want[s], "stream %d (seed %d, rho %.1f)" % ((s,) + STREAMS[s])


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import line_loop_cases as T
got = T.encode_two_calls(T.BATCHES["44k"], T.batch_pcm(T.BATCHES["44k"]))
sys.stdout.buffer.write(b"".join(len(g).to_bytes(4, "little") + g for g in got))
"""


def test_strict_sums_run_on_the_same_line_loops():
    """HMP3AMD_EXACT_SUMS=1 sends every band sum down sweep_sum_strict / sweep_run_stored and inverse_sf2's strict path.  The
    library reads the variable when it is loaded: a fresh child process."""
    pcm, want, stats = reference("44k")
    env = dict(os.environ, HMP3AMD_EXACT_SUMS="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    out, got = r.stdout, []
    while out:
        n = int.from_bytes(out[:4], "little")
        got.append(out[4:4 + n])
        out = out[4 + n:]
    assert len(got) == len(want)
    for s in range(len(want)):
        assert got[s] == want[s], "stream %d" % s


def test_mono_runs_the_loops_without_a_helper_channel():
    kw = dict(BATCHES["44k"], mode=3)
    pcm, want, stats = reference("44k", True)
    got = encode_two_calls(kw, pcm)
    assert got[0] == want[0]
