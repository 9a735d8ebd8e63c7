"""The allocator path census on a real MI355X: the committed cases of tests/alloc_path_cases.py (inputs on which the oracle
takes the rare branches of the rate control, the Huffman pick and the frame driver; tests/test_alloc_path_cases.py asserts on
the CPU which) go through the C ABI batch by batch, once as one call and once as calls of one frame, and every frame is
compared with the oracle by ==, with no tolerance, through tests/stage_taps.py's TapBatch: the stages before the allocator,
the side information, the quantised lines and signs, the long-block scalefactors, MNR_after, byte_pool and main_bytes, and the
bytes - so a failure names the first frame, granule and field.  MPEG-1 batches run on k_alloc and on k_alloc_slim.
Run with: python -m pytest tests -m gpu"""
import os
import subprocess
import sys

import pytest

import alloc_path_cases as K
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import ROOT
from hmp3_amd import api

pytestmark = pytest.mark.gpu
BATCHES = K.batches()


def check(batch):
    one = K.run_batch(api, batch, K.FRAMES)
    by_frame = K.run_batch(api, batch, 1)
    assert one.got == by_frame.got


@pytest.mark.parametrize("batch", [b for b in BATCHES if b.startswith("m1_")])
def test_mpeg1_paths(batch):
    """k_alloc and k_alloc_slim (the k6_build fixture runs both)"""
    check(batch)


@pytest.mark.one_k6_build
@pytest.mark.parametrize("batch", [b for b in BATCHES if b.startswith("m2_")])
def test_mpeg2_paths(batch):
    """k_alloc_lsf"""
    check(batch)


@pytest.mark.one_k6_build
@pytest.mark.parametrize("batch", [b for b in BATCHES if b.startswith("a1_")])
def test_first_generation_paths(batch):
    """k_alloc1 / k_alloc1_lsf"""
    skip_unless_host_libm_is_the_restated_one()
    check(batch)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import alloc_path_cases as K
from hmp3_amd import api
K.run_batch(api, "m1_long", K.FRAMES)
print("compared")
"""


@pytest.mark.one_k6_build
def test_strict_sums_on_the_decrease_paths():
    """HMP3AMD_EXACT_SUMS=1 on the MPEG-1 long batch: decrease_bits runs the gain search again, and the strict sums write over
    the line buffer.  The library reads the variable when it is loaded: a fresh child process, which compares as above."""
    env = dict(os.environ, HMP3AMD_EXACT_SUMS="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert r.stdout.decode().strip().endswith("compared")
