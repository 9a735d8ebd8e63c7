"""hx_xing_crc_combine (hmp3_amd/csrc/hx_xhead.cpp): the MusicCRC of A ++ B from the CRCs of A and B and the length of B, against
hx_xing_update_crc over the concatenation (which tests/test_xing_tag.py pins to the reference).  CPU only: needs the built
library and no GPU.  Every comparison is equality."""
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hmp3_amd", "libhmp3amd.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="hmp3_amd/libhmp3amd.so not built (hmp3_amd/build.sh)")

LENGTHS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 4097, 1 << 20)


def crc(data, seed=0):
    from hmp3_amd import api
    return int(api.lib().hx_xing_update_crc(seed, bytes(data), len(data)))


def combine(a, b, n):
    from hmp3_amd import api
    return api.crc_combine(a, b, n)


def test_check_value_of_the_convention():
    """reflected CRC-16, polynomial 0xA001, seed 0 (CRC-16/ARC)"""
    assert crc(b"123456789") == 0xBB3D


def test_combine_equals_one_pass_over_the_concatenation():
    """every pair of lengths from LENGTHS, random bytes; the CRC of each string is taken once"""
    rng = np.random.default_rng(20240)
    parts = {n: [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(2)] for n in LENGTHS}
    crcs = {n: [crc(p) for p in parts[n]] for n in LENGTHS}
    for la, lb in itertools.product(LENGTHS, LENGTHS):
        a, b = parts[la][0], parts[lb][1]
        assert combine(crcs[la][0], crcs[lb][1], lb) == crc(a + b), (la, lb)


def test_left_fold_over_fifty_pieces():
    """50 pieces of random length, empty ones among them, folded left to right against one pass over all of them"""
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 3000, 50)
    lens[[0, 7, 8, 49]] = 0
    pieces = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    run = 0
    for p in pieces:
        run = combine(run, crc(p), len(p))
    assert run == crc(b"".join(pieces))
    assert sum(len(p) for p in pieces) > 50000


def test_empty_and_zero_operands():
    """len_b = 0 (an empty B, whose CRC is 0) leaves crc_a; crc_b = 0 with a length is crc_a followed by bytes that leave
    a zero register at zero: a run of zero bytes from seed 0 keeps the register 0, so B = zeros is such a string"""
    for a in (0, 1, 0x8000, 0xBB3D, 0xFFFF):
        assert combine(a, 0, 0) == a
        for n in (1, 16, 4097):
            assert combine(a, 0, n) == crc(bytes(n), a)
    assert combine(0, 0x1234, 99) == 0x1234         # an empty A in front


def test_negative_length_returns_crc_a_unchanged():
    """the documented refusal (include/hmp3_amd.h): a negative len_b is no length"""
    for n in (-1, -4097, -(1 << 40)):
        assert combine(0xBB3D, 0x1234, n) == 0xBB3D
