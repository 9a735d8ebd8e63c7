"""k_pack (hmp3_amd/csrc/hx_pack.hip) on the constructed frames of tests/pack_cases.py, through hx_debug_pack: the real kernel,
launched by the batch's own launch expression, on records made for its edges instead of what a rate loop happens to emit.
The expectation is built in plain numpy from the oracle's writer (hxo_pack_frame, which tests/test_pack_cases.py holds against
the reference's own): main data spread over the slots behind each one's header and side information, zero stuffing up to
`bytes`.  Rows and packet buffer are pre-filled with 0xA5 and compared whole, so a byte the kernel does not own and writes
all the same shows."""
import numpy as np
import pytest

import pack_cases as P
from hmp3_amd import api

# (the packer does not depend on which build of the stream walk a batch would run)
pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, the first at %s: got 0x%02x, want 0x%02x" % (
        len(bad), tuple(int(i) for i in bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def run(name):
    b = P.build(P.tables(), P.case_list(name))
    assert (b["rows"] == 0xA5).all() and (b["packet"] == 0xA5).all()
    rc, status = P.debug_pack(b)
    assert rc == 0, api.lib().hx_last_error().decode()
    return b, status


@pytest.mark.parametrize("name", P.LIST_NAMES)
def test_k_pack_writes_the_oracles_bytes_and_nothing_else(name):
    b, status = run(name)
    assert np.array_equal(b["rows"], b["want_rows"]), first_difference(b["rows"], b["want_rows"])
    assert np.array_equal(b["packet"], b["want_packet"]), first_difference(b["packet"], b["want_packet"])
    assert status == 0
    assert (b["want_rows"] != 0xA5).any()


def test_a_wrong_bit_count_sets_status_bit_4_and_nothing_else():
    b, status = run("status")
    assert status == 4
    assert np.array_equal(b["rows"], b["want_rows"]), first_difference(b["rows"], b["want_rows"])
    assert np.array_equal(b["packet"], b["want_packet"])


def test_a_refused_record_launches_nothing():
    b = P.build(P.tables(), P.case_list("status"))
    b["ixq"][0, 2, 1, 0] = 9        # above the largest table dimension among the segment's tables
    rc, status = P.debug_pack(b)
    assert rc != 0 and "above its table's range" in api.lib().hx_last_error().decode()
    assert status == -1 and (b["rows"] == 0xA5).all() and (b["packet"] == 0xA5).all()
