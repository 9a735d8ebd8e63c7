"""The stream walk's quantiser and Huffman counter on the constructed granules of tests/count_cases.py, through hx_debug_count:
do_quant, quant_count_bits, count_bits, s_do_quant and s_count_bits_ch as each of the five stream-walk units builds them,
channel 1 on the helper wave through the walk's work orders, on records made for their edges instead of what a rate loop
happens to reach.  Every output - lines, band maxima, tables, region ends, nbig, nquads, bits, the returned sum - is compared
with the oracle's by ==; tests/test_count_cases.py holds the oracle to the reference's own functions on the same records.
A failure names the record's rule, the channel and the first field that differs."""
import numpy as np
import pytest

import count_cases as K
import gpu_support as G
from hmp3_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def run(unit, mode, sr):
    """(records, the indices that ran, (lines, band maxima, out) of the device)"""
    R = K.records(mode, sr)
    keep = K.runs(mode, unit, R)
    a = R.pick(keep)
    quant = mode in ("quant_count", "quant_then_count", "short")
    ec = api.default_control(samprate=sr, **K.UNITS[unit][1])
    rc, ix, ixmax, out = api.debug_count(ec, unit, mode, a["hdr"], a["ix"], a["ixmax"], a["x34"] if quant else None, a["gsf"] if quant else None, device=G.dev().index)
    assert rc == 0, api.last_error()
    return R, keep, (ix.reshape(len(keep), 1152), ixmax.reshape(len(keep), -1), out)


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("unit", list(K.UNITS))
def test_the_walks_functions_leave_what_the_oracle_leaves(unit, mode):
    """one launch per (unit, mode) and band table: the MPEG-1 rates on k_alloc, k_alloc_slim and k_alloc1, the MPEG-2 rates on
    the two _lsf units"""
    for sr in K.RATES[K.UNITS[unit][0]]:
        R, keep, got = run(unit, mode, sr)
        want = K.expected(mode, sr, unit == "k_alloc_slim")
        short = mode.startswith("short")
        # (a short record's maxima: the bands the quantiser walks; the device clears the rest, the oracle leaves them alone)
        bad = K.first_difference(R, keep, got, want, 48 if short else 22, K.tables(sr).nsfs if short else None)
        assert bad is None, "%s %s %d Hz: %s" % (unit, mode, sr, bad)
        assert len(keep) >= 100


@pytest.mark.parametrize("unit", ["k_alloc", "k_alloc_slim", "k_alloc_lsf"])
def test_both_routes_of_quantise_and_count_agree(unit):
    """quant_count_bits, and do_quant followed by count_bits, on the records both may run: the same lines, maxima and counts"""
    for sr in K.RATES[K.UNITS[unit][0]]:
        R, keep1, fused = run(unit, "quant_count", sr)
        _, keep2, unfused = run(unit, "quant_then_count", sr)
        sel = np.isin(keep2, keep1)
        assert sel.sum() == len(keep1)
        for a, b in zip(fused, unfused):
            assert np.array_equal(a, b[sel]), "%s %d Hz: the two routes differ at record %d (%s)" % (
                unit, sr, keep1[np.flatnonzero((a != b[sel]).reshape(len(keep1), -1).any(axis=1))[0]], R.rules[keep1[np.flatnonzero((a != b[sel]).reshape(len(keep1), -1).any(axis=1))[0]]])


def test_one_channel_0_record_counts_the_same_beside_any_channel_1():
    """nothing leaks from the helper wave: channel 0's outputs do not depend on what channel 1 holds"""
    sr = K.RATES["mpeg1"][0]
    R, keep, (_, _, out) = run("k_alloc", "count", sr)
    for bt in (0, 1, 3):
        rows = [i for i, r in enumerate(keep) if R.rules[r].startswith("beside") and R.rules[r].endswith("bt=%d" % bt)]
        assert len(rows) == 3 and all(np.array_equal(out[rows[0], :10], out[i, :10]) for i in rows[1:])
        assert len({tuple(out[i, 10:20]) for i in rows}) == 3


def test_a_refused_record_launches_nothing_and_a_unit_takes_its_own_controls_only():
    sr = K.RATES["mpeg1"][0]
    R = K.records("count", sr)
    a = R.pick(np.arange(4))
    a["ix"][2, 1, 7] = 9000
    ec = api.default_control(samprate=sr, bitrate=64)
    rc, ix, _, out = api.debug_count(ec, "k_alloc", "count", a["hdr"], a["ix"], a["ixmax"])
    assert rc == -1 and "record 2 channel 1" in api.last_error() and not out.any() and np.array_equal(ix.reshape(a["ix"].shape), a["ix"])
    a = R.pick(np.arange(4))
    assert api.debug_count(ec, "k_alloc_lsf", "count", a["hdr"], a["ix"], a["ixmax"])[0] == -1 and "does not run" in api.last_error()
