"""The stream walk's gain search and inverse_sf2 on the constructed granules of tests/noise_cases.py, through hx_debug_seek:
seek_actual and inverse_sf2 as k_alloc, k_alloc_slim and k_alloc_lsf build them - the lanes' line runs, the segmented scan,
the bucket certificates, the strict and the double-table fall-backs - channel 1 on the helper wave through the walk's work
orders, on records made for the edges of those sums instead of what a signal happens to reach.  Every output is compared
with the oracle's by ==; tests/test_noise_cases.py holds the oracle to the reference's own functions on the same records.
The count of strict fall-backs and of double-table passes is the one the case module's restatement of the device's summation
order predicts.  A failure names the record's rule, the channel, the band and the first field that differs."""
import numpy as np
import pytest

import gpu_support as G
import noise_cases as K
from hmp3_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def run(unit, mode, sr, strict_sums=False, edit=None):
    """(records, the indices that ran, rc, out [n][184] of the device)"""
    R = K.records(mode, sr)
    keep = K.runs(unit, R)
    a = R.pick(keep)
    if edit:
        edit(a)
    seek = mode == "seek"
    rc, out = api.debug_seek(R.T.ec, unit, mode, a["hdr"], a["xr"], a["band"], x34=a["x34"] if seek else None, x34max=a["x34max"] if seek else None,
                             ix=None if seek else a["ix"], strict_sums=strict_sums, device=G.dev().index)
    return R, keep, rc, out


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("unit", list(K.UNITS))
def test_the_walks_sums_leave_what_the_oracle_leaves(unit, mode):
    """one launch per (unit, mode, rate) and a second with strict sums forced: the same outputs, every measured sweep strict"""
    for sr in K.RATES[K.UNITS[unit]]:
        want, res, forced = K.reference(mode, sr)
        R, keep, rc, got = run(unit, mode, sr)
        assert rc == 0, api.last_error()
        assert len(keep) >= 100
        bad = K.first_difference(R, keep, got, want[keep])
        assert bad is None, "%s %s %d Hz: %s" % (unit, mode, sr, bad)
        for name, col, pred in (("strict fall-backs", 176, res["nstrict"]),) + ((("double-table passes", 177, res["big"]),) if mode == "seek" else ()):
            off = np.flatnonzero(got[:, col] != pred[keep])
            assert not len(off), "%s %s %d Hz: record %d (%s: %s) counted %d %s, the restatement predicts %d" % (
                unit, mode, sr, keep[off[0]], R.lists[keep[off[0]]], R.rules[keep[off[0]]], got[off[0], col], name, pred[keep][off[0]])
        _, _, rc, again = run(unit, mode, sr, strict_sums=True)
        assert rc == 0, api.last_error()
        bad = K.first_difference(R, keep, again, want[keep])
        assert bad is None, "%s %s %d Hz, strict sums forced: %s" % (unit, mode, sr, bad)
        assert np.array_equal(again[:, 176], forced["nstrict"][keep]), "%s %s %d Hz, strict sums forced: not every measured sweep counted as strict" % (unit, mode, sr)
        if mode == "seek":
            assert np.array_equal(again[:, 177], res["big"][keep])


def test_channel_0_searches_the_same_beside_any_channel_1():
    """nothing leaks from the helper wave: channel 0's outputs do not depend on what channel 1 holds"""
    sr = K.RATES["mpeg1"][0]
    R, keep, rc, out = run("k_alloc", "seek", sr)
    assert rc == 0, api.last_error()
    rows = [i for i, r in enumerate(keep) if R.rules[r].startswith("beside")]
    assert len(rows) == 3 and all(np.array_equal(out[rows[0], :88], out[i, :88]) for i in rows[1:])
    assert len({tuple(out[i, 88:176]) for i in rows}) == 3


def test_a_refused_record_launches_nothing_and_a_unit_takes_its_own_controls_only():
    sr = K.RATES["mpeg1"][0]

    def step(a):
        a["band"][2, 1, 3, 2] = 108
    _, _, rc, out = run("k_alloc", "seek", sr, edit=step)
    assert rc == -1 and "record 2 channel 1 band 3: gsf" in api.last_error() and not out.any()

    def maximum(a):
        a["band"][5, 0, 4, 3] += 1
    _, _, rc, out = run("k_alloc_slim", "isf2", sr, edit=maximum)
    assert rc == -1 and "record 5 channel 0 band 4: ixmax" in api.last_error() and not out.any()
    assert run("k_alloc_lsf", "seek", sr)[2] == -1 and "does not run" in api.last_error()
    R = K.records("seek", sr)
    a = R.pick(np.arange(2))
    rc, out = api.debug_seek(api.default_control(samprate=sr, bitrate=64, nsbstereo=8), "k_alloc1", "seek", a["hdr"], a["xr"], a["band"], x34=a["x34"], x34max=a["x34max"])
    assert rc == -1 and "first-generation" in api.last_error() and not out.any()
