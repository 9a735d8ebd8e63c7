"""CPU side of the stage-tap cases (tests/stage_tap_cases.py, run on the GPU by tests/test_gpu_stage_taps.py): the oracle
alone is run on the committed inputs, and the branches the cases exist for must be reached - block-type transitions at call
boundaries, short granules, the pre-echo clamp taken and held by its floor.  Also the layout of the oracle's tap record and of
the tests' mirror of HxBandPrep, and the new taps against the values they are defined from."""
import ctypes as C

import numpy as np
import pytest

import stage_tap_cases as K
from hmp3_amd import api
from oracle import oracle as O
from stage_taps import GBand, bits, host_table, short_masks


def test_frame_debug_mirror_has_the_size_of_the_struct():
    O.lib().hxo_sizeof_frame_debug.restype = C.c_int
    assert O.lib().hxo_sizeof_frame_debug() == C.sizeof(O.FrameDebug)
    O.lib().hxo_sizeof_stage_taps.restype = C.c_int
    assert O.lib().hxo_sizeof_stage_taps() == C.sizeof(O.StageTaps)


def test_band_prep_mirror_has_the_size_of_the_struct():
    assert int(host_table(api, {}, "sizeof_band_prep", 1)[0]) == C.sizeof(GBand) == 6 * 44 * 4


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_reaches_its_branches(name):
    cfg, S, F, how, _, pos = K.CASES[name]
    assert S <= 6 and F <= 24 and len(pos) == S
    t = K.case_trace(name)
    assert [len(b) for b in t["bt"]] == [2 * F] * S
    if name.endswith("_sw") or "thr" in name:
        assert min(t["short"]) >= 1, t["short"]
    if name.startswith("thr0"):
        assert all(set(b[2:]) == {2} for b in t["bt"]), t["bt"]     # every granule after the first frame is short
        return
    assert t["taken"] >= 1 and t["floor"] >= 1 or name.startswith("thr100") and t["taken"] >= 1, (t["taken"], t["floor"])
    if how != "one":            # ... and on a call's first granule: the clamp against the memory a call starts with
        assert t["first_taken"] >= 1
    if cfg.startswith("a1"):
        assert all(set(b) == {0} for b in t["bt"])


def test_call_boundaries_meet_every_transition():
    names = [n for n in K.CASES if (n.startswith("frame_by_frame") and n.endswith("_sw")) or n.startswith("thr")]
    assert len(names) == 4
    met = set().union(*(K.case_trace(n)["boundaries"] for n in names))
    assert met == K.TRANSITIONS, met
    # the uneven calls start on other granules than their streams' neighbours do
    plan = K.plan("uneven_counts_vbr50_sw")
    assert any(0 in row for row in plan) and any(len({n for n in row if n}) > 1 for row in plan)
    assert max(max(row) for row in plan) == 3


@pytest.mark.parametrize("cfg", list(K.CONFIGS))
def test_line_ranges_of_the_prep_comparison(cfg):
    """the ranges TapBatch._prep takes from the host tables: x^(3/4) is formed of lines that have a magnitude"""
    kw = K.CONFIGS[cfg][0]
    tab = lambda n, k: host_table(api, kw, n, k)
    hf, nbmax, nbmax2, nbmax3, start = int(tab("scalars", 16)[7]), tab("nbmax", 2), tab("nbmax2", 2), tab("nbmax3", 2), tab("startBand_l", 23)
    nl_mag = int(start[22]) if hf else int(nbmax[0])
    nch = int(tab("nchan", 1)[0])
    assert all(0 < int(nbmax2[ch]) <= nl_mag <= 576 for ch in range(nch))
    assert all(0 < int(nbmax3[ch]) <= 576 for ch in range(nch))
    assert 0 < (int(tab("psy_short_npart", 1)[0]) + 1) >> 1 <= 12


@pytest.mark.parametrize("name", ["thr100_mostly_short", "frame_by_frame_lsf_mono_vbr_16k", "hf_48k_sw"])
def test_new_taps_agree_with_what_they_are_defined_from(name):
    """mask_short is thr_short after pre-echo control (short_masks: the formula the GPU comparison applies to the kernels'
    sums, here fed the oracle's own and its own carry); mask_mb is hxo_mblog of the mask tap; the counts are in range"""
    kw = K.control(name)
    mono = kw.get("mode") == 3
    mpart = (int(host_table(api, kw, "psy_short_npart", 1)[0]) + 1) >> 1
    pcm = K.case_pcm(name)
    shorts = longs = 0
    for s in range(pcm.shape[0]):
        enc = O.OracleEncoder(O.default_control(**kw))
        d, t = O.oracle_enable_debug(enc), O.oracle_enable_stage_taps(enc)
        prev_bt, carry = 0, [None, None]
        for f in range(pcm.shape[1] // 1152):
            enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152])
            ts = np.array(t.thr_short).reshape(2, 2, 36)
            msk = np.array(t.mask_short).reshape(2, 2, 3, 12)
            for igr in range(2):
                bt = int(d.block_type[igr])
                for ch in range(1 if mono else 2):
                    if bt == 2:
                        if prev_bt == 2:
                            want = short_masks(ts[igr, ch], mpart, True, carry[ch])
                        else:
                            want = short_masks(ts[igr, ch], mpart, False, np.zeros(12, np.float32))
                        assert np.array_equal(bits(want), bits(msk[igr, ch, :, :mpart])), (s, f, igr, ch)
                        carry[ch] = np.float32(2.0) * ts[igr, ch, 24:36]
                        shorts += 1
                    else:
                        m = np.array(d.mask).reshape(2, 2, 22)[igr, ch]
                        mb = np.array(t.mask_mb).reshape(2, 2, 22)[igr, ch]
                        assert [O.lib().hxo_mblog(float(v)) for v in m[:21]] == list(mb[:21]), (s, f, igr, ch)
                        nb = [int(np.array(v).reshape(2, 2)[igr, ch]) for v in (t.nb_x, t.nb_e, t.nb_z)]
                        assert all(0 < n <= 22 for n in nb), nb
                        assert int(t.attack_prev[igr]) in (0, 1)
                        longs += 1
                prev_bt = bt
    assert shorts > 0 and longs > 0
