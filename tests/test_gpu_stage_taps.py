"""Stage taps on a real MI355X at the shapes and boundaries the one-call, four-stream cases of test_gpu_parity.py never
reach (tests/stage_taps.py is the comparison, tests/stage_tap_cases.py the inputs): calls of one frame, so that every
carry between calls - pre-echo memory, stereo hysteresis, detector history, block-type state - is handed over at every
frame and the last workgroups of k_prep (4 granules each) and k_detect (4 streams each) are partly filled; odd frame
counts; per-stream frame counts; short granules following short granules across calls; the paths on which k_prep returns
early; M/S frames with the high-frequency band.  What a case must reach is asserted from what was compared, and
tests/test_stage_tap_cases.py asserts the same of the inputs on the CPU."""
import numpy as np
import pytest

import stage_tap_cases as K
from conftest import skip_unless_host_libm_is_the_restated_one
from stage_taps import TapBatch
from hmp3_amd import api

pytestmark = pytest.mark.gpu
COMPARED = {}       # case -> the call-boundary transitions its last run compared


def run_case(name):
    """the case's calls through a TapBatch; asserts what the oracle alone says was compared, returns the TapBatch (closed)"""
    cfg, S, F, how, _, _ = K.CASES[name]
    pcm = K.case_pcm(name)
    calls = K.plan(name)
    stride = max(max(row) for row in calls)
    tb = TapBatch(api, K.control(name), S, stride, K.taps(name))
    done = [0] * S
    for row in calls:
        blk = np.zeros((S, stride * 1152) + pcm.shape[2:], dtype=pcm.dtype)
        for s, n in enumerate(row):
            blk[s, :n * 1152] = pcm[s, done[s] * 1152:(done[s] + n) * 1152]
            blk[s, n * 1152:] = 12345           # (behind a stream's frames: never read)
            done[s] += n
        tb.call(blk, None if how != "counts" else row)
    tb.close()
    t = K.case_trace(name)
    assert tb.frames == [F] * S and all(len(g) > 0 for g in tb.got)
    assert tb.short_granules == t["short"]
    assert tb.boundary_bt == t["boundaries"]
    assert (tb.clamp_taken, tb.clamp_floor, tb.clamp_first) == (t["taken"], t["floor"], t["first_taken"])
    nlong = sum(len(b) - b.count(2) for b in t["bt"])
    assert tb.prep_granules == (0 if tb.alloc1 else nlong)
    COMPARED[name] = set(tb.boundary_bt)
    return tb


FRAME_BY_FRAME = ["vbr50_sw", "cbr128_lr_sw", "mono_vbr50"]
LSF = ["lsf_cbr64_22k", "lsf_mono_vbr_16k"]


def check_frame_by_frame(name):
    tb = run_case(name)
    assert min(tb.short_granules) >= 1 and tb.clamp_first >= 1 and tb.clamp_floor >= 1
    assert tb.msscan_paths == {"scalar"}
    return tb


@pytest.mark.parametrize("cfg", FRAME_BY_FRAME)
def test_frame_by_frame(cfg):
    """S = 5, 24 calls of one frame: every odd -> even granule boundary is a call boundary (thrprev, ms_memory, attack_hist and
    bt_prev carried 23 times); 10 units in k_prep's workgroups of 4, 5 streams in k_detect's workgroups of 4"""
    check_frame_by_frame("frame_by_frame_" + cfg)


@pytest.mark.parametrize("cfg", LSF)
def test_frame_by_frame_mpeg2(cfg):
    check_frame_by_frame("frame_by_frame_" + cfg)


def check_one_call(name):
    tb = run_case(name)
    # NG = 46 is no multiple of 8: k_msscan's scalar loop (test_every_stage_bit_exact, F = 24, takes the vector one)
    assert tb.msscan_paths == {"scalar"} and tb.clamp_floor >= 1


@pytest.mark.parametrize("cfg", FRAME_BY_FRAME)
def test_one_call_odd_counts(cfg):
    """S = 3, F = 23 in one call: 138 units, 3 streams - partly filled last workgroups - and NG % 8 != 0"""
    check_one_call("one_call_" + cfg)


@pytest.mark.parametrize("cfg", LSF)
def test_one_call_odd_counts_mpeg2(cfg):
    check_one_call("one_call_" + cfg)


def test_uneven_counts_vbr50_sw():
    """S = 6, calls of up to 3 frames under per-stream counts until every stream has 12: NGs != NG, so the pre-echo memory a
    call leaves is that of granule NGs - 1, and a stream that sits a call out keeps its own"""
    tb = run_case("uneven_counts_vbr50_sw")
    assert min(tb.short_granules) >= 1 and tb.clamp_first >= 1


@pytest.mark.parametrize("name", ["thr0_all_short", "thr100_mostly_short"])
def test_short_after_short_across_calls(name):
    """S = 3, 8 calls of one frame at a detector threshold of 0 / 100: short -> short and short -> stop across calls, the
    window-2 carry of k_msscan under the short model's pre-echo control"""
    tb = run_case(name)
    assert (2, 2) in tb.boundary_bt
    if name.startswith("thr0"):
        assert tb.short_granules == [14] * 3        # everything after the first frame
    else:
        assert {(2, 3), (3, 1)} <= tb.boundary_bt


def test_call_boundaries_met_every_transition():
    """what the four boundary cases compared adds up to every legal transition (a case not yet run in this process is run)"""
    names = ["frame_by_frame_vbr50_sw", "frame_by_frame_cbr128_lr_sw", "thr0_all_short", "thr100_mostly_short"]
    met = set()
    for n in names:
        met |= COMPARED[n] if n in COMPARED else set(run_case(n).boundary_bt)
    assert met == K.TRANSITIONS, met


@pytest.mark.parametrize("name", ["a1_intensity", "a1_dual_lsf"])
def test_psy_taps_of_intensity_and_dual_lsf_streams(name):
    """S = 2, F = 12 on the first-generation allocator (k_prep returns early): the long psy model's taps"""
    skip_unless_host_libm_is_the_restated_one()
    tb = run_case(name)
    assert tb.alloc1 == 1 and tb.clamp_taken >= 1 and tb.seen_bt == {0}


def test_hf_48k_sw():
    """S = 3, F = 12, -V100 -HF2 -F19000 at 48 kHz: M/S frames whose magnitudes run to the end of band 21"""
    tb = run_case("hf_48k_sw")
    assert tb.hf and min(tb.short_granules) >= 1 and tb.clamp_floor >= 1
    assert 0 < tb.prep_ms < tb.prep_granules        # frames coded M/S and frames coded L/R
