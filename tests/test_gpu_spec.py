"""K4 on the constructed subband granules of tests/spec_cases.py, through hx_debug_spec: k_spec and k_spec_direct, unmodified,
launched by the batch's own launch expression (launch_spec) with the tables a batch stages - hybrid MDCT, alias reduction, the
long and short psy models, and the L/R-vs-M/S metric before hysteresis with its certified band sums - on blocks made for the
edges of that code instead of what a signal happens to reach.  Every float of xr, etab and thr and every msbase is compared
with the oracle's (hxo_spec_record) by bits; tests/test_spec_cases.py holds the oracle to its own frame path and to the
reference's functions on the same records, and shows what each list reaches.  The kernel has no counter of its strict
fall-backs: a wrong certificate shows in msbase on the bands of bucket_edge and worst_case, where the value the lanes would
hand over lies in another mbLogC bucket than the strict sum's.  A failure names rate, class, list, rule, stream, granule and
the first field and index that differ."""
import numpy as np
import pytest

import gpu_support as G
import spec_cases as K
from hmp3_amd import api

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
FORMS = {"k_spec": False, "k_spec_direct": True}


@pytest.mark.parametrize("sr", K.RATES)
@pytest.mark.parametrize("form", list(FORMS))
def test_the_kernel_leaves_what_the_oracle_leaves(form, sr):
    """one launch per (form, rate): every list, every class kind; granules past a stream's count keep the fill pattern"""
    L = K.launch(sr)
    got = L.run(FORMS[form], device=G.dev().index)
    assert got[0] == 0, api.last_error()
    bad = L.first_difference(got)
    assert bad is None, "%s %d Hz: %s" % (form, sr, bad)


@pytest.mark.parametrize("form", list(FORMS))
def test_every_grid_size_and_count_leaves_what_the_oracle_leaves(form):
    """launches of 1, 7, 8, 9, 17 and 20 workgroups (the grid remap's branches), streams of different classes side by side,
    per-stream counts from 0 to NG / 2, outputs pre-filled"""
    for sr in K.RATES:
        for L in K.geometry(sr):
            got = L.run(FORMS[form], device=G.dev().index)
            assert got[0] == 0, api.last_error()
            bad = L.first_difference(got)
            assert bad is None, "%s %d Hz, %d streams x %d granules, counts %s: %s" % (form, sr, L.S, L.NG, L.nfr, bad)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_mono_streams_channel_0_is_the_same_beside_any_channel_1(form):
    """a mono class defines channel 0 alone (compared with the oracle above); what it leaves there does not depend on the
    blocks the second channel's lanes read"""
    sr = K.RATES[0]
    L = K.launch(sr)
    mono = [s for s in range(L.S) if L.classes[L.cls_of[s]].nchan == 1]
    assert len(mono) >= 2
    first = L.run(FORMS[form], device=G.dev().index)
    sb = L.sb.copy()
    rng = np.random.Generator(np.random.PCG64(77))
    sb[mono, 1] = (rng.standard_normal(sb[mono, 1].shape) * 5000.0).astype(np.float32)
    second = L.run(FORMS[form], device=G.dev().index, sb=sb)
    assert first[0] == 0 and second[0] == 0, api.last_error()
    for name, a, b in zip(("xr", "etab", "thr"), first[1:4], second[1:4]):
        assert np.array_equal(a[mono][:, :, 0].view(np.uint32), b[mono][:, :, 0].view(np.uint32)), name
    assert not np.array_equal(first[1][mono][:, :, 1].view(np.uint32), second[1][mono][:, :, 1].view(np.uint32))
    # ... and the streams of the other classes are the oracle's beside them
    live = [s for s in range(L.S) if s not in mono]
    assert np.array_equal(first[1][live].view(np.uint32), second[1][live].view(np.uint32)) and np.array_equal(first[4][live], second[4][live])


def test_a_refused_launch_launches_nothing_and_unread_blocks_are_not_looked_at():
    L = K.counted(K.RATES[0])
    for what, change, words in K.refusals(L):
        rc, xr, etab, thr, ms = L.run(False, device=G.dev().index, **change)
        assert rc == -1 and all(w in api.last_error() for w in words), (what, api.last_error())
        for a in (xr, etab, thr, ms):
            assert (a.reshape(-1).view(np.uint32) == K.FILL).all(), what
    L1, words = K.first_generation_refusal(K.RATES[0])
    assert L1.run(False, device=G.dev().index)[0] == -1 and all(w in api.last_error() for w in words), api.last_error()
    # bad values where no wave reads - a stream without frames, blocks and types past a stream's count - change nothing
    for form in FORMS.values():
        got = L.run(form, device=G.dev().index, **K.accepted(L))
        assert got[0] == 0, api.last_error()
        assert L.first_difference(got) is None, L.first_difference(got)
