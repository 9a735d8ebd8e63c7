"""k_recon_hybrid, k_recon_synth and k_recon_carry (hmp3_amd/csrc/hx_recon.hip) on the constructed granules of
tests/recon_granule_cases.py, through hx_debug_recon: the real kernels, launched by the batch's own launch expression with
the batch's tables, on records made for their edges instead of what a rate loop happens to emit.  The hybrid output and the
rows are held to the float64 decoder of tests/mp3_decode.py, driven from the same records, under the bound that module
derives from the kernels' own roundings (gamma_k times the magnitude pass, k = 30 for the hybrid tap and 82 for the output,
no slack on top); zeros, what no kernel writes, the carried slots and the split are held by float bits.  The stream walk is
not involved.  tests/test_recon_granule_cases.py shows on the CPU that these cases and this bound would catch an error of
one part in 4096 in any table entry."""
import numpy as np
import pytest

import recon_granule_cases as R
from hmp3_amd import api

# (the decoded PCM does not depend on which build of the stream walk a batch would run)
pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def run(name):
    """every launch of a list through the kernels and check(): [(launch, state, hyb, out)]"""
    worst, results = [0.0, 0.0], []
    for i, (L, ref) in enumerate(zip(R.case_list(name), R.references(name))):
        rc, state, hyb, out = R.debug_recon(L)
        assert rc == 0, api.last_error()
        r = R.check(name, i, L, ref, state, hyb, out)
        worst = [max(a, b) for a, b in zip(worst, r)]
        results.append((L, state, hyb, out))
    print("%s: largest error / bound on the device: hybrid tap %.3f, output %.3f" % (name, worst[0], worst[1]))
    return results


@pytest.mark.parametrize("name", [n for n in R.LIST_NAMES if n not in ("counts_and_kinds", "split")])
def test_the_kernels_stay_within_the_derived_bound_of_the_float64_decoder(name):
    results = run(name)
    assert any(out.any() for _, _, _, out in results)


def test_counts_and_kinds_leave_what_they_do_not_own_untouched():
    ((L, state, hyb, out),) = run("counts_and_kinds")
    sentinel = R.bits(R.SENTINEL)
    for s in range(L.S):
        nf, nch = L.frames(s), L.nchan(s)
        assert (R.bits(out[s, nf * 1152 * nch:]) == sentinel).all(), "stream %d: a row is written behind the stream's blocks" % s
        assert (R.bits(hyb[s, 2 * nf:]) == sentinel).all() and (R.bits(hyb[s, :, nch:]) == sentinel).all(), s
        assert nf == 0 or (R.bits(out[s, :nf * 1152 * nch]) != sentinel).all(), s
        if nf == 0:
            assert np.array_equal(R.bits(state[s]), R.bits(L.state[s])), "stream %d: the state of a stream without frames is written" % s
    assert (R.bits(state[0, 576:1152]) == sentinel).all()       # a mono stream's second channel of tails


def test_a_call_split_in_two_gives_the_same_float_bits():
    ((L, state, hyb, out),) = run("split")
    rc1, s1, h1, o1 = R.debug_recon(L.half(0))
    assert rc1 == 0, api.last_error()
    rc2, s2, h2, o2 = R.debug_recon(L.half(1, s1))
    assert rc2 == 0, api.last_error()
    assert np.array_equal(R.bits(hyb), R.bits(np.concatenate([h1, h2], axis=1))), "the hybrid output differs between one call and two"
    for s in range(L.S):
        m = (L.NG // 4) * 1152 * L.nchan(s)
        got, want = R.bits(np.concatenate([o1[s, :m], o2[s, :m]])), R.bits(out[s, :2 * m])
        bad = np.flatnonzero(got != want)
        assert not bad.size, "stream %d sample %d of the row: 0x%08x in two calls, 0x%08x in one (%d differ)" % (s, bad[0], got[bad[0]], want[bad[0]], bad.size)
    assert np.array_equal(R.bits(state), R.bits(s2)), "the carried state differs between one call and two"


def test_the_device_agrees_with_the_float32_restatement_where_it_must():
    """the restatement of tests/recon_granule_cases.py is the kernels' operation order in numpy: no sum of theirs may be
    reordered or contracted by the compiler, so it gives the device's float bits, and what tests/test_recon_granule_cases.py
    shows of it (the mutants, the bound's share) is shown of the kernels"""
    for name in R.LIST_NAMES:
        for L in R.case_list(name):
            rc, state, hyb, out = R.debug_recon(L)
            assert rc == 0, api.last_error()
            rs, rh, ro = R.restate(L)
            for what, a, b in (("hyb", hyb, rh), ("out", out, ro), ("state", state, rs)):
                bad = np.argwhere(R.bits(a) != R.bits(b))
                assert not len(bad), "list %s: %s %s: device %r, restatement %r (%d differ)" % (
                    name, what, tuple(int(v) for v in bad[0]), float(a[tuple(bad[0])]), float(b[tuple(bad[0])]), len(bad))


def test_a_refused_record_launches_nothing():
    (L,) = R.case_list("ms")
    a = R.device_arrays(L)
    a["ixq"][0, 1, 0, 7] = 8207
    rc, state, hyb, out = R.debug_recon(L, **a)
    assert rc == -1 and "ixq: a magnitude" in api.last_error() and "stream 0 granule 1 channel 0" in api.last_error()
    assert not hyb.any() and not out.any() and np.array_equal(R.bits(state), R.bits(L.state))
