"""The kernels' device math over its domains, on a real MI355X: every function of hx_batch_debug_math - the very device
functions the allocator kernels call, built with their flags - against its host-side value on the inputs of
tests/math_cases.py (tests/test_math_cases.py asserts what they cover).  No tolerance: every assertion is == on bit patterns
or integers, NaN results compare as NaN on both sides.

The restated logf / log10f and the two expressions built on them are compared with the host build of the same header, which
is what is pinned to glibc 2.35 - so nothing here is skipped on a host with another libm.  dblog and trade_dual's gain step
are compared with the oracle's functions, i.e. with the libm of the machine the test runs on, as the pow() test of
tests/test_gpu_dynamic_range.py is.

What these tests notice, measured on scratch builds whose device code alone was changed (MI355X, glibc 2.35):
  one entry of hx_logf's table (logc of interval 5) changed in bit 28, a step of 2^-24 of its value: logf differs for
      397 445 of the 43 087 415 inputs, log10f for 372 255, a1_mask_db for 15 077 of 9 532 983, a1_gz for 10 window inputs;
  the same entry changed in its last bit, and A0 * r2 + y contracted to an fma: nothing differs.  Both move the double
      result by about one part in 2^53, which reaches the float only within that distance of a rounding boundary - some
      1e-9 of the arguments; hx_libm32.h says as much of glibc's own FMA build.  No test on float results can see either;
  dblog's 10.0 * log10 done in float: the gain step differs for 16 593 of the 11 091 968 window inputs."""
import numpy as np
import pytest

import math_cases as M
from hmp3_amd import api
from oracle import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


class batch:
    """one small batch of a control, closed on the way out"""

    def __init__(self, kw):
        self.kw = kw

    def __enter__(self):
        self.b = api.Batch(api.default_control(**self.kw), nstreams=1, max_frames=1)
        return self.b

    def __exit__(self, *exc):
        self.b.close()


@pytest.mark.parametrize("name", ["logf", "log10f"])
def test_restated_logf_device_build_equals_its_host_build_on_strata(name):
    u = M.strata()
    with batch(M.KW_FIRST_GEN) as b:
        got = M.device(b, name, u)
    M.check_same(name, got, M.host_logf(u) if name == "logf" else M.host_log10f(u), True, u)


def test_a1_mask_db_equals_the_host_build():
    """r over every mantissa of [1, 2) and STRATA's sample of every exponent, paired with the 21 band widths in turn"""
    r = np.concatenate([M.full_mantissas(127), M.sampled()])
    cbw = np.resize(M.a1_log_cbw(), r.size).view(np.uint32)
    with batch(M.KW_FIRST_GEN) as b:
        got = M.device(b, "a1_mask_db", r, cbw)
    M.check_same("a1_mask_db", got, M.host_mask_db(r, cbw), True, r, cbw)


def test_a1_gz_equals_the_host_build_at_every_threshold_and_on_strata():
    values, first, win = M.a1_gz_windows()
    w, s = win.reshape(-1), M.positive(M.strata())
    with batch(M.KW_FIRST_GEN) as b:
        got_w, got_s = M.device(b, "a1_gz", w), M.device(b, "a1_gz", s)
    print("a1_gz: %d windows" % len(values))
    M.check_same("a1_gz on the threshold windows", got_w, M.host_a1_gz(w), False, w)
    M.check_same("a1_gz on STRATA", got_s, M.host_a1_gz(s), False, s)


def test_dblog_device_log10_census_and_within_one_ulp():
    """The device's double log10 is not glibc's: dblog's float result is allowed to differ, by one float ulp at the most;
    how often and by how much is printed.  What the bitstream reads of it is the gain step, asserted in the next test."""
    u = M.strata()
    with batch(M.KW_JOINT) as b:
        got = M.device(b, "dblog", u)
    want = O.math("dblog", u)
    d = M.differing(got, want, True)
    ulps = M.ulp_distance(got[d], want[d])
    print("glibc %s: device dblog differs from the host's for %d of %d inputs (largest difference %d ulp), first at %s"
          % (api.libm_report(100)["glibc"], len(d), u.size, int(ulps.max()) if len(d) else 0, "0x%08x" % int(u[d[0]]) if len(d) else None))
    fin = (got[d] & 0x7FFFFFFF) < 0x7F800000
    assert fin.all() and (ulps <= 1).all(), "%d inputs differ by more than one ulp or in kind, first at 0x%08x" % (
        np.count_nonzero(~fin | (ulps > 1)), int(u[d[np.flatnonzero(~fin | (ulps > 1))[0]]]))


def test_dual_g_equals_the_oracle_at_every_threshold_and_on_strata():
    values, first, win = M.dual_g_windows()
    w, s = win.reshape(-1), M.positive(M.strata())
    with batch(M.KW_JOINT) as b:
        got_w, got_s = M.device(b, "dual_g", w), M.device(b, "dual_g", s)
    print("glibc %s; dual_g: %d windows" % (api.libm_report(100)["glibc"], len(values)))
    M.check_same("dual_g on the threshold windows", got_w, M.host_dual_g(w), False, w)
    M.check_same("dual_g on STRATA", got_s, M.host_dual_g(s), False, s)


@pytest.mark.parametrize("name", ["is_scale", "is_scale_lsf"])
def test_intensity_rescale_equals_float64_with_one_rounding(name):
    t, cls = M.is_scale_tuples()
    with batch(M.KW_FIRST_GEN) as b:
        got = M.device(b, name, t[0], t[1], t[2])
    want = (M.ref_is_scale if name == "is_scale" else M.ref_is_scale_lsf)(t[0], t[1], t[2])
    for k, sl in cls.items():       # by operand class: which one a difference belongs to is what a reader needs first
        M.check_same("%s, operand class %s" % (name, k), got[sl], want[sl], True, t[0][sl], t[1][sl], t[2][sl])


def test_fp32_division_is_ieee_with_subnormal_quotients():
    ab = M.div_pairs()
    with batch(M.KW_FIRST_GEN) as b:
        got = M.device(b, "div", ab[0], ab[1])
    want = M.ref_div(ab[0], ab[1])
    q4 = ab.shape[1] // 4
    for k, sl in (("subnormal quotient", slice(0, q4)), ("next to a power of two", slice(q4, 2 * q4)), ("random patterns", slice(2 * q4, 4 * q4))):
        M.check_same("div, operand class %s" % k, got[sl], want[sl], True, ab[0][sl], ab[1][sl])


def test_table_primitives_equal_the_oracles_on_the_batchs_tables():
    u, mb, r = M.strata(), M.mbexp_args(), M.round_args()
    with batch(M.KW_JOINT) as b:
        got = {n: M.device(b, n, a) for n, a in (("mblog", u), ("mblog16", u), ("mbexp", mb), ("pow34", u), ("round", r))}
    want_mblog = O.math("mblog", u)
    M.check_same("mblog", got["mblog"], want_mblog, False, u)
    M.check_same("mblog16", got["mblog16"], want_mblog, False, u)
    M.check_same("mbexp", got["mbexp"], O.math("mbexp", mb), True, mb)
    M.check_same("pow34", got["pow34"], O.pow34(M.f32(u)), True, u)
    M.check_same("round", got["round"], O.math("round", r), False, r)


def test_debug_math_refuses_what_it_cannot_take_before_any_launch():
    with batch(M.KW_JOINT) as b:
        L = api.lib()
        big = np.zeros((1 << 25) + 1, dtype=np.uint32)
        out = np.zeros(1, dtype=np.uint32)
        assert L.hx_batch_debug_math(b.h, b"logf", big.ctypes.data, big.size, out.ctypes.data) == -1 and "2^25" in api.last_error()
        assert L.hx_batch_debug_math(b.h, b"logf", big.ctypes.data, 0, out.ctypes.data) == -1
        assert L.hx_batch_debug_math(b.h, b"expf", big.ctypes.data, 1, out.ctypes.data) == -1 and "expf" in api.last_error()
        assert out[0] == 0
        with pytest.raises(RuntimeError):
            b.debug_math("nothing", big[:4])
        with pytest.raises(ValueError):
            b.debug_math("div", big[:4], big[:5])
        assert b.debug_math("div", np.float32([6.0]), np.float32([3.0])).view(np.float32)[0] == 2.0
        assert b.status() == 0
