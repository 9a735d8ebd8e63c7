"""What the inputs of tests/test_gpu_math.py (tests/math_cases.py) cover, asserted on the CPU, and the host-side functions
they are compared with held to what they restate."""
import ctypes as C
import ctypes.util

import numpy as np

import math_cases as M
from hmp3_amd import api
from oracle import oracle as O


def test_strata_hold_every_rule():
    """every mantissa at biased exponents 1, 126, 127, 128, 254; 4096 evenly spaced mantissas and the 64 lowest and highest
    at every exponent 1 .. 254; 2^16 subnormals from the smallest to the largest; +-0, +inf, a NaN, -1.0f; hx_logf's
    sixteen interval edges +-64 patterns at three exponents"""
    s = M.strata()
    bits = np.unique(s)

    def has(u):
        u = np.asarray(u, dtype=np.uint32)
        i = np.minimum(np.searchsorted(bits, u), len(bits) - 1)
        return bool((bits[i] == u).all())
    for e in M.FULL_EXPONENTS:
        assert has(M.full_mantissas(e)), e
    m = np.concatenate([np.arange(4096, dtype=np.uint32) * 2048, np.arange(64, dtype=np.uint32), np.arange((1 << 23) - 64, 1 << 23, dtype=np.uint32)])
    for e in range(1, 255):
        assert has(m | np.uint32(e << 23)), e
    sub = bits[(bits > 0) & (bits < M.MIN_NORMAL)]
    assert len(sub) == 1 << 16 and sub[0] == 1 and sub[-1] == 0x7FFFFF
    assert has([0, 0x80000000, 0x7F800000, 0xBF800000]) and np.isnan(M.f32(bits)).any()
    for k in M.LOGF_EDGE_EXPONENTS:
        for i in range(16):
            edge = M.LOGF_OFF + (i << 19) + (k << 23)
            assert has(np.arange(edge - 64, edge + 65, dtype=np.uint32)), (k, i)
    print("STRATA: %d patterns, %d distinct" % (len(s), len(bits)))


def test_strata_reach_every_table_interval_of_logf_at_every_exponent():
    """hx_logf splits its argument into an exponent k and one of sixteen table intervals i = (tmp >> 19) % 16: every (k, i)
    that a positive normal float can have occurs in STRATA (16 k + i is every integer between its values at the smallest and
    the largest normal), and the subnormals, which the function normalises first, add the exponents below"""
    s = M.strata()
    normal = s[(s >= M.MIN_NORMAL) & (s <= M.MAX_FINITE)]
    keys = np.unique(M.logf_key(normal))
    lo, hi = int(M.logf_key(np.array([M.MIN_NORMAL], dtype=np.uint32))[0]), int(M.logf_key(np.array([M.MAX_FINITE], dtype=np.uint32))[0])
    assert lo >> 4 == -126 and hi >> 4 == 128
    assert len(keys) == hi - lo + 1 and keys[0] == lo and keys[-1] == hi
    for k in range(-125, 128):      # (the first and the last exponent hold a part of the sixteen)
        assert {int(v) & 15 for v in keys[(keys >> 4) == k]} == set(range(16)), k
    sub = s[(s > 0) & (s < M.MIN_NORMAL)]
    scaled = (M.f32(sub) * np.float32(2.0 ** 23)).view(np.uint32).astype(np.int64) - (23 << 23)        # as hx_logf normalises
    ksub = np.unique((scaled - M.LOGF_OFF) >> 23)
    assert ksub[0] == -149 and ksub[-1] == -126 and len(ksub) == 24
    print("logf: %d (k, interval) pairs over the normals, exponents %d .. %d below them" % (len(keys), ksub[0], ksub[-1]))


def check_windows(name, f, values, first, win, expect):
    s = M.positive(M.strata())
    ends = f(np.array([M.MIN_NORMAL, M.MAX_FINITE], dtype=np.uint32))
    # every integer between the range's ends has a window, and the window sits on that integer's threshold
    assert list(values) == list(range(int(ends[0]) + 1, int(ends[1]) + 1))
    assert win.shape == (len(values), 2 * M.WINDOW) and (win[:, M.WINDOW] == first).all()
    assert (f(first) >= values).all() and (f(first - np.uint32(1)) < values).all()
    # the bisection relies on a non-decreasing host function: on every window, and on STRATA in ascending order
    fw = f(win.reshape(-1)).reshape(win.shape)
    assert (np.diff(win.astype(np.int64), axis=1) >= 0).all() and (np.diff(fw.astype(np.int64), axis=1) >= 0).all()
    ss = np.sort(s)
    assert (np.diff(f(ss).astype(np.int64)) >= 0).all()
    print("%s: %d windows (%d inputs), values %d .. %d" % (name, len(values), win.size, values[0], values[-1]))
    assert expect[0] <= len(values) <= expect[1]


def test_dual_g_windows_sit_on_every_threshold_of_a_monotone_host_function():
    """trade_dual's gain step (int) (1.7717f * dblog(x) + 1.0f) over the positive normal floats: dblog runs from -379 to
    +385 dB, the step over some 1 350 integers"""
    values, first, win = M.dual_g_windows()
    check_windows("dual_g", M.host_dual_g, values, first, win, (1300, 1450))


def test_a1_gz_windows_sit_on_every_threshold_of_a_monotone_host_function():
    """the first-generation allocator's zero-gain step (int) (a1_gz1 * hx_logf(m) + a1_gz2): a1_gz1 = 16 / (3 ln 2) = 7.69
    and logf runs from -87.3 to 88.7, some 1 350 integers"""
    values, first, win = M.a1_gz_windows()
    check_windows("a1_gz", M.host_a1_gz, values, first, win, (1300, 1450))


def test_first_generation_control_is_one_and_the_joint_one_is_not():
    for kw, want in ((M.KW_FIRST_GEN, 1), (M.KW_JOINT, 0)):
        v = np.zeros(1, dtype=np.int32)
        assert api.lib().hx_debug_host_table(C.byref(api.default_control(**kw)), b"alloc1", v.ctypes.data, 4) == 4 and v[0] == want
    assert len(M.a1_log_cbw()) == 21 and (M.a1_log_cbw() > 0).all()


def test_is_scale_tuples_hold_every_operand_class():
    t, cls = M.is_scale_tuples()
    e0, e1, r = M.f32(t[0]), M.f32(t[1]), M.f32(t[2])
    u = cls["log_uniform"]
    assert u.stop - u.start == 1 << 20
    for v in (e0[u], e1[u], r[u]):      # log-uniform over 1e-12 .. 1e30: every decade holds its share
        assert v.min() >= np.float32(1e-12) and v.max() <= np.float32(1e30)
        h = np.histogram(np.log10(v.astype(np.float64)), bins=42, range=(-12, 30))[0]
        assert h.min() > 0.9 * (1 << 20) / 42 and h.max() < 1.1 * (1 << 20) / 42
    assert abs(np.corrcoef(np.log10(e0[u].astype(np.float64)), np.log10(e1[u].astype(np.float64)))[0, 1]) < 0.01
    assert (e0[cls["e0_eq_e1"]] == e1[cls["e0_eq_e1"]]).all()
    assert (t[0][cls["e0_floor"]] == np.float32(1.0e-12).view(np.uint32)).all()
    assert (r[cls["r_one"]] == 1.0).all()
    with np.errstate(all="ignore"):
        p = e0 * e1
    ps, po = p[cls["product_subnormal"]], p[cls["product_overflows"]]
    assert np.count_nonzero((ps > 0) & (ps < np.float32(2.0 ** -126))) > 1000 and np.count_nonzero(np.isinf(po)) > 1000
    for name, sl in cls.items():
        assert sl.stop - sl.start >= M.SPECIAL, name


def test_div_pairs_hold_every_quotient_class():
    ab = M.div_pairs()
    assert ab.shape == (2, 1 << 20)
    q4 = 1 << 18
    with np.errstate(all="ignore"):
        q = M.f32(ab[0]).astype(np.float64) / M.f32(ab[1]).astype(np.float64)
    # the first quarter: the exact quotient is below the smallest normal float (or rounds up to it)
    assert np.count_nonzero((q[:q4] > 0) & (q[:q4] < 2.0 ** -126)) > 0.99 * q4
    # the second: within one float ulp of a power of two (2^-23 relative above it, 2^-24 below), on both sides and on it
    m, _ = np.frexp(q[q4:2 * q4])       # m in [0.5, 1)
    above, below = (m - 0.5) * 2, (1.0 - m)
    assert ((above <= 2.0 ** -23 * 1.0000001) | (below <= 2.0 ** -24 * 2.0000001)).all()
    assert np.count_nonzero(m == 0.5) > 0.2 * q4 and np.count_nonzero((m > 0.5) & (m < 0.75)) > 0.2 * q4 and np.count_nonzero(m > 0.75) > 0.2 * q4
    rest = M.f32(ab[:, 2 * q4:])
    assert np.isnan(rest).any() and (rest < 0).any() and np.count_nonzero(np.abs(rest) < np.float32(2.0 ** -126)) > 1000


def test_host_array_forms_are_the_spot_checks_functions():
    """hx_libm_spot_check counts, on its own points, where this host's libm gives another logf or log10f than the host build
    of hx_libm32.h.  The array forms are that build: on the same points they differ from libm in exactly as many places
    (none on glibc 2.35)."""
    n = 200000
    span = 0x7F800000 - 0x00800000
    u = (0x00800000 + (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(span)).astype(np.uint32)
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.logf.restype = libm.log10f.restype = C.c_float
    libm.logf.argtypes = libm.log10f.argtypes = [C.c_float]
    x = M.f32(u)
    want_log = np.array([libm.logf(float(v)) for v in x[:20000]], dtype=np.float32).view(np.uint32)
    want_log10 = np.array([libm.log10f(float(v)) for v in x[:20000]], dtype=np.float32).view(np.uint32)
    bad = np.count_nonzero((M.host_logf(u[:20000]) != want_log) | (M.host_log10f(u[:20000]) != want_log10))
    rep = api.libm_report(20000)
    print("glibc %s: %d of %d spot-check points differ from the restatement" % (rep["glibc"], rep["mismatches"], rep["points"]))
    assert bad == rep["mismatches"]
    # the two named expressions are what their text says, on the array forms themselves
    l10 = M.f32(M.host_log10f(u))
    cbw = np.resize(M.a1_log_cbw(), n)
    want = (-10.0 * l10.astype(np.float64) - cbw.astype(np.float64)).astype(np.float32)
    assert (M.f32(M.host_mask_db(u, cbw)) == want).all()
    gz = M.host_a1_gz(u)
    lg = M.f32(M.host_logf(u))
    assert (gz == (np.float32(16.0 / (3.0 * np.log(2.0))) * lg + np.float32(1 - (16.0 / (3.0 * np.log(2.0))) * np.log(.5946) + 8)).astype(np.int32)).all()


def test_oracle_array_forms_are_the_scalar_functions():
    rng = np.random.default_rng(7)
    u = np.concatenate([rng.integers(0, 1 << 32, 2000, dtype=np.uint64).astype(np.uint32), M.sampled()[-2100:]])
    L = O.lib()
    notnan = u[(u & 0x7FFFFFFF) <= 0x7F800000]          # (a NaN does not keep its payload through a float argument)
    assert [int(v) for v in O.math("mblog", notnan).view(np.int32)] == [L.hxo_mblog(float(x)) for x in M.f32(notnan)]
    fin = M.positive(u)
    db = M.f32(O.math("dblog", fin))
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.log10.restype, libm.log10.argtypes = C.c_double, [C.c_double]
    ref = np.array([10.0 * libm.log10(float(v)) for v in M.f32(fin)], dtype=np.float64).astype(np.float32)
    assert (db == ref).all()
    g = O.math("dual_g", fin).view(np.int32)
    assert (g == (np.float32(1.7717) * db + np.float32(1.0)).astype(np.int32)).all()
    i32 = M.mbexp_args()[::97]
    L.hxo_mbexp.argtypes, L.hxo_mbexp.restype = [C.c_int], C.c_float
    assert (M.f32(O.math("mbexp", i32)) == np.array([L.hxo_mbexp(int(v)) for v in i32], dtype=np.float32)).all()
    r = M.round_args()[-6000:]
    x = M.f32(r)
    assert (O.math("round", r).view(np.int32) == (x + np.copysign(np.float32(0.5), x)).astype(np.int32)).all()
