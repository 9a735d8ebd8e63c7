"""The kernels' device math over its domains: the inputs of tests/test_gpu_math.py, the host-side values they are compared
with, and the comparison.  tests/test_math_cases.py asserts on the CPU what the inputs cover.

A few device expressions decide bytes of the bitstream and are not the same function on the GPU and on the host: the
restated logf / log10f of the first-generation allocator (hx_libm32.h, another compiler and other flags than its host
build), the device's double log10 behind trade_dual's gain step, double sqrt and divide in the intensity rescale, fp32
division, and the table primitives of hx_dev.h.  Streams reach them with a few hundred arguments.  Each is a pure function
of one to three scalars, so the inputs here are built from rules, not from streams; everything is a 32-bit pattern
(uint32 for floats), every comparison is == on patterns or integers (NaN results: NaN on both sides).

STRATA      stratified floats for the functions compared by bits: every mantissa at five exponents, a mantissa sample at
            every exponent, subnormals, the special values, and the edges of hx_logf's sixteen table intervals.
windows     for the two expressions that end in an integer (trade_dual's gain step, the first-generation allocator's
            zero-gain step) a last-bit difference of the logarithm matters only where the integer changes: the 4096 floats
            on either side of every such threshold of the host function, found by bisection on the bit pattern.
tuples      operands of the intensity rescale and of fp32 division."""
import ctypes as C
import functools

import numpy as np

from hmp3_amd import api
from oracle import oracle as O

MAX_CALL = 1 << 25              # arguments hx_batch_debug_math takes per call
MIN_NORMAL, MAX_FINITE = 0x00800000, 0x7F7FFFFF
FULL_EXPONENTS = (1, 126, 127, 128, 254)       # every mantissa: the smallest normals, around 1.0, the largest finite
SAMPLE_STEP = 2048              # 4096 evenly spaced mantissas per exponent
LOGF_OFF = 0x3F330000           # hx_logf: tmp = ix - LOGF_OFF, interval (tmp >> 19) % 16, exponent k = tmp >> 23 (arithmetic)
LOGF_EDGE_EXPONENTS = (-120, 0, 120)
WINDOW = 4096                   # floats on either side of a threshold

KW_JOINT = dict(bitrate=64)                     # MPEG-1 joint stereo, second-generation allocator
KW_FIRST_GEN = dict(bitrate=64, nsbstereo=8)    # intensity stereo: the first-generation allocator (k_alloc1)


def _ro(a):
    a.setflags(write=False)
    return a


def full_mantissas(e):
    return (np.arange(1 << 23, dtype=np.uint32) | np.uint32(e << 23))


@functools.lru_cache(maxsize=None)
def sampled():
    """the part of STRATA that is not the five full exponents: uint32 patterns"""
    m = np.unique(np.concatenate([np.arange(4096, dtype=np.uint32) * SAMPLE_STEP, np.arange(64, dtype=np.uint32),
                                  np.arange((1 << 23) - 64, 1 << 23, dtype=np.uint32)]))
    parts = [m | np.uint32(e << 23) for e in range(1, 255)]
    # 2^16 subnormals: the 2^15 smallest (every exponent down to the last bit), 2^15 evenly spaced over the rest, the largest
    sub = np.concatenate([np.arange(1, (1 << 15) + 1, dtype=np.uint32), (1 << 15) + 1 + np.arange(1 << 15, dtype=np.uint32) * 255])
    sub[-1] = 0x7FFFFF
    parts.append(sub)
    parts.append(np.array([0, 0x80000000, 0x7F800000, 0x7FC00000, 0xBF800000], dtype=np.uint32))       # +-0, +inf, a NaN, -1.0f
    for k in LOGF_EDGE_EXPONENTS:
        for i in range(16):
            edge = LOGF_OFF + (i << 19) + (k << 23)
            parts.append(np.arange(edge - 64, edge + 65, dtype=np.uint32))
    return _ro(np.concatenate(parts))


@functools.lru_cache(maxsize=None)
def strata():
    return _ro(np.concatenate([full_mantissas(e) for e in FULL_EXPONENTS] + [sampled()]))


def positive(u):
    """the patterns of u that are positive finite non-zero floats (where a logarithm is finite and its integer defined)"""
    return u[(u > 0) & (u <= MAX_FINITE)]


def logf_key(u):
    """hx_logf's (k, interval) of positive normal patterns as one number: (int32) tmp >> 19 = 16 k + i"""
    return (u.astype(np.int64) - LOGF_OFF) >> 19


# ---- host-side values ----

def host_logf(u):
    return api.host_math(api.default_control(**KW_FIRST_GEN), "logf", u)


def host_log10f(u):
    return api.host_math(api.default_control(**KW_FIRST_GEN), "log10f", u)


def host_a1_gz(u):
    return api.host_math(api.default_control(**KW_FIRST_GEN), "a1_gz", u).view(np.int32)


def host_mask_db(r, cbw):
    return api.host_math(api.default_control(**KW_FIRST_GEN), "a1_mask_db", r, cbw)


def host_dual_g(u):
    return O.math("dual_g", u).view(np.int32)


def a1_log_cbw():
    a = np.zeros(21, dtype=np.float32)
    assert api.lib().hx_debug_host_table(C.byref(api.default_control(**KW_FIRST_GEN)), b"a1_log_cbw", a.ctypes.data, a.nbytes) == a.nbytes
    return a


def f32(u):
    return np.ascontiguousarray(u).view(np.float32)


def ref_div(a, b):
    """IEEE division is correctly rounded: float64 quotient of two float32, one rounding to float32 (53 >= 2 * 24 + 2 bits:
    the double rounding is innocuous, in the subnormal range too)"""
    with np.errstate(all="ignore"):
        return (f32(a).astype(np.float64) / f32(b).astype(np.float64)).astype(np.float32).view(np.uint32)


def ref_is_scale(e0, e1, r):
    """hx_alloc1.inc a1_is_scale in float64 with the code's float32 roundings: the sum, the product and the inner square
    root are float32 values, the rest is double, one rounding to float32 at the end"""
    with np.errstate(all="ignore"):
        s, pr = f32(e0) + f32(e1), f32(e0) * f32(e1)
        inner = np.sqrt(pr.astype(np.float64)).astype(np.float32)
        return np.sqrt((s.astype(np.float64) + 2.0 * inner.astype(np.float64)) / f32(r).astype(np.float64)).astype(np.float32).view(np.uint32)


def ref_is_scale_lsf(e0, e1, r):
    with np.errstate(all="ignore"):
        a = np.where(f32(e0) > f32(e1), f32(e0), f32(e1))
        return np.sqrt((a / f32(r)).astype(np.float64)).astype(np.float32).view(np.uint32)


# ---- threshold windows ----

def thresholds(f, lo=MIN_NORMAL, hi=MAX_FINITE):
    """f: a non-decreasing int32 function of uint32 patterns (vectorised).  For every integer v in (f(lo), f(hi)] the first
    pattern p in (lo, hi] with f(p) >= v -> (values, patterns)"""
    ends = f(np.array([lo, hi], dtype=np.uint32))
    values = np.arange(int(ends[0]) + 1, int(ends[1]) + 1, dtype=np.int64)
    a, b = np.full(values.size, lo, dtype=np.int64), np.full(values.size, hi, dtype=np.int64)      # f(a) < v <= f(b)
    while int((b - a).max()) > 1:
        mid = (a + b) >> 1
        ge = f(mid.astype(np.uint32)).astype(np.int64) >= values
        b, a = np.where(ge, mid, b), np.where(ge, a, mid)
    return values, b.astype(np.uint32)


def windows(first, lo=MIN_NORMAL, hi=MAX_FINITE):
    """uint32 [len(first)][2 * WINDOW]: the WINDOW patterns below each threshold and the WINDOW from it on, ascending, kept
    inside [lo, hi] (a window at the domain's end repeats the end)"""
    w = first.astype(np.int64)[:, None] + np.arange(-WINDOW, WINDOW, dtype=np.int64)[None, :]
    return np.clip(w, lo, hi).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def dual_g_windows():
    values, first = thresholds(host_dual_g)
    return values, first, _ro(windows(first))


@functools.lru_cache(maxsize=None)
def a1_gz_windows():
    values, first = thresholds(host_a1_gz)
    return values, first, _ro(windows(first))


# ---- operand tuples ----

N_TUPLES = 1 << 20
SPECIAL = 4096


def _log_uniform(rng, n, lo, hi):
    return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def is_scale_tuples():
    """(e0, e1, r) uint32 [3][n], and the slices of the special classes {name: slice}"""
    rng = np.random.default_rng(20260101)
    cols = [np.stack([_log_uniform(rng, N_TUPLES, 1e-12, 1e30) for _ in range(3)])]
    cls, pos = {"log_uniform": slice(0, N_TUPLES)}, N_TUPLES

    def add(name, e0, e1, r):
        nonlocal pos
        cols.append(np.stack([e0, e1, r]).astype(np.float32))
        cls[name] = slice(pos, pos + len(e0))
        pos += len(e0)
    e = _log_uniform(rng, SPECIAL, 1e-12, 1e30)
    add("e0_eq_e1", e, e, _log_uniform(rng, SPECIAL, 1e-12, 1e30))
    add("e0_floor", np.full(SPECIAL, np.float32(1.0e-12)), _log_uniform(rng, SPECIAL, 1e-12, 1e30), _log_uniform(rng, SPECIAL, 1e-12, 1e30))
    add("r_one", _log_uniform(rng, SPECIAL, 1e-12, 1e30), _log_uniform(rng, SPECIAL, 1e-12, 1e30), np.ones(SPECIAL, dtype=np.float32))
    add("product_subnormal", _log_uniform(rng, SPECIAL, 1e-22, 1e-20), _log_uniform(rng, SPECIAL, 1e-22, 1e-20), _log_uniform(rng, SPECIAL, 1e-12, 1e30))
    add("product_overflows", _log_uniform(rng, SPECIAL, 1e20, 1e30), _log_uniform(rng, SPECIAL, 1e20, 1e30), _log_uniform(rng, SPECIAL, 1e-12, 1e30))
    return _ro(np.ascontiguousarray(np.concatenate(cols, axis=1)).view(np.uint32)), cls


@functools.lru_cache(maxsize=None)
def div_pairs():
    """(a, b) uint32 [2][2^20]: a quarter with a subnormal quotient, a quarter with a quotient within one ulp of a power of
    two, the rest random bit patterns (all of float32: both signs, zeros, subnormals, infinities and NaNs among them)"""
    rng = np.random.default_rng(20260102)
    q4 = N_TUPLES // 4
    # q subnormal, b anything from 1 to 2^20, a = q * b rounded: a / b lands on q or next to it
    q = rng.integers(1, 1 << 23, q4, dtype=np.uint32).view(np.float32)
    b1 = _log_uniform(rng, q4, 1.0, 2.0 ** 20)
    a1 = (q.astype(np.float64) * b1.astype(np.float64)).astype(np.float32)
    # a = (b moved by -1, 0 or +1 in its last place) * 2^k: a / b = 2^k (1 + j ulp(b) / b)
    b2 = _log_uniform(rng, q4, 1e-6, 1e6)
    j = rng.integers(-1, 2, q4).astype(np.int64)
    a2 = np.ldexp((b2.view(np.uint32).astype(np.int64) + j).astype(np.uint32).view(np.float32), rng.integers(-20, 21, q4).astype(np.int32)).astype(np.float32)
    a3, b3 = rng.integers(0, 1 << 32, 2 * q4, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, 2 * q4, dtype=np.uint64).astype(np.uint32)
    a = np.concatenate([a1.view(np.uint32), a2.view(np.uint32), a3])
    b = np.concatenate([b1.view(np.uint32), b2.view(np.uint32), b3])
    return _ro(np.stack([a, b]))


@functools.lru_cache(maxsize=None)
def mbexp_args():
    """int32: every millibel value the clamps of hx_mbexp leave alone and 8000 beyond them on each side, the clamps' edges,
    the ends of int32 and 2^16 random ints (the function reads the low 16 bits of any int)"""
    rng = np.random.default_rng(20260103)
    return _ro(np.concatenate([np.arange(-40000, 40001, dtype=np.int64), [32000, 32001, -32000, -32001, -(1 << 31), (1 << 31) - 1],
                               rng.integers(-(1 << 31), 1 << 31, 1 << 16)]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def round_args():
    """float32 patterns with |x| < 2^31 (beyond it the conversion to int is not defined): STRATA's, and k + 0.5 with its two
    neighbours for |k| <= 1024 - the ties that rounding half away from zero is about"""
    s = strata()
    s = s[(s & 0x7FFFFFFF) < 0x4F000000]
    h = (np.arange(-1024, 1025, dtype=np.float32) + np.float32(0.5)).view(np.uint32)
    return _ro(np.concatenate([s, h, h + np.uint32(1), h - np.uint32(1)]))


# ---- the device call and the comparison ----

def device(b, name, *ops):
    """Batch.debug_math over arrays of any length, MAX_CALL arguments a call"""
    n = ops[0].size
    return np.concatenate([b.debug_math(name, *[o[i:i + MAX_CALL] for o in ops]) for i in range(0, n, MAX_CALL)])


def differing(got, want, floats):
    """indices where two arrays of 32-bit patterns differ; floats: two NaNs of any payload are the same result"""
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    ne = got != want
    if floats:
        ne &= ~(((got & 0x7FFFFFFF) > 0x7F800000) & ((want & 0x7FFFFFFF) > 0x7F800000))
    return np.flatnonzero(ne)


def check_same(what, got, want, floats, *ops):
    """every output equal; the message gives the count, the first differing input as hex and both outputs"""
    d = differing(got, want, floats)
    if len(d):
        i = int(d[0])
        g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
        raise AssertionError("%s: %d of %d inputs differ, first at (%s): device 0x%08x, host 0x%08x" % (
            what, len(d), g.size, ", ".join("0x%08x" % int(np.ascontiguousarray(o).view(np.uint32).reshape(-1)[i]) for o in ops), int(g[i]), int(w[i])))


def ulp_distance(got, want):
    """distance in float32 steps between two arrays of finite float patterns (monotone integer image of the floats)"""
    def key(u):
        i = np.ascontiguousarray(u).view(np.uint32).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)
    return np.abs(key(got) - key(want))
