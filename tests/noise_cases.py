"""The stream walk's two certified band sums on constructed granules: the records of tests/test_gpu_noise.py (handed to the
walk's own seek_actual and inverse_sf2 by hx_debug_seek), what the oracle makes of them, and a float32 restatement of the
device's summation order; tests/test_noise_cases.py asserts on the CPU what the lists reach and holds the oracle to the
reference's own functions.

The walk does not add a band's noise terms left to right: each lane adds a run of W lines as a tree of pairs, a segmented
scan over the band's lanes leaves the total in its last lane, and an interval around that total either proves the mbLogC
bucket of the reference's strict sum or sends the band to the strict sum (hx_dev.h, "certified band sums").  Whole streams
meet the fall-back, the double-table pass, the last band's clamp and the search's limits by chance.  Here every record is
built from a rule and a seed for one of them.  The restatement (`sweep`, `seek`, `isf2`) follows the device's order - pair
tree as sweep_run / isf2_run write it, pair after pair in a double-table pass as sweep_run_stored does, then hx_seg_scan's
additions from the class's lane_run - and serves two ends only: to select records whose two sums fall into different
buckets, and to predict how often the device must fall back.  What a record's outputs must be comes from the oracle.

In a band whose x^(3/4) is zero every line quantises to 0 at every step and its term is x * x: there the builder controls the
terms through the lines, and a bisection on one line's bit pattern moves the strict sum onto a bucket boundary.

A unit leaves a record out only by a rule of LEFT_OUT; there is none today: the low-footprint build's 16-bit lines hold every
value the host accepts (0 .. 8206)."""
import ctypes as C
import functools

import numpy as np

from hmp3_amd import api
from oracle import oracle as O

RATES = {"mpeg1": (44100, 48000, 32000), "mpeg2": (22050, 24000, 16000)}
UNITS = {"k_alloc": "mpeg1", "k_alloc_slim": "mpeg1", "k_alloc_lsf": "mpeg2"}
CONTROL = dict(bitrate=64)
MODES = ("seek", "isf2")
LISTS = {"seek": ("walk", "layout", "bucket_edge", "worst_case", "double_table"), "isf2": ("select", "ratio_edge", "ratio_worst_case")}
LEFT_OUT = {}           # unit -> predicate on a rule name: records the unit does not run
EDGE_RECORDS = 10       # records of a bisected list per band table (every band of both channels is an edge)
F = np.float32
C0946 = F(0.0) - F(0.0946)
HALF = F(0.5)
TINY = F(1.0e-12)
U24 = F(5.9604644775390625e-08)
SENTINEL = F(12345.0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.int64).astype(np.uint32).view(np.float32)


def bucket(x):
    """what mbLogC reads of x: sign, exponent and the top 8 mantissa bits"""
    return bits(x) >> 15


class Tables:
    """one rate's tables, from hx_debug_host_table: bands, gain tables, the lanes' line runs"""

    def __init__(self, sr):
        self.sr = sr
        self.ec = api.default_control(samprate=sr, **CONTROL)
        self.o = O.CountTables(O.default_control(samprate=sr, **CONTROL))

        def tab(name, dtype, count):
            a = np.zeros(count, dtype)
            n = api.lib().hx_debug_host_table(C.byref(self.ec), name.encode(), a.ctypes.data, a.nbytes)
            assert n == a.nbytes, (name, api.last_error())
            return a
        self.start, self.width = tab("startBand_l", np.int32, 24).astype(int), tab("nBand_l", np.int32, 22).astype(int)
        nsf, nchan = tab("nsf", np.int32, 2), int(tab("nchan", np.int32, 1)[0])
        self.nb = max(int(nsf[0]), int(nsf[1]) if nchan == 2 else 0)       # the bands that have lanes
        self.W = int(tab("run_w", np.int32, 1)[0])
        run, self.last = tab("lane_run", np.uint16, 64).astype(int), tab("band_last_lane", np.uint8, 24).astype(int)[:22]
        self.gain, self.igain, self.ix43 = tab("look_gain", np.float32, 128), tab("look_34igain", np.float32, 128), tab("look_ix43", np.float32, 256)
        self.logcbw, self.mblog_tab = tab("look_log_cbwmb", np.int32, 22).astype(np.int64), tab("mblog", np.int32, 256).astype(np.int64)
        self.pow43_tab = tab("pow43", np.float64, 16384)
        assert self.ix43[0] == 0 and np.array_equal(self.start[:23], np.concatenate(([0], np.cumsum(self.width)))[:23])
        self.band_of_line = np.minimum(np.searchsorted(self.start[1:23], np.arange(576), side="right"), 21)
        # lanes (lane_run of hx_alloc.hip): first line, lines, lanes back to the band's first lane
        self.l_start, self.l_cnt, self.l_d = (run & 511) * 2, ((run >> 9) & 7) * 2, run >> 12
        k = np.arange(10)
        pair = np.minimum(self.l_start[:, None] + (k & ~1)[None, :], 574)       # (the address of a pair past the class's W is clamped)
        self.l_idx = pair + (k & 1)[None, :]
        self.l_valid = (k & ~1)[None, :] < self.l_cnt[:, None]
        self.maxw = int(self.width[:self.nb].max())
        j = np.arange(self.maxw)
        self.b_idx = np.minimum(self.start[:22, None] + j[None, :], 575)
        self.b_valid = j[None, :] < self.width[:, None]
        self.du = (self.width + self.W + 16).astype(np.float32) * U24             # hx_cert_delta
        self._beyond = {}

    def mblog(self, x):
        u = bits(x)
        return self.mblog_tab[(u >> 15) & 255] + 301 * (u >> 23)

    def pow43(self, qx):
        """qx^(4/3) as the reference's pow() returns it: the host's table, the oracle's libm past it"""
        out = self.pow43_tab[np.clip(qx, 0, 16383)]
        for v in np.unique(qx[qx >= 16384]):
            if int(v) not in self._beyond:
                d = np.zeros(1, np.float64)
                O.lib().hxo_pow43.argtypes = [C.c_int, C.c_int, C.c_void_p]
                O.lib().hxo_pow43(int(v), 1, d.ctypes.data)
                self._beyond[int(v)] = d[0]
            out = np.where(qx == v, self._beyond[int(v)], out)
        return out


@functools.lru_cache(maxsize=None)
def tables(sr):
    return Tables(sr)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: rows are channels of records, [M][576] lines and [M][22] bands
# ---------------------------------------------------------------------------------------------------------------------

def pair_tree(t):
    """sweep_run / isf2_run: ten terms of a lane's run"""
    return (((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])) + ((t[..., 4] + t[..., 5]) + (t[..., 6] + t[..., 7]))) + (t[..., 8] + t[..., 9])


def pair_after_pair(t):
    """sweep_run_stored: acc += t[k] + t[k + 1]"""
    acc = np.zeros(t.shape[:-1], np.float32)
    for k in range(0, 10, 2):
        acc = acc + (t[..., k] + t[..., k + 1])
    return acc


def seg_scan(v, d):
    """hx_seg_scan over the 64 lanes [.., 64]: row_shr 1 / 2 / 4 / 8 inside the 16-lane rows, then the row before's last lane"""
    lane = np.arange(64)
    zero = F(0.0)
    for sh in (1, 2, 4, 8):
        t = np.zeros_like(v)
        ok = (lane & 15) >= sh
        t[..., ok] = v[..., lane[ok] - sh]
        v = v + np.where(d >= sh, t, zero)
    cross = d > (lane & 15)
    t = np.zeros_like(v)
    t[..., 16:32] = v[..., 15:16]
    t[..., 48:64] = v[..., 47:48]
    v = v + np.where(cross, t, zero)
    t = np.zeros_like(v)
    t[..., 32:48] = v[..., 31:32]
    return v + np.where(cross, t, zero)


def running_sum(t):
    """the terms of the last axis added left to right in float32, from 0 (a zero behind a band's end changes nothing)"""
    return np.cumsum(t, axis=-1, dtype=np.float32)[..., -1]


def strict_sum(T, t):
    """band_sum: a band's terms in line order -> [M][22]"""
    return running_sum(np.where(T.b_valid, t[..., T.b_idx], F(0.0)))


def lane_sums(T, t, slow=None):
    """the band totals as the lanes form them: [M][576] terms -> [M][22]"""
    tl = np.where(T.l_valid, t[..., T.l_idx], F(0.0))
    part = pair_tree(tl)
    if slow is not None and slow.any():
        part = np.where(slow[..., None], pair_after_pair(tl), part)
    return seg_scan(part, T.l_d)[..., T.last]


def line_terms(T, xr, x34, g):
    """the noise terms of a sweep that measures band b at step g[.., b] (-1: not), and which bands take the double table"""
    meas = g >= 0
    gi = np.clip(g, 0, 127)
    bl = T.band_of_line
    with np.errstate(all="ignore"):
        igl, gnl, ml = T.igain[gi][..., bl], T.gain[gi][..., bl], meas[..., bl]
        tmp = igl * x34 + C0946
        qx = np.where(ml, np.trunc(tmp + np.copysign(HALF, tmp)), 0).astype(np.int64)
        d = xr - gnl * T.ix43[np.clip(qx, 0, 255)]
        big = qx >= 256
        if big.any():
            d = np.where(big, xr - (gnl.astype(np.float64) * T.pow43(qx)).astype(np.float32), d)
        return np.where(ml, d * d, F(0.0)), qx


def sweep(T, xr, x34, x34max, g, forced=False):
    """one noise_sweep per row -> noise [M][22] (the strict sum's: the oracle's), and per band whether the device adds it
    strictly, whether the lanes' bucket is another than the strict sum's, and per row whether the pass takes the double table"""
    g = np.where(np.arange(22) < T.nb, g, -1)        # (the other bands have no lanes: no record measures them)
    meas = g >= 0
    gi = np.clip(g, 0, 127)
    with np.errstate(all="ignore"):
        tmp = T.igain[gi] * x34max + C0946
        slow = (meas & (np.trunc(tmp + np.copysign(HALF, tmp)) >= 256)).any(axis=-1)
        t, _ = line_terms(T, xr, x34, g)
        tree, exact = lane_sums(T, t, slow), strict_sum(T, t)
        e = tree * T.du
        cert = bucket(TINY + (tree - e)) == bucket(TINY + (tree + e))
        differs = meas & (bucket(TINY + tree) != bucket(TINY + exact))
        strict = meas & ~cert
        assert not (differs & ~strict).any(), "a certificate passed a band whose lane sum is in another bucket than the strict sum"
        if forced:
            strict = meas
        return T.mblog(TINY + exact) - T.logcbw, strict, differs, slow


def seek(T, xr, x34, x34max, nsf, NT, Noise0, gsf, gzero, ntadj, forced=False):
    """seek_actual_ch on every row: all bands of a channel advance in the same sweep.  -> dict: gsf, Noise, NTadjust [M][22];
    per row sweeps, strict (sweeps with a band added strictly), big (double-table passes); per band differs (measurements whose
    lane bucket is not the strict sum's), measured (measurements), and the step list's end: "kind" 0 not measured, 1 settled,
    2 / 3 walked down / up to the target, 4 / 5 walked down / up until the steps were used"""
    M = xr.shape[0]
    band = np.arange(22)[None, :] < nsf[:, None]
    mode = np.where(band & (Noise0 > NT), 1, 0)
    s, t = gsf.copy(), np.zeros_like(gsf)
    smin, tnmin = np.where(band & (mode == 0), gzero + 5, gsf), np.where(band & (mode == 0), Noise0, 0)
    absmin, it, niter, ntadj = np.zeros_like(gsf), np.zeros_like(gsf), np.zeros_like(gsf), ntadj.copy()
    kind = np.zeros_like(gsf)
    res = dict(sweeps=np.zeros(M, int), strict=np.zeros(M, int), big=np.zeros(M, int), differs=np.zeros((M, 22), int), measured=np.zeros((M, 22), int))
    while (mode != 0).any():
        rows = (mode != 0).any(axis=1)
        g = np.where(mode == 0, -1, np.where(mode == 1, s, t))
        noise, strict, differs, slow = sweep(T, xr, x34, x34max, g, forced)
        res["sweeps"] += rows
        res["strict"] += strict.any(axis=1)
        res["big"] += slow
        res["differs"] += differs
        res["measured"] += g >= 0
        first, walk = mode == 1, mode >= 2
        dn = noise - NT
        ntadj = np.where(first, ntadj + (dn >> 3), ntadj)
        ad = np.abs(dn)
        better = first | (walk & (ad < absmin))
        absmin, tnmin, smin = np.where(better, ad, absmin), np.where(better, noise, tnmin), np.where(better, np.where(first, s, t), smin)
        it = np.where(first, 0, it + walk)
        down, up = first & (dn > 100), first & (dn < -100)
        niter = np.where(down, np.minimum(s - 1, 20), np.where(up, 20, niter))
        stop = np.where(mode == 2, noise <= NT, noise >= NT)
        done = walk & (stop | (it >= niter))
        kind = np.where(first, 1, kind)
        kind = np.where(down & (niter <= 0), 4, kind)
        kind = np.where(done, np.where(stop, mode, mode + 2), kind)
        nmode = np.where(first, np.where(down, np.where(niter > 0, 2, 0), np.where(up, 3, 0)), np.where(done, 0, mode))
        t = np.where(down, s - 1, np.where(up, s + 1, np.where(walk & ~done, np.where(mode == 2, t - 1, t + 1), t)))
        mode = nmode
    res.update(gsf=np.where(band, smin, gsf), Noise=np.where(band, tnmin, 0), NTadjust=ntadj, kind=kind)
    return res


def isf2(T, xr, ix, ixmax, nsf, G, scale, up, lo, sf, forced=False):
    """isf2_ch on every row -> dict: sf [M][22], sel, per row strict (0 / 1: the channel added a band strictly), per band differs"""
    sel = (np.arange(22)[None, :] < nsf[:, None]) & ((ixmax == 1) | (ixmax == 2))
    q = T.ix43[np.minimum(ix, 255)]
    tq, tx = q * q, xr * xr
    with np.errstate(all="ignore"):
        qt, xt, qs, xs = lane_sums(T, tq), lane_sums(T, tx), strict_sum(T, tq), strict_sum(T, tx)
        eq, ex = qt * T.du, xt * T.du
        cert = bucket((xt - ex) / (qt + eq)) == bucket((xt + ex) / (qt - eq))
        differs = sel & (bucket(xt / qt) != bucket(xs / qs))
        strict = sel & ~cert
        assert not (differs & ~strict).any(), "a certificate passed a band whose quotient of lane sums is in another bucket than the strict sums'"
        if forced:
            strict = sel
        t = 54 * T.mblog(np.where(sel, xs / qs, F(1.0))) + (8 << 13)
    sh = np.where(scale != 0, 14, 13)[:, None]
    s = (((G[:, None] << 13) - t + (1 << sh)) & ~((1 << (sh + 1)) - 1)) >> 13
    free = s
    s = np.maximum(np.minimum(s, up), lo)
    return dict(sf=np.where(sel, s, sf), free=free, sel=sel, strict=strict.any(axis=1).astype(int), differs=differs.astype(int))


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------

class Records:
    """one (mode, rate)'s records in the layout of hx_debug_seek (include/hmp3_amd.h); arrays once frozen"""
    KEYS = ("hdr", "xr", "x34", "ix", "band", "x34max")

    def __init__(self, mode, sr):
        self.mode, self.sr, self.T = mode, sr, tables(sr)
        self.rules, self.lists = [], []
        for k in self.KEYS:
            setattr(self, k, [])

    def add(self, lst, rule, xr, nsf, nchan=2, x34=None, ix=None, G=(0, 0), scale=(0, 0), **bands):
        """bands: seek NT, Noise0, gsf, gzero, NTadjust; isf2 up, lo, sf - each [2][22] or a scalar"""
        T = self.T
        h = np.zeros(16, np.int32)
        nsf = [int(nsf[c]) if c < nchan else 0 for c in range(2)]
        h[:9] = [nchan, nsf[0], nsf[1], T.start[nsf[0]], T.start[nsf[1]] if nchan == 2 else 0, G[0], G[1], scale[0], scale[1]]
        w = np.zeros((2, 22, 8), np.int32)
        names = ("NT", "Noise0", "gsf", "gzero", "NTadjust") if self.mode == "seek" else ("up", "lo", "sf")
        for k, name in enumerate(names):
            w[:, :, k] = bands.get(name, 0)
        x34 = np.zeros((2, 576), np.float32) if x34 is None else np.asarray(x34, np.float32).reshape(2, 576)
        ix = np.zeros((2, 576), np.int32) if ix is None else np.asarray(ix, np.int32).reshape(2, 576)
        edges = np.append(T.start[:22], 576)
        if self.mode == "isf2":
            w[:, :, 3] = np.maximum.reduceat(ix, T.start[:22], axis=1)
        self.x34max.append(np.maximum.reduceat(x34, T.start[:22], axis=1).astype(np.float32))
        assert edges[-1] == 576
        self.rules.append(rule), self.lists.append(lst), self.hdr.append(h), self.band.append(w)
        self.xr.append(np.asarray(xr, np.float32).reshape(2, 576).copy()), self.x34.append(x34.copy()), self.ix.append(ix.copy())
        return len(self.rules) - 1

    def freeze(self):
        for k in self.KEYS:
            a = np.stack(getattr(self, k))
            a.setflags(write=False)
            setattr(self, k, a)
        self.n = len(self.rules)
        self.lists = np.array(self.lists)
        return self

    def pick(self, keep):
        return {k: np.ascontiguousarray(getattr(self, k)[keep]) for k in self.KEYS}

    def rows(self, lst):
        return np.flatnonzero(self.lists == lst)


def restate(R, forced=False, keep=None):
    """the restatement on the records `keep` of R -> its dict, rows [2 r + channel]; "nstrict" and "big" per record"""
    a = R.pick(np.arange(R.n) if keep is None else keep)
    n = a["hdr"].shape[0]
    nsf = a["hdr"][:, 1:3].reshape(-1).astype(int)
    w = a["band"].reshape(2 * n, 22, 8).astype(np.int64)
    if R.mode == "seek":
        res = seek(R.T, a["xr"].reshape(-1, 576), a["x34"].reshape(-1, 576), a["x34max"].reshape(-1, 22), nsf, w[..., 0], w[..., 1], w[..., 2], w[..., 3], w[..., 4], forced)
        res["big"] = res["big"].reshape(n, 2).sum(axis=1)
    else:
        res = isf2(R.T, a["xr"].reshape(-1, 576), a["ix"].reshape(-1, 576).astype(int), w[..., 3], nsf, a["hdr"][:, 5:7].reshape(-1).astype(np.int64),
                   a["hdr"][:, 7:9].reshape(-1), w[..., 0], w[..., 1], w[..., 2], forced)
    res["nstrict"] = res["strict"].reshape(n, 2).sum(axis=1)
    return res


def expected(R, keep=None):
    """the oracle's out [n][184] (hxo_seek_record / hxo_isf2_record)"""
    a = R.pick(np.arange(R.n) if keep is None else keep)
    return O.noise_records(R.T.o, R.mode, a["hdr"], a["xr"], a["band"], x34=a["x34"], ix=a["ix"])


FIELDS = {"seek": ("gsf", "Noise", "NTadjust", "geval"), "isf2": ("sf", "geval")}


def first_difference(R, keep, got, want):
    """None, or "record r (rule) channel c band b: field got x, want y" of the first of the band words that differs"""
    f = FIELDS[R.mode]
    g, w = got[:, :176].reshape(-1, 2, 22, 4)[..., :len(f)], want[:, :176].reshape(-1, 2, 22, 4)[..., :len(f)]
    bad = np.argwhere(g != w)
    if not len(bad):
        return None
    r, c, b, k = bad[0]
    return "record %d (%s: %s) channel %d band %d: %s is %d, the oracle's %d" % (keep[r], R.lists[keep[r]], R.rules[keep[r]], c, b, f[k], g[r, c, b, k], w[r, c, b, k])


def runs(unit, R):
    rule = LEFT_OUT.get(unit)
    return np.array([i for i in range(R.n) if rule is None or not rule(R.rules[i])])


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------

def spectrum(T, rng, lo=5.0, hi=2000.0, nchan=2):
    """magnitudes [2][576] with a level of its own per band, and their x^(3/4) (the oracle's pow34)"""
    amp = np.exp(rng.uniform(np.log(lo), np.log(hi), (2, 22)))[:, T.band_of_line]
    xr = (np.abs(rng.standard_normal((2, 576))) * amp + 0.01).astype(np.float32)
    if nchan == 1:
        xr[1] = 0
    x34 = np.zeros_like(xr)
    O.lib().hxo_pow34.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    O.lib().hxo_pow34(xr.ctypes.data, x34.ctypes.data, xr.size)
    return xr, x34


def noise_table(T, xr, x34, steps=range(128)):
    """the strict noise of every band of one channel at the gain steps `steps` -> [128][22] (zeros at the other steps)"""
    steps = np.array(sorted(set(int(v) for v in steps if 0 <= v < 128)))
    x34max = np.maximum.reduceat(x34, T.start[:22]).astype(np.float32)
    g = np.where(np.arange(22)[None, :] < T.nb, np.repeat(steps[:, None], 22, axis=1), -1)     # (the other bands have no lanes)
    n = len(steps)
    N = np.zeros((128, 22), np.int64)
    N[steps] = sweep(T, np.broadcast_to(xr, (n, 576)), np.broadcast_to(x34, (n, 576)), np.broadcast_to(x34max, (n, 22)), g)[0]
    return N


WALK_RULES = ("unmeasured", "dn=100", "dn=101", "dn=-100", "dn=-101", "down to target", "down 20 steps", "start 1", "start 2", "start 3",
              "up to target", "up 20 steps", "tie down", "tie up", "dn=-5")


def walk_band(rule, N, rng, s):
    """(start step, NT, Noise0) that put a band with noise table N [128] (steps s - 21 .. s + 21 and 0 .. 3) into the state `rule`
    names from start step s; None if N has no such place"""
    if rule == "unmeasured":
        return s, int(N[s]), int(N[s]) - int(rng.integers(0, 2))
    if rule.startswith("dn="):
        return s, int(N[s]) - int(rule[3:]), 100000
    if rule == "down to target":
        k = next((int(k) for k in rng.permutation(np.arange(2, 19)) if N[s] - N[s - k] > 100), None)
        return k and (s, int(N[s - k]), 100000)
    if rule == "down 20 steps":
        return s, int(N[s - 20:s].min()) - 500, 100000
    if rule.startswith("start "):
        s = int(rule[6:])
        return s, int(N[0]) - 2000, 100000
    if rule == "up to target":
        k = next((int(k) for k in rng.permutation(np.arange(2, 19)) if N[s + k] - N[s] > 100), None)
        return k and (s, int(N[s + k]), 100000)
    if rule == "up 20 steps":
        return s, int(N[s + 1:s + 21].max()) + 500, 100000
    if rule in ("tie down", "tie up"):
        # two neighbouring steps as far above as below the target: the walk meets the far one first and keeps it
        sg = -1 if rule == "tie down" else 1
        for k in rng.permutation(np.arange(2, 18)):
            a, b = int(N[s + sg * k]), int(N[s + sg * (k + 1)])
            nt = (a + b) // 2
            before = N[s + sg * np.arange(0, k)]        # the first measurement and the steps of the walk before the two
            if (a + b) % 2 == 0 and sg * (b - a) >= 2 and (sg * (nt - before) > abs(a - nt)).all() and sg * (nt - int(N[s])) > 100:
                return s, nt, 100000
        return None
    if rule == "dn=-5":
        return s, int(N[s]) + 5, 100000
    raise KeyError(rule)


WALK_CANDIDATES = 3     # draws of a group per round
WALK_ROUNDS = 10


def build_walk(R, rng):
    """Groups of records, drawn WALK_CANDIDATES at a time: the first draw on which the restatement sees no certificate fail in any
    sweep is the one the list keeps, so that the list's expected count of strict fall-backs is zero"""
    T = R.T
    tmp = None

    def channel(rule_of, c, nsf):
        """lines and band words of one channel: band b starts at a step of its own and its largest line quantises to about 12
        there - below 256 twenty steps down, above zero twenty steps up, so the noise moves with every step of a walk"""
        s0 = int(rng.integers(24, 60))
        step = np.array([int(rule_of(c, b)[6:]) if rule_of(c, b).startswith("start ") else s0 + int(rng.integers(0, 4)) for b in range(22)])
        top = (12.0 * rng.uniform(0.7, 1.3, 22) / T.igain[step]) ** (4.0 / 3.0)
        shape = np.abs(rng.standard_normal(576)) + 0.05
        shape /= np.maximum.reduceat(shape, T.start[:22])[T.band_of_line]
        xr = (shape * top[T.band_of_line]).astype(np.float32)
        x34 = np.zeros_like(xr)
        O.lib().hxo_pow34.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        O.lib().hxo_pow34(xr.ctypes.data, x34.ctypes.data, xr.size)
        N = noise_table(T, xr, x34, list(range(s0 - 21, s0 + 26)) + list(range(25)))
        w = np.zeros((22, 5), np.int64)
        w[:, 3], w[:, 4] = rng.integers(0, 123, 22), rng.integers(-400, 401, 22)
        for b in range(nsf):
            got = walk_band(rule_of(c, b), N[:, b], rng, int(step[b])) or walk_band("dn=-5", N[:, b], rng, int(step[b]))
            w[b, 2], w[b, 0], w[b, 1] = got
        return xr, x34, w

    def record(rule_of, nchan=2, nsf=None, tag="", ch0=None):
        nsf = nsf or (T.nb, T.nb)
        xr, x34, w = np.zeros((2, 576), np.float32), np.zeros((2, 576), np.float32), np.zeros((2, 22, 5), np.int64)
        for c in range(nchan):
            xr[c], x34[c], w[c] = ch0 if (c == 0 and ch0) else channel(rule_of, c, nsf[c])
        words = dict(NT=w[..., 0], Noise0=w[..., 1], gsf=w[..., 2], gzero=w[..., 3], NTadjust=w[..., 4])
        return tmp.add("walk", tag + " | ".join(rule_of(c, 0) for c in range(nchan)), xr, nsf, nchan, x34=x34, **words), (xr[0], x34[0], w[0])

    makers = []

    def single(*a, **kw):
        makers.append(lambda: [record(*a, **kw)[0]])

    def beside():       # one channel 0 beside three channels 1
        first, ch0 = record(lambda c, b: WALK_RULES[(b + 3) % len(WALK_RULES)], tag="beside 0: ")
        return [first] + [record(lambda c, b, k=k: WALK_RULES[(b + 3 + 4 * k * c) % len(WALK_RULES)], tag="beside %d: " % k, ch0=ch0)[0] for k in (1, 2)]

    for i, rule in enumerate(WALK_RULES):
        single(lambda c, b, rule=rule: rule)                                    # every band of both channels in the state
        if i % 2 == 0:
            single(lambda c, b, i=i: WALK_RULES[(i + b + 7 * c) % len(WALK_RULES)], tag="mixed: ")
    single(lambda c, b: WALK_RULES[b % len(WALK_RULES)], nsf=(T.nb, max(T.nb - 5, 1)), tag="nsf differ: ")
    single(lambda c, b: WALK_RULES[b % len(WALK_RULES)], nsf=(max(T.nb - 9, 1), T.nb), tag="nsf differ: ")
    for rule in ("down 20 steps", "up to target", "dn=100"):
        single(lambda c, b, rule=rule: rule, nchan=1, tag="mono: ")
    single(lambda c, b: "dn=100" if c == 0 else "up 20 steps", tag="channel 1 goes on: ")
    single(lambda c, b: "down 20 steps" if c == 0 else "unmeasured", tag="channel 0 goes on: ")
    makers.append(beside)
    chosen = [None] * len(makers)
    for _ in range(WALK_ROUNDS):
        pending = [k for k in range(len(makers)) if chosen[k] is None]
        if not pending:
            break
        tmp = Records("seek", R.sr)
        draws = [(k, makers[k]()) for k in pending for _ in range(WALK_CANDIDATES)]
        tmp.freeze()
        clean = restate(tmp)["nstrict"] == 0
        for k, rows in draws:
            if chosen[k] is None and clean[rows].all():
                chosen[k] = [(tmp.rules[i], {key: getattr(tmp, key)[i].copy() for key in R.KEYS}) for i in rows]
    assert all(c is not None for c in chosen), "a group of the walk list has no draw free of strict fall-backs"
    for group in chosen:
        for rule, arrays in group:
            R.rules.append(rule), R.lists.append("walk")
            for key in R.KEYS:
                getattr(R, key).append(arrays[key])


def settled(R, lst, rule, xr, x34, nsf, nchan, measure, rng, walk=0):
    """a record whose bands `measure` [2][22] are measured at a random step and settle there (walk: the target up to that far
    from the first measurement, so that some go on for a step or two)"""
    T = R.T
    w = {k: np.zeros((2, 22), np.int64) for k in ("NT", "Noise0", "gsf", "gzero", "NTadjust")}
    w["gsf"][:] = rng.integers(20, 100, (2, 22))
    w["gzero"][:] = rng.integers(0, 123, (2, 22))
    for c in range(nchan):
        x34max = np.maximum.reduceat(x34[c], T.start[:22]).astype(np.float32)
        N = sweep(T, xr[c][None], x34[c][None], x34max[None], w["gsf"][c][None])[0][0]
        w["NT"][c] = N + (rng.integers(-walk, walk + 1, 22) if walk else 0)
        w["Noise0"][c] = np.where(measure[c], 100000, w["NT"][c] - 7)
    return R.add(lst, rule, xr, nsf, nchan, x34=x34, **w)


def build_layout(R, rng):
    T = R.T
    for b in range(T.nb):       # each band alone, on either channel; the other channel measures nothing or another band
        for c in range(2):
            xr, x34 = spectrum(T, rng)
            m = np.zeros((2, 22), bool)
            m[c, b] = True
            if b & 1:
                m[1 - c, (b + 5) % T.nb] = True
            settled(R, "layout", "band %d of channel %d alone" % (b, c), xr, x34, (T.nb, T.nb), 2, m, rng, walk=200 if b % 3 == 0 else 0)
    for k in range(6):          # every band, lines up to 575
        xr, x34 = spectrum(T, rng)
        settled(R, "layout", "every band", xr, x34, (T.nb, T.nb), 2, np.ones((2, 22), bool), rng, walk=300 if k & 1 else 0)
    for k in range(4):          # fewer bands than the class has, with and without a pattern in the lines behind them
        nsf = (int(rng.integers(1, T.nb)), int(rng.integers(1, T.nb)))
        xr, x34 = spectrum(T, rng)
        state = rng.bit_generator.state
        for sentinel in (0, 1):
            rng.bit_generator.state = state
            y, y34 = xr.copy(), x34.copy()
            for c in range(2):
                y[c, T.start[nsf[c]]:] = SENTINEL * sentinel
                y34[c, T.start[nsf[c]]:] = SENTINEL * sentinel
            settled(R, "layout", "nsf %d %d, %s behind" % (nsf + ("sentinel" if sentinel else "zeros",)), y, y34, nsf, 2, np.ones((2, 22), bool), rng, walk=200)


def bisect_line(value, lo, hi, target):
    """the largest bit pattern u in [lo, hi) with bucket(value(u)) < target, per candidate; value is monotone in u and
    bucket(value(lo)) < target <= bucket(value(hi))"""
    lo, hi = lo.copy(), hi.copy()
    while (hi - lo > 1).any():
        mid = (lo + hi) >> 1
        below = bucket(value(mid)) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return lo


def edge_lines(T, rng, n, tail=12):
    """K bands' lines [K][maxw] (zeros behind each band's n[k] lines) whose strict sum of squares lies on a bucket boundary: one of
    the last lines is bisected until the sum is the largest below the boundary (u) - the next pattern (u + 1) is across it.
    -> (lines with u, lines with u + 1)"""
    K = len(n)
    j = np.arange(T.maxw)[None, :]
    x = (np.abs(rng.standard_normal((K, T.maxw))) * np.exp(rng.uniform(np.log(0.5), np.log(500.0), (K, 1))) + 0.01).astype(np.float32)
    x = np.where(j < n[:, None], x, F(0.0))
    pos = n - 1 - rng.integers(0, np.minimum(n, tail))
    rows = np.arange(K)
    x[rows, pos] = x.max(axis=1)        # (a line large enough for the sum to cross the next boundary within 16 times its square)

    def total(u):
        y = x.copy()
        y[rows, pos] = from_bits(u)
        return TINY + running_sum(y * y)
    lo = bits(x[rows, pos])
    hi = bits(x[rows, pos] * F(4.0))
    target = bucket(total(lo)) + 1
    assert (bucket(total(hi)) >= target).all()
    u = bisect_line(total, lo, hi, target)
    a, b = x.copy(), x.copy()
    a[rows, pos], b[rows, pos] = from_bits(u), from_bits(u + 1)
    return a, b


def band_rows(T, nrec):
    """(record, channel, band) of every band with lanes in nrec records, and the bands' widths"""
    r, c, b = np.meshgrid(np.arange(nrec), np.arange(2), np.arange(T.nb), indexing="ij")
    return r.reshape(-1), c.reshape(-1), b.reshape(-1), T.width[b.reshape(-1)]


def place(T, xr, r, c, b, lines):
    for k in range(len(r)):
        xr[r[k], c[k], T.start[b[k]]:T.start[b[k]] + T.width[b[k]]] = lines[k, :T.width[b[k]]]


def pick_differing(T, a, b, differs):
    """per band the variant of a / b whose lane bucket is not the strict sum's (a if neither is)"""
    da, db = differs(a), differs(b)
    take_b = db & ~da
    return np.where(take_b[..., None], b, a)


def squares_record(R, lst, rule, xr, rng, loud=None):
    """a record of bands whose x^(3/4) is zero - every term is x * x at every step - each measured once at a random step with
    its own noise as the target.  loud (channel, band, step): that band's x^(3/4) quantises to 256 and more at the step, so the
    one sweep of that channel is a double-table pass"""
    T = R.T
    x34 = np.zeros((2, 576), np.float32)
    gsf = rng.integers(0, 108, (2, 22))
    if loud:
        c, b, s, qx = loud
        sl = slice(T.start[b], T.start[b] + T.width[b])
        x34[c, sl] = (rng.uniform(0.3, 1.0, T.width[b]) * (qx / T.igain[s])).astype(np.float32)
        x34[c, T.start[b]] = F(qx / T.igain[s])
        xr[c, sl] = (x34[c, sl].astype(np.float64) ** (4.0 / 3.0)).astype(np.float32)
        gsf[c, b] = s
    N = np.stack([sweep(T, xr[c][None], x34[c][None], np.maximum.reduceat(x34[c], T.start[:22])[None].astype(np.float32), gsf[c][None])[0][0] for c in range(2)])
    return R.add(lst, rule, xr, (T.nb, T.nb), 2, x34=x34, NT=N, Noise0=100000, gsf=gsf, gzero=rng.integers(0, 123, (2, 22)))


def lane_differs(T, r, c, b, nrec, loud_rows=None):
    """for bands of squares placed at (r, c, b): does the lanes' bucket differ from the strict sum's -> f(lines [K][maxw]) -> [K]"""
    def f(lines):
        xr = np.zeros((nrec, 2, 576), np.float32)
        place(T, xr, r, c, b, lines)
        t = (xr * xr).reshape(-1, 576)
        slow = None if loud_rows is None else loud_rows.reshape(-1)
        tree, exact = lane_sums(T, t, slow), strict_sum(T, t)
        return (bucket(TINY + tree) != bucket(TINY + exact)).reshape(nrec, 2, 22)[r, c, b]
    return f


def build_bucket_edge(R, rng, lst="bucket_edge", nrec=EDGE_RECORDS, loud=False):
    T = R.T
    r, c, b, n = band_rows(T, nrec)
    lo_lines, hi_lines = edge_lines(T, rng, n)
    loud_rows = None
    if loud:        # the first band of channel r & 1 is the loud one: that channel's lanes add pair after pair
        loud_rows = np.zeros((nrec, 2), bool)
        loud_rows[np.arange(nrec), np.arange(nrec) & 1] = True
    lines = pick_differing(T, lo_lines, hi_lines, lane_differs(T, r, c, b, nrec, loud_rows))
    xr = np.zeros((nrec, 2, 576), np.float32)
    place(T, xr, r, c, b, lines)
    for k in range(nrec):
        if loud:
            squares_record(R, lst, "edges beside a loud band", xr[k], rng, loud=(k & 1, 0, int(rng.integers(0, 20)), int(rng.integers(256, 2000))))
        else:
            squares_record(R, lst, "every band on a boundary", xr[k], rng)


def worst_lines(T, n, e, sqq=None):
    """a band of n lines: one whose square L is the largest below the boundary 2^e (1 + 2^-8) - with sqq, the largest whose
    quotient L / sqq is below it - then n - 1 whose squares are the largest below half an ulp of L: the strict sum drops every
    one of them, the lanes' runs add them up first and keep them.  The boundary's mantissa is next to 1, where an ulp is
    largest against the value: the two sums are (n - 3) 2^-24 apart in relative terms at the least, which c = n + W + 16 covers
    and n / 2 does not"""
    B = F(2.0 ** e) * (F(1.0) + F(2.0 ** -8))
    div = F(1.0) if sqq is None else F(sqq)

    def largest_below(limit, div):
        root = np.sqrt(F(limit) * div)
        lo, hi = int(bits(root * F(0.5))[0]), int(bits(root * F(2.0))[0])
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            v = from_bits(mid)[0]
            lo, hi = (mid, hi) if (v * v) / div < limit else (lo, mid)
        return from_bits(lo)[0]
    x0 = largest_below(B, div)
    L = x0 * x0
    half_ulp = from_bits(((int(bits(L)[0]) >> 23) - 24) << 23)[0]
    out = np.zeros(T.maxw, np.float32)
    out[:n] = largest_below(half_ulp, F(1.0))
    out[0] = x0
    return out


def build_worst_case(R, rng):
    T = R.T
    for k in range(4):
        xr = np.zeros((2, 576), np.float32)
        for c in range(2):
            for b in range(T.nb):
                xr[c, T.start[b]:T.start[b] + T.width[b]] = worst_lines(T, T.width[b], int(rng.integers(-8, 24)))[:T.width[b]]
        squares_record(R, "worst_case", "one large term, then terms under half its ulp", xr, rng)


def build_double_table(R, rng):
    T = R.T
    # quantised values from 256 up, beyond 16384: in one band only, in several
    for k, qx in enumerate((256, 257, 300, 1000, 8000, 16383, 16384, 16400, 20000)):
        for several in (0, 1):
            xr, x34 = spectrum(T, rng, hi=50.0)
            s = int(rng.integers(0, 12))
            gsf = rng.integers(s, 40, (2, 22))
            for c, b in ([(k & 1, k % T.nb)] if not several else [(0, 0), (0, 3), (1, 1), (1, min(5, T.nb - 1))]):
                sl = slice(T.start[b], T.start[b] + T.width[b])
                x34[c, sl] = (rng.uniform(0.2, 1.0, T.width[b]) * (qx / T.igain[s])).astype(np.float32)
                x34[c, T.start[b] + int(rng.integers(0, T.width[b]))] = F((qx + 0.2) / T.igain[s])
                xr[c, sl] = (x34[c, sl].astype(np.float64) ** (4.0 / 3.0) * rng.uniform(0.97, 1.03, T.width[b])).astype(np.float32)
                gsf[c, b] = s
            N = np.stack([sweep(T, xr[c][None], x34[c][None], np.maximum.reduceat(x34[c], T.start[:22])[None].astype(np.float32), gsf[c][None])[0][0] for c in range(2)])
            R.add("double_table", "values to %d in %s" % (qx, "several bands" if several else "one band"), xr, (T.nb, T.nb), 2, x34=x34,
                  NT=N + rng.integers(-250, 251, (2, 22)), Noise0=100000, gsf=gsf, gzero=rng.integers(0, 123, (2, 22)))
    # a bucket edge inside a double-table pass: the strict sum finds its terms stored (have_terms = 1)
    build_bucket_edge(R, rng, "double_table", nrec=4, loud=True)
    # a double-table pass, then plain sweeps with a strict band: the loud band's first measurement takes the double table and
    # settles or walks up out of it, while the bands of squares walk up beside it - their noise is the same at every step, so
    # each is on its boundary in every later sweep, which must form its terms anew (have_terms = 0)
    r, c, b, n = band_rows(T, 4)
    lo_lines, hi_lines = edge_lines(T, rng, n)
    lines = pick_differing(T, lo_lines, hi_lines, lane_differs(T, r, c, b, 4))
    xr4 = np.zeros((4, 2, 576), np.float32)
    place(T, xr4, r, c, b, lines)
    for k in range(4):
        xr, x34 = xr4[k], np.zeros((2, 576), np.float32)
        s = int(rng.integers(2, 20))
        gsf = rng.integers(0, 80, (2, 22))
        NT, gz = np.zeros((2, 22), np.int64), rng.integers(0, 123, (2, 22))
        for c in range(2):
            sl = slice(T.start[0], T.start[0] + T.width[0])
            x34[c, sl] = F(258.0 / T.igain[s])
            xr[c, sl] = F(np.float64(T.gain[s]) * T.pow43_tab[258])       # (no noise at the start step, more at every step above)
            gsf[c, 0] = s
            N = noise_table(T, xr[c], x34[c])
            NT[c] = N[gsf[c], np.arange(22)] + 500          # the squares never get there: 20 steps up
            NT[c, 0] = N[s + (3 if k & 1 else 0), 0]          # the loud band settles at once, or walks three steps up
        R.add("double_table", "a strict band in the plain sweeps behind a double-table pass", xr, (T.nb, T.nb), 2, x34=x34,
              NT=NT, Noise0=100000, gsf=gsf, gzero=gz)


def lines_of_maxima(T, rng, maxima):
    ix = np.zeros(576, np.int32)
    for b in range(22):
        m, lo, hi = int(maxima[b]), T.start[b], T.start[b] + T.width[b] if b < 21 else 576
        if m > 0 and hi > lo:
            ix[lo:hi] = rng.integers(0, m + 1, hi - lo)
            ix[rng.integers(lo, hi)] = m
    return ix


def isf2_record(R, lst, rule, xr, ix, rng, nsf=None, nchan=2, G=None, scale=None, clamp=None):
    """clamp: per band 0 inside the limits, 1 the free value above up, 2 below lo (needs the free value: the restatement's)"""
    T = R.T
    nsf = nsf or (T.nb, T.nb)
    G = rng.integers(0, 256, 2) if G is None else G
    scale = rng.integers(0, 2, 2) if scale is None else scale
    ixmax = np.maximum.reduceat(np.asarray(ix), T.start[:22], axis=1)
    z = np.zeros((2, 22), np.int64)
    free = isf2(T, np.asarray(xr, np.float32), np.asarray(ix).astype(int), ixmax, np.array(nsf), np.asarray(G, np.int64), np.asarray(scale), z + 255, z, z)["free"]
    clamp = rng.integers(0, 3, (2, 22)) if clamp is None else clamp
    lo = np.clip(np.where(clamp == 2, free + rng.integers(1, 9, (2, 22)), free - rng.integers(0, 9, (2, 22))), 0, 255)
    up = np.clip(np.where(clamp == 1, free - rng.integers(1, 9, (2, 22)), free + rng.integers(0, 9, (2, 22))), lo, 255)
    return R.add(lst, rule, xr, nsf, nchan, ix=ix, G=G, scale=scale, up=up, lo=lo, sf=rng.integers(0, 256, (2, 22)))


def build_select(R, rng):
    T = R.T
    pattern = np.array([0, 1, 2, 3, 8191])
    for k in range(40):
        xr, _ = spectrum(T, rng, lo=0.05, hi=50.0)
        maxima = np.stack([pattern[(np.arange(22) + k + 2 * c) % 5] for c in range(2)])
        ix = np.stack([lines_of_maxima(T, rng, maxima[c]) for c in range(2)])
        # G across its range on either scale: a low G sends every band below lo, a high one above up
        isf2_record(R, "select", "maxima 0 1 2 3 8191 side by side", xr, ix, rng, G=np.array([(k * 13) % 256, 255 - (k * 7) % 256]), scale=np.array([k & 1, (k >> 1) & 1]))
    for k in range(40):
        xr, _ = spectrum(T, rng, lo=0.05, hi=50.0)
        ix = np.stack([lines_of_maxima(T, rng, rng.integers(1, 3, 22)) for c in range(2)])
        isf2_record(R, "select", "every band refined, clamp %d" % (k % 3), xr, ix, rng, G=rng.integers(120, 200, 2), clamp=np.full((2, 22), k % 3))
    for k in range(4):
        xr, _ = spectrum(T, rng)
        ix = np.stack([lines_of_maxima(T, rng, np.array([0, 3, 8191, 5])[rng.integers(0, 4, 22)]) for c in range(2)])
        isf2_record(R, "select", "no band refined", xr, ix, rng)
    for k in range(8):
        xr, _ = spectrum(T, rng, nchan=1)
        ix = np.stack([lines_of_maxima(T, rng, rng.integers(0, 4, 22)), np.zeros(576, np.int32)])
        isf2_record(R, "select", "mono", xr, ix, rng, nchan=1)
    for k in range(12):
        nsf = (int(rng.integers(1, T.nb + 1)), int(rng.integers(1, T.nb + 1)))
        xr, _ = spectrum(T, rng)
        ix = np.stack([lines_of_maxima(T, rng, rng.integers(0, 4, 22)) for c in range(2)])
        isf2_record(R, "select", "nsf %d %d" % nsf, xr, ix, rng, nsf=nsf)


def ratio_differs(T, r, c, b, nrec, ix):
    def f(lines):
        xr = np.zeros((nrec, 2, 576), np.float32)
        place(T, xr, r, c, b, lines)
        q = T.ix43[np.minimum(ix, 255)].reshape(-1, 576)
        tx = (xr * xr).reshape(-1, 576)
        with np.errstate(all="ignore"):
            return (bucket(lane_sums(T, tx) / lane_sums(T, q * q)) != bucket(strict_sum(T, tx) / strict_sum(T, q * q))).reshape(nrec, 2, 22)[r, c, b]
    return f


def build_ratio_edge(R, rng, nrec=EDGE_RECORDS):
    """every band refined and its quotient sxx / sqq on a bucket boundary: one line bisected against the band's strict sqq"""
    T = R.T
    r, c, b, n = band_rows(T, nrec)
    K = len(r)
    ix = np.stack([np.stack([lines_of_maxima(T, rng, rng.integers(1, 3, 22)) for _ in range(2)]) for _ in range(nrec)])
    q = T.ix43[ix]
    sqq = strict_sum(T, (q * q).reshape(-1, 576)).reshape(nrec, 2, 22)[r, c, b]
    j = np.arange(T.maxw)[None, :]
    x = (np.abs(rng.standard_normal((K, T.maxw))) * np.exp(rng.uniform(np.log(0.05), np.log(50.0), (K, 1))) + 0.01).astype(np.float32)
    x = np.where(j < n[:, None], x, F(0.0))
    pos = n - 1 - rng.integers(0, np.minimum(n, 12))
    rows = np.arange(K)
    x[rows, pos] = x.max(axis=1)

    def quotient(u):
        y = x.copy()
        y[rows, pos] = from_bits(u)
        return running_sum(y * y) / sqq
    lo, hi = bits(x[rows, pos]), bits(x[rows, pos] * F(4.0))
    target = bucket(quotient(lo)) + 1
    assert (bucket(quotient(hi)) >= target).all()
    u = bisect_line(quotient, lo, hi, target)
    a, bb = x.copy(), x.copy()
    a[rows, pos], bb[rows, pos] = from_bits(u), from_bits(u + 1)
    lines = pick_differing(T, a, bb, ratio_differs(T, r, c, b, nrec, ix))
    xr = np.zeros((nrec, 2, 576), np.float32)
    place(T, xr, r, c, b, lines)
    for k in range(nrec):
        isf2_record(R, "ratio_edge", "every quotient on a boundary", xr[k], ix[k], rng, G=rng.integers(100, 220, 2), clamp=np.zeros((2, 22), int))


def build_ratio_worst_case(R, rng):
    """worst_lines in every band, all of whose lines quantise to 1 (sqq = n, exact in either order) or to 2 and 1"""
    T = R.T
    for k in range(4):
        xr, ix = np.zeros((2, 576), np.float32), np.zeros((2, 576), np.int32)
        for c in range(2):
            for b in range(T.nb):
                n, sl = T.width[b], slice(T.start[b], T.start[b] + T.width[b])
                ix[c, sl] = 1 if (k & 1) == 0 else rng.integers(1, 3, n)
                ix[c, T.start[b]] = 1 + (k & 1)
                sqq = running_sum(T.ix43[ix[c, sl]] ** 2)
                xr[c, sl] = worst_lines(T, n, int(rng.integers(-4, 20)), sqq)[:n]
        isf2_record(R, "ratio_worst_case", "one large square, then squares under half its ulp", xr, ix, rng, G=rng.integers(100, 220, 2), clamp=np.zeros((2, 22), int))


BUILDERS = {"walk": build_walk, "layout": build_layout, "bucket_edge": build_bucket_edge, "worst_case": build_worst_case, "double_table": build_double_table,
            "select": build_select, "ratio_edge": build_ratio_edge, "ratio_worst_case": build_ratio_worst_case}


@functools.lru_cache(maxsize=None)
def records(mode, sr):
    R = Records(mode, sr)
    for k, lst in enumerate(LISTS[mode]):
        BUILDERS[lst](R, np.random.default_rng([sr, MODES.index(mode), k]))
    return R.freeze()


@functools.lru_cache(maxsize=None)
def reference(mode, sr):
    """(the oracle's out [n][184], the restatement's dict, the restatement's with strict sums forced) of records(mode, sr): computed once"""
    R = records(mode, sr)
    return expected(R), restate(R), restate(R, forced=True)
