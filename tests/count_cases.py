"""The stream walk's quantiser and Huffman counter on constructed granules: the records of tests/test_gpu_count.py (handed to
the walk's own functions by hx_debug_count) and what the oracle makes of them; tests/test_count_cases.py asserts on the CPU
what the records reach and holds the oracle to the reference's own functions on every one of them.

Whole streams reach the rate loop's quantise-and-count with what their signals happen to produce.  Here a record is built
from a rule and a seed, no data file: the band maxima that make each candidate class the maximum of each region, the band
patterns that take each branch of the two region-shrink rules, lines whose candidate tables tie (found with the oracle's
pair lengths), boundaries placed on lanes 63 | 0, magnitudes on either side of every rounding threshold of every gain step
(found by bisection on the bit pattern through the oracle's quantiser), and random granules.  Everything is an integer or a
32-bit pattern; every comparison is ==.

A record set is one control's (its band tables): hdr / ix / ixmax / x34 / gsf as hx_debug_count takes them (include/hmp3_amd.h)
and, per record, the rule that made it and two flags: `slim` (lines past the coded range hold something, which only the
low-footprint line buffer may - its quantiser writes them) and `unfused` (channel 0's last quadruple reads channel 1's first
lines, which the fused quantise-and-count would be writing)."""
import functools
import itertools

import numpy as np

from oracle import oracle as O

RATES = {"mpeg1": (44100, 48000, 32000), "mpeg2": (22050, 24000, 16000)}
# unit -> (family, control keywords beside the sample rate): a control whose streams the unit walks
UNITS = {"k_alloc": ("mpeg1", dict(bitrate=64)), "k_alloc_slim": ("mpeg1", dict(bitrate=64)), "k_alloc_lsf": ("mpeg2", dict(bitrate=64)),
         "k_alloc1": ("mpeg1", dict(bitrate=64, nsbstereo=8)), "k_alloc1_lsf": ("mpeg2", dict(bitrate=64, nsbstereo=8))}
MODES = ("count", "quant_count", "quant_then_count", "short", "short_count")
# the smallest and the largest value of each of the 19 candidate classes (reference cnttab.h: 0, 1, 2, 3, 4-5, 6-7, 8-15, 16,
# 17-18, 19-22, 23-30, 31-46, 47-78, 79-142, 143-270, 271-526, 527-1038, 1039-2062, 2063-8206)
CLASS_LO = [0, 1, 2, 3, 4, 6, 8, 16, 17, 19, 23, 31, 47, 79, 143, 271, 527, 1039, 2063]
CLASS_HI = [0, 1, 2, 3, 5, 7, 15, 16, 18, 22, 30, 46, 78, 142, 270, 526, 1038, 2062, 8206]
EDGES = sorted(set(CLASS_LO + CLASS_HI))
IX_MAX = 8206
REG0 = [1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 7]       # region_table (reference bitalloc.cpp:124-197)
REG1 = [1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 5, 5, 6, 6, 7, 7, 7, 8, 8, 8, 8]
THRESHOLD_TARGETS = list(range(34)) + [8205, 8206]
WINDOW = 4              # floats on either side of a rounding threshold
RANDOM_PER_BT = 400     # random granules per block type and control


def value_class(v):
    return next(c for c in range(19) if v <= CLASS_HI[c])


@functools.lru_cache(maxsize=None)
def candidates(rmax):
    """(tables, tmax) of a region whose largest band maximum is rmax"""
    n, t, tmax = O.C.c_int(), (O.C.c_int * 4)(), O.C.c_int()
    O.lib().hxo_huff_candidates(int(rmax), O.C.byref(n), t, O.C.byref(tmax))
    return tuple(t[:n.value]), tmax.value


@functools.lru_cache(maxsize=None)
def pair_len(t, x, y):
    return O.huff_pair_len(t, x, y)


@functools.lru_cache(maxsize=None)
def quada_len(v):
    return int(O.lib().hxo_quada_len(int(v)))


def region_sums(tables, lines):
    """the coded length of `lines` (pairs) in each of `tables`, as the counters add them up"""
    return [sum(pair_len(t, int(lines[i]), int(lines[i + 1])) for i in range(0, len(lines), 2)) for t in tables]


@functools.lru_cache(maxsize=None)
def tables(sr, use_ref=False):
    """the band tables of a sample rate (they are the same for every control of the rate without -HF) and the oracle's handle"""
    return O.CountTables(O.default_control(samprate=sr, bitrate=64), use_ref=use_ref)


class Records:
    """one control's records of one kind ("long" or "short"); arrays once frozen"""

    def __init__(self, kind):
        self.kind = kind
        self.rules, self.hdr, self.ix, self.ixmax, self.x34, self.gsf, self.slim, self.unfused = [], [], [], [], [], [], [], []

    def add(self, rule, ix, ixmax, bt=0, nchan=2, ncb=(22, 22), opt=0, zero21=0, nsf=(0, 0), nbmax=(0, 0), x34=None, gsf=None, slim=False, unfused=False):
        nb = 22 if self.kind == "long" else 48
        h = np.zeros(16, np.int32)
        h[:10] = [bt, nchan, ncb[0], ncb[1] if nchan == 2 else 0, opt, zero21, nsf[0], nsf[1] if nchan == 2 else 0, nbmax[0], nbmax[1] if nchan == 2 else 0]
        if self.kind == "short":
            h[:] = 0
            h[1], h[4] = nchan, opt
        self.rules.append(rule)
        self.hdr.append(h)
        self.ix.append(np.asarray(ix, np.int32).reshape(2, 576).copy())
        self.ixmax.append(np.asarray(ixmax, np.int32).reshape(2, nb).copy())
        self.x34.append(np.zeros((2, 576), np.float32) if x34 is None else np.asarray(x34, np.float32).reshape(2, 576).copy())
        self.gsf.append(np.zeros((2, nb), np.int32) if gsf is None else np.asarray(gsf, np.int32).reshape(2, nb).copy())
        self.slim.append(slim)
        self.unfused.append(unfused)

    def freeze(self):
        for k in ("hdr", "ix", "ixmax", "x34", "gsf", "slim", "unfused"):
            a = np.stack(getattr(self, k)) if k not in ("slim", "unfused") else np.array(getattr(self, k), bool)
            a.setflags(write=False)
            setattr(self, k, a)
        self.n = len(self.rules)
        return self

    def pick(self, keep):
        """the records at the indices `keep`, as arrays of a call"""
        return {k: np.ascontiguousarray(getattr(self, k)[keep]) for k in ("hdr", "ix", "ixmax", "x34", "gsf")}


def lines_of_maxima(t, rng, maxima, ncb_lines=None, dense=True):
    """lines [576] whose band maxima are `maxima` [22]: each band's maximum once, at a random line of it, the rest random
    below it (dense) or zero.  Lines 572 .. 575 stay zero: a last quadruple that reaches past line 575 is a case of its own"""
    ix = np.zeros(576, np.int64)
    for b in range(22):
        lo, hi = int(t.startBand_l[b]), min(int(t.startBand_l[b + 1]), 572)
        m = int(maxima[b])
        if m <= 0 or hi <= lo:
            continue
        if dense:
            ix[lo:hi] = np.minimum(rng.geometric(min(1.0, 2.0 / (m + 1)), hi - lo) - 1, m)
        ix[rng.integers(lo, hi)] = m
    return ix


# ---------------------------------------------------------------------------------------------------------------------
# count: lines and band maxima as given
# ---------------------------------------------------------------------------------------------------------------------

def _search_tie(cands, m, npairs, want, rng, pad=0):
    """lines of `npairs` pairs, values 0 .. m, whose lengths in the candidate tables - with those of `pad` further pairs of
    zeros - tie the way `want` says, or None"""
    zero = [pad * pair_len(t, 0, 0) for t in cands]
    vals = list(range(min(m, 15) + 1)) + ([m] if m > 15 else [])

    def miss(b):
        """0 where the sums tie as wanted, else how far off they are"""
        if len(b) == 2:
            return abs(b[0] - b[1])
        best = b[0] if b[0] < b[1] else b[1]
        return {"t2": abs(b[2] - best) + max(b[2] - b[3] + 1, 0), "t3": abs(b[3] - best) + max(best - b[2] + 1, 0),
                "both": abs(b[2] - best) + abs(b[3] - best)}[want]

    def sums(f):
        return [a + z for a, z in zip(region_sums(cands, f), zero)]
    if len(vals) ** (2 * npairs) <= 5000:
        for f in itertools.product(vals, repeat=2 * npairs):
            if any(f) and miss(sums(f)) == 0:
                return list(f)
        return None
    # a larger region: from a random fill, one line at a time to the value that brings the sums closest
    for _ in range(6):
        f = [int(v) for v in rng.choice(vals, 2 * npairs)]
        cur = miss(sums(f))
        for _ in range(60 * npairs):
            if cur == 0:
                break
            i = int(rng.integers(0, 2 * npairs))
            trial = []
            for v in vals:
                g = f[:i] + [v] + f[i + 1:]
                trial.append((miss(sums(g)), int(rng.integers(0, 1 << 30)), v))
            m_, _, v = min(trial)
            if m_ <= cur:
                f[i], cur = v, m_
        if cur == 0 and any(f):
            return f
    return None


def _count_long(sr):
    t = tables(sr)
    sb = t.startBand_l
    R = Records("long")
    rng = np.random.default_rng(1000 + sr)
    other = np.zeros((576,), np.int64), np.zeros(22, np.int64)

    def two(rule, ix0, mx0, ix1=None, mx1=None, **kw):
        ix1 = other[0] if ix1 is None else ix1
        mx1 = other[1] if mx1 is None else mx1
        R.add(rule, np.stack([ix0, ix1]), np.stack([mx0, mx1]), **kw)

    for ncb in (21, 22):
        # every edge value of every class as the maximum of every region; the other regions hold 1 .. 3 (region 2: 2 .. 3,
        # so that the big values reach it)
        for bt in (0, 1, 3):
            cb2 = ncb
            cb0 = REG0[cb2] if bt == 0 else 8
            cb1 = min(cb0 + REG1[cb2], cb0 + 8) if bt == 0 else 8
            regions = [(0, cb0), (cb0, cb1), (cb1, cb2)]
            for v in EDGES:
                for r in ((0, 1, 2) if bt == 0 else (0, 2)):
                    mx = np.zeros(22, np.int64)
                    for q, (a, b) in enumerate(regions):
                        mx[a:b] = rng.integers(2 if q == 2 else 1, 4, b - a) if q != r else 0
                    a, b = regions[r]
                    mx[a:b] = rng.integers(0, v + 1, b - a) if v < 16 else np.minimum(rng.geometric(0.02, b - a), v)
                    mx[rng.integers(a, b)] = v
                    if r == 2:
                        mx[b - 1] = max(mx[b - 1], 2 if v >= 2 else mx[b - 1])
                    mx[ncb:] = 0
                    two("class_edge v=%d region=%d bt=%d ncb=%d" % (v, r, bt, ncb), lines_of_maxima(t, rng, mx), mx, bt=bt, ncb=(ncb, ncb))
        # every cb2: the last band with a value above 1
        for cb2 in range(1, ncb + 1):
            for bt in (0, 1, 3):
                mx = np.zeros(22, np.int64)
                mx[:cb2] = rng.integers(0, 8, cb2)
                mx[cb2 - 1] = rng.integers(2, 8)
                mx[cb2:ncb] = rng.integers(0, 2, ncb - cb2)
                two("cb2=%d bt=%d ncb=%d" % (cb2, bt, ncb), lines_of_maxima(t, rng, mx), mx, bt=bt, ncb=(ncb, ncb))
        # the region-shrink rules: for every cb2 the band patterns that take each branch.  hi / lo: a value of a class above /
        # at most the neighbouring region's table range
        for cb2 in range(2, ncb + 1):
            cb0 = REG0[cb2]
            cb1 = min(max(cb0 + REG1[cb2], cb0 + 1), cb0 + 8)
            for where1 in ("off", "top", "bottom", "none"):
                for where0 in ("off", "top", "bottom", "none"):
                    mx = np.zeros(22, np.int64)
                    lo, mid, hi = 1, 3, 6          # region 2 <= lo; region 1's raised bands mid; region 0's raised bands hi
                    mx[:cb2] = lo
                    mx[cb2 - 1] = 2 if cb2 > cb1 else mx[cb2 - 1]
                    if cb2 > cb1 and where1 == "off":
                        mx[cb1:cb2] = mid
                    if where1 == "top":
                        mx[cb1 - 1] = mid
                    elif where1 == "bottom":
                        mx[min(cb0 + 1, cb1 - 1)] = mid
                    elif where1 == "none":
                        mx[cb0] = mid
                    elif where1 == "off":
                        mx[cb0:cb1] = mid
                    new_cb1 = {"off": cb1, "top": cb1, "bottom": min(cb0 + 1, cb1 - 1) + 1, "none": cb0 + 1}[where1]
                    n = max(new_cb1 - 8, 1)
                    if where0 == "top":
                        mx[cb0 - 1] = hi
                    elif where0 == "bottom":
                        mx[min(n + 1, cb0 - 1)] = hi
                    elif where0 == "none":
                        mx[min(n, cb0 - 1)] = hi
                        mx[0] = hi
                    mx[cb2 - 1] = max(mx[cb2 - 1], 2)
                    two("shrink cb2=%d r1=%s r0=%s ncb=%d" % (cb2, where1, where0, ncb), lines_of_maxima(t, rng, mx), mx, ncb=(ncb, ncb))
    # ties between candidate tables, in region 0 (band 0) and region 1 (band 1) of a granule with cb2 = 2
    n0, n1 = int(sb[1]), int(sb[2])
    for c in range(1, 19):
        for m in sorted({CLASS_LO[c], CLASS_HI[c]}):
            cands, _ = candidates(m)
            for want in (("two",) if len(cands) == 2 else ("t2", "t3", "both")):
                for region in (0, 1):
                    npairs = (n0 if region == 0 else n1 - n0) // 2
                    f = _search_tie(cands, m, min(npairs, 2), want, rng, npairs - min(npairs, 2))
                    if f is None:
                        continue
                    ix, mx = np.zeros(576, np.int64), np.zeros(22, np.int64)
                    base = 0 if region == 0 else n0
                    ix[base:base + len(f)] = f
                    mx[region] = m
                    mx[1 - region] = 1
                    ix[n0 if region == 0 else 0] = 1
                    two("tie %s class=%d m=%d region=%d" % (want, c, m, region), ix, mx)
    # the two count1 tables tie: quadruples whose table-A lengths add up to four each
    for quads in ([1], [2], [4], [8], [1, 2, 4, 8], [0, 5], [0, 0, 3, 5]):
        if sum(quada_len(v) for v in quads) != 4 * len(quads):
            continue
        for bt in (0, 1, 3):
            ix, mx = np.zeros(576, np.int64), np.zeros(22, np.int64)
            first = int(sb[2 if bt == 0 else 8])
            ix[0] = 3
            mx[0] = 3
            for k, v in enumerate(quads):
                ix[first + 4 * k:first + 4 * k + 4] = [(v >> 3) & 1, (v >> 2) & 1, (v >> 1) & 1, v & 1]
            for b in range(22):
                if ix[sb[b]:sb[b + 1]].max(initial=0) > 0:
                    mx[b] = max(mx[b], 1)
            two("count1_tie quads=%s bt=%d" % (quads, bt), ix, mx, bt=bt)
    # nothing, and a single 1
    for bt in (0, 1, 3):
        for nchan in (1, 2):
            z, zm = np.zeros(576, np.int64), np.zeros(22, np.int64)
            R.add("zeros bt=%d nchan=%d" % (bt, nchan), np.stack([z, z]), np.stack([zm, zm]), bt=bt, nchan=nchan)
            one, om = z.copy(), zm.copy()
            one[0], om[0] = 1, 1
            R.add("single_one bt=%d nchan=%d" % (bt, nchan), np.stack([one, one if nchan == 2 else z]), np.stack([om, om if nchan == 2 else zm]), bt=bt, nchan=nchan)
    # band maxima above the lines: the last big band holds nothing above 1, the last count1 band nothing at all (an earlier
    # -HF pass leaves such maxima behind)
    for bt in (0, 1, 3):
        for cb2, cb3 in ((5, 9), (10, 10), (12, 22), (21, 22), (22, 22), (9, 21)):
            mx = np.zeros(22, np.int64)
            mx[:cb2] = rng.integers(2, 6, cb2)
            mx[cb2:cb3] = 1
            ix = lines_of_maxima(t, rng, mx)
            ix[sb[cb2 - 1]:sb[cb2]] = np.minimum(ix[sb[cb2 - 1]:sb[cb2]], 1)
            if cb3 > cb2:
                ix[sb[cb3 - 1]:sb[cb3]] = 0
            two("maxima_above_lines cb2=%d cb3=%d bt=%d" % (cb2, cb3, bt), ix, mx, bt=bt)
    # where the big values end: the floor of the first bands, 574, 576, and every 64-pair step (the boundary between the pairs
    # of lanes 63 and 0), each with a value above 1 right below it and count1 values right behind it
    for bt in (0, 1, 3):
        floor = int(sb[2 if bt == 0 else 8])
        for nbig in sorted({floor, 128, 256, 384, 512, 572, 574, 576} | {int(v) for v in sb[3:22] if v % 2 == 0}):
            if nbig < floor:
                continue
            for tail in (0, 1, 2, 5):
                ix = np.zeros(576, np.int64)
                if nbig > floor:
                    ix[:nbig] = np.minimum(rng.geometric(0.4, nbig) - 1, 7)
                    ix[nbig - 2:nbig] = [2, 1] if tail % 2 else [0, 3]
                else:
                    ix[:nbig] = rng.integers(0, 2, nbig)
                end = min(nbig + 4 * tail, 576)
                ix[nbig:end] = rng.integers(0, 2, end - nbig)
                if end > nbig:
                    ix[nbig], ix[end - 1] = 1, 1
                mx = np.array([ix[sb[b]:sb[b + 1]].max(initial=0) for b in range(22)])
                two("nbig=%d tail=%d bt=%d" % (nbig, tail, bt), ix, mx, bt=bt)
    # the region boundaries n0 and n1: values right below and right above each (the lanes' table select flips there)
    for cb2 in range(3, 23):
        mx = np.zeros(22, np.int64)
        mx[:cb2] = rng.integers(2, 16, cb2)
        ix = lines_of_maxima(t, rng, mx)
        cb0 = REG0[cb2]
        cb1 = min(max(cb0 + REG1[cb2], cb0 + 1), cb0 + 8)
        for edge, (a, b) in ((int(sb[cb0]), (cb0 - 1, cb0)), (int(sb[cb1]), (cb1 - 1, cb1))):
            if edge + 2 <= int(sb[cb2]):
                ix[edge - 2:edge] = [mx[a], 1]
                ix[edge:edge + 2] = [1, mx[b]]
        two("region_edges cb2=%d" % cb2, ix, mx)
    # 8206 throughout: the largest sums the packed 16-bit accumulators of the lanes and of the wave see
    for bt in (0, 1, 3):
        for nchan in (1, 2):
            full, fm = np.full(576, IX_MAX, np.int64), np.full(22, IX_MAX, np.int64)
            z, zm = np.zeros(576, np.int64), np.zeros(22, np.int64)
            R.add("all_8206 bt=%d nchan=%d" % (bt, nchan), np.stack([full, full if nchan == 2 else z]), np.stack([fm, fm if nchan == 2 else zm]), bt=bt, nchan=nchan)
    # channels that differ in everything; mono; one channel-0 record beside three channel-1 records
    for bt in (0, 1, 3):
        chans = []
        for k in range(4):
            top = [22, 9, 15, 3][k]
            mx = np.zeros(22, np.int64)
            mx[:top] = np.minimum(rng.geometric([0.05, 0.5, 0.2, 0.01][k], top), IX_MAX)
            chans.append((lines_of_maxima(t, rng, mx), mx))
        for k in (1, 2, 3):
            R.add("beside k=%d bt=%d" % (k, bt), np.stack([chans[0][0], chans[k][0]]), np.stack([chans[0][1], chans[k][1]]), bt=bt, ncb=(22, [21, 22, 9][k - 1]))
        R.add("swapped bt=%d" % bt, np.stack([chans[1][0], chans[0][0]]), np.stack([chans[1][1], chans[0][1]]), bt=bt, ncb=(21, 22))
        R.add("mono bt=%d" % bt, np.stack([chans[0][0], np.zeros(576, np.int64)]), np.stack([chans[0][1], np.zeros(22, np.int64)]), bt=bt, nchan=1)
    # channel 0's last quadruple on lines 574 .. 577: it counts channel 1's lines 0 and 1 (CMp3Enc::ix[2][576] is contiguous)
    for bt in (0, 1, 3):
        for last in (574, 575):
            ix = np.zeros(576, np.int64)
            ix[:570] = np.minimum(rng.geometric(0.4, 570) - 1, 7)
            ix[568:570] = [2, 2]
            ix[last] = 1
            mx = np.array([ix[sb[b]:sb[b + 1]].max(initial=0) for b in range(22)])
            for l0, l1 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                ix1, mx1 = np.zeros(576, np.int64), np.zeros(22, np.int64)
                ix1[0], ix1[1], mx1[0] = l0, l1, max(l0, l1)
                R.add("over_read ch1=%d%d last=%d bt=%d" % (l0, l1, last, bt), np.stack([ix, ix1]), np.stack([mx, mx1]), bt=bt, unfused=True)
    # random granules, geometric magnitudes
    for bt in (0, 1, 3):
        for k in range(RANDOM_PER_BT):
            nchan = 1 if k % 8 == 0 else 2
            ncb = (int(rng.choice([21, 22])), int(rng.choice([21, 22, 13])))
            ch = []
            for c in range(2):
                top = int(rng.integers(0, 23))
                mx = np.zeros(22, np.int64)
                scale = float(rng.choice([0.9, 0.6, 0.3, 0.1, 0.02, 0.002]))
                mx[:top] = np.minimum(rng.geometric(scale, top) - (k % 2), IX_MAX).clip(0)
                ix = lines_of_maxima(t, rng, mx, dense=bool(k % 3))
                ix[sb[ncb[c]]:] = 0             # (behind the counted bands: maxima without lines)
                if k % 5 == 0:
                    mx[:top] += rng.integers(0, 3, top)         # maxima above the lines
                ch.append((ix, mx) if c < nchan else (np.zeros(576, np.int64), np.zeros(22, np.int64)))
            R.add("random k=%d bt=%d" % (k, bt), np.stack([ch[0][0], ch[1][0]]), np.stack([ch[0][1], ch[1][1]]), bt=bt, nchan=nchan,
                  ncb=ncb)
    return R.freeze()


@functools.lru_cache(maxsize=None)
def count_long(sr):
    return _count_long(sr)


# ---------------------------------------------------------------------------------------------------------------------
# the quantisers' rounding thresholds
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def thresholds(sr, rule):
    """uint32 [128][targets]: for every gain step the smallest float pattern x with quantiser(rule, x) >= target, by
    bisection on the bit pattern through the oracle's quantiser (monotone in x; 0 where even the largest finite float stays
    below the target)"""
    t = tables(sr)
    tg = np.array(THRESHOLD_TARGETS, np.int64)
    out = np.zeros((128, len(tg)), np.uint32)
    for g in range(128):
        lo = np.zeros(len(tg), np.int64)                     # q(lo) < target, or lo = 0 and target = 0
        top = np.float32(20000.0 * 2.0 ** (3.0 * (g - 8) / 16.0))         # quantises to some 20000: above every target, below 2^31
        hi = np.full(len(tg), int(top.view(np.uint32)), np.int64)
        reach = t.quant_lines(rule, hi.astype(np.uint32).view(np.float32), g).astype(np.int64) >= tg
        assert reach.all()
        while (hi - lo > 1).any():
            mid = (lo + hi) >> 1
            ge = t.quant_lines(rule, mid.astype(np.uint32).view(np.float32), g).astype(np.int64) >= tg
            hi = np.where(ge, mid, hi)
            lo = np.where(ge, lo, mid)
        out[g] = np.where(reach & (tg > 0), hi, 0)
    out.setflags(write=False)
    return out


def threshold_lines(sr, rule, g):
    """float32 patterns around every threshold of gain step g that keep the quantiser at or below 8206, then zero and subnormals"""
    t = tables(sr)
    th = thresholds(sr, rule)[g].astype(np.int64)
    u = np.concatenate([np.arange(x - WINDOW, x + WINDOW) for x in th if x > 0] + [np.array([0, 1, 2, 0x7FFFFF, 0x400000, 0x800000])])
    u = np.unique(u[(u >= 0) & (u <= int(th.max()) + WINDOW)]).astype(np.uint32)
    q = t.quant_lines(rule, u.view(np.float32), g)
    return u[q <= IX_MAX]


def _quant_long(sr, with_thresholds):
    t = tables(sr)
    sb = t.startBand_l
    R = Records("long")
    rng = np.random.default_rng(2000 + sr)
    igain = lambda g: 2.0 ** (-3.0 * (g - 8) / 16.0)

    def magnitudes(gsf, nl, level):
        """x^(3/4) of lines that quantise to about `level` under the band gains gsf"""
        x = np.zeros(576, np.float32)
        for b in range(22):
            lo, hi = int(sb[b]), min(int(sb[b + 1]), nl)
            if hi > lo:
                x[lo:hi] = (np.minimum(rng.geometric(min(1.0, 1.0 / max(level, 1.0)), hi - lo) - 1, 8000) + rng.random(hi - lo)) / igain(int(gsf[b])) * 0.999
        x[572:] = 0.0           # (a last quadruple past line 575 is a case of its own)
        return x

    if with_thresholds:
        # every gain step, both rounding rules: one channel per gain step, all bands at that step, the threshold floats in line order
        for opt in (0, 1):
            for g0 in range(0, 128, 2):
                x34, gsf = np.zeros((2, 576), np.float32), np.zeros((2, 22), np.int64)
                for c in range(2):
                    u = threshold_lines(sr, opt, g0 + c)
                    nl = int(sb[21])
                    assert u.size <= nl, (u.size, nl)
                    x34[c, :u.size] = u.view(np.float32)
                    gsf[c] = g0 + c
                R.add("thresholds opt=%d gsf=%d,%d" % (opt, g0, g0 + 1), np.zeros((2, 576)), np.zeros((2, 22)), opt=opt, ncb=(21, 22), nsf=(21, 21),
                      nbmax=(int(sb[21]), int(sb[21])), x34=x34, gsf=gsf)
    for k in range(240):
        bt = (0, 1, 3)[k % 3]
        nchan = 1 if k % 7 == 0 else 2
        opt = (0, 1, 3)[(k // 3) % 3]
        zero21 = int(k % 4 == 1 and nchan == 2)
        nsf = [int(rng.choice([21, 21, 22, 13, 6])) for _ in range(2)]
        if zero21:
            nsf[0] = min(nsf[0], 21)        # (the walk clears band 21's maximum where that band was not quantised: M/S under -HF)
        ncb = [max(n, int(rng.choice([21, 22]))) for n in nsf]
        gsf = rng.integers(0, 128, (2, 22))
        level = float(rng.choice([0.3, 1.0, 3.0, 20.0, 400.0]))
        x34 = np.stack([magnitudes(gsf[c], int(sb[nsf[c]]), level) for c in range(2)])
        ix, mx = np.zeros((2, 576), np.int64), np.zeros((2, 22), np.int64)
        slim = False
        for c in range(nchan):
            if opt & 2 and k % 2:           # band 21 as an earlier -HF pass left it, its maximum beside it
                lo = int(sb[21])
                w = min(40, 572 - lo - 4)       # (out of the reach of band 20's last quadruple, and short of line 572)
                ix[c, lo + 4:lo + 4 + w] = rng.integers(0, 3, w) * (rng.random(w) < 0.3)
                mx[c, 21] = max(int(ix[c, lo:].max()), 1)
            elif k % 5 == 2 and nsf[c] < 22:   # band maxima behind the quantised bands are kept
                mx[c, nsf[c]:] = rng.integers(0, 2, 22 - nsf[c])
            if not (opt & 2) and k % 6 == 3 and nsf[c] < 22:    # what the low-footprint line buffer holds before its quantiser writes it: anything
                ix[c, int(sb[nsf[c]]):] = rng.integers(0, IX_MAX + 1, 576 - int(sb[nsf[c]]))
                slim = True
        if zero21:
            mx[0, 21] = max(mx[0, 21], 1)
        R.add("random_quant k=%d bt=%d opt=%d zero21=%d" % (k, bt, opt, zero21), ix, mx, bt=bt, nchan=nchan, ncb=ncb, opt=opt, zero21=zero21, nsf=nsf,
              nbmax=[int(sb[n]) for n in nsf], x34=x34, gsf=gsf, slim=slim)
    # the quantiser's own lines under channel 0's last quadruple: band 21 coded to line 575, channel 1's first lines 0 / 1
    want = np.zeros(576)
    want[:570] = np.minimum(rng.geometric(0.4, 570) - 1, 7)
    want[568:570] = 2
    want[575] = 1
    for l0, l1 in ((0, 1), (1, 1), (1, 0)):
        gsf = np.full((2, 22), 40)
        x34 = np.zeros((2, 576), np.float32)
        x34[0] = (want + 0.2) / igain(40)
        x34[1, :2] = (np.array([l0, l1]) + 0.2) / igain(40)
        R.add("over_read_quant ch1=%d%d" % (l0, l1), np.zeros((2, 576)), np.zeros((2, 22)), opt=1, ncb=(22, 22), nsf=(22, 21), nbmax=(576, int(sb[21])),
              x34=x34, gsf=gsf, unfused=True)
    return R.freeze()


@functools.lru_cache(maxsize=None)
def quant_long(sr):
    """the quantising records of a rate; the threshold records ride with the first rate of each family"""
    return _quant_long(sr, sr in (RATES["mpeg1"][0], RATES["mpeg2"][0]))


# ---------------------------------------------------------------------------------------------------------------------
# short blocks
# ---------------------------------------------------------------------------------------------------------------------

def _short(sr, quant):
    t = tables(sr)
    ss, nsfs = t.startBand_s, t.nsfs
    nl = int(ss[nsfs])
    R = Records("short")
    rng = np.random.default_rng((3000 if quant else 4000) + sr)
    igain = lambda g: 2.0 ** (-3.0 * (g - 8) / 16.0)
    if quant and sr in (RATES["mpeg1"][0], RATES["mpeg2"][0]):
        # every gain step under both rules (opt: the table offsets with the first at -0.30): a window per chunk of threshold floats
        for opt in (0, 1):
            chunks = []
            for g in range(128):
                u = threshold_lines(sr, 2 if opt else 0, g)
                chunks += [(g, u[i:i + nl]) for i in range(0, u.size, nl)]
            for i in range(0, len(chunks), 6):
                x34, gsf = np.zeros((2, 3, 192), np.float32), np.zeros((2, 3, 16), np.int64)
                for k, (g, u) in enumerate(chunks[i:i + 6]):
                    x34[k // 3, k % 3, :u.size] = u.view(np.float32)
                    gsf[k // 3, k % 3] = g
                R.add("short_thresholds opt=%d chunk=%d" % (opt, i // 6), np.zeros((2, 576)), np.zeros((2, 48)), opt=opt, x34=x34, gsf=gsf)
    for k in range(300):
        nchan = 1 if k % 6 == 0 else 2
        opt = k % 2 if quant else 0
        top = int(rng.integers(0, nsfs + 1))
        ix, mx = np.zeros((2, 3, 192), np.int64), np.zeros((2, 3, 16), np.int64)
        x34, gsf = np.zeros((2, 3, 192), np.float32), rng.integers(0, 128, (2, 3, 16))
        scale = float(rng.choice([0.9, 0.5, 0.2, 0.05, 0.004]))
        for c in range(2 if quant else nchan):
            for w in range(3):
                for b in range(top):
                    lo, hi = int(ss[b]), int(ss[b + 1])
                    v = np.minimum(rng.geometric(scale, hi - lo) - 1, 8000 if k % 9 else 7) * (rng.random(hi - lo) < (0.8 if k % 4 else 0.2))
                    ix[c, w, lo:hi] = v
                    mx[c, w, b] = v.max(initial=0) + (1 if k % 5 == 0 else 0)
                    x34[c, w, lo:hi] = (v + rng.random(hi - lo) * 0.9) / igain(int(gsf[c, w, b])) * 0.999
        if quant:
            ix[:], mx[:] = 0, 0
        R.add("short_random k=%d" % k, ix, mx, nchan=nchan, opt=opt, x34=x34 if quant else None, gsf=gsf if quant else None)
    # the class edges as the maximum of the two regions; ties; zeros; 8206 throughout
    if not quant:
        for v in EDGES:
            for region in (0, 1):
                ix, mx = np.zeros((2, 3, 192), np.int64), np.zeros((2, 3, 16), np.int64)
                for c in range(2):
                    band = int(rng.integers(0, 3)) if region == 0 else int(rng.integers(3, nsfs))
                    w = int(rng.integers(0, 3))
                    mx[c, :, :band + 1] = rng.integers(0, min(v, 3) + 1, (3, band + 1))
                    mx[c, w, band] = v
                    if region == 1 and v < 2:
                        mx[c, :, 3:] = np.minimum(mx[c, :, 3:], v)
                    for ww in range(3):
                        for b in range(nsfs):
                            if mx[c, ww, b]:
                                lo, hi = int(ss[b]), int(ss[b + 1])
                                ix[c, ww, lo:hi] = rng.integers(0, mx[c, ww, b] + 1, hi - lo)
                                ix[c, ww, rng.integers(lo, hi)] = mx[c, ww, b]
                R.add("short_class_edge v=%d region=%d" % (v, region), ix, mx)
        z, zm = np.zeros((2, 3, 192), np.int64), np.zeros((2, 3, 16), np.int64)
        R.add("short_zeros", z, zm)
        R.add("short_zeros_mono", z, zm, nchan=1)
        full = z.copy()
        full[:, :, :nl] = IX_MAX
        fm = zm.copy()
        fm[:, :, :nsfs] = IX_MAX
        R.add("short_all_8206", full, fm)
        n0 = int(ss[3])
        for c in (4, 5, 1, 2, 3, 6):
            m = CLASS_HI[c]
            cands, _ = candidates(m)
            for want in (("two",) if len(cands) == 2 else ("t2", "t3", "both")):
                f = _search_tie(cands, m, 3 * n0 // 2, want, rng)      # region 0: the first three bands of the three windows
                if f is None:
                    continue
                ix, mx = z.copy(), zm.copy()
                ix[0, :, :n0] = np.array(f).reshape(3, n0)
                mx[0, :, :3] = m
                R.add("short_tie %s class=%d" % (want, c), ix, mx)
    return R.freeze()


@functools.lru_cache(maxsize=None)
def short_quant(sr):
    return _short(sr, True)


@functools.lru_cache(maxsize=None)
def short_count(sr):
    return _short(sr, False)


# ---------------------------------------------------------------------------------------------------------------------
# what a mode runs on a unit, and what the oracle makes of it
# ---------------------------------------------------------------------------------------------------------------------

def records(mode, sr):
    return {"count": count_long, "quant_count": quant_long, "quant_then_count": quant_long, "short": short_quant, "short_count": short_count}[mode](sr)


def runs(mode, unit, R):
    """the indices of R that `mode` runs on `unit`"""
    keep = np.ones(R.n, bool)
    if unit != "k_alloc_slim":
        keep &= ~R.slim
    if mode == "quant_count":
        keep &= ~R.unfused
    return np.flatnonzero(keep)


@functools.lru_cache(maxsize=None)
def expected(mode, sr, slim, use_ref=False):
    """(lines, band maxima, out, sums) of every record of (mode, sr) by the oracle - slim: with the low-footprint line buffer's
    rule for the lines past the coded range - or by the reference's own functions"""
    R = records(mode, sr)
    omode = {"count": "count", "quant_count": "quant", "quant_then_count": "quant", "short": "short", "short_count": "short_count"}[mode]
    ix = R.ix
    if R.slim.any() and (use_ref or not slim):
        # what only the low-footprint line buffer may hold is no input of the reference's functions (lines above their band
        # maxima): there the record is what that buffer's rule makes of it, zeros past the coded range
        ix = R.ix.copy()
        for r in np.flatnonzero(R.slim):
            for c in range(int(R.hdr[r, 1])):
                ix[r, c, int(R.hdr[r, 8 + c]):] = 0
    res = O.count_records(tables(sr, use_ref), omode, R.hdr, ix, R.ixmax, R.x34, R.gsf, clear_past=slim, use_ref=use_ref)
    for a in res:
        a.setflags(write=False)
    return res


FIELDS = ["table0", "table1", "table2", "count1table", "cb0", "cb1", "cb2", "nbig", "nquads", "bits"]


def first_difference(R, keep, got, want, nband, compare_maxima_below=None):
    """None, or a message naming the first record, its rule, the channel and the field where (lines, maxima, out) differ.
    got: the arrays of the records `keep`; want: those of all records"""
    g_ix, g_mx, g_out = got
    w_ix, w_mx, w_out = (np.asarray(a)[keep] for a in want[:3])
    for i, r in enumerate(keep):
        nchan = int(R.hdr[r, 1])
        for ch in range(nchan):
            o, w = g_out[i, 10 * ch:10 * ch + 10], w_out[i, 10 * ch:10 * ch + 10]
            for k, name in enumerate(FIELDS):
                if o[k] != w[k]:
                    return "record %d (%s) channel %d: %s is %d, expected %d" % (r, R.rules[r], ch, name, o[k], w[k])
            a, b = g_ix[i].reshape(2, 576)[ch], w_ix[i].reshape(2, 576)[ch]
            if (a != b).any():
                j = int(np.flatnonzero(a != b)[0])
                return "record %d (%s) channel %d: line %d is %d, expected %d" % (r, R.rules[r], ch, j, a[j], b[j])
            a, b = g_mx[i].reshape(2, nband)[ch], w_mx[i].reshape(2, nband)[ch]
            if compare_maxima_below is not None:
                a, b = a.reshape(3, 16)[:, :compare_maxima_below], b.reshape(3, 16)[:, :compare_maxima_below]
            if (a != b).any():
                j = int(np.flatnonzero((a != b).reshape(-1))[0])
                return "record %d (%s) channel %d: band maximum %d is %d, expected %d" % (r, R.rules[r], ch, j, a.reshape(-1)[j], b.reshape(-1)[j])
        if g_out[i, 20] != w_out[i, 20]:
            return "record %d (%s): the returned sum is %d, expected %d" % (r, R.rules[r], g_out[i, 20], w_out[i, 20])
    return None
