"""K4 (k_spec / k_spec_direct: hybrid MDCT, alias reduction, the psy models and the L/R-vs-M/S metric before hysteresis) on
constructed subband granules: the launches of tests/test_gpu_spec.py (handed to the kernels by hx_debug_spec), what the oracle
makes of them (hxo_spec_record), and a float32 restatement of the device's summation order for the certified stereo-metric
sums; tests/test_spec_cases.py asserts on the CPU what the lists reach and holds the oracle's record function to its own
frame path and to the reference.

The kernel is stateless per granule: it reads two subband blocks per channel and a block type.  A launch is a set of streams,
each a chain of blocks B[0 .. NG] per channel and NG block types; granule g reads B[g] and B[g + 1], so neighbours share a
block as they do in a call.  A constructed record is a pair (prev, cur) appended to its class's chain; the granule that then
joins the chain's last block to `prev` is a record too (list "link"), with the next block type of a sequence that meets every
ordered pair of types.  What every granule's outputs must be comes from the oracle alone.

Records that need a spectrum are reached from it in float64: the alias butterflies are rotations and invert exactly, the
MDCT of a subband (18 x 36, probed from the oracle) through its pseudo-inverse.  The oracle's forward transform of the
resulting float32 blocks is the truth; the target is only approached, and every rule is an inequality on what comes out.

The restatement (`restate`) follows msmetric_unit: the lanes' line runs pair after pair, hx_seg_scan's additions
(noise_cases.seg_scan), the interval arithmetic of the certificate.  It serves to select and to count: which bands pass the
certificate, in which of the four mbLogC arguments the value the device would take differs in bucket from the strict sum's,
and - on every band of every record - that no passing certificate has a differing bucket."""
import ctypes as C
import functools

import numpy as np

from hmp3_amd import api
from noise_cases import bits, bucket, from_bits, seg_scan
from oracle import oracle as O

F = np.float32
U24 = F(5.9604644775390625e-08)
RATES = (44100, 48000, 32000, 22050, 24000, 16000)
SAMPLE_MAX = api.SPEC_SAMPLE_MAX
NG = 32                 # granule positions per stream of the main launch
FILL = 0x7FC5A5A5       # the outputs' fill pattern (a NaN no kernel produces)
LISTS = ("link", "transform", "psy", "metric_kinds", "clamps", "bucket_edge", "worst_case", "thresholds")
ARGS = ("el+er", "max(el,er)", "es+ed", "max(es,ed)")

KINDS = {       # name: control beside the sample rate
    "js": dict(),
    "lr": dict(bitrate=64, mode=0),
    "mono": dict(mode=3),
    "a1": dict(bitrate=64, nsbstereo=8),
    "f4k": dict(freq_limit=4000),
    "nsb12": dict(nsb_limit=12),
    "hf": dict(vbr_mnr=100, hf_flag=3, freq_limit=22000),
    "dual": dict(bitrate=32, mode=2),
}


def kinds(sr):
    """the class kinds of a rate: every kind a batch accepts (both MPEG generations over the rates, both allocators, mono)
    and controls that give three and more nsb values per generation"""
    return [k for k in KINDS if k != "dual" or sr < 32000]


class Cls:
    """one class: its controls, an oracle encoder, and the host tables the builders and the restatement read"""

    def __init__(self, sr, kind):
        self.sr, self.kind = sr, kind
        self.kw = dict(KINDS[kind], samprate=sr)
        self.ec = api.default_control(**self.kw)
        self.oec = O.default_control(**self.kw)
        self.enc = O.OracleEncoder(self.oec)
        assert self.enc.ok(), self.kw

        def tab(name, dtype, count):
            a = np.zeros(count, dtype)
            n = api.lib().hx_debug_host_table(C.byref(self.ec), name.encode(), a.ctypes.data, a.nbytes)
            assert n == a.nbytes, (name, self.kw, api.last_error())
            return a
        sc = tab("scalars", np.int32, 16)
        self.nsb, self.ms_flag = int(sc[1]), int(sc[6])
        self.alloc1, self.nchan = int(tab("alloc1", np.int32, 1)[0]), int(tab("nchan", np.int32, 1)[0])
        self.start, self.width = tab("startBand_l", np.int32, 24).astype(int), tab("nBand_l", np.int32, 22).astype(int)
        self.nsf0 = int(tab("nsf", np.int32, 2)[0])
        self.W = int(tab("run_w", np.int32, 1)[0])
        run, self.last = tab("lane_run", np.uint16, 64).astype(int), tab("band_last_lane", np.uint8, 24).astype(int)[:22]
        self.mblog_tab = tab("mblog", np.int32, 256).astype(np.int64)
        self.npart = int(tab("psy_npart", np.int32, 1)[0])
        nsum = tab("psy_nsum", np.int32, 64).astype(int)
        self.pstart = np.concatenate(([0], np.cumsum(nsum)))[:64]
        self.pnsum = nsum
        self.csa = tab("csa", np.float32, 16).reshape(2, 8).astype(np.float64)
        l = O.lib()
        l.hxo_params_of.restype, l.hxo_params_of.argtypes = C.c_void_p, [C.c_void_p]
        l.hxo_band_tables.argtypes = [C.c_void_p] * 3
        tl, ts = np.zeros(46, np.int32), np.zeros(28, np.int32)
        l.hxo_band_tables(l.hxo_params_of(self.enc.h), tl.ctypes.data, ts.ctypes.data)
        assert np.array_equal(tl[:22], self.width) and np.array_equal(tl[22:], self.start)
        self.width_s, self.start_s, self.nsfs = ts[:13].astype(int), ts[13:27].astype(int), int(ts[27])
        # the lanes of the metric's sums (msmetric_unit): first line, lines, lanes back to the band's first lane
        self.l_start, self.l_cnt, self.l_d = (run & 511) * 2, ((run >> 9) & 7) * 2, run >> 12
        k = np.arange(10)
        self.l_idx = np.minimum(self.l_start[:, None] + k[None, :], 575)
        self.l_valid = ((k & ~1)[None, :] < self.l_cnt[:, None]) & (k[None, :] < self.W)
        self.maxw = int(self.width[:self.nsf0].max())
        j = np.arange(self.maxw)
        self.b_idx = np.minimum(self.start[:22, None] + j[None, :], 575)
        self.b_valid = j[None, :] < self.width[:, None]
        self.du = (self.width + 1 + self.W + 16).astype(np.float32) * U24       # hx_cert_delta(sb_n + 1, W)
        self.metric_long = bool(self.ms_flag and not self.alloc1)

    def mblog(self, x):
        u = bits(x)
        return self.mblog_tab[(u >> 15) & 255] + 301 * (u >> 23)

    def oracle(self, prev, cur, bt):
        return O.spec_records(self.enc, prev, cur, bt)


@functools.lru_cache(maxsize=None)
def cls(sr, kind):
    return Cls(sr, kind)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of msmetric_unit's long path: xr [M][2][576] (the oracle's spectrum) -> per band what the device does
# ---------------------------------------------------------------------------------------------------------------------

def _pairs(t):
    """sa += (a0 + a1), pair after pair, from 0"""
    acc = np.zeros(t.shape[:-1], np.float32)
    for k in range(0, 10, 2):
        acc = acc + (t[..., k] + t[..., k + 1])
    return acc


def _strict(T, t, first):
    """a band's terms in line order, added to `first` -> [M][22]"""
    tt = np.where(T.b_valid, t[..., T.b_idx], F(0.0))
    lead = np.full(tt.shape[:-1] + (1,), first, np.float32)
    return np.cumsum(np.concatenate([lead, tt], axis=-1), axis=-1, dtype=np.float32)[..., -1]


def restate(T, xr, mutant=None):
    """-> dict over [M][22] (bands from nsf0 on: nothing): ok (the certificate passes), lo [..][4] the values the device would
    take (the intervals' lower ends), lane [..][4] the lane-order values, strict [..][4] the strict sums' values, differs
    [..][4] (bucket of the lane-order value != bucket of the strict one), differs_lo [..][4] (the same of the lower end),
    metric [M] from the strict sums, metric_dev [M] as the device forms it (certified bands from the lower ends).  mutant: one
    of MUTANTS, restated here to tell on the CPU which records show it"""
    l, r = xr[:, 0], xr[:, 1]
    band = np.arange(22) < T.nsf0
    with np.errstate(all="ignore"):
        a, b, c = l * l, r * r, l * r
        el, er, t = _strict(T, a, F(100.0)), _strict(T, b, F(100.0)), _strict(T, c, F(0.0))
        p1 = el + er
        t2 = t + t
        es, ed = p1 + t2, p1 - t2
        strict = np.stack([p1, np.maximum(el, er), es + ed, np.maximum(es, ed)], -1)
        valid = T.l_valid if mutant != "mask" else (np.arange(10)[None, :] < T.W) & np.ones((64, 1), bool)
        lane = lambda v: np.where(valid, v[..., T.l_idx], F(0.0))
        scan = (lambda v, d: seg_scan(v, d)) if mutant != "cross_row" else _scan_no_cross
        tot = lambda v: scan(_pairs(lane(v)), T.l_d)[..., T.last]
        SA, SB, SC, SM = tot(a), tot(b), tot(c), tot(np.abs(c))
        du = T.du if mutant != "n_half" else ((T.width + 1) // 2 + T.W + 16).astype(np.float32) * U24
        tel, ter = F(100.0) + SA, F(100.0) + SB
        e1, e2, e3 = tel * du, ter * du, (np.abs(SC) if mutant == "e3_sc" else SM) * du
        el_lo, el_hi = np.maximum(tel - e1, F(100.0)), tel + e1
        er_lo, er_hi = np.maximum(ter - e2, F(100.0)), ter + e2
        t_lo, t_hi = SC - e3, SC + e3
        tl2, th2 = t_lo + t_lo, t_hi + t_hi
        p1_lo, p1_hi = el_lo + er_lo, el_hi + er_hi
        p2_lo, p2_hi = np.maximum(el_lo, er_lo), np.maximum(el_hi, er_hi)
        es_lo, es_hi, ed_lo, ed_hi = p1_lo + tl2, p1_hi + th2, p1_lo - th2, p1_hi - tl2
        p3_lo, p3_hi = es_lo + ed_lo, es_hi + ed_hi
        p4_lo = np.maximum(es_lo, ed_lo) if mutant == "no_floor" else np.maximum(np.maximum(es_lo, ed_lo), p1_lo)
        p4_hi = np.maximum(es_hi, ed_hi)
        lo, hi = np.stack([p1_lo, p2_lo, p3_lo, p4_lo], -1), np.stack([p1_hi, p2_hi, p3_hi, p4_hi], -1)
        ok = (bucket(lo) == bucket(hi)).all(-1) & (p4_lo > 0)
        if mutant != "no_floor":
            ok &= p3_lo > 0
        if mutant == "ok_true":
            ok = np.ones_like(ok)
        ok &= band
        tt2 = SC + SC
        les, led = (tel + ter) + tt2, (tel + ter) - tt2
        lanev = np.stack([tel + ter, np.maximum(tel, ter), les + led, np.maximum(les, led)], -1)

        def value(v):       # v [..][4] -> the band's term of the metric
            mb = T.mblog(v)
            mblr, mbsd = mb[..., 0] - mb[..., 1], mb[..., 2] - mb[..., 3]
            psd = np.maximum(75 - np.abs(mblr - 120), 0)
            mbsd = np.minimum(mbsd, (mbsd >> 1) + 120) + psd
            return np.where(band, T.width * (mblr - mbsd), 0), mblr, mb[..., 2] - mb[..., 3]
        vs, mblr, mbsd = value(strict)
        vd, _, _ = value(np.where(ok[..., None], lo, strict))
    differs = (bucket(lanev) != bucket(strict)) & band[:, None]
    differs_lo = (bucket(lo) != bucket(strict)) & band[:, None]
    return dict(ok=ok, lo=lo, lane=lanev, strict=strict, differs=differs, differs_lo=differs_lo, metric=vs.sum(-1), metric_dev=vd.sum(-1),
                mblr=mblr, mbsd=mbsd, SC=SC, SM=SM, t=t, band=band)


def _scan_no_cross(v, d):
    """hx_seg_scan without its cross-row step (a mutant)"""
    lane = np.arange(64)
    for sh in (1, 2, 4, 8):
        t = np.zeros_like(v)
        okl = (lane & 15) >= sh
        t[..., okl] = v[..., lane[okl] - sh]
        v = v + np.where(d >= sh, t, F(0.0))
    return v


MUTANTS = ("ok_true", "e3_sc", "n_half", "cross_row", "mask", "no_floor")


def one_band_d(xr, k, m):
    """d in {0, 1, 3} of the band of m lines from line k of one granule's spectrum xr [2][576]"""
    a, b = xr[0, k:k + m] * xr[0, k:k + m], xr[1, k:k + m] * xr[1, k:k + m]
    s0 = float(np.cumsum(a + b, dtype=np.float32)[-1])
    s1 = float(np.cumsum(np.abs(a - b), dtype=np.float32)[-1])
    return int(s1 > 0.80 * s0) + 2 * int(s1 > 0.95 * s0)


def band_d(T, xr, short):
    """the short metric's (short) or the first-generation classes' per-band d in {0, 1, 3}: [M][3][nsfs] or [M][nsf0], and
    the metric they add up to"""
    with np.errstate(all="ignore"):
        a, b = xr[:, 0] * xr[:, 0], xr[:, 1] * xr[:, 1]
        s, df = a + b, np.abs(a - b)
        if short:
            n, w0 = T.nsfs, [(192 * w + T.start_s[i], T.width_s[i]) for w in range(3) for i in range(T.nsfs)]
        else:
            n, w0 = T.nsf0, [(T.start[i], T.width[i]) for i in range(T.nsf0)]
        d = np.zeros((xr.shape[0], len(w0)), int)
        for j, (k, m) in enumerate(w0):
            s0 = np.cumsum(s[:, k:k + m], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
            s1 = np.cumsum(df[:, k:k + m], axis=1, dtype=np.float32)[:, -1].astype(np.float64)
            d[:, j] = (s1 > 0.80 * s0) + 2 * (s1 > 0.95 * s0)
    if short:
        return d.reshape(-1, 3, n), (n - d.sum(1)) * 1024
    return d, n - 3 * d.sum(1)


# ---------------------------------------------------------------------------------------------------------------------
# from a spectrum to subband blocks
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mdct_pinv(bt):
    """(M [18][36], its pseudo-inverse [36][18]) of one even subband's windowed MDCT at block type bt, probed from the oracle:
    inputs prev[0 .. 17], cur[0 .. 17] -> the subband's 18 values before the alias butterflies (short: [6 w + k])"""
    T = cls(44100, "js")
    prev, cur = np.zeros((36, 2, 576), np.float32), np.zeros((36, 2, 576), np.float32)
    for j in range(18):
        prev[j, 0, 4 * 18 + j] = 1.0        # subband 4: even, away from the edges
        cur[18 + j, 0, 4 * 18 + j] = 1.0
    xr = T.oracle(prev, cur, [bt] * 36)["xr"][:, 0].astype(np.float64)
    if bt == 2:
        y = np.stack([xr[:, 192 * w + 24 + k] for w in range(3) for k in range(6)], 1)
    else:
        y = unalias(T, xr, 32)[:, 72:90]     # (a probe of subband 4 alone: the butterflies only rotate its edges out)
    M = y.T
    return M, np.linalg.pinv(M)


def unalias(T, x, nsb):
    """the alias butterflies of subbands 0 .. nsb - 1 undone, in float64: x [..][576] -> the values before them (every line
    is in one butterfly at most, so all of them at once)"""
    x = np.array(x, np.float64)
    cs, ca = T.csa[0], T.csa[1]
    k, i = np.meshgrid(np.arange(nsb - 1), np.arange(8), indexing="ij")
    up, dn = (18 * k + 17 - i).reshape(-1), (18 * k + 18 + i).reshape(-1)
    c, s = cs[i.reshape(-1)], ca[i.reshape(-1)]
    a, b = x[..., up], x[..., dn]
    x[..., up] = (a * c - b * s) / (c * c + s * s)
    x[..., dn] = (a * s + b * c) / (c * c + s * s)
    x[..., 18 * (nsb - 1) + 17 - np.arange(8)] /= cs
    return x


def synth(T, target, bt):
    """float32 blocks (prev, cur) [..][576] of one channel whose spectrum at block type bt approaches target [..][576] (lines
    from 18 nsb on are out of reach and ignored; the blocks are zero in subbands from nsb on)"""
    target = np.asarray(target, np.float64)
    nsb = T.nsb
    _, P = mdct_pinv(bt)
    if bt == 2:
        y = np.stack([target[..., 192 * w + 6 * np.arange(32)[:, None] + np.arange(6)[None, :]] for w in range(3)], -2)   # [..][32][3][6]
        y = y.reshape(target.shape[:-1] + (32, 18))
    else:
        y = unalias(T, target, nsb).reshape(target.shape[:-1] + (32, 18))
    x = y @ P.T                                                             # [..][32][36]
    x[..., nsb:, :] = 0.0
    sign = np.ones((32, 18))
    sign[1::2, 1::2] = -1.0             # frequency inversion: odd time slots of odd subbands
    prev, cur = x[..., :18] * sign, x[..., 18:] * sign
    shape = target.shape[:-1] + (576,)
    return prev.reshape(shape).astype(np.float32), cur.reshape(shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------------------------

BT_CYCLE = (0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 0, 3, 1, 3, 2, 1)         # closed: every ordered pair of types follows one another


class Chain:
    """one class's blocks and granules in construction order"""

    def __init__(self):
        self.blocks, self.bt, self.label = [], [], []     # blocks [n + 1] of [2][576]; per granule its type and (list, rule)


class Launch:
    """what one hx_debug_spec call gets"""

    def __init__(self, classes, cls_of, sb, bt, labels, nfr=None):
        self.classes, self.cls_of = classes, np.asarray(cls_of, np.int32)
        self.sb, self.bt, self.labels, self.nfr = np.ascontiguousarray(sb, np.float32), np.ascontiguousarray(bt, np.uint8), labels, nfr
        self.S, self.NG = self.bt.shape
        assert self.sb.shape == (self.S, 2, self.NG + 1, 576)

    def counts(self):
        return [self.NG // 2] * self.S if self.nfr is None else list(self.nfr)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        """the oracle's outputs of every granule a wave runs: dict of [S][NG] arrays, and `live` [S][NG]"""
        S, n = self.S, self.NG
        out = dict(xr=np.zeros((S, n, 2, 576), np.float32), etab=np.zeros((S, n, 2, 64), np.float32), thr=np.zeros((S, n, 2, 64), np.float32),
                   msbase=np.zeros((S, n), np.int32), live=np.zeros((S, n), bool))
        for s in range(S):
            m = 2 * self.counts()[s]
            if m == 0:
                continue
            T = self.classes[self.cls_of[s]]
            blk = self.sb[s].transpose(1, 0, 2)       # [NG + 1][2][576]
            o = T.oracle(blk[:m], blk[1:m + 1], self.bt[s, :m])
            out["xr"][s, :m], out["etab"][s, :m], out["thr"][s, :m], out["msbase"][s, :m] = o["xr"], o["etab"], o["thr"], o["metric"]
            out["live"][s, :m] = True
        return out

    def filled(self):
        """the output arrays as the caller fills them: FILL everywhere"""
        S, n = self.S, self.NG
        f = lambda *shape: np.full(shape, FILL, np.uint32).view(np.float32)
        return f(S, n, 2, 576), f(S, n, 2, 64), f(S, n, 2, 64), np.full((S, n), FILL, np.uint32).view(np.int32)

    def run(self, direct, device=0, sb=None, **change):
        """hx_debug_spec on the launch -> (rc, xr, etab, thr, msbase)"""
        xr, etab, thr, ms = self.filled()
        a = dict(ecs=[T.ec for T in self.classes], cls=self.cls_of, NG=self.NG, nfr=self.nfr, direct=direct, sb=self.sb if sb is None else sb,
                 bt=self.bt, xr=xr, etab=etab, thr=thr, msbase=ms, device=device)
        a.update(change)
        return api.debug_spec(**a)

    def first_difference(self, got):
        """None, or what names the first granule and field where the kernel's outputs are not the oracle's / the fill pattern"""
        want = self.expected()
        _, xr, etab, thr, ms = got
        fill = np.uint32(FILL)
        for s in range(self.S):
            T = self.classes[self.cls_of[s]]
            nch = T.nchan
            for g in range(self.NG):
                where = dict(stream=s, granule=g, cls=T.kind, rate=T.sr, list=self.labels[s][g][0], rule=self.labels[s][g][1], bt=int(self.bt[s, g]))
                fields = [("xr", xr[s, g], want["xr"][s, g]), ("etab", etab[s, g], want["etab"][s, g]), ("thr", thr[s, g], want["thr"][s, g])]
                if not want["live"][s, g]:
                    for name, a, _ in fields + [("msbase", ms[s, g:g + 1], None)]:
                        bad = np.flatnonzero(a.reshape(-1).view(np.uint32) != fill)
                        if bad.size:
                            return dict(where, field=name, index=int(bad[0]), what="a granule past the stream's count was written")
                    continue
                for name, a, w in fields:
                    ga, wa = a[:nch].reshape(-1).view(np.uint32), w[:nch].reshape(-1).view(np.uint32)
                    bad = np.flatnonzero(ga != wa)
                    if bad.size:
                        i = int(bad[0])
                        return dict(where, field=name, index=i, got=hex(int(ga[i])), want=hex(int(wa[i])))
                if T.ms_flag and int(ms[s, g]) != int(want["msbase"][s, g]):
                    return dict(where, field="msbase", index=0, got=int(ms[s, g]), want=int(want["msbase"][s, g]))
        return None


class Builder:
    def __init__(self, sr):
        self.sr = sr
        self.kinds = kinds(sr)
        self.classes = [cls(sr, k) for k in self.kinds]
        self.chains = {k: Chain() for k in self.kinds}

    def add(self, lst, rule, kind, prev, cur, bt):
        """one record: blocks prev, cur [2][576] at block type bt"""
        ch = self.chains[kind]
        alloc1 = cls(self.sr, kind).alloc1       # (the first-generation allocator codes long blocks only: type 0 throughout)
        if alloc1 and bt != 0:
            return
        prev, cur = np.asarray(prev, np.float32), np.asarray(cur, np.float32)
        assert prev.shape == cur.shape == (2, 576) and np.isfinite(prev).all() and np.isfinite(cur).all()
        assert max(np.abs(prev).max(), np.abs(cur).max()) <= SAMPLE_MAX, (lst, rule)
        if ch.blocks:
            ch.bt.append(0 if alloc1 else BT_CYCLE[(len(ch.bt) // 2) % len(BT_CYCLE)])
            ch.label.append(("link", "the granule between two records"))
        ch.blocks += [prev, cur]
        ch.bt.append(int(bt))
        ch.label.append((lst, rule))

    def launch(self):
        cls_of, sb, bts, labels, nfr = [], [], [], [], []
        for ci, k in enumerate(self.kinds):
            ch = self.chains[k]
            n = len(ch.bt)
            for g0 in range(0, n, NG):
                m = min(NG, n - g0)
                blk = np.zeros((NG + 1, 2, 576), np.float32)
                blk[:m + 1] = np.stack(ch.blocks[g0:g0 + m + 1])
                bt = np.zeros(NG, np.uint8)
                bt[:m] = ch.bt[g0:g0 + m]
                lab = ch.label[g0:g0 + m] + [("pad", "behind the chain's end")] * (NG - m)
                cls_of.append(ci); sb.append(blk.transpose(1, 0, 2)); bts.append(bt); labels.append(lab)
                nfr.append((m + 1) // 2)        # (an odd end: the last granule reads a zero block, which is a record as good as any)
        return Launch(self.classes, cls_of, np.stack(sb), np.stack(bts), labels, np.array(nfr, np.int32))


def loud(rng, shape, lo=20.0, hi=3000.0):
    """a spectrum with a random level per group of 6 lines"""
    n = shape[-1]
    lev = np.exp(rng.uniform(np.log(lo), np.log(hi), shape[:-1] + ((n + 5) // 6,)))
    return rng.standard_normal(shape) * np.repeat(lev, 6, axis=-1)[..., :n]


def build_transform(B, rng):
    for k in B.kinds:
        T = cls(B.sr, k)
        scales = (1.0e-41, 1.0e-12, 3.0e4, SAMPLE_MAX)
        for bt in range(4):
            for sc in scales:
                x = rng.uniform(-1.0, 1.0, (2, 2, 576))
                if sc == SAMPLE_MAX:
                    x.reshape(-1)[rng.integers(0, x.size, 64)] = rng.choice([-1.0, 1.0], 64)
                x = (x * sc).astype(np.float32)
                B.add("transform", "dense blocks at scale %g" % sc, k, x[0], x[1], bt)
        for j in range(len(BT_CYCLE)):      # (with the links in between: every ordered pair of types on neighbouring granules)
            x = (rng.standard_normal((2, 2, 576)) * 1000.0).astype(np.float32)
            B.add("transform", "types in sequence", k, x[0], x[1], BT_CYCLE[j])
        z = np.zeros((2, 576), np.float32)
        for bt in (0, 2):
            x = (rng.standard_normal((2, 2, 576)) * 1000.0).astype(np.float32)
            B.add("transform", "zero blocks", k, z, z, bt)
            B.add("transform", "previous block zero", k, z, x[1], bt)
            for c in range(2):
                y = x.copy()
                y[:, c] = 0
                B.add("transform", "channel %d zero" % c, k, y[0], y[1], bt)
            if T.nsb < 32:
                y = x.copy()
                y.reshape(2, 2, 32, 18)[:, :, :T.nsb] = 0
                B.add("transform", "energy only in subbands from nsb on", k, y[0], y[1], bt)
                y = x.copy()
                y.reshape(2, 2, 32, 18)[:, :, :T.nsb - 1] = 0
                B.add("transform", "energy only in subbands from nsb - 1 on", k, y[0], y[1], bt)


def add_spectrum(B, lst, rule, kind, target, bt=0):
    """a record whose spectrum approaches target [2][576]"""
    T = cls(B.sr, kind)
    prev, cur = synth(T, target, bt)
    B.add(lst, rule, kind, prev, cur, bt)
    return prev, cur


def build_psy(B, rng):
    for k in B.kinds:
        T = cls(B.sr, k)
        n_e = int(np.count_nonzero(T.pnsum))
        parts = sorted({0, 1, T.npart // 2, T.npart - 2, T.npart - 1, min(n_e - 1, ((T.npart + 1) & ~1) - 1), n_e - 1})
        for j in parts:
            y = np.zeros((2, 576))
            sl = slice(T.pstart[j], T.pstart[j] + T.pnsum[j])
            y[:, sl] = rng.standard_normal((2, T.pnsum[j])) * 2000.0
            add_spectrum(B, "psy", "long partition %d alone" % j, k, y)
        z = np.zeros((2, 576), np.float32)
        B.add("psy", "silence", k, z, z, 0)
        B.add("psy", "silence", k, z, z, 2)
        for bt in (0, 2):
            x = (rng.choice([-1.0, 1.0], (2, 2, 576)) * SAMPLE_MAX).astype(np.float32)
            B.add("psy", "the bound's magnitude", k, x[0], x[1], bt)
        for w in range(3):
            y = np.zeros((2, 576))
            y[:, 192 * w:192 * w + 6 * T.nsb] = loud(rng, (2, 6 * T.nsb))
            add_spectrum(B, "psy", "short window %d alone" % w, k, y, 2)


def rot(l):
    """a spectrum of the same line energies pairwise orthogonal to l: (a, b) -> (b, -a)"""
    r = np.empty_like(l)
    r[..., 0::2], r[..., 1::2] = l[..., 1::2], -l[..., 0::2]
    return r


def cancel(T, l, r, trim, rounds=5):
    """blocks of the spectrum (l, r) with every band's strict sum of l r brought to zero through the right channel's trim line,
    judged by the oracle's spectrum"""
    r = r.copy()
    best = None
    for it in range(rounds + 1):
        pl, cl = synth(T, l, 0)
        pr, cr = synth(T, r, 0)
        p, c = np.stack([pl, pr]), np.stack([cl, cr])
        R = restate(T, T.oracle(p[None], c[None], [0])["xr"])
        t = R["t"][0, :T.nsf0].astype(np.float64)
        worst = float((np.abs(t) / R["SM"][0, :T.nsf0]).max())
        if best is None or worst < best[0]:
            best = (worst, p, c)
        r[trim] -= t / l[trim]
    return best[1], best[2]


def metric_kinds_of(B):
    return [k for k in B.kinds if cls(B.sr, k).metric_long]


def build_metric_kinds(B, rng):
    for k in metric_kinds_of(B):
        T = cls(B.sr, k)
        n = 18 * T.nsb
        for rep in range(2):
            l = np.zeros(576)
            l[:n] = loud(rng, (n,))
            r = np.zeros(576)
            r[:n] = loud(rng, (n,))
            pl, cl = synth(T, l, 0)
            pr, cr = synth(T, r, 0)
            z = np.zeros(576, np.float32)
            B.add("metric_kinds", "identical channels", k, np.stack([pl, pl]), np.stack([cl, cl]), 0)
            B.add("metric_kinds", "antiphase channels", k, np.stack([pl, -pl]), np.stack([cl, -cl]), 0)
            B.add("metric_kinds", "right channel silent", k, np.stack([pl, z]), np.stack([cl, z]), 0)
            B.add("metric_kinds", "left channel silent", k, np.stack([z, pr]), np.stack([z, cr]), 0)
            B.add("metric_kinds", "uncorrelated channels", k, np.stack([pl, pr]), np.stack([cl, cr]), 0)
            p, c = cancel(T, l, rot(l), T.start[:T.nsf0] + 1)
            B.add("metric_kinds", "t near zero under a large sum of |l r|", k, p, c, 0)
            tiny = rng.standard_normal((2, 576)) * 10.0 ** rng.uniform(-5.0, -3.5)
            add_spectrum(B, "metric_kinds", "every sum the 100 it starts from", k, tiny)
            add_spectrum(B, "metric_kinds", "all bands together", k, np.stack([l, 0.6 * l + 0.8 * rot(l)]))
        for b in range(T.nsf0):
            y = np.zeros((2, 576))
            sl = slice(T.start[b], T.start[b] + T.width[b])
            y[:, sl] = loud(rng, (2, T.width[b]))
            add_spectrum(B, "metric_kinds", "band %d alone" % b, k, y)


def build_clamps(B, rng):
    """per record one ratio er / el (which sets mblr) or one correlation (which sets mbsd) in every band"""
    for k in metric_kinds_of(B):
        T = cls(B.sr, k)
        n = 18 * T.nsb
        for ratio in (0.02, 0.10, 0.125, 0.30, 0.52, 0.58, 1.0):       # 75 - |mblr - 120| > 0 between 0.109 and 0.567
            l = np.zeros(576)
            l[:n] = loud(rng, (n,), 300.0, 3000.0)
            add_spectrum(B, "clamps", "er / el = %g" % ratio, k, np.stack([l, np.sqrt(ratio) * rot(l)]))
        for alpha in (0.0, 0.12, 0.145, 0.16, 0.2, 0.6, 0.999, -0.145, -0.16):      # mbsd > 240 below 2 t / (el + er) = 0.151
            l = np.zeros(576)
            l[:n] = loud(rng, (n,), 300.0, 3000.0)
            add_spectrum(B, "clamps", "correlation %g" % alpha, k, np.stack([l, alpha * l + np.sqrt(1 - alpha * alpha) * rot(l)]))
        # mbsd < 0 needs max(es, ed) above es + ed, so ed = (el + er) - 2 t below zero, which no exact sums give (2 l r <= l l + r r):
        # it comes from the sums' rounding alone.  Channels that differ by 1e-4 in level: 2 t is el + er to 5e-9, the three sums
        # round apart by ulps of 1e12 and more, ed is negative in about half of the bands, and with es on a bucket boundary
        # es + ed falls into the bucket below es
        for sc in (3.0e5, 3.0e7):
            l = np.zeros(576)
            l[:n] = loud(rng, (n,), 0.3 * sc, sc)
            l = np.where(np.abs(l) < 1.0, sc, l)
            for j, (p, c) in zip((0, 1), drive(T, l, l * (1.0 + 1.0e-4), T.start[:T.nsf0] + 1, 3, (0, 1))):
                B.add("clamps", "loud channels 1e-4 apart in level, es on a boundary, %+d ulp" % j, k, p, c, 0)


# ---- bucket_edge and worst_case: a band's strict sum moved onto a bucket boundary through one line of the target ----

def next_boundary(v):
    """the first value of the bucket above v's"""
    return from_bits((bucket(v) + 1) << 15)


def drive(T, l, r, trim, arg, offsets, rounds=3):
    """Move, in every band at once, argument `arg` of the strict sums onto the next bucket boundary above where it starts, by
    Newton steps on the band's trim line (trim [nsf0]: its line; the line's l is changed and its r with it, in their
    ratio), each judged by the oracle's spectrum of the blocks; then one record per entry of offsets, that many ulps of the
    boundary past it.  -> [(prev, cur)] per offset"""
    l, r = l.copy(), r.copy()
    nb = T.nsf0
    rho = r[trim] / l[trim]
    gain = {0: 1 + rho * rho, 1: np.ones(nb), 2: 2 * (1 + rho * rho), 3: 1 + rho * rho + 2 * rho}[arg]

    def blocks(l, r):
        pl, cl = synth(T, l, 0)
        pr, cr = synth(T, r, 0)
        return np.stack([pl, pr]), np.stack([cl, cr])

    def strict(l, r):
        p, c = blocks(l, r)
        return restate(T, T.oracle(p[None], c[None], [0])["xr"])["strict"][0, :nb, arg].astype(np.float64)
    v = strict(l, r)
    goal = next_boundary(v.astype(np.float32)).astype(np.float64)
    ulp = goal * 2.0 ** -23

    def step(l, r, want):
        m2 = np.maximum(l[trim] ** 2 + (want - strict(l, r)) / gain, 1e-30)
        l, r = l.copy(), r.copy()
        l[trim] = np.sign(l[trim]) * np.sqrt(m2)
        r[trim] = rho * l[trim]
        return l, r
    for _ in range(rounds):
        l, r = step(l, r, goal)
    out = []
    for j in offsets:
        lj, rj = step(l, r, goal + j * ulp)
        out.append(blocks(lj, rj))
    return out


def edge_target(T, rng, family):
    """a loud spectrum with a trim line per band (5 % of the band's energy, its second line), shaped for the family: 0 el + er,
    1 max(el, er), 3 max(es, ed)"""
    n = 18 * T.nsb
    l = np.zeros(576)
    l[:n] = rng.standard_normal(n) * np.repeat(np.exp(rng.uniform(np.log(50.0), np.log(3000.0), 32)), 18)[:n]
    l = np.where(np.abs(l) < 1e-3, 1.0, l)
    alpha = {0: 0.0, 1: 0.0, 3: 0.5}[family]
    r = (alpha * l + np.sqrt(1 - alpha * alpha) * rot(l)) * (0.7 if family == 1 else 0.9)
    trim = T.start[:T.nsf0] + 1
    return l, r, trim


def worst_target(T, rng, family, kind):
    """cert_sums_check.c's vectors per band: 'first' one large line, then lines whose squares are 0.49 ulp of the band's sum;
    'last' the same with the large line last; 'equal' near-equal lines.  The band's sum lies in the first bucket of its
    binade, where an ulp is largest against the value: the strict sum drops every small term, the lanes add them up first
    and keep them, and the two are (n - 2) 2^-24 apart in relative terms - which hx_cert_delta's n + W + 17 covers and half
    of n does not, in the widest bands.  The trim line (second of the band) carries 3 % of the energy.  The right channel has
    the left one's magnitudes (family 1: 0.7 of them, so that mblr lies above 120, where a step of it is not taken back by psd), with the left one's signs in family 3 so that the products add up
    the way the squares do"""
    nb = T.nsf0
    l, r = np.zeros(576), np.zeros(576)
    for b in range(nb):
        s, n = T.start[b], T.width[b]
        v = 2.0 ** rng.integers(14, 34) * (1.0 + 2.0 ** -9)        # the band's el: the middle of its binade's first bucket
        if kind == "equal":
            x = np.sqrt((v - 100.0) / n) * (1.0 + 1e-3 * rng.standard_normal(n))
        else:
            x = np.full(n, np.sqrt(0.49 * v * 2.0 ** -23))
            x[0 if kind == "first" else n - 1] = np.sqrt(0.97 * (v - 100.0))
        x[1] = np.sqrt(0.03 * (v - 100.0))
        sg = rng.choice([-1.0, 1.0], n)
        l[s:s + n] = x * sg
        r[s:s + n] = x * (sg if family == 3 else rng.choice([-1.0, 1.0], n)) * (0.7 if family == 1 else 1.0)
    return l, r, T.start[:nb] + 1


EDGE_OFFSETS = (-2, -1, 0, 1, 2, 3)
WORST_OFFSETS = (-4, -3, -2, -1, 0, 1)


def build_edges(B, rng):
    k = "js"
    T = cls(B.sr, k)
    for family in (0, 1, 3):
        for rep in range(3):
            l, r, trim = edge_target(T, rng, family)
            for j, (p, c) in zip(EDGE_OFFSETS, drive(T, l, r, trim, family, EDGE_OFFSETS)):
                B.add("bucket_edge", "%s on a boundary, %+d ulp" % (ARGS[family], j), k, p, c, 0)
        for kind in ("first", "last", "equal"):
            l, r, trim = worst_target(T, rng, family, kind)
            for j, (p, c) in zip(WORST_OFFSETS, drive(T, l, r, trim, family, WORST_OFFSETS)):
                B.add("worst_case", "%s, large term %s, %+d ulp" % (ARGS[family], kind, j), k, p, c, 0)
    # max(el, er) alone on a boundary (el + er is 1.49 times it, elsewhere in its binade): a wrong bucket there moves mblr and
    # nothing that takes it back.  Just under the boundary the strict sum has dropped (n - 2) 2^-24 of itself, which an interval
    # of half hx_cert_delta's width no longer covers in the widest bands
    for rep in range(4):
        l, r, trim = worst_target(T, rng, 1, "first")
        for j, (p, c) in zip((-1, -2, -3, -4), drive(T, l, r, trim, 1, (-1, -2, -3, -4))):
            B.add("worst_case", "max(el,er) alone under a boundary, large term first, %+d ulp" % j, k, p, c, 0)


# ---- thresholds: the short metric and the first-generation classes' metric on either side of 0.80 and 0.95 ----

def threshold_bands(T, short):
    """(first line, lines) of every band position: [3 * nsfs] (short: [12 w + i]) or [nsf0]"""
    if short:
        return [(192 * w + T.start_s[i], T.width_s[i]) for w in range(3) for i in range(T.nsfs)]
    return [(T.start[i], T.width[i]) for i in range(T.nsf0)]


def build_thresholds(B, rng):
    for k, short in (("js", True), ("a1", False)):
        T = cls(B.sr, k)
        bt = 2 if short else 0
        bands = threshold_bands(T, short)
        nline = 6 * T.nsb if short else 18 * T.nsb
        bands = [(s, n) for s, n in bands if (s % 192 if short else s) + n <= nline]

        def spectrum(gammas):
            l = np.zeros(576)
            r = np.zeros(576)
            for (s, n), g in zip(bands, gammas):
                l[s:s + n] = rng.standard_normal(n) * 1000.0 + np.sign(rng.standard_normal(n)) * 200.0
                r[s:s + n] = g * l[s:s + n]
            return np.stack([l, r])
        # each of d = 0, 1 and 3 at every band position: r = gamma l gives s1 / s0 = (1 - gamma^2) / (1 + gamma^2)
        for shift in range(3):
            g = [(0.5, 0.25, 0.0)[(j + shift) % 3] for j in range(len(bands))]
            add_spectrum(B, "thresholds", "d = 0, 1 and 3 in turn over the bands", k, spectrum(g), bt)
        # adjacent floats: one sample of the right channel bisected between two records that differ in the band's d
        _, P = mdct_pinv(bt)
        for thr, gamma in ((0.80, 1.0 / 3.0), (0.95, np.sqrt(0.05 / 1.95))):
            base = spectrum([0.5] * len(bands))
            for j, (s, n) in enumerate(bands):
                y = base.copy()
                y[1, s:s + n] = gamma * y[0, s:s + n]
                prev, cur = synth(T, y, bt)
                # the sample with the most weight in the band's first line
                line = s % 192 if short else s
                sb_ = line // 6 if short else line // 18
                row = 6 * (s // 192) + line % 6 if short else line % 18
                for col in np.argsort(-np.abs(P[:, row]))[:8]:       # the samples with the most weight in the band's first line, in turn
                    blk, pos = (prev, cur)[col // 18], 18 * sb_ + col % 18

                    def d_of(u):
                        v = blk[1, pos]
                        blk[1, pos] = from_bits(np.array([u]))[0]
                        xr = T.oracle(prev[None], cur[None], [bt])["xr"][0]
                        blk[1, pos] = v
                        return one_band_d(xr, s, n)
                    x0 = float(blk[1, pos])
                    need = 1 if thr == 0.80 else 3         # d >= need flips at this threshold alone
                    if x0 == 0.0:
                        continue
                    # (the band's right-channel energy is a parabola in the sample: a bracket is two neighbours of a ladder)
                    us = [int(bits(F(x0 * f))[0]) for f in (0.25, 0.5, 0.8, 0.95, 1.0, 1.05, 1.25, 2.0, 4.0)]
                    ds = [d_of(u) >= need for u in us]
                    i = [i for i in range(len(us) - 1) if ds[i] != ds[i + 1]]
                    if i:
                        ua, ub, da = us[i[0]], us[i[0] + 1], ds[i[0]]
                        break
                else:
                    continue
                while ub - ua > 1:
                    um = (ua + ub) >> 1
                    dm = d_of(um) >= need
                    ua, ub = (um, ub) if dm == da else (ua, um)
                for u in (ua, ub):
                    blk[1, pos] = from_bits(np.array([u]))[0]
                    B.add("thresholds", "band position %d on either side of %.2f" % (j, thr), k, prev.copy(), cur.copy(), bt)


@functools.lru_cache(maxsize=None)
def launch(sr):
    """the main launch of a rate: every list, every class"""
    rng = np.random.Generator(np.random.PCG64(0x5BEC + sr))
    B = Builder(sr)
    build_transform(B, rng)
    build_psy(B, rng)
    build_metric_kinds(B, rng)
    build_clamps(B, rng)
    build_edges(B, rng)
    build_thresholds(B, rng)
    return B.launch()


GEOMETRY = ((1, 2), (7, 2), (1, 16), (3, 6), (17, 2), (5, 8))       # (S, NG): 1, 7, 8, 9, 17 and 20 workgroups


@functools.lru_cache(maxsize=None)
def geometry(sr):
    """small launches: the grid remap's branches (workgroup counts that are and are not multiples of 8, and below 8), streams
    of different classes side by side, per-stream counts from 0 to NG / 2"""
    rng = np.random.Generator(np.random.PCG64(0x6E0 + sr))
    classes = [cls(sr, k) for k in kinds(sr)]
    out = []
    for S, ng in GEOMETRY:
        cls_of = [(s * 3 + ng) % len(classes) for s in range(S)]
        sb = (rng.standard_normal((S, 2, ng + 1, 576)) * 1000.0).astype(np.float32)
        bt = rng.integers(0, 4, (S, ng)).astype(np.uint8)
        bt[[s for s in range(S) if classes[cls_of[s]].alloc1]] = 0
        labels = [[("geometry", "%d workgroups" % (S * ng // 2))] * ng for _ in range(S)]
        out.append(Launch(classes, cls_of, sb, bt, labels, None))
        if S > 1:
            nfr = np.array([(s * 5 + 1) % (ng // 2 + 1) for s in range(S)], np.int32)
            nfr[0], nfr[-1] = 0, ng // 2
            out.append(Launch(classes, cls_of, sb, bt, labels, nfr))
    return out


def counted(sr, S=3):
    """the geometry launch of S streams with per-stream counts"""
    return [L for L in geometry(sr) if L.S == S and L.nfr is not None][0]


def refusals(L):
    """(what, the arguments changed, words the message must hold) - one bad field per rule of hx_debug_spec's host check, in
    a launch of three streams with counts [0, n, NG / 2]"""
    assert L.S == 3 and L.nfr[0] == 0 and 0 < L.nfr[1] and L.nfr[2] == L.NG // 2

    def sample(s, c, g, v):
        sb = L.sb.copy()
        sb[s, c, g, 77] = v
        return dict(sb=sb)
    bt = L.bt.copy()
    bt[1, 2] = 4
    yield "a block type of 4", dict(bt=bt), ("stream 1", "granule 2", "bt")
    for v, word in ((L.NG // 2 + 1, "frame count"), (-1, "frame count")):
        nfr = L.nfr.copy()
        nfr[2] = v
        yield "a count of %d" % v, dict(nfr=nfr), ("stream 2", word)
    yield "a NaN", sample(1, 1, 3, np.nan), ("stream 1", "granule 3", "channel 1", "sb", "finite")
    yield "an infinity", sample(2, 0, 0, -np.inf), ("stream 2", "granule 0", "channel 0", "sb", "finite")
    yield "a sample above the bound", sample(2, 0, L.NG, np.nextafter(F(SAMPLE_MAX), F(np.inf))), ("stream 2", "granule %d" % L.NG, "channel 0", "sb", "HX_SPEC_SAMPLE_MAX")
    yield "a sample below minus the bound", sample(1, 0, 2 * int(L.nfr[1]), -2.0 * SAMPLE_MAX), ("stream 1", "granule %d" % (2 * int(L.nfr[1])), "channel 0", "sb", "HX_SPEC_SAMPLE_MAX")


def accepted(L):
    """the same launch with bad values where no wave reads: a stream without frames, blocks and types past a stream's count"""
    sb, bt = L.sb.copy(), L.bt.copy()
    sb[0] = np.nan
    bt[0] = 9
    sb[1, :, 2 * int(L.nfr[1]) + 1:] = np.inf
    bt[1, 2 * int(L.nfr[1]):] = 200
    return dict(sb=sb, bt=bt)


def first_generation_refusal(sr):
    """(launch, words): one stream of the first-generation allocator with a start block at granule 1"""
    T = cls(sr, "a1")
    L = Launch([T], [0], np.zeros((1, 2, 3, 576), np.float32), np.array([[0, 1]], np.uint8), [[("refusal", "a start block")] * 2])
    return L, ("stream 0", "granule 1", "bt", "first-generation")
