"""The cases of tests/test_gpu_recon_granules.py and tests/test_recon_granule_cases.py: granules constructed for the
decoded-PCM kernels (k_recon_hybrid, k_recon_synth, k_recon_carry; hmp3_amd/csrc/hx_recon.hip), as plain records made from
seeds and rules, the float64 reference of what a decoder makes of them, the bound the kernels are held to, and a float32
restatement of the kernels' own operation order.  Nothing here is taken from an encoder run.

A launch (Launch) is what one hx_debug_recon call gets: S streams x NG granule positions, each stream of a class of CLASSES,
with per (stream, granule, channel) the side information the kernels read, 576 int16 lines in bitstream order, one sign per
line, and per stream the carried state.  A list (case_list(name), name of LIST_NAMES) is a tuple of launches.

The reference is the back half of tests/mp3_decode.py driven from the same records (frame_info), in float64, twice: once as
a decoder computes it, and once as its magnitude pass - every operand, table entry and partial product replaced by its
absolute value, every subtraction by an addition - which is the sum of |terms| that the standard forward error bound of a
sum of products multiplies by gamma_k = k u / (1 - k u), u = 2^-24:

    |got - want| <= gamma_k * magnitude + floor

k is the number of fp32 roundings on the deepest path from the double requantised value to the compared value, counted from
hx_recon.hip (one for each operation that rounds, one for each fp32 table entry or constant the term is multiplied by):

  hybrid tap (K_HYB = 30)
     1   the requantised double to float
     3   M/S: the addition, the product, the constant 0.70710678f
     3   alias butterfly: the product, its cs / ca entry, the addition
    20   IMDCT: the product, its cos36 entry, at most 18 additions of the running sum (a short block: 6, and 3 of acc)
     2   window: the product, its win entry
     1   overlap add (the frequency inversion is exact; a carried tail is an input and has none of the above)
  output (K_OUT = 82): the hybrid tap's 30 and
    34   matrixing: the product, its synth entry, at most 32 additions of the running sum
    18   window: the product, its dwin entry, at most 16 additions (dw0 v + dw1 v, then acc +=, 8 times)

What the double path adds ahead of the first rounding (pow43, pow2q, their product: three roundings at 2^-53, where the
reference has its own) is 2^-27 of one fp32 rounding and is not counted.  floor covers products that underflow (denormals
are kept, so nothing is flushed, and each rounding of a denormal loses at most 2^-150): 256 * 2^-149 for the hybrid tap - 36
products and additions of two transforms, each line behind at most seven roundings - and for the output those through 16 x 32
products with window taps below 2^16: 2^-116.  No factor goes on top.

Held by float bits, not by the bound: a hybrid value whose magnitude is zero is +0 (-0 where the frequency inversion negates
it: odd subband, odd slot); an output whose magnitude is zero is +0; what no kernel writes keeps the caller's bytes; the
state's 15 carried slots are the returned hybrid output's last 15, and the tails are held through the split list.
"""
import functools

import numpy as np

import mp3_decode as D
from hmp3_amd import api

K_HYB, K_OUT = 30, 82
RATES = (44100, 48000, 32000)
U = 2.0 ** -24
FLOOR_HYB, FLOOR_OUT = 256 * 2.0 ** -149, 2.0 ** -116
CLASSES = {     # name: control, channels, rate
    "s44": dict(kw=dict(), nchan=2, rate=44100), "s48": dict(kw=dict(samprate=48000), nchan=2, rate=48000),
    "s32": dict(kw=dict(samprate=32000), nchan=2, rate=32000), "m44": dict(kw=dict(mode=3), nchan=1, rate=44100),
    "m48": dict(kw=dict(mode=3, samprate=48000), nchan=1, rate=48000)}
LIST_NAMES = ("pow43", "exponent_long", "exponent_short", "coded_range", "signs", "ms", "alias", "transforms", "synthesis",
              "counts_and_kinds", "split", "random")
SUCC = {0: (0, 1), 1: (2,), 2: (2, 3), 3: (0, 1)}      # the block types that can follow one
PRED = {0: (0, 3), 1: (0, 3), 2: (1, 2), 3: (2,)}
TRANSITIONS = [(a, b) for a in range(4) for b in SUCC[a]]
SENTINEL = np.float32(-12345.678)
MAX_MAG = 8206
GR_FIELDS = ["part2_3_length", "big_values", "global_gain", "scalefac_compress", "window_switching_flag", "block_type", "mixed_block_flag",
             ("table_select", 3), ("subblock_gain", 3), "region0_count", "region1_count", "preflag", "scalefac_scale", "count1table_select",
             "aux_nquads", "aux_bits", "aux_not_null", ("aux_nreg", 3)]


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the records' layouts (hx_types.h; sizes: hx_debug_host_table "sizeof_recon_records") ----
def host_table(name, dtype, n, **kw):
    import ctypes as C
    a = np.zeros(n, dtype=dtype)
    assert api.lib().hx_debug_host_table(C.byref(api.default_control(**kw)), name.encode(), a.ctypes.data, a.nbytes) == a.nbytes, name
    return a


@functools.lru_cache(maxsize=None)
def layouts():
    """{"seg", "rec": numpy dtypes of HxSegOut and HxFrameDebug, "sgn_words", "state", "tail", "hist"}"""
    v = host_table("sizeof_recon_records", np.int32, 8)
    gr = np.dtype([(f, "<i4") if isinstance(f, str) else (f[0], "<i4", (f[1],)) for f in GR_FIELDS])
    rec = np.dtype([("ms", "<i4"), ("ms_metric", "<i4", (2,)), ("byte_pool", "<i4"), ("MNR_after", "<i4"), ("mask_mb", "<i4", (2, 2, 22)),
                    ("gr", gr, (2, 2)), ("sf", "<i4", (2, 2, 22)), ("scfsi", "<i4", (2,)), ("main_bytes", "<i4")])
    seg = np.dtype({"names": ["head", "sf"], "formats": [("<i4", (6,)), ("<u2", (40,))], "offsets": [0, int(v[7])], "itemsize": int(v[0])})
    assert gr.itemsize == v[6] and rec.itemsize == v[1] and v[3] == v[4] + 2 * v[5] * 32 and v[4] == 1152, v
    return {"seg": seg, "rec": rec, "sgn_words": int(v[2]), "state": int(v[3]), "tail": int(v[4]), "hist": int(v[5])}


@functools.lru_cache(maxsize=None)
def device_tables():
    """the tables hx_recon_tabs builds, as the kernels get them"""
    f = np.float32
    return {"pow43": host_table("pow43", np.float64, 16384), "pow2q": host_table("recon_pow2q", np.float64, 4),
            "cos36": host_table("recon_cos36", f, 36 * 18).reshape(36, 18), "cos12": host_table("recon_cos12", f, 72).reshape(12, 6),
            "win": host_table("recon_win", f, 4 * 36).reshape(4, 36), "cs": host_table("recon_cs", f, 8), "ca": host_table("recon_ca", f, 8),
            "synth": host_table("recon_synth", f, 32 * 64).reshape(32, 64), "dwin": host_table("recon_dwin", f, 512),
            "pretab": np.array(D.PRETAB), "r2": f(0.70710678118654752440)}


# ---- a launch ----
class Launch:
    def __init__(self, cls, NG, nfr=None, note=""):
        self.cls, self.NG, self.note = list(cls), NG, note
        S = self.S = len(self.cls)
        assert 1 <= S <= 10 and NG % 2 == 0 and 2 <= NG <= 16
        self.nfr = None if nfr is None else np.array(nfr, dtype=np.int32)
        z = lambda *shape: np.zeros((S, NG, 2) + shape, dtype=np.int64)
        self.bt, self.ms = np.zeros((S, NG), dtype=np.int64), np.zeros((S, NG // 2), dtype=np.int64)
        self.gg, self.sbg, self.sfl, self.sfs = z() + 210, z(3), z(22), z(12, 3)       # sfs: [band][window]
        self.scale, self.pre, self.bv, self.nq, self.nn = z(), z(), z() + 288, z(), z() + 1
        self.ix = np.zeros((S, NG, 2, 576), dtype=np.int16)
        self.sign = np.zeros((S, NG, 2, 576), dtype=np.uint8)
        self.state = np.zeros((S, layouts()["state"]), dtype=np.float32)
        self.fill = np.float32(0.0)         # what hyb and out hold before the call
        self.row = (NG // 2) * 1152 * 2

    def nchan(self, s):
        return CLASSES[self.cls[s]]["nchan"]

    def rate(self, s):
        return CLASSES[self.cls[s]]["rate"]

    def frames(self, s):
        return self.NG // 2 if self.nfr is None else int(self.nfr[s])

    def ncoded(self, s, g, ch):
        return min(576, 2 * int(self.bv[s, g, ch]) + 4 * int(self.nq[s, g, ch])) if self.nn[s, g, ch] else 0

    def units(self):
        """every (stream, granule, channel) a kernel reads"""
        return [(s, g, ch) for s in range(self.S) for g in range(2 * self.frames(s)) for ch in range(self.nchan(s))]

    def classes(self):
        return sorted(set(self.cls))

    def set_types(self, s, seq):
        assert len(seq) == self.NG and all(b in SUCC[a] for a, b in zip(seq, seq[1:])), seq
        self.bt[s] = seq

    def half(self, h, state=None):
        """granules h * NG / 2 .. of every stream as a launch of their own"""
        n = self.NG // 2
        assert self.nfr is None and n % 2 == 0
        L = Launch(self.cls, n)
        for a in ("bt", "gg", "sbg", "sfl", "sfs", "scale", "pre", "bv", "nq", "nn", "ix", "sign"):
            setattr(L, a, getattr(self, a)[:, h * n:(h + 1) * n].copy())
        L.ms = self.ms[:, h * n // 2:(h + 1) * n // 2].copy()
        L.state = (self.state if state is None else state).copy()
        return L


def short_line(rate, sb_line, w):
    """bitstream position of line sb_line (0 .. 191) of window w in a short granule"""
    ss = D.SFB_SHORT[rate]
    b = max(k for k in range(13) if ss[k] <= sb_line)
    return 3 * ss[b] + w * (ss[b + 1] - ss[b]) + sb_line - ss[b]


def device_arrays(L):
    """what hx_debug_recon takes of a launch: ixq, sgn, seg, rec, and hyb / out filled with L.fill"""
    lay = layouts()
    S, NG = L.S, L.NG
    bits = np.packbits(L.sign.astype(bool), axis=-1, bitorder="little")         # bit j & 31 of word j >> 5
    sgn = np.zeros((S, NG, 2, lay["sgn_words"]), dtype=np.uint32)
    sgn[..., :18] = np.ascontiguousarray(bits).view("<u4")
    seg = np.zeros((S, NG, 2), dtype=lay["seg"])
    seg["sf"][..., :36] = (4 << 8) | L.sfs.reshape(S, NG, 2, 36)                # (length << 8) | value at field 3 * band + window
    rec = np.zeros((S, NG // 2), dtype=lay["rec"])
    rec["ms"] = L.ms
    q = rec["gr"]
    for name, a in (("block_type", np.repeat(L.bt[:, :, None], 2, axis=2)), ("global_gain", L.gg), ("preflag", L.pre), ("scalefac_scale", L.scale),
                    ("big_values", L.bv), ("aux_nquads", L.nq), ("aux_not_null", L.nn)):
        q[name] = a.reshape(S, NG // 2, 2, 2)
    q["window_switching_flag"] = q["block_type"] != 0
    q["subblock_gain"] = L.sbg.reshape(S, NG // 2, 2, 2, 3)
    rec["sf"] = L.sfl.reshape(S, NG // 2, 2, 2, 22)
    return {"cls": np.array([L.classes().index(c) for c in L.cls], dtype=np.int32), "ecs": [api.default_control(**CLASSES[c]["kw"]) for c in L.classes()],
            "ixq": L.ix.copy(), "sgn": sgn, "seg": seg, "rec": rec, "state": L.state.copy(),
            "hyb": np.full((S, NG, 2, 576), L.fill, dtype=np.float32), "out": np.full((S, L.row), L.fill, dtype=np.float32)}


def debug_recon(L, device=0, **change):
    """hx_debug_recon on a launch -> (rc, state, hyb [S][NG][2][18][32], out [S][row])"""
    a = device_arrays(L)
    a.update(change)
    rc, state, hyb, out = api.debug_recon(a["ecs"], a["cls"], L.NG, L.nfr, a["ixq"], a["sgn"], a["seg"].view(np.uint8), a["rec"].view(np.uint8),
                                          a["state"], a["hyb"], a["out"], device)
    return rc, state, hyb.reshape(L.S, L.NG, 2, 18, 32), out


# ---- the float64 reference and its magnitude pass ----
def frame_info(L, s, f):
    """the dict mp3_decode.Decoder.back_half takes for frame f of stream s: what lies from the coded range on is zero"""
    nch = L.nchan(s)
    info = {"samprate": L.rate(s), "nch": nch, "ms": int(L.ms[s, f]) if nch == 2 else 0, "gr": [[None] * nch for _ in range(2)]}
    for g in range(2):
        for ch in range(nch):
            G = 2 * f + g
            coded = np.arange(576) < L.ncoded(s, G, ch)
            bt = int(L.bt[s, G])
            info["gr"][g][ch] = {
                "ix": np.where(coded, L.ix[s, G, ch].astype(np.int64) & 0xFFFF, 0), "sign": np.where(coded, L.sign[s, G, ch], 0).astype(np.int64),
                "sf": [list(map(int, r)) for r in L.sfs[s, G, ch]] + [[0, 0, 0]] if bt == 2 else list(map(int, L.sfl[s, G, ch])),
                "global_gain": int(L.gg[s, G, ch]), "subblock_gain": list(map(int, L.sbg[s, G, ch])), "scalefac_scale": int(L.scale[s, G, ch]),
                "preflag": int(L.pre[s, G, ch]), "block_type": bt}
    return info


def reference(L):
    """{"hyb", "hyb_mag": [S][NG][2][18][32], "out", "out_mag": [S][row]} float64; zero where no kernel writes"""
    lay = layouts()
    r = {"hyb": np.zeros((L.S, L.NG, 2, 18, 32)), "out": np.zeros((L.S, L.row))}
    r["hyb_mag"], r["out_mag"] = np.zeros_like(r["hyb"]), np.zeros_like(r["out"])
    for s in range(L.S):
        nch = L.nchan(s)
        st = L.state[s].astype(np.float64)
        tail, hist = st[:lay["tail"]].reshape(2, 32, 18), st[lay["tail"]:].reshape(2, lay["hist"], 32)
        for key, magnitude in (("", False), ("_mag", True)):
            d = D.Decoder(None, magnitude=magnitude)
            d.tail = np.abs(tail) if magnitude else tail.copy()
            for ch in range(2):     # the matrixed vectors of the carried slots, newest first
                d.vhist[ch] = ((np.abs(hist[ch]) if magnitude else hist[ch]) @ d.matrix.T)[::-1]
            for f in range(L.frames(s)):
                d.taps = []
                pcm = d.back_half(frame_info(L, s, f))
                for i, h in enumerate(d.taps):
                    r["hyb" + key][s, 2 * f + i // nch, i % nch] = h
                r["out" + key][s, f * 1152 * nch:(f + 1) * 1152 * nch] = pcm.reshape(-1)
    return r


# ---- the kernels' operation order in float32 numpy ----
MUTANTS = {     # name: the list it must break the bound on
    "ca7_negated": "alias", "pretab20_is_3": "exponent_long", "windows_1_and_3_exchanged": "transforms", "subblock_gain_of_next_window": "exponent_short",
    "short_scalefactor_at_3w_plus_b": "exponent_short", "ms_constant_0.7071": "ms", "inversion_on_even_subbands": "transforms", "one_dwin_tap_negated": "synthesis"}


@functools.lru_cache(maxsize=None)
def line_maps(rate, short):
    """per bitstream line j: (band, window, position in the hybrid's [32][18] order)"""
    j = np.arange(576)
    if not short:
        return np.minimum(np.searchsorted(np.array(D.SFB_LONG[rate][1:22]), j, side="right"), 21), np.zeros(576, dtype=np.int64), j
    ss = np.array(D.SFB_SHORT[rate])
    b = np.minimum(np.searchsorted(3 * ss[1:13], j, side="right"), 12)
    wd, r = ss[b + 1] - ss[b], j - 3 * ss[b]
    w = r // wd
    l = ss[b] + r - w * wd
    return b, w, (l // 6) * 18 + 6 * w + l % 6


def restate(L, mutant=None, dtype=np.float32, parts=None):
    """the three kernels on a launch, operation by operation in their order, float32 -> (state, hyb, out) as debug_recon.
    dtype=float64 evaluates the same expressions in double (the reach analysis of tests/test_recon_granule_cases.py), and
    parts, a dict, gets what stands between them: "lines" [S][NG][2][32][18] ahead of the alias reduction, "alias" behind it,
    "full" [S][NG][2][32][36] the windowed transforms ahead of the overlap"""
    f = dtype
    T = {k: (v.astype(f) if k not in ("pow43", "pow2q", "pretab") else v) for k, v in device_tables().items()}
    pretab = T["pretab"].copy()
    if mutant == "ca7_negated":
        T["ca"] = T["ca"].copy()
        T["ca"][7] = -T["ca"][7]
    if mutant == "pretab20_is_3":
        pretab[20] = 3
    if mutant == "windows_1_and_3_exchanged":
        T["win"] = T["win"][[0, 3, 2, 1]]
    if mutant == "ms_constant_0.7071":
        T["r2"] = f(0.7071)
    if mutant == "one_dwin_tap_negated":
        T["dwin"] = T["dwin"].copy()
        T["dwin"][65] = -T["dwin"][65]
    lay = layouts()
    S, NG = L.S, L.NG
    x = np.zeros((S, NG, 2, 576), dtype=f)
    for s, g, ch in L.units():      # requantisation (recon_lines)
        short = L.bt[s, g] == 2
        b, w, at = line_maps(L.rate(s), bool(short))
        mul = 4 if L.scale[s, g, ch] else 2
        e4 = int(L.gg[s, g, ch]) - 210
        if short:
            sbg = L.sbg[s, g, ch][(w + 1) % 3] if mutant == "subblock_gain_of_next_window" else L.sbg[s, g, ch][w]
            fields = np.concatenate([L.sfs[s, g, ch].reshape(36), np.zeros(4, dtype=np.int64)])
            idx = np.minimum(3 * w + b, 39) if mutant == "short_scalefactor_at_3w_plus_b" else np.minimum(3 * b + w, 39)
            e4 = e4 - (8 * sbg + mul * fields[idx] * (b < 12))
        else:
            e4 = e4 - np.where(b < 21, mul * (L.sfl[s, g, ch][b] + (pretab[b] if L.pre[s, g, ch] else 0)), 0)
        mag = np.minimum(L.ix[s, g, ch].astype(np.int64) & 0xFFFF, 16383)
        v = np.ldexp(T["pow43"][mag] * T["pow2q"][e4 & 3], e4 >> 2).astype(f)
        v = np.where(L.sign[s, g, ch] != 0, -v, v)
        x[s, g, ch, at] = np.where(np.arange(576) < L.ncoded(s, g, ch), v, f(0.0))
    for s in range(S):              # M/S
        for g in range(2 * L.frames(s)):
            if L.nchan(s) == 2 and L.ms[s, g // 2]:
                m, sd = x[s, g, 0].copy(), x[s, g, 1].copy()
                x[s, g, 0], x[s, g, 1] = (m + sd) * T["r2"], (m - sd) * T["r2"]
    lo = 18 * np.arange(1, 32)[:, None] - 1 - np.arange(8)[None, :]
    hi = 18 * np.arange(1, 32)[:, None] + np.arange(8)[None, :]
    a, b = x[..., lo], x[..., hi]
    xa = x.copy()
    xa[..., lo], xa[..., hi] = a * T["cs"] - b * T["ca"], b * T["cs"] + a * T["ca"]
    long_ = (L.bt != 2)[:, :, None, None]
    if parts is not None:
        parts["lines"] = x.reshape(S, NG, 2, 32, 18).copy()
    x = np.where(long_, xa, x).reshape(S, NG, 2, 32, 18)
    # the windowed IMDCT of every granule: 36 points, or three 12-point transforms laid at 6, 12 and 18
    full = np.zeros((S, NG, 2, 32, 36), dtype=f)
    for k in range(18):
        full = full + x[..., k, None] * T["cos36"][:, k]
    full = full * T["win"][L.bt][:, :, None, None, :]
    sh = np.zeros((S, NG, 2, 32, 36), dtype=f)
    for w in range(3):
        y = np.zeros((S, NG, 2, 32, 12), dtype=f)
        for k in range(6):
            y = y + x[..., 6 * w + k, None] * T["cos12"][:, k]
        sh[..., 6 + 6 * w:18 + 6 * w] = sh[..., 6 + 6 * w:18 + 6 * w] + y * T["win"][2, :12]
    full = np.where(long_[..., None], full, sh)
    if parts is not None:
        parts["alias"], parts["full"] = x, full
    carried = L.state[:, :lay["tail"]].reshape(S, 2, 32, 18).astype(f)
    tail = np.concatenate([carried[:, None], full[:, :-1, :, :, 18:]], axis=1)
    h = full[..., :18] + tail
    inv = (np.arange(32)[:, None] & 1) & (np.arange(18)[None, :] & 1)
    if mutant == "inversion_on_even_subbands":
        inv = (1 - (np.arange(32)[:, None] & 1)) & (np.arange(18)[None, :] & 1)
    h = np.where(inv.astype(bool), -h, h).transpose(0, 1, 2, 4, 3)        # [S][NG][2][18][32]
    hyb = np.full((S, NG, 2, 18, 32), L.fill, dtype=f)
    out = np.full((S, L.row), L.fill, dtype=f)
    state = L.state.astype(f)
    H = lay["hist"]
    for s in range(S):
        nf, nch = L.frames(s), L.nchan(s)
        if nf == 0:
            continue
        hyb[s, :2 * nf, :nch] = h[s, :2 * nf, :nch]
        for ch in range(nch):
            hist = L.state[s, lay["tail"]:].reshape(2, H, 32)[ch].astype(f)
            seq = np.concatenate([hist, hyb[s, :2 * nf, ch].reshape(-1, 32)])      # the time slots, oldest first
            v = np.zeros((seq.shape[0], 64), dtype=f)
            for k in range(32):     # matrixing, k ascending
                v = v + T["synth"][k][None, :] * seq[:, k, None]
            nt = 36 * nf
            t = H + np.arange(nt)
            acc = np.zeros((nt, 32), dtype=f)
            for k in range(8):
                acc = acc + (T["dwin"][64 * k:64 * k + 32] * v[t - 2 * k, :32] + T["dwin"][64 * k + 32:64 * k + 64] * v[t - 2 * k - 1, 32:])
            out[s, :nt * 32 * nch].reshape(-1, nch)[:, ch] = acc.reshape(-1)
            state[s, ch * 576:(ch + 1) * 576] = full[s, 2 * nf - 1, ch, :, 18:].reshape(-1)
            state[s, lay["tail"] + ch * H * 32:lay["tail"] + (ch + 1) * H * 32] = seq[-H:].reshape(-1)
    return state, hyb, out


# ---- holding a result to the reference ----
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(name, i, L, ref, state, hyb, out):
    """holds one launch's result (of the device or of restate) to its reference; -> the largest error / bound of the hybrid
    tap and of the output.  A failure names list, launch, stream, granule, channel, slot / subband or sample, got, want, bound."""
    lay = layouts()
    where = "list %s launch %d%s" % (name, i, (" (" + L.note + ")") if L.note else "")
    written_h = np.zeros(hyb.shape, dtype=bool)
    written_o = np.zeros(out.shape, dtype=bool)
    for s in range(L.S):
        written_h[s, :2 * L.frames(s), :L.nchan(s)] = True
        written_o[s, :L.frames(s) * 1152 * L.nchan(s)] = True
    ratios = []
    for what, got, key, k, floor, written in (("hyb", hyb, "hyb", K_HYB, FLOOR_HYB, written_h), ("out", out, "out", K_OUT, FLOOR_OUT, written_o)):
        want, mag = ref[key], ref[key + "_mag"]
        names = "(stream, granule, channel, slot, subband)" if what == "hyb" else "(stream, sample of the row)"
        keep = ~written & (bits(got) != bits(np.full(1, L.fill))[0])
        assert not keep.any(), "%s: %s %s %s is written and belongs to no frame of the call" % (where, what, names, tuple(int(v) for v in np.argwhere(keep)[0]))
        assert np.isfinite(got[written]).all(), "%s: %s is not finite" % (where, what)
        bound = gamma(k) * mag + floor
        err = np.abs(got.astype(np.float64) - want)
        bad = written & (err > bound)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: %s %s %s: got %r, want %r, bound %.3g (error %.3g; %d values beyond their bounds)" % (
                where, what, names, at, float(got[at]), float(want[at]), bound[at], err[at], bad.sum()))
        # zeros are exact: +0, or -0 where the frequency inversion negates a hybrid value
        zero = np.zeros(got.shape, dtype=np.uint32)
        if what == "hyb":
            zero[..., 1::2, 1::2] = 0x80000000
        bad = written & (mag == 0) & (bits(got) != zero)
        at = tuple(int(v) for v in np.argwhere(bad)[0]) if bad.any() else None
        assert at is None, "%s: %s %s %s: got %r where nothing is coded, want a zero of bits 0x%08x" % (where, what, names, at, float(got[at]), zero[at])
        ratios.append(float((err[written] / bound[written]).max()) if written.any() else 0.0)
    # the state: untouched where no frame was coded, else the last 15 slots of the returned hybrid output by bits
    H = lay["hist"]
    for s in range(L.S):
        nf, nch = L.frames(s), L.nchan(s)
        st, st0 = bits(state[s]), bits(L.state[s])
        same = np.ones(st.size, dtype=bool)
        if nf:
            for ch in range(nch):
                same[ch * 576:(ch + 1) * 576] = False
                a = lay["tail"] + ch * H * 32
                same[a:a + H * 32] = False
                slots = np.concatenate([L.state[s, a:a + H * 32].reshape(H, 32), hyb[s, :2 * nf, ch].reshape(-1, 32)])[-H:]
                assert np.array_equal(st[a:a + H * 32], bits(slots).reshape(-1)), "%s: stream %d channel %d: the carried slots are not the hybrid output's last 15" % (where, s, ch)
                assert np.isfinite(state[s, ch * 576:(ch + 1) * 576]).all(), "%s: stream %d: a tail is not finite" % (where, s)
        assert np.array_equal(st[same], st0[same]), "%s: stream %d: state no frame of the call owns was written" % (where, s)
    return ratios


# ---- the lists ----
def walk_types(rng, NG, first=None):
    seq = [int(rng.integers(4)) if first is None else first]
    while len(seq) < NG:
        seq.append(int(rng.choice(SUCC[seq[-1]])))
    return seq


def types_through(a, b, NG, at):
    """a legal sequence with (a, b) at granules (at - 1, at)"""
    seq = [a, b]
    for _ in range(at - 1):
        seq.insert(0, PRED[seq[0]][len(seq) % len(PRED[seq[0]])])
    while len(seq) < NG:
        seq.append(SUCC[seq[-1]][len(seq) % len(SUCC[seq[-1]])])
    return seq


GAINS = (0, 255, 210, 211, 212, 213, 180, 161, 230, 243, 127, 94)       # both ends, the four residues, a few exponents


def list_pow43():
    """every magnitude 0 .. 8206 alone in its subband (line 18 sb + 8: outside every butterfly) of a long granule between
    zero long granules, zero state: the subband's 36 outputs depend on that one table entry"""
    rng = np.random.default_rng(4301)
    mags, out, k = np.arange(MAX_MAG + 1), [], 0
    while k < mags.size:
        L = Launch(["s44"] * 10, 16, note="magnitudes from %d" % k)
        for s in range(10):
            for g in range(1, 15, 2):
                for ch in range(2):
                    m = mags[k:k + 32]
                    L.ix[s, g, ch, 18 * np.arange(m.size) + 8] = m
                    L.sign[s, g, ch] = rng.integers(0, 2, 576)
                    L.gg[s, g, ch] = GAINS[(k // 32) % len(GAINS)]
                    k += m.size
        out.append(L)
    return out


def list_exponent_long():
    """at each rate: the first and last line of every long band, over scalefac_scale x preflag x scalefactor 0 / 1 / largest"""
    out = []
    for cls in ("s44", "s48", "s32"):
        L = Launch([cls] * 6, 2, note=cls)
        bl = D.SFB_LONG[CLASSES[cls]["rate"]]
        combos = [(sc, pre, v) for sc in (0, 1) for pre in (0, 1) for v in (0, 1, None)]
        for i, (sc, pre, v) in enumerate(combos):
            s, ch = i // 2, i % 2
            L.scale[s, 0, ch], L.pre[s, 0, ch], L.gg[s, 0, ch] = sc, pre, 200 + i
            for b in range(22):
                L.sfl[s, 0, ch, b] = 0 if b == 21 else (15 if b < 11 else 7) if v is None else v
                L.ix[s, 0, ch, bl[b]], L.ix[s, 0, ch, bl[b + 1] - 1] = 1 + (5 * b + i) % 17, 2 + (3 * b + i) % 13
                L.sign[s, 0, ch, bl[b]] = (b + i) & 1
        out.append(L)
    return out


def list_exponent_short():
    """at each rate: the first and last line of every short band's three runs, three different subblock gains (7, 0, 3 and
    rotations), three different scalefactors per band, scalefac_scale both ways; band 12 takes no scalefactor"""
    out = []
    for cls in ("s44", "s48", "s32"):
        L = Launch([cls] * 3, 2, note=cls)
        ss = D.SFB_SHORT[CLASSES[cls]["rate"]]
        L.bt[:] = 2
        for i in range(6):
            s, ch = i // 2, i % 2
            L.scale[s, 0, ch], L.gg[s, 0, ch] = i & 1, 215 + i
            L.sbg[s, 0, ch] = np.roll([7, 0, 3], i // 2)
            for b in range(13):
                wd = ss[b + 1] - ss[b]
                for w in range(3):
                    if b < 12:
                        L.sfs[s, 0, ch, b, w] = (1 + 5 * w + b + i) % 16 if b < 6 else (1 + 3 * w + b + i) % 8
                    j = 3 * ss[b] + w * wd
                    L.ix[s, 0, ch, j], L.ix[s, 0, ch, j + wd - 1] = 1 + (5 * b + w + i) % 17, 2 + (3 * b + 2 * w + i) % 13
                    L.sign[s, 0, ch, j] = (b + w + i) & 1
        out.append(L)
    return out


def dense(rng, L, s, g, ch, top=15):
    L.ix[s, g, ch] = rng.integers(1, top + 1, 576)
    L.sign[s, g, ch] = rng.integers(0, 2, 576)


CODED = ((0, 0, 1), (1, 0, 1), (0, 1, 1), (287, 0, 1), (288, 0, 1), (288, 10, 1), (200, 50, 1), (288, 0, 0))       # big_values, quads, aux_not_null


def list_coded_range():
    """the coded range at 0, 2, 4, 574, 576, twice above 576, and aux_not_null 0 over non-zero lines; the lines from it on
    hold 0x7FFF (left) or negative values (right), with their sign bits set: the reference sees zeros there"""
    rng = np.random.default_rng(4302)
    L = Launch(["s44"] * len(CODED), 4)
    for s, (bv, nq, nn) in enumerate(CODED):
        L.set_types(s, [0, 1, 2, 2] if s & 1 else [0, 0, 0, 0])
        for g in range(3):
            for ch in range(2):
                dense(rng, L, s, g, ch)
                L.bv[s, g, ch], L.nq[s, g, ch], L.nn[s, g, ch] = bv, nq, nn
                n = L.ncoded(s, g, ch)
                L.ix[s, g, ch, n:] = 0x7FFF if ch == 0 else -1 - (np.arange(576 - n) * 1237) % 32768
                L.sign[s, g, ch, n:] = 1
    return [L]


SIGN_LINES = sorted({0, 575} | {32 * k - 1 for k in range(1, 18)} | {32 * k for k in range(1, 18)})


def list_signs():
    """a set sign bit at one line at a time, at both sides of every word boundary, and the complement of that pattern"""
    out, todo = [], [(j, c) for j in SIGN_LINES for c in (0, 1)]
    for k in range(0, len(todo), 18):
        part = todo[k:k + 18]
        L = Launch(["s44"] * ((len(part) + 1) // 2), 2, note="lines from %d" % part[0][0])
        for i, (j, c) in enumerate(part):
            s, ch = i // 2, i % 2
            L.ix[s, 0, ch] = 1 + np.arange(576) % 7
            L.sign[s, 0, ch] = c
            L.sign[s, 0, ch, j] = 1 - c
        out.append(L)
    return out


def list_ms():
    """ms with both channels non-zero, one zero, equal channels; on a mono class (ignored); differing between a call's frames"""
    rng = np.random.default_rng(4303)
    L = Launch(["s44"] * 5 + ["m44"], 4)
    for s in range(6):
        L.set_types(s, [0, 1, 2, 3] if s & 1 else [0, 0, 0, 0])
        for g in range(4):
            for ch in range(2):
                dense(rng, L, s, g, ch, 100)
    L.ms[:3], L.ms[5] = 1, 1
    L.ix[1, :, 1] = 0
    L.ix[2, :, 1], L.sign[2, :, 1] = L.ix[2, :, 0], L.sign[2, :, 0]
    L.ms[3], L.ms[4] = (1, 0), (0, 1)
    return [L]


def list_alias():
    """unit lines at each of the 16 butterfly positions around subband boundaries 1, 16 and 31, on block types 0, 1 and 3,
    and the same lines in a short granule, where no butterfly may act"""
    L = Launch(["s44"] * 8, 4)
    for p in range(16):
        s, ch = p // 2, p % 2
        L.set_types(s, [0, 1, 2, 3])
        for g in range(4):
            for sb in (1, 16, 31):
                L.ix[s, g, ch, 18 * sb - 1 - p if p < 8 else 18 * sb + p - 8] = 1
            L.sign[s, g, ch, 18 * 16:] = (p + g) & 1
    return [L]


TRANSFORM_SB = (4, 5)


def transform_streams():
    """block-type sequences in which every legal transition stands at an odd granule, at an even one, and at (7, 8)"""
    a = [0, 0, 1, 2, 2, 3, 0, 1, 2, 3, 1, 2, 2, 3, 0, 0]
    return [a, [0] + a[:15]] + [types_through(x, y, 16, 8) for x, y in TRANSITIONS]


def list_transforms():
    """one non-zero line at a time at each of the 18 positions of an even and an odd subband on block types 0, 1 and 3, and
    at each of the 6 positions of each window of a short block, in sequences that hold every legal transition inside a frame
    and at a frame boundary (and, split, across the carried state)"""
    seqs = transform_streams()
    L = Launch(["s44"] * len(seqs), 16)
    count = {0: 0, 1: 0, 2: 0, 3: 0}
    for s, seq in enumerate(seqs):
        L.set_types(s, seq)
        for g in range(16):
            for ch in range(2):
                bt, n = seq[g], count[seq[g]]
                count[bt] += 1
                sb = TRANSFORM_SB[n % 2]
                if bt == 2:
                    w, k = (n // 2) % 3, (n // 6) % 6
                    j = short_line(44100, 6 * sb + k, w)
                else:
                    j = 18 * sb + (n // 2) % 18
                L.ix[s, g, ch, j], L.sign[s, g, ch, j], L.gg[s, g, ch] = 1 + n % 3, n & 1, 210 + n % 4
    return [L]


def list_synthesis():
    """a carried state of the test's with all lines zero: one slot of one subband non-zero at a time over all 32 x 15, and
    random tails - the matrixing's columns and the window's 512 taps, and the read of a state no kernel of the run wrote"""
    rng = np.random.default_rng(4304)
    lay, out = layouts(), []
    todo = [(sb, slot) for sb in range(32) for slot in range(15)]
    for k in range(0, len(todo), 20):
        L = Launch(["s44"] * 10, 2, note="(subband, slot) from %s" % (todo[k],))
        L.state[:, :lay["tail"]] = rng.normal(0.0, 100.0, (10, lay["tail"]))
        for i, (sb, slot) in enumerate(todo[k:k + 20]):
            L.state[i // 2, lay["tail"] + ((i % 2) * 15 + slot) * 32 + sb] = (1000.0 + 7 * sb + slot) * (-1) ** (sb + slot)
        out.append(L)
    return out


def random_granule(rng, L, s, g, ch):
    L.ix[s, g, ch] = np.where(rng.random(576) < 0.02, rng.integers(0, MAX_MAG + 1, 576), rng.integers(0, 16, 576))
    L.sign[s, g, ch] = rng.integers(0, 2, 576)
    L.gg[s, g, ch] = rng.integers(0, 256)
    L.sbg[s, g, ch] = rng.integers(0, 8, 3)
    L.sfl[s, g, ch, :11], L.sfl[s, g, ch, 11:21] = rng.integers(0, 16, 11), rng.integers(0, 8, 10)
    L.sfs[s, g, ch, :6], L.sfs[s, g, ch, 6:] = rng.integers(0, 16, (6, 3)), rng.integers(0, 8, (6, 3))
    L.scale[s, g, ch], L.pre[s, g, ch] = rng.integers(0, 2, 2)
    L.bv[s, g, ch], L.nq[s, g, ch], L.nn[s, g, ch] = rng.integers(0, 289), rng.integers(0, 60), rng.random() < 0.9
    if rng.random() < 0.1:      # (the ends of the range)
        L.bv[s, g, ch] = rng.choice([0, 288])
    L.ix[s, g, ch, L.ncoded(s, g, ch):] = rng.integers(-32768, 32768, 576 - L.ncoded(s, g, ch))


def random_launch(seed, cls, NG, nfr=None):
    rng = np.random.default_rng(seed)
    L = Launch(cls, NG, nfr)
    for s in range(L.S):
        L.set_types(s, walk_types(rng, NG))
        L.ms[s] = rng.integers(0, 2, NG // 2)
        for g in range(NG):
            for ch in range(2):
                random_granule(rng, L, s, g, ch)
    L.state[:] = rng.normal(0.0, 300.0, L.state.shape)
    return L


def list_counts_and_kinds():
    """a mono and a stereo class in one launch, counts 0, 1 and NG / 2, everything pre-filled with a sentinel: the blocks
    behind a stream's count, a mono row's unused half and a count-0 stream's state come back untouched"""
    L = random_launch(4305, ["m44", "s44", "s44", "m44", "s44", "m44"], 4, nfr=[2, 0, 1, 1, 2, 0])
    L.fill = SENTINEL
    L.state[1], L.state[5], L.state[0, 576:1152] = SENTINEL, SENTINEL, SENTINEL
    return [L]


def list_split():
    """a handful of the transforms' and random streams as one launch of 16 granules - and, in the GPU test, as two of 8 with
    the first's state fed to the second: the same float bits"""
    T = list_transforms()[0]
    L = random_launch(4306, ["s44", "m48", "s32"] + ["s44"] * 7, 16)
    for i, (a, b) in enumerate(TRANSITIONS):
        s = 3 + i
        for name in ("bt", "gg", "ix", "sign"):
            getattr(L, name)[s] = getattr(T, name)[2 + i]
        for name in ("sbg", "sfl", "sfs", "scale", "pre", "nq"):
            getattr(L, name)[s] = 0
        L.bv[s], L.nn[s], L.ms[s] = 288, 1, 0
    return [L]


def list_random():
    """dense random granules over the whole legal range of every field, with a random carried state"""
    return [random_launch(4307, ["s44", "m44", "s48", "s32", "s44", "m48", "s48", "s32", "s44", "s44"], 16),
            random_launch(4308, ["s32", "s48", "m44", "s44", "s44"], 6)]


@functools.lru_cache(maxsize=None)
def case_list(name):
    assert name in LIST_NAMES, name
    return tuple(globals()["list_" + name]())


@functools.lru_cache(maxsize=None)
def references(name):
    """the float64 reference of every launch of a list, computed once and left unchanged"""
    return tuple(reference(L) for L in case_list(name))
