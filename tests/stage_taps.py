"""Stage-by-stage comparison of a batch with the oracle's taps (test infrastructure): K1 polyphase, the attack metric of
K2, K4 MDCT (long and short layouts) and psy model (long on every path; short: the spread sums, and the masks after
pre-echo control formed from them and the carried memory), block types, K5 stereo decision, K5b (k_prep) magnitudes,
x^(3/4), band start values and masks after pre-echo control, K6 side info / scalefactors / reservoir, what K6 hands to the
packer (quantised lines and signs), and every call's bytes.  Float values are compared by bit pattern, so -0.0 and +0.0,
and a subnormal and the zero a flush would leave, are different values.  Index ranges come from the oracle's counts and the
host tables, never from the GPU's output.  The PCM is int16 or float32 (the oracle is then fed through encode_s16 or
encode_f32), in one call or in several, with or without per-stream frame counts: the taps are read after every call."""
import ctypes as C

import numpy as np

from oracle import oracle as O

TINY = np.float32(2.0 ** -126)      # the smallest normal float32
F01 = np.float32(0.1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def subnormals(a):
    """how many values of a (taken as float32) are subnormal: non-zero and below 2^-126 in magnitude"""
    a = np.abs(np.asarray(a, dtype=np.float32))
    return int(((a > 0) & (a < TINY)).sum())


def same(stage, where, got, want, as_bits=True):
    """assert two arrays equal (floats by bit pattern), naming the stage, the place and the first index that differs"""
    a, b = (bits(got), bits(want)) if as_bits else (np.asarray(got), np.asarray(want))
    assert a.shape == b.shape, (stage,) + tuple(where) + (a.shape, b.shape)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero((a != b).reshape(-1))[0])
        raise AssertionError((stage,) + tuple(where) + ("index %d" % i, "gpu %r" % np.asarray(got).reshape(-1)[i].item(),
                                                        "oracle %r" % np.asarray(want).reshape(-1)[i].item()))


def preecho_branches(thr, prev2):
    """(taken, floor): in how many partitions the long model's pre-echo control clamps thr against prev2 = twice the previous
    granule's unclamped thresholds (thr > prev2), and in how many of those the result is the 0.1 * thr floor (prev2 < 0.1 * thr)"""
    thr, prev2 = np.asarray(thr, dtype=np.float32), np.asarray(prev2, dtype=np.float32)
    taken = thr > prev2
    return int(taken.sum()), int((taken & (prev2 < F01 * thr)).sum())


def short_masks(thr36, mpart, prev_short, carry):
    """[3, mpart] float32: the masks of a short granule after pre-echo control (reference spdsmr.c:112-184) formed from the
    spread sums thr36 = [12 * w + sfb], with the reference's float32 operations.  carry: window 2's doubled sums of the
    granule before, used when that one was short too (prev_short)."""
    t = np.asarray(thr36, dtype=np.float32).reshape(3, 12)[:, :mpart]
    m = t.copy()
    two = np.float32(2.0)
    lim = [np.asarray(carry, dtype=np.float32)[:mpart], two * t[0], two * t[1]]
    for w in range(3):
        if w == 0 and not prev_short:
            continue
        floor = F01 * t[w]
        m[w] = np.where(t[w] > lim[w], np.where(lim[w] > floor, lim[w], floor), t[w])
    out = m.copy()
    out[1] = m[1] + F01 * m[0]
    out[2] = m[2] + F01 * m[1]
    return out


class GDbg(C.Structure):
    """HxFrameDebug (hmp3_amd/csrc/hx_types.h): the "dbg" tap, one per stream and frame.  mask_mb is written by no kernel
    (unused): the masks after pre-echo control are the "band" tap's maskmb (GBand)."""
    _fields_ = [("ms", C.c_int), ("ms_metric", C.c_int * 2), ("byte_pool", C.c_int), ("MNR_after", C.c_int),
                ("mask_mb", C.c_int * 88), ("gr", C.c_int * 96), ("sf", C.c_int * 88), ("scfsi", C.c_int * 2),
                ("main_bytes", C.c_int)]


class GBand(C.Structure):
    """HxBandPrep (hmp3_amd/csrc/hx_types.h): the "band" tap, k_prep's output per stream and granule, [ch][sfb]"""
    _fields_ = [("xsxx", C.c_float * 44), ("x34max", C.c_float * 44), ("n0", C.c_int * 44), ("n0ms", C.c_int * 44),
                ("gzero", C.c_int * 44), ("maskmb", C.c_int * 44)]


def host_table(api, kw, name, n):
    """int32 [n]: a table or scalar the host resolves for this control (hx_debug_host_table)"""
    a = np.zeros(n, np.int32)
    assert api.lib().hx_debug_host_table(C.byref(api.default_control(**kw)), name.encode(), a.ctypes.data, a.nbytes) == a.nbytes, name
    return a


class TapBatch:
    """A batch of S streams of one configuration with the debug taps on, and one oracle encoder per stream.
    call(pcm, counts=None) encodes the next frames of every stream (of stream s: its first counts[s] frames of the call; a
    stream with 0 sits the call out, is compared with nothing and its oracle does not advance) on the GPU and in the oracle
    and asserts every tap and the bytes.
    taps: "full" (stereo MPEG-1 on the second-generation allocator: every tap) or "lines" (the other paths: everything but
    polyphase and the frame record of the allocator, which the oracle taps on the MPEG-1 stereo path only).
    After the calls: seen_bt (block types compared), frames (per stream), per stream and frame sub_sb / sub_xr, the number
    of subnormal values in the oracle's own sample_new / xr_pre taps; boundary_bt, the set of (block type of a stream's
    last granule before a call, type of its first granule in that call) compared; short_granules, per stream how many short
    granules went through the short-model comparison; prep_granules, how many long granules went through k_prep's (prep_ms:
    those of them coded M/S); from
    the oracle's own thr taps of the long granules compared, clamp_taken / clamp_floor: how many had the pre-echo clamp
    taken in some partition / held by the 0.1 * thr floor in some partition, and clamp_first: those of them that were a
    call's first granule; msscan_paths: which of k_msscan's loops the calls took ("vector": NG % 8 == 0, "scalar")."""

    def __init__(self, api, kw, nstreams, max_frames, taps="full", alloc_state=False):
        """kw: one control, or a list of nstreams controls of one kind (channel count, MPEG version and allocator
        generation in common; sample rates, bit rates and switches may differ).  alloc_state: compare the allocator's frame
        record on the "lines" paths too (reservoir, MNR, main-data bytes, long-block scalefactors granule by granule), and
        on the "full" path the scalefactors of the long granule of a frame that has a short one.  The scalefactors of short
        granules are in neither record: they are compared through scalefac_compress in the side information and the bytes"""
        self.api, self.S, self.maxF, self.taps, self.alloc_state = api, nstreams, max_frames, taps, alloc_state
        self.kws = list(kw) if isinstance(kw, (list, tuple)) else [kw] * nstreams
        assert len(self.kws) == nstreams
        self.kw = self.kws[0]
        self.mono = self.kw.get("mode") == 3
        assert all((k.get("mode") == 3) == self.mono for k in self.kws)
        if isinstance(kw, (list, tuple)):
            self.b = api.Batch([api.default_control(**k) for k in self.kws], max_frames=max_frames)
        else:
            self.b = api.Batch(api.default_control(**kw), nstreams=nstreams, max_frames=max_frames)
        self.b.debug_enable(True)
        self.tabs = []
        for k in self.kws:
            tab = lambda name, n: host_table(api, k, name, n)
            t = dict(np2=int(tab("psy_npart", 1)[0] + 1) & ~1, mpart=int(tab("psy_short_npart", 1)[0] + 1) >> 1,
                     alloc1=int(tab("alloc1", 1)[0]), hf=int(tab("scalars", 16)[7]), nbmax=tab("nbmax", 2), nbmax2=tab("nbmax2", 2),
                     nbmax3=tab("nbmax3", 2), start_l=tab("startBand_l", 23))
            assert int(tab("sizeof_band_prep", 1)[0]) == C.sizeof(GBand)
            assert 0 < t["mpart"] <= 12 and t["np2"] <= 64
            self.tabs.append(t)
        assert len({t["alloc1"] for t in self.tabs}) == 1
        self._use(0)
        self.enc = [O.OracleEncoder(O.default_control(**k)) for k in self.kws]
        self.dbg = [O.oracle_enable_debug(e) for e in self.enc]
        self.tap = [O.oracle_enable_stage_taps(e) for e in self.enc]      # (the taps beside the frame record: short model, start values, attack_prev)
        self.seen_bt = set()
        self.boundary_bt = set()
        self.msscan_paths = set()
        self.frames = [0] * nstreams
        self.short_granules = [0] * nstreams
        self.prep_granules = self.prep_ms = self.clamp_taken = self.clamp_floor = self.clamp_first = 0
        self.last_bt = [None] * nstreams
        self.last_thr = [None] * nstreams       # the oracle's thr taps of the stream's last granule, if it was a long one
        self.sub_sb = [[] for _ in range(nstreams)]
        self.sub_xr = [[] for _ in range(nstreams)]
        self.got = [b""] * nstreams

    def close(self):
        self.b.close()

    def _use(self, s):
        """the host tables of stream s's control"""
        t = self.tabs[s]
        self.np2, self.mpart, self.alloc1, self.hf = t["np2"], t["mpart"], t["alloc1"], t["hf"]
        self.nbmax, self.nbmax2, self.nbmax3, self.start_l = t["nbmax"], t["nbmax2"], t["nbmax3"], t["start_l"]

    def _prep(self, where, d, igr, xp, xmag, x34, band):
        """k_prep's outputs of one long granule against the allocator's start values in the oracle"""
        nch = 1 if self.mono else 2
        ms = int(d.start_ms[igr])
        nbx, nbe, nbz = (np.array(v).reshape(2, 2)[igr] for v in (d.nb_x, d.nb_e, d.nb_z))
        assert nbx[0] > 0 and nbe[0] > 0 and nbz[0] > 0, ("the oracle formed no start values",) + where
        # the line ranges k_prep documents (nl_mag, nl_p), from the host tables
        if ms:
            nl_mag = [int(self.start_l[22]) if self.hf else int(self.nbmax[0])] * 2
            nl_p = [int(self.nbmax2[0]), int(self.nbmax2[1])]
            lr = xp[igr].astype(np.float32)
            m, s = lr[0] + lr[1], lr[0] - lr[1]
            mag = [np.where(m < 0, -m, m), np.where(s < 0, -s, s)]
        else:
            nl_mag = nl_p = [int(self.nbmax3[0]), int(self.nbmax3[1])]
            mag = [np.where(xp[igr, ch] >= 0, xp[igr, ch], -xp[igr, ch]) for ch in range(2)]
        o = {k: np.array(getattr(d, k)).reshape(2, 2, 22)[igr] for k in ("xsxx", "x34max", "gzero", "noise0", "noise0_ms", "mask_mb")}
        g = {k: np.array(getattr(band, k)).reshape(2, 22) for k in ("xsxx", "x34max", "n0", "n0ms", "gzero", "maskmb")}
        nmask = min(21, self.np2 // 2)
        for ch in range(nch):
            w = where + (ch,)
            n = nl_mag[ch]
            same("xmag", w, xmag[ch, :n], mag[ch][:n])
            n = nl_p[ch]
            assert n <= nl_mag[ch]
            same("x34", w, x34[ch, :n], O.pow34(mag[ch][:n]))
            same("band xsxx", w, g["xsxx"][ch, :nbx[ch]], o["xsxx"][ch, :nbx[ch]])
            same("band x34max", w, g["x34max"][ch, :nbz[ch]], o["x34max"][ch, :nbz[ch]])
            same("band gzero", w, g["gzero"][ch, :nbz[ch]], o["gzero"][ch, :nbz[ch]], False)
            same("band n0", w, g["n0"][ch, :nbe[ch]], o["noise0"][ch, :nbe[ch]], False)
            if ms:
                same("band n0ms", w, g["n0ms"][ch, :nbe[ch]], o["noise0_ms"][ch, :nbe[ch]], False)
            same("band maskmb", w, g["maskmb"][ch, :nmask], o["mask_mb"][ch, :nmask], False)
        self.prep_granules += 1
        self.prep_ms += ms

    def call(self, pcm, counts=None):
        pcm = np.asarray(pcm)
        f32 = pcm.dtype == np.float32
        assert f32 or pcm.dtype == np.int16
        b, S, mono = self.b, self.S, self.mono
        F = pcm.shape[1] // 1152
        NG = 2 * F
        assert pcm.shape[0] == S and pcm.shape[1] == F * 1152 and 0 < F <= self.maxF
        if counts is not None:
            counts = [int(c) for c in counts]
            assert len(counts) == S and all(0 <= c <= F for c in counts) and max(counts) > 0
        b.frame_counts(counts)
        cnt = counts if counts is not None else [F] * S
        self.msscan_paths.add("vector" if NG % 8 == 0 and max(cnt) >= 4 else "scalar")
        got = b.encode_host(pcm)
        assert b.status() == 0
        nch = 1 if mono else 2
        sb = b.debug_read("sb", np.float32, S * 2 * (2 * self.maxF + 3) * 576).reshape(S, 2, 2 * self.maxF + 3, 576)
        xr = b.debug_read("xr", np.float32, S * NG * 1152).reshape(S, NG, 2, 576)
        etab = b.debug_read("etab", np.float32, S * NG * 128).reshape(S, NG, 2, 64)
        thr = b.debug_read("thr", np.float32, S * NG * 128).reshape(S, NG, 2, 64)
        thrprev = b.debug_read("thrprev", np.float32, S * 128).reshape(S, 2, 64)
        btg = b.debug_read("bt", np.uint8, S * NG).reshape(S, NG)
        atk = b.debug_read("attack", np.int32, S * NG * 4).reshape(S, NG, 2, 2)        # [short_flag_prev][ch]
        ixq = b.debug_read("ixq", np.int16, S * NG * 1152).reshape(S, NG, 2, 576).astype(np.int32) & 0xFFFF
        # the signs travel as one bit per line (bit j & 31 of word j >> 5; 20 words per granule and channel, 18 used)
        sgw = b.debug_read("sgn", np.uint32, S * NG * 2 * 20).reshape(S, NG, 2, 20)
        sgn = np.unpackbits(sgw[..., :18].copy().view(np.uint8), axis=-1, bitorder="little").reshape(S, NG, 2, 576)
        raw = b.debug_read("dbg", np.uint8, S * F * C.sizeof(GDbg))
        if not self.alloc1:
            xmag = b.debug_read("xmag", np.float32, S * NG * 1152).reshape(S, NG, 2, 576)
            x34 = b.debug_read("x34", np.float32, S * NG * 1152).reshape(S, NG, 2, 576)
            braw = b.debug_read("band", np.uint8, S * NG * C.sizeof(GBand)).reshape(S, NG, C.sizeof(GBand))
        for s in range(S):
            if cnt[s] == 0:
                assert got[s] == b"", ("bytes of a stream that took no frame", s)
                continue
            enc, d, t = self.enc[s], self.dbg[s], self.tap[s]
            self._use(s)
            np2, mpart = self.np2, self.mpart
            where = lambda *a: (s, self.frames[s] + f) + a      # stream, frame of the stream
            out = []
            for f in range(cnt[s]):
                frame = pcm[s, f * 1152:(f + 1) * 1152]
                out.append(enc.encode_f32(frame) if f32 else enc.encode_s16(frame))
                xp = np.array(d.xr_pre).reshape(2, 2, 576)
                oix = np.array(d.ix).reshape(2, 2, 576)
                osg = np.array(d.signx).reshape(2, 2, 576)
                ogr = np.array(d.gr).reshape(2, 2, 27)
                oe = np.array(d.etab).reshape(2, 2, 64)
                ot = np.array(d.thr).reshape(2, 2, 64)
                ots = np.array(t.thr_short).reshape(2, 2, 3, 12)
                oms = np.array(t.mask_short).reshape(2, 2, 3, 12)
                oat = np.array(d.attack).reshape(2, 2)
                self.sub_xr[s].append(subnormals(xp[:, :1] if mono else xp))
                gd = GDbg.from_buffer_copy(raw[(s * F + f) * C.sizeof(GDbg):(s * F + f + 1) * C.sizeof(GDbg)].tobytes())
                ggr = np.array(gd.gr).reshape(2, 2, 24)
                for igr in range(2):
                    g = 2 * f + igr
                    bt = int(d.block_type[igr])
                    self.seen_bt.add(bt)
                    assert btg[s, g] == bt, ("block type",) + where(igr)
                    if g == 0 and self.last_bt[s] is not None:
                        self.boundary_bt.add((self.last_bt[s], bt))
                    if not self.alloc1:         # (the first-generation allocator's streams run no detector in the reference)
                        prev = int(t.attack_prev[igr])
                        assert prev in (0, 1)
                        assert list(atk[s, g, prev, :nch]) == list(oat[igr, :nch]), ("attack",) + where(igr, prev)
                    for ch in range(nch):
                        assert np.array_equal(bits(xr[s, g, ch]), bits(xp[igr, ch])), ("mdct",) + where(igr, ch, bt)
                        if bt != 2:     # the long model's partition tables
                            assert np.array_equal(bits(etab[s, g, ch, :np2]), bits(oe[igr, ch, :np2])), ("etab",) + where(igr, ch)
                            assert np.array_equal(bits(thr[s, g, ch, :np2]), bits(ot[igr, ch, :np2])), ("thr",) + where(igr, ch)
                        else:           # the short model: spread sums [12 * w + sfb], nothing else
                            gts = thr[s, g, ch, :36].reshape(3, 12)
                            assert np.array_equal(bits(gts[:, :mpart]), bits(ots[igr, ch, :, :mpart])), ("thr short",) + where(igr, ch)
                            assert not bits(gts[:, mpart:]).any() and not bits(thr[s, g, ch, 36:]).any(), ("thr short tail",) + where(igr, ch)
                            assert not bits(etab[s, g, ch]).any(), ("etab short",) + where(igr, ch)
                            # ... and the masks after pre-echo control, from the GPU's sums and the GPU's carried memory: the one the
                            # call started with (k_msscan's hand-over) or window 2 of the granule before
                            prev_bt = self.last_bt[s] if g == 0 else int(btg[s, g - 1])
                            carry = thrprev[s, ch, :12] if g == 0 else np.float32(2.0) * thr[s, g - 1, ch, 24:36]
                            gm = short_masks(thr[s, g, ch, :36], mpart, prev_bt == 2, carry)
                            assert np.array_equal(bits(gm), bits(oms[igr, ch, :, :mpart])), ("mask short",) + where(igr, ch, prev_bt)
                    # (the front end's stages before K6's, so that a mismatch names the earliest stage it shows at)
                    if bt == 2:
                        self.short_granules[s] += 1
                        self.last_thr[s] = None
                    else:
                        if bt != 3 and self.last_thr[s] is not None:       # which branches of the clamp this granule takes (oracle's taps alone)
                            tk, fl = preecho_branches(ot[igr, :nch, :np2], np.float32(2.0) * self.last_thr[s])
                            self.clamp_taken += tk > 0
                            self.clamp_floor += fl > 0
                            self.clamp_first += tk > 0 and g == 0
                        self.last_thr[s] = ot[igr, :nch, :np2].copy()
                        if not self.alloc1:
                            band = GBand.from_buffer_copy(braw[s, g].tobytes())
                            self._prep(where(igr), t, igr, xp, xmag[s, g], x34[s, g], band)
                    self.last_bt[s] = bt
                    for ch in range(nch):
                        # what K6 hands to k_pack: the quantised lines of the coded range and the signs of the non-zero ones
                        n = 2 * int(ggr[igr, ch, 1]) + 4 * max(int(ggr[igr, ch, 18]), 0) if ggr[igr, ch, 20] else 0
                        assert np.array_equal(ixq[s, g, ch, :n], oix[igr, ch, :n]), ("ix",) + where(igr, ch, bt)
                        nz = oix[igr, ch, :n] != 0
                        assert np.array_equal(sgn[s, g, ch, :n][nz], osg[igr, ch, :n][nz]), ("signs",) + where(igr, ch, bt)
                        assert np.array_equal(ggr[igr, ch], ogr[igr, ch, :24]), ("side info",) + where(igr, ch, bt)
                if self.taps != "full":
                    self.sub_sb[s].append(0)
                    if self.alloc_state:        # (at the MPEG-2 rates both records hold the block's second frame)
                        assert gd.byte_pool == d.byte_pool and gd.main_bytes == d.main_bytes, ("reservoir",) + where(gd.byte_pool, d.byte_pool, gd.main_bytes, d.main_bytes)
                        if not self.alloc1:
                            assert gd.MNR_after == d.MNR_after, ("MNR",) + where(gd.MNR_after, d.MNR_after)
                        gsf, osf = np.array(gd.sf).reshape(2, 2, 22), np.array(d.sf).reshape(2, 2, 22)
                        for igr in range(2):
                            if d.block_type[igr] != 2:
                                for ch in range(nch):
                                    if ogr[igr, ch, 20]:        # (a granule coded as nothing carries no scalefactors)
                                        assert np.array_equal(gsf[igr, ch, :21], osf[igr, ch, :21]), ("scalefactors",) + where(igr, ch)
                    continue
                sn = np.array(d.sample_new).reshape(2, 2, 576)
                self.sub_sb[s].append(subnormals(sn))
                for igr in range(2):
                    g = 2 * f + igr
                    for ch in range(2):
                        assert np.array_equal(bits(sb[s, ch, 3 + g]), bits(sn[igr, ch])), ("polyphase",) + where(igr, ch)
                assert gd.ms == d.ms and list(gd.ms_metric) == list(d.ms_metric), where()
                assert gd.byte_pool == d.byte_pool and gd.MNR_after == d.MNR_after and gd.main_bytes == d.main_bytes, where()
                if d.block_type[0] != 2 and d.block_type[1] != 2:
                    assert np.array_equal(np.array(gd.sf), np.array(d.sf)), where()
                    assert list(gd.scfsi) == list(d.scfsi), where()
                elif self.alloc_state:      # a frame with a short granule: the scalefactors of its long (start / stop) granule
                    gsf, osf = np.array(gd.sf).reshape(2, 2, 22), np.array(d.sf).reshape(2, 2, 22)
                    for igr in range(2):
                        if d.block_type[igr] != 2:
                            for ch in range(2):
                                if ogr[igr, ch, 20]:
                                    assert np.array_equal(gsf[igr, ch, :21], osf[igr, ch, :21]), ("scalefactors",) + where(igr, ch)
            assert got[s] == b"".join(out), ("bytes", s, self.frames[s])
            self.got[s] += got[s]
            self.frames[s] += cnt[s]
