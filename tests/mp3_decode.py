"""An MPEG-1 Layer III decoder for what this encoder writes (test infrastructure only; nothing of the product imports it).

Written from ISO/IEC 11172-3: header and side information, main data through main_data_begin across frames, scalefactors
with scfsi, Huffman decode of the big values (linbits) and both count1 tables, then requantisation, M/S, reorder of short
blocks, alias reduction, IMDCT with the four windows, overlap-add, frequency inversion and polyphase synthesis, everything
in float64 and in the direct O(N^2) forms of the standard's formulas.  The output is neither clipped nor rounded.

Not covered, because the encoder never writes them: MPEG-2 rates, CRC protection, mixed blocks, intensity stereo.

The code tables come from the oracle (oracle.huff_tables()).  The 512-tap window is Table C.1 of the standard put back
together from the oracle's table of ISO constants, which holds it in the analysis bank's own layout (per-tap weights with
the fold's signs; taps n % 64 != 16 at half scale, taps n % 64 == 48 absent because their cosine term is zero): the
magnitudes come from that table and the prototype's symmetry h[n] = h[512 - n], the prototype's sign from its six zero
crossings (a main lobe of 111 taps, side lobes alternating), and C[n] = (-1)^(n >> 6) h[n], C[256] = 0.035780907.  The
synthesis window is D[n] = 32 C[n].  tests/test_recon_cases.py holds the result to the bank's own property: analysis with
C followed by synthesis with D gives the input back, 481 samples late.
The standard's banks work on samples in [-1, 1): the output is scaled by 32768 to int16 scale, as the encoder's input is.
"""
import os
import re

import numpy as np

BITRATES = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
SAMPRATES = [44100, 48000, 32000]
SFB_LONG = {
    44100: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576],
    48000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 42, 50, 60, 72, 88, 106, 128, 156, 190, 230, 276, 330, 384, 576],
    32000: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 54, 66, 82, 102, 126, 156, 194, 240, 296, 364, 448, 550, 576]}
SFB_SHORT = {
    44100: [0, 4, 8, 12, 16, 22, 30, 40, 52, 66, 84, 106, 136, 192],
    48000: [0, 4, 8, 12, 16, 22, 28, 38, 50, 64, 80, 100, 126, 192],
    32000: [0, 4, 8, 12, 16, 22, 30, 42, 58, 78, 104, 138, 180, 192]}
SLEN1 = [0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
SLEN2 = [0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3]
PRETAB = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2, 0]
ZERO_CROSSINGS = [85.5, 143.5, 200.5, 311.5, 368.5, 426.5]        # of the prototype low-pass h[n], n = 0 .. 511
ALIAS_C = [-0.6, -0.535, -0.33, -0.185, -0.095, -0.041, -0.0142, -0.0037]
SIDE_FIELDS = ["part2_3_length", "big_values", "global_gain", "scalefac_compress", "window_switching_flag", "block_type",
               "mixed_block_flag", "table_select", "subblock_gain", "region0_count", "region1_count", "preflag",
               "scalefac_scale", "count1table_select"]


def _window_d():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "hxo_iso_data.inc")
    text = open(path).read()
    body = re.search(r"HX_ANWIN_BITS\[512\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    v = np.array([int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]+", body)], dtype=np.uint32).view(np.float32).astype(np.float64)
    assert v.size == 512
    n = np.arange(512)
    h = 2.0 * np.abs(v)
    h[n % 64 == 16] = np.abs(v[n % 64 == 16])
    h[n % 64 == 48] = h[512 - n[n % 64 == 48]]
    assert abs(h[256] - 0.035780907) < 1e-8 and np.abs(h[1:] - h[:0:-1]).max() < 1e-9
    lobe = np.searchsorted(np.array(ZERO_CROSSINGS), n)         # 0: the outermost lobe on the left ... 3: the main lobe ... 6
    h *= np.where(lobe % 2 == 1, 1.0, -1.0)
    return 32.0 * h * np.where((n >> 6) & 1, -1.0, 1.0)


def _tables():
    i36, k18 = np.arange(36)[:, None], np.arange(18)[None, :]
    cos36 = np.cos(np.pi / 72.0 * (2 * i36 + 1 + 18) * (2 * k18 + 1))
    i12, k6 = np.arange(12)[:, None], np.arange(6)[None, :]
    cos12 = np.cos(np.pi / 24.0 * (2 * i12 + 1 + 6) * (2 * k6 + 1))
    i = np.arange(36)
    win = np.zeros((4, 36))
    win[0] = np.sin(np.pi / 36.0 * (i + 0.5))
    win[1, :18] = win[0, :18]
    win[1, 18:24] = 1.0
    win[1, 24:30] = np.sin(np.pi / 12.0 * (i[24:30] - 18 + 0.5))
    win[3, 6:12] = np.sin(np.pi / 12.0 * (i[6:12] - 6 + 0.5))
    win[3, 12:18] = 1.0
    win[3, 18:] = win[0, 18:]
    win[2, :12] = np.sin(np.pi / 12.0 * (i[:12] + 0.5))
    c = np.array(ALIAS_C)
    cs, ca = 1.0 / np.sqrt(1.0 + c * c), c / np.sqrt(1.0 + c * c)
    vi, vk = np.arange(64)[:, None], np.arange(32)[None, :]
    matrix = np.cos((16 + vi) * (2 * vk + 1) * np.pi / 64.0)
    return cos36, cos12, win, cs, ca, matrix, _window_d()


class _Bits:
    def __init__(self, data, pos=0):
        self.d, self.pos = data, pos

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


class Decoder:
    """feed(bytes) decodes every complete frame; frames: one dict per frame (header and side information, per granule
    and channel the decoded lines `ix`, `sign`, `sf` and `huff_end` = the bit the Huffman decode stopped at, counted like
    part2_3_length), pcm: one [1152, nch] float64 array per frame.

    The back half can be driven without a bitstream (huff=None; tests/recon_granule_cases.py): back_half(info) takes a
    frame's dict with "samprate", "nch", "ms" and per granule and channel "ix", "sign", "sf", "global_gain",
    "subblock_gain", "scalefac_scale", "preflag" and "block_type", tail / vhist may be seeded, and with taps = [] every
    granule-channel's hybrid output [18][32] is appended to it.  magnitude=True makes the second pass of that module: the
    same formulas with every operand, table entry and partial product replaced by its absolute value and every subtraction
    by an addition - what a forward error bound of the sums of products is taken of."""

    def __init__(self, huff, magnitude=False):
        self.cos36, self.cos12, self.win, self.cs, self.ca, self.matrix, self.D = _tables()
        self.mag, self.taps = bool(magnitude), None
        if self.mag:
            self.cos36, self.cos12, self.ca, self.matrix, self.D = (np.abs(t) for t in (self.cos36, self.cos12, self.ca, self.matrix, self.D))
        self.dec = {}
        for (t, x, y), ln in (huff["len"].items() if huff else ()):
            if ln > 0:
                self.dec.setdefault(t, {})[(ln, huff["code"][t, x, y])] = (x, y)
        self.linbits = huff["linbits"] if huff else None
        self.quada = {(ln, code): v for v, (code, ln) in enumerate(huff["quada"])} if huff else {}
        self.buf = b""
        self.main = bytearray()
        self.tail = np.zeros((2, 32, 18))
        self.vhist = np.zeros((2, 15, 64))      # the 15 previous matrixed vectors, newest first
        self.frames, self.pcm = [], []

    # ---- front half ----
    def feed(self, data):
        self.buf += bytes(data)
        while len(self.buf) >= 4:
            b = self.buf
            assert b[0] == 0xFF and (b[1] & 0xFE) == 0xFA, "no MPEG-1 Layer III header without CRC: %02x %02x" % (b[0], b[1])
            br, sr = BITRATES[b[2] >> 4], SAMPRATES[(b[2] >> 2) & 3]
            size = 144000 * br // sr + ((b[2] >> 1) & 1)
            if len(b) < size:
                break
            self._frame(b[:size], br, sr)
            self.buf = b[size:]
        return self

    def _frame(self, fr, br, sr):
        mode, mode_ext = fr[3] >> 6, (fr[3] >> 4) & 3
        nch = 1 if mode == 3 else 2
        side = 17 if nch == 1 else 32
        s = _Bits(fr, 32)
        info = {"bitrate": br, "samprate": sr, "mode": mode, "mode_ext": mode_ext, "nch": nch, "bytes": len(fr),
                "ms": int(mode == 1 and (mode_ext & 2) != 0), "main_data_begin": s.get(9)}
        s.get(5 if nch == 1 else 3)
        info["scfsi"] = [[s.get(1) for _ in range(4)] for _ in range(nch)]
        info["gr"] = [[None] * nch for _ in range(2)]
        for g in range(2):
            for ch in range(nch):
                q = {"part2_3_length": s.get(12), "big_values": s.get(9), "global_gain": s.get(8), "scalefac_compress": s.get(4),
                     "window_switching_flag": s.get(1), "block_type": 0, "mixed_block_flag": 0, "subblock_gain": [0, 0, 0]}
                if q["window_switching_flag"]:
                    q["block_type"], q["mixed_block_flag"] = s.get(2), s.get(1)
                    q["table_select"] = [s.get(5), s.get(5), 0]
                    q["subblock_gain"] = [s.get(3), s.get(3), s.get(3)]
                    q["region0_count"] = 8 if (q["block_type"] == 2 and not q["mixed_block_flag"]) else 7
                    q["region1_count"] = 20 - q["region0_count"]
                    assert q["block_type"] != 0 and not q["mixed_block_flag"]
                else:
                    q["table_select"] = [s.get(5), s.get(5), s.get(5)]
                    q["region0_count"], q["region1_count"] = s.get(4), s.get(3)
                q["preflag"], q["scalefac_scale"], q["count1table_select"] = s.get(1), s.get(1), s.get(1)
                info["gr"][g][ch] = q
        assert s.pos == 8 * (4 + side)
        # main data: this frame's begins main_data_begin bytes before the end of what earlier frames brought
        start = len(self.main) - info["main_data_begin"]
        self.main += fr[4 + side:]
        info["decodable"] = start >= 0
        if start < 0:       # (a stream cut at its head: the frame cannot be decoded, the decoder outputs silence)
            self.frames.append(info)
            self.pcm.append(np.zeros((1152, nch)))
            return
        m = _Bits(self.main, 8 * start)
        for g in range(2):
            for ch in range(nch):
                self._granule(m, info, g, ch)
        if len(self.main) > 4096:       # (main_data_begin reaches back 511 bytes at the most)
            self.main = self.main[-2048:]
        self.frames.append(info)
        self.pcm.append(self._back_half(info))

    def _granule(self, m, info, g, ch):
        q, sr = info["gr"][g][ch], info["samprate"]
        p0 = m.pos
        end = p0 + q["part2_3_length"]
        s1, s2 = SLEN1[q["scalefac_compress"]], SLEN2[q["scalefac_compress"]]
        if q["block_type"] == 2:
            sf = [[m.get(s1 if b < 6 else s2) for _ in range(3)] for b in range(12)] + [[0, 0, 0]]     # [sfb][window]
        else:
            sf = [0] * 22
            for b in range(21):
                grp = 0 if b < 6 else 1 if b < 11 else 2 if b < 16 else 3
                if g == 1 and info["scfsi"][ch][grp]:
                    sf[b] = info["gr"][0][ch]["sf"][b]
                else:
                    sf[b] = m.get(s1 if b < 11 else s2)
        q["sf"] = sf
        ix, sign = np.zeros(576, dtype=np.int64), np.zeros(576, dtype=np.int64)
        nbig = 2 * q["big_values"]
        assert nbig <= 576
        if q["window_switching_flag"]:
            r1, r2 = (36 if q["block_type"] == 2 else SFB_LONG[sr][8]), 576
        else:
            r1 = SFB_LONG[sr][q["region0_count"] + 1]
            r2 = SFB_LONG[sr][min(q["region0_count"] + q["region1_count"] + 2, 22)]
        q["linbits_used"] = False
        i = 0
        while i < nbig:
            t = q["table_select"][0 if i < r1 else 1 if i < r2 else 2]
            x = y = 0
            if t:
                ln = code = 0
                tab = self.dec[t]
                while (ln, code) not in tab:
                    code = (code << 1) | m.get(1)
                    ln += 1
                    assert ln <= 19, "no code word of table %d" % t
                x, y = tab[ln, code]
                lb = self.linbits[t]
                if lb and x == 15:
                    x += m.get(lb)
                    q["linbits_used"] = True
                if x:
                    sign[i] = m.get(1)
                if lb and y == 15:
                    y += m.get(lb)
                    q["linbits_used"] = True
                if y:
                    sign[i + 1] = m.get(1)
            ix[i], ix[i + 1] = x, y
            i += 2
        nquads = 0
        while m.pos < end and i <= 572:
            if q["count1table_select"]:
                v = 15 - m.get(4)
            else:
                ln = code = 0
                while (ln, code) not in self.quada:
                    code = (code << 1) | m.get(1)
                    ln += 1
                    assert ln <= 6
                v = self.quada[ln, code]
            for k in range(4):
                if (v >> (3 - k)) & 1:
                    ix[i + k] = 1
                    sign[i + k] = m.get(1)
            i += 4
            nquads += 1
        q["ix"], q["sign"], q["nquads"], q["huff_end"] = ix, sign, nquads, m.pos - p0
        m.pos = end

    # ---- back half ----
    def _requantise(self, info, g, ch):
        q, sr = info["gr"][g][ch], info["samprate"]
        mag = q["ix"].astype(np.float64) ** (4.0 / 3.0) * (1.0 if self.mag else np.where(q["sign"], -1.0, 1.0))
        mult = 1.0 if q["scalefac_scale"] else 0.5
        if q["block_type"] == 2:        # bitstream order: band, window, line; out: [window][line of the window]
            xs = np.zeros((3, 192))
            bs, j = SFB_SHORT[sr], 0
            for b in range(13):
                wd = bs[b + 1] - bs[b]
                for w in range(3):
                    e = 0.25 * (q["global_gain"] - 210 - 8 * q["subblock_gain"][w]) - mult * q["sf"][b][w]
                    xs[w, bs[b]:bs[b + 1]] = mag[j:j + wd] * 2.0 ** e
                    j += wd
            return xs
        xr = np.zeros(576)
        bl = SFB_LONG[sr]
        for b in range(22):
            e = 0.25 * (q["global_gain"] - 210) - mult * (q["sf"][b] + q["preflag"] * PRETAB[b])
            xr[bl[b]:bl[b + 1]] = mag[bl[b]:bl[b + 1]] * 2.0 ** e
        return xr

    def _hybrid(self, x, bt, ch):
        """one granule's 576 requantised lines of a channel -> [18 time slots][32 subbands]"""
        out = np.zeros((32, 36))
        if bt == 2:
            for w in range(3):
                y = (x[w].reshape(32, 6) @ self.cos12.T) * self.win[2, :12]
                out[:, 6 + 6 * w:18 + 6 * w] += y
        else:
            x = x.copy()
            for sb in range(1, 32):
                lo, hi = x[18 * sb - 1 - np.arange(8)].copy(), x[18 * sb + np.arange(8)].copy()
                if self.mag:        # (ca holds magnitudes here)
                    x[18 * sb - 1 - np.arange(8)] = lo * self.cs + hi * self.ca
                    x[18 * sb + np.arange(8)] = hi * self.cs + lo * self.ca
                    continue
                x[18 * sb - 1 - np.arange(8)] = lo * self.cs - hi * self.ca
                x[18 * sb + np.arange(8)] = hi * self.cs + lo * self.ca
            out = (x.reshape(32, 18) @ self.cos36.T) * self.win[bt]
        res = out[:, :18] + self.tail[ch]
        self.tail[ch] = out[:, 18:]
        if not self.mag:
            res[1::2, 1::2] *= -1.0
        return res.T

    def _synth(self, sb, ch):
        """[18][32] subband samples -> 576 samples"""
        v = np.concatenate([(sb @ self.matrix.T)[::-1], self.vhist[ch]])      # newest first: slot 17 ... slot 0, then history
        pcm = np.zeros((18, 32))
        for t in range(18):
            vh = v[17 - t:17 - t + 16]
            for i in range(8):
                pcm[t] += self.D[64 * i:64 * i + 32] * vh[2 * i, :32] + self.D[64 * i + 32:64 * i + 64] * vh[2 * i + 1, 32:]
        self.vhist[ch] = v[:15]
        return pcm.reshape(576)

    def _back_half(self, info):
        nch = info["nch"]
        pcm = np.zeros((1152, nch))
        for g in range(2):
            bt = info["gr"][g][0]["block_type"]
            x = [self._requantise(info, g, ch) for ch in range(nch)]
            if info["ms"] and self.mag:
                x = [(x[0] + x[1]) / np.sqrt(2.0), (x[0] + x[1]) / np.sqrt(2.0)]
            elif info["ms"]:
                assert info["gr"][g][1]["block_type"] == bt
                x = [(x[0] + x[1]) / np.sqrt(2.0), (x[0] - x[1]) / np.sqrt(2.0)]
            for ch in range(nch):
                hyb = self._hybrid(x[ch], info["gr"][g][ch]["block_type"], ch)
                if self.taps is not None:
                    self.taps.append(hyb)
                pcm[576 * g:576 * (g + 1), ch] = self._synth(hyb, ch)
        return 32768.0 * pcm

    back_half = _back_half


def decode(data, huff):
    """(pcm [frames * 1152, nch] float64, frames) of a whole bitstream"""
    d = Decoder(huff).feed(data)
    assert not d.buf, "%d bytes behind the last whole frame" % len(d.buf)
    return (np.concatenate(d.pcm) if d.pcm else np.zeros((0, 2))), d.frames
