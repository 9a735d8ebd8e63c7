"""ctypes bindings for the CPU oracle (oracle/liboracle.so) and, when present, the real
reference (oracle/_ref/libhmp3ref.so).  TEST INFRASTRUCTURE ONLY - see oracle/hxo.h."""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class Control(C.Structure):
    """E_CONTROL (pub/encapp.h:42-72)"""
    _fields_ = [(n, C.c_int) for n in (
        "mode", "bitrate", "samprate", "nsbstereo", "filter_select", "freq_limit", "nsb_limit",
        "layer", "cr_bit", "original", "hf_flag", "vbr_flag", "vbr_mnr", "vbr_br_limit",
        "vbr_delta_mnr", "chan_add_f0", "chan_add_f1", "sparse_scale")] + \
        [("mnr_adjust", C.c_int * 21)] + \
        [(n, C.c_int) for n in ("cpu_select", "quick", "test1", "test2", "test3", "short_block_threshold")]


def default_control(**kw):
    """CLI defaults (test/tomp3.cpp:357-384); bitrate=N (per channel) selects CBR like -B N"""
    ec = Control()
    ec.mode = 1; ec.bitrate = -1; ec.samprate = 44100; ec.nsbstereo = -1; ec.filter_select = -1
    ec.freq_limit = 24000; ec.nsb_limit = -1; ec.layer = 3; ec.cr_bit = 1; ec.original = 1
    ec.hf_flag = 0; ec.vbr_flag = 1; ec.vbr_mnr = 50; ec.vbr_br_limit = 160; ec.vbr_delta_mnr = 0
    ec.chan_add_f0 = ec.chan_add_f1 = 24000; ec.sparse_scale = -1; ec.cpu_select = 0
    ec.quick = -1; ec.test1 = -1; ec.test2 = ec.test3 = 0; ec.short_block_threshold = 700
    for k, v in kw.items():
        setattr(ec, k, v)
    if "bitrate" in kw and kw["bitrate"] > 0 and "vbr_flag" not in kw:
        ec.vbr_flag = 0
    return ec


def _load(path):
    return C.CDLL(path) if os.path.exists(path) else None


_lib = None
_ref = None
_ref_zero = None


def lib():
    global _lib
    if _lib is None:
        p = os.path.join(HERE, "liboracle.so")
        if not os.path.exists(p):
            raise RuntimeError("oracle/liboracle.so missing: run `make -C oracle`")
        _lib = C.CDLL(p)
        _lib.hxo_new.restype = C.c_void_p
        _lib.hxo_free.argtypes = [C.c_void_p]
        _lib.hxo_init.argtypes = [C.c_void_p, C.POINTER(Control)]
        _lib.hxo_encode_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.hxo_encode_frame_s16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.hxo_encode_frame_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.hxo_mblog.argtypes = [C.c_float]
        _lib.hxo_mbexp.argtypes = [C.c_int]
        _lib.hxo_mbexp.restype = C.c_float
        _lib.hxo_frames_out.argtypes = [C.c_void_p]
        _lib.hxo_frames_out.restype = C.c_uint
        _lib.hxo_bytes_out.argtypes = [C.c_void_p]
        _lib.hxo_bytes_out.restype = C.c_uint
        _lib.hxo_range_counts_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.hxo_range_counts_get.restype = None
        _lib.hxo_stream_kind.argtypes = [C.c_void_p]
        _lib.hxo_stream_kind.restype = C.c_int
    return _lib


def ref():
    """the real reference, or None when oracle/_ref has not been built"""
    global _ref
    if _ref is None:
        _ref = _load(os.path.join(HERE, "_ref", "libhmp3ref.so"))
        if _ref is not None:
            _ref.ref_new.restype = C.c_void_p
            _ref.ref_free.argtypes = [C.c_void_p]
            _ref.ref_init.argtypes = [C.c_void_p, C.POINTER(Control)]
            _ref.ref_init_s16.argtypes = [C.c_void_p, C.POINTER(Control)]
            _ref.ref_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            _ref.ref_encode_s16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            _ref.ref_encode_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _ref.ref_encode_stream_s16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long]
            _ref.ref_encode_stream_s16.restype = C.c_long
            _ref.ref_dump.argtypes = [C.c_void_p, C.c_void_p]
            _ref.ref_frames.argtypes = [C.c_void_p]
            _ref.ref_frames.restype = C.c_uint
            if hasattr(_ref, "ref_bitrate2_float"):     # (a reference build made before the harness had the getters lacks them)
                _ref.ref_bitrate2_float.argtypes = _ref.ref_bitrate_float.argtypes = _ref.ref_bitrate.argtypes = [C.c_void_p]
                _ref.ref_bitrate2_float.restype = _ref.ref_bitrate_float.restype = C.c_float
            _ref.ref_mbLogC.argtypes = [C.c_float]
            _ref.ref_mbExp.argtypes = [C.c_int]
            _ref.ref_mbExp.restype = C.c_float
    return _ref


def ref_zero():
    """the reference compiled with every uninitialised local defined as zero (make -C oracle ref_zero), or None"""
    global _ref_zero
    if _ref_zero is None:
        _ref_zero = _load(os.path.join(HERE, "_ref", "libhmp3ref_zero.so"))
        if _ref_zero is not None:
            _ref_zero.ref_new.restype = C.c_void_p
            _ref_zero.ref_free.argtypes = [C.c_void_p]
            _ref_zero.ref_init.argtypes = [C.c_void_p, C.POINTER(Control)]
            _ref_zero.ref_init_s16.argtypes = [C.c_void_p, C.POINTER(Control)]
            _ref_zero.ref_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            _ref_zero.ref_encode_s16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return _ref_zero


class RefDump(C.Structure):
    _fields_ = [
        ("sample", C.c_float * (2 * 4 * 576)), ("xr", C.c_float * (2 * 2 * 576)),
        ("sig_mask", C.c_float * (2 * 36 * 2)), ("ix", C.c_int * (2 * 576)),
        ("signx", C.c_ubyte * (2 * 576)), ("sf_l", C.c_int * (2 * 2 * 23)),
        ("gr", C.c_int * (2 * 2 * 26)), ("scfsi", C.c_int * 2), ("attack_buf", C.c_int * 64),
        ("ecsave", C.c_float * 128), ("igrx", C.c_int), ("byte_pool", C.c_int), ("MNR", C.c_int),
        ("PoolFraction", C.c_int), ("call_count", C.c_int), ("ms_correlation_memory", C.c_int),
        ("NTadjust", C.c_int * 44), ("nsb_limit", C.c_int), ("nsb_limitMS", C.c_int * 2),
        ("band_limit", C.c_int), ("AveTargetBits", C.c_int), ("main_framebytes", C.c_int),
        ("initialMNR", C.c_int), ("nsf", C.c_int * 2)]


def pow43(first, n):
    """float64 [n]: pow(ix, 4/3) for ix = first .. first + n - 1 as the oracle's noise measurement calls it (this machine's libm)"""
    out = np.zeros(n, dtype=np.float64)
    lib().hxo_pow43.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib().hxo_pow43.restype = None
    lib().hxo_pow43(first, n, out.ctypes.data)
    return out


def pow34(x):
    """float32 [n]: x^(3/4) of non-negative float32 values as the allocator forms it (hxo_pow34)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros(x.shape, dtype=np.float32)
    lib().hxo_pow34.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib().hxo_pow34.restype = None
    lib().hxo_pow34(x.ctypes.data, y.ctypes.data, x.size)
    return y


MATH = {"mblog": 0, "mbexp": 1, "round": 2, "dblog": 3, "dual_g": 4}


def math(name, x):
    """uint32 [n]: the 32-bit patterns of hxo_mblog / hxo_mbexp / hxo_round / hxo_dblog / hxo_dual_g on the 32-bit patterns
    x (float32 bits; int32 for mbexp), through the C functions the oracle's encoder calls (this machine's libm)"""
    x = np.ascontiguousarray(x).reshape(-1)
    assert x.dtype.itemsize == 4
    out = np.zeros(x.size, dtype=np.uint32)
    lib().hxo_math_array.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    rc = lib().hxo_math_array(MATH[name], x.ctypes.data, x.size, out.ctypes.data)
    assert rc == 0
    return out


class OracleEncoder:
    """one stream through the restatement"""

    def __init__(self, ec):
        self.l = lib()
        self.h = self.l.hxo_new()
        self.bytes_in = self.l.hxo_init(self.h, C.byref(ec))
        self.out = (C.c_ubyte * 16384)()

    def ok(self):
        return self.bytes_in != 0

    def encode_s16(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.int16)
        n = self.l.hxo_encode_frame_s16(self.h, frame.ctypes.data, self.out)
        return bytes(self.out[:n])

    def encode_f32(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        n = self.l.hxo_encode_frame(self.h, frame.ctypes.data, self.out)
        return bytes(self.out[:n])

    def encode_packet(self, frame):
        """-> (bitstream bytes, reformatted packet bytes) of L3_audio_encode_Packet"""
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        pk = (C.c_ubyte * 4096)()
        nb = (C.c_int * 2)()
        n = self.l.hxo_encode_frame_packet(self.h, frame.ctypes.data, self.out, pk, nb)
        self.packet_sizes = (nb[0], nb[1])      # MPEG-2: two single-granule packets back to back
        return bytes(self.out[:n]), bytes(pk[:nb[0] + nb[1]])

    def frames_out(self):
        """frames emitted so far (L3_audio_encode_get_frames)"""
        return int(self.l.hxo_frames_out(self.h))

    def bytes_out(self):
        """bytes emitted so far"""
        return int(self.l.hxo_bytes_out(self.h))

    def range_counts(self, short_blocks=False):
        """what the noise measurement of the long-block (or short-block) allocator met beyond the 256-entry float table of
        ix^(4/3) so far: {"beyond_table": lines dequantised through pow(), "from_16384": those quantised to 16384 or more
        (past the kernels' double table, HX_POW43_N), "max_qx": the largest quantised value}"""
        v = (C.c_longlong * 3)()
        self.l.hxo_range_counts_get(self.h, 1 if short_blocks else 0, v)
        return {"beyond_table": int(v[0]), "from_16384": int(v[1]), "max_qx": int(v[2])}

    def __del__(self):
        try:
            self.l.hxo_free(self.h)
        except Exception:
            pass


class RefEncoder:
    """one stream through the real reference (None-safe: check oracle.ref() first)"""

    def __init__(self, ec, s16=True, zero_locals=False):
        self.r = ref_zero() if zero_locals else ref()
        self.h = self.r.ref_new()
        self.s16 = s16
        self.bytes_in = (self.r.ref_init_s16 if s16 else self.r.ref_init)(self.h, C.byref(ec))
        self.out = (C.c_ubyte * 16384)()

    def encode_s16(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.int16)
        n = self.r.ref_encode_s16(self.h, frame.ctypes.data, self.out)
        return bytes(self.out[:n])

    def encode_f32(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        n = self.r.ref_encode(self.h, frame.ctypes.data, self.out)
        return bytes(self.out[:n])

    def encode_packet(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        pk = (C.c_ubyte * 4096)()
        nb = (C.c_int * 2)()
        n = self.r.ref_encode_packet(self.h, frame.ctypes.data, self.out, pk, nb)
        self.packet_sizes = (nb[0], nb[1])
        return bytes(self.out[:n]), bytes(pk[:nb[0] + nb[1]])

    def frames(self):
        """L3_audio_encode_get_frames"""
        return int(self.r.ref_frames(self.h))

    def bitrates(self):
        """(L3_audio_encode_get_bitrate2_float, _get_bitrate_float as float32, _get_bitrate)"""
        return np.float32(self.r.ref_bitrate2_float(self.h)), np.float32(self.r.ref_bitrate_float(self.h)), int(self.r.ref_bitrate(self.h))

    def dump(self):
        d = RefDump()
        self.r.ref_dump(self.h, C.byref(d))
        return d

    def __del__(self):
        try:
            self.r.ref_free(self.h)
        except Exception:
            pass


def encode_stream(enc, pcm_i16, flush_frames=2):
    """encode [n*1152, 2] int16 through enc, then feed zero frames; returns bytes"""
    nfr = pcm_i16.shape[0] // 1152
    out = []
    for f in range(nfr):
        out.append(enc.encode_s16(pcm_i16[f * 1152:(f + 1) * 1152]))
    z = np.zeros((1152, 2), dtype=np.int16)
    for _ in range(flush_frames):
        out.append(enc.encode_s16(z))
    return b"".join(out)


GR_FIELDS = ["part2_3_length", "big_values", "global_gain", "scalefac_compress", "window_switching_flag",
             "block_type", "mixed_block_flag", "table_select0", "table_select1", "table_select2",
             "subblock_gain0", "subblock_gain1", "subblock_gain2", "region0_count", "region1_count",
             "preflag", "scalefac_scale", "count1table_select", "aux_nquads", "aux_bits", "aux_not_null",
             "aux_nreg0", "aux_nreg1", "aux_nreg2"]


class FrameDebug(C.Structure):
    """hxo_frame_debug (oracle/hxo.h)"""
    _fields_ = [
        ("sample_new", C.c_float * (2 * 2 * 576)), ("xr_pre", C.c_float * (2 * 2 * 576)),
        ("etab", C.c_float * (2 * 2 * 64)), ("thr", C.c_float * (2 * 2 * 64)), ("mask", C.c_float * (2 * 2 * 22)),
        ("block_type", C.c_int * 2), ("attack", C.c_int * 4),
        ("ms", C.c_int), ("ms_metric", C.c_int * 2), ("byte_pool", C.c_int), ("MNR_after", C.c_int),
        ("gr", C.c_int * (2 * 2 * 27)), ("sf", C.c_int * (2 * 2 * 22)), ("ix", C.c_int * (2 * 2 * 576)),
        ("signx", C.c_ubyte * (2 * 2 * 576)), ("scfsi", C.c_int * 2), ("main_bytes", C.c_int)]


class StageTaps(C.Structure):
    """hxo_stage_taps (oracle/hxo.h): the taps beside FrameDebug, a record of their own"""
    _fields_ = [
        # short granules [gr][ch][12 * w + sfb]: spread sums before pre-echo control, masks after it
        ("thr_short", C.c_float * (2 * 2 * 36)), ("mask_short", C.c_float * (2 * 2 * 36)),
        # start values of the long-block allocator [gr][ch][sfb], and how many bands of each were formed [gr][ch]
        ("xsxx", C.c_float * (2 * 2 * 22)), ("x34max", C.c_float * (2 * 2 * 22)), ("gzero", C.c_int * (2 * 2 * 22)),
        ("noise0", C.c_int * (2 * 2 * 22)), ("noise0_ms", C.c_int * (2 * 2 * 22)), ("mask_mb", C.c_int * (2 * 2 * 22)),
        ("nb_x", C.c_int * 4), ("nb_e", C.c_int * 4), ("nb_z", C.c_int * 4),
        ("start_ms", C.c_int * 2), ("attack_prev", C.c_int * 2)]


def oracle_enable_debug(enc):
    """attach a FrameDebug record to an OracleEncoder; returns it (refilled on every frame)"""
    l = lib()
    l.hxo_sizeof_frame_debug.restype = C.c_int
    assert l.hxo_sizeof_frame_debug() == C.sizeof(FrameDebug), (l.hxo_sizeof_frame_debug(), C.sizeof(FrameDebug))
    d = FrameDebug()
    l.hxo_set_debug.argtypes = [C.c_void_p, C.c_void_p]
    l.hxo_set_debug(enc.h, C.byref(d))
    enc._dbg = d
    return d


def oracle_enable_stage_taps(enc):
    """attach a StageTaps record to an OracleEncoder; returns it (refilled on every frame)"""
    l = lib()
    l.hxo_sizeof_stage_taps.restype = C.c_int
    assert l.hxo_sizeof_stage_taps() == C.sizeof(StageTaps), (l.hxo_sizeof_stage_taps(), C.sizeof(StageTaps))
    t = StageTaps()
    l.hxo_set_stage_taps.argtypes = [C.c_void_p, C.c_void_p]
    l.hxo_set_stage_taps(enc.h, C.byref(t))
    enc._taps = t
    return t


# Path census (oracle/hxo_int.h, HXO_PATHS): the names of hxo_path_counts, in its order.  Not part of the encoder.
# L_ long allocator, S_ short allocator, A_ first-generation allocator, H_ Huffman pick per coded channel-granule,
# D_ frame driver; H_tab0 .. H_tab31 (a region of one or more pairs coded with that table) follow.
PATH_NAMES = """
    L_inc_ms L_inc_lr L_inc_hf L_inc_first L_inc_several L_inc_cap L_inc_gmin_hold L_inc_stepback L_dec_ms L_dec_lr
    L_dec_one L_dec_several L_dec_cap L_dec_delta_floor L_dec_delta_formula L_dec_after_stepback L_lim_max
    L_lim_max_several L_lim_p23_one L_lim_p23_both L_lim_after_dec_cap L_isf2_refined L_isf2_clamp_up
    L_isf2_clamp_lo L_fb_dmnr_raised L_fb_dmnr_cut L_fb_mnr_cap L_fb_reset L_bt1_adjust L_bt3_adjust
    L_short_mnr0_cbr L_short_mnr0_vbr S_inc_enter S_inc_first S_inc_several S_inc_cap S_dec_enter S_dec_first
    S_dec_several S_dec_cap S_lim_enter S_lim_first S_lim_several S_lim_cap S_p23_enter S_p23_first S_p23_several
    S_p23_cap S_mnr_raise S_only_over_skip A_seek1_dsf0 A_seek1_dsf2 A_seek1_four A_seek2_dsf0 A_seek2_dsf2
    A_seek2_four A_minbits_corr A_more_enter A_more_gz A_more_three A_back_enter A_back_several A_back_gg100
    H_count1_a H_count1_b H_escape H_bigv_limit H_empty_region H_no_bigv D_pool_cap_stuffing D_cbr_padding_slot
    D_vbr_ibr_min D_vbr_ibr_max D_vbr_pool_step D_vbr_limit_cut D_ms_frame D_lr_frame D_scfsi_shared D_no_frame_out
    D_two_frames_out D_lsf_bitmin_40 D_lsf_vbr_span10 D_lsf_vbr_span16 D_lsf_vbr_span25
""".split() + ["H_tab%d" % t for t in range(32)]
HUFF_TABLES = [t for t in range(32) if t not in (4, 14)]        # the format's 30 big-value table indices


def path_counts():
    """{name: count}: the branches every oracle encoder of this process has taken so far (hxo_path_counts)"""
    l = lib()
    l.hxo_path_count_n.restype = C.c_int
    l.hxo_path_count_names.restype = C.c_char_p
    assert l.hxo_path_count_n() == len(PATH_NAMES)
    assert l.hxo_path_count_names().decode().split() == PATH_NAMES[:-32]
    v = (C.c_longlong * len(PATH_NAMES)).in_dll(l, "hxo_path_counts")
    return dict(zip(PATH_NAMES, (int(x) for x in v)))


def path_counts_since(before):
    """{name: count} of the entries counted since `before` (an earlier path_counts()), zero ones left out"""
    now = path_counts()
    return {k: now[k] - before[k] for k in PATH_NAMES if now[k] != before[k]}


# ---- the bit writer on a list of segments (hxo_pack_frame, oracle/hxo.h; ref_pack_frame, oracle/ref_harness.cpp) ----
# A segment is a plain record (tests/pack_cases.py): "fields" 40 entries in transmission order, None or (value, length),
# "not_null", "pairs" (n0, n1, n2), "tables" (t0, t1, t2), "c1", "quads", "ix" and "sign" of 576 lines each.
def _pack_frame_args(segs):
    n = len(segs)
    hdr = np.zeros((n, 9), np.int32)
    val = np.zeros((n, 40), np.int32)
    ln = np.full((n, 40), -1, np.int32)
    ix = np.zeros((n, 576), np.int32)
    sg = np.zeros((n, 576), np.uint8)
    for i, s in enumerate(segs):
        hdr[i] = [s["not_null"], *s["pairs"], s["quads"], *s["tables"], s["c1"]]
        for j, f in enumerate(s["fields"]):
            if f is not None:
                val[i, j], ln[i, j] = f
        ix[i] = s["ix"]
        sg[i] = s["sign"]
    return n, hdr, val, ln, ix, sg


def ref_has_pack_frame():
    """whether the reference build at hand was made with ref_pack_frame in its harness"""
    return ref() is not None and hasattr(ref(), "ref_pack_frame")


def ref_has_getters():
    """whether the reference build at hand was made with the bitrate getters in its harness"""
    return ref() is not None and hasattr(ref(), "ref_bitrate2_float")


def _ref_pack_frame_direct(n, hdr, val, ln, ix, sg, out, bits):
    """ref_pack_frame's steps (oracle/ref_harness.cpp) made from here, on the writer functions every reference build
    exports - L3_outbits_init, L3_outbits, L3_pack_huff, L3_outbits_flush: a machine that has no reference sources runs the
    oracle/_ref it was handed, which may have been made before the harness had ref_pack_frame.  GR (pub/l3e.h:72-96) as 27
    ints: big_values [1], table_select [7..9], count1table_select [17], aux_nquads [18], aux_nreg [21..23]."""
    r = ref()
    r.L3_outbits_init.argtypes = [C.c_void_p]
    r.L3_outbits.argtypes = [C.c_uint, C.c_int]
    r.L3_pack_huff.argtypes = [C.c_void_p] * 3
    r.L3_pack_huff.restype = r.L3_outbits_flush.restype = C.c_int
    none = (C.c_int * 27)()
    pos = lambda: r.L3_pack_huff(none, ix.ctypes.data, sg.ctypes.data)      # (codes nothing: the writer's position against a file static)
    r.L3_outbits_init(out.ctypes.data)
    for s in range(n):
        start = pos()
        for j in range(40):
            if ln[s, j] >= 0:
                r.L3_outbits(int(val[s, j]) & 0xFFFFFFFF, int(ln[s, j]))
        if hdr[s, 0]:
            g = (C.c_int * 27)()
            g[21], g[22], g[23] = (int(v) for v in hdr[s, 1:4])
            g[1], g[18] = int(hdr[s, 1:4].sum()), int(hdr[s, 4])
            g[7], g[8], g[9], g[17] = (int(v) for v in hdr[s, 5:9])
            r.L3_pack_huff(g, ix[s].ctypes.data, sg[s].ctypes.data)
        bits[s] = pos() - start
    return r.L3_outbits_flush()


def pack_frame(segs, use_ref=False, harness=None):
    """(main-data bytes, [bit length of each segment]) of one frame made of `segs`, by the oracle's writer or (use_ref) the
    reference's own: through the harness's ref_pack_frame where the reference build has it (harness: None = that rule,
    True / False = that way)"""
    n, hdr, val, ln, ix, sg = _pack_frame_args(segs)
    out = np.zeros(4 * 512 + 64, np.uint8)
    bits = np.zeros(max(n, 1), np.int32)
    if use_ref and not (ref_has_pack_frame() if harness is None else harness):
        nb = _ref_pack_frame_direct(n, hdr, val, ln, ix, sg, out, bits)
    else:
        f = ref().ref_pack_frame if use_ref else lib().hxo_pack_frame
        f.restype = C.c_int
        f.argtypes = [C.c_int] + [C.c_void_p] * 7
        nb = f(n, hdr.ctypes.data, val.ctypes.data, ln.ctypes.data, ix.ctypes.data, sg.ctypes.data, out.ctypes.data, bits.ctypes.data)
    return out[:nb].tobytes(), [int(b) for b in bits[:n]]


def huff_pair_len(t, x, y):
    """coded length of one pair in table t: code word, sign bits, linbits (hxo_huff_pair_len)"""
    return int(lib().hxo_huff_pair_len(int(t), int(x), int(y)))


# ---- the quantisers and Huffman counters on records (hxo_count_record*, oracle/hxo.h; ref_count_record*, oracle/ref_harness.cpp) ----
# The record layout is hx_debug_count's (include/hmp3_amd.h): hdr [n][16], lines [n][2][576], band maxima [n][2][22] or, of a
# short record, [n][2][3][16], x34 and gain steps likewise.  COUNT_GR: what output_subdivide2 hands on of a long channel.
COUNT_OUT = ["table0", "table1", "table2", "count1table", "cb0", "cb1", "cb2", "nbig", "nquads", "bits"]
COUNT_GR = ["table_select0", "table_select1", "table_select2", "count1table_select", "big_values", "region0_count", "region1_count",
            "aux_nreg0", "aux_nreg1", "aux_nreg2", "aux_nquads"]


class CountTables:
    """the tables of one control that the records are built on and counted with: an initialised oracle encoder's (and, with
    use_ref, a reference encoder's of the same control)"""

    def __init__(self, ec, use_ref=False):
        self.enc = OracleEncoder(ec)
        assert self.enc.ok()
        l = lib()
        l.hxo_params_of.restype = C.c_void_p
        l.hxo_params_of.argtypes = [C.c_void_p]
        self.p = l.hxo_params_of(self.enc.h)
        tl, ts = np.zeros(46, np.int32), np.zeros(28, np.int32)
        l.hxo_band_tables.argtypes = [C.c_void_p] * 3
        l.hxo_band_tables(self.p, tl.ctypes.data, ts.ctypes.data)
        self.nBand_l, self.startBand_l = tl[:22].copy(), tl[22:].copy()
        self.nBand_s, self.startBand_s, self.nsfs = ts[:13].copy(), ts[13:27].copy(), int(ts[27])
        self.ref = RefEncoder(ec) if use_ref else None
        if use_ref:
            rl, rs = np.zeros(46, np.int32), np.zeros(28, np.int32)
            ref().ref_band_tables.argtypes = [C.c_void_p] * 3
            ref().ref_band_tables(self.ref.h, rl.ctypes.data, rs.ctypes.data)
            assert (rl == tl).all() and (rs == ts).all(), "the oracle's band tables are not the reference's"

    def quant_lines(self, rule, x34, gsf, use_ref=False):
        """int32 [n]: x34 through quantiser `rule` (0 plain, 1 table offsets, 2 the same with the first offset at -0.30) at gain step gsf"""
        x = np.ascontiguousarray(x34, dtype=np.float32).copy()
        out = np.zeros(x.size, np.int32)
        if use_ref:
            f = ref().ref_quant_lines
            f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            f(int(rule), x.ctypes.data, out.ctypes.data, int(gsf), x.size)
        else:
            f = lib().hxo_quant_lines
            f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            f(self.p, int(rule), x.ctypes.data, out.ctypes.data, int(gsf), x.size)
        return out


def ref_has_count_records():
    """whether the reference build at hand was made with the quantise-and-count entries in its harness"""
    return ref() is not None and hasattr(ref(), "ref_count_record")


def count_records(tabs, mode, hdr, ix, ixmax, x34=None, gsf=None, clear_past=False, use_ref=False):
    """n records through the oracle's quantiser and counter (use_ref: the reference's own).  mode: "count", "quant" (either of
    the device's two long routes), "short", "short_count".  -> (lines, band maxima, out, sums): copies of ix and ixmax as
    the functions left them; the returned sum of every record; out [n][24] as hx_debug_count leaves it (oracle) or, from the
    reference, per channel at [.., 12 ch:] the returned bits and COUNT_GR (long) / at [.., 10 ch:] COUNT_OUT (short)."""
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    n = hdr.shape[0]
    short = mode.startswith("short")
    quant = mode in ("quant", "short")
    nb = 96 if short else 44
    ix = np.array(ix, dtype=np.int32, order="C").reshape(n, 1152)
    ixmax = np.array(ixmax, dtype=np.int32, order="C").reshape(n, nb)
    x34 = np.zeros((n, 1152), np.float32) if x34 is None else np.array(x34, dtype=np.float32, order="C").reshape(n, 1152)
    gsf = np.zeros((n, nb), np.int32) if gsf is None else np.ascontiguousarray(gsf, dtype=np.int32).reshape(n, nb)
    out = np.zeros((n, 24), np.int32)
    total = np.zeros(n, np.int32)
    V = C.c_void_p
    if use_ref:
        f = ref().ref_count_record_short if short else ref().ref_count_record
        f.argtypes = [V, C.c_int] + [V] * 6
        for r in range(n):
            total[r] = f(tabs.ref.h, int(quant), hdr[r].ctypes.data, ix[r].ctypes.data, ixmax[r].ctypes.data, x34[r].ctypes.data, gsf[r].ctypes.data, out[r].ctypes.data)
        return ix, ixmax, out, total
    elif short:
        f = lib().hxo_count_record_short
        f.argtypes = [V, C.c_int] + [V] * 6
        for r in range(n):
            f(tabs.p, int(quant), hdr[r].ctypes.data, ix[r].ctypes.data, ixmax[r].ctypes.data, x34[r].ctypes.data, gsf[r].ctypes.data, out[r].ctypes.data)
    else:
        f = lib().hxo_count_record
        f.argtypes = [V, C.c_int, C.c_int] + [V] * 6
        for r in range(n):
            f(tabs.p, int(quant), int(clear_past), hdr[r].ctypes.data, ix[r].ctypes.data, ixmax[r].ctypes.data, x34[r].ctypes.data, gsf[r].ctypes.data, out[r].ctypes.data)
    return ix, ixmax, out, out[:, 20].copy()


def ref_has_noise_records():
    """whether the reference build at hand was made with the noise-search entries in its harness"""
    return ref() is not None and hasattr(ref(), "ref_seek_record")


def noise_records(tabs, mode, hdr, xr, band, x34=None, ix=None, use_ref=False):
    """n records (the layout: hx_debug_seek, include/hmp3_amd.h) through the oracle's seek_actual (mode "seek") or inverse_sf2
    ("isf2"), or with use_ref through CBitAllo3::noise_seek_actual / inverse_sf2 -> out [n][184]: per (channel, band) four
    words as hx_debug_seek leaves them - the reference fills gsf, Noise, NTadjust / sf only - and from the oracle at [178:181]
    what the record reached (hxo_seek_record)"""
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    n = hdr.shape[0]
    xr = np.array(xr, dtype=np.float32, order="C").reshape(n, 1152)
    band = np.ascontiguousarray(band, dtype=np.int32).reshape(n, 352)
    other = np.array(x34, dtype=np.float32, order="C").reshape(n, 1152) if mode == "seek" else np.array(ix, dtype=np.int32, order="C").reshape(n, 1152)
    out = np.zeros((n, 184), np.int32)
    if use_ref:
        f, h = (ref().ref_seek_record if mode == "seek" else ref().ref_isf2_record), tabs.ref.h
    else:
        f, h = (lib().hxo_seek_record if mode == "seek" else lib().hxo_isf2_record), tabs.enc.h
    f.argtypes, f.restype = [C.c_void_p] * 6, None
    for r in range(n):
        f(h, hdr[r].ctypes.data, xr[r].ctypes.data, other[r].ctypes.data, band[r].ctypes.data, out[r].ctypes.data)
    return out


def noise_band(tabs, x34, x, gsf, logn):
    """the oracle's noise_actual (l3math.c:512) of one band's lines at gain step gsf"""
    x34, x = (np.ascontiguousarray(a, dtype=np.float32) for a in (x34, x))
    f = lib().hxo_noise_band
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int], C.c_int
    return int(f(tabs.enc.h, x34.ctypes.data, x.ctypes.data, int(gsf), x.size, int(logn)))


def count_out_to_gr(tabs, out10):
    """COUNT_GR of a long channel's COUNT_OUT, by the oracle's output_subdivide2 (hxo_huffsel_to_gr)"""
    hs = np.ascontiguousarray(out10, dtype=np.int32)
    g = np.zeros(27, np.int32)
    f = lib().hxo_huffsel_to_gr
    f.argtypes = [C.c_void_p] * 3
    f.restype = None
    f(tabs.p, hs.ctypes.data, g.ctypes.data)
    return [int(g[7]), int(g[8]), int(g[9]), int(g[17]), int(g[1]), int(g[13]), int(g[14]), int(g[21]), int(g[22]), int(g[23]), int(g[18])]


def huff_tables():
    """the oracle's code tables: {"dim": [32], "linbits": [32], "len": {(t, x, y): bits}, "code": {(t, x, y): word},
    "quada": [(code, len)] * 16}; x, y below the table's dimension"""
    l = lib()
    dim = [int(l.hxo_huff_dim(t)) for t in range(32)]
    tabs = {"dim": dim, "linbits": [int(l.hxo_huff_linbits(t)) for t in range(32)], "len": {}, "code": {},
            "quada": [(int(l.hxo_quada_code(v)), int(l.hxo_quada_len(v))) for v in range(16)]}
    for t in range(32):
        for x in range(dim[t]):
            for y in range(dim[t]):
                tabs["len"][t, x, y] = int(l.hxo_huff_len(t, x, y))
                tabs["code"][t, x, y] = int(l.hxo_huff_code(t, x, y))
    return tabs


# ---- one granule's front end on subband blocks (hxo_spec_record, oracle/hxo.h; ref_spec_record, oracle/ref_harness.cpp) ----
def ref_has_spec_record():
    """whether the reference build at hand was made with the front-end entry in its harness"""
    return ref() is not None and hasattr(ref(), "ref_spec_record")


def ref_zero_has_spec_record():
    """the same of the build with uninitialised locals defined as zero (make -C oracle ref_zero)"""
    return ref_zero() is not None and hasattr(ref_zero(), "ref_spec_record")


def last_ms_metric(enc):
    """the two granules' metrics of the frame an OracleEncoder coded last, hysteresis included (every path)"""
    v = (C.c_int * 2)()
    lib().hxo_last_ms_metric.argtypes = [C.c_void_p, C.c_void_p]
    lib().hxo_last_ms_metric(enc.h, v)
    return int(v[0]), int(v[1])


def spec_records(enc, prev, cur, bt, use_ref=False, nchan=2, want_metric=True):
    """n granules through the front end between the polyphase filter and the allocator: prev / cur [n][2][576] the two
    subband blocks per channel, bt [n] the block types; enc an OracleEncoder (use_ref: a RefEncoder of the same control, with
    the channel count and whether the path forms a metric, which the reference's objects do not tell).  -> dict of copies:
    xr [n][2][576], metric [n] (before hysteresis), esave [n][2][64], sm [n][2][36][2], and from the oracle etab and thr
    [n][2][64] in the kernels' layout"""
    prev, cur = (np.ascontiguousarray(a, dtype=np.float32) for a in (prev, cur))
    n = prev.shape[0]
    assert prev.shape == cur.shape == (n, 2, 576) and len(bt) == n
    out = dict(xr=np.zeros((n, 2, 576), np.float32), etab=np.zeros((n, 2, 64), np.float32), thr=np.zeros((n, 2, 64), np.float32),
               metric=np.zeros(n, np.int32), esave=np.zeros((n, 2, 64), np.float32), sm=np.zeros((n, 2, 36, 2), np.float32))
    V = C.c_void_p
    if use_ref:
        f = enc.r.ref_spec_record       # (the build the RefEncoder was made with: the plain one or ref_zero's)
        f.argtypes, f.restype = [V, V, V, C.c_int, C.c_int, C.c_int, V, V, V, V], None
        for r in range(n):
            f(enc.h, prev[r].ctypes.data, cur[r].ctypes.data, int(bt[r]), int(nchan), int(want_metric), out["xr"][r].ctypes.data,
              out["esave"][r].ctypes.data, out["sm"][r].ctypes.data, out["metric"][r:].ctypes.data)
        return out
    f = lib().hxo_spec_record
    f.argtypes, f.restype = [V, V, V, C.c_int, V, V, V, V, V, V], None
    for r in range(n):
        f(enc.h, prev[r].ctypes.data, cur[r].ctypes.data, int(bt[r]), out["xr"][r].ctypes.data, out["etab"][r].ctypes.data,
          out["thr"][r].ctypes.data, out["metric"][r:].ctypes.data, out["esave"][r].ctypes.data, out["sm"][r].ctypes.data)
    return out
