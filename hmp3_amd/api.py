"""Python binding of the C ABI in include/hmp3_amd.h (hmp3_amd/libhmp3amd.so).

The library is the product: hand-written HIP kernels for gfx950 behind a C ABI.  This module
only loads it (ctypes) and mirrors the reference's CMp3Enc interface for tests / bench.  There
is no CPU fallback: if the library or a GPU is missing, calls raise.
"""
import ctypes as C
import os
import re
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# HMP3AMD_LIB selects another build of the same library (tools/: the -DHX_PROFILE build)
LIB_PATH = os.environ.get("HMP3AMD_LIB") or os.path.join(HERE, "libhmp3amd.so")


class EControl(C.Structure):
    """E_CONTROL (reference pub/encapp.h:42-72)"""
    _fields_ = [(n, C.c_int) for n in (
        "mode", "bitrate", "samprate", "nsbstereo", "filter_select", "freq_limit", "nsb_limit",
        "layer", "cr_bit", "original", "hf_flag", "vbr_flag", "vbr_mnr", "vbr_br_limit",
        "vbr_delta_mnr", "chan_add_f0", "chan_add_f1", "sparse_scale")] + \
        [("mnr_adjust", C.c_int * 21)] + \
        [(n, C.c_int) for n in ("cpu_select", "quick", "test1", "test2", "test3", "short_block_threshold")]


class Source(C.Structure):
    """HX_SOURCE: the other arguments of CMp3Enc::MP3_audio_encode_init (mp3enc.cpp:2655) for one source"""
    _fields_ = [(n, C.c_int) for n in ("bits", "is_float", "mpeg_select", "mono_convert")]


class MpegHead(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("sync", "id", "option", "prot", "br_index", "sr_index", "pad",
                                       "private_bit", "mode", "mode_ext", "cr", "original", "emphasis")]


class InOut(C.Structure):
    _fields_ = [("in_bytes", C.c_int), ("out_bytes", C.c_int)]


class IntPair(C.Structure):
    _fields_ = [("a", C.c_int), ("b", C.c_int)]


LEDGER_POINTS = 513     # HX_LEDGER_POINTS


class Ledger(C.Structure):
    """HX_LEDGER: one stream's file record (include/hmp3_amd.h: where the file ends, its MusicCRC, its seek points)"""
    _fields_ = [(n, C.c_int) for n in ("ncalls", "frames_per_call", "head_bytes", "flags", "open", "ended", "fed")] + \
        [(n, C.c_uint) for n in ("frames", "bytes", "crc")] + \
        [(n, C.c_int) for n in ("call_bytes", "toc_counter", "npt", "every")] + \
        [("pad0", C.c_int * 2), ("pt", C.c_int * 2 * LEDGER_POINTS), ("pad1", C.c_int * 2)]

    def tobytes(self):
        return bytes(memoryview(self))


class LedgerBrief(C.Structure):
    """HX_LEDGER_BRIEF: the short form of a record, with the slot's image_bytes (include/hmp3_amd.h, "file images")"""
    _fields_ = [(n, C.c_int) for n in ("open", "ended", "fed")] + [(n, C.c_uint) for n in ("frames", "bytes", "crc")] + \
        [("call_bytes", C.c_int), ("image_bytes", C.c_uint)]

    def tobytes(self):
        return bytes(memoryview(self))


class LedgerOpen(C.Structure):
    """HX_LEDGER_OPEN: what hx_batch_ledger_begin takes per listed slot"""
    _fields_ = [(n, C.c_int) for n in ("ncalls", "head_bytes", "flags", "reserved")]


class FileTag(C.Structure):
    """HX_FILE_TAG: what a finished file's tag frame needs beside its record (include/hmp3_amd.h, "finished files")"""
    _fields_ = [(n, C.c_int) for n in ("samprate", "h_mode", "cr_bit", "original_bit", "flags", "kbps", "vbr_scale")] + \
        [(n, C.c_uint) for n in ("lowpass", "in_samplerate", "reserved")] + [("samples_audio", C.c_ulonglong)]


# The ctypes type of every C type in include/hmp3_amd.h.  A parameter that is any other pointer or an array is a
# c_void_p, which takes byref(...), ctypes arrays, string buffers, plain integers and None.
CTYPES = {
    "int": C.c_int, "unsigned": C.c_uint, "unsigned short": C.c_ushort,
    "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float, "void": None,
    "HX_IN_OUT": InOut, "HX_INT_PAIR": IntPair, "const char *": C.c_char_p,
    "hx_batch *": C.c_void_p, "hx_enc *": C.c_void_p, "hx_multi *": C.c_void_p, "hx_src *": C.c_void_p,
    "hx_xing *": C.c_void_p, "void *": C.c_void_p, "unsigned char *": C.c_void_p,
}
HEADER = os.path.join(os.path.dirname(HERE), "include", "hmp3_amd.h")


def _norm(t):
    return " ".join(t.replace("*", " * ").split())


def _param_type(decl):
    """`const HX_E_CONTROL *ec` -> "const HX_E_CONTROL *", `int nbytes_out[2]` -> "int *" """
    m = re.fullmatch(r"\s*(.*?)\b\w+\s*(\[\w*\])?\s*", decl, re.S)
    return _norm(m.group(1) + ("*" if m.group(2) else ""))


def prototypes(path=HEADER):
    """every hx_* prototype of a C header: [(name, return type, [parameter types])]"""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*|^\s*#[^\n]*", " ", f.read(), flags=re.S | re.M)
    protos = []
    for decl in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*(.*?)\b(hx_\w+)\s*\((.*)\)\s*", decl, re.S)
        if m:
            args = m.group(3).strip()
            params = [] if args in ("", "void") else [_param_type(a) for a in args.split(",")]
            protos.append((m.group(2), _norm(m.group(1)), params))
    return protos


def signature(name, ret, params):
    """(restype, argtypes) of a prototype; a type outside CTYPES raises"""
    def ctype(t, param):
        if param and t.endswith("*") and t != "const char *":
            return C.c_void_p
        if t not in CTYPES:
            raise TypeError("include/hmp3_amd.h: %s %s(%s): no ctypes type for '%s'" % (ret, name, ", ".join(params), t))
        return CTYPES[t]
    return ctype(ret, False), [ctype(t, True) for t in params]


PROTOTYPES = prototypes()
EXPORTS = [p[0] for p in PROTOTYPES]
_lib = None


def lib():
    """load libhmp3amd.so (raises if it has not been built: run hmp3_amd/build.sh), every function declared as
    include/hmp3_amd.h declares it"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("hmp3_amd/libhmp3amd.so is missing - build it with hmp3_amd/build.sh "
                               "(there is no CPU fallback)")
        sigs = {p[0]: signature(*p) for p in PROTOTYPES}
        # One HIP runtime per process: PyTorch bundles its own libamdhip64, and whichever copy is
        # mapped first serves both.  Import torch (when present) before our library so that tensors
        # and our kernels share a runtime; without torch the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in sigs.items():
            if hasattr(L, name):        # a build picked through HMP3AMD_LIB (A/B runs) may predate the header
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def default_control(**kw):
    """CLI defaults (reference test/tomp3.cpp:357-384); bitrate=N per channel selects CBR (-B N)"""
    ec = EControl()
    lib().hx_default_control(C.byref(ec))
    for k, v in kw.items():
        setattr(ec, k, v)
    if kw.get("bitrate", -1) > 0 and "vbr_flag" not in kw:
        ec.vbr_flag = 0
    return ec


def libm_report(points=1000):
    """the host's C library and whether its logf / log10f agree with the restatement the first-generation allocator's
    kernels use (hx_libm32.h = glibc 2.35): {"glibc": "2.35", "points": 1000, "mismatches": 0}"""
    L = lib()
    return {"glibc": L.hx_libc_version().decode(), "points": points, "mismatches": int(L.hx_libm_spot_check(points))}


def _math_operands(arrays):
    """the operands of a debug math call as uint32 [k][n]: each array's 32-bit patterns, none converted"""
    ops = [np.ascontiguousarray(a).reshape(-1) for a in arrays]
    if not ops or any(a.dtype.itemsize != 4 or a.size != ops[0].size for a in ops):
        raise ValueError("operands are equally long arrays of 32-bit values")
    return np.ascontiguousarray(np.stack([a.view(np.uint32) for a in ops]))


def host_math(ec, name, *arrays):
    """hx_debug_host_math: the host build of the first-generation allocator's logf / log10f restatement on arrays, the
    host-side counterpart of Batch.debug_math for "logf", "log10f", "a1_mask_db" and "a1_gz" -> uint32 [n]"""
    ops = _math_operands(arrays)
    out = np.zeros(ops.shape[1], dtype=np.uint32)
    if lib().hx_debug_host_math(C.byref(ec), name.encode(), ops.ctypes.data, ops.shape[1], out.ctypes.data) != 0:
        raise RuntimeError("hx_debug_host_math(%s): rejected" % name)
    return out


COUNT_MODES = {"count": 0, "quant_count": 1, "quant_then_count": 2, "short": 3, "short_count": 4}
COUNT_UNITS = ("k_alloc", "k_alloc_slim", "k_alloc_lsf", "k_alloc1", "k_alloc1_lsf")


def debug_count(ec, unit, mode, hdr, ix, ixmax, x34=None, gsf=None, device=0):
    """hx_debug_count: the stream walk's quantiser and Huffman counter, as `unit` builds them, on n records (the layouts:
    include/hmp3_amd.h).  mode is a name of COUNT_MODES.  -> (rc, lines, band maxima, out [n][24]): copies of ix and ixmax
    as the functions left them; rc = -1: refused (last_error() says why) and nothing was launched"""
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    n = hdr.shape[0]
    ix = np.array(ix, dtype=np.int32, order="C")
    ixmax = np.array(ixmax, dtype=np.int32, order="C")
    x34 = None if x34 is None else np.ascontiguousarray(x34, dtype=np.float32)
    gsf = None if gsf is None else np.ascontiguousarray(gsf, dtype=np.int32)
    nband = 48 if mode.startswith("short") else 22
    if hdr.shape != (n, 16) or ix.size != n * 1152 or ixmax.size != n * 2 * nband or (x34 is not None and x34.size != n * 1152) or \
            (gsf is not None and gsf.size != n * 2 * nband):
        raise ValueError("arrays of %d records expected" % n)
    out = np.zeros((n, 24), dtype=np.int32)
    rc = lib().hx_debug_count(int(device), C.byref(ec), unit.encode(), COUNT_MODES[mode], n, hdr.ctypes.data, ix.ctypes.data, ixmax.ctypes.data,
                              None if x34 is None else x34.ctypes.data, None if gsf is None else gsf.ctypes.data, out.ctypes.data)
    return rc, ix, ixmax, out


SEEK_MODES = {"seek": 0, "isf2": 1}
SEEK_UNITS = COUNT_UNITS[:3]


def debug_seek(ec, unit, mode, hdr, xr, band, x34=None, x34max=None, ix=None, strict_sums=False, device=0):
    """hx_debug_seek: the stream walk's gain search ("seek") or inverse_sf2 ("isf2"), as `unit` builds them, on n records (the
    layouts: include/hmp3_amd.h).  -> (rc, out [n][184]); rc = -1: refused (last_error() says why), nothing was launched and
    out is zeros"""
    hdr = np.ascontiguousarray(hdr, dtype=np.int32)
    n = hdr.shape[0]
    xr = np.ascontiguousarray(xr, dtype=np.float32)
    band = np.ascontiguousarray(band, dtype=np.int32)
    x34, x34max = (None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (x34, x34max))
    ix = None if ix is None else np.ascontiguousarray(ix, dtype=np.int32)
    if hdr.shape != (n, 16) or xr.size != n * 1152 or band.size != n * 44 * 8 or (x34 is not None and x34.size != n * 1152) or \
            (x34max is not None and x34max.size != n * 44) or (ix is not None and ix.size != n * 1152):
        raise ValueError("arrays of %d records expected" % n)
    out = np.zeros((n, 184), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib().hx_debug_seek(int(device), C.byref(ec), unit.encode(), SEEK_MODES[mode], int(bool(strict_sums)), n, hdr.ctypes.data, xr.ctypes.data,
                             ptr(x34), ptr(ix), band.ctypes.data, ptr(x34max), out.ctypes.data)
    return rc, out


def debug_recon(ecs, cls, NG, nfr, ixq, sgn, seg, rec, state, hyb, out, device=0):
    """hx_debug_recon: the decoded-PCM kernels on records of the caller's (the layouts: include/hmp3_amd.h).  ecs: the
    controls of the classes in play, cls [S] each stream's class, nfr [S] or None; seg and rec are arrays of the records'
    bytes.  -> (rc, state, hyb, out): copies of state [S][2112], hyb [S][NG][2][576] and out [S][row] as the kernels left
    them; rc = -1: refused (last_error() says why) and nothing was launched"""
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    S = cls.size
    nfr = None if nfr is None else np.ascontiguousarray(nfr, dtype=np.int32)
    ixq = np.ascontiguousarray(ixq, dtype=np.int16)
    sgn = np.ascontiguousarray(sgn, dtype=np.uint32)
    seg, rec = np.ascontiguousarray(seg), np.ascontiguousarray(rec)
    state, hyb, out = (np.array(a, dtype=np.float32, order="C") for a in (state, hyb, out))
    if ixq.size != S * NG * 1152 or sgn.size * 576 != ixq.size * (sgn.shape[-1] if sgn.ndim else 1) or hyb.size != ixq.size or \
            out.ndim != 2 or out.shape[0] != S or state.shape[0] != S or (nfr is not None and nfr.size != S):
        raise ValueError("arrays of %d streams x %d granules expected" % (S, NG))
    arr = (EControl * len(ecs))(*ecs)
    rc = lib().hx_debug_recon(int(device), arr, len(ecs), cls.ctypes.data, S, int(NG), None if nfr is None else nfr.ctypes.data, ixq.ctypes.data,
                              sgn.ctypes.data, seg.ctypes.data, rec.ctypes.data, state.ctypes.data, hyb.ctypes.data, out.ctypes.data, out.shape[1])
    return rc, state, hyb, out


SPEC_SAMPLE_MAX = 2.0 ** 33        # HX_SPEC_SAMPLE_MAX (include/hmp3_amd.h)


def debug_spec(ecs, cls, NG, nfr, direct, sb, bt, xr, etab, thr, msbase, device=0):
    """hx_debug_spec: K4 (direct False: k_spec, True: k_spec_direct) on subband blocks of the caller's (the layouts:
    include/hmp3_amd.h).  ecs: the controls of the classes in play, cls [S] each stream's class, nfr [S] or None;
    sb [S][2][NG + 1][576], bt [S][NG].  -> (rc, xr [S][NG][2][576], etab [S][NG][2][64], thr [S][NG][2][64], msbase [S][NG]):
    copies of the caller's arrays as the kernel left them; rc = -1: refused (last_error() says why) and nothing was launched"""
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    S = cls.size
    nfr = None if nfr is None else np.ascontiguousarray(nfr, dtype=np.int32)
    sb = np.ascontiguousarray(sb, dtype=np.float32)
    bt = np.ascontiguousarray(bt, dtype=np.uint8)
    xr, etab, thr = (np.array(a, dtype=np.float32, order="C") for a in (xr, etab, thr))
    msbase = np.array(msbase, dtype=np.int32, order="C")
    if sb.size != S * 2 * (NG + 1) * 576 or bt.size != S * NG or xr.size != S * NG * 1152 or etab.size != S * NG * 128 or \
            thr.size != S * NG * 128 or msbase.size != S * NG or (nfr is not None and nfr.size != S):
        raise ValueError("arrays of %d streams x %d granules expected" % (S, NG))
    arr = (EControl * len(ecs))(*ecs)
    rc = lib().hx_debug_spec(int(device), arr, len(ecs), cls.ctypes.data, S, int(NG), None if nfr is None else nfr.ctypes.data, int(bool(direct)),
                             sb.ctypes.data, bt.ctypes.data, xr.ctypes.data, etab.ctypes.data, thr.ctypes.data, msbase.ctypes.data)
    return rc, xr, etab, thr, msbase


def device_numa_node(device):
    return int(lib().hx_device_numa_node(int(device)))


def bind_thread_to_device(device):
    """restrict the calling thread to the CPUs of the device's NUMA node; returns their number (0: nothing changed)"""
    return int(lib().hx_bind_thread_to_device(int(device)))


def refresh_process_cpus():
    """re-capture the CPUs the process may use (after a launcher narrowed it); returns their number"""
    return int(lib().hx_refresh_process_cpus())


def bind_thread_to_node(node):
    """restrict the calling thread to the CPUs of NUMA node `node` that the process may use; returns their number (0: nothing changed)"""
    return int(lib().hx_bind_thread_to_node(int(node)))


def build_id():
    """hash of the sources / flags the loaded library was built from (None for builds that predate it)"""
    L = lib()
    return L.hx_build_id().decode() if hasattr(L, "hx_build_id") else None


def last_error():
    return lib().hx_last_error().decode()


def recon_delay():
    """D: the samples a batch's decoded PCM (Batch.recon_buffer) trails its input by (hx_recon_delay)"""
    return int(lib().hx_recon_delay())


def crc_combine(a, b, n):
    """the MusicCRC of A ++ B from a = CRC(0, A), b = CRC(0, B) and n = len(B) (hx_xing_crc_combine)"""
    return int(lib().hx_xing_crc_combine(int(a), int(b), int(n)))


def ledger_open(ncalls, frames_per_call=1, head_bytes=0, flags=0):
    """a new open record (hx_ledger_open)"""
    r = Ledger()
    lib().hx_ledger_open(C.byref(r), int(ncalls), int(frames_per_call), int(head_bytes), int(flags))
    return r


def ledger_update(rec, stats, crc, out_bytes):
    """one stream's slice of one call into its record, on the host (hx_ledger_update): stats [n][2] frame counters, crc [n]
    per-frame CRCs, out_bytes the stream's byte count of the call; True when the call ended the file"""
    st = np.ascontiguousarray(stats, dtype=np.int32).reshape(-1, 2)
    cr = np.ascontiguousarray(crc, dtype=np.uint16).reshape(-1)
    if len(cr) != len(st):
        raise ValueError("%d frame counters and %d CRCs" % (len(st), len(cr)))
    return bool(lib().hx_ledger_update(C.byref(rec), st.ctypes.data, cr.ctypes.data, len(st), int(out_bytes)))


def ledger_brief(rec, image_bytes=0):
    """the short form of a record, on the host (hx_ledger_brief)"""
    out = LedgerBrief()
    lib().hx_ledger_brief(C.byref(rec), int(image_bytes), C.byref(out))
    return out


def _ledger_poll(fn, handle, n):
    out = (LedgerBrief * n)()
    if fn(handle, out) != 0:
        raise RuntimeError("%s failed: %s" % (fn.__name__, last_error()))
    return [LedgerBrief.from_buffer_copy(out[e]) for e in range(n)]


def _file_fetch(fn, handle, i, cap, fill):
    """-> the file's bytes as fetched into a buffer of cap bytes pre-filled with `fill` (the tag's bytes keep the fill)"""
    buf = np.full(max(int(cap), 1), fill, dtype=np.uint8)
    n = int(fn(handle, int(i), buf.ctypes.data, int(cap)))
    if n < 0:
        raise RuntimeError("%s failed: %s" % (fn.__name__, last_error()))
    return buf[:n].tobytes()


def file_tag_bytes(tag):
    """the size of the tag frame a FileTag describes, 0 = none (hx_file_tag_bytes): the head_bytes of the file's ledger_begin"""
    return int(lib().hx_file_tag_bytes(C.byref(tag)))


def file_tag_build(rec, tag):
    """the tag frame of a record, on the host (hx_file_tag_build) -> bytes, b"" where the function returns 0"""
    buf = (C.c_ubyte * 1440)()
    return bytes(buf[:int(lib().hx_file_tag_build(C.byref(rec), C.byref(tag), buf, 1440))])


def _tag_array(tags, n):
    tags = list(tags)
    if len(tags) != n:
        raise ValueError("%d tags for %d slots" % (len(tags), n))
    return (FileTag * max(n, 1))(*tags)


def _file_fetch_many(fn, handle, idx, cap, fill):
    """-> (the dense image as fetched into a buffer of cap bytes pre-filled with `fill`, whole; off [n + 1]; the call's return)"""
    idx = [int(i) for i in idx]
    n = len(idx)
    buf = np.full(max(int(cap), 1), fill, dtype=np.uint8)
    off = np.full(n + 1, -1, dtype=np.int64)
    r = int(fn(handle, (C.c_int * max(n, 1))(*idx), n, buf.ctypes.data, int(cap), off.ctypes.data))
    return buf[:int(cap)], off, r


def _files_status(name, r):
    if r < 0:
        raise RuntimeError("%s failed: %s" % (name, last_error()))
    return int(r)


def _encode_src_files_host(fn, handle, n, rows, nframes, counts, frame_off):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    assert rows.ndim == 2 and rows.shape[0] == n
    off = None if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
    used = np.zeros(n, dtype=np.int64)
    r = fn(handle, rows.ctypes.data, rows.shape[1], None if off is None else off.ctypes.data, nframes, _counts_array(n, counts), used.ctypes.data)
    return _files_status(fn.__name__, r), used


def xing_load_points(xing_handle, rec):
    """the record's seek points into an hx_xing (hx_xing_load_points)"""
    if lib().hx_xing_load_points(xing_handle, C.byref(rec)) != 1:
        raise RuntimeError("hx_xing_load_points: not a record's seek-point state")


def _ledger_open_array(idx, ncalls, head_bytes, flags):
    idx = [int(i) for i in idx]
    n = len(idx)

    def per_slot(v):
        v = [int(v)] * n if np.isscalar(v) else [int(x) for x in v]
        if len(v) != n:
            raise ValueError("%d values for %d slots" % (len(v), n))
        return v
    nc, hb, fl = per_slot(ncalls), per_slot(head_bytes), per_slot(flags)
    return (C.c_int * max(n, 1))(*idx), (LedgerOpen * max(n, 1))(*[LedgerOpen(nc[e], hb[e], fl[e], 0) for e in range(n)]), n


def _counts_array(n, counts):
    if counts is None:
        return None
    counts = [int(c) for c in counts]
    if len(counts) != n:
        raise ValueError("frame counts: %d values for %d streams" % (len(counts), n))
    return (C.c_int * n)(*counts)


def _encode_src_counts_host(fn, handle, n, stride, rows, nframes, counts, frame_off, stats, crc):
    """the converting host calls under per-call counts (hx_batch_ / hx_multi_encode_src_counts_host)"""
    if crc and not stats:
        raise TypeError("encode_src_counts_host(crc=True) needs stats=True (the CRCs follow from the call's frame counters)")
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    assert rows.ndim == 2 and rows.shape[0] == n
    off = None if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
    assert off is None or off.shape == (n, nframes)
    out = np.zeros((n, stride), dtype=np.uint8)
    nb = np.zeros(n, dtype=np.int32)
    used = np.zeros(n, dtype=np.int64)
    st = np.zeros((n, nframes, 2), dtype=np.int32) if stats else None
    cr = np.zeros((n, nframes), dtype=np.uint16) if crc else None
    r = fn(handle, rows.ctypes.data, rows.shape[1], None if off is None else off.ctypes.data, nframes, _counts_array(n, counts),
           out.ctypes.data, stride, nb.ctypes.data, used.ctypes.data, None if st is None else st.ctypes.data, None if cr is None else cr.ctypes.data)
    if r != 0:
        raise RuntimeError("%s failed: %s" % (fn.__name__, last_error()))
    res = [out[i, :nb[i]].tobytes() for i in range(n)]
    return (res, used) + ((st,) if stats else ()) + ((cr,) if crc else ())


def _menu_args(controls, sources, nstreams, cfg):
    """ctypes arguments of the menu constructors: (ec array, nmenu, src array or None, cfg array or None)"""
    nmenu = len(controls)
    ec = (EControl * nmenu)(*controls)
    src = None
    if sources is not None:
        if len(sources) != nmenu:
            raise ValueError("a menu of %d controls and %d sources" % (nmenu, len(sources)))
        src = (Source * nmenu)(*sources)
    return ec, nmenu, src, _counts_array(nstreams, cfg)


def _int_pair_arrays(idx, cfg):
    idx, cfg = [int(i) for i in idx], [int(c) for c in cfg]
    if len(idx) != len(cfg):
        raise ValueError("%d slots and %d configurations" % (len(idx), len(cfg)))
    n = len(idx)
    return (C.c_int * max(n, 1))(*idx), (C.c_int * max(n, 1))(*cfg), n


def _frame_counts(setter, handle, n, counts):
    if setter(handle, _counts_array(n, counts)) != 0:
        raise RuntimeError("%s failed: %s" % (setter.__name__, last_error()))


def packed_layout(nframes, channels, counts=None, f32=False):
    """the tight layout of a call's PCM image (hx_pcm_packed_layout; host only): stream i's segment is counts[i] (None:
    nframes) frames of channels[i] channels, int16 or float32, the segments back to back -> (offsets int64 [n + 1], the
    image's bytes = offsets[n])"""
    ch = [int(c) for c in channels]
    n = len(ch)
    off = np.zeros(n + 1, dtype=np.int64)
    total = int(lib().hx_pcm_packed_layout(n, int(nframes), _counts_array(n, counts), (C.c_int * max(n, 1))(*ch), 4 if f32 else 2, off.ctypes.data))
    if total < 0:
        raise ValueError("hx_pcm_packed_layout: bad arguments (channels 1 or 2, counts within 0 .. nframes)")
    return off, total


def _pcm_segments(setter, handle, n, off, in_bytes):
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        if len(off) not in (n, n + 1):
            raise ValueError("PCM segments: %d offsets for %d streams" % (len(off), n))
    if setter(handle, None if off is None else off.ctypes.data, int(in_bytes)) != 0:
        raise RuntimeError("%s failed: %s" % (setter.__name__, last_error()))


def planar_layout(nframes, channels, counts=None, f32=False):
    """the tight planar layout of a call's PCM image (hx_pcm_planar_layout; host only): stream i's channels[i] planes of
    counts[i] (None: nframes) frames back to back, the streams back to back -> (offsets int64 [n + 1], chan_stride int64 [n],
    the image's bytes = offsets[n])"""
    ch = [int(c) for c in channels]
    n = len(ch)
    off, stride = np.zeros(n + 1, dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    total = int(lib().hx_pcm_planar_layout(n, int(nframes), _counts_array(n, counts), (C.c_int * max(n, 1))(*ch), 4 if f32 else 2, off.ctypes.data,
                                           stride.ctypes.data))
    if total < 0:
        raise ValueError("hx_pcm_planar_layout: bad arguments (channels 1 or 2, counts within 0 .. nframes)")
    return off, stride[:n], total


def _pcm_planes(setter, handle, n, off, chan_stride, in_bytes, unit_scale):
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
        if len(off) not in (n, n + 1):
            raise ValueError("PCM planes: %d offsets for %d streams" % (len(off), n))
        if chan_stride is not None:
            chan_stride = np.ascontiguousarray(chan_stride, dtype=np.int64).reshape(-1)
            if len(chan_stride) != n:
                raise ValueError("PCM planes: %d strides for %d streams" % (len(chan_stride), n))
    if setter(handle, None if off is None else off.ctypes.data, None if off is None or chan_stride is None else chan_stride.ctypes.data,
              int(in_bytes), int(unit_scale)) != 0:
        raise RuntimeError("%s failed: %s" % (setter.__name__, last_error()))


def tensor_planes(shape, strides, itemsize):
    """the PCM planes of a waveform tensor [S, C, T] or [S, T], from its shape and its strides in elements alone (nothing of
    the tensor is read or copied) -> (off int64 [S], chan_stride int64 [S], in_bytes, first): byte offsets and strides for
    pcm_planes, relative to the lowest element the tensor addresses, which lies `first` elements from element [0, .. 0] (0
    unless a stride is negative).  T must be a positive multiple of 1152 and the last dimension's stride 1."""
    shape, strides = [int(v) for v in shape], [int(v) for v in strides]
    if len(shape) == 2:
        shape, strides = [shape[0], 1, shape[1]], [strides[0], 0, strides[1]]
    if len(shape) != 3 or len(strides) != 3:
        raise ValueError("a waveform is [streams, channels, time] or [streams, time], not %d-dimensional" % len(shape))
    S, Cn, T = shape
    if Cn not in (1, 2):
        raise ValueError("a waveform has 1 or 2 channels, not %d" % Cn)
    if T <= 0 or T % 1152 != 0:
        raise ValueError("a waveform's time dimension must be a positive multiple of 1152, not %d" % T)
    if strides[2] != 1:
        raise ValueError("the last (time) dimension of a waveform must have stride 1, not %d: planes are consecutive samples" % strides[2])
    start = [s * strides[0] + c * strides[1] for s in range(S) for c in range(Cn)]
    first = min(start) if start else 0
    off = np.array([(s * strides[0] - first) * itemsize for s in range(S)], dtype=np.int64)
    chan_stride = np.full(S, strides[1] * itemsize, dtype=np.int64)
    return off, chan_stride, ((max(start) - first + T) if start else 0) * itemsize, first


def _pcm_image(image):
    """-> a host call's flat PCM image as the C ABI takes it: contiguous int16 or float32 (at int16 scale), any shape"""
    f32 = np.asarray(image).dtype == np.float32
    return np.ascontiguousarray(image, dtype=np.float32 if f32 else np.int16)


def _pitch(batch_handle):
    """hx_batch_pcm_channels, or None from a library build that predates it (A/B runs through HMP3AMD_LIB)"""
    L = lib()
    return int(L.hx_batch_pcm_channels(batch_handle)) if hasattr(L, "hx_batch_pcm_channels") else None


def _pcm_rows(pcm, n, P):
    """-> (a host call's PCM as the C ABI takes it, [n, nframes * 1152 * P], and nframes) from [n, nframes * 1152, P] or from
    the rows as they lie in memory, [n, nframes * 1152 * P]: the form the callers of a mixed batch fill, a mono stream's
    samples first in its row.  P: the batch's pitch (_pitch), or None: the channels of the three-dimensional form, else 1"""
    f32 = np.asarray(pcm).dtype == np.float32
    pcm = np.ascontiguousarray(pcm, dtype=np.float32 if f32 else np.int16)
    if pcm.ndim == 3:
        ch, nsamp = pcm.shape[2], pcm.shape[1]
        if ch not in (1, 2) or (P is not None and ch != P):
            raise ValueError("PCM of %d channels for a batch whose rows hold %s" % (ch, P))
    elif pcm.ndim == 2:
        nsamp, rem = divmod(pcm.shape[1], P or 1)
        if rem:
            raise ValueError("a PCM row of %d samples is no multiple of the %d channels it holds" % (pcm.shape[1], P))
    else:
        raise ValueError("PCM must be [n, nframes * 1152 * channels] or [n, nframes * 1152, channels]")
    if pcm.shape[0] != n or nsamp % 1152 != 0:
        raise ValueError("PCM must hold %d rows of whole frames (1152 samples per channel)" % n)
    return pcm.reshape(n, -1), nsamp // 1152


class Batch:
    """N independent streams on one GPU (hx_batch_*)."""

    def __init__(self, controls, nstreams=None, max_frames=256, device=0):
        L = lib()
        if isinstance(controls, EControl):
            self.n = int(nstreams)
            self._ec = controls
            self.h = L.hx_batch_create(device, self.n, C.byref(controls), 1, max_frames)
        else:
            self.n = len(controls)
            arr = (EControl * self.n)(*controls)
            self._ec = arr
            self.h = L.hx_batch_create(device, self.n, arr, 0, max_frames)
        if not self.h:
            raise RuntimeError("hx_batch_create failed: " + last_error())
        self.max_frames, self.device = max_frames, int(device)

    @classmethod
    def menu(cls, controls, nstreams, cfg=None, max_frames=256, device=0, sources=None):
        """a batch over a menu of configurations (hx_batch_create_menu): controls = the menu's entries, cfg = the entry each
        of the nstreams slots starts with (None: entry 0); assign_streams hands slots other entries later.  sources (one
        Source per entry): a converting batch - SrcBatch.menu passes it"""
        return cls._from_menu("hx_batch_create_menu", controls, nstreams, cfg, max_frames, device, sources)

    @classmethod
    def mixed(cls, controls, nstreams, cfg=None, max_frames=256, device=0, sources=None):
        """Batch.menu whose entries may differ in channel count (hx_batch_create_mixed): the PCM rows are pitched for
        P = pcm_channels() channels, and a mono stream of a P = 2 batch has its samples contiguous at the start of its row"""
        return cls._from_menu("hx_batch_create_mixed", controls, nstreams, cfg, max_frames, device, sources)

    @classmethod
    def any(cls, controls, nstreams, cfg=None, max_frames=256, device=0, sources=None):
        """Batch.mixed whose entries may also differ in MPEG version and allocator generation (hx_batch_create_any): MPEG-1
        and MPEG-2 rates, dual channel and intensity stereo beside the others; stream_frames_per_block says how many frames a
        slot makes of a 1152-sample block"""
        return cls._from_menu("hx_batch_create_any", controls, nstreams, cfg, max_frames, device, sources)

    @classmethod
    def _from_menu(cls, create, controls, nstreams, cfg, max_frames, device, sources):
        self = cls.__new__(cls)
        self.n = int(nstreams)
        self._ec, nmenu, self._src, arr = _menu_args(controls, sources, self.n, cfg)
        self.h = getattr(lib(), create)(device, self.n, self._ec, nmenu, self._src, arr, max_frames)
        if not self.h:
            raise RuntimeError(create + " failed: " + last_error())
        self.max_frames, self.device = max_frames, int(device)
        return self

    def pcm_channels(self):
        """P: the channels every PCM row is pitched for = the largest channel count over the menu"""
        return int(lib().hx_batch_pcm_channels(self.h))

    def stream_channels(self, i):
        """channels of the entry slot i runs, as of the calls made so far"""
        k = int(lib().hx_batch_stream_channels(self.h, int(i)))
        if k < 0:
            raise IndexError(i)
        return k

    def stream_frames_per_block(self, i):
        """frames per 1152-sample block (1, or 2 at the MPEG-2 rates) of the entry slot i runs, as of the calls made so far"""
        k = int(lib().hx_batch_stream_frames_per_block(self.h, int(i)))
        if k < 0:
            raise IndexError(i)
        return k

    def nconfigs(self):
        """entries of the batch's menu (a batch not created from a menu: its distinct controls)"""
        return int(lib().hx_batch_nconfigs(self.h))

    def stream_config(self, i):
        """the menu entry slot i runs, as of the calls made so far"""
        k = int(lib().hx_batch_stream_config(self.h, int(i)))
        if k < 0:
            raise IndexError(i)
        return k

    def assign_streams(self, idx, cfg, stream=None):
        """slot idx[e] starts a new stream of menu entry cfg[e]: one launch, asynchronous on `stream` and ordered like a
        plain device call, exactly as reset_streams (hx_batch_assign_streams)"""
        ai, ac, n = _int_pair_arrays(idx, cfg)
        if lib().hx_batch_assign_streams(self.h, ai, ac, n, stream) != 0:
            raise RuntimeError("hx_batch_assign_streams failed: " + last_error())

    def out_stride(self, nframes):
        return int(lib().hx_batch_out_stride(self.h, nframes))

    def packet_buffers(self, d_packet_ptr, frame_stride, d_packet_bytes_ptr):
        """device buffers [n, nframes, frame_stride] uint8 and [n, nframes, 2] int32 that the calls that follow write
        every frame's self-contained packet and its size(s) to; packet_buffers(None, 0, None) switches them off"""
        lib().hx_batch_packet_buffers(self.h, d_packet_ptr, frame_stride, d_packet_bytes_ptr)

    def frame_stats_buffer(self, d_stats_ptr):
        """device buffer [n, nframes, 2] int32 that the calls that follow write the stream's frames / bytes emitted so far
        to, after every input frame; None switches it off"""
        lib().hx_batch_frame_stats_buffer(self.h, d_stats_ptr)

    def crc_buffer(self, d_crc_ptr):
        """device buffer [n, nframes] uint16 that the calls that follow write the MusicCRC of their bytes up to every input
        frame to (include/hmp3_amd.h, "MusicCRC"; needs a frame_stats_buffer in force); None switches it off"""
        if lib().hx_batch_crc_buffer(self.h, d_crc_ptr) != 0:
            raise RuntimeError("hx_batch_crc_buffer failed: " + last_error())

    def recon_buffer(self, d_recon_ptr):
        """device buffer [n, nframes * 1152 * P] float32 that the calls that follow write their decoded PCM to
        (include/hmp3_amd.h, "decoded PCM"): laid out like the f32 PCM rows; None switches it off"""
        if lib().hx_batch_recon_buffer(self.h, d_recon_ptr) != 0:
            raise RuntimeError("hx_batch_recon_buffer failed: " + last_error())

    def encode_host_recon(self, pcm):
        """encode_host of float32 PCM that also returns the call's decoded PCM -> (list of bytes per stream, float32
        [n, nframes * 1152 * P]; what lies behind a stream's blocks of the call is zero)"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.h))
        if pcm.dtype != np.float32:
            raise TypeError("encode_host_recon takes float32 PCM (hx_batch_encode_f32_host_recon)")
        stride = self.out_stride(nfr)
        out = np.zeros((self.n, stride), dtype=np.uint8)
        nb = np.zeros(self.n, dtype=np.int32)
        rec = np.zeros((self.n, nfr * 1152 * _pitch(self.h)), dtype=np.float32)
        if lib().hx_batch_encode_f32_host_recon(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data, rec.ctypes.data) != 0:
            raise RuntimeError("hx_batch_encode_f32_host_recon failed: " + last_error())
        return [out[i, :nb[i]].tobytes() for i in range(self.n)], rec

    def frame_counts(self, counts):
        """per-stream frame counts of the calls that follow: a sequence of n ints (stream i takes the first counts[i] frames of
        its row; 0 = it sits the call out), or None = every stream takes the call's nframes (hx_batch_frame_counts)"""
        _frame_counts(lib().hx_batch_frame_counts, self.h, self.n, counts)
        self._counts = None if counts is None else [int(c) for c in counts]

    def pcm_segments(self, off, in_bytes=0):
        """PCM segments of the calls that follow (hx_batch_pcm_segments): off = n byte offsets (n + 1, as packed_layout returns
        them, is taken too) into one image of in_bytes bytes - the pcm / d_pcm argument of every encode and submit call is
        then the image's base, and stream i's input the bytes at off[i]; None = back to rows"""
        _pcm_segments(lib().hx_batch_pcm_segments, self.h, self.n, off, in_bytes)

    def pcm_planes(self, off, chan_stride=None, in_bytes=0, unit_scale=False):
        """PCM planes of the calls that follow (hx_batch_pcm_planes): off = n byte offsets (n + 1, as planar_layout returns them,
        is taken too) of the streams' first planes in one image of in_bytes bytes, chan_stride = n byte distances to their
        second planes (None: tight) - the pcm / d_pcm argument of every encode and submit call is then the image's base;
        unit_scale: float32 samples are in [-1, 1) and taken as x * 32768; off None = back to rows"""
        _pcm_planes(lib().hx_batch_pcm_planes, self.h, self.n, off, chan_stride, in_bytes, unit_scale)

    def encode_tensor(self, waveform, d_out_ptr=None, out_stride=None, d_out_bytes_ptr=None, stream=None, unit_scale=None, stats=False, crc=False):
        """encode a torch waveform [n, C, T] or [n, T], int16 or float32, T a multiple of 1152, where it lies: its planes are
        derived from waveform.stride() (tensor_planes; the last dimension must have stride 1) and set with pcm_planes, which
        stay in force.  unit_scale (None: True for float32): the samples are in [-1, 1).  A tensor on the batch's device
        makes the device call into d_out_ptr / out_stride / d_out_bytes_ptr on `stream`, as encode_device; a host tensor
        the host call and returns what encode_host returns (stats, crc: as there).  The waveform has as many channels as
        the batch's rows (pcm_channels()).  Every argument is checked before the planes are set: a call that raises
        ValueError or TypeError leaves the batch as it was"""
        import torch
        if waveform.dtype not in (torch.int16, torch.float32):
            raise TypeError("encode_tensor takes an int16 or float32 waveform, not %s" % waveform.dtype)
        f32 = waveform.dtype == torch.float32
        item = 4 if f32 else 2
        if waveform.shape[0] != self.n:
            raise ValueError("a waveform of %d streams for a batch of %d" % (waveform.shape[0], self.n))
        off, chan_stride, in_bytes, first = tensor_planes(waveform.shape, waveform.stride(), item)
        nch = 1 if waveform.dim() == 2 else int(waveform.shape[1])
        if nch != self.pcm_channels():
            raise ValueError("a waveform of %d channel(s) for a batch whose rows have %d" % (nch, self.pcm_channels()))
        nframes = int(waveform.shape[-1]) // 1152
        if nframes > self.max_frames:
            raise ValueError("a waveform of %d frames for a batch of max_frames = %d" % (nframes, self.max_frames))
        if waveform.is_cuda:
            if waveform.device.index != self.device:
                raise ValueError("the waveform lies on device %s, the batch on device %d" % (waveform.device.index, self.device))
            if d_out_ptr is None or d_out_bytes_ptr is None:
                raise ValueError("a device waveform needs d_out_ptr and d_out_bytes_ptr, as encode_device")
        elif waveform.device.type != "cpu":
            raise ValueError("a waveform lies on the batch's device or on the host, not on %s" % waveform.device)
        base = waveform.data_ptr() + first * item
        self.pcm_planes(off, chan_stride, in_bytes, (f32 if unit_scale is None else unit_scale))
        if waveform.is_cuda:
            return self.encode_device(base, nframes, d_out_ptr, self.out_stride(nframes) if out_stride is None else out_stride, d_out_bytes_ptr, stream, f32=f32)
        image = np.frombuffer((C.c_ubyte * in_bytes).from_address(base), dtype=np.float32 if f32 else np.int16)     # (a view: waveform stays alive through the call)
        return self._encode_host(image, nframes, stats, crc)

    def packed_layout(self, nframes, f32=False):
        """the tight layout (api.packed_layout) of a call of nframes made now: the counts in force (frame_counts) and the
        channels of the entries the slots run -> (offsets int64 [n + 1], the image's bytes)"""
        return packed_layout(nframes, [self.stream_channels(i) for i in range(self.n)], getattr(self, "_counts", None), f32)

    def encode_host(self, pcm, stats=False, crc=False):
        """pcm: int16 (or float32 at int16 scale) [n, nframes*1152, P] or [n, nframes*1152*P], P = pcm_channels() (a mono
        stream of a mixed batch: its samples first in its row) -> list of bytes per stream; with stats (float32
        only) -> (that list, int32 [n, nframes, 2]: frames / bytes emitted so far after every input frame); with stats and
        crc -> (list, stats, uint16 [n, nframes]: the CRC of the call's bytes up to every input frame)"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.h))
        return self._encode_host(pcm, nfr, stats, crc)

    def encode_host_image(self, image, nframes, stats=False, crc=False):
        """encode_host under pcm_segments: image = the flat PCM image the segments in force address (int16, or float32 at
        int16 scale; any shape), nframes = the call's frames, which no shape gives here.  The device calls take a pointer
        and nframes already: under segments encode_device / submit_device / submit_host get the image's base"""
        return self._encode_host(_pcm_image(image), int(nframes), stats, crc)

    def _encode_host(self, pcm, nfr, stats, crc):
        f32 = pcm.dtype == np.float32
        stride = self.out_stride(nfr)
        out = np.zeros((self.n, stride), dtype=np.uint8)
        nb = np.zeros(self.n, dtype=np.int32)
        if crc and not stats:
            raise TypeError("encode_host(crc=True) needs stats=True (hx_batch_encode_f32_host_crc returns both)")
        if stats:
            if not f32:
                raise TypeError("encode_host(stats=True) takes float32 PCM (hx_batch_encode_f32_host_stats)")
            st = np.zeros((self.n, nfr, 2), dtype=np.int32)
            if crc:
                cr = np.zeros((self.n, nfr), dtype=np.uint16)
                r = lib().hx_batch_encode_f32_host_crc(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data, cr.ctypes.data)
            else:
                r = lib().hx_batch_encode_f32_host_stats(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data)
        else:
            fn = lib().hx_batch_encode_f32_host if f32 else lib().hx_batch_encode_s16_host
            r = fn(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data)
        if r != 0:
            raise RuntimeError("hx_batch_encode host call failed: " + last_error())
        res = [out[i, :nb[i]].tobytes() for i in range(self.n)]
        return (res, st, cr) if crc else (res, st) if stats else res

    def dense_bound(self, nframes):
        """worst-case bytes of a call's dense image"""
        return int(lib().hx_batch_dense_bound(self.h, nframes))

    def dense_buffers(self, d_dense_ptr, dense_cap, d_dense_off_ptr):
        """device buffers [dense_cap] uint8 (16-byte aligned) and [n + 1] int64 that the device calls that follow write
        their dense image and its offsets to (include/hmp3_amd.h, "dense output"); dense_buffers(None, 0, None) switches
        it off"""
        if lib().hx_batch_dense_buffers(self.h, d_dense_ptr, dense_cap, d_dense_off_ptr) != 0:
            raise RuntimeError("hx_batch_dense_buffers failed: " + last_error())

    def encode_host_dense(self, pcm, dense_cap=None):
        """encode_host of which only the dense image crosses the link -> (list of bytes per stream, offsets int64 [n + 1]);
        dense_cap: the image buffer's size (default: dense_bound) - streams whose segment does not fit it come back as None"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.h))
        return self._encode_host_dense(pcm, nfr, dense_cap)

    def encode_host_dense_image(self, image, nframes, dense_cap=None):
        """encode_host_dense under pcm_segments: a flat image plus nframes, as encode_host_image"""
        return self._encode_host_dense(_pcm_image(image), int(nframes), dense_cap)

    def _encode_host_dense(self, pcm, nfr, dense_cap):
        f32 = pcm.dtype == np.float32
        cap = self.dense_bound(nfr) if dense_cap is None else int(dense_cap)
        dense = np.zeros(max(cap, 1), dtype=np.uint8)
        off = np.zeros(self.n + 1, dtype=np.int64)
        nb = np.zeros(self.n, dtype=np.int32)
        fn = lib().hx_batch_encode_f32_host_dense if f32 else lib().hx_batch_encode_s16_host_dense
        if fn(self.h, pcm.ctypes.data, nfr, dense.ctypes.data, cap, off.ctypes.data, nb.ctypes.data) != 0:
            raise RuntimeError("hx_batch_encode host-dense call failed: " + last_error())
        return [dense[off[i]:off[i] + nb[i]].tobytes() if off[i + 1] <= cap else None for i in range(self.n)], off

    def submit_host_dense(self, pcm_ptr, nframes, dense_ptr, dense_cap, dense_off_ptr, out_bytes_ptr, f32=False):
        """pipelined host-dense call: dense / dense_off are page-locked host memory the image kernels write; valid after
        wait_host()"""
        fn = lib().hx_batch_submit_f32_host_dense if f32 else lib().hx_batch_submit_s16_host_dense
        if fn(self.h, pcm_ptr, nframes, dense_ptr, dense_cap, dense_off_ptr, out_bytes_ptr) != 0:
            raise RuntimeError("hx_batch_submit_%s_host_dense failed: " % ("f32" if f32 else "s16") + last_error())

    def encode_device(self, d_pcm_ptr, nframes, d_out_ptr, out_stride, d_out_bytes_ptr, stream=None, f32=False):
        """f32: the PCM is float32 at int16 scale (here and in the submits)"""
        fn = lib().hx_batch_encode_f32_device if f32 else lib().hx_batch_encode_s16_device
        if fn(self.h, d_pcm_ptr, nframes, d_out_ptr, out_stride, d_out_bytes_ptr, stream) != 0:
            raise RuntimeError("hx_batch_encode_%s_device failed: " % ("f32" if f32 else "s16") + last_error())

    def submit_device(self, d_pcm_ptr, nframes, d_out_ptr, out_stride, d_out_bytes_ptr, stream=None, f32=False):
        """pipelined encode_device: outputs are ordered on `stream` by wait()"""
        fn = lib().hx_batch_submit_f32_device if f32 else lib().hx_batch_submit_s16_device
        if fn(self.h, d_pcm_ptr, nframes, d_out_ptr, out_stride, d_out_bytes_ptr, stream) != 0:
            raise RuntimeError("hx_batch_submit_%s_device failed: " % ("f32" if f32 else "s16") + last_error())

    def submit_host(self, pcm_ptr, nframes, out_ptr, out_stride, out_bytes_ptr, f32=False):
        """pipelined host-buffer call; outputs are valid after wait_host()"""
        fn = lib().hx_batch_submit_f32_host if f32 else lib().hx_batch_submit_s16_host
        if fn(self.h, pcm_ptr, nframes, out_ptr, out_stride, out_bytes_ptr) != 0:
            raise RuntimeError("hx_batch_submit_%s_host failed: " % ("f32" if f32 else "s16") + last_error())

    def wait_host(self):
        if lib().hx_batch_wait_host(self.h) != 0:
            raise RuntimeError("hx_batch_wait_host failed: " + last_error())

    def reset_stream(self, i):
        """slot i starts a new stream (same configuration)"""
        if lib().hx_batch_reset_stream(self.h, i) != 0:
            raise RuntimeError("hx_batch_reset_stream failed: " + last_error())

    def get_stream_state(self, i):
        """checkpoint of stream i (bytes)"""
        buf = (C.c_ubyte * int(lib().hx_batch_stream_state_bytes(self.h)))()
        if lib().hx_batch_get_stream_state(self.h, i, buf) != 0:
            raise RuntimeError("hx_batch_get_stream_state failed: " + last_error())
        return bytes(buf)

    def set_stream_state(self, i, state):
        need = int(lib().hx_batch_stream_state_bytes(self.h))
        if len(state) != need:
            raise ValueError("stream state blob has %d bytes, this library's has %d" % (len(state), need))
        buf = (C.c_ubyte * len(state)).from_buffer_copy(state)
        if lib().hx_batch_set_stream_state(self.h, i, buf) != 0:
            raise RuntimeError("hx_batch_set_stream_state failed: " + last_error())

    def states_stride(self):
        """blob_stride of the calls below: the blob size rounded up to 16"""
        return int(lib().hx_batch_stream_states_stride(self.h))

    def _slots(self, idx):
        idx = [int(i) for i in idx]
        return (C.c_int * max(len(idx), 1))(*idx), len(idx)

    def reset_streams(self, idx, stream=None):
        """every slot of idx starts a new stream (same configuration), in one launch, asynchronous on `stream` and ordered
        like a plain device call (hx_batch_reset_streams)"""
        arr, n = self._slots(idx)
        if lib().hx_batch_reset_streams(self.h, arr, n, stream) != 0:
            raise RuntimeError("hx_batch_reset_streams failed: " + last_error())

    def ledger_begin(self, idx, ncalls, head_bytes=0, flags=0, stream=None):
        """slot idx[e] gets a new open file record (hx_batch_ledger_begin): ncalls, head_bytes, flags per slot or one value
        for all; one launch, asynchronous on `stream`, ordered like a plain device call.  It does not reset the encoder"""
        ai, ao, n = _ledger_open_array(idx, ncalls, head_bytes, flags)
        if lib().hx_batch_ledger_begin(self.h, ai, ao, n, stream) != 0:
            raise RuntimeError("hx_batch_ledger_begin failed: " + last_error())

    def ledger_read(self, idx):
        """the records of the slots in idx, synchronous: one gather launch and one copy -> list of Ledger"""
        arr, n = self._slots(idx)
        out = (Ledger * max(n, 1))()
        if lib().hx_batch_ledger_read(self.h, arr, n, out) != 0:
            raise RuntimeError("hx_batch_ledger_read failed: " + last_error())
        return [Ledger.from_buffer_copy(out[e]) for e in range(n)]

    def ledger_read_device(self, idx, d_out_ptr, stream=None):
        """the records into device memory [len(idx)] HX_LEDGER (16-byte aligned), asynchronous on `stream`"""
        arr, n = self._slots(idx)
        if lib().hx_batch_ledger_read_device(self.h, arr, n, d_out_ptr, stream) != 0:
            raise RuntimeError("hx_batch_ledger_read_device failed: " + last_error())

    def file_images(self, cap):
        """file images of cap bytes per slot on, or off with cap = 0 (hx_batch_file_images); refused while a record is live"""
        if lib().hx_batch_file_images(self.h, int(cap)) != 0:
            raise RuntimeError("hx_batch_file_images failed: " + last_error())

    def file_image_cap(self):
        return int(lib().hx_batch_file_image_cap(self.h))

    def file_image_ptr(self, i):
        """the device address of slot i's image (None: images off)"""
        return lib().hx_batch_file_image_ptr(self.h, int(i))

    def ledger_poll(self):
        """the short form of every slot's record, synchronous: one launch, one copy -> list of LedgerBrief"""
        return _ledger_poll(lib().hx_batch_ledger_poll, self.h, self.n)

    def ledger_poll_device(self, d_out_ptr, stream=None):
        """the same into device memory [n] HX_LEDGER_BRIEF (16-byte aligned), asynchronous on `stream`"""
        if lib().hx_batch_ledger_poll_device(self.h, d_out_ptr, stream) != 0:
            raise RuntimeError("hx_batch_ledger_poll_device failed: " + last_error())

    def file_fetch(self, i, cap, fill=0):
        """slot i's file (hx_batch_file_fetch) -> bytes: head_bytes of `fill`, which the call leaves alone, then the audio"""
        return _file_fetch(lib().hx_batch_file_fetch, self.h, i, cap, fill)

    def file_tags(self, idx, tags, stream=None):
        """the tag frame of slot idx[e]'s file, described by the FileTag tags[e], into the head room of its image
        (hx_batch_file_tags): one launch, asynchronous on `stream`, ordered like a plain device call"""
        arr, n = self._slots(idx)
        if lib().hx_batch_file_tags(self.h, arr, _tag_array(tags, n), n, stream) != 0:
            raise RuntimeError("hx_batch_file_tags failed: " + last_error())

    def file_fetch_many(self, idx, cap, fill=0):
        """the files of the slots in idx as one dense image (hx_batch_file_fetch_many) -> (the buffer of cap bytes, pre-filled
        with `fill`, that took the image; off [n + 1]; off[n], the image's size); RuntimeError when the image does not fit cap"""
        buf, off, r = _file_fetch_many(lib().hx_batch_file_fetch_many, self.h, idx, cap, fill)
        if r < 0:
            raise RuntimeError("hx_batch_file_fetch_many failed: " + last_error())
        return buf, off, r

    def file_gather_device(self, idx, d_dst_ptr, dst_cap, d_off_ptr, stream=None):
        """the same image into device memory (16-byte aligned) and its offsets [len(idx) + 1] long long, asynchronous on
        `stream` (hx_batch_file_gather_device)"""
        arr, n = self._slots(idx)
        if lib().hx_batch_file_gather_device(self.h, arr, n, d_dst_ptr, int(dst_cap), d_off_ptr, stream) != 0:
            raise RuntimeError("hx_batch_file_gather_device failed: " + last_error())

    def encode_host_files(self, pcm):
        """encode_host that brings nothing down but the status (hx_batch_encode_*_host_files) -> the status bits"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.h))
        return self._encode_host_files(pcm, nfr)

    def encode_host_files_image(self, image, nframes):
        """encode_host_files under pcm_segments: a flat image plus nframes, as encode_host_image"""
        return self._encode_host_files(_pcm_image(image), int(nframes))

    def _encode_host_files(self, pcm, nfr):
        fn = lib().hx_batch_encode_f32_host_files if pcm.dtype == np.float32 else lib().hx_batch_encode_s16_host_files
        return _files_status(fn.__name__, fn(self.h, pcm.ctypes.data, nfr))

    def get_stream_states(self, idx):
        """checkpoints of the streams in idx, one launch and one copy -> list of bytes, blob e of slot idx[e]"""
        arr, n = self._slots(idx)
        stride, need = self.states_stride(), int(lib().hx_batch_stream_state_bytes(self.h))
        buf = np.zeros(max(n, 1) * stride, dtype=np.uint8)
        if lib().hx_batch_get_stream_states(self.h, arr, n, buf.ctypes.data, stride) != 0:
            raise RuntimeError("hx_batch_get_stream_states failed: " + last_error())
        return [buf[e * stride:e * stride + need].tobytes() for e in range(n)]

    def set_stream_states(self, idx, blobs):
        """blob e continues in slot idx[e]; all slots or (RuntimeError) none"""
        arr, n = self._slots(idx)
        stride, need = self.states_stride(), int(lib().hx_batch_stream_state_bytes(self.h))
        if len(blobs) != n:
            raise ValueError("%d blobs for %d slots" % (len(blobs), n))
        buf = np.zeros(max(n, 1) * stride, dtype=np.uint8)
        for e, blob in enumerate(blobs):
            if len(blob) != need:
                raise ValueError("stream state blob has %d bytes, this library's has %d" % (len(blob), need))
            buf[e * stride:e * stride + need] = np.frombuffer(blob, dtype=np.uint8)
        if lib().hx_batch_set_stream_states(self.h, arr, n, buf.ctypes.data, stride) != 0:
            raise RuntimeError("hx_batch_set_stream_states failed: " + last_error())

    def get_stream_states_device(self, idx, d_blobs_ptr, blob_stride, stream=None):
        """the blobs into device memory [len(idx), blob_stride] (16-byte aligned), asynchronous on `stream`"""
        arr, n = self._slots(idx)
        if lib().hx_batch_get_stream_states_device(self.h, arr, n, d_blobs_ptr, blob_stride, stream) != 0:
            raise RuntimeError("hx_batch_get_stream_states_device failed: " + last_error())

    def set_stream_states_device(self, idx, d_blobs_ptr, blob_stride, stream=None):
        """the reverse; a blob its slot does not take leaves the slot as it was and sets status bit 32"""
        arr, n = self._slots(idx)
        if lib().hx_batch_set_stream_states_device(self.h, arr, n, d_blobs_ptr, blob_stride, stream) != 0:
            raise RuntimeError("hx_batch_set_stream_states_device failed: " + last_error())

    def set_gate(self, percent):
        lib().hx_batch_set_gate(self.h, percent)

    def wait(self, stream=None):
        if lib().hx_batch_wait(self.h, stream) != 0:
            raise RuntimeError("hx_batch_wait failed: " + last_error())

    def status(self):
        return int(lib().hx_batch_status(self.h))

    def k6_variant(self):
        """0 = k_alloc (four streams per CU), 1 = k_alloc_slim (six)"""
        return int(lib().hx_batch_k6_variant(self.h))

    def resident_streams(self):
        return int(lib().hx_batch_resident_streams(self.h))

    def gate_timeouts(self):
        return int(lib().hx_batch_gate_timeouts(self.h))

    def frames_bytes(self, i):
        p = lib().hx_batch_frames_bytes(self.h, i)
        return p.a, p.b

    def alloc_kernel_ms(self):
        n = C.c_int(0)
        ms = lib().hx_batch_alloc_kernel_ms(self.h, C.byref(n))
        return float(ms), n.value

    def debug_enable(self, on=True):
        lib().hx_batch_debug_enable(self.h, 1 if on else 0)

    def debug_read(self, name, dtype, count):
        a = np.zeros(count, dtype=dtype)
        n = lib().hx_batch_debug_read(self.h, name.encode(), a.ctypes.data, a.nbytes)
        if n < 0:
            raise RuntimeError("unknown debug buffer " + name)
        return a[: n // a.itemsize]

    def debug_pcm_rows(self, d_pcm_ptr, nframes, f32=False, stream=None):
        """the row kernel of a call under pcm_segments / pcm_planes alone (hx_batch_debug_pcm_rows): fills the row buffer from
        the device image at d_pcm_ptr and runs nothing behind it; read the rows with debug_read("pcmrows", ...)"""
        if lib().hx_batch_debug_pcm_rows(self.h, d_pcm_ptr, nframes, int(f32), stream) != 0:
            raise RuntimeError("hx_batch_debug_pcm_rows failed: " + last_error())

    def debug_math(self, name, *arrays):
        """the kernels' device function `name` (hx_batch_debug_math) on equally long arrays of 32-bit values, one per
        operand: uint32 [n], the result's 32-bit patterns (view them as float32 or int32); at most 2^25 arguments a call"""
        ops = _math_operands(arrays)
        out = np.zeros(ops.shape[1], dtype=np.uint32)
        if lib().hx_batch_debug_math(self.h, name.encode(), ops.ctypes.data, ops.shape[1], out.ctypes.data) != 0:
            raise RuntimeError("hx_batch_debug_math(%s): %s" % (name, last_error()))
        return out

    def close(self):
        if self.h:
            lib().hx_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SrcBatch(Batch):
    """A converting batch (hx_batch_create_src): N streams whose sources are in any format and at any rate the converter
    takes, converted on the GPU.  controls: what MP3_audio_encode_init takes per stream (samprate = the source's rate,
    mode 3 = a mono source); sources: Source per stream (or one for all)."""

    def __init__(self, controls, sources, nstreams=None, max_frames=256, device=0):
        L = lib()
        if isinstance(controls, EControl):
            self.n = int(nstreams if nstreams is not None else (1 if isinstance(sources, Source) else len(sources)))
            self._ec, ec_arg, shared_ec = controls, C.byref(controls), 1
        else:
            self.n = len(controls)
            self._ec = (EControl * self.n)(*controls)
            ec_arg, shared_ec = self._ec, 0
        if isinstance(sources, Source):
            self._src, src_arg, shared_src = sources, C.byref(sources), 1
        else:
            assert len(sources) == self.n
            self._src = (Source * self.n)(*sources)
            src_arg, shared_src = self._src, 0
        self.h = L.hx_batch_create_src(device, self.n, ec_arg, shared_ec, src_arg, shared_src, max_frames)
        if not self.h:
            raise RuntimeError("hx_batch_create_src failed: " + last_error())
        self.max_frames, self.device = max_frames, int(device)

    @classmethod
    def menu(cls, controls, sources, nstreams, cfg=None, max_frames=256, device=0):
        """a converting batch over a menu whose entry j is the pair (controls[j], sources[j]) (hx_batch_create_menu)"""
        return super().menu(controls, nstreams, cfg=cfg, max_frames=max_frames, device=device, sources=sources)

    @classmethod
    def mixed(cls, controls, sources, nstreams, cfg=None, max_frames=256, device=0):
        """SrcBatch.menu whose entries may differ in the converter's output channels (hx_batch_create_mixed)"""
        return super().mixed(controls, nstreams, cfg=cfg, max_frames=max_frames, device=device, sources=sources)

    @classmethod
    def any(cls, controls, sources, nstreams, cfg=None, max_frames=256, device=0):
        """SrcBatch.mixed whose entries may also differ in the encoder's MPEG version and allocator generation (hx_batch_create_any)"""
        return super().any(controls, nstreams, cfg=cfg, max_frames=max_frames, device=device, sources=sources)

    def schedule(self, i, nframes):
        """(bytes each of stream i's next nframes calls consumes, bytes they read)"""
        nb = np.zeros(nframes, dtype=np.int64)
        rd = int(lib().hx_batch_src_schedule(self.h, i, nframes, nb.ctypes.data))
        if rd < 0:
            raise RuntimeError("hx_batch_src_schedule failed: " + last_error())
        return nb, rd

    def in_stride(self, nframes):
        return int(lib().hx_batch_src_in_stride(self.h, nframes))

    def encode_src_host(self, rows, nframes, frame_off=None, stats=False):
        """rows: uint8 [n, in_stride], row i starting at stream i's first unconsumed byte; frame_off: None or int64
        [n, nframes] byte offsets of each call's input in the row -> (list of bytes per stream, in_used int64 [n]
        [, stats int32 [n, nframes, 2]])"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.shape[0] == self.n
        off = None if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
        stride = self.out_stride(nframes)
        out = np.zeros((self.n, stride), dtype=np.uint8)
        nb = np.zeros(self.n, dtype=np.int32)
        used = np.zeros(self.n, dtype=np.int64)
        st = np.zeros((self.n, nframes, 2), dtype=np.int32) if stats else None
        r = lib().hx_batch_encode_src_host(self.h, rows.ctypes.data, rows.shape[1], None if off is None else off.ctypes.data, nframes,
                                          out.ctypes.data, stride, nb.ctypes.data, used.ctypes.data, None if st is None else st.ctypes.data)
        if r != 0:
            raise RuntimeError("hx_batch_encode_src_host failed: " + last_error())
        res = [out[i, :nb[i]].tobytes() for i in range(self.n)]
        return (res, used, st) if stats else (res, used)


    def encode_src_counts_host(self, rows, nframes, counts, frame_off=None, stats=False, crc=False):
        """encode_src_host under per-stream frame counts: counts = a sequence of n ints (stream i makes the first counts[i]
        calls of the nframes; 0 = it sits the call out, and its row and offsets are not read), or None = all of them; only
        the offsets f < counts[i] are read -> (list of bytes per stream, in_used int64 [n][, stats int32 [n, nframes, 2]]
        [, crc uint16 [n, nframes]]); crc needs stats (hx_batch_encode_src_counts_host)"""
        return _encode_src_counts_host(lib().hx_batch_encode_src_counts_host, self.h, self.n, self.out_stride(nframes), rows, nframes,
                                       counts, frame_off, stats, crc)

    def encode_src_files_host(self, rows, nframes, counts=None, frame_off=None):
        """encode_src_counts_host that brings nothing down but the status (hx_batch_encode_src_files_host)
        -> (the status bits, in_used int64 [n])"""
        return _encode_src_files_host(lib().hx_batch_encode_src_files_host, self.h, self.n, rows, nframes, counts, frame_off)

    def encode_src_counts_device(self, d_in_ptr, in_stride, nframes, counts, d_out_ptr, out_stride, d_out_bytes_ptr, frame_off=None, stream=None):
        """the device call (hx_batch_encode_src_counts_device): counts and frame_off are host arrays as above, the buffers
        device pointers; asynchronous on stream -> in_used int64 [n]"""
        off = None if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
        used = np.zeros(self.n, dtype=np.int64)
        r = lib().hx_batch_encode_src_counts_device(self.h, d_in_ptr, in_stride, None if off is None else off.ctypes.data, nframes,
                                                    _counts_array(self.n, counts), d_out_ptr, out_stride, d_out_bytes_ptr, used.ctypes.data, stream)
        if r != 0:
            raise RuntimeError("hx_batch_encode_src_counts_device failed: " + last_error())
        return used


def src_encode_control(ec, source):
    """the control the encoder runs behind the converter for a source (what MP3_audio_encode_init derives), and the bytes
    per call; (None, 0) when rejected"""
    out = EControl()
    n = int(lib().hx_src_encode_control(C.byref(ec), C.byref(source), C.byref(out)))
    return (out if n else None), n


class Multi:
    """nstreams streams over several GPUs of one node (hx_multi_*): contiguous blocks, one host thread per device"""

    def __init__(self, controls, nstreams=None, max_frames=256, ndev=0, devices=None):
        L = lib()
        dv = (C.c_int * len(devices))(*devices) if devices else None
        if devices:
            ndev = len(devices)
        if isinstance(controls, EControl):
            self.n = int(nstreams)
            self._ec = controls
            self.h = L.hx_multi_create(ndev, dv, self.n, C.byref(controls), 1, max_frames)
        else:
            self.n = len(controls)
            self._ec = (EControl * self.n)(*controls)
            self.h = L.hx_multi_create(ndev, dv, self.n, self._ec, 0, max_frames)
        if not self.h:
            raise RuntimeError("hx_multi_create failed: " + last_error())

    @classmethod
    def menu(cls, controls, nstreams, cfg=None, max_frames=256, ndev=0, devices=None, sources=None):
        """as Batch.menu, in blocks over several devices (hx_multi_create_menu): every block gets the whole menu"""
        return cls._from_menu("hx_multi_create_menu", controls, nstreams, cfg, max_frames, ndev, devices, sources)

    @classmethod
    def mixed(cls, controls, nstreams, cfg=None, max_frames=256, ndev=0, devices=None, sources=None):
        """as Batch.mixed, in blocks over several devices (hx_multi_create_mixed)"""
        return cls._from_menu("hx_multi_create_mixed", controls, nstreams, cfg, max_frames, ndev, devices, sources)

    @classmethod
    def any(cls, controls, nstreams, cfg=None, max_frames=256, ndev=0, devices=None, sources=None):
        """as Batch.any, in blocks over several devices (hx_multi_create_any)"""
        return cls._from_menu("hx_multi_create_any", controls, nstreams, cfg, max_frames, ndev, devices, sources)

    @classmethod
    def _from_menu(cls, create, controls, nstreams, cfg, max_frames, ndev, devices, sources):
        self = cls.__new__(cls)
        dv = (C.c_int * len(devices))(*devices) if devices else None
        if devices:
            ndev = len(devices)
        self.n = int(nstreams)
        self._ec, nmenu, self._src, arr = _menu_args(controls, sources, self.n, cfg)
        self.h = getattr(lib(), create)(ndev, dv, self.n, self._ec, nmenu, self._src, arr, max_frames)
        if not self.h:
            raise RuntimeError(create + " failed: " + last_error())
        return self

    def pcm_channels(self):
        """as Batch.pcm_channels: the same for every block"""
        return int(lib().hx_batch_pcm_channels(self.batch(0)))

    def stream_channels(self, i):
        """channels of the entry stream i (counted over all blocks) runs"""
        for k in range(self.ndevices()):
            _, first, count = self.shard(k)
            if first <= i < first + count:
                return int(lib().hx_batch_stream_channels(self.batch(k), int(i) - first))
        raise IndexError(i)

    def stream_frames_per_block(self, i):
        """frames per 1152-sample block of the entry stream i (counted over all blocks) runs"""
        for k in range(self.ndevices()):
            _, first, count = self.shard(k)
            if first <= i < first + count:
                return int(lib().hx_batch_stream_frames_per_block(self.batch(k), int(i) - first))
        raise IndexError(i)

    def batch(self, k):
        """block k's batch handle, for the per-batch C calls (hx_multi_batch)"""
        return lib().hx_multi_batch(self.h, int(k))

    def nconfigs(self):
        return int(lib().hx_batch_nconfigs(self.batch(0)))

    def stream_config(self, i):
        """the menu entry stream i (counted over all blocks) runs"""
        for k in range(self.ndevices()):
            _, first, count = self.shard(k)
            if first <= i < first + count:
                return int(lib().hx_batch_stream_config(self.batch(k), int(i) - first))
        raise IndexError(i)

    def assign_streams(self, idx, cfg):
        """as Batch.assign_streams over all blocks, synchronous; all blocks or (RuntimeError) none (hx_multi_assign_streams)"""
        ai, ac, n = _int_pair_arrays(idx, cfg)
        if lib().hx_multi_assign_streams(self.h, ai, ac, n) != 0:
            raise RuntimeError("hx_multi_assign_streams failed: " + last_error())

    def ledger_begin(self, idx, ncalls, head_bytes=0, flags=0):
        """as Batch.ledger_begin over all blocks, synchronous; all blocks or (RuntimeError) none (hx_multi_ledger_begin)"""
        ai, ao, n = _ledger_open_array(idx, ncalls, head_bytes, flags)
        if lib().hx_multi_ledger_begin(self.h, ai, ao, n) != 0:
            raise RuntimeError("hx_multi_ledger_begin failed: " + last_error())

    def ledger_read(self, idx):
        """as Batch.ledger_read over all blocks (hx_multi_ledger_read)"""
        idx = [int(i) for i in idx]
        n = len(idx)
        out = (Ledger * max(n, 1))()
        if lib().hx_multi_ledger_read(self.h, (C.c_int * max(n, 1))(*idx), n, out) != 0:
            raise RuntimeError("hx_multi_ledger_read failed: " + last_error())
        return [Ledger.from_buffer_copy(out[e]) for e in range(n)]

    def file_images(self, cap):
        """as Batch.file_images over all blocks; all blocks or (RuntimeError) none (hx_multi_file_images)"""
        if lib().hx_multi_file_images(self.h, int(cap)) != 0:
            raise RuntimeError("hx_multi_file_images failed: " + last_error())

    def ledger_poll(self):
        """as Batch.ledger_poll over all blocks (hx_multi_ledger_poll)"""
        return _ledger_poll(lib().hx_multi_ledger_poll, self.h, self.n)

    def file_fetch(self, i, cap, fill=0):
        """as Batch.file_fetch, i over all blocks (hx_multi_file_fetch)"""
        return _file_fetch(lib().hx_multi_file_fetch, self.h, i, cap, fill)

    def file_tags(self, idx, tags):
        """as Batch.file_tags over all blocks, synchronous (hx_multi_file_tags)"""
        idx = [int(i) for i in idx]
        n = len(idx)
        if lib().hx_multi_file_tags(self.h, (C.c_int * max(n, 1))(*idx), _tag_array(tags, n), n) != 0:
            raise RuntimeError("hx_multi_file_tags failed: " + last_error())

    def file_fetch_many(self, idx, cap, fill=0):
        """as Batch.file_fetch_many, idx over all blocks (hx_multi_file_fetch_many)"""
        buf, off, r = _file_fetch_many(lib().hx_multi_file_fetch_many, self.h, idx, cap, fill)
        if r < 0:
            raise RuntimeError("hx_multi_file_fetch_many failed: " + last_error())
        return buf, off, r

    def encode_host_files(self, pcm):
        """as Batch.encode_host_files, over all streams"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.batch(0)))
        return self._encode_host_files(pcm, nfr)

    def encode_host_files_image(self, image, nframes):
        """as Batch.encode_host_files_image, over all streams"""
        return self._encode_host_files(_pcm_image(image), int(nframes))

    def _encode_host_files(self, pcm, nfr):
        fn = lib().hx_multi_encode_f32_host_files if pcm.dtype == np.float32 else lib().hx_multi_encode_s16_host_files
        return _files_status(fn.__name__, fn(self.h, pcm.ctypes.data, nfr))

    def ndevices(self):
        return int(lib().hx_multi_ndevices(self.h))

    def shard(self, k):
        d, f, c = C.c_int(), C.c_int(), C.c_int()
        if lib().hx_multi_shard(self.h, k, C.byref(d), C.byref(f), C.byref(c)) != 0:
            raise IndexError(k)
        return d.value, f.value, c.value

    def frame_counts(self, counts):
        """as Batch.frame_counts, over all streams (hx_multi_frame_counts)"""
        _frame_counts(lib().hx_multi_frame_counts, self.h, self.n, counts)
        self._counts = None if counts is None else [int(c) for c in counts]

    def pcm_segments(self, off, in_bytes=0):
        """as Batch.pcm_segments, over all streams: the offsets address the caller's one image (hx_multi_pcm_segments)"""
        _pcm_segments(lib().hx_multi_pcm_segments, self.h, self.n, off, in_bytes)

    def pcm_planes(self, off, chan_stride=None, in_bytes=0, unit_scale=False):
        """as Batch.pcm_planes, over all streams: offsets and strides address the caller's one image (hx_multi_pcm_planes)"""
        _pcm_planes(lib().hx_multi_pcm_planes, self.h, self.n, off, chan_stride, in_bytes, unit_scale)

    def packed_layout(self, nframes, f32=False):
        """as Batch.packed_layout, over all streams"""
        return packed_layout(nframes, [self.stream_channels(i) for i in range(self.n)], getattr(self, "_counts", None), f32)

    def encode_host(self, pcm, stats=False, crc=False):
        """as Batch.encode_host, over all streams"""
        pcm, nfr = _pcm_rows(pcm, self.n, _pitch(self.batch(0)))
        return self._encode_host(pcm, nfr, stats, crc)

    def encode_host_image(self, image, nframes, stats=False, crc=False):
        """as Batch.encode_host_image, over all streams"""
        return self._encode_host(_pcm_image(image), int(nframes), stats, crc)

    def _encode_host(self, pcm, nfr, stats, crc):
        f32 = pcm.dtype == np.float32
        stride = int(lib().hx_multi_out_stride(self.h, nfr))
        out = np.zeros((self.n, stride), dtype=np.uint8)
        nb = np.zeros(self.n, dtype=np.int32)
        if crc and not stats:
            raise TypeError("encode_host(crc=True) needs stats=True (hx_multi_encode_f32_host_crc returns both)")
        if stats:
            if not f32:
                raise TypeError("encode_host(stats=True) takes float32 PCM (hx_multi_encode_f32_host_stats)")
            st = np.zeros((self.n, nfr, 2), dtype=np.int32)
            if crc:
                cr = np.zeros((self.n, nfr), dtype=np.uint16)
                r = lib().hx_multi_encode_f32_host_crc(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data, cr.ctypes.data)
            else:
                r = lib().hx_multi_encode_f32_host_stats(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data)
        else:
            fn = lib().hx_multi_encode_f32_host if f32 else lib().hx_multi_encode_s16_host
            r = fn(self.h, pcm.ctypes.data, nfr, out.ctypes.data, stride, nb.ctypes.data)
        if r != 0:
            raise RuntimeError("hx_multi_encode host call failed: " + last_error())
        res = [out[i, :nb[i]].tobytes() for i in range(self.n)]
        return (res, st, cr) if crc else (res, st) if stats else res

    def status(self):
        return int(lib().hx_multi_status(self.h))

    def close(self):
        if self.h:
            lib().hx_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SrcMulti(Multi):
    """converting batches over several GPUs of one node (hx_multi_create_src): contiguous blocks, one host thread per device"""

    def __init__(self, controls, sources, max_frames=256, ndev=0, devices=None):
        L = lib()
        dv = (C.c_int * len(devices))(*devices) if devices else None
        if devices:
            ndev = len(devices)
        self.n = len(controls)
        assert len(sources) == self.n
        self._ec = (EControl * self.n)(*controls)
        self._src = (Source * self.n)(*sources)
        self.h = L.hx_multi_create_src(ndev, dv, self.n, self._ec, 0, self._src, 0, max_frames)
        if not self.h:
            raise RuntimeError("hx_multi_create_src failed: " + last_error())

    @classmethod
    def menu(cls, controls, sources, nstreams, cfg=None, max_frames=256, ndev=0, devices=None):
        """as SrcBatch.menu, in blocks over several devices"""
        return super().menu(controls, nstreams, cfg=cfg, max_frames=max_frames, ndev=ndev, devices=devices, sources=sources)

    @classmethod
    def mixed(cls, controls, sources, nstreams, cfg=None, max_frames=256, ndev=0, devices=None):
        """as SrcBatch.mixed, in blocks over several devices"""
        return super().mixed(controls, nstreams, cfg=cfg, max_frames=max_frames, ndev=ndev, devices=devices, sources=sources)

    @classmethod
    def any(cls, controls, sources, nstreams, cfg=None, max_frames=256, ndev=0, devices=None):
        """as SrcBatch.any, in blocks over several devices"""
        return super().any(controls, nstreams, cfg=cfg, max_frames=max_frames, ndev=ndev, devices=devices, sources=sources)

    def in_stride(self, nframes):
        return int(lib().hx_multi_src_in_stride(self.h, nframes))

    def encode_src_host(self, rows, nframes, frame_off=None):
        """as SrcBatch.encode_src_host, over all streams -> (list of bytes per stream, in_used int64 [n])"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        off = None if frame_off is None else np.ascontiguousarray(frame_off, dtype=np.int64)
        stride = int(lib().hx_multi_out_stride(self.h, nframes))
        out = np.zeros((self.n, stride), dtype=np.uint8)
        nb = np.zeros(self.n, dtype=np.int32)
        used = np.zeros(self.n, dtype=np.int64)
        r = lib().hx_multi_encode_src_host(self.h, rows.ctypes.data, rows.shape[1], None if off is None else off.ctypes.data, nframes,
                                           out.ctypes.data, stride, nb.ctypes.data, used.ctypes.data, None)
        if r != 0:
            raise RuntimeError("hx_multi_encode_src_host failed: " + last_error())
        return [out[i, :nb[i]].tobytes() for i in range(self.n)], used

    def encode_src_files_host(self, rows, nframes, counts=None, frame_off=None):
        """as SrcBatch.encode_src_files_host, over all streams (hx_multi_encode_src_files_host)"""
        return _encode_src_files_host(lib().hx_multi_encode_src_files_host, self.h, self.n, rows, nframes, counts, frame_off)

    def encode_src_counts_host(self, rows, nframes, counts, frame_off=None, stats=False, crc=False):
        """as SrcBatch.encode_src_counts_host, over all streams (hx_multi_encode_src_counts_host)"""
        return _encode_src_counts_host(lib().hx_multi_encode_src_counts_host, self.h, self.n, int(lib().hx_multi_out_stride(self.h, nframes)),
                                       rows, nframes, counts, frame_off, stats, crc)


class Mp3Enc:
    """Same surface as the reference's CMp3Enc (pub/mp3enc.h:74-139), one stream."""

    def __init__(self, device=0):
        self.h = lib().hx_enc_create(device)
        self._out = (C.c_ubyte * (1 << 17))()

    def L3_audio_encode_init(self, ec):
        return lib().hx_enc_L3_audio_encode_init(self.h, C.byref(ec))

    def MP3_audio_encode_init(self, ec, source_bits=16, source_is_float=0, mpeg_select=0, mono_convert=0):
        return lib().hx_enc_MP3_audio_encode_init(self.h, C.byref(ec), source_bits, source_is_float, mpeg_select, mono_convert)

    def L3_audio_encode(self, pcm_f32):
        pcm = np.ascontiguousarray(pcm_f32, dtype=np.float32)
        x = lib().hx_enc_L3_audio_encode(self.h, pcm.ctypes.data, self._out)
        return x.in_bytes, bytes(self._out[: x.out_bytes])

    def L3_audio_encode_Packet(self, pcm_f32):
        """-> (in_bytes, bitstream bytes, packet bytes); self.packet_sizes = nbytes_out[2] (MPEG-2: two packets)"""
        pcm = np.ascontiguousarray(pcm_f32, dtype=np.float32)
        pk = (C.c_ubyte * 4096)()
        nb = (C.c_int * 2)()
        x = lib().hx_enc_L3_audio_encode_Packet(self.h, pcm.ctypes.data, self._out, pk, nb)
        self.packet_sizes = (nb[0], nb[1])
        return x.in_bytes, bytes(self._out[: x.out_bytes]), bytes(pk[: nb[0] + nb[1]])

    def _packet_call(self, fn, pcm_ptr, bs_out, packet):
        """a *_Packet call; bs_out / packet False: that argument NULL (its part of the result is then None)"""
        pk = (C.c_ubyte * 4096)() if packet else None
        nb = (C.c_int * 2)(-1, -1)
        x = fn(self.h, pcm_ptr, self._out if bs_out else None, pk, nb)
        self.packet_sizes = (nb[0], nb[1])      # (left at -1, -1 by a call without a packet)
        return x.in_bytes, x.out_bytes, bytes(self._out[: x.out_bytes]) if bs_out else None, bytes(pk[: nb[0] + nb[1]]) if packet else None

    def MP3_audio_encode(self, pcm_i16):
        pcm = np.ascontiguousarray(pcm_i16, dtype=np.int16)
        x = lib().hx_enc_MP3_audio_encode(self.h, pcm.ctypes.data, self._out)
        return x.in_bytes, bytes(self._out[: x.out_bytes])

    def MP3_audio_encode_Packet(self, data, bs_out=True, packet=True):
        """data: the source's bytes from the first unconsumed one, in the source's format: bytes (copied), or whatever ctypes
        takes for a pointer, such as byref(buffer, position)
        -> (in_bytes, out_bytes, bitstream bytes or None, packet bytes or None); self.packet_sizes = nbytes_out[2]"""
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data) if isinstance(data, (bytes, bytearray)) else data
        return self._packet_call(lib().hx_enc_MP3_audio_encode_Packet, buf, bs_out, packet)

    def L3_audio_encode_Packet_opt(self, pcm_f32, bs_out=True, packet=True):
        """L3_audio_encode_Packet whose bs_out or packet argument may be NULL
        -> (in_bytes, out_bytes, bitstream bytes or None, packet bytes or None)"""
        pcm = np.ascontiguousarray(pcm_f32, dtype=np.float32)
        return self._packet_call(lib().hx_enc_L3_audio_encode_Packet, pcm.ctypes.data, bs_out, packet)

    def debug_calls(self):
        """(calls made the plain way, calls replayed from the recorded graph, the graph's state) since the last init
        (hx_enc_debug_calls)"""
        out = (C.c_int * 3)()
        if lib().hx_enc_debug_calls(self.h, out) != 0:
            raise RuntimeError("hx_enc_debug_calls failed")
        return out[0], out[1], out[2]

    def L3_audio_encode_get_frames(self):
        return int(lib().hx_enc_get_frames(self.h))

    def L3_audio_encode_get_bitrate(self):
        return int(lib().hx_enc_get_bitrate(self.h))

    def L3_audio_encode_get_bitrate_float(self):
        return float(lib().hx_enc_get_bitrate_float(self.h))

    def L3_audio_encode_get_bitrate2_float(self):
        return float(lib().hx_enc_get_bitrate2_float(self.h))

    def L3_audio_encode_get_frames_bytes(self):
        p = lib().hx_enc_get_frames_bytes(self.h)
        return p.a, p.b

    def L3_audio_encode_info_ec(self):
        ec = EControl()
        lib().hx_enc_info_ec(self.h, C.byref(ec))
        return ec

    def L3_audio_encode_info_head(self):
        h = MpegHead()
        lib().hx_enc_info_head(self.h, C.byref(h))
        return h

    def L3_audio_encode_info_string(self):
        s = C.create_string_buffer(160)
        lib().hx_enc_info_string(self.h, s)
        return s.value.decode()

    def close(self):
        if self.h:
            lib().hx_enc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
