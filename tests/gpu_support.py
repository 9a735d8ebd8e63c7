"""The scaffolding the GPU tests share, each piece once: paths, the device handles, the host's CRC and the oracle's bytes, the
device output buffers of one call (CallBufs, Image), the device call into them, page-locked host arrays and the command
line's batch run against its single-file runs.  A plain module beside the tests (tests/ is on sys.path); no test module is
imported by another.  torch is imported inside the functions that need it, so collecting the CPU suite does not pay for it.

What belongs to one feature's contract - what a call's outputs must equal - stays with that feature's tests (or, where
several suites assert it, in tests/output_checks.py) and takes the buffers as an argument."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np

from hmp3_amd import api
from oracle import oracle as O
from stage_taps import bits  # noqa: F401  (the one definition; re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "hmp3_amd", "hmp3amd")
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "hmp3")
SHIM_CLI = os.path.join(ROOT, "oracle", "_ref", "hmp3_on_amd")
sys.path.insert(0, GOLD)
import make_golden_cli as GOLDEN_CLI  # noqa: E402
from make_golden_cli import write_wav  # noqa: E402,F401  (path, int16 PCM, rate, False s16 | True f32 | 8 / 24 / 32, container)

FILL = 0xA5
CURRENT = "current"         # device_call(stream=CURRENT): torch's current stream


def dev():
    import torch
    return torch.device("cuda:0")


def sync():
    import torch
    torch.cuda.synchronize()


def cur_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def hip():
    """the HIP runtime the library runs on (the copy the process has mapped), for copies from and to an image's address"""
    api.lib()
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            h = C.CDLL(line.split()[-1])
            h.hipMemcpy.argtypes, h.hipMemset.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p, C.c_int, C.c_size_t]
            return h
    raise RuntimeError("no HIP runtime mapped")


def host_crc(data, seed=0):
    data = bytes(data)
    return int(api.lib().hx_xing_update_crc(seed, data, len(data)))


def oracle_bytes(kw, pcm, nfr=None):
    """the oracle's bytes for the first nfr frames of one stream's int16 PCM (None: all whole frames)"""
    enc = O.OracleEncoder(O.default_control(**kw))
    return b"".join(enc.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(len(pcm) // 1152 if nfr is None else nfr))


def controls(menu):
    return [api.default_control(**kw) for kw in menu]


def cut(pcm, f0, nf):
    return np.ascontiguousarray(pcm[:, f0 * 1152:(f0 + nf) * 1152])


def ints(v):
    return (C.c_int * max(len(v), 1))(*v), len(v)


def states(b, idx=None, single=False):
    """the checkpoint blobs of the listed slots (None: all) through hx_batch_get_stream_states, or - single - through one
    hx_batch_get_stream_state per slot: different calls of the ABI, and a test keeps the one it is about"""
    idx = range(b.n) if idx is None else idx
    return [b.get_stream_state(i) for i in idx] if single else b.get_stream_states(idx)


# ---- the device output buffers of one call ----

class Image:
    """a prefilled dense image of `cap` bytes with a guard region behind it, and its offsets"""

    def __init__(self, S, cap, fill=FILL, guard=4096):
        import torch
        self.cap, self.fill, self.guard = int(cap), fill, guard
        self.buf = torch.full((self.cap + guard + 16,), fill, dtype=torch.uint8, device=dev())
        self.o = (-self.buf.data_ptr()) % 16
        self.off = torch.full((S + 1,), -1, dtype=torch.int64, device=dev())
        self.ptr = self.buf.data_ptr() + self.o

    def set_on(self, b):
        b.dense_buffers(self.ptr, self.cap, self.off.data_ptr())

    def prefill(self):
        """(again: the same buffers for a further call, the batch's setter untouched)"""
        self.buf.fill_(self.fill)
        self.off.fill_(-1)
        sync()

    def host(self):
        return self.buf.cpu().numpy()[self.o:self.o + self.cap + self.guard], self.off.cpu().numpy()


class CallBufs:
    """every device output buffer of one call, prefilled.  Rows and byte counts (-1) always; the rest as asked for:
    rows_fill        what the rows hold before the call
    shift, extra     the first row `shift` bytes past a 16-byte boundary, `extra` bytes added to hx_batch_out_stride
    counters, odd    frame counters [S][nf][2] of -1; odd: starting 4 bytes past an 8-byte boundary
    crc              per-frame CRCs [S][nf], prefilled with the 16-bit value crc_fill, crc_guard more entries behind them
    packets          the packets' frame_stride: packets [S][nf][frame_stride] of pk_fill and their sizes [S][nf][2] of -1
    image            an Image, set with the rest"""

    def __init__(self, b, nf, rows_fill=0, shift=0, extra=0, counters=False, odd=False, crc=False, crc_fill=0xFFFF, crc_guard=0,
                 packets=None, pk_fill=FILL, image=None):
        import torch
        d = dev()
        self.S, self.nf, self.stride, self.rows_fill = b.n, nf, b.out_stride(nf) + extra, rows_fill
        self.buf = torch.empty(self.S * self.stride + 64, dtype=torch.uint8, device=d)
        self.o = (-self.buf.data_ptr()) % 16 + shift
        self.ptr = self.buf.data_ptr() + self.o
        self.out = self.buf[self.o:self.o + self.S * self.stride].view(self.S, self.stride)
        self.nb = torch.empty((self.S,), dtype=torch.int32, device=d)
        self.stats = self.crc = self.pk = self.pkb = None
        if counters:
            self.stats = torch.empty((self.S * nf * 2 + 2,), dtype=torch.int32, device=d)[2 - int(odd):][:self.S * nf * 2].view(self.S, nf, 2)
            assert self.stats.data_ptr() % 8 == 4 * int(odd)
        if crc:
            self.crc, self.crc_fill = torch.empty((self.S * nf + crc_guard,), dtype=torch.int16, device=d), crc_fill - 65536 * (crc_fill >= 32768)
        if packets:
            self.frame_stride, self.pk_fill = packets, pk_fill
            self.pk = torch.empty((self.S, nf, packets), dtype=torch.uint8, device=d)
            self.pkb = torch.empty((self.S, nf, 2), dtype=torch.int32, device=d)
        self.image = image
        self.prefill(image=False)

    def prefill(self, image=True):
        """(again: the same buffers for a further call, the batch's setters untouched)"""
        self.buf.fill_(self.rows_fill)
        for t in (self.nb, self.stats, self.pkb):
            if t is not None:
                t.fill_(-1)
        if self.crc is not None:
            self.crc.fill_(self.crc_fill)
        if self.pk is not None:
            self.pk.fill_(self.pk_fill)
        if image and self.image is not None:
            self.image.prefill()
        sync()

    def set_on(self, b, stats=True, crc=True, packets=True, image=True):
        """the setters of every buffer this object has (a switch that is False: that output off, a null pointer); -> self"""
        if self.pk is not None:
            b.packet_buffers(*((self.pk.data_ptr(), self.frame_stride, self.pkb.data_ptr()) if packets else (None, 0, None)))
        if self.stats is not None:
            b.frame_stats_buffer(self.stats.data_ptr() if stats else None)
        if self.crc is not None:
            b.crc_buffer(self.crc.data_ptr() if crc else None)
        if self.image is not None and image:
            self.image.set_on(b)
        return self

    def rows(self):
        return self.out.cpu().numpy(), self.nb.cpu().numpy()

    def host(self):
        """rows, nb, then what there is of: counters, CRCs [S, nf] as uint16, the CRC buffer's guard region"""
        res = self.rows()
        if self.stats is not None:
            res += (self.stats.cpu().numpy(),)
        if self.crc is not None:
            c, n = self.crc.cpu().numpy().view(np.uint16), self.S * self.nf
            res += (c[:n].reshape(self.S, self.nf),) + ((c[n:],) if len(c) > n else ())
        return res

    def packets(self):
        """packets, their sizes, the frame counters"""
        return self.pk.cpu().numpy(), self.pkb.cpu().numpy(), self.stats.cpu().numpy()

    def bitstreams(self):
        o, n = self.rows()
        assert (n >= 0).all(), "a byte count was not written"
        return [o[s, :n[s]].tobytes() for s in range(len(n))]


def device_call(b, pcm, nf, bufs, submit=False, stream=CURRENT, f32=None, shift=0):
    """upload the call's PCM (`shift` elements past a 16-byte boundary), synchronise, and make the device call - or the
    submit - into bufs, on torch's current stream or the one given (None: the null stream).  Neither waited for nor checked.
    -> bufs, which keeps the device PCM alive (bufs.keep) and knows its address (bufs.pcm_ptr)"""
    import torch
    flat = np.array(pcm).reshape(-1)            # (a copy: shared signals are read-only)
    d_pcm = torch.zeros(flat.size + 16, dtype=torch.from_numpy(flat[:0]).dtype, device=dev())
    assert d_pcm.data_ptr() % 16 == 0
    d_pcm[shift:shift + flat.size] = torch.from_numpy(flat).to(dev())
    bufs.keep, bufs.pcm_ptr = d_pcm, d_pcm.data_ptr() + shift * flat.itemsize
    sync()
    (b.submit_device if submit else b.encode_device)(bufs.pcm_ptr, nf, bufs.ptr, bufs.stride, bufs.nb.data_ptr(), cur_stream() if stream == CURRENT else stream,
                                                     f32=flat.dtype == np.float32 if f32 is None else f32)
    return bufs


def plain_call(b, pcm, nf, shift=0):
    """a plain device call on the null stream into zeroed rows, waited for -> (the streams' bytes, the PCM's device address)"""
    o = device_call(b, pcm, nf, CallBufs(b, nf), stream=None, shift=shift)
    sync()
    return o.bitstreams(), o.pcm_ptr


# ---- page-locked host memory ----

class Pinned:
    """page-locked host arrays from hx_pinned_alloc, until free()"""

    def __init__(self):
        self.ptrs = []

    def array(self, n, dtype, fill):
        nbytes = int(n) * np.dtype(dtype).itemsize
        p = api.lib().hx_pinned_alloc(max(nbytes, 16))
        assert p
        self.ptrs.append(p)
        a = np.frombuffer((C.c_ubyte * nbytes).from_address(p), dtype=dtype)
        a[:] = fill
        return a

    def copy(self, arr):
        """a copy of arr in page-locked memory"""
        v = self.array(arr.size, arr.dtype, 0).reshape(arr.shape)
        v[...] = arr
        return v

    def free(self):
        while self.ptrs:
            api.lib().hx_pinned_free(self.ptrs.pop())


# ---- the command line ----

def run_cli(args, exe=CLI, **kw):
    """hmp3amd (or exe) on args; it must end with 0 -> the finished process"""
    assert os.path.exists(exe), "hmp3_amd/build.sh builds the CLI"
    r = subprocess.run([exe] + list(args), capture_output=True, **dict(dict(timeout=120), **kw))
    assert r.returncode == 0, r.stderr.decode()[-400:]
    return r


def batch_vs_single_vs_reference(files, flags=(), slots=(), floor=-1, single=True, reference=True):
    """`hmp3amd -batch [slots] wav out ... flags` on files [(label, wav, out)]: every output has more than `floor` bytes and
    is byte for byte the file's single-file run and, where oracle/_ref/hmp3 is built, the reference binary's
    -> (the batch run's stderr, the outputs' bytes)"""
    flags = list(flags)
    r = run_cli(["-batch"] + list(slots) + [p for _, wav, out in files for p in (wav, out)] + flags)
    got = []
    for label, wav, out in files:
        data = open(out, "rb").read()
        assert len(data) > floor, label
        if single:
            run_cli([wav, out + ".single"] + flags)
            want = open(out + ".single", "rb").read()
            assert data == want, "%s: differs from its single-file run (first at byte %d)" % (
                label, next((k for k in range(min(len(data), len(want))) if data[k] != want[k]), -1))
        if reference and os.path.exists(REF_CLI):
            subprocess.run([REF_CLI, wav, out + ".ref"] + flags, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
            assert data == open(out + ".ref", "rb").read(), "%s: differs from the reference binary's output" % label
        got.append(data)
    return r.stderr.decode(), got
