"""The sources of the converting-batch tests (tests/test_gpu_src_batch.py, tests/test_gpu_src_counts.py and the suites that
put a converting batch through their own feature): one source with its control, HX_SOURCE and bytes, the reference's
MP3_audio_encode loop and converter on it (oracle/_ref/libhmp3ref.so), this library's per-frame encoder, and the rows of a
converting call."""
import ctypes as C

import numpy as np

from hmp3_amd import api
from oracle import oracle as O


def ref():
    R = O.ref()
    R.ref_src_new.restype = C.c_void_p
    R.ref_src_free.argtypes = [C.c_void_p]
    R.ref_src_init.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    R.ref_src_convert.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    R.ref_init_mp3.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    R.ref_encode_mp3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return R


def source_data(x, bits, is_float):
    """float signal in [-1, 1) (interleaved) -> the source format's bytes"""
    if is_float:
        return x.astype("<f4").tobytes()
    if bits == 8:
        return np.clip(np.round(x * 127 + 128), 0, 255).astype(np.uint8).tobytes()
    if bits == 16:
        return np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes()
    v = np.clip(np.round(x * 2147483647.0), -2 ** 31, 2 ** 31 - 1).astype("<i4")
    if bits == 32:
        return v.tobytes()
    b = v.view(np.uint8).reshape(-1, 4)
    return b[:, 1:].tobytes()


def source_signal(seed, nsamp, channels, noise=False):
    rng = np.random.default_rng(seed)
    if noise:
        return rng.uniform(-1, 1, nsamp * channels)
    t = np.arange(nsamp)[:, None]
    f = rng.uniform(100, 3000, (1, channels))
    x = 0.4 * np.sin(2 * np.pi * f * t / 32000.0) + 0.05 * rng.standard_normal((nsamp, channels))
    x[nsamp // 3:nsamp // 3 + 300] *= 2.0        # an onset
    return np.clip(x, -1, 0.999).reshape(-1)


class Stream:
    """one source: its control (samprate = source rate), its HX_SOURCE and its bytes"""

    def __init__(self, source, bits, is_float, channels=2, mpeg_select=0, mono_convert=0, seed=0, seconds=3.0, noise=False, **kw):
        self.ec = api.default_control(**({"bitrate": 64} | kw))
        self.ec.samprate = source
        if channels == 1:
            self.ec.mode = 3
        self.src = api.Source(bits, is_float, mpeg_select, mono_convert)
        self.channels, self.bits, self.is_float, self.source = channels, bits, is_float, source
        self.mono_convert, self.mpeg_select = mono_convert, mpeg_select
        n = int(source * seconds)
        self.data = source_data(source_signal(seed, n, channels, noise), bits, is_float) + bytes(1 << 18)
        self.fb = channels * bits // 8

    def reference(self, nframes, offsets=None):
        """the reference's MP3_audio_encode loop: bytes, sum of in_bytes (offsets: the pointer of every call)"""
        R = ref()
        h = R.ref_new()
        e = api.EControl()
        C.memmove(C.byref(e), C.byref(self.ec), C.sizeof(e))
        assert R.ref_init_mp3(h, C.byref(e), self.bits, self.is_float, self.src.mpeg_select, self.src.mono_convert) > 0
        buf = (C.c_ubyte * len(self.data)).from_buffer_copy(self.data)
        out = (C.c_ubyte * 65536)()
        res, pos, used = b"", 0, C.c_int(0)
        for f in range(nframes):
            p = pos if offsets is None else int(offsets[f])
            n = R.ref_encode_mp3(h, C.byref(buf, p), out, C.byref(used))
            res += bytes(out[:n])
            pos = p + used.value
        R.ref_free(h)
        return res, pos

    def per_frame(self, nframes):
        """this library's one-stream MP3_audio_encode: bytes, sum of in_bytes"""
        L = api.lib()
        e = api.Mp3Enc()
        assert e.MP3_audio_encode_init(self.ec, self.bits, self.is_float, self.src.mpeg_select, self.src.mono_convert) > 0
        buf = (C.c_ubyte * len(self.data)).from_buffer_copy(self.data)
        res, pos = b"", 0
        for _ in range(nframes):
            x = L.hx_enc_MP3_audio_encode(e.h, C.byref(buf, pos), e._out)
            res += bytes(e._out[:x.out_bytes])
            pos += x.in_bytes
        e.close()
        return res, pos


def make_batch(streams, max_frames):
    return api.SrcBatch([s.ec for s in streams], [s.src for s in streams], max_frames=max_frames)


def make_rows(b, streams, pos, nf, counts, garbage=None, extra=0):
    """the call's rows, row i from stream i's first unconsumed byte; garbage: that byte over everything beyond what the
    stream's counts[i] calls read (the whole row of a stream that sits the call out)"""
    stride = b.in_stride(nf) + extra
    rows = np.zeros((len(streams), stride), np.uint8)
    for i, s in enumerate(streams):
        chunk = np.frombuffer(s.data[pos[i]:pos[i] + stride], np.uint8)
        rows[i, :len(chunk)] = chunk
        if garbage is not None:
            rd = b.schedule(i, counts[i])[1] if counts[i] else 0
            rows[i, rd:] = garbage
    return rows


def run(b, streams, calls, pos=None, taps=False):
    """consecutive calls of the given frame counts; rows start at each stream's first unconsumed byte"""
    pos = [0] * len(streams) if pos is None else pos
    outs = [b""] * len(streams)
    pcm = []
    for nf in calls:
        res, used = b.encode_src_host(make_rows(b, streams, pos, nf, None), nf)
        assert b.status() == 0
        if taps:
            pcm.append(b.debug_read("srcpcm", np.float32, len(streams) * nf * 1152 * 2).reshape(len(streams), nf * 1152, -1))
        for i in range(len(streams)):
            outs[i] += res[i]
            pos[i] += int(used[i])
    return outs, pos, pcm


def ref_converted(s, target, nframes):
    """the reference's Csrc over nframes calls: [nframes * 1152][target channels] float32"""
    R = ref()
    tch = 1 if (s.channels == 1 or s.mono_convert) else 2
    h = R.ref_src_new()
    cut = C.c_int(0)
    assert R.ref_src_init(h, s.source, s.channels, s.bits, s.is_float, target, tch, C.byref(cut)) > 0
    buf = (C.c_ubyte * len(s.data)).from_buffer_copy(s.data)
    ys, pos, ob = [], 0, C.c_int(0)
    for _ in range(nframes):
        y = np.zeros(2304, np.float32)
        pos += R.ref_src_convert(h, C.byref(buf, pos), y.ctypes.data, C.byref(ob))
        ys.append(y[:1152 * tch].reshape(1152, tch))
    R.ref_src_free(h)
    return np.concatenate(ys)


def host_converted(s, nframes, target=None):
    """this library's host converter over the source's first nframes calls -> (float32 [nframes * 1152(, 2)], bytes used per
    call, channels); target: the encode rate (None: the source's mpeg_select where it is a rate, else the source's rate; a
    source whose mpeg_select is 1 or 2 - "an MPEG-1 / MPEG-2 rate" - passes the rate api.src_encode_control derives)"""
    L = api.lib()
    tch = 1 if (s.channels == 1 or s.mono_convert) else 2
    h = L.hx_src_create()
    cut = C.c_int(0)
    assert L.hx_src_init(h, s.source, s.channels, s.bits, s.is_float, target or s.mpeg_select or s.source, tch, C.byref(cut)) > 0
    buf = (C.c_ubyte * len(s.data)).from_buffer_copy(s.data)
    ys, used, pos = [], [], 0
    for _ in range(nframes):
        y = np.zeros(2304, np.float32)
        n = L.hx_src_convert(h, C.byref(buf, pos), y.ctypes.data, None)
        used.append(n)
        pos += n
        ys.append(y[:1152 * tch])
    L.hx_src_destroy(h)
    y = np.concatenate(ys)
    return (y if tch == 1 else y.reshape(-1, 2)), used, tch
