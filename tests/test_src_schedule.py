"""The converter's schedule and the encode control of converted sources (host only, no GPU).

hx_src_schedule states in closed form what the stepping converter (hmp3_amd/csrc/hx_src.cpp, pinned to the reference's
Csrc by test_src_convert.py) consumes and reads per call; the converting batch computes every call's input extent from it.
hx_src_encode_control is the derivation that hx_enc_MP3_audio_encode_init and the converting batch share, checked against
what the reference's own MP3_audio_encode_init leaves behind.  Skipped where oracle/_ref has not been built."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.skipif(O.ref() is None, reason="oracle/_ref not built")

# the pairs of test_src_convert.py and two more up-sampling ones
PAIRS = [(44100, 44100), (11025, 22050), (8000, 16000), (12000, 16000), (11025, 16000), (32000, 44100), (22050, 24000),
         (48000, 24000), (44100, 22050), (48000, 32000), (24000, 16000), (44100, 32000), (48000, 44100), (44100, 24000),
         (32000, 22050), (8000, 22050), (16000, 24000)]
LAYOUTS = [(1, 1), (2, 2), (2, 1)]
FORMATS = [(8, 0), (16, 0), (24, 0), (32, 0), (32, 1)]


def lib():
    from hmp3_amd import api
    return api.lib()


def converter(source, target, channels, target_channels, bits, is_float):
    L = lib()
    h = L.hx_src_create()
    cut = C.c_int(0)
    need = L.hx_src_init(h, source, channels, bits, is_float, target, target_channels, C.byref(cut))
    assert need > 0
    return h


def schedule(h, calls, nframes):
    nb = np.zeros(nframes, dtype=np.int64)
    rd = lib().hx_src_schedule(h, calls, nframes, nb.ctypes.data)
    return nb, rd


def stage_bytes(source, target, channels, bits):
    """bytes hx_src_convert stages per call (it converts this many before filtering)"""
    return 1152 * (source // target + 1 if source > target else 1) * channels * bits // 8


@pytest.mark.parametrize("source,target", PAIRS, ids=["%d_%d" % p for p in PAIRS])
def test_schedule_equals_the_stepping_converter(source, target):
    """600 consecutive calls: the schedule's consumed bytes are the in_bytes of the converter's own calls"""
    L = lib()
    for channels, tch in LAYOUTS:
        for bits, is_float in FORMATS:
            h = converter(source, target, channels, tch, bits, is_float)
            want, rd = schedule(h, 0, 600)
            buf = (C.c_ubyte * (stage_bytes(source, target, channels, bits) + 64))()
            y = np.zeros(2304, np.float32)
            got = [L.hx_src_convert(h, buf, y.ctypes.data, None) for _ in range(600)]
            assert list(want) == got, (channels, tch, bits, is_float)
            assert rd >= sum(got)
            # the schedule depends on the call count only: from call 37 on it is the tail of the one from call 0
            tail, _ = schedule(h, 37, 100)
            assert list(tail) == got[37:137]
            L.hx_src_destroy(h)


def intermediate_rate(source, target):
    """the two-stage plan's intermediate rate (hx_src.cpp intermediate_rate; the source rate when there is no stage 1)"""
    def taps(s, t):
        return 1 if s <= t else (max(1, min(48, (12 * s + t // 2) // t)) & ~1) | 1
    if source <= target or target // np.gcd(source, target) * taps(source, target) <= 780:
        return source
    g = int(np.gcd(source, target))
    s, t = source // g, target // g
    up = down = 0
    for i in range(7, t):
        if s % i or t % (i + 1):
            continue
        down, up = i, i + 1
        if taps(up * source // down, target) * (t // up) <= 780:
            break
    return up * source // down


@pytest.mark.parametrize("source,target", PAIRS, ids=["%d_%d" % p for p in PAIRS])
def test_schedule_far_into_a_stream(source, target):
    """far into a stream (positions beyond 32 bits, call counts beyond 10^7): the schedule at call c + T equals the one
    at call c for a T after which the phase provably repeats, and the read bound stays the same"""
    h = converter(source, target, 2, 2, 16, 0)
    # after T = 128 n n1 calls every phase repeats (the main stage's n divides the target rate, stage 1's n1 the
    # intermediate rate): the outputs advance by whole bank periods, the intermediate samples by whole refills and
    # whole stage-1 periods
    # (from call 1 on: call 0 starts with no intermediate samples formed, a state the stream does not come back to)
    T = 128 * target * intermediate_rate(source, target)
    for c in (1, 5, 1234):
        a, ra = schedule(h, c, 50)
        for far in (T, (10 ** 7 // T + 1) * T, 3 * T, (2 ** 40 // T + 1) * T):
            b, rb = schedule(h, c + far, 50)
            assert list(a) == list(b) and ra == rb, (c, far)
    lib().hx_src_destroy(h)


@pytest.mark.parametrize("source,target", [(32000, 44100), (11025, 16000), (44100, 32000), (48000, 44100)], ids=lambda p: str(p))
def test_schedule_equals_the_converter_stepped_far(source, target):
    """the closed form at call 20000 (output index x bank step beyond 2^32 for the first two pairs) equals the consumption
    of a converter stepped through 20000 calls"""
    L = lib()
    h = converter(source, target, 2, 2, 16, 0)
    buf = (C.c_ubyte * (stage_bytes(source, target, 2, 16) + 64))()
    y = np.zeros(2304, np.float32)
    for _ in range(20000):
        L.hx_src_convert(h, buf, y.ctypes.data, None)
    want, _ = schedule(h, 20000, 40)
    assert list(want) == [L.hx_src_convert(h, buf, y.ctypes.data, None) for _ in range(40)]
    L.hx_src_destroy(h)


@pytest.mark.parametrize("source,target", PAIRS[::2] + [(44100, 32000), (48000, 44100)], ids=lambda p: str(p))
def test_read_bound_is_a_bound(source, target):
    """bytes past what the schedule says a call reads do not change its samples (filled with garbage here)"""
    L = lib()
    rng = np.random.default_rng(source + target)
    for channels, tch in LAYOUTS:
        for bits, is_float in FORMATS:
            ha = converter(source, target, channels, tch, bits, is_float)
            hb = converter(source, target, channels, tch, bits, is_float)
            fb = channels * bits // 8
            nst = stage_bytes(source, target, channels, bits) + 64
            if is_float:
                data = rng.uniform(-1, 1, 40 * nst // 4).astype("<f4").tobytes()
            else:
                data = rng.integers(0, 256, 40 * nst, dtype=np.uint8).tobytes()
            pos = 0
            for call in range(6):
                nb, rd = schedule(ha, call, 1)
                clean = bytearray(data[pos:pos + nst])
                dirty = bytearray(clean)
                dirty[rd:] = rng.integers(0, 256, nst - rd, dtype=np.uint8).tobytes()
                ya, yb = np.zeros(2304, np.float32), np.zeros(2304, np.float32)
                ia = L.hx_src_convert(ha, (C.c_ubyte * nst).from_buffer(clean), ya.ctypes.data, None)
                ib = L.hx_src_convert(hb, (C.c_ubyte * nst).from_buffer(dirty), yb.ctypes.data, None)
                assert ia == ib == nb[0] and ia % fb == 0
                assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), (channels, tch, bits, is_float, call)
                pos += ia
            L.hx_src_destroy(ha)
            L.hx_src_destroy(hb)


def ref_control(ec, bits, is_float, mpeg_select, mono_convert):
    R = O.ref()
    R.ref_init_mp3.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    R.ref_info_ec.argtypes = [C.c_void_p, C.c_void_p]
    from hmp3_amd import api
    h = R.ref_new()
    e = api.EControl()
    C.memmove(C.byref(e), C.byref(ec), C.sizeof(e))
    n = R.ref_init_mp3(h, C.byref(e), bits, is_float, mpeg_select, mono_convert)
    out = api.EControl()
    if n:
        R.ref_info_ec(h, C.byref(out))
    R.ref_free(h)
    return n, out


def fields(ec):
    return {f: (list(getattr(ec, f)) if f == "mnr_adjust" else getattr(ec, f)) for f, _ in ec._fields_}


@pytest.mark.parametrize("source", [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000])
def test_encode_control_equals_the_reference_init(source):
    """the control the shared derivation gives a converted source, resolved like an encoder resolves it, is what the
    reference's MP3_audio_encode_init leaves behind (L3_audio_encode_info_ec), and so are the bytes per call"""
    from hmp3_amd import api
    L = lib()
    controls = [api.default_control(bitrate=64), api.default_control(), api.default_control(bitrate=48, nsb_limit=20),
                api.default_control(bitrate=96, freq_limit=12000), api.default_control(mode=3, bitrate=64),
                api.default_control(mode=3, nsb_limit=26)]
    checked = 0
    for ec0 in controls:
        for mpeg_select in (0, 1, 2, 32000, 22050):
            for mono_convert in (0, 1):
                for bits, is_float in ((16, 0), (24, 0), (32, 1)):
                    ec = api.EControl()
                    C.memmove(C.byref(ec), C.byref(ec0), C.sizeof(ec))
                    ec.samprate = source
                    src = api.Source(bits, is_float, mpeg_select, mono_convert)
                    mine, n = api.src_encode_control(ec, src)
                    rn, rec = ref_control(ec, bits, is_float, mpeg_select, mono_convert)
                    assert n == rn, (ec0.mode, mpeg_select, mono_convert, bits)
                    if not n:
                        continue
                    resolved = api.EControl()
                    assert L.hx_control_info(C.byref(mine), C.byref(resolved), None) == 1
                    assert fields(resolved) == fields(rec), (ec0.mode, mpeg_select, mono_convert, bits)
                    checked += 1
    assert checked > 0
