"""The per-frame encoder (hx_enc_*, the CMp3Enc drop-in) on its replayed route: inputs, expectations and drivers of
tests/test_gpu_enc.py; tests/test_enc_cases.py asserts on the CPU what the inputs cover.

The inputs are the allocator census's (tests/alloc_path_cases.py: 37 cases of 10 calls over all eight kinds, the PCM regenerated
by case_pcm, none committed).  From the third call on a call of hx_enc_L3_audio_encode is the replay of a HIP graph recorded
once, so calls 2 .. 9 of every case are replays.  What a case expects of every call is the oracle's: the bytes, frames_out()
after the call and the running byte total; the getters follow from those (bitrate2_float below restates the reference's
running average, pinned to the reference's own getter on the CPU).  An encoder under test is an Enc: every call it makes is
compared as it is made, so several of them can be driven in any interleaving (the schedules below) or from threads of their
own."""
import functools

import numpy as np

import alloc_path_cases as K
from oracle import oracle as O

CALLS = K.FRAMES
PLAIN_FIRST = 2         # calls an encoder makes the plain way before it records its graph (hx_enc.cpp, encode_one)

# one case per kernel: k_alloc / k_alloc_slim, k_alloc_lsf, k_alloc1, k_alloc1_lsf
PER_KERNEL = ["m1_long_02", "m2_long_01", "a1_m1_00", "a1_m2_01"]
# one per kernel family, for encoders that live side by side: stereo, mono, -HF, MPEG-2 with short blocks, first generation
LIVE_GROUP = ["m1_long_02", "m1_mono_00", "m1_hf_01", "m2_short_03", "a1_m1_00", "a1_m2_01"]
THREADED = ["m1_long_02", "m1_mono_00", "m2_long_01", "m2_short_03"]
# (the cases the oracle gives a replayed call of no byte, of two frames and of three: tests/test_enc_cases.py holds them to it)
ZERO_BYTE = ["m1_long_02", "m1_long_04", "m1_long_07", "m1_mono_00", "m1_mono_02", "m1_mono_03", "m2_long_01", "m2_long_06", "m2_short_03"]
TWO_FRAMES = ["m1_long_02", "m1_long_07", "m1_mono_00"]
THREE_FRAMES = ["m2_long_01", "m2_long_03", "m2_long_05", "m2_short_01", "m2_short_03", "a1_m2_01"]


def names(*kinds):
    return [n for n in K.CASES if K.CASES[n][0] in kinds]


def kind(name):
    return K.CASES[name][0]


def control_kw(name):
    return K.CASES[name][2]


def samprate(name):
    return control_kw(name).get("samprate", 44100)


def is_mpeg1(name):
    return samprate(name) >= 32000


def channels(name):
    return 1 if control_kw(name).get("mode") == 3 else 2


def first_generation(name):
    """a stream of k_alloc1 / k_alloc1_lsf: its oracle follows this host's libm (conftest.skip_unless_host_libm_is_the_restated_one)"""
    return kind(name).startswith("a1_")


@functools.lru_cache(maxsize=None)
def pcm(name):
    _, seed, _, sig = K.CASES[name]
    x = K.case_pcm(seed, sig, CALLS)
    x.setflags(write=False)
    return x


def block(name, f):
    return pcm(name)[f * 1152:(f + 1) * 1152]


class Expected:
    """what the oracle gives for a case: per call the bytes, frames_out() after it and the running byte total"""

    def __init__(self, name):
        enc = O.OracleEncoder(O.default_control(**control_kw(name)))
        assert enc.ok(), name
        self.name, self.in_bytes = name, 4608 * channels(name)
        self.bytes, self.frames, self.total = [], [], []
        for f in range(CALLS):
            self.bytes.append(enc.encode_f32(block(name, f)))
            self.frames.append(enc.frames_out())
            self.total.append(enc.bytes_out())
        assert self.total == list(np.cumsum([len(b) for b in self.bytes]))
        self.sizes = [len(b) for b in self.bytes]

    def frames_advance(self, f):
        return self.frames[f] - (self.frames[f - 1] if f else 0)

    def bitrate_float(self, ncalls=CALLS):
        return bitrate_float(is_mpeg1(self.name), samprate(self.name), self.total[ncalls - 1], self.frames[ncalls - 1])

    def bitrate2_float(self, ncalls=CALLS):
        return bitrate2_float(is_mpeg1(self.name), samprate(self.name), self.sizes[:ncalls], self.frames[ncalls - 1])


@functools.lru_cache(maxsize=None)
def expected(name):
    """computed once per process and shared: nothing writes to it"""
    return Expected(name)


# ---- the getters, restated from the per-call byte counts ----

def running_average(mpeg1, sizes):
    """ave_tot_bytes_out after calls of these byte counts: ave += ((bytes << 8) - ave) >> shift in C ints, the shift as the
    reference has it - 7 in its MPEG-1 drivers, 6 in its MPEG-2 drivers (mp3enc.cpp:2209 / :2316, :2476 / :2590)"""
    shift = 7 if mpeg1 else 6
    ave = 0
    for n in sizes:
        ave = ave + (((int(n) << 8) - ave) >> shift)        # (Python's >> floors as the reference's arithmetic shift does)
    return ave


def bitrate2_float(mpeg1, rate, sizes, frames):
    """CMp3Enc::L3_audio_encode_get_bitrate2_float (mp3enc.cpp:3467): the constant's numerator in single precision, the
    products in double, the result rounded to single once"""
    if frames <= 0:
        return np.float32(0.0)
    c = float(np.float32(0.001) * np.float32(8.0)) / (1152.0 * 256.0)
    return np.float32(c * running_average(mpeg1, sizes) * rate)


def bitrate_float(mpeg1, rate, total, frames):
    """CMp3Enc::L3_audio_encode_get_bitrate_float (mp3enc.cpp:3451): single precision throughout, left to right"""
    if frames <= 0:
        return np.float32(0.0)
    f = np.float32
    return f(f(f(f(0.001) * f(8.0)) * f(total)) * f(rate)) / f(f(1152.0 if mpeg1 else 576.0) * f(frames))


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- interleaving schedules: the order in which n live encoders make their calls ----

def round_robin(n, calls=CALLS):
    return [k for _ in range(calls) for k in range(n)]


def uneven(n, calls=CALLS):
    """encoder k advances on the steps where step % (k + 2) == 0, until every encoder has made its calls"""
    left, order, step = [calls] * n, [], 0
    while any(left):
        for k in range(n):
            if left[k] and step % (k + 2) == 0:
                order.append(k)
                left[k] -= 1
        step += 1
    return order


SCHEDULES = {"round_robin": round_robin, "uneven": uneven}


def most_replaying_together(order, n, calls=CALLS):
    """the largest number of encoders that are between their 3rd and their last call - graph recorded, calls to go - at one
    point of the schedule"""
    done, most = [0] * n, 0
    for k in order:
        done[k] += 1
        most = max(most, sum(1 for d in done if PLAIN_FIRST < d < calls))
    return most


# ---- an encoder under test ----

class Enc:
    """an hx_enc on a case: call() makes the case's next call through hx_enc_L3_audio_encode and compares in_bytes, the
    bitstream, hx_enc_get_frames and hx_enc_get_frames_bytes with the oracle's, by =="""

    def __init__(self, api, name, e=None):
        self.api, self.e = api, e if e is not None else api.Mp3Enc()
        self.init(name)

    def init(self, name):
        """(again: re-initialise the same hx_enc to another case)"""
        self.name, self.want, self.f = name, expected(name), 0
        got = self.e.L3_audio_encode_init(self.api.default_control(**control_kw(name)))
        assert got == self.want.in_bytes, "%s: init returned %d: %s" % (name, got, self.api.last_error())
        assert self.e.debug_calls() == (0, 0, 0), name
        assert self.e.L3_audio_encode_get_frames_bytes() == (0, 0), name

    def call(self):
        f, w = self.f, self.want
        where = "%s call %d" % (self.name, f)
        nin, bs = self.e.L3_audio_encode(block(self.name, f))
        assert nin == w.in_bytes, "%s: in_bytes %d: %s" % (where, nin, self.api.last_error())
        assert bs == w.bytes[f], "%s: %d bytes, the oracle has %d (%s)" % (where, len(bs), len(w.bytes[f]), self.api.last_error())
        assert self.e.L3_audio_encode_get_frames() == w.frames[f], where
        assert self.e.L3_audio_encode_get_frames_bytes() == (w.frames[f], w.total[f]), where
        self.f += 1

    def done(self):
        return self.f >= CALLS

    def check_getters(self):
        """after the calls made so far: the three bitrate getters"""
        e, w, n = self.e, self.want, self.f
        br = e.L3_audio_encode_get_bitrate_float()
        assert f32_bits(br) == f32_bits(w.bitrate_float(n)), (self.name, br, w.bitrate_float(n))
        assert e.L3_audio_encode_get_bitrate() == int(np.float32(br) + np.float32(0.5)), self.name
        br2 = e.L3_audio_encode_get_bitrate2_float()
        assert f32_bits(br2) == f32_bits(w.bitrate2_float(n)), (self.name, br2, w.bitrate2_float(n))

    def run(self, ncalls=CALLS):
        while self.f < ncalls:
            self.call()
        return self

    def close(self):
        self.e.close()


def run_case(api, name, route=(PLAIN_FIRST, CALLS - PLAIN_FIRST, 1)):
    """a case's ten calls on a new encoder, every call compared, then the getters and the route the calls took"""
    x = Enc(api, name).run()
    x.check_getters()
    got = x.e.debug_calls()
    x.close()
    assert got == route, "%s: debug_calls() %s, expected %s: %s" % (name, got, route, api.last_error())


# ---- the reference's own getter (oracle/_ref/libhmp3ref.so, where it is built) ----

def ref_has_getters():
    return O.ref_has_getters()


def ref_getters(name):
    """the case through the reference itself -> per call (out_bytes, frames, get_bitrate2_float, get_bitrate_float, get_bitrate)"""
    enc = O.RefEncoder(O.default_control(**control_kw(name)), s16=False)
    assert enc.bytes_in > 0, name
    return [(len(enc.encode_f32(block(name, f))), enc.frames()) + enc.bitrates() for f in range(CALLS)]


NULL_BS_CALL, NULL_PACKET_CALL = 4, 5       # the calls of the packet test that pass bs_out = NULL / packet = NULL


def ref_packet_null_forms(name):
    """the case through the reference's L3_audio_encode_Packet, call 4 with bs_out = NULL and call 5 with packet = NULL
    -> per call (out_bytes, bitstream bytes or None, frames, packet bytes or None, nbytes_out as the call left it)"""
    import ctypes as C
    enc = O.RefEncoder(O.default_control(**control_kw(name)), s16=False)
    assert enc.bytes_in > 0, name
    res = []
    for f in range(CALLS):
        x = np.ascontiguousarray(block(name, f), dtype=np.float32)
        out, pk, nb = (C.c_ubyte * 16384)(), (C.c_ubyte * 4096)(), (C.c_int * 2)(-1, -1)
        n = enc.r.ref_encode_packet(enc.h, x.ctypes.data, None if f == NULL_BS_CALL else out, None if f == NULL_PACKET_CALL else pk, nb)
        res.append((n, None if f == NULL_BS_CALL else bytes(out[:n]), enc.frames(), None if f == NULL_PACKET_CALL else bytes(pk[:nb[0] + nb[1]]),
                    (nb[0], nb[1])) + enc.bitrates())
    return res


def packet_null_expected(name):
    """what that sequence of calls must give, from the oracle: per call (out_bytes, bitstream, frames_out, running byte total,
    packet, nbytes_out, bitrate2_float, bitrate_float).  The call without a bitstream buffer sends its frames - the counter
    advances, later calls' bytes are unchanged - and returns and counts no byte (mp3enc.cpp:2964-2994)"""
    o = O.OracleEncoder(O.default_control(**control_kw(name)))
    res, sizes, total = [], [], 0
    for f in range(CALLS):
        bs, pk = o.encode_packet(block(name, f))
        n = 0 if f == NULL_BS_CALL else len(bs)
        sizes.append(n)
        total += n
        res.append((n, bs, o.frames_out(), total, pk, tuple(o.packet_sizes),
                    bitrate2_float(is_mpeg1(name), samprate(name), sizes, o.frames_out()),
                    bitrate_float(is_mpeg1(name), samprate(name), total, o.frames_out())))
    return res
