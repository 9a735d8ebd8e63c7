"""The oracle (oracle/hxo_*.c) against the committed golden vectors that tests/golden/make_golden.py
captured from the real reference.  CPU only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from hmp3_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "streams.json")))
ALL_CASES = list(META)      # long-only and default (block switching) configurations


def test_known_answers_mblog_mbexp_pow34():
    g = np.load(os.path.join(GOLD, "kat_math.npz"))
    l = O.lib()
    got = np.array([l.hxo_mblog(C.c_float(float(x))) for x in g["mblog_x"]], dtype=np.int32)
    assert np.array_equal(got, g["mblog_y"])
    # the survey's spot values
    for x, y in ((1.0, 1), (2.0, 302), (10.0, 1001), (1000.0, 3000), (0.0, -38226)):
        assert l.hxo_mblog(C.c_float(x)) == y
    got = np.array([l.hxo_mbexp(int(i)) for i in g["mbexp_x"]], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), g["mbexp_y"].view(np.uint32))
    x = np.ascontiguousarray(g["pow34_x"]); y = np.zeros_like(x)
    l.hxo_pow34.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    l.hxo_pow34(x.ctypes.data, y.ctypes.data, len(x))
    assert np.array_equal(y.view(np.uint32), g["pow34_y"].view(np.uint32))


def _params(kw):
    enc = O.OracleEncoder(O.default_control(**kw))
    assert enc.ok()
    return enc


def test_stage_polyphase_hybrid_attack_bit_exact():
    g = np.load(os.path.join(GOLD, "stage_frontend.npz"))
    l = O.lib()
    enc = _params(dict(bitrate=64))
    p = enc.h       # hxo_params is the first member of hxo_encoder
    l.hxo_polyphase_granule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for v, want in zip(g["sbt_in"], g["sbt_out"]):
        v = np.ascontiguousarray(v); out = np.zeros(576, dtype=np.float32)
        l.hxo_polyphase_granule(p, v.ctypes.data, out.ctypes.data)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    l.hxo_freq_invert.argtypes = [C.c_void_p, C.c_int]
    l.hxo_hybrid_long.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.hxo_antialias.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    for x1, x2, want, bt in zip(g["hy_x1"], g["hy_x2"], g["hy_out"], g["hy_bt"]):
        x1 = np.ascontiguousarray(x1); x2 = np.ascontiguousarray(x2).copy(); y = np.zeros(576, dtype=np.float32)
        l.hxo_freq_invert(x2.ctypes.data, 23)
        l.hxo_hybrid_long(p, x1.ctypes.data, x2.ctypes.data, y.ctypes.data, int(bt), 23, 0)
        l.hxo_antialias(p, y.ctypes.data, 23)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    l.hxo_attack_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    eng = np.full(32, 9000, dtype=np.int32)
    prev = 0
    for smp, want, weng in zip(g["at_in"], g["at_out"], g["at_eng"]):
        smp = np.ascontiguousarray(smp)
        m = l.hxo_attack_detect(smp.ctypes.data, eng.ctypes.data, prev)
        assert m == int(want) and np.array_equal(eng, weng)
        prev = 1 if m > 700 else 0


@pytest.mark.parametrize("name", ALL_CASES)
def test_stream_bytes_and_sizes_match_reference(name):
    m = META[name]
    pcm = synth.stream_pcm(m["stream_seed"], m["frames"], sr=m["samprate"], rho=m["rho"], bursts=m["bursts"])
    enc = O.OracleEncoder(O.default_control(**m["control"]))
    assert enc.ok()
    out = []
    for f in range(m["frames"] + 2):
        fr = pcm[f * 1152:(f + 1) * 1152] if f < m["frames"] else np.zeros((1152, 2), dtype=np.int16)
        out.append(enc.encode_s16(fr))
    assert [len(b) for b in out] == m["out_sizes"]          # first call emits nothing, reservoir timing
    want = open(os.path.join(GOLD, name + ".mp3frames"), "rb").read()
    assert b"".join(out) == want


@pytest.mark.parametrize("name", ["cbr128_long", "vbr100_hf2_48k_long", "cbr128_32k_long"])
def test_resolved_parameters_match_reference(name):
    m = META[name]
    enc = O.OracleEncoder(O.default_control(**m["control"]))
    l = O.lib()
    l.hxo_debug_table.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_longlong]
    l.hxo_debug_table.restype = C.c_longlong
    v = np.zeros(16, dtype=np.int32)
    l.hxo_debug_table(enc.h, b"scalars", v.ctypes.data, v.nbytes)
    r = m["resolved"]
    assert v[0] == r["nsb_limit"] and [v[1], v[15]] == r["nsb_limitMS"] and v[2] == r["band_limit"]
    assert v[3] == r["main_framebytes"] and v[4] == r["AveTargetBits"] and v[5] == r["initialMNR"]
    nsf = np.zeros(2, dtype=np.int32)
    l.hxo_debug_table(enc.h, b"nsf", nsf.ctypes.data, nsf.nbytes)
    assert list(nsf) == r["nsf"]


def test_init_rejections_follow_reference():
    # mp3enc.cpp:346-351: CBR below 48 kbps per channel above 24 kHz; Layer != III (mp3enc.cpp:388)
    assert not O.OracleEncoder(O.default_control(bitrate=40)).ok()
    assert not O.OracleEncoder(O.default_control(bitrate=64, layer=2)).ok()
    assert O.OracleEncoder(O.default_control(bitrate=64, mode=3)).ok()      # mono
    assert O.OracleEncoder(O.default_control(bitrate=64, mode=2)).ok()      # dual channel (first-generation allocator)
    assert not O.OracleEncoder(O.default_control(bitrate=40, mode=2)).ok()
    assert O.OracleEncoder(O.default_control(bitrate=32, samprate=22050)).ok()      # MPEG-2 LSF
    assert O.OracleEncoder(O.default_control(bitrate=8, samprate=16000)).ok()       # 16 kbps joint stereo: intensity stereo
    assert O.OracleEncoder(O.default_control(bitrate=64)).bytes_in == 9216


def test_silence_and_full_scale_edge_inputs():
    """all-zero input gives frames of the nominal size; full-scale square wave does not overflow"""
    enc = O.OracleEncoder(O.default_control(bitrate=64, short_block_threshold=99999))
    z = np.zeros((1152, 2), dtype=np.int16)
    sizes = [len(enc.encode_s16(z)) for _ in range(12)]
    assert sizes[0] == 0 and all(s in (0, 417, 418, 835, 836) for s in sizes) and sum(sizes[1:]) > 0
    enc = O.OracleEncoder(O.default_control(bitrate=64, short_block_threshold=99999))
    sq = np.where((np.arange(1152) // 24) % 2 == 0, 32767, -32768).astype(np.int16)
    fr = np.stack([sq, -sq - 1], axis=1).astype(np.int16)
    total = sum(len(enc.encode_s16(fr)) for _ in range(12))
    assert total > 0


def _extra():
    import sys
    sys.path.insert(0, GOLD)
    import make_golden as M
    return M


@pytest.mark.parametrize("name", ["a1_dual_16k_antiphase", "stab_odd_npart_32k"])
def test_extra_golden_streams(name):
    """streams whose signal is more than a seed (make_golden.EXTRA_CASES): the first-generation allocator's dual-channel
    case that separates libm's log10f (what the reference's C++ calls) from the double log10; the 32 kHz VBR stream on which
    spd_smrLongEcho reads stab[npart] unwritten (golden = reference built with -ftrivial-auto-var-init=zero)"""
    M = _extra()
    kw = M.EXTRA_CASES[name][0]
    got = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), M.extra_case_pcm(name))
    assert got == open(os.path.join(GOLD, name + ".mp3frames"), "rb").read()


@pytest.mark.parametrize("name", ["range_tone_x64_cbr320", "range_dc_tail_cbr128_dc"])
def test_range_golden_streams(name):
    """the ends of the float range (make_golden.RANGE_CASES): float input at 64 x full scale, whose noise measurement goes
    through pow() beyond 16384; int16 input whose DC-blocker tail is subnormal for 54 frames"""
    M = _extra()
    kw = M.RANGE_CASES[name][0]
    enc = O.OracleEncoder(O.default_control(**kw))
    assert M.encode_range_case(enc, name) == open(os.path.join(GOLD, name + ".mp3frames"), "rb").read()
    if name == "range_tone_x64_cbr320":
        assert enc.range_counts()["from_16384"] > 0 and enc.range_counts()["max_qx"] > 65536
