"""Live pin of the oracle against the real reference (oracle/_ref, built from /root/reference by
`make -C oracle ref`).  Skipped where the reference build is not present.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from hmp3_amd import synth
import packet_cases as PC
import dynamic_range_cases as DR

pytestmark = pytest.mark.skipif(O.ref() is None, reason="oracle/_ref not built")

CASES = [
    ("cbr128", dict(bitrate=64), 44100, 0.7, 150),
    ("cbr128_lr", dict(bitrate=64, mode=0), 44100, 0.3, 80),
    ("cbr128_rho1", dict(bitrate=64), 44100, 1.0, 80),
    ("cbr96", dict(bitrate=48), 44100, 0.7, 80),
    ("cbr320", dict(bitrate=160), 44100, 0.7, 60),
    ("cbr128_32k", dict(bitrate=64, samprate=32000), 32000, 0.7, 80),
    ("cbr128_48k", dict(bitrate=64, samprate=48000), 48000, 0.7, 80),
    ("vbr50", dict(), 44100, 0.7, 120),
    ("vbr0", dict(vbr_mnr=0), 44100, 0.7, 60),
    ("vbr150", dict(vbr_mnr=150), 44100, 0.7, 60),
    ("vbr100_hf2_48k", dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000), 48000, 0.7, 120),
    ("cbr256_hf", dict(bitrate=128, hf_flag=3), 44100, 0.7, 60),
    ("dc_filter", dict(bitrate=64, filter_select=1), 44100, 0.7, 60),
]


@pytest.mark.parametrize("name,kw,sr,rho,nfr", CASES, ids=[c[0] for c in CASES])
def test_long_block_streams_byte_identical(name, kw, sr, rho, nfr):
    kw = dict(kw, short_block_threshold=99999)
    pcm = synth.stream_pcm(11, nfr, sr=sr, rho=rho)
    a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
    b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
    assert len(a) > 0 and a == b


SHORT_CASES = [
    ("cbr128_bursts", dict(bitrate=64), 44100, 0.7, 160),
    ("cbr128_lr_bursts", dict(bitrate=64, mode=0), 44100, 0.3, 100),
    ("vbr50_bursts", dict(), 44100, 0.7, 160),
    ("vbr100_hf2_48k_bursts", dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000), 48000, 0.7, 120),
    ("cbr128_32k_bursts", dict(bitrate=64, samprate=32000), 32000, 0.0, 100),
    ("vbr50_thr100_mostly_short", dict(short_block_threshold=100), 44100, 0.7, 100),
    ("cbr128_thr0_all_short", dict(bitrate=64, short_block_threshold=0), 44100, 1.0, 60),
]


@pytest.mark.parametrize("name,kw,sr,rho,nfr", SHORT_CASES, ids=[c[0] for c in SHORT_CASES])
def test_block_switching_streams_byte_identical(name, kw, sr, rho, nfr):
    pcm = synth.stream_pcm(13, nfr, sr=sr, rho=rho, bursts=True)
    a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
    b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
    assert len(a) > 0 and a == b


@pytest.mark.parametrize("kw", [dict(bitrate=48), dict(bitrate=160), dict(vbr_mnr=150, hf_flag=3, freq_limit=22000), dict(vbr_mnr=0),
                                dict(bitrate=64, mode=0)], ids=["cbr96", "cbr320", "vbr150hf", "vbr0", "cbr128lr"])
def test_stress_signals_byte_identical(kw):
    """the rare-branch signals of tests/test_gpu_parity.py::test_stress_signals_rare_paths, oracle vs reference"""
    F = 36
    n = F * 1152
    rng = np.random.default_rng(77)
    t = np.arange(n)
    noise = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    tone = np.round(32767 * np.sin(2 * np.pi * 110.0 * t / 44100.0)).astype(np.int16)
    lowtone = np.stack([tone, tone], axis=1)
    nyq = np.stack([np.where(t % 2 == 0, 32767, -32768), np.where(t % 2 == 0, -20000, 20000)], axis=1).astype(np.int16)
    clicks = np.zeros((n, 2), dtype=np.int16); clicks[::4001, 0] = 32767; clicks[1000::5003, 1] = -32768
    anti = np.stack([noise[:, 0] // 2, -(noise[:, 0] // 2)], axis=1).astype(np.int16)
    for pcm in (noise, lowtone, nyq, clicks, anti):
        a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
        b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
        assert len(a) > 0 and a == b


MONO_CASES = [
    ("mono_cbr64", dict(bitrate=64, mode=3), 44100),
    ("mono_vbr50", dict(mode=3), 44100),
    ("mono_cbr96_48k", dict(bitrate=96, mode=3, samprate=48000), 48000),
    ("mono_cbr48_32k_long", dict(bitrate=48, mode=3, samprate=32000, short_block_threshold=99999), 32000),
    ("mono_cbr160", dict(bitrate=160, mode=3), 44100),
    ("mono_vbr100_hf_48k", dict(mode=3, vbr_mnr=100, hf_flag=3, samprate=48000, freq_limit=19000), 48000),
    ("mono_cbr64_dc", dict(bitrate=64, mode=3, filter_select=1), 44100),
]


@pytest.mark.parametrize("name,kw,sr", MONO_CASES, ids=[c[0] for c in MONO_CASES])
def test_mono_streams_byte_identical(name, kw, sr):
    """mode 3 (encode_singleB, 17-byte side info), block switching on unless disabled"""
    nfr = 100
    pcm = synth.stream_pcm(31, nfr, sr=sr, bursts=True)[:, 0].copy()
    r = O.RefEncoder(O.default_control(**kw))
    o = O.OracleEncoder(O.default_control(**kw))
    a = b"".join(r.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    b = b"".join(o.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    assert len(a) > 0 and a == b


def test_float_input_byte_identical():
    """L3_audio_encode takes float at int16 scale; non-integral samples must not be rounded"""
    kw = dict(bitrate=64, short_block_threshold=99999)
    nfr = 60
    pcm = synth.stream_pcm(17, nfr).astype(np.float32)
    pcm += np.random.default_rng(5).uniform(-0.49, 0.49, pcm.shape).astype(np.float32)
    r = O.RefEncoder(O.default_control(**kw), s16=False)
    o = O.OracleEncoder(O.default_control(**kw))
    a = b"".join(r.encode_f32(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    b = b"".join(o.encode_f32(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    assert len(a) > 0 and a == b


@pytest.mark.parametrize("kw", [dict(bitrate=64), dict(vbr_mnr=60)], ids=["cbr128", "vbr60"])
def test_packet_variant_byte_identical(kw):
    """L3_audio_encode_Packet: bitstream and the reformatted (self-contained) frame"""
    nfr = 50
    pcm = synth.stream_pcm(23, nfr, bursts=True).astype(np.float32)
    r = O.RefEncoder(O.default_control(**kw), s16=False)
    o = O.OracleEncoder(O.default_control(**kw))
    for f in range(nfr):
        a = r.encode_packet(pcm[f * 1152:(f + 1) * 1152])
        b = o.encode_packet(pcm[f * 1152:(f + 1) * 1152])
        assert a == b and len(a[1]) >= 36, "frame %d" % f
        assert r.packet_sizes == o.packet_sizes and r.packet_sizes[1] == 0


LSF_CASES = [
    # MPEG-2 LSF rates: one granule per frame, 8-bit main_data_begin, 9-bit scalefac_compress
    ("lsf_cbr64_22k", dict(bitrate=32, samprate=22050), 22050, 0.7),
    ("lsf_cbr64_22k_long", dict(bitrate=32, samprate=22050, short_block_threshold=99999), 22050, 0.7),
    ("lsf_cbr64_24k", dict(bitrate=32, samprate=24000), 24000, 0.7),
    ("lsf_cbr48_16k", dict(bitrate=24, samprate=16000), 16000, 0.7),
    ("lsf_cbr160_24k", dict(bitrate=80, samprate=24000), 24000, 0.3),
    ("lsf_cbr64_lr", dict(bitrate=32, samprate=22050, mode=0), 22050, 0.3),
    ("lsf_vbr50_22k", dict(samprate=22050), 22050, 0.7),
    ("lsf_vbr0_16k", dict(samprate=16000, vbr_mnr=0), 16000, 0.7),
    ("lsf_vbr150_24k", dict(samprate=24000, vbr_mnr=150), 24000, 0.7),
    ("lsf_dc", dict(bitrate=32, samprate=22050, filter_select=1), 22050, 0.7),
    ("lsf_mono_cbr32_22k", dict(bitrate=32, samprate=22050, mode=3), 22050, 0.7),
    ("lsf_mono_vbr_16k", dict(samprate=16000, mode=3), 16000, 0.7),
    ("lsf_mono_cbr8_16k", dict(bitrate=8, samprate=16000, mode=3), 16000, 0.7),
]


@pytest.mark.parametrize("name,kw,sr,rho", LSF_CASES, ids=[c[0] for c in LSF_CASES])
@pytest.mark.parametrize("bursts", [False, True], ids=["steady", "bursts"])
def test_mpeg2_streams_byte_identical(name, kw, sr, rho, bursts):
    pcm = synth.stream_pcm(17, 100, sr=sr, rho=rho, bursts=bursts)
    r = O.RefEncoder(O.default_control(**kw))
    o = O.OracleEncoder(O.default_control(**kw))
    if kw.get("mode") == 3:
        pcm = pcm[:, 0].copy()
        a = b"".join(r.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(100))
        b = b"".join(o.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(100))
    else:
        a = O.encode_stream(r, pcm)
        b = O.encode_stream(o, pcm)
    assert len(a) > 0 and a == b


@pytest.mark.parametrize("kw", [dict(bitrate=32, samprate=22050), dict(samprate=24000, vbr_mnr=80), dict(bitrate=32, samprate=16000, mode=3)],
                         ids=["cbr64_22k", "vbr80_24k", "mono_cbr32_16k"])
def test_mpeg2_packet_variant_byte_identical(kw):
    """L3_audio_encode_MPEG2Packet / _vbr_MPEG2Packet: two packets per call, nbytes_out[0..1]"""
    nfr = 50
    pcm = synth.stream_pcm(23, nfr, sr=kw["samprate"], bursts=True).astype(np.float32)
    if kw.get("mode") == 3:
        pcm = pcm[:, 0].copy()
    r = O.RefEncoder(O.default_control(**kw), s16=False)
    o = O.OracleEncoder(O.default_control(**kw))
    for f in range(nfr):
        a = r.encode_packet(pcm[f * 1152:(f + 1) * 1152])
        b = o.encode_packet(pcm[f * 1152:(f + 1) * 1152])
        assert a == b and r.packet_sizes == o.packet_sizes and min(r.packet_sizes) >= 13, "frame %d" % f


@pytest.mark.parametrize("kw", PC.MPEG1 + PC.MPEG2 + PC.A1, ids=PC.case_id)
def test_packets_and_frame_counters_for_the_batched_outputs_controls(kw):
    """The controls of tests/test_gpu_packets.py (both allocators, MPEG-1 and MPEG-2 rates, mono): the oracle's packets, packet
    sizes and running frame / byte counters - the expectation of the batched calls' optional outputs - against the
    reference's L3_audio_encode_Packet and L3_audio_encode_get_frames, 4 streams x 16 frames of fp32 input with
    non-integral samples."""
    S, F = 4, 16
    pcm = PC.packet_pcm(6100, S, F, kw)
    lsf = kw.get("samprate", 44100) < 32000
    for s in range(S):
        r = O.RefEncoder(O.default_control(**kw), s16=False)
        assert r.bytes_in != 0
        want = PC.oracle_frames(kw, pcm[s])
        emitted = 0
        for f in range(F):
            bs, pk = r.encode_packet(pcm[s, f * 1152:(f + 1) * 1152])
            w = want[f]
            assert (bs, pk) == (w.bs, w.packet) and r.packet_sizes == w.sizes, "stream %d frame %d" % (s, f)
            assert len(pk) == sum(w.sizes) and w.sizes[0] > 0 and (w.sizes[1] > 0) == lsf
            emitted += len(bs)
            assert r.frames() == w.frames_out and w.bytes_out == emitted, "stream %d frame %d" % (s, f)
        assert emitted > 0 and want[-1].frames_out > 0


def test_carried_state_matches_every_frame():
    kw = dict(bitrate=64, short_block_threshold=99999)
    pcm = synth.stream_pcm(3, 40)
    r = O.RefEncoder(O.default_control(**kw))
    o = O.OracleEncoder(O.default_control(**kw))
    d = O.oracle_enable_debug(o)
    for f in range(40):
        fr = pcm[f * 1152:(f + 1) * 1152]
        assert r.encode_s16(fr) == o.encode_s16(fr)
        rd = r.dump()
        assert rd.MNR == d.MNR_after and rd.byte_pool == d.byte_pool
        # last granule's quantised spectrum and scalefactors
        assert np.array_equal(np.array(rd.ix), np.array(d.ix).reshape(2, 2, 576)[1].reshape(-1))
        assert np.array_equal(np.array(rd.sf_l).reshape(2, 2, 23)[:, :, :21], np.array(d.sf).reshape(2, 2, 22)[:, :, :21])


def test_random_configurations_byte_identical():
    """the random controls of tests/test_gpu_parity.py::test_random_configurations_against_the_oracle, oracle vs reference"""
    from parity_cases import random_control
    rng = np.random.default_rng(20240917)
    done = 0
    for trial in range(200):
        kw = random_control(rng)
        o = O.OracleEncoder(O.default_control(**kw))
        if not o.ok():
            continue
        sr, mono = kw["samprate"], kw["mode"] == 3
        pcm = synth.stream_pcm(3000 + 7 * trial, 22, sr=sr, rho=[0.7, 0.0, 1.0, 0.3][trial % 4], bursts=True)
        r = O.RefEncoder(O.default_control(**kw))
        if mono:
            pcm = pcm[:, 0].copy()
        a = b"".join(r.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(22))
        b = b"".join(o.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(22))
        assert a == b, kw
        done += 1
        if done == 60:
            break
    assert done == 60



A1_CASES = [
    # streams the reference codes with its first-generation allocator (CBitAllo1): intensity stereo, dual channel
    # (at the MPEG-1 rates CBR below 48 kbps per channel is rejected, mp3enc.cpp:346-351, and from 96 kbps total
    # on no intensity is used: there it only happens on request, E_CONTROL nsbstereo / -N)
    ("is_n8_cbr128_44k", dict(bitrate=64, nsbstereo=8), 44100, 0.7),
    ("is_n4_cbr96_48k", dict(bitrate=48, nsbstereo=4, samprate=48000), 48000, 0.3),
    ("is_n12_cbr112_32k", dict(bitrate=56, nsbstereo=12, samprate=32000), 32000, 0.0),
    ("is_n3_cbr128_44k_rho1", dict(bitrate=64, nsbstereo=3), 44100, 1.0),
    ("is_n16_cbr192_44k", dict(bitrate=96, nsbstereo=16), 44100, 0.7),
    ("dual_cbr128", dict(bitrate=64, mode=2), 44100, 0.0),
    ("dual_cbr96_48k", dict(bitrate=48, mode=2, samprate=48000), 48000, 0.7),
    ("lsf_is_cbr32_22k", dict(bitrate=16, samprate=22050), 22050, 0.7),
    ("lsf_is_cbr16_16k", dict(bitrate=8, samprate=16000), 16000, 0.3),
    ("lsf_is_cbr40_24k", dict(bitrate=20, samprate=24000), 24000, 0.0),
    ("lsf_dual_cbr64_22k", dict(bitrate=32, samprate=22050, mode=2), 22050, 0.3),
    ("lsf_dual_cbr32_16k", dict(bitrate=16, samprate=16000, mode=2), 16000, 0.7),
]


@pytest.mark.parametrize("name,kw,sr,rho", A1_CASES, ids=[c[0] for c in A1_CASES])
def test_first_generation_allocator_streams_byte_identical(name, kw, sr, rho):
    nfr = 120
    pcm = synth.stream_pcm(41, nfr, sr=sr, rho=rho, bursts=True)
    r, o = O.RefEncoder(O.default_control(**kw)), O.OracleEncoder(O.default_control(**kw))
    assert r.bytes_in != 0 and o.bytes_in != 0
    a = O.encode_stream(r, pcm)
    b = O.encode_stream(o, pcm)
    assert len(a) > 0 and a == b


def test_first_generation_allocator_stress_signals():
    n = 30 * 1152
    rng = np.random.default_rng(99)
    t = np.arange(n)
    noise = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    tone = np.round(32767 * np.sin(2 * np.pi * 110.0 * t / 44100.0)).astype(np.int16)
    silence = np.zeros((n, 2), np.int16)
    quiet = (noise // 4096).astype(np.int16)
    for kw in (dict(bitrate=64, nsbstereo=6), dict(bitrate=64, mode=2), dict(bitrate=16, samprate=22050)):
        for pcm in (noise, np.stack([tone, tone], axis=1), silence, quiet, np.stack([tone, -tone], axis=1)):
            a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
            b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
            assert a == b, kw


@pytest.mark.parametrize("kw,seed,rho,F,bursts", [
    (dict(samprate=48000, mode=2, vbr_mnr=131), 109814, 0.0, 12, False),
    (dict(samprate=48000, mode=2, vbr_mnr=36, hf_flag=3, short_block_threshold=2000, filter_select=1), 370635, 0.7, 12, True)],
    ids=["dual_vbr131", "dual_vbr36_hf"])
def test_negative_scalefactor_frames_byte_identical(kw, seed, rho, F, bursts):
    """quiet dual-channel material on which the first-generation allocator writes negative scalefactors through the
    reference's unmasked bit writer (cases found by tools/fuzz_parity.py)"""
    pcm = synth.stream_pcm(seed, F, sr=kw["samprate"], rho=rho, bursts=bursts)
    pcm = (pcm.astype(np.float64) * 0.02).astype(np.int16)
    a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
    b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
    assert len(a) > 0 and a == b


def test_random_controls_byte_identical():
    """a slice of tools/fuzz_oracle_vs_ref.py: random controls x random signals"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_oracle_vs_ref.py"), "40", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-800:]


A1_LIBM_CASE = dict(kw=dict(samprate=16000, mode=2, bitrate=8), seed=181220, F=40, amp=0.25)


def a1_libm_case_pcm():
    c = A1_LIBM_CASE
    pcm = synth.stream_pcm(c["seed"], c["F"], sr=c["kw"]["samprate"], rho=1.0, bursts=True)
    pcm = (pcm.astype(np.float64) * c["amp"]).astype(np.int16)
    pcm[:, 1] = -pcm[:, 0]
    return pcm


def test_first_generation_allocator_uses_the_float_libm_functions():
    """bitallo1.cpp is C++: log10(float) there is log10f.  With the double functions the oracle's masks differ from the
    reference's in the last place now and then, and this stream (found by tools/fuzz_oracle_vs_ref.py, 1 case in 3000)
    then codes one more line in its second frame."""
    pcm = a1_libm_case_pcm()
    kw = A1_LIBM_CASE["kw"]
    a = O.encode_stream(O.RefEncoder(O.default_control(**kw)), pcm)
    b = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
    assert a == b


def test_first_generation_allocator_random_controls_byte_identical():
    """a slice of tools/fuzz_oracle_vs_ref.py --a1: dual channel and low-rate joint stereo only"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_oracle_vs_ref.py"), "--a1", "150", "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]


@pytest.mark.skipif(O.ref_zero() is None, reason="oracle/_ref/libhmp3ref_zero.so not built (make -C oracle ref_zero)")
def test_uninitialised_psy_local_is_defined_as_zero():
    """spdsmr.c spd_smrLongEcho reads stab[i + 1] with i + 1 == npart, a slot nothing wrote, when npart is odd (32 kHz
    long blocks).  Its value is stack residue: usually harmless, after short-block frames it can move a mask.  The oracle
    (and the GPU) read 0 there; the reference compiled with clang -ftrivial-auto-var-init=zero is the same encoder with
    that read defined, and the oracle must equal it on the stream where the gcc build's residue changes the output."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as M
    name = "stab_odd_npart_32k"
    kw = M.EXTRA_CASES[name][0]
    pcm = M.extra_case_pcm(name)
    z = O.encode_stream(O.RefEncoder(O.default_control(**kw), zero_locals=True), pcm)
    o = O.encode_stream(O.OracleEncoder(O.default_control(**kw)), pcm)
    assert z == o
    # ... and on ordinary material the zeroed-locals build is the reference, byte for byte
    kw2 = dict(samprate=44100, vbr_mnr=50)
    pcm2 = synth.stream_pcm(7, 24, sr=44100, rho=0.7, bursts=True)
    assert O.encode_stream(O.RefEncoder(O.default_control(**kw2), zero_locals=True), pcm2) == \
        O.encode_stream(O.RefEncoder(O.default_control(**kw2)), pcm2)


# ---- the ends of the float range: exactly the inputs of tests/test_gpu_dynamic_range.py (tests/dynamic_range_cases.py) ----
def _both(kw, pcm, nfr, f32):
    """-> (reference bytes, oracle bytes, the oracle encoder) of one stream, frame by frame"""
    r = O.RefEncoder(O.default_control(**kw), s16=not f32)
    o = O.OracleEncoder(O.default_control(**kw))
    a = b"".join((r.encode_f32 if f32 else r.encode_s16)(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    b = b"".join((o.encode_f32 if f32 else o.encode_s16)(pcm[f * 1152:(f + 1) * 1152]) for f in range(nfr))
    return a, b, o


@pytest.mark.parametrize("name", list(DR.OVER_RANGE))
def test_over_range_float_input_byte_identical(name):
    """float input up to 2^16 x full scale (a tone and its gated form at six gains): the oracle is the reference there too, and
    the streams that are there for the pow() path of the noise measurement reach it (the oracle's counters)"""
    kw = DR.OVER_RANGE[name]
    pcm = DR.over_range_batch(kw)
    for s in range(len(pcm)):
        a, b, o = _both(kw, pcm[s], DR.OVER_RANGE_F, True)
        assert len(a) > 0 and a == b, s
        lo, sh = o.range_counts(), o.range_counts(short_blocks=True)
        if s in DR.OVER_RANGE_REACHES_POW.get(name, {}):
            assert lo["from_16384"] > 0, (s, lo)
        assert (lo["from_16384"] > 0) == (lo["max_qx"] >= 16384) and lo["from_16384"] <= lo["beyond_table"]
        # no input of this set takes the short-block noise measurement past the double table: its largest quantised value is
        # 7915 (cbr128_thr0_all_short, gain 65536); the first-generation allocator has no such measurement at all
        assert sh["from_16384"] == 0 and sh["max_qx"] < 16384, (s, sh)
        if name == "a1_is_n8":
            assert lo["beyond_table"] == 0 and sh["beyond_table"] == 0
    if name == "cbr128_thr0_all_short":
        assert sh["beyond_table"] > 0 and sh["max_qx"] >= 256      # (the last stream: the gated tone at gain 65536)


@pytest.mark.parametrize("name", list(DR.SUBNORMAL))
def test_subnormal_float_input_byte_identical(name):
    """float input with its peak at 1e-18 .. 1e-44 and the two 60-decade ramps: bytes (which are the silence pattern for the
    peaks, whatever an encoder does with subnormals: the GPU test compares taps)"""
    kw = DR.SUBNORMAL[name][0]
    for pcm, nfr in ((DR.subnormal_peaks(kw), DR.PEAKS_F), (DR.subnormal_ramps(kw), DR.RAMPS_F)):
        for s in range(len(pcm)):
            a, b, _ = _both(kw, pcm[s], nfr, True)
            assert a == b, (nfr, s)
    assert len(a) > 0


@pytest.mark.parametrize("name", list(DR.DC_TAIL))
def test_dc_blocker_tail_byte_identical(name):
    """int16 material on a DC offset, then digital silence, DC blocker on: the blocker's state goes subnormal and stays"""
    kw, nfr, _ = DR.DC_TAIL[name]
    pcm = DR.dc_tail_batch(kw, nfr)
    for s in range(len(pcm)):
        a, b, _ = _both(kw, pcm[s], nfr, False)
        assert len(a) > 0 and a == b, s


def test_range_goldens_regenerate_from_the_reference():
    """tests/golden/range_*.mp3frames are what the reference built here writes for make_golden.RANGE_CASES, and what the
    oracle writes"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as M
    for name, (kw, nfr, fmt) in M.RANGE_CASES.items():
        want = open(os.path.join(M.GOLD, name + ".mp3frames"), "rb").read()
        assert M.encode_range_case(O.RefEncoder(O.default_control(**kw), s16=(fmt == "s16")), name) == want, name
        assert M.encode_range_case(O.OracleEncoder(O.default_control(**kw)), name) == want, name
