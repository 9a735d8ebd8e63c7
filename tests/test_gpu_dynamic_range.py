"""Parity across the float range on a real MI355X: float samples from float32's subnormal range up to 2^16 x full scale
(finite values only; NaN and infinite samples are not defined by the reference).

The rest of the suite feeds int16-scale material.  Two regimes lie outside it.  Above full scale the noise measurement of
the stream walk quantises lines past the host-built double table of ix^(4/3) (HX_POW43_N = 16384 entries) and calls the
device's pow(), where the reference calls libm's; the oracle's counters (OracleEncoder.range_counts) say which streams get
there.  At the other end the DC blocker's state after digital silence, and quiet float input, are subnormal for seconds:
the bytes are the silence pattern whatever a kernel does with such values, so the subband and spectrum taps are compared
by bit pattern (tests/stage_taps.py), which tells a subnormal from the zero a flush would leave, and -0.0 from +0.0.

The inputs are in tests/dynamic_range_cases.py; tests/test_oracle_vs_ref.py pins the oracle to the reference on exactly
these.  MPEG-1 second-generation cases run on both stream-walk builds, MPEG-2 and first-generation ones once."""
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from conftest import skip_unless_host_libm_is_the_restated_one
import dynamic_range_cases as DR
from stage_taps import TapBatch
from hmp3_amd import api

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_over_range(name):
    """one configuration of DR.OVER_RANGE as a batch of 12 float streams: bytes, status and the oracle's counters"""
    kw = DR.OVER_RANGE[name]
    pcm = DR.over_range_batch(kw)
    S, F = len(pcm), DR.OVER_RANGE_F
    assert S == 12 and float(np.abs(pcm).max()) > 65536.0 * 32000 and np.isfinite(pcm).all()
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=F)
    got = b.encode_host(pcm)
    assert b.status() == 0
    short_beyond = 0
    for s in range(S):
        enc = O.OracleEncoder(O.default_control(**kw))
        want = b"".join(enc.encode_f32(pcm[s, f * 1152:(f + 1) * 1152]) for f in range(F))
        lo, sh = enc.range_counts(), enc.range_counts(short_blocks=True)
        print("%s stream %d: long %s short %s" % (name, s, lo, sh))
        assert len(want) > 0 and got[s] == want, "stream %d" % s
        if s in DR.OVER_RANGE_REACHES_POW.get(name, {}):
            assert lo["from_16384"] > 0 and lo["max_qx"] >= 16384, (s, lo)
        assert sh["from_16384"] == 0, (s, sh)
        short_beyond += sh["beyond_table"]
    if name != "a1_is_n8":
        assert short_beyond > 0      # the short-block measurement's double-table path is in
    b.close()


@pytest.mark.parametrize("name", ["cbr320", "mono_cbr160", "vbr150_hf", "cbr128_dc", "cbr128_lr", "cbr128_thr0_all_short"])
def test_over_range_float_input_byte_identical_to_oracle(name):
    """Streams 0-5: the 110 Hz tone as [x, 0.5 x] (mono: x) at gains 1, 2, 16, 64, 1024, 65536; 6-11: the tone gated 3000
    samples on, 3000 at -60 dB; 12 frames.  Every stream's bytes equal the oracle's, and the streams that are there for it
    have long-block noise terms from pow() at 16384 or more (DR.OVER_RANGE_REACHES_POW: 9, 65, 85, 94 events on the tone
    of cbr320 at gains 16 .. 65536, 2 and 17 on its gated form at 16 and 64; mono 11 and 47 at 64 and 1024; vbr150_hf 35 at
    1024; cbr128_dc 5 at 16; the largest quantised value is 70215, cbr320 at gain 64).
    Short blocks: none of these inputs takes the short-block noise measurement to 16384.  Its largest quantised value is
    7915 (cbr128_thr0_all_short, gain 65536), 6357 on the gated streams of vbr150_hf, 4902 on those of cbr320: that
    measurement runs here between 256 and 16384, on the double table, and its pow() call stays unreached."""
    check_over_range(name)


@pytest.mark.one_k6_build
def test_over_range_float_input_mpeg2():
    """samprate=22050, bitrate=32: quantised values stay below 16384 (largest 5519), but this kernel has not seen over-range
    samples either"""
    check_over_range("lsf_cbr64_22k")


@pytest.mark.one_k6_build
def test_over_range_float_input_first_generation_allocator():
    """bitrate=64, nsbstereo=8 (intensity stereo): the first-generation allocator has no noise measurement of this kind"""
    skip_unless_host_libm_is_the_restated_one()
    check_over_range("a1_is_n8")


def test_over_range_stream_through_the_per_frame_entry():
    """bitrate=160, the tone at gain 64, through Mp3Enc.L3_audio_encode: 12 calls, ten of them replayed from the recorded
    graph; every call's bytes"""
    kw = DR.OVER_RANGE["cbr320"]
    pcm = DR.over_range_stream(kw, 64)
    e = api.Mp3Enc()
    assert e.L3_audio_encode_init(api.default_control(**kw)) == 9216
    o = O.OracleEncoder(O.default_control(**kw))
    total = 0
    for f in range(DR.OVER_RANGE_F):
        blk = pcm[f * 1152:(f + 1) * 1152]
        nin, bs = e.L3_audio_encode(blk)
        assert nin == 9216 and bs == o.encode_f32(blk), "call %d" % f
        total += len(bs)
    assert total > 0 and o.range_counts()["from_16384"] > 0
    e.close()


@pytest.mark.one_k6_build
def test_device_pow_gives_the_reference_noise_term_at_every_gain_step():
    """Beyond the double table the stream walk takes ix^(4/3) from the device's pow(), the reference from libm's, and the
    two are different functions: on an MI355X the device's result differs from glibc's in its last bit for 26 % of the
    integers 256 .. 2^21 (13 854 of the 53 832 values 16384 .. 70215).  What the noise sum reads is the float
    (float) (gain * pw), gain one of the 128 steps of look_gain; a last-bit difference of pw changes it only where gain * pw
    lies within 2^-29 (relative) of a float rounding boundary.  The byte comparisons above cover a few hundred such terms;
    this test covers the domain: for every ix from 16384 (HX_POW43_N) to 2^21 - 1, thirty times the largest quantised value
    any input of this file reaches (70215), and every gain step, the float is the same for both values of pw.  The device's
    values come from the debug read "pow43_beyond" (the kernels' expression, hx_batch.hip), the reference's from the oracle
    (oracle.pow43: the C library of the machine the test runs on)."""
    import math
    first, n = 16384, (1 << 21) - 16384
    b = api.Batch(api.default_control(bitrate=64), nstreams=1, max_frames=1)
    dev = b.debug_read("pow43_beyond", np.float64, n)
    b.close()
    host = O.pow43(first, n)
    assert len(dev) == n and host[0] == math.pow(16384.0, 4.0 / 3.0) and abs(dev[0] / host[0] - 1.0) < 1e-12
    differ = np.flatnonzero(dev.view(np.uint64) != host.view(np.uint64))
    ulps = np.abs(dev.view(np.int64)[differ] - host.view(np.int64)[differ])
    print("device pow(ix, 4/3) differs from the host's for %d of %d ix (largest difference %d ulp), first at ix = %s"
          % (len(differ), n, int(ulps.max()) if len(differ) else 0, first + int(differ[0]) if len(differ) else None))
    bad = 0
    for g in range(128):
        gain = float(np.float32(math.pow(2.0, 0.25 * (g - 8))))        # look_gain[g] (bitallo3.cpp:366), promoted as the product is
        bad += int(np.count_nonzero((gain * dev[differ]).astype(np.float32) != (gain * host[differ]).astype(np.float32)))
    assert bad == 0, "%d (ix, gain step) pairs give another noise term" % bad


def run_subnormal(name, which):
    kw, taps = DR.SUBNORMAL[name]
    pcm, F = (DR.subnormal_peaks(kw), DR.PEAKS_F) if which == "peaks" else (DR.subnormal_ramps(kw), DR.RAMPS_F)
    tb = TapBatch(api, kw, len(pcm), F, taps)
    tb.call(pcm)
    sb, xr = [sum(v) for v in tb.sub_sb], [sum(v) for v in tb.sub_xr]
    print("%s %s: subnormal values in the oracle's sample_new %s, xr_pre %s" % (name, which, sb, xr))
    tb.close()
    return pcm, sb, xr, tb


@pytest.mark.parametrize("name", ["vbr50_sw", "cbr128_dc", "mono_vbr50"])
def test_subnormal_float_input_taps_bit_exact(name):
    """float input whose full scale sits at 1e-18, 1e-30, 1e-36, 1e-40 and 1e-44 (float32 is subnormal below 1.18e-38), 8
    frames: subband samples, spectrum, block types, psy tables, side info and bytes against the oracle, bit patterns.
    What makes it mean something: the oracle's own sample_new tap holds at least 10 000 subnormal values on each of the
    1e-36 and 1e-40 streams (measured 12 974 and 18 160 of 18 432 for {}; 12 969 and 18 191 with the DC blocker), and the
    spectrum tap thousands (10 797 and 11 335; mono 5 451 and 5 696), so a kernel that flushed would differ.  At 1e-44 the
    input is non-zero and everything behind the window underflows to zero: there the zeros' signs are what is compared.
    (Mono has the spectrum tap only.)"""
    pcm, sb, xr, tb = run_subnormal(name, "peaks")
    assert np.count_nonzero(pcm[4]) > 5000 and sb[4] == 0 and xr[4] == 0
    assert sb[0] == 0 and xr[0] == 0            # 1e-18: nothing subnormal, the same code far below int16 scale
    for s in (2, 3):
        if DR.SUBNORMAL[name][1] == "full":
            assert sb[s] >= 10000, (s, sb)
        assert xr[s] >= 5000, (s, xr)


@pytest.mark.parametrize("name", ["vbr50_sw", "cbr128_dc", "mono_vbr50"])
def test_float_input_ramps_through_the_subnormal_range_taps_bit_exact(name):
    """the base signal at full scale falling 60 decades over 20 frames (through the subnormal range to zero), and the reverse
    times 8, which climbs out of the subnormal range and ends over-range (peak 113 965): the same comparison.  The falling
    ramp goes through every block type."""
    pcm, sb, xr, tb = run_subnormal(name, "ramps")
    assert float(np.abs(pcm[1]).max()) > 65536.0 and {0, 1, 2, 3} <= tb.seen_bt
    assert all(len(g) > 0 for g in tb.got)
    assert xr[1] >= 2000, xr        # (measured 4 638; mono 2 290; the falling ramp under the DC blocker has none)


@pytest.mark.one_k6_build
@pytest.mark.parametrize("which", ["peaks", "ramps"])
def test_subnormal_float_input_mpeg2_spectrum_bit_exact(which):
    """samprate=22050, bitrate=32 (the spectrum tap only): measured 13 777 and 14 367 subnormal spectrum values on the 1e-36
    and 1e-40 streams, 5 635 and 4 921 on the ramps"""
    pcm, sb, xr, tb = run_subnormal("lsf_cbr64_22k", which)
    for s in ((2, 3) if which == "peaks" else (0, 1)):
        assert xr[s] >= (10000 if which == "peaks" else 2000), (s, xr)


def check_dc_tail(name):
    kw, F, need = DR.DC_TAIL[name]
    pcm = DR.dc_tail_batch(kw, F)
    calls = [1, 7, 40, 30, F - 78] if F > 78 else [1, 7, 40, F - 48]
    starts = list(np.cumsum(calls)[:-1])
    tb = TapBatch(api, kw, len(pcm), max(calls), "full" if kw.get("samprate", 44100) >= 32000 else "lines")
    pos = 0
    for n in calls:
        tb.call(pcm[:, pos * 1152:(pos + n) * 1152])
        pos += n
    assert pos == F and tb.frames == [F] * len(pcm)
    for s in range(len(pcm)):
        tot = [a + c for a, c in zip(tb.sub_sb[s], tb.sub_xr[s])]
        first = next((f for f in range(F) if tot[f]), None)
        print("%s stream %d: first frame with subnormal taps %s, last %s, values %d" % (name, s, first, max(f for f in range(F) if tot[f]), sum(tot)))
        assert first is not None and first <= DR.DC_TAIL_FIRST_FRAME and sum(tot) >= need, (s, first, sum(tot))
        assert tot[F - 1] > 0       # the recurrence stalls on a subnormal state: it never reaches zero
        assert starts[-1] > first       # a call starts in the tail: the blocker's state is carried between calls while subnormal
    tb.close()
    return tb


@pytest.mark.parametrize("name", ["cbr128_dc", "vbr50_dc"])
def test_dc_blocker_tail_after_silence_taps_bit_exact(name):
    """int16 material on a DC offset for 4 frames, then zeros, with filter_select=1, 120 frames, three seeds, in calls of
    1, 7, 40, 30 and 42 frames (the last one starts inside the tail).  The blocker's state decays geometrically, is subnormal from frame 66 (67 for one seed) and
    stalls there: 145 763 .. 145 818 subnormal values in the oracle's sample_new and xr_pre taps per stream.  Every tap and
    every call's bytes against the oracle."""
    check_dc_tail(name)


@pytest.mark.one_k6_build
def test_dc_blocker_tail_after_silence_mpeg2():
    """the same at 16 kHz (bitrate=16: alpha is larger, the tail is subnormal from frame 27 or 28), 60 frames in calls of 1, 7,
    40 and 12: 17 600 .. 17 680 subnormal spectrum values per stream; the state crosses the last call's start subnormal"""
    check_dc_tail("lsf_cbr32_16k_dc")


@pytest.mark.parametrize("name", ["range_tone_x64_cbr320", "range_dc_tail_cbr128_dc"])
def test_range_golden_reference_streams(name):
    """committed reference bitstreams of make_golden.RANGE_CASES.  The oracle calls the pow() of the machine it runs on;
    these pin the kernels to the reference as built where the goldens were made."""
    sys.path.insert(0, GOLD)
    import make_golden as M
    kw, nfr, fmt = M.RANGE_CASES[name]
    pcm = M.range_case_pcm(name)
    pcm = np.concatenate([pcm, np.zeros((2 * 1152, 2), dtype=pcm.dtype)])
    b = api.Batch(api.default_control(**kw), nstreams=3, max_frames=nfr + 2)
    got = b.encode_host(np.stack([pcm, pcm, pcm]))
    assert b.status() == 0
    want = open(os.path.join(GOLD, name + ".mp3frames"), "rb").read()
    assert got[0] == want and got[1] == want and got[2] == want
    b.close()
