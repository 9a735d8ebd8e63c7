"""CPU side of the per-frame encoder's tests (tests/enc_cases.py; tests/test_gpu_enc.py drives the same inputs through hx_enc_*
on the GPU): what the inputs cover, as conditions on the oracle's output, so a census change that takes a condition away fails
here and the case is searched again, not relaxed.  Calls with index >= 2 are the ones the encoder replays from its graph."""
import numpy as np
import pytest

import alloc_path_cases as K
import enc_cases as E
from oracle import oracle as O

REPLAYED = range(E.PLAIN_FIRST, E.CALLS)


def zero_byte_calls(name):
    return [f for f in REPLAYED if E.expected(name).sizes[f] == 0]


def calls_advancing(name, n):
    return [f for f in REPLAYED if E.expected(name).frames_advance(f) >= n]


def test_every_kind_has_a_case_and_every_case_ten_calls():
    assert len(K.CASES) == 37 and E.CALLS == 10
    for kind in K.KINDS:
        assert E.names(kind), kind
    assert sorted(E.names(*K.KINDS)) == sorted(K.CASES)
    for name in K.CASES:
        w = E.expected(name)
        assert len(w.bytes) == len(w.frames) == len(w.total) == 10 and w.total[-1] > 0, name
        assert E.pcm(name).shape == ((11520,) if E.channels(name) == 1 else (11520, 2)), name
        assert E.is_mpeg1(name) == (E.kind(name).startswith("m1_") or E.kind(name) == "a1_m1"), name


def test_the_named_cases_are_of_the_kernels_they_stand_for():
    assert [E.kind(n) for n in E.PER_KERNEL] == ["m1_long", "m2_long", "a1_m1", "a1_m2"]
    assert [E.kind(n) for n in E.LIVE_GROUP] == ["m1_long", "m1_mono", "m1_hf", "m2_short", "a1_m1", "a1_m2"]
    assert [E.kind(n) for n in E.THREADED] == ["m1_long", "m1_mono", "m2_long", "m2_short"]
    assert not any(E.first_generation(n) for n in E.THREADED)
    # the re-initialisation test goes from two channels to one and on to an MPEG-2 rate
    assert (E.channels("m1_long_02"), E.channels("m1_mono_00"), E.channels("m2_long_01")) == (2, 1, 2)
    assert not E.is_mpeg1("m2_long_01")
    assert not O.OracleEncoder(O.default_control(bitrate=40)).ok()      # the rejected control of that test


@pytest.mark.parametrize("name", E.ZERO_BYTE)
def test_case_has_a_replayed_call_of_no_byte(name):
    assert zero_byte_calls(name), E.expected(name).sizes


@pytest.mark.parametrize("name", E.TWO_FRAMES)
def test_mpeg1_case_has_a_replayed_call_of_two_frames(name):
    assert E.is_mpeg1(name) and calls_advancing(name, 2), E.expected(name).frames


@pytest.mark.parametrize("name", E.THREE_FRAMES)
def test_mpeg2_case_has_a_replayed_call_of_three_frames(name):
    assert not E.is_mpeg1(name) and calls_advancing(name, 3), E.expected(name).frames


def test_the_sweeps_reach_every_edge_of_the_copy_out():
    """a replayed call of no byte at MPEG-1 stereo, MPEG-1 mono and MPEG-2; one of two frames at MPEG-1, of three at MPEG-2"""
    zero = [n for n in K.CASES if zero_byte_calls(n)]
    assert any(E.is_mpeg1(n) and E.channels(n) == 2 for n in zero)
    assert any(E.is_mpeg1(n) and E.channels(n) == 1 for n in zero)
    assert any(not E.is_mpeg1(n) for n in zero)
    assert any(E.is_mpeg1(n) and calls_advancing(n, 2) for n in K.CASES)
    assert any(not E.is_mpeg1(n) and calls_advancing(n, 3) for n in K.CASES)
    # the encoders that live side by side meet them too: a call of no byte and one of several frames while others record
    assert any(zero_byte_calls(n) for n in E.LIVE_GROUP) and any(calls_advancing(n, 2) for n in E.LIVE_GROUP)
    assert any(zero_byte_calls(n) for n in E.THREADED) and any(calls_advancing(n, 3) for n in E.THREADED)
    # the encoder beside a batch makes calls 0 .. 5 of this case: a replayed call of no byte is among them
    assert [f for f in zero_byte_calls("m1_long_02") if f < 6]


@pytest.mark.parametrize("schedule", list(E.SCHEDULES))
def test_schedules_give_every_encoder_its_calls_and_overlap_the_replays(schedule):
    n = len(E.LIVE_GROUP)
    order = E.SCHEDULES[schedule](n)
    assert [order.count(k) for k in range(n)] == [E.CALLS] * n
    assert E.most_replaying_together(order, n) >= 4
    if schedule == "uneven":
        # encoders record their graphs - their third call - while others are at different calls
        third = [[i for i, k in enumerate(order) if k == e][E.PLAIN_FIRST] for e in range(n)]
        at = [tuple(order[:i].count(k) for k in range(n)) for i in third]
        assert len(set(third)) == n and all(len(set(a)) >= 2 for a in at), at
        # the rule itself: encoder k moves on the first ten steps that k + 2 divides
        assert order == [k for _, k in sorted((m * (k + 2), k) for k in range(n) for m in range(E.CALLS))]


def test_running_average_shifts_and_rounding():
    """the recurrence on numbers worked by hand: one call of 417 bytes, then one of none"""
    assert E.running_average(True, [417]) == (417 << 8) >> 7 == 834
    assert E.running_average(False, [417]) == (417 << 8) >> 6 == 1668
    assert E.running_average(True, [417, 0]) == 834 + ((0 - 834) >> 7) == 834 - 7      # floors: -834 / 128 = -6.5 -> -7
    assert E.bitrate2_float(True, 44100, [417], 0) == 0.0
    # settles where the shifted difference reaches 0: less than 2^shift below the stream's bytes << 8
    assert E.running_average(True, [417] * 2000) == (417 << 8) - 127 and E.running_average(False, [417] * 2000) == (417 << 8) - 63
    assert abs(float(E.bitrate2_float(True, 44100, [417] * 2000, 1999)) - 127.7 * (1 - 127 / (417 << 8))) < 0.01
    assert abs(float(E.bitrate_float(True, 44100, 417 * 50, 50)) - 127.7) < 0.1
    assert abs(float(E.bitrate_float(False, 22050, 208 * 50, 50)) - 63.7) < 0.1


@pytest.mark.skipif(not E.ref_has_getters(), reason="oracle/_ref/libhmp3ref.so not built with the getters (make -C oracle ref)")
@pytest.mark.parametrize("name", ["m1_long_02", "m1_long_01", "m2_long_01"], ids=["mpeg1_cbr", "mpeg1_vbr", "mpeg2"])
def test_bitrate_getters_restated_equal_the_references_own(name):
    """enc_cases.bitrate2_float / bitrate_float from the oracle's per-call byte counts against the reference's getters, after
    every call, bit for bit"""
    assert ("bitrate" in E.control_kw(name)) == (name == "m1_long_02") and E.is_mpeg1(name) == (name != "m2_long_01")
    w = E.expected(name)
    for f, (n, frames, br2, br, ibr) in enumerate(E.ref_getters(name)):
        assert (n, frames) == (w.sizes[f], w.frames[f]), (name, f)
        assert E.f32_bits(br2) == E.f32_bits(w.bitrate2_float(f + 1)), (name, f, br2, w.bitrate2_float(f + 1))
        assert E.f32_bits(br) == E.f32_bits(w.bitrate_float(f + 1)), (name, f, br, w.bitrate_float(f + 1))
        assert ibr == int(np.float32(br) + np.float32(0.5)), (name, f)
    assert w.bitrate2_float() > 0


@pytest.mark.skipif(not E.ref_has_getters(), reason="oracle/_ref/libhmp3ref.so not built with the getters (make -C oracle ref)")
@pytest.mark.parametrize("name", ["m1_long_02", "m1_long_01", "m2_long_01"], ids=["mpeg1_cbr", "mpeg1_vbr", "mpeg2"])
def test_packet_calls_with_null_arguments_as_the_reference_makes_them(name):
    """enc_cases.packet_null_expected against the reference's own L3_audio_encode_Packet: the call with bs_out = NULL returns
    no byte and counts none while the frame counter advances, the call with packet = NULL gives the usual bitstream, and every
    other output of every call - later bitstreams, packets, sizes, both bitrate getters - is as the oracle has it"""
    want = E.packet_null_expected(name)
    assert want[E.NULL_BS_CALL][0] == 0 and len(want[E.NULL_BS_CALL][1]) > 0        # bytes were due in that call
    for f, (n, bs, frames, pk, nb, br2, br, ibr) in enumerate(E.ref_packet_null_forms(name)):
        w_n, w_bs, w_frames, w_total, w_pk, w_nb, w_br2, w_br = want[f]
        assert (n, frames) == (w_n, w_frames), (name, f)
        assert bs is None if f == E.NULL_BS_CALL else bs == w_bs, (name, f)
        assert pk is None if f == E.NULL_PACKET_CALL else (pk == w_pk and nb == w_nb), (name, f)
        assert E.f32_bits(br2) == E.f32_bits(w_br2) and E.f32_bits(br) == E.f32_bits(w_br), (name, f, br2, w_br2, br, w_br)
