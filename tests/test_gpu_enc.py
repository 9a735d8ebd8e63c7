"""The per-frame encoder (hx_enc_*, the CMp3Enc drop-in) on a real MI355X, through the C ABI: every kind of stream on the
route its calls take from the third on - the replay of a HIP graph recorded once, k_pack's solo branch writing the results to
page-locked host memory - and on the plain route; several encoders alive at once, on one thread in two interleavings, beside a
batch with a pipelined submit in flight, and on threads of their own; re-initialisation of an encoder that holds a graph; the
packet calls and their NULL forms.  The inputs and what they cover: tests/enc_cases.py, tests/test_enc_cases.py.  Every
comparison is == against the oracle (bytes, counters, the getters bit for bit), and hx_enc_debug_calls says which route the
calls took: a recording that fails leaves the bytes right and these tests red.
Run with: python -m pytest tests/test_gpu_enc.py -m gpu"""
import ctypes as C
import threading

import numpy as np
import pytest

import enc_cases as E
import src_cases
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import CallBufs, cur_stream, device_call, oracle_bytes, sync
from hmp3_amd import api, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
REPLAYED = (E.PLAIN_FIRST, E.CALLS - E.PLAIN_FIRST, 1)


def libm_gate(names):
    if any(E.first_generation(n) for n in names):
        skip_unless_host_libm_is_the_restated_one()


# ---- every case on the replayed route ----

@pytest.mark.parametrize("name", E.names("m1_long", "m1_short", "m1_mono", "m1_hf"))
def test_replayed_route_on_k_alloc_and_k_alloc_slim(name):
    """the four MPEG-1 kinds of the second-generation allocator, on both builds of the stream walk (the k6_build fixture)"""
    E.run_case(api, name, REPLAYED)


@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", E.names("m2_long", "m2_short", "a1_m1", "a1_m2"))
def test_replayed_route_on_the_other_kernels(name):
    """k_alloc_lsf, k_alloc1, k_alloc1_lsf"""
    libm_gate([name])
    E.run_case(api, name, REPLAYED)


# ---- the plain route gives the same bytes, and the switch works ----

@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", E.PER_KERNEL)
def test_plain_route_under_the_environment_switch(name, monkeypatch):
    """HMP3AMD_ENC_GRAPH=0, read when the encoder first considers recording: ten plain calls, the same bytes and counters"""
    libm_gate([name])
    monkeypatch.setenv("HMP3AMD_ENC_GRAPH", "0")
    E.run_case(api, name, (E.CALLS, 0, -1))


# ---- several live encoders on one thread ----

@pytest.mark.one_k6_build
@pytest.mark.parametrize("schedule", list(E.SCHEDULES))
def test_live_encoders_interleaved_on_one_thread(schedule):
    """Six encoders, one per kernel family, created before the first call and driven call by call in the schedule's order, so
    that each records its graph while the others hold theirs or have yet to; the first two to finish are destroyed while the
    others still have calls to make, the rest in an order that is not the order of creation."""
    libm_gate(E.LIVE_GROUP)
    encs = [E.Enc(api, n) for n in E.LIVE_GROUP]
    closed = []
    for k in E.SCHEDULES[schedule](len(encs)):
        encs[k].call()
        if encs[k].done() and len(closed) < 2:
            assert not all(x.done() for x in encs)
            encs[k].check_getters()
            assert encs[k].e.debug_calls() == REPLAYED, (encs[k].name, encs[k].e.debug_calls(), api.last_error())
            encs[k].close()
            closed.append(k)
    assert len(closed) == 2 and all(x.done() for x in encs)
    rest = [k for k in (3, 5, 2, 4, 0, 1) if k not in closed]
    for k in rest:
        encs[k].check_getters()
        assert encs[k].e.debug_calls() == REPLAYED, (encs[k].name, encs[k].e.debug_calls(), api.last_error())
    assert rest != sorted(rest)
    for k in rest:
        encs[k].close()


# ---- re-initialisation among live encoders ----

@pytest.mark.one_k6_build
def test_reinitialising_an_encoder_that_holds_a_graph():
    """m1_long_02 to completion, then the same hx_enc initialised to m1_mono_00 (one channel: another stride), then a rejected
    control, then m2_long_01; every segment compared from its first call, the counters restart with each init, and a neighbour
    that holds a graph of its own makes calls in between and stays right."""
    neighbour = E.Enc(api, "m2_short_03")
    x = E.Enc(api, "m1_long_02")
    neighbour.run(3)
    x.run()
    x.check_getters()
    assert x.e.debug_calls() == REPLAYED
    neighbour.run(5)
    x.init("m1_mono_00")        # (asserts the init's return value, debug_calls() == (0, 0, 0) and zeroed counters)
    x.run(4)
    neighbour.run(7)
    x.run()
    x.check_getters()
    assert x.e.debug_calls() == REPLAYED
    assert x.e.L3_audio_encode_init(api.default_control(bitrate=40)) == 0
    assert x.e.debug_calls() == (0, 0, 0)
    neighbour.run(8)
    x.init("m2_long_01")
    x.run(5)
    neighbour.run()
    x.run()
    x.check_getters()
    assert x.e.debug_calls() == REPLAYED
    neighbour.check_getters()
    assert neighbour.e.debug_calls() == REPLAYED
    x.close()
    neighbour.close()


# ---- packet calls ----

def oracle_of(ec):
    """an oracle encoder of an api.EControl (the two structures have one layout)"""
    oc = O.Control()
    assert C.sizeof(oc) == C.sizeof(ec)
    C.memmove(C.byref(oc), C.byref(ec), C.sizeof(oc))
    enc = O.OracleEncoder(oc)
    assert enc.ok()
    return enc


@pytest.mark.one_k6_build
@pytest.mark.parametrize("source", ["s16_44k_stereo_cbr128", "s16_44k_to_22k_mono"])
def test_mp3_audio_encode_packet_from_a_source(source):
    """hx_enc_MP3_audio_encode_Packet: convert, encode, and the call's frame(s) as packets.  The expected floats are the host
    converter's (pinned to the reference's in tests/test_src_convert.py), the expected bytes and packets the oracle's on them."""
    if source == "s16_44k_stereo_cbr128":
        s, packets = src_cases.Stream(44100, 16, 0, channels=2, seed=71, bitrate=64), 1
    else:
        s, packets = src_cases.Stream(44100, 16, 0, channels=2, mpeg_select=2, mono_convert=1, seed=72, bitrate=32), 2
    ec2, need = api.src_encode_control(s.ec, s.src)
    assert ec2 is not None and ec2.samprate == (44100 if packets == 1 else 22050) and (ec2.mode == 3) == (packets == 2)
    y, used, tch = src_cases.host_converted(s, E.CALLS, target=ec2.samprate)
    assert tch == (1 if packets == 2 else 2)
    o = oracle_of(ec2)
    e = api.Mp3Enc()
    assert e.MP3_audio_encode_init(s.ec, s.bits, s.is_float, s.mpeg_select, s.mono_convert) == need
    buf = (C.c_ubyte * len(s.data)).from_buffer_copy(s.data)
    pos, total = 0, 0
    for f in range(E.CALLS):
        want_bs, want_pk = o.encode_packet(y[f * 1152:(f + 1) * 1152])
        nin, nout, bs, pk = e.MP3_audio_encode_Packet(C.byref(buf, pos))
        assert nin == used[f], "call %d: in_bytes" % f
        assert nout == len(want_bs) and bs == want_bs, "call %d: bitstream" % f
        assert e.packet_sizes == tuple(o.packet_sizes) and pk == want_pk, "call %d: packet" % f
        assert e.packet_sizes[0] > 0 and (e.packet_sizes[1] > 0) == (packets == 2), "call %d" % f
        pos += nin
        total += nout
        assert e.L3_audio_encode_get_frames_bytes() == (o.frames_out(), total) and o.bytes_out() == total, "call %d" % f
    assert total > 0
    assert e.debug_calls() == (E.CALLS, 0, 0)
    e.close()


@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", ["m1_long_02", "m2_long_01"])
def test_packet_calls_with_a_null_bitstream_or_a_null_packet(name):
    """hx_enc_L3_audio_encode_Packet: call 4 with bs_out = NULL, call 5 with packet = NULL.  Every output of every call is
    enc_cases.packet_null_expected's, which tests/test_enc_cases.py pins to the reference: the call without a bitstream buffer
    returns and counts no byte while its frames count as sent, and every later call's bitstream is the oracle's.  No call of
    an encoder driven by packet calls alone is a replay."""
    e = api.Mp3Enc()
    assert e.L3_audio_encode_init(api.default_control(**E.control_kw(name))) == 4608 * E.channels(name)
    for f, (w_n, w_bs, w_frames, w_total, w_pk, w_nb, w_br2, w_br) in enumerate(E.packet_null_expected(name)):
        nin, nout, bs, pk = e.L3_audio_encode_Packet_opt(E.block(name, f), bs_out=f != E.NULL_BS_CALL, packet=f != E.NULL_PACKET_CALL)
        assert nin == 4608 * E.channels(name) and nout == w_n, "call %d: %d bytes, expected %d" % (f, nout, w_n)
        assert (bs is None) if f == E.NULL_BS_CALL else (bs == w_bs), "call %d: bitstream" % f
        if f == E.NULL_PACKET_CALL:
            assert pk is None and e.packet_sizes == (-1, -1)       # nothing written without a packet
        else:
            assert pk == w_pk and e.packet_sizes == w_nb, "call %d: packet" % f
        assert e.L3_audio_encode_get_frames_bytes() == (w_frames, w_total), "call %d" % f
        assert E.f32_bits(e.L3_audio_encode_get_bitrate2_float()) == E.f32_bits(w_br2), "call %d" % f
        assert E.f32_bits(e.L3_audio_encode_get_bitrate_float()) == E.f32_bits(w_br), "call %d" % f
    assert e.debug_calls() == (E.CALLS, 0, 0)
    e.close()


# ---- an encoder beside a working batch ----

def test_encoder_records_its_graph_beside_a_batch_in_flight():
    """An 8-stream CBR-128 batch has pipelined device submits in flight; between the last submit and the wait an encoder
    makes calls 0 .. 5 of m1_long_02 (call 2 records its graph, and is a call of no byte).  Both sides against the oracle."""
    kw, S, F, submits = dict(bitrate=64), 8, 32, 4
    pcm = np.stack([synth.stream_pcm(1300 + i, F * submits, rho=[0.7, 0.0, 1.0, 0.3][i % 4], bursts=True) for i in range(S)])
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=F)
    bufs = [CallBufs(b, F) for _ in range(submits)]
    x = E.Enc(api, "m1_long_02")
    sync()
    for c in range(submits):
        device_call(b, pcm[:, c * F * 1152:(c + 1) * F * 1152], F, bufs[c], submit=True)
    x.run(6)
    b.wait(cur_stream())
    sync()
    assert b.status() == 0
    assert x.e.debug_calls() == (2, 4, 1), api.last_error()
    x.check_getters()
    got = [b"".join(bufs[c].bitstreams()[s] for c in range(submits)) for s in range(S)]
    for s in range(S):
        assert got[s] == oracle_bytes(kw, pcm[s], F * submits), "stream %d" % s
    x.close()
    b.close()


# ---- encoders on threads of their own ----

@pytest.mark.one_k6_build
def test_encoders_on_threads_of_their_own():
    """Four threads, each with an encoder it creates, drives through its case's ten calls and destroys; a barrier lets them
    start together (ctypes releases the GIL in a call).  The main thread has made a call before, so the code objects are
    loaded.  Once, not in a loop."""
    E.Enc(api, "m1_long_02").run(1).close()
    for n in E.THREADED:
        E.expected(n)               # (computed here: the threads only read them)
    gate = threading.Barrier(len(E.THREADED))
    route, failed = {}, {}

    def work(name):
        try:
            x = E.Enc(api, name)
            gate.wait(timeout=60)
            x.run()
            x.check_getters()
            route[name] = x.e.debug_calls()
            x.close()
        except BaseException as err:       # (reported by the main thread, with this thread's hx_last_error)
            failed[name] = "%r; hx_last_error: %s" % (err, api.last_error())
            gate.abort()

    threads = [threading.Thread(target=work, args=(n,)) for n in E.THREADED]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failed, failed
    assert route == {n: REPLAYED for n in E.THREADED}, route
