"""The optional outputs of the batched calls on a real MI355X: every frame as a self-contained packet
(hx_batch_packet_buffers) and the frames / bytes emitted so far after every input frame (hx_batch_frame_stats_buffer,
hx_batch_encode_f32_host_stats, the stats of hx_batch_encode_src_host), against the oracle's restatement of
L3_audio_encode_Packet and its counters, which tests/test_oracle_vs_ref.py pins to the reference for the same controls.

Every comparison is equality.  Before each call the packet buffer is filled with 0xA5 and the sizes and counters with -1:
what a call does not write stays recognisable, and so does a byte written past a packet's end."""
import numpy as np
import pytest

import gpu_support as G
import packet_cases as PC
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import CallBufs, cut, sync
from hmp3_amd import api
from output_checks import check_call
from src_cases import Stream, make_batch

pytestmark = pytest.mark.gpu


def outputs(b, nf, frame_stride):
    """the device buffers of one call, prefilled: zeroed rows, packets of 0xA5, byte counts, sizes and counters of -1"""
    return CallBufs(b, nf, counters=True, packets=frame_stride)


def device_call(b, blk, nf, frame_stride):
    """a plain fp32 device-buffer call with packet and counter buffers of its own -> (bitstreams, packets, sizes, counters)"""
    o = G.device_call(b, blk, nf, outputs(b, nf, frame_stride).set_on(b))
    sync()
    return (o.bitstreams(),) + o.packets()


def host_call(b, blk, nf, frame_stride):
    """the fp32 host-buffer call that returns the counters (hx_batch_encode_f32_host_stats), packets to device buffers"""
    o = outputs(b, nf, frame_stride)
    o.set_on(b, stats=False)
    bs, stats = b.encode_host(blk, stats=True)
    pk, pkb, _ = o.packets()
    return bs, pk, pkb, stats


def run_calls(kw, S, calls, frame_stride, seed, bursts=lambda i: i % 2 == 0):
    """calls: [(frames, device_call | host_call)] on one batch, every call against the oracle; -> (the oracle's frames, the
    calls' packets, the calls' "bt" taps)"""
    F = sum(nf for nf, _ in calls)
    pcm = PC.packet_pcm(seed, S, F, kw, bursts=bursts)
    want = [PC.oracle_frames(kw, pcm[s]) for s in range(S)]
    lsf = kw.get("samprate", 44100) < 32000
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=max(nf for nf, _ in calls))
    f0, packets, bts = 0, [], []
    for c, (nf, route) in enumerate(calls):
        bs, pk, pkb, stats = route(b, cut(pcm, f0, nf), nf, frame_stride)
        assert b.status() == 0
        check_call(want, f0, nf, bs, pk, pkb, stats, lsf, "call %d" % c)
        packets.append((pk, pkb))
        bts.append(b.debug_read("bt", np.uint8, S * 2 * nf))
        f0 += nf
    assert all(b.frames_bytes(s) == (want[s][-1].frames_out, want[s][-1].bytes_out) for s in range(S))
    b.close()
    return want, packets, bts


# S * 3 > 8: every call is packed by the many-workgroup k_pack, not by the one-workgroup form the per-frame encoder gets.
# The layout follows the call's frame count (3, 9, 1 of max_frames 12); a stream's first frames fill the reservoir - nothing
# is emitted for them, their packets are there all the same - and frames pending at a call's end are carried into the next;
# the last call goes through the host-buffer call that returns the counters.
CALLS = [(3, device_call), (9, device_call), (1, host_call)]


# frame_stride: 4096, and an odd one (unaligned rows) that still holds the largest packet of its case: 36 bytes of header and
# side info + the 128 kbps frame's 381 + 1 + the 511-byte reservoir = 929
@pytest.mark.parametrize("kw,frame_stride", [(kw, 2003 if i == 0 else 4096) for i, kw in enumerate(PC.MPEG1)], ids=[PC.case_id(kw) for kw in PC.MPEG1])
def test_batched_packets_and_counters_equal_the_per_frame_oracle(kw, frame_stride):
    """six streams on k_alloc and k_alloc_slim (the k6_build fixture): packets, sizes, counters and bitstream of every stream
    and frame"""
    want, packets, bts = run_calls(kw, 6, CALLS, frame_stride, seed=6200)
    assert max(len(w.packet) for ws in want for w in ws) <= frame_stride
    hdr = 21 if kw.get("mode") == 3 else 36
    assert all(pkb[:, :, 0].min() >= hdr and (pkb[:, :, 1] == 0).all() for _, pkb in packets)
    # block switching is on (threshold 700) and every stream's onset is coded with short blocks: their packets are compared
    assert (np.concatenate(bts) == 2).sum() > 0


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kw", PC.MPEG2, ids=PC.case_id)
def test_mpeg2_batched_packets_and_counters(kw):
    """k_alloc_lsf: every call yields two single-granule packets back to back, the second behind the first's size"""
    want, packets, bts = run_calls(kw, 6, CALLS, 4096, seed=6300)
    assert all(pkb.min() > 0 for _, pkb in packets)
    assert (np.concatenate(bts) == 2).sum() > 0


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kw", PC.A1, ids=PC.case_id)
def test_intensity_and_dual_channel_batched_packets(kw):
    """k_alloc1 / k_alloc1_lsf: the first-generation allocator's side info in a packet, and the header's mode extension with
    the intensity flag"""
    skip_unless_host_libm_is_the_restated_one()
    want, packets, bts = run_calls(kw, 6, CALLS, 4096, seed=6400)
    if kw.get("mode", 1) != 2:      # joint stereo with an intensity part: mode extension = bits 4-5 of header byte 3, intensity = bit 4
        lsf = kw.get("samprate", 44100) < 32000
        flagged = 0
        for pk, pkb in packets:
            flagged += int((pk[:, :, 3] & 0x10 != 0).sum())
            if lsf:     # ... of the call's second packet too
                second = np.take_along_axis(pk, (pkb[:, :, 0:1] + 3).astype(np.int64), axis=2)
                flagged += int((second & 0x10 != 0).sum())
        assert flagged > 0
    else:
        assert all(((pk[:, :, 3] >> 6) == 2).all() for pk, _ in packets)        # dual channel


@pytest.mark.parametrize("kw,S", [(dict(bitrate=64), 3), (dict(bitrate=32, samprate=22050), 2)], ids=["mpeg1_3x2", "mpeg2_2x2x2"])
def test_solo_packing_with_more_than_one_stream(kw, S):
    """at most 4 streams and 8 frames in a call: one workgroup packs them all and moves the pending frames' images in and
    out of the stream state (k_pack, solo); streams behind the first, the second case with exactly 8 frames"""
    run_calls(kw, S, [(2, device_call), (2, host_call), (2, device_call)], 4096, seed=6500)


@pytest.mark.parametrize("S", [3, 6], ids=["one_workgroup_packing", "many_workgroup_packing"])
def test_buffers_set_once_hold_across_a_host_call_that_returns_the_counters(S):
    """The setters are sticky, and a host call that returns the counters takes them for itself only: packet and counter
    buffers set once, then a device call, hx_batch_encode_f32_host_stats and a device call, the buffers prefilled again
    before each without a word to the batch.  The device calls write packets, sizes and counters; the host call writes
    packets and sizes, returns its counters to the host and leaves the device counter buffer as it was prefilled.  CBR
    128, calls of 2 frames: 3 streams are packed by one workgroup, 6 by the many-workgroup k_pack."""
    import torch
    kw, nf = dict(bitrate=64), 2
    pcm = PC.packet_pcm(6800, S, 3 * nf, kw)
    want = [PC.oracle_frames(kw, pcm[s]) for s in range(S)]
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=nf)
    o = outputs(b, nf, 4096)
    o.set_on(b)
    for c in range(3):
        blk = cut(pcm, c * nf, nf)
        if c > 0:
            o.prefill()
        if c == 1:
            bs, stats = b.encode_host(blk, stats=True)
            pk, pkb, st = o.packets()
            assert (st == -1).all(), "the host call wrote the caller's device counter buffer"
        else:
            d_pcm = torch.from_numpy(blk).to(torch.device("cuda:0"))
            torch.cuda.synchronize()
            b.encode_device(d_pcm.data_ptr(), nf, o.ptr, o.stride, o.nb.data_ptr(), torch.cuda.current_stream().cuda_stream, f32=True)
            torch.cuda.synchronize()
            bs, (pk, pkb, stats) = o.bitstreams(), o.packets()
        assert b.status() == 0
        check_call(want, c * nf, nf, bs, pk, pkb, stats, 0, "call %d" % c)
    b.close()


def test_packets_and_counters_are_indexed_by_stream_under_a_launch_order(monkeypatch):
    """HMP3AMD_LPT=3: the stream walk's workgroups start in the order of the previous call's durations; packets, sizes and
    counters belong to the stream, not to the workgroup"""
    monkeypatch.setenv("HMP3AMD_LPT", "3")
    kw, S, nf, calls = dict(vbr_mnr=60), 24, 6, 3
    pcm = PC.packet_pcm(6600, S, nf * calls, kw, bursts=lambda i: i % 3 == 0)
    want = [PC.oracle_frames(kw, pcm[s]) for s in range(S)]
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=nf)
    for c in range(calls):
        bs, pk, pkb, stats = device_call(b, cut(pcm, c * nf, nf), nf, 4096)
        assert b.status() == 0
        check_call(want, c * nf, nf, bs, pk, pkb, stats, 0, "call %d" % c)
        # the next call's order is this call's durations, longest first: not the identity
        dur = b.debug_read("dur", np.uint32, S).astype(np.int64)
        assert (np.diff(dur) > 0).any()
    b.close()


def submit_calls(gate, host):
    """four back-to-back submits, each with output, packet and counter buffers of its own; the packet outputs are
    switched off behind the last submit, before the wait that sends its packing out"""
    import torch
    kw, S, nf, calls = dict(bitrate=64), 24, 6, 4
    pcm = PC.packet_pcm(6700, S, nf * calls, kw)
    f32 = [True, host, True, host]          # device submits 1 and 3: the int16 form, on integral samples
    for c in range(calls):
        if not f32[c]:
            pcm[:, c * nf * 1152:(c + 1) * nf * 1152] = np.round(pcm[:, c * nf * 1152:(c + 1) * nf * 1152])
    want = [PC.oracle_frames(kw, pcm[s]) for s in range(S)]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=nf)
    if gate is not None:
        b.set_gate(gate)
    outs = [outputs(b, nf, 4096) for _ in range(calls)]
    blks = [cut(pcm, c * nf, nf) if f32[c] else cut(pcm, c * nf, nf).astype(np.int16) for c in range(calls)]
    if host:
        ins = [torch.from_numpy(x).pin_memory() for x in blks]
        h_out = [torch.zeros((S, o.stride), dtype=torch.uint8).pin_memory() for o in outs]
        h_nb = [torch.full((S,), -1, dtype=torch.int32).pin_memory() for _ in outs]
    else:
        ins = [torch.from_numpy(x).to(dev) for x in blks]
    torch.cuda.synchronize()
    for c in range(calls):
        outs[c].set_on(b)
        if host:
            b.submit_host(ins[c].data_ptr(), nf, h_out[c].data_ptr(), outs[c].stride, h_nb[c].data_ptr(), f32=True)
        else:
            b.submit_device(ins[c].data_ptr(), nf, outs[c].ptr, outs[c].stride, outs[c].nb.data_ptr(), st, f32=f32[c])
    b.packet_buffers(None, 0, None)
    b.frame_stats_buffer(None)
    if host:
        b.wait_host()
    else:
        b.wait(st)
    torch.cuda.synchronize()
    assert b.status() == 0
    for c in range(calls):
        if host:
            o, n = h_out[c].numpy(), h_nb[c].numpy()
            bs = [o[s, :n[s]].tobytes() for s in range(S)]
        else:
            bs = outs[c].bitstreams()
        check_call(want, c * nf, nf, bs, *outs[c].packets(), 0, "%s submit %d" % ("host" if host else "device", c))
    b.close()


@pytest.mark.parametrize("route", ["device_gate90", "device_gate0", "host"])
def test_submitted_calls_write_the_packet_buffers_set_at_their_submit(route):
    """A device-buffer submit's packing goes out later - behind the next submit's stream walk, or at the wait - and must
    write the packet buffer that was in force at the submit, where the stream walk has put the packets' headers and side
    info: with buffers alternated per submit, a packing that took the buffer in force when it went out put call n's main
    data into call n + 1's packets, and behind a switch-off stored through a null pointer.  hx_batch_submit_f32_device and
    the int16 form in turn, under the default gate and ungated; the host-buffer submits (hx_batch_submit_f32_host), which
    pack at once, the same."""
    submit_calls({"device_gate90": None, "device_gate0": 0, "host": None}[route], route == "host")


def test_converting_batch_packets_and_counters():
    """a converting batch (hx_batch_create_src): the packets and counters of what k_src converted - expected from the call's
    "srcpcm" tap (pinned to the reference's converter by test_srcpcm_tap_equals_the_reference_converter) through the
    oracle under the control the encoder runs behind the converter"""
    A = api
    streams = [Stream(48000, 24, 0, mpeg_select=44100, seed=71), Stream(32000, 32, 1, mpeg_select=44100, seed=72)]
    S = len(streams)
    controls = []
    for s in streams:
        ec, nbytes = A.src_encode_control(s.ec, s.src)
        assert nbytes > 0 and ec.samprate == 44100
        controls.append(ec)
    b = make_batch(streams, 6)
    pos, f0 = [0] * S, 0
    encs = [PC.O.OracleEncoder(PC.oracle_control(ec)) for ec in controls]
    for c, nf in enumerate((4, 6)):
        stride = b.in_stride(nf)
        rows = np.zeros((S, stride), np.uint8)
        for i, s in enumerate(streams):
            chunk = np.frombuffer(s.data[pos[i]:pos[i] + stride], np.uint8)
            rows[i, :len(chunk)] = chunk
        o = outputs(b, nf, 4096)
        o.set_on(b, stats=False)
        bs, used, stats = b.encode_src_host(rows, nf, stats=True)
        assert b.status() == 0
        pk, pkb, _ = o.packets()
        conv = b.debug_read("srcpcm", np.float32, S * nf * 1152 * 2).reshape(S, nf * 1152, 2)
        assert (conv != np.round(conv)).any()
        want = []
        for i in range(S):
            frames = []
            for f in range(nf):
                wbs, wpk = encs[i].encode_packet(conv[i, f * 1152:(f + 1) * 1152])
                frames.append(PC.Frame(wbs, wpk, tuple(encs[i].packet_sizes), encs[i].frames_out(), encs[i].bytes_out()))
            want.append(frames)
            pos[i] += int(used[i])
        check_call(want, 0, nf, bs, pk, pkb, stats, 0, "call %d" % c)
    assert all(e.bytes_out() > 0 for e in encs)
    b.close()
