"""Slot operations in stream order (hx_batch_reset_streams, hx_batch_get / set_stream_states[_device]; kernels in
hmp3_amd/csrc/hx_slots.hip): many slots reset, saved or restored in one launch, enqueued like a plain device call.

Shapes are the smallest that can go wrong: six slots over three configuration classes, calls of 2 to 7 frames cut out of
a signal around one of its noise bursts, so that the reservoir, the pending-frame ring and the block-switching state all
hold something when a slot is saved.  Expected bytes are the oracle's; blobs are compared bit for bit."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import ints, oracle_bytes, states
from hmp3_amd import api, synth
from src_cases import Stream, make_batch, make_rows, run

pytestmark = pytest.mark.gpu

KWS = [dict(bitrate=64), dict(vbr_mnr=70), dict(bitrate=64, samprate=48000)]
S = 6
T0 = 9          # the calls start at frame T0 of a 24-frame signal: its first burst lies in frame 13 (44.1 kHz) / 14 (48 kHz)
RESET = [5, 0, 2]   # not monotone, first and last slot included


@functools.lru_cache(maxsize=None)
def sig(seed, i, rate=None, mono=False):
    """frames T0 .. 23 of a signal with bursts, at the rate of stream i's class in KWS (or at `rate`)"""
    sr = KWS[i % 3].get("samprate", 44100) if rate is None else rate
    x = synth.stream_pcm(seed + i, 24, sr=sr, bursts=True)[T0 * 1152:]
    x = np.ascontiguousarray(x[:, 0] if mono else x)
    x.setflags(write=False)
    return x


def calls_pcm(seed, F, rate=None, mono=False, n=S):
    return np.stack([sig(seed, i, rate, mono)[:F * 1152] for i in range(n)])


@functools.lru_cache(maxsize=None)
def expected(i, n1, n2, fresh):
    """stream i over n1 frames of the first signal and n2 of the second: (bytes of the first call, of the second) - the second
    as a new stream (fresh) or as the continuation"""
    a, b = sig(1500, i)[:n1 * 1152], sig(1600, i)[:n2 * 1152]
    first = oracle_bytes(KWS[i % 3], a)
    if fresh:
        return first, oracle_bytes(KWS[i % 3], b)
    both = oracle_bytes(KWS[i % 3], np.concatenate([a, b]))
    assert both[:len(first)] == first
    return first, both[len(first):]


def slot_controls():
    return [api.default_control(**KWS[i % 3]) for i in range(S)]


@pytest.mark.parametrize("F1,F2", [(6, 5), (7, 2)], ids=["6_then_5", "7_then_2_stale_subband_slots"])
def test_reset_of_many_slots(F1, F2, k6_build):
    """the reset slots equal a new batch's bit for bit, the others are not touched, and the next call encodes the new
    inputs from scratch - also when it is shorter than the one before, so that subband slots written by the earlier call
    lie beyond its extent (only slots 0..2 are zeroed)"""
    b = api.Batch(slot_controls(), nstreams=S, max_frames=7)
    fresh = api.Batch(slot_controls(), nstreams=S, max_frames=7)
    out1 = b.encode_host(calls_pcm(1500, F1))
    before = states(b, single=True)
    b.reset_streams(RESET)
    after, new = states(b, single=True), states(fresh, single=True)
    for i in range(S):
        assert after[i] == (new[i] if i in RESET else before[i]), i
        assert (before[i] != new[i]), i         # (the first call left something to reset)
    out2 = b.encode_host(calls_pcm(1600, F2))
    assert b.status() == 0
    for i in range(S):
        assert (out1[i], out2[i]) == expected(i, F1, F2, i in RESET), i
    b.close(); fresh.close()


@pytest.mark.parametrize("counts", [False, True], ids=["uniform", "per_stream_counts"])
def test_reset_between_pipelined_submits_without_a_wait(counts, k6_build):
    """submit, reset_streams, submit on one stream with two output sets in turn, then wait: the reset is ordered behind
    the first submit (its deferred packing included) and in front of the second; under counts some reset slots sat the
    first submit out"""
    import torch
    F1, F2 = 6, 5
    n1 = [0, 6, 4, 5, 6, 0] if counts else [F1] * S
    n2 = [5, 5, 3, 0, 4, 5] if counts else [F2] * S
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_pcm = [torch.from_numpy(calls_pcm(1500, F1)).to(dev), torch.from_numpy(calls_pcm(1600, F2)).to(dev)]
    b = api.Batch(slot_controls(), nstreams=S, max_frames=7)
    stride = b.out_stride(7)
    d_out = [torch.zeros((S, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
    d_nb = [torch.zeros((S,), dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    if counts:
        b.frame_counts(n1)
    b.submit_device(d_pcm[0].data_ptr(), F1, d_out[0].data_ptr(), stride, d_nb[0].data_ptr(), st)
    b.reset_streams(RESET, st)
    if counts:
        b.frame_counts(n2)
    b.submit_device(d_pcm[1].data_ptr(), F2, d_out[1].data_ptr(), stride, d_nb[1].data_ptr(), st)
    b.wait(st)
    torch.cuda.synchronize()
    assert b.status() == 0
    got = []
    for c in range(2):
        o, n = d_out[c].cpu().numpy(), d_nb[c].cpu().numpy()
        got.append([o[s, :n[s]].tobytes() for s in range(S)])
    for i in range(S):
        assert (got[0][i], got[1][i]) == expected(i, n1[i], n2[i], i in RESET), i
    b.close()


def test_single_slot_reset_over_stale_subband_slots(k6_build):
    """hx_batch_reset_stream zeroes subband slots 0..2 like the list call: a 7-frame call, two slots reset one by one, then
    2-frame calls of new input - the subband slots the long call wrote lie beyond the short calls' extent.  The reset slots
    encode the new input from scratch, the others continue"""
    F1, F2, reset = 7, 2, [4, 1]
    b = api.Batch(slot_controls(), nstreams=S, max_frames=7)
    out1 = b.encode_host(calls_pcm(1500, F1))
    for i in reset:
        b.reset_stream(i)
    new = calls_pcm(1600, 2 * F2)
    out2 = [x + y for x, y in zip(b.encode_host(new[:, :F2 * 1152]), b.encode_host(new[:, F2 * 1152:]))]
    assert b.status() == 0
    for i in range(S):
        assert (out1[i], out2[i]) == expected(i, F1, 2 * F2, i in reset), i
    b.close()


HEADER = struct.Struct("<IIIIQ")        # HxStateHeader: magic, format version, sizeof(HxStream), 0, configuration fingerprint
CARRY = 3 * 576 * 4                     # bytes of the three carried subband granules of one channel


def saved_both_ways(b, idx):
    """the blobs of the slots in idx from the list call - nothing is written behind the array, every blob ends in zeros up to
    the stride - and from the single-slot call, which gives the same bytes -> the blobs"""
    need, stride = int(api.lib().hx_batch_stream_state_bytes(b.h)), b.states_stride()
    arr, n = ints(idx)
    buf = np.full(n * stride + 64, 0xA5, np.uint8)
    assert api.lib().hx_batch_get_stream_states(b.h, arr, n, buf.ctypes.data, stride) == 0, api.last_error()
    assert (buf[n * stride:] == 0xA5).all()
    blobs = []
    for e, i in enumerate(idx):
        blob = buf[e * stride:(e + 1) * stride]
        assert not blob[need:].any(), (e, i)
        blobs.append(blob[:need].tobytes())
        assert blobs[e] == b.get_stream_state(i), (e, i)
    return blobs


def header_state_carry(b, i, blob, magic, max_frames):
    """blob = header {magic, 3, sizeof(HxStream), 0, cfg}, row i of the "state" tap, slots 0..2 of both channels of row i of the
    "sb" tap, the rest -> (cfg, the rest)"""
    n = b.n
    state = b.debug_read("state", np.uint8, 1 << 22)
    st = len(state) // n
    row = (2 * max_frames + 3) * 576
    sb = b.debug_read("sb", np.float32, n * 2 * row).reshape(n, 2, row)
    assert len(state) == n * st and blob[:4] == magic
    m, version, state_bytes, pad, cfg = HEADER.unpack(blob[:HEADER.size])
    assert (version, state_bytes, pad) == (3, st, 0)
    assert blob[HEADER.size:HEADER.size + st] == state[i * st:(i + 1) * st].tobytes(), i
    assert blob[HEADER.size + st:HEADER.size + st + 2 * CARRY] == sb[i, :, :3 * 576].tobytes(), i
    return cfg, blob[HEADER.size + st + 2 * CARRY:]


@functools.lru_cache(maxsize=None)
def converting_streams():
    """six sources over two converter plans and configurations: 48 kHz -> 44.1 kHz (case 4, carried samples) and 44.1 -> 32 kHz"""
    return [Stream(*((48000, 16, 0) if i % 2 == 0 else (44100, 16, 0)), mpeg_select=44100 if i % 2 == 0 else 32000, seed=60 + i, seconds=1.0)
            for i in range(S)]


@pytest.mark.one_k6_build
@pytest.mark.parametrize("idx", [[4, 0, 3], [2], list(range(S))], ids=["three", "one", "all"])
def test_gather_equals_the_single_slot_call(idx):
    """what a blob holds, after two uneven calls, against the batch's debug taps; the list form and the single-slot form give
    the same bytes.  A plain batch of three classes; a converting batch of two plans, whose blob goes on with the plan's
    fingerprint, the stream's converter call count and the carried samples"""
    b = api.Batch(slot_controls(), nstreams=S, max_frames=7)
    for seed, F, counts in ((1500, 5, [5, 2, 4, 0, 3, 5]), (1600, 3, [2, 3, 0, 3, 1, 2])):
        b.frame_counts(counts)
        b.encode_host(calls_pcm(seed, F))
    blobs = saved_both_ways(b, idx)
    for e, i in enumerate(idx):
        cfg, rest = header_state_carry(b, i, blobs[e], b"HX3S", 7)
        assert rest == b"", i
    cfgs = [HEADER.unpack(x[:HEADER.size])[4] for x in states(b, single=True)]
    for i in range(S):
        for j in range(S):
            assert (cfgs[i] == cfgs[j]) == (i % 3 == j % 3), (i, j)
    assert b.status() == 0
    b.close()

    streams = converting_streams()
    b = make_batch(streams, 7)
    pos, done = [0] * S, [0] * S
    for F, counts in ((5, [5, 2, 4, 0, 3, 5]), (3, [2, 3, 0, 3, 1, 2])):
        _, used = b.encode_src_counts_host(make_rows(b, streams, pos, F, counts), F, counts)
        pos = [p + int(u) for p, u in zip(pos, used)]
        done = [d + c for d, c in zip(done, counts)]

    def converter_words(idx):
        out = {}
        for i, blob in zip(idx, saved_both_ways(b, idx)):
            cfg, rest = header_state_carry(b, i, blob, b"HX3C", 7)
            assert len(rest) == 16 + 2 * 192 * 4, i     # plan fingerprint, call count, HX_SRC_CARRY samples per channel
            out[i] = (cfg,) + struct.unpack("<Qq", rest[:16])
        return out
    got = converter_words(idx)
    for i in idx:
        assert got[i][2] == done[i], i
        for j in idx:
            assert (got[i][1] == got[j][1]) == (i % 2 == j % 2) and (got[i][0] == got[j][0]) == (i % 2 == j % 2), (i, j)
    b.reset_stream(idx[0])
    b.reset_streams(idx[1:])
    assert all(v[2] == 0 for v in converter_words(idx).values())
    assert b.status() == 0
    b.close()


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kind", ["plain", "converting"])
def test_single_slot_save_writes_no_byte_beyond_the_state(kind):
    """hx_batch_get_stream_state into a buffer of hx_batch_stream_state_bytes + 64 bytes: the state, and the 64 bytes behind it
    untouched (the list form's blob goes on with zeros up to its stride; the single-slot call's buffer ends with the state)"""
    L = api.lib()
    if kind == "plain":
        b = api.Batch(slot_controls(), nstreams=S, max_frames=7)
        b.encode_host(calls_pcm(1500, 4))
    else:
        b = make_batch(converting_streams(), 7)
    need = int(L.hx_batch_stream_state_bytes(b.h))
    assert need < b.states_stride()
    for i in (0, S - 1):
        buf = (C.c_ubyte * (need + 64))(*([0xA5] * (need + 64)))
        assert L.hx_batch_get_stream_state(b.h, i, buf) == 0, api.last_error()
        assert bytes(buf[need:]) == b"\xA5" * 64, i
        assert bytes(buf[:need]) == b.get_stream_states([i])[0], i
    assert b.status() == 0
    b.close()


KW4 = dict(vbr_mnr=55)
PLACE = [5, 0, 3, 2]        # stream i of the source batch goes to slot PLACE[i]


@functools.lru_cache(maxsize=None)
def moved_expected(i, F1, F2):
    x = sig(1700, i, 44100)[:(F1 + F2) * 1152]
    first = oracle_bytes(KW4, x[:F1 * 1152])
    both = oracle_bytes(KW4, x)
    assert both[:len(first)] == first
    return first, both[len(first):]


def moved_second_call(F1, F2, place, nslots):
    pcm2 = np.zeros((nslots, F2 * 1152, 2), np.int16)
    for i, slot in enumerate(place):
        pcm2[slot] = sig(1700, i, 44100)[F1 * 1152:(F1 + F2) * 1152]
    return pcm2


@pytest.mark.one_k6_build
def test_scatter_into_another_batch():
    """four streams saved in one call continue in slots [5, 0, 3, 2] of a batch of another size and max_frames; its two
    other slots keep their blobs"""
    F1, F2 = 5, 6
    b1 = api.Batch(api.default_control(**KW4), nstreams=4, max_frames=5)
    out1 = b1.encode_host(calls_pcm(1700, F1, 44100, n=4))
    saved = b1.get_stream_states(range(4))
    b1.close()
    b2 = api.Batch(api.default_control(**KW4), nstreams=6, max_frames=7)
    before = states(b2, single=True)
    b2.set_stream_states(PLACE, saved)
    after = states(b2, single=True)
    for slot in (1, 4):
        assert after[slot] == before[slot]
    for i, slot in enumerate(PLACE):
        assert after[slot] == saved[i]
    out2 = b2.encode_host(moved_second_call(F1, F2, PLACE, 6))
    assert b2.status() == 0
    for i, slot in enumerate(PLACE):
        assert (out1[i], out2[slot]) == moved_expected(i, F1, F2), i
    b2.close()


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kind", ["plain", "converting"])
def test_single_slot_and_list_forms_cross(kind):
    """streams saved with the single-slot call are restored with the list call and the other way round, into other slots of a
    second batch, and continue there over two calls as if nothing had happened"""
    if kind == "plain":
        F1, F2 = 5, 6
        b1 = api.Batch(api.default_control(**KW4), nstreams=4, max_frames=5)
        out1 = b1.encode_host(calls_pcm(1700, F1, 44100, n=4))
        single, listed = [b1.get_stream_state(i) for i in (0, 1)], b1.get_stream_states([2, 3])
        b1.close()
        b2 = api.Batch(api.default_control(**KW4), nstreams=6, max_frames=7)
        b2.set_stream_states(PLACE[:2], single)
        for slot, blob in zip(PLACE[2:], listed):
            b2.set_stream_state(slot, blob)
        pcm2 = moved_second_call(F1, F2, PLACE, 6)
        out2 = [x + y for x, y in zip(b2.encode_host(pcm2[:, :4 * 1152]), b2.encode_host(pcm2[:, 4 * 1152:]))]
        assert b2.status() == 0
        for i, slot in enumerate(PLACE):
            assert (out1[i], out2[slot]) == moved_expected(i, F1, F2), i
        b2.close()
        return
    s0, s1 = (Stream(48000, 16, 0, mpeg_select=44100, seed=k, seconds=1.0) for k in (41, 42))
    b1 = make_batch([s0, s1], 8)
    o1, p1, _ = run(b1, [s0, s1], [6])
    single, listed = b1.get_stream_state(0), b1.get_stream_states([1])[0]
    b1.close()
    b2 = make_batch([s0, s0, s0], 7)
    b2.set_stream_states([2], [single])
    b2.set_stream_state(0, listed)
    o2, _, _ = run(b2, [s1, s0, s0], [3, 2], pos=[p1[1], 0, p1[0]])
    assert o1[0] + o2[2] == s0.per_frame(11)[0]
    assert o1[1] + o2[0] == s1.per_frame(11)[0]
    assert o2[1] == s0.per_frame(5)[0]
    b2.close()


@pytest.mark.one_k6_build
def test_device_blobs_move_streams_without_a_host_wait():
    """gather into a device buffer, scatter into another batch and that batch's next call, all on one stream: the bytes
    continue, nothing beyond n * blob_stride is written, a blob's tail up to the stride is zero, and the blobs are the
    host call's"""
    import torch
    F1, F2 = 5, 6
    idx, place = [2, 0, 3], [4, 1, 0]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    b1 = api.Batch(api.default_control(**KW4), nstreams=4, max_frames=5)
    out1 = b1.encode_host(calls_pcm(1700, F1, 44100, n=4))
    b2 = api.Batch(api.default_control(**KW4), nstreams=6, max_frames=7)
    need, stride = len(b1.get_stream_state(0)), b1.states_stride() + 32       # (a stride larger than the smallest)
    n, canary = len(idx), 256
    d_blobs = torch.full((n * stride + canary,), 0xA5, dtype=torch.uint8, device=dev)
    pcm2 = np.zeros((6, F2 * 1152, 2), np.int16)
    for e, i in enumerate(idx):
        pcm2[place[e]] = sig(1700, i, 44100)[F1 * 1152:(F1 + F2) * 1152]
    d_pcm = torch.from_numpy(pcm2).to(dev)
    ostride = b2.out_stride(F2)
    d_out = torch.zeros((6, ostride), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros((6,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    b1.get_stream_states_device(idx, d_blobs.data_ptr(), stride, st)
    b2.set_stream_states_device(place, d_blobs.data_ptr(), stride, st)
    b2.encode_device(d_pcm.data_ptr(), F2, d_out.data_ptr(), ostride, d_nb.data_ptr(), st)
    torch.cuda.synchronize()
    assert b1.status() == 0 and b2.status() == 0
    o, nb = d_out.cpu().numpy(), d_nb.cpu().numpy()
    for e, i in enumerate(idx):
        assert (out1[i], o[place[e], :nb[place[e]]].tobytes()) == moved_expected(i, F1, F2), i
    h = d_blobs.cpu().numpy()
    assert (h[n * stride:] == 0xA5).all()
    host = b1.get_stream_states(idx)
    for e in range(n):
        blob = h[e * stride:(e + 1) * stride]
        assert blob[:need].tobytes() == host[e], e
        assert not blob[need:].any(), e
    b1.close(); b2.close()


@pytest.mark.one_k6_build
def test_refusals_leave_the_batch_unchanged():
    import torch
    A = api
    L = A.lib()
    b = A.Batch(slot_controls(), nstreams=S, max_frames=7)
    b.encode_host(calls_pcm(1500, 5))
    before = states(b, single=True)
    need, stride = len(before[0]), b.states_stride()
    assert stride % 16 == 0 and need <= stride < need + 16
    host = np.zeros(S * (stride + 16), dtype=np.uint8)
    d_buf = torch.zeros(S * (stride + 16) + 16, dtype=torch.uint8, device="cuda:0")
    hp, dp = host.ctypes.data, d_buf.data_ptr()
    for idx, n, word in (([1, 3, 1], None, "entry 2"), ([0, -1], None, "entry 1"), ([S], None, "entry 0"), ([0, 1], -1, "n = -1")):
        arr, k = ints(idx)
        k = k if n is None else n
        for call in (lambda: L.hx_batch_reset_streams(b.h, arr, k, None),
                     lambda: L.hx_batch_get_stream_states(b.h, arr, k, hp, stride),
                     lambda: L.hx_batch_set_stream_states(b.h, arr, k, hp, stride),
                     lambda: L.hx_batch_get_stream_states_device(b.h, arr, k, dp, stride, None),
                     lambda: L.hx_batch_set_stream_states_device(b.h, arr, k, dp, stride, None)):
            assert call() == -1 and word in A.last_error(), (idx, n, A.last_error())
    arr, k = ints([0, 1])
    for bad in (stride - 16, need | 8):
        assert bad < need or bad % 16
        for call in (lambda: L.hx_batch_get_stream_states(b.h, arr, k, hp, bad), lambda: L.hx_batch_set_stream_states(b.h, arr, k, hp, bad),
                     lambda: L.hx_batch_get_stream_states_device(b.h, arr, k, dp, bad, None),
                     lambda: L.hx_batch_set_stream_states_device(b.h, arr, k, dp, bad, None)):
            assert call() == -1 and "blob_stride %d" % bad in A.last_error(), A.last_error()
    for call in (lambda: L.hx_batch_get_stream_states_device(b.h, arr, k, dp + 8, stride, None),
                 lambda: L.hx_batch_set_stream_states_device(b.h, arr, k, dp + 8, stride, None)):
        assert call() == -1 and "16-byte aligned" in A.last_error()
    assert L.hx_batch_reset_streams(b.h, None, 2, None) == -1 and "idx" in A.last_error()
    # n = 0: nothing to do
    assert L.hx_batch_reset_streams(b.h, None, 0, None) == 0
    assert L.hx_batch_get_stream_states(b.h, None, 0, None, stride) == 0 and L.hx_batch_set_stream_states(b.h, None, 0, None, stride) == 0
    assert L.hx_batch_get_stream_states_device(b.h, None, 0, None, stride, None) == 0
    assert L.hx_batch_set_stream_states_device(b.h, None, 0, None, stride, None) == 0
    assert not host.any() and not d_buf.cpu().numpy().any()
    assert states(b, single=True) == before
    assert b.status() == 0

    # a host blob with a flipped fingerprint: none of the listed slots is written
    saved = b.get_stream_states([0, 1, 2])
    bad = bytearray(saved[1]); bad[16] ^= 1
    b2 = A.Batch(slot_controls(), nstreams=S, max_frames=7)
    new = states(b2, single=True)
    with pytest.raises(RuntimeError, match="entry 1: the stream state was saved under a different configuration"):
        b2.set_stream_states([3, 4, 5], [saved[0], bytes(bad), saved[2]])
    assert states(b2, single=True) == new and b2.status() == 0
    # the device variant cannot refuse: the kernel leaves that slot alone, restores the others and says so in the status
    up = np.zeros(3 * stride, dtype=np.uint8)
    for e, blob in enumerate([saved[0], bytes(bad), saved[2]]):
        up[e * stride:e * stride + need] = np.frombuffer(blob, dtype=np.uint8)
    d_up = torch.from_numpy(up).to("cuda:0")
    torch.cuda.synchronize()
    b2.set_stream_states_device([3, 4, 5], d_up.data_ptr(), stride, None)
    assert b2.status() == 32
    got = states(b2, single=True)
    assert got[3] == saved[0] and got[5] == saved[2] and got[4] == new[4]
    assert got[:3] == new[:3]
    b.close(); b2.close()


OTHER = {"mpeg2_22k": (dict(bitrate=32, samprate=22050), False), "first_generation_intensity": (dict(bitrate=64, nsbstereo=8), False),
         "mono": (dict(bitrate=64, mode=3), True)}


@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", list(OTHER))
def test_other_kinds_of_batch(name):
    """MPEG-2 (two frames per block), the first-generation allocator's kernels and a mono batch (its second carry channel is
    unused): one slot is reset, another saved and restored into a second batch, in one sequence"""
    kw, mono = OTHER[name]
    if "intensity" in name:
        skip_unless_host_libm_is_the_restated_one()
    F, n, sr = 4, 3, kw.get("samprate", 44100)
    first, second = calls_pcm(1800, F, sr, mono, n), calls_pcm(1900, F, sr, mono, n)
    b = api.Batch(api.default_control(**kw), nstreams=n, max_frames=F)
    b2 = api.Batch(api.default_control(**kw), nstreams=n, max_frames=F + 1)
    out1 = b.encode_host(first)
    b.reset_streams([1])
    b2.set_stream_states([0], b.get_stream_states([2]))
    out2 = b.encode_host(second)
    moved = b2.encode_host(np.stack([second[2], second[0], second[1]]))
    assert b.status() == 0 and b2.status() == 0
    for i in range(n):
        assert out1[i] == oracle_bytes(kw, first[i]), i
    assert out2[1] == oracle_bytes(kw, second[1])
    for i in (0, 2):
        assert out1[i] + out2[i] == oracle_bytes(kw, np.concatenate([first[i], second[i]])), i
    assert moved[0] == out2[2]
    assert moved[1] == oracle_bytes(kw, second[0])
    b.close(); b2.close()


@pytest.mark.one_k6_build
def test_converting_batch():
    """48 kHz s16 -> 44.1 kHz (a case-4 plan, with carried samples): reset_streams restarts the converter too, the host
    calls move a stream with its converter to another converting batch, and device blobs are refused"""
    import torch
    A = api
    L = A.lib()
    s0, s1, snew = (Stream(48000, 16, 0, mpeg_select=44100, seed=k, seconds=1.0) for k in (41, 42, 43))
    b1 = make_batch([s0, s1], 8)
    o1, p1, _ = run(b1, [s0, s1], [6])
    def schedule(b):
        nb, rd = b.schedule(0, 5)
        return nb.tolist(), rd
    bnew = make_batch([s0], 8)
    new_schedule = schedule(bnew)
    bnew.close()
    assert schedule(b1) != new_schedule
    saved = b1.get_stream_states([1])
    assert saved == [b1.get_stream_state(1)]
    b1.reset_streams([0])
    assert schedule(b1) == new_schedule
    o2, _, _ = run(b1, [snew, s1], [5], pos=[0, p1[1]])
    assert o2[0] == snew.per_frame(5)[0]
    assert o1[1] + o2[1] == s1.per_frame(11)[0]
    b2 = make_batch([s0, s0, s0], 7)
    b2.set_stream_states([2], saved)
    o3, _, _ = run(b2, [s0, s0, s1], [5], pos=[0, 0, p1[1]])
    assert o3[2] == o2[1]
    assert o3[0] == s0.per_frame(5)[0]
    d = torch.zeros(b1.states_stride(), dtype=torch.uint8, device="cuda:0")
    arr, k = ints([0])
    before = states(b1, single=True)
    assert L.hx_batch_get_stream_states_device(b1.h, arr, k, d.data_ptr(), b1.states_stride(), None) == -1 and "converting" in A.last_error()
    assert L.hx_batch_set_stream_states_device(b1.h, arr, k, d.data_ptr(), b1.states_stride(), None) == -1 and "converting" in A.last_error()
    assert states(b1, single=True) == before and b1.status() == 0
    b1.close(); b2.close()
