"""Slot operations in stream order (hx_batch_reset_streams, hx_batch_get / set_stream_states[_device]; kernels in
hmp3_amd/csrc/hx_slots.hip): many slots reset, saved or restored in one launch, enqueued like a plain device call.

Shapes are the smallest that can go wrong: six slots over three configuration classes, calls of 2 to 7 frames cut out of
a signal around one of its noise bursts, so that the reservoir, the pending-frame ring and the block-switching state all
hold something when a slot is saved.  Expected bytes are the oracle's; blobs are compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from hmp3_amd import synth
from conftest import skip_unless_host_libm_is_the_restated_one

pytestmark = pytest.mark.gpu

KWS = [dict(bitrate=64), dict(vbr_mnr=70), dict(bitrate=64, samprate=48000)]
S = 6
T0 = 9          # the calls start at frame T0 of a 24-frame signal: its first burst lies in frame 13 (44.1 kHz) / 14 (48 kHz)
RESET = [5, 0, 2]   # not monotone, first and last slot included


def api():
    from hmp3_amd import api as a
    return a


@functools.lru_cache(maxsize=None)
def sig(seed, i, rate=None, mono=False):
    """frames T0 .. 23 of a signal with bursts, at the rate of stream i's class in KWS (or at `rate`)"""
    sr = KWS[i % 3].get("samprate", 44100) if rate is None else rate
    x = synth.stream_pcm(seed + i, 24, sr=sr, bursts=True)[T0 * 1152:]
    x = np.ascontiguousarray(x[:, 0] if mono else x)
    x.setflags(write=False)
    return x


def cut(seed, F, rate=None, mono=False, n=S):
    return np.stack([sig(seed, i, rate, mono)[:F * 1152] for i in range(n)])


def oracle_of(kw, pcm):
    enc = O.OracleEncoder(O.default_control(**kw))
    return b"".join(enc.encode_s16(pcm[f * 1152:(f + 1) * 1152]) for f in range(len(pcm) // 1152))


@functools.lru_cache(maxsize=None)
def expected(i, n1, n2, fresh):
    """stream i over n1 frames of the first signal and n2 of the second: (bytes of the first call, of the second) - the second
    as a new stream (fresh) or as the continuation"""
    a, b = sig(1500, i)[:n1 * 1152], sig(1600, i)[:n2 * 1152]
    first = oracle_of(KWS[i % 3], a)
    if fresh:
        return first, oracle_of(KWS[i % 3], b)
    both = oracle_of(KWS[i % 3], np.concatenate([a, b]))
    assert both[:len(first)] == first
    return first, both[len(first):]


def controls():
    return [api().default_control(**KWS[i % 3]) for i in range(S)]


def all_blobs(b):
    return [b.get_stream_state(i) for i in range(b.n)]


@pytest.mark.parametrize("F1,F2", [(6, 5), (7, 2)], ids=["6_then_5", "7_then_2_stale_subband_slots"])
def test_reset_of_many_slots(F1, F2, k6_build):
    """the reset slots equal a new batch's bit for bit, the others are not touched, and the next call encodes the new
    inputs from scratch - also when it is shorter than the one before, so that subband slots written by the earlier call
    lie beyond its extent (only slots 0..2 are zeroed)"""
    b = api().Batch(controls(), nstreams=S, max_frames=7)
    fresh = api().Batch(controls(), nstreams=S, max_frames=7)
    out1 = b.encode_host(cut(1500, F1))
    before = all_blobs(b)
    b.reset_streams(RESET)
    after, new = all_blobs(b), all_blobs(fresh)
    for i in range(S):
        assert after[i] == (new[i] if i in RESET else before[i]), i
        assert (before[i] != new[i]), i         # (the first call left something to reset)
    out2 = b.encode_host(cut(1600, F2))
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
    d_pcm = [torch.from_numpy(cut(1500, F1)).to(dev), torch.from_numpy(cut(1600, F2)).to(dev)]
    b = api().Batch(controls(), nstreams=S, max_frames=7)
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


@pytest.mark.one_k6_build
@pytest.mark.parametrize("idx", [[4, 0, 3], [2], list(range(S))], ids=["three", "one", "all"])
def test_gather_equals_the_single_slot_call(idx):
    b = api().Batch(controls(), nstreams=S, max_frames=7)
    b.encode_host(cut(1500, 5))
    got = b.get_stream_states(idx)
    assert len(got) == len(idx)
    for e, i in enumerate(idx):
        assert got[e] == b.get_stream_state(i), (e, i)
    assert b.status() == 0
    b.close()


KW4 = dict(vbr_mnr=55)
PLACE = [5, 0, 3, 2]        # stream i of the source batch goes to slot PLACE[i]


@functools.lru_cache(maxsize=None)
def moved_expected(i, F1, F2):
    x = sig(1700, i, 44100)[:(F1 + F2) * 1152]
    first = oracle_of(KW4, x[:F1 * 1152])
    both = oracle_of(KW4, x)
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
    b1 = api().Batch(api().default_control(**KW4), nstreams=4, max_frames=5)
    out1 = b1.encode_host(cut(1700, F1, 44100, n=4))
    saved = b1.get_stream_states(range(4))
    b1.close()
    b2 = api().Batch(api().default_control(**KW4), nstreams=6, max_frames=7)
    before = all_blobs(b2)
    b2.set_stream_states(PLACE, saved)
    after = all_blobs(b2)
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
def test_device_blobs_move_streams_without_a_host_wait():
    """gather into a device buffer, scatter into another batch and that batch's next call, all on one stream: the bytes
    continue, nothing beyond n * blob_stride is written, a blob's tail up to the stride is zero, and the blobs are the
    host call's"""
    import torch
    F1, F2 = 5, 6
    idx, place = [2, 0, 3], [4, 1, 0]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    b1 = api().Batch(api().default_control(**KW4), nstreams=4, max_frames=5)
    out1 = b1.encode_host(cut(1700, F1, 44100, n=4))
    b2 = api().Batch(api().default_control(**KW4), nstreams=6, max_frames=7)
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


def ints(v):
    return (C.c_int * max(len(v), 1))(*v), len(v)


@pytest.mark.one_k6_build
def test_refusals_leave_the_batch_unchanged():
    import torch
    A = api()
    L = A.lib()
    b = A.Batch(controls(), nstreams=S, max_frames=7)
    b.encode_host(cut(1500, 5))
    before = all_blobs(b)
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
    assert all_blobs(b) == before
    assert b.status() == 0

    # a host blob with a flipped fingerprint: none of the listed slots is written
    saved = b.get_stream_states([0, 1, 2])
    bad = bytearray(saved[1]); bad[16] ^= 1
    b2 = A.Batch(controls(), nstreams=S, max_frames=7)
    new = all_blobs(b2)
    with pytest.raises(RuntimeError, match="entry 1: the stream state was saved under a different configuration"):
        b2.set_stream_states([3, 4, 5], [saved[0], bytes(bad), saved[2]])
    assert all_blobs(b2) == new and b2.status() == 0
    # the device variant cannot refuse: the kernel leaves that slot alone, restores the others and says so in the status
    up = np.zeros(3 * stride, dtype=np.uint8)
    for e, blob in enumerate([saved[0], bytes(bad), saved[2]]):
        up[e * stride:e * stride + need] = np.frombuffer(blob, dtype=np.uint8)
    d_up = torch.from_numpy(up).to("cuda:0")
    torch.cuda.synchronize()
    b2.set_stream_states_device([3, 4, 5], d_up.data_ptr(), stride, None)
    assert b2.status() == 32
    got = all_blobs(b2)
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
    first, second = cut(1800, F, sr, mono, n), cut(1900, F, sr, mono, n)
    b = api().Batch(api().default_control(**kw), nstreams=n, max_frames=F)
    b2 = api().Batch(api().default_control(**kw), nstreams=n, max_frames=F + 1)
    out1 = b.encode_host(first)
    b.reset_streams([1])
    b2.set_stream_states([0], b.get_stream_states([2]))
    out2 = b.encode_host(second)
    moved = b2.encode_host(np.stack([second[2], second[0], second[1]]))
    assert b.status() == 0 and b2.status() == 0
    for i in range(n):
        assert out1[i] == oracle_of(kw, first[i]), i
    assert out2[1] == oracle_of(kw, second[1])
    for i in (0, 2):
        assert out1[i] + out2[i] == oracle_of(kw, np.concatenate([first[i], second[i]])), i
    assert moved[0] == out2[2]
    assert moved[1] == oracle_of(kw, second[0])
    b.close(); b2.close()


@pytest.mark.one_k6_build
def test_converting_batch():
    """48 kHz s16 -> 44.1 kHz (a case-4 plan, with carried samples): reset_streams restarts the converter too, the host
    calls move a stream with its converter to another converting batch, and device blobs are refused"""
    import torch
    from test_gpu_src_batch import Stream, make_batch, run
    A = api()
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
    before = all_blobs(b1)
    assert L.hx_batch_get_stream_states_device(b1.h, arr, k, d.data_ptr(), b1.states_stride(), None) == -1 and "converting" in A.last_error()
    assert L.hx_batch_set_stream_states_device(b1.h, arr, k, d.data_ptr(), b1.states_stride(), None) == -1 and "converting" in A.last_error()
    assert all_blobs(b1) == before and b1.status() == 0
    b1.close(); b2.close()
