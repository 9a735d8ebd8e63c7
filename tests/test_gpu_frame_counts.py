"""Per-stream frame counts (hx_batch_frame_counts, hx_multi_frame_counts) on a real MI355X: each stream of a batched call
takes its own number of frames, 0 included.

The expectation is one oracle encoder per stream fed frame by frame (packet_cases.oracle_frames), which is any partition of
the stream's frames into calls.  Every comparison is equality.  Before a call the rows and the packet buffer are filled with
0xA5 and the sizes, byte counts and counters with -1, so what a call does not write stays recognisable.  In a call's input
the samples behind a stream's count are NaN (fp32) or full-scale garbage (int16): they must reach no output and no state."""
import os

import numpy as np
import pytest

import gpu_support as G
import packet_cases as PC
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import FILL, REF_CLI, CallBufs, Image, batch_vs_single_vs_reference, host_crc, oracle_bytes, sync, write_wav
from hmp3_amd import api, synth
from output_checks import check_crc, check_dense, check_idle_rows
from src_cases import Stream, make_batch

pytestmark = pytest.mark.gpu


def make_pcm(seed, kws, F):
    """float32 [S, F * 1152, 2] ([S, F * 1152] for mono controls) at int16 scale with non-integral samples, every stream at
    its own control's rate, every second one with bursts (block switching)"""
    rows = [synth.stream_pcm(seed + i, F, kw.get("samprate", 44100), rho=PC.RHOS[i % 4], bursts=i % 2 == 0) for i, kw in enumerate(kws)]
    pcm = np.stack(rows).astype(np.float32)
    pcm += np.random.default_rng(seed).uniform(-0.49, 0.49, pcm.shape).astype(np.float32)
    if kws[0].get("mode") == 3:
        pcm = np.ascontiguousarray(pcm[:, :, 0])
    return pcm


class Streams:
    """the oracle's frames of every stream and how far each stream has come"""

    def __init__(self, kws, pcm):
        self.kws, self.pcm, self.S = kws, pcm, len(kws)
        self.want = [PC.oracle_frames(kws[s], self.pcm[s]) for s in range(self.S)]
        self.pos = [0] * self.S
        self.lsf = kws[0].get("samprate", 44100) < 32000

    def left(self, s):
        return len(self.want[s]) - self.pos[s]

    def block(self, counts, nf, dtype=np.float32):
        """the call's input [S, nf * 1152(, 2)]: row s starts with the stream's next counts[s] frames, garbage behind them"""
        blk = np.empty((self.S, nf * 1152) + self.pcm.shape[2:], dtype=dtype)
        blk[...] = np.nan if dtype == np.float32 else -32768
        for s, n in enumerate(counts):
            blk[s, :n * 1152] = self.pcm[s, self.pos[s] * 1152:(self.pos[s] + n) * 1152]
        return blk

    def counters(self, s, upto):
        """the stream's (frames, bytes) emitted after `upto` of its frames"""
        return (self.want[s][upto - 1].frames_out, self.want[s][upto - 1].bytes_out) if upto > 0 else (0, 0)

    def check(self, counts, nf, bs, pk=None, pkb=None, stats=None, tag=""):
        """one call's outputs under `counts` (bs: the rows' used parts); advances the streams"""
        for s, n in enumerate(counts):
            p = self.pos[s]
            assert bs[s] == b"".join(w.bs for w in self.want[s][p:p + n]), "%s stream %d (count %d): bitstream" % (tag, s, n)
            for f in range(nf):
                at = "%s stream %d (count %d) frame %d" % (tag, s, n, f)
                if stats is not None:
                    assert tuple(stats[s, f]) == self.counters(s, p + min(f + 1, n)), at + ": frames / bytes emitted so far"
                if pk is None:
                    continue
                if f < n:
                    w = self.want[s][p + f]
                    n0, n1 = w.sizes
                    assert n0 > 0 and (n1 > 0) == bool(self.lsf), at
                    assert tuple(pkb[s, f]) == (n0, n1), at + ": packet sizes"
                    assert pk[s, f, :n0 + n1].tobytes() == w.packet, at + ": packet"
                    assert (pk[s, f, n0 + n1:] == FILL).all(), at + ": bytes written behind the packet"
                else:
                    assert tuple(pkb[s, f]) == (0, 0), at + ": packet sizes behind the count"
                    assert (pk[s, f] == FILL).all(), at + ": packet bytes written behind the count"
            self.pos[s] = p + n

    def check_totals(self, b):
        for s in range(self.S):
            assert b.frames_bytes(s) == self.counters(s, self.pos[s]), "stream %d: hx_batch_frames_bytes" % s


def outputs(b, nf, frame_stride=4096, dense=False):
    """every device output buffer of one call, prefilled: rows, packets and the dense image with 0xA5, byte counts, sizes,
    counters, CRCs and offsets with -1"""
    return CallBufs(b, nf, rows_fill=FILL, counters=True, crc=True, packets=frame_stride, image=Image(b.n, b.dense_bound(nf), guard=0) if dense else None)


def device_call(b, st, counts, nf):
    """one plain fp32 device-buffer call under `counts` (None: no counts, every stream takes nf frames), with packet and counter
    buffers of its own"""
    b.frame_counts(counts)
    o = G.device_call(b, st.block(counts if counts is not None else [nf] * st.S, nf, np.float32), nf, outputs(b, nf).set_on(b, crc=False))
    sync()
    assert b.status() == 0
    return o


# call after call of this table, every row a call, every column a stream (then from the top again), each count cut to what
# the stream has left: stream 0 takes nothing in the very first call, stream 1 nothing twice running; 3 and 4 frames are 6 and
# 8 granules, either side of k_polyphase's 7-granule tile; 5 frames are 10 granules - k_msscan's eight-granule rounds stop
# off a multiple of 8; 8 is the full call, 1 the shortest, 7 cuts the second tile
TABLE = [
    [0, 8, 3, 4, 5, 7, 1, 8],
    [5, 0, 4, 3, 8, 1, 7, 0],
    [8, 0, 5, 7, 0, 4, 3, 1],
    [3, 7, 0, 8, 4, 5, 0, 8],
    [1, 4, 8, 0, 7, 3, 5, 4],
    [7, 5, 1, 5, 3, 0, 8, 3],
]
MIXED = [dict(samprate=32000, bitrate=48), dict(samprate=44100), dict(samprate=48000, vbr_mnr=70), dict(samprate=48000, bitrate=64),
         dict(samprate=32000, vbr_mnr=40), dict(samprate=44100, bitrate=96), dict(samprate=48000), dict(samprate=32000)]
UNEVEN = {
    "vbr_block_switching": dict(),
    "cbr128_joint": dict(bitrate=64),
    "mono_cbr64": dict(bitrate=64, mode=3),
    "dc_filter_fp32": dict(bitrate=64, filter_select=1),
    "mixed_rates": MIXED,
}


@pytest.mark.parametrize("case", list(UNEVEN))
def test_uneven_calls_equal_each_streams_own_oracle(case):
    """8 streams, calls of 8 frames, 40 frames per stream in uneven pieces (TABLE) on both builds of the stream walk: rows,
    byte counts, counters, packets and sizes of every call, and the streams' totals at the end"""
    S, nf, F = 8, 8, 40
    kws = UNEVEN[case] if isinstance(UNEVEN[case], list) else [UNEVEN[case]] * S
    st = Streams(kws, make_pcm(8100, kws, F))
    a = api
    b = a.Batch([a.default_control(**kw) for kw in kws], max_frames=nf)
    c = 0
    while any(st.left(s) for s in range(S)):
        counts = [min(TABLE[c % len(TABLE)][s], st.left(s)) for s in range(S)]
        o = device_call(b, st, counts, nf)
        st.check(counts, nf, o.bitstreams(), *o.packets(), tag="call %d" % c)
        check_idle_rows(o, counts)
        c += 1
        assert c < 40
    assert all(p == F for p in st.pos)
    st.check_totals(b)
    b.close()


def test_a_stream_that_takes_no_frames_keeps_its_state():
    """three uniform frames, then a call of 2 frames with counts [0, 2, 0, 2]: the checkpoints of streams 0 and 2 are the same
    bytes before and after it, their prefilled rows are untouched, and uniform calls afterwards match the oracle for all four
    (4 streams x 2 frames: packed by the one-workgroup form of k_pack)"""
    S, kw = 4, dict()
    st = Streams([kw] * S, make_pcm(8200, [kw] * S, 9))
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=3)
    o = device_call(b, st, [3] * S, 3)
    st.check([3] * S, 3, o.bitstreams(), *o.packets(), tag="uniform")
    before = [b.get_stream_state(s) for s in range(S)]
    counts = [0, 2, 0, 2]
    o = device_call(b, st, counts, 2)
    rows, nb = o.rows()
    after = [b.get_stream_state(s) for s in range(S)]
    for s in (0, 2):
        assert after[s] == before[s], "stream %d took no frame and its checkpoint changed" % s
        assert nb[s] == 0 and (rows[s] == FILL).all(), "stream %d took no frame and its row was written" % s
    for s in (1, 3):
        assert after[s] != before[s]
    st.check(counts, 2, o.bitstreams(), *o.packets(), tag="counts")
    for c, n in enumerate((2, 2)):
        o = device_call(b, st, None, n)
        st.check([n] * S, n, o.bitstreams(), *o.packets(), tag="uniform again %d" % c)
    st.check_totals(b)
    b.close()


LSF_A1 = [PC.MPEG2[0], PC.MPEG2[2], PC.A1[0], PC.A1[3]]


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kw", LSF_A1, ids=PC.case_id)
def test_mpeg2_and_first_generation_allocator_under_counts(kw):
    """k_alloc_lsf, k_alloc1 and k_alloc1_lsf: 4 streams, calls of 5 frames, counts from {0, 1, 2, 5}, 20 frames per stream,
    packets included (an MPEG-2 call yields two)"""
    if kw in PC.A1:
        skip_unless_host_libm_is_the_restated_one()
    S, nf, F = 4, 5, 20
    table = [[0, 5, 2, 1], [2, 0, 5, 5], [5, 0, 1, 2], [1, 2, 0, 5], [5, 1, 5, 0]]
    st = Streams([kw] * S, make_pcm(8300, [kw] * S, F))
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=nf)
    c = 0
    while any(st.left(s) for s in range(S)):
        counts = [min(table[c % len(table)][s], st.left(s)) for s in range(S)]
        o = device_call(b, st, counts, nf)
        st.check(counts, nf, o.bitstreams(), *o.packets(), tag="call %d" % c)
        c += 1
        assert c < 30
    st.check_totals(b)
    b.close()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_submits_take_the_counts_in_force_at_the_submit(host):
    """six submits of 4 frames, the setter called with other counts before each and with nonsense behind the last one, output
    buffers of its own for every submit, counters, CRC and dense image on, one wait at the end: every submit's outputs are
    the oracle's for the counts in force when it was made (a device-buffer submit is packed later, behind the next one)"""
    import torch
    S, nf, kw = 6, 4, dict(bitrate=64)
    table = [[4, 0, 1, 3, 2, 4], [0, 0, 4, 1, 3, 2], [2, 4, 0, 4, 0, 1], [4, 1, 2, 0, 4, 3], [1, 3, 4, 2, 0, 0], [3, 2, 0, 4, 1, 4]]
    st = Streams([kw] * S, make_pcm(8400, [kw] * S, 24))
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=nf)
    outs = [outputs(b, nf, dense=True) for _ in table]
    pos, blks = [0] * S, []
    for counts in table:        # (the inputs up front: Streams.block cuts at the streams' positions)
        st.pos = list(pos)
        blks.append(st.block(counts, nf))
        pos = [p + n for p, n in zip(pos, counts)]
    st.pos = [0] * S
    if host:
        ins = [torch.from_numpy(x).pin_memory() for x in blks]
        h_out = [torch.full((S, o.stride), FILL, dtype=torch.uint8).pin_memory() for o in outs]
        h_nb = [torch.full((S,), -1, dtype=torch.int32).pin_memory() for _ in outs]
    else:
        ins = [torch.from_numpy(x).to(dev) for x in blks]
    torch.cuda.synchronize()
    for c, counts in enumerate(table):
        outs[c].set_on(b, crc=True)
        b.frame_counts(counts)
        if host:
            b.submit_host(ins[c].data_ptr(), nf, h_out[c].data_ptr(), outs[c].stride, h_nb[c].data_ptr(), f32=True)
        else:
            b.submit_device(ins[c].data_ptr(), nf, outs[c].ptr, outs[c].stride, outs[c].nb.data_ptr(), q, f32=True)
    b.frame_counts([nf] * S)     # reaches no submit already made
    if host:
        b.wait_host()
    else:
        b.wait(q)
    torch.cuda.synchronize()
    assert b.status() == 0
    for c, counts in enumerate(table):
        o = outs[c]
        if host:
            rows, n = h_out[c].numpy(), h_nb[c].numpy()
            bs = [rows[s, :n[s]].tobytes() for s in range(S)]
            for s in range(S):          # (the staging row of such a stream holds an earlier submit's bytes: it is not copied back)
                assert counts[s] > 0 or (n[s] == 0 and (rows[s] == FILL).all()), "submit %d stream %d took no frame and its host row was written" % (c, s)
            o.out.copy_(h_out[c])       # (the checks of CRC and dense image read the rows from the device buffers)
            o.nb.copy_(h_nb[c])
        else:
            bs = o.bitstreams()
            check_idle_rows(o, counts)
        st.check(counts, nf, bs, *o.packets(), tag="submit %d" % c)
        check_crc(o)
        check_dense(o)
    b.frame_counts(None)
    st.check_totals(b)
    b.close()


def test_host_calls_under_counts():
    """encode_host(stats, crc) and encode_host_dense under counts: the CRC of every frame, those behind a stream's count
    included, is hx_xing_update_crc over the row's first e[f] bytes; a stream that takes nothing has an empty dense segment"""
    S, nf, kw = 5, 6, dict(vbr_mnr=60)
    st = Streams([kw] * S, make_pcm(8500, [kw] * S, 18))
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=nf)
    for c, counts in enumerate([[6, 0, 3, 1, 5], [2, 0, 6, 0, 4]]):
        b.frame_counts(counts)
        bs, stats, crc = b.encode_host(st.block(counts, nf), stats=True, crc=True)
        assert b.status() == 0
        for s in range(S):
            for f in range(nf):
                e = len(bs[s]) - (int(stats[s, -1, 1]) - int(stats[s, f, 1]))
                assert 0 <= e <= len(bs[s]) and (f < counts[s] or e == len(bs[s]))
                assert crc[s, f] == host_crc(bs[s][:e]), "call %d stream %d frame %d: CRC" % (c, s, f)
        st.check(counts, nf, bs, stats=stats, tag="host call %d" % c)
    counts = [0, 3, 0, 0, 2]        # the caller's own rows: those of streams that take nothing are left out of the copy back
    b.frame_counts(counts)          # (every staging row holds bytes of the calls above)
    stride = b.out_stride(nf)
    rows, nb = np.full((S, stride), FILL, dtype=np.uint8), np.full(S, -1, dtype=np.int32)
    blk = st.block(counts, nf)
    assert a.lib().hx_batch_encode_f32_host(b.h, blk.ctypes.data, nf, rows.ctypes.data, stride, nb.ctypes.data) == 0 and b.status() == 0
    for s in range(S):
        assert counts[s] > 0 or (nb[s] == 0 and (rows[s] == FILL).all()), "stream %d took no frame and its host row was written" % s
    st.check(counts, nf, [rows[s, :nb[s]].tobytes() for s in range(S)], tag="host call into prefilled rows")
    counts = [0, 6, 1, 4, 0]
    b.frame_counts(counts)
    segs, off = b.encode_host_dense(st.block(counts, nf))
    assert b.status() == 0
    assert off[1] == off[0] == 0 and off[5] == off[4] and segs[0] == b"" and segs[4] == b""
    st.check(counts, nf, segs, tag="host dense call")
    b.frame_counts(None)
    bs = b.encode_host(st.block([2] * S, 2))
    st.check([2] * S, 2, bs, tag="uniform host call")
    st.check_totals(b)
    b.close()


def uneven_host_calls(b, pcm, counts_of_call, nf):
    """int16 host calls under counts_of_call(c, durations of the previous call) -> (each stream's bytes, its frames)"""
    S = len(pcm)
    got, pos = [b"" for _ in range(S)], np.zeros(S, dtype=np.int64)
    for c in range(3):
        counts = counts_of_call(c)
        blk = np.full((S, nf * 1152, 2), -32768, dtype=np.int16)
        for s in range(S):
            blk[s, :counts[s] * 1152] = pcm[s, pos[s] * 1152:(pos[s] + counts[s]) * 1152]
        b.frame_counts(counts)
        out = b.encode_host(blk)
        assert b.status() == 0
        for s in range(S):
            assert (counts[s] == 0) <= (out[s] == b"")
            got[s] += out[s]
        pos += np.asarray(counts)
    return got, pos


@pytest.mark.one_k6_build
def test_persistent_workgroups_under_counts(monkeypatch):
    """k_alloc_slim's persistent workgroups claim stream after stream of the launch order, streams that take nothing
    included: 1600 streams on 1536 slots, calls of 3 frames, counts (s + call) % 4, three calls, every stream against the
    oracle - the claim counter is back at zero after every launch, or streams would be missing from the next"""
    monkeypatch.setenv("HMP3AMD_K6", "slim")
    kw, S, nf = dict(), 1600, 3
    base = [synth.stream_pcm(8600 + u, 6, rho=PC.RHOS[u % 4], bursts=True) for u in range(50)]
    pcm = np.stack([np.roll(base[i % 50], 1152 * (i // 50), axis=0) for i in range(S)])
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=nf)
    assert b.k6_variant() == 1 and b.resident_streams() < S
    got, pos = uneven_host_calls(b, pcm, lambda c: [(s + c) % 4 for s in range(S)], nf)
    b.close()
    from oracle_pool import oracle_bytes_many
    want = {}
    for n in sorted(set(pos.tolist())):
        want.update(oracle_bytes_many(kw, pcm, n, ids=[s for s in range(S) if pos[s] == n]))
    bad = [s for s in range(S) if got[s] != want[s]]
    assert not bad, "%d of %d streams differ from the oracle, first: %s" % (len(bad), S, bad[:8])


@pytest.mark.one_k6_build
def test_parked_workgroups_wake_when_a_straggler_takes_no_frames(monkeypatch):
    """The 256-register build under a launch order (HMP3AMD_LPT=3): the first positions of the order - the previous call's
    slowest streams - publish their CU, and workgroups that run out of work there sleep until that position retires.  300
    streams, three calls; in each a different eighth of the streams takes nothing, the previous call's slowest among them:
    they retire all the same, the call ends, and every stream matches the oracle"""
    monkeypatch.setenv("HMP3AMD_K6", "fat")
    monkeypatch.setenv("HMP3AMD_LPT", "3")
    kw, S, nf = dict(), 300, 3
    base = [synth.stream_pcm(8700 + u, 9, rho=PC.RHOS[u % 4], bursts=True) for u in range(30)]
    pcm = np.stack([np.roll(base[i % 30], 1152 * (i // 30), axis=0) for i in range(S)])
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=nf)
    assert b.k6_variant() == 0 and b.resident_streams() >= S
    idle = []

    def counts_of_call(c):
        counts = [0 if s % 8 == c else nf for s in range(S)]
        if c > 0:
            dur = b.debug_read("dur", np.uint32, S)
            for s in np.argsort(dur)[::-1][:16]:     # (the first eight positions of the order park their CU)
                counts[int(s)] = 0
        idle.append(sum(n == 0 for n in counts))
        return counts

    got, pos = uneven_host_calls(b, pcm, counts_of_call, nf)
    b.close()
    assert min(idle) >= S // 8 and len(set(pos.tolist())) > 1
    for s in range(S):
        assert got[s] == oracle_bytes(kw, pcm[s], int(pos[s])), s


def test_refusals_leave_the_batch_usable():
    """a count of -1 or nframes + 1 makes the call return -1 and name the stream, nothing is written into prefilled outputs,
    the next valid call matches the oracle; NULL restores uniform calls; a converting batch refuses the setter"""
    import torch
    S, nf, kw = 3, 2, dict(bitrate=64)
    st = Streams([kw] * S, make_pcm(8800, [kw] * S, 6))
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=nf)
    o = outputs(b, nf)
    o.set_on(b, crc=False)
    d_pcm = torch.from_numpy(st.block([nf] * S, nf)).to(torch.device("cuda:0"))
    q = torch.cuda.current_stream().cuda_stream
    for bad, who in (([2, -1, 2], "stream 1"), ([2, 2, nf + 1], "stream 2")):
        b.frame_counts(bad)
        for call in (b.encode_device, b.submit_device):
            with pytest.raises(RuntimeError, match=who):
                call(d_pcm.data_ptr(), nf, o.ptr, o.stride, o.nb.data_ptr(), q, f32=True)
        with pytest.raises(RuntimeError, match=who):
            b.encode_host(st.block([nf] * S, nf))
        torch.cuda.synchronize()
        rows, nb = o.rows()
        pk, pkb, stats = o.packets()
        assert (rows == FILL).all() and (nb == -1).all() and (pk == FILL).all() and (pkb == -1).all() and (stats == -1).all()
    with pytest.raises(ValueError):
        b.frame_counts([1, 1])
    counts = [1, 0, 2]
    o = device_call(b, st, counts, nf)
    st.check(counts, nf, o.bitstreams(), *o.packets(), tag="valid call")
    o = device_call(b, st, None, nf)
    st.check([nf] * S, nf, o.bitstreams(), *o.packets(), tag="uniform call")
    bs = b.encode_host(st.block([1] * S, 1))
    st.check([1] * S, 1, bs, tag="uniform host call")
    b.close()
    cb = make_batch([Stream(48000, 24, 0, mpeg_select=44100, seed=71), Stream(32000, 32, 1, mpeg_select=44100, seed=72)], 4)
    with pytest.raises(RuntimeError, match="converting batch"):
        cb.frame_counts([1, 1])
    cb.close()


def multi_call(m, blk, nf, rows=None, nb=None, stats=None):
    """hx_multi_encode_f32_host_stats into the caller's own (prefilled) arrays -> its return value"""
    return int(api.lib().hx_multi_encode_f32_host_stats(m.h, blk.ctypes.data, nf, rows.ctypes.data, rows.shape[1], nb.ctypes.data, stats.ctypes.data))


def multi_states(m):
    """the checkpoint of every stream, through the blocks' batches"""
    L = api.lib()
    blobs = []
    for k in range(m.ndevices()):
        h, (_, first, count) = L.hx_multi_batch(m.h, k), m.shard(k)
        for i in range(count):
            buf = (api.C.c_ubyte * int(L.hx_batch_stream_state_bytes(h)))()
            assert L.hx_batch_get_stream_state(h, i, buf) == 0
            blobs.append(bytes(buf))
    return blobs


def test_multi_frame_counts_over_two_blocks():
    """hx_multi_frame_counts: 5 streams in two blocks (3 + 2) on device 0, the counts fanned out to the blocks' batches"""
    a = api
    kws = [dict(bitrate=64), dict(vbr_mnr=60), dict(bitrate=96, short_block_threshold=99999), dict(bitrate=64), dict(vbr_mnr=60)]
    S, nf = 5, 4
    st = Streams(kws, make_pcm(8900, kws, 10))
    m = a.Multi([a.default_control(**kw) for kw in kws], max_frames=nf, devices=[0, 0])
    assert [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    for c, counts in enumerate([[4, 0, 2, 1, 3], [0, 4, 1, 3, 0], [3, 2, 4, 0, 4]]):
        m.frame_counts(counts)
        bs, stats = m.encode_host(st.block(counts, nf), stats=True)
        assert m.status() == 0
        st.check(counts, nf, bs, stats=stats, tag="multi call %d" % c)
    m.frame_counts(None)
    bs = m.encode_host(st.block([2] * S, 2))
    st.check([2] * S, 2, bs, tag="uniform multi call")
    m.close()


@pytest.mark.parametrize("bad", [(4, 5), (1, -1), (3, 5)], ids=["last_block", "first_block", "second_block_first_stream"])
def test_multi_call_refused_for_one_block_moves_no_stream_of_the_other(bad):
    """One count beyond nframes (or below 0) while the other block's streams have counts that a call would act on: the call is
    refused for all five streams before a block starts - the message names the stream by its number over all blocks, every
    checkpoint is the same bytes as before, the prefilled rows, byte counts and counters are untouched, and the next valid call
    continues every stream where the oracle stands"""
    a = api
    kws = [dict(bitrate=64), dict(vbr_mnr=60), dict(bitrate=96, short_block_threshold=99999), dict(bitrate=64), dict(vbr_mnr=60)]
    S, nf = 5, 4
    st = Streams(kws, make_pcm(8950, kws, 9))
    m = a.Multi([a.default_control(**kw) for kw in kws], max_frames=nf, devices=[0, 0])
    counts = [3, 1, 4, 2, 0]
    m.frame_counts(counts)
    bs, stats = m.encode_host(st.block(counts, nf), stats=True)
    st.check(counts, nf, bs, stats=stats, tag="first call")
    before = multi_states(m)
    stride = int(a.lib().hx_multi_out_stride(m.h, nf))
    rows, nb, stats = np.full((S, stride), FILL, dtype=np.uint8), np.full(S, -1, dtype=np.int32), np.full((S, nf, 2), -1, dtype=np.int32)
    counts = [2, 4, 1, 3, 2]
    counts[bad[0]] = bad[1]
    m.frame_counts(counts)
    assert multi_call(m, st.block([nf] * S, nf), nf, rows, nb, stats) == -1
    assert a.last_error().startswith("stream %d: frame count %d " % bad), a.last_error()
    assert multi_states(m) == before, "a refused call moved a stream"
    assert (rows == FILL).all() and (nb == -1).all() and (stats == -1).all(), "a refused call wrote an output"
    counts = [2, 4, 1, 3, 2]
    m.frame_counts(counts)
    assert multi_call(m, st.block(counts, nf), nf, rows, nb, stats) == 0 and m.status() == 0
    st.check(counts, nf, [rows[s, :nb[s]].tobytes() for s in range(S)], stats=stats, tag="valid call after the refusal")
    m.close()


def cli_files(tmp_path):
    """three 44.1 kHz int16 WAVs of 5, 40 and 130 frames for one `hmp3amd -batch` run: the first two files end inside the first
    call of 96 frames, and every call gives a file only the frames it still needs -> [(label, wav, mp3)]"""
    files = []
    for i, frames in enumerate((5, 40, 130)):
        wav, mp3 = str(tmp_path / ("in%d.wav" % i)), str(tmp_path / ("batch%d.mp3" % i))
        write_wav(wav, synth.stream_pcm(9300 + i, frames, bursts=True)[:frames * 1152 - 211 * i], 44100, False)
        files.append((wav, wav, mp3))
    return files


@pytest.mark.one_k6_build
def test_cli_batch_of_files_of_different_lengths_equals_the_single_file_runs(tmp_path):
    """files, tags, TOC and MusicCRC byte for byte what `hmp3amd in.wav out.mp3` writes for each file alone"""
    batch_vs_single_vs_reference(cli_files(tmp_path), floor=1000, reference=False)


@pytest.mark.one_k6_build
@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="oracle/_ref/hmp3 (the reference's CLI, prebuilt) not present")
def test_cli_batch_of_files_of_different_lengths_equals_the_reference_binary(tmp_path):
    """... and what the reference's own command line writes for each file"""
    batch_vs_single_vs_reference(cli_files(tmp_path), single=False)


RANDOM_CASES = list(range(10))


@pytest.mark.parametrize("case", RANDOM_CASES)
def test_fixed_seed_random_slice(case):
    """random batch size, call length, counts and control (packet_cases.MPEG1), four calls each, against the oracle"""
    rng = np.random.default_rng(9000 + case)
    S, nf = int(rng.integers(2, 7)), int(rng.integers(1, 13))
    kw = PC.MPEG1[int(rng.integers(len(PC.MPEG1)))]
    calls = [[int(rng.integers(0, nf + 1)) for _ in range(S)] for _ in range(4)]
    F = max(sum(c[s] for c in calls) for s in range(S))
    st = Streams([kw] * S, make_pcm(9100 + case, [kw] * S, max(F, 1)))
    a = api
    b = a.Batch(a.default_control(**kw), nstreams=S, max_frames=nf)
    for c, counts in enumerate(calls):
        o = device_call(b, st, counts, nf)
        st.check(counts, nf, o.bitstreams(), *o.packets(), tag="case %d (%s, S %d, nframes %d) call %d" % (case, PC.case_id(kw), S, nf, c))
        check_idle_rows(o, counts)
    st.check_totals(b)
    b.close()
