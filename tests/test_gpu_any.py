"""One batch for every stream kind (hx_batch_create_any, hx_multi_create_any): MPEG-1 and MPEG-2 rates and both allocator
generations in one batch and one menu.

A stream's kind is 2 * (first-generation allocator) + (MPEG-2 rate); every kind has its own stream-walk kernel, launched over
its span of one launch order.  The slots here are assigned interleaved (kinds 0, 1, 2, 3, 0, 1, ...), so no kind is
contiguous in stream order, the four waves of a k_detect workgroup differ in MPEG version and every span but the first
starts at a position > 0.  Every expectation is byte identity against the oracle, one encoder per stream life fed frame by
frame, as in test_gpu_mixed.py (both on tests/mixed_cases.py); converting streams go through this library's host converter
and then the oracle.  Blob comparisons across batches use device calls into zeroed rows, as explained there."""
import ctypes as C

import numpy as np
import pytest

import packet_cases as PC
from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import FILL, CallBufs, Image, controls, plain_call as device_call, run_cli, write_wav
from hmp3_amd import api, synth
from mixed_cases import RHOS, blob_diff, joined, key, rows_of, streams_of, want_f32
from oracle_pool import oracle_bytes_many
from output_checks import check_image, expected_crc
from src_cases import Stream, host_converted

pytestmark = pytest.mark.gpu

# kind 0: stereo 44.1 kHz CBR, mono 48 kHz VBR (test_gpu_mixed.ENTRIES); kind 1: stereo 22.05 kHz CBR-32, mono 16 kHz CBR-32
# behind the DC blocker, 24 kHz VBR (test_gpu_slot_menu's mpeg2 menu, packet_cases.MPEG2); kind 2: dual channel at 44.1 kHz and
# intensity stereo (packet_cases.A1); kind 3: dual channel at 16 kHz (the golden a1_dual_16k_antiphase).  In slot order the
# kinds run 0 1 2 3 0 1 2 1.
ENTRIES = [dict(bitrate=64), dict(bitrate=32, samprate=22050), dict(bitrate=64, mode=2), dict(samprate=16000, mode=2, bitrate=8),
           dict(mode=3, samprate=48000), dict(bitrate=32, mode=3, samprate=16000, filter_select=1), dict(bitrate=64, nsbstereo=8),
           dict(samprate=24000)]
KINDS = [0, 1, 2, 3, 0, 1, 2, 1]
S = len(ENTRIES)
FPB = [2 if k & 1 else 1 for k in KINDS]
CHANNELS = [1 if kw.get("mode") == 3 else 2 for kw in ENTRIES]
SWITCHING = [s for s in range(S) if KINDS[s] < 2]        # (the first-generation allocator codes long blocks only)


def any_batch(menu=ENTRIES, cfg=None, n=None, max_frames=4):
    n = len(menu) if n is None else n
    return api.Batch.any(controls(menu), n, cfg=list(range(n)) if cfg is None else cfg, max_frames=max_frames)


def eight(f32, seed=1700):
    """the eight streams of ENTRIES: (signals, the oracle's bytes per frame)"""
    return streams_of(ENTRIES, f32, seed)


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_plain_parity_over_two_calls(f32, k6_build):
    skip_unless_host_libm_is_the_restated_one()
    pcm, want = eight(f32)
    b = any_batch()
    assert b.pcm_channels() == 2 and [b.stream_channels(i) for i in range(S)] == CHANNELS
    assert [b.stream_frames_per_block(i) for i in range(S)] == FPB
    got, short = [], np.zeros(S, bool)
    for c in range(2):
        got.append(b.encode_host(rows_of(pcm, [4 * c] * S, [4] * S, 4, f32)))
        bt = b.debug_read("bt", np.uint8, S * 8).reshape(S, 8)
        print("call %d block types: %s" % (c, bt.tolist()))
        short |= (bt == 2).any(axis=1)
    assert b.status() == 0
    assert all(short[s] for s in SWITCHING), "the streams' onsets no longer give short blocks: %s" % short.tolist()
    for s in range(S):
        assert got[0][s] == joined(want[s], 0, 4), "stream %d, first call" % s
        assert got[1][s] == joined(want[s], 4, 4), "stream %d, second call" % s
    assert [b.frames_bytes(s)[1] for s in range(S)] == [len(joined(want[s], 0, 8)) for s in range(S)]
    b.close()


def test_device_pcm_pointer_two_bytes_off_a_16_byte_boundary(k6_build):
    skip_unless_host_libm_is_the_restated_one()
    pcm, want = eight(False)
    b = any_batch()
    got, ptr = device_call(b, rows_of(pcm, [0] * S, [4] * S, 4, False), 4, shift=1)
    assert ptr % 16 == 2
    assert b.status() == 0
    for s in range(S):
        assert got[s] == joined(want[s], 0, 4), "stream %d" % s
    b.close()


def test_the_one_workgroup_packing_of_a_tiny_call(k6_build):
    """two slots of kinds 0 and 1, calls of two frames: 2 streams x 4 frame positions = 8, which k_pack takes as ONE workgroup
    (its `solo` path: the pending frames' images in and out by the same workgroup) - the MPEG-1 stream's positions 2 and 3
    leave, the MPEG-2 stream's four are frames.  Three calls, so that carried images cross two of them."""
    menu = [ENTRIES[0], ENTRIES[1]]
    w = [want_f32(1760 + i, key(kw)) for i, kw in enumerate(menu)]
    b = any_batch(menu, max_frames=2)
    assert [b.stream_frames_per_block(i) for i in range(2)] == [1, 2]
    for c in range(3):
        got = device_call(b, rows_of([x for x, _ in w], [2 * c] * 2, [2] * 2, 2, True), 2)[0]
        assert b.status() == 0
        for s in range(2):
            assert got[s] == b"".join(f.bs for f in w[s][1][2 * c:2 * c + 2]), "call %d stream %d" % (c, s)
    assert [b.frames_bytes(s)[1] for s in range(2)] == [sum(len(f.bs) for f in w[s][1][:6]) for s in range(2)]
    b.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_a_menu_of_one_kind_is_the_mixed_batch(kind, k6_build):
    """Batch.any over entries of one kind: kernel choice, resident set, out_stride, rows, out_bytes and checkpoint blobs are
    Batch.mixed's on the same input, byte for byte"""
    menu = [kw for kw, k in zip(ENTRIES, KINDS) if k == kind]
    x = [want_f32(1740 + i, key(kw))[0] for i, kw in enumerate(menu)]
    res = []
    for make in (api.Batch.any, api.Batch.mixed):
        b = make(controls(menu), len(menu), cfg=list(range(len(menu))), max_frames=4)
        assert [b.stream_frames_per_block(i) for i in range(b.n)] == [1 + kind] * b.n
        outs = []
        for c in range(2):
            blk = rows_of(x, [4 * c] * b.n, [4] * b.n, 4, True)
            outs.append(device_call(b, blk, 4)[0])
        assert b.status() == 0
        res.append((outs, b.get_stream_states(range(b.n)), b.k6_variant(), b.resident_streams(), b.out_stride(4)))
        b.close()
    for i in range(len(menu)):
        assert blob_diff(res[0][1][i], res[1][1][i]) == "", "stream %d: checkpoint blob" % i
    assert res[0] == res[1]
    for i, kw in enumerate(menu):
        frames = want_f32(1740 + i, key(kw))[1]
        assert res[0][0][0][i] + res[0][0][1][i] == b"".join(f.bs for f in frames[:8]), i


def test_per_stream_counts(k6_build):
    """a full call; counts 0, 1, 3 and 4 spread over all kinds; a call that every stream of kind 1 sits out (its launch still
    goes out: stream_idle does the bookkeeping); a last full call.  A stream that takes no frame keeps its blob bit for bit
    and has out_bytes 0, and the counters of the frames behind a stream's count repeat its last."""
    skip_unless_host_libm_is_the_restated_one()
    w = [want_f32(1700 + i, key(kw)) for i, kw in enumerate(ENTRIES)]
    pcm, frames = [x for x, _ in w], [f for _, f in w]
    b = any_batch()
    pos = [0] * S
    table = [[4] * S, [4, 0, 3, 1, 1, 3, 0, 4], [0, 4, 1, 0, 3, 1, 4, 3], [3, 0, 1, 4, 4, 0, 3, 0], [4] * S]
    assert all(table[3][s] == 0 for s in range(S) if KINDS[s] == 1) and all(table[3][s] > 0 for s in range(S) if KINDS[s] != 1)
    for c, counts in enumerate(table):
        idle = [i for i in range(S) if counts[i] == 0]
        before = b.get_stream_states(idle)
        b.frame_counts(counts)
        got, stats = b.encode_host(rows_of(pcm, pos, counts, 4, True), stats=True)
        assert b.status() == 0
        assert b.get_stream_states(idle) == before, "call %d: a stream that took no frame changed" % c
        for s in range(S):
            at = "call %d stream %d (count %d)" % (c, s, counts[s])
            assert got[s] == b"".join(f.bs for f in frames[s][pos[s]:pos[s] + counts[s]]), at
            for f in range(4):
                upto = pos[s] + min(f + 1, counts[s])
                want = (frames[s][upto - 1].frames_out, frames[s][upto - 1].bytes_out) if upto else (0, 0)
                assert tuple(stats[s, f]) == want, at + " frame %d: frames / bytes emitted so far" % f
            pos[s] += counts[s]
    b.close()


@pytest.mark.parametrize("mode", ["plain", "submits"])
def test_assign_across_kinds(mode, k6_build):
    """four slots of kinds 0, 1, 2, 0; slot 0 goes kind 0 -> 1 -> 3 -> 2 -> 0, two calls of two frames in every life (plain
    device calls, or two pipelined submits and one wait).  After the third assign no stream of kind 3 is left: that kind
    launches nothing.  In every life the slot's rows are a new stream's, and after the life's two calls its checkpoint blob is
    that of slot 0 of a new uniform batch fed the same frames (but for the class index).  Slots 1 - 3 run on undisturbed."""
    import torch
    skip_unless_host_libm_is_the_restated_one()
    menu = [ENTRIES[0], ENTRIES[1], ENTRIES[3], ENTRIES[2]]        # kinds 0, 1, 3, 2
    F = 2       # (slots 1 - 3 walk 20 frames of their 22-frame signals)
    lives = [[1800, 0, 0], [1801, 1, 0], [1802, 3, 0], [1803, 0, 0]]      # per slot: [seed, menu entry, frames done]
    b = api.Batch.any(controls(menu), 4, cfg=[e for _, e, _ in lives], max_frames=F)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def two_calls(tag):
        w = [want_f32(seed, key(menu[e]), 0.5) for seed, e, _ in lives]
        pos = [p for _, _, p in lives]
        blks = [rows_of([x for x, _ in w], [p + F * c for p in pos], [F] * 4, F, True) for c in range(2)]
        if mode == "plain":
            got = [device_call(b, blk, F)[0] for blk in blks]
        else:
            stride = b.out_stride(F)
            d_pcm = [torch.from_numpy(blk).to(dev) for blk in blks]
            d_out = [torch.zeros((4, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
            d_nb = [torch.full((4,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
            torch.cuda.synchronize()
            for c in range(2):
                b.submit_device(d_pcm[c].data_ptr(), F, d_out[c].data_ptr(), stride, d_nb[c].data_ptr(), st, f32=True)
            b.wait(st)
            torch.cuda.synchronize()
            got = [[d_out[c].cpu().numpy()[s, :int(d_nb[c][s])].tobytes() for s in range(4)] for c in range(2)]
        assert b.status() == 0
        for c in range(2):
            for s in range(4):
                p = pos[s] + F * c
                assert got[c][s] == b"".join(f.bs for f in w[s][1][p:p + F]), "%s call %d slot %d (entry %d)" % (tag, c, s, lives[s][1])
        for s in range(4):
            lives[s][2] += 2 * F
        # slot 0's blob against a new uniform batch of its control, fed the same frames
        if lives[0][2] == 2 * F:
            one = api.Batch(api.default_control(**menu[lives[0][1]]), nstreams=1, max_frames=F)
            for c in range(2):
                blk = np.ascontiguousarray(w[0][0][F * c * 1152:F * (c + 1) * 1152].reshape(1, -1))
                assert device_call(one, blk, F)[0][0] == got[c][0]
            alone = one.get_stream_state(0)
            one.close()
            assert blob_diff(b.get_stream_state(0), alone, True) == "", "%s: slot 0's blob is not a new stream's of entry %d" % (tag, lives[0][1])

    two_calls("kind 0")
    for entry, kind in ((1, 1), (2, 3), (3, 2), (0, 0)):
        b.assign_streams([0], [entry], stream=st)
        lives[0] = [lives[0][0] + 100, entry, 0]
        assert b.stream_frames_per_block(0) == 1 + (kind & 1) and b.stream_config(0) == entry
        two_calls("slot 0 as kind %d" % kind)
    b.close()


def test_optional_outputs_of_pipelined_submits(k6_build):
    """three submit_f32_device calls with two sets of row buffers in turn, the ledger's records read into device memory behind
    every one of them, and one wait: rows, packets and their sizes (an MPEG-2 stream's two beside an MPEG-1 stream's
    {size, 0}), frame counters, per-frame CRCs, the dense image and the records after every call equal what the host rules
    derive from the oracle's frames.  Every record was opened with its slot's own frames per block; the files in slots 1
    (MPEG-2) and 4 (MPEG-1) end inside the second call."""
    import torch
    skip_unless_host_libm_is_the_restated_one()
    A = api
    F, NC, PK = 4, 3, 2048
    w = [want_f32(1700 + i, key(kw)) for i, kw in enumerate(ENTRIES)]
    pcm, frames = [x for x, _ in w], [list(f) for _, f in w]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    b = any_batch()
    stride, cap = b.out_stride(F), b.dense_bound(F)
    ncalls = [20, 5, 20, 20, 5, 20, 20, 20]
    b.ledger_begin(list(range(S)), ncalls, stream=st)
    recs = [A.ledger_open(n, FPB[s], 0, 0) for s, n in enumerate(ncalls)]
    LB = C.sizeof(A.Ledger)

    # rows and byte counts alternate between two sets, so call 2 overwrites call 0's; the optional outputs are per call
    sets = [CallBufs(b, F, counters=True, crc=True, packets=PK, image=Image(S, cap, guard=0)) for _ in range(NC)]
    leds = [torch.full((S * LB,), FILL, dtype=torch.uint8, device=dev) for _ in range(NC)]
    assert all(led.data_ptr() % 16 == 0 for led in leds)
    d_pcm = [torch.from_numpy(rows_of(pcm, [F * c] * S, [F] * S, F, True)).to(dev) for c in range(NC)]
    torch.cuda.synchronize()
    for c in range(NC):
        sets[c].set_on(b)
        b.submit_device(d_pcm[c].data_ptr(), F, sets[c & 1].ptr, stride, sets[c & 1].nb.data_ptr(), st, f32=True)
        b.ledger_read_device(list(range(S)), leds[c].data_ptr(), stream=st)
    b.wait(st)
    torch.cuda.synchronize()
    assert b.status() == 0
    for c in range(NC):
        rows = np.zeros((S, stride), np.uint8)
        nb = np.zeros(S, np.int32)
        stats = np.zeros((S, F, 2), np.int32)
        for s in range(S):
            bs = b"".join(f.bs for f in frames[s][F * c:F * (c + 1)])
            rows[s, :len(bs)] = np.frombuffer(bs, np.uint8)
            nb[s] = len(bs)
            stats[s] = [(f.frames_out, f.bytes_out) for f in frames[s][F * c:F * (c + 1)]]
        crc, _ = expected_crc(rows, nb, stats)
        ended = [bool(A.ledger_update(recs[s], stats[s], crc[s], nb[s])) for s in range(S)]
        assert ended == [c == 1 and s in (1, 4) for s in range(S)], "call %d: which files the host's rule ends" % c
        o, tag = sets[c], "call %d" % c
        dense, off = o.image.host()
        check_image(rows, nb, dense, off, cap, tag=tag)
        pk, pkb, g_stats = o.packets()
        for s in range(S):
            assert dense[off[s]:off[s] + nb[s]].tobytes() == rows[s, :nb[s]].tobytes(), "%s stream %d: bitstream" % (tag, s)
            for f in range(F):
                fr = frames[s][F * c + f]
                at = "%s stream %d frame %d" % (tag, s, f)
                n0, n1 = fr.sizes
                assert n0 > 0 and (n1 > 0) == (FPB[s] == 2), at         # (the expectation itself: one packet, or the MPEG-2 block's two)
                assert tuple(pkb[s, f]) == (n0, n1), at + ": packet sizes"
                assert pk[s, f, :n0 + n1].tobytes() == fr.packet, at + ": packet"
                assert (pk[s, f, n0 + n1:] == FILL).all(), at + ": bytes written behind the packet"
                assert tuple(g_stats[s, f]) == (fr.frames_out, fr.bytes_out), at + ": frames / bytes emitted so far"
        if c > 0:
            g_rows, g_nb = sets[c & 1].rows()
            assert g_nb.tolist() == nb.tolist() and all(g_rows[s, :nb[s]].tobytes() == rows[s, :nb[s]].tobytes() for s in range(S)), tag + ": rows"
        assert (o.host()[3] == crc).all(), tag + ": per-frame CRCs"
        led = leds[c].cpu().numpy()
        for s in range(S):
            assert led[s * LB:(s + 1) * LB].tobytes() == recs[s].tobytes(), "%s: the record of slot %d differs from hx_ledger_update's" % (tag, s)
    got = b.ledger_read(list(range(S)))
    assert [r.frames_per_call for r in got] == FPB
    assert [bool(r.ended) for r in got] == [s in (1, 4) for s in range(S)]
    b.close()


@pytest.mark.one_k6_build
def test_beyond_the_resident_set(monkeypatch, k6_build):
    """HMP3AMD_K6=slim, the resident set + 64 streams of kind 0 with 8 MPEG-2 and 4 first-generation streams among them, three
    calls of two frames: the persistent workgroups claim their streams under a span shorter than the batch, the claim counter
    is back at zero for the kinds' launches that follow and for the next call, and every stream comes out the oracle's"""
    skip_unless_host_libm_is_the_restated_one()
    monkeypatch.setenv("HMP3AMD_K6", "slim")
    menu = [dict(), ENTRIES[1], ENTRIES[7], ENTRIES[2], ENTRIES[3]]      # VBR -V50 stereo; 22.05 and 24 kHz; dual channel 44.1 and 16 kHz
    probe = api.Batch.any(controls(menu), 1, cfg=[0], max_frames=2)
    resident = probe.resident_streams()
    assert probe.k6_variant() == 1
    probe.close()
    F, calls = 2, 3
    n0 = resident + 64
    S_all = n0 + 12
    cfg = [0] * S_all
    for j in range(12):         # the others spread over the batch, first and last slot included
        cfg[j * (S_all - 1) // 11] = [1, 2, 1, 3, 2, 1, 4, 2, 1, 3, 2, 4][j]
    assert sorted(set(cfg)) == [0, 1, 2, 3, 4] and cfg.count(0) == n0 and cfg.count(3) + cfg.count(4) == 4
    base = {e: [synth.stream_pcm(7400 + 20 * e + u, F * calls, sr=menu[e].get("samprate", 44100), rho=RHOS[u % 4], bursts=True) for u in range(16 if e == 0 else 2)]
            for e in range(len(menu))}
    pcm = np.stack([np.roll(base[e][i % len(base[e])], 1152 * ((i // 16) % (F * calls)), axis=0) for i, e in enumerate(cfg)])
    b = api.Batch.any(controls(menu), S_all, cfg=cfg, max_frames=F)
    assert b.k6_variant() == 1 and b.resident_streams() < n0
    got = [b"" for _ in range(S_all)]
    for c in range(calls):
        out = b.encode_host(pcm[:, c * F * 1152:(c + 1) * F * 1152])
        for s in range(S_all):
            got[s] += out[s]
    assert b.status() == 0
    b.close()
    want = oracle_bytes_many([menu[e] for e in cfg], pcm, F * calls)
    bad = [s for s in range(S_all) if got[s] != want[s]]
    assert not bad, "%d of %d streams differ from the oracle, first: %s (entries %s)" % (len(bad), S_all, bad[:8], [cfg[s] for s in bad[:8]])


def test_multi_over_two_blocks(k6_build):
    """five streams in blocks of three and two on one device, the kinds split unevenly - 0, 1, 2 in the first block, 1 and 3
    in the second, every block with the whole menu; one call, an assign that crosses both blocks, another call"""
    skip_unless_host_libm_is_the_restated_one()
    menu = [ENTRIES[0], ENTRIES[1], ENTRIES[2], ENTRIES[3], ENTRIES[4]]      # kinds 0, 1, 2, 3, 0 (mono)
    cfg = [0, 1, 2, 1, 3]
    m = api.Multi.any(controls(menu), 5, cfg=cfg, max_frames=3, devices=[0, 0])
    assert m.ndevices() == 2 and [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    assert m.pcm_channels() == 2 and [m.stream_frames_per_block(i) for i in range(5)] == [1, 2, 1, 2, 2]
    w = [want_f32(1900 + i, key(menu[c])) for i, c in enumerate(cfg)]
    got = m.encode_host(rows_of([x for x, _ in w], [0] * 5, [3] * 5, 3, True))
    assert m.status() == 0
    for s in range(5):
        assert got[s] == b"".join(f.bs for f in w[s][1][:3]), "first call, stream %d" % s
    m.assign_streams([2, 3], [3, 4])
    assert [m.stream_frames_per_block(i) for i in range(5)] == [1, 2, 2, 1, 2] and [m.stream_channels(i) for i in range(5)] == [2, 2, 2, 1, 2]
    pos = [3, 3, 0, 0, 3]
    for s, c in ((2, 3), (3, 4)):
        w[s] = want_f32(1950 + s, key(menu[c]))
    got = m.encode_host(rows_of([x for x, _ in w], pos, [3] * 5, 3, True))
    assert m.status() == 0
    for s in range(5):
        assert got[s] == b"".join(f.bs for f in w[s][1][pos[s]:pos[s] + 3]), "second call, stream %d" % s
    m.close()


@pytest.mark.parametrize("counts", [None, [[3, 1, 2], [0, 3, 3]]], ids=["uniform", "per_stream_counts"])
def test_converting_batch(counts, k6_build):
    """44.1 kHz s16 sources into a 44.1 kHz entry and into a 22.05 kHz entry, a 48 kHz s24 source summed to mono into a 16 kHz
    entry: the rows are the oracle's for hx_src_convert's PCM under the control src_encode_control derives"""
    A = api
    F = 3
    streams = [Stream(44100, 16, 0, seed=31, seconds=1.0), Stream(44100, 16, 0, mpeg_select=22050, seed=32, seconds=1.0, bitrate=32),
               Stream(48000, 24, 0, mono_convert=1, mpeg_select=16000, seed=33, seconds=1.0, bitrate=32)]
    n = len(streams)
    b = A.SrcBatch.any([s.ec for s in streams], [s.src for s in streams], n, cfg=list(range(n)), max_frames=F)
    assert [b.stream_frames_per_block(i) for i in range(n)] == [1, 2, 2] and [b.stream_channels(i) for i in range(n)] == [2, 2, 1]
    conv = [host_converted(s, 2 * F) for s in streams]
    frames = []
    for s, (y, _, _) in zip(streams, conv):
        ec2, nbytes = A.src_encode_control(s.ec, s.src)
        assert nbytes > 0
        frames.append(PC.oracle_frames(ec2, y))
    done, pos = [0] * n, [0] * n
    for c in range(2):
        cnt = [F] * n if counts is None else counts[c]
        stride = b.in_stride(F)
        rows = np.zeros((n, stride), np.uint8)
        for i, s in enumerate(streams):
            chunk = np.frombuffer(s.data[pos[i]:pos[i] + stride], np.uint8)
            rows[i, :len(chunk)] = chunk
        if counts is None:
            res, used = b.encode_src_host(rows, F)
        else:
            res, used = b.encode_src_counts_host(rows, F, cnt)
        assert b.status() == 0
        for i in range(n):
            _, ub, _ = conv[i]
            at = "call %d stream %d (%d calls)" % (c, i, cnt[i])
            assert res[i] == b"".join(f.bs for f in frames[i][done[i]:done[i] + cnt[i]]), at + ": bitstream"
            assert int(used[i]) == sum(ub[done[i]:done[i] + cnt[i]]), at + ": input bytes used"
            done[i] += cnt[i]
            pos[i] += int(used[i])
    b.close()


@pytest.mark.parametrize("flags", [[], ["-M2"]], ids=["joint_stereo", "dual_channel"])
def test_cli_batch_of_files_of_every_kind(tmp_path, flags, k6_build):
    """hmp3amd -batch and -batch -slots2 on four short files - 44.1 kHz stereo, 22.05 kHz stereo, 16 kHz mono and another
    44.1 kHz stereo one: every output is the file's single-file run.  The tool's flags hold for all files of a run, so the
    dual-channel flag (-M2) is a run of its own: the stereo files are then first-generation streams at both versions, beside
    the mono MPEG-2 one."""
    if flags:
        skip_unless_host_libm_is_the_restated_one()
    files = [("a", 44100, 2, 21), ("b", 22050, 2, 9), ("c", 16000, 1, 14), ("d", 44100, 2, 6)]
    args = {"batch": [], "slots2": []}
    for k, (name, sr, ch, nframes) in enumerate(files):
        nsamp = nframes * 1152 - 301 * k - 7
        x = synth.stream_pcm(80 + k, nframes, sr=sr, rho=RHOS[k % 4], bursts=True)[:nsamp]
        wav = str(tmp_path / (name + ".wav"))
        write_wav(wav, x if ch == 2 else np.ascontiguousarray(x[:, 0]), sr, False)
        one = str(tmp_path / (name + ".one.mp3"))
        run_cli([wav, one] + flags)
        for how in args:
            args[how] += [wav, str(tmp_path / ("%s.%s.mp3" % (name, how)))]
    for how, slots in (("batch", []), ("slots2", ["-slots2"])):
        run_cli(["-batch"] + slots + args[how] + flags)
        for name, *_ in files:
            got = open(str(tmp_path / ("%s.%s.mp3" % (name, how))), "rb").read()
            assert len(got) > 1000 and got == open(str(tmp_path / (name + ".one.mp3")), "rb").read(), "%s (%s): differs from its single-file run" % (name, how)
