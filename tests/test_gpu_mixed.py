"""Mixed batches (hx_batch_create_mixed, hx_multi_create_mixed): mono and stereo streams in one batch and one menu.

The PCM rows of a mixed batch are pitched for P = 2 channels; a mono stream's samples sit contiguous at the start of its row
and the rest of the row is filled with 0x7FFF (s16) or NaN (f32) here: nothing may depend on it.  Every expectation is
byte identity against the oracle, one encoder per stream life fed frame by frame (packet_cases.oracle_frames for fp32 input,
OracleEncoder.encode_s16 for int16); converting streams go through this library's host converter (hx_src_convert) and then
the oracle.  Shapes are the smallest that cross every seam: six streams, three or four frames per call, two calls or more.
Blob comparisons across batches use device calls into zeroed output buffers: a stream's ring of pending main data keeps
whatever bytes lie behind its frames in the call's row."""
import numpy as np
import pytest

import packet_cases as PC
from gpu_support import CallBufs, Image, batch_vs_single_vs_reference, controls, plain_call as device_call, write_wav
from hmp3_amd import api, synth
from mixed_cases import RHOS, blob_diff, joined, key, mono, rows_of, streams_of, want_f32
from output_checks import check_call, check_image, expected_crc
from src_cases import Stream, host_converted

pytestmark = pytest.mark.gpu

# stereo CBR-128 44.1 kHz, mono CBR-64 44.1 kHz, joint-stereo VBR 48 kHz, mono 32 kHz behind the DC blocker (test_gpu_parity's
# MONO["mono_cbr48_32k_long_dc"]), stereo behind the DC blocker, mono VBR 48 kHz
ENTRIES = [dict(bitrate=64), dict(bitrate=64, mode=3), dict(samprate=48000),
           dict(bitrate=48, mode=3, samprate=32000, short_block_threshold=99999, filter_select=1),
           dict(bitrate=64, filter_select=1), dict(mode=3, samprate=48000)]
S = len(ENTRIES)
CHANNELS = [1 if kw.get("mode") == 3 else 2 for kw in ENTRIES]


def six(f32, seed=700):
    """the six streams of ENTRIES: (signals, the oracle's bytes per frame)"""
    return streams_of(ENTRIES, f32, seed)


def mixed_batch(menu=ENTRIES, cfg=None, n=None, max_frames=4):
    n = len(menu) if n is None else n
    return api.Batch.mixed(controls(menu), n, cfg=list(range(n)) if cfg is None else cfg, max_frames=max_frames)


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_plain_parity_over_two_calls(f32, k6_build):
    pcm, want = six(f32)
    b = mixed_batch()
    assert b.pcm_channels() == 2 and [b.stream_channels(i) for i in range(S)] == CHANNELS
    assert b.nconfigs() == S and [b.stream_config(i) for i in range(S)] == list(range(S))
    got = [b.encode_host(rows_of(pcm, [0] * S, [4] * S, 4, f32))]
    bt = b.debug_read("bt", np.uint8, S * 8).reshape(S, 8)
    assert all((bt[s] == 2).any() for s in (0, 1, 2, 4, 5)), "the streams' onsets no longer give short blocks: %s" % bt.tolist()
    got.append(b.encode_host(rows_of(pcm, [4] * S, [4] * S, 4, f32)))
    assert b.status() == 0
    for s in range(S):
        assert got[0][s] == joined(want[s], 0, 4), "stream %d, first call" % s
        assert got[1][s] == joined(want[s], 4, 4), "stream %d, second call" % s
    assert [b.frames_bytes(s)[1] for s in range(S)] == [len(joined(want[s], 0, 8)) for s in range(S)]
    b.close()


def test_three_dimensional_pcm_is_the_same_rows(k6_build):
    """encode_host takes [S][n][P] as well as [S][n * P]"""
    pcm, want = six(True)
    b = mixed_batch()
    got = b.encode_host(rows_of(pcm, [0] * S, [4] * S, 4, True).reshape(S, 4 * 1152, 2))
    assert b.status() == 0 and all(got[s] == joined(want[s], 0, 4) for s in range(S))
    with pytest.raises(ValueError):
        b.encode_host(np.zeros((S, 4 * 1152, 1), np.float32))
    b.close()


def test_device_pcm_pointer_two_bytes_off_a_16_byte_boundary(k6_build):
    pcm, want = six(False)
    b = mixed_batch()
    got, ptr = device_call(b, rows_of(pcm, [0] * S, [4] * S, 4, False), 4, shift=1)
    assert ptr % 16 == 2
    assert b.status() == 0
    for s in range(S):
        assert got[s] == joined(want[s], 0, 4), "stream %d" % s
    b.close()


@pytest.mark.parametrize("which", ["mono", "stereo"])
def test_a_uniform_menu_is_the_menu_batch(which, k6_build):
    """Batch.mixed over entries of one channel count: pcm_channels is that count, and rows, out_bytes and checkpoint blobs
    are Batch.menu's on the same input, byte for byte"""
    menu = [kw for kw in ENTRIES if mono(kw) == (which == "mono")]
    ch = 1 if which == "mono" else 2
    x = [want_f32(740 + i, key(kw))[0] for i, kw in enumerate(menu)]
    res = []
    for make in (api.Batch.mixed, api.Batch.menu):
        b = make(controls(menu), len(menu), cfg=list(range(len(menu))), max_frames=4)
        assert b.pcm_channels() == ch and [b.stream_channels(i) for i in range(b.n)] == [ch] * b.n
        outs = []
        for c in range(2):
            blk = np.stack([p[4 * c * 1152:4 * (c + 1) * 1152].reshape(-1) for p in x])
            outs.append(device_call(b, blk, 4)[0])
        assert b.status() == 0
        res.append((outs, b.get_stream_states(range(b.n)), b.k6_variant(), b.out_stride(4)))
        b.close()
    for i in range(len(menu)):
        assert blob_diff(res[0][1][i], res[1][1][i]) == "", "stream %d: checkpoint blob" % i
    assert res[0] == res[1]
    for i, kw in enumerate(menu):
        frames = want_f32(740 + i, key(kw))[1]
        assert res[0][0][0][i] + res[0][0][1][i] == b"".join(f.bs for f in frames[:8]), i


def test_per_stream_counts(k6_build):
    """a full call, then counts [4, 0, 3, 1, 4, 2] and [0, 2, 1, 4, 3, 4]: every stream advances by its own count, and the
    mono and the stereo stream that sit a call out keep their blobs bit for bit"""
    pcm, want = six(True)
    b = mixed_batch()
    pos = [0] * S
    for c, counts in enumerate([[4] * S, [4, 0, 3, 1, 4, 2], [0, 2, 1, 4, 3, 4]]):
        idle = [i for i in range(S) if counts[i] == 0]
        before = b.get_stream_states(idle)
        b.frame_counts(counts)
        got = b.encode_host(rows_of(pcm, pos, counts, 4, True))
        assert b.status() == 0
        assert b.get_stream_states(idle) == before, "call %d: a stream that took no frame changed" % c
        for s in range(S):
            assert got[s] == joined(want[s], pos[s], counts[s]), "call %d stream %d (count %d)" % (c, s, counts[s])
            pos[s] += counts[s]
    assert CHANNELS[1] == 1 and CHANNELS[0] == 2        # (the two that sat out)
    b.close()


def test_assign_across_channel_counts(k6_build):
    """four slots on loud stereo for two calls; slots 0 and 2 become mono streams for two calls; slot 0 goes back to stereo
    for two calls.  After each assign the slot's rows are a new stream's, and after its first call its checkpoint blob is
    that of slot 0 of a new uniform batch fed the same frames (but for the class index): a mono stream's second-channel
    subband rows, pre-echo memory and PCM history hold nothing of the stereo stream before it, and the reverse.  Slots 1
    and 3 run through all six calls undisturbed."""
    menu = [dict(bitrate=64), dict(bitrate=64, mode=3)]
    F = 3
    lives = [[800 + i, 0, 0] for i in range(4)]        # per slot: [seed, menu entry, frames done]
    b = api.Batch.mixed(controls(menu), 4, cfg=[0] * 4, max_frames=F)
    assert b.pcm_channels() == 2

    def call(tag, fresh=()):
        w = [want_f32(seed, key(menu[e]), 0.5) for seed, e, _ in lives]
        pos = [p for _, _, p in lives]
        got, _ = device_call(b, rows_of([x for x, _ in w], pos, [F] * 4, F, True), F)
        assert b.status() == 0
        for s in range(4):
            assert got[s] == b"".join(f.bs for f in w[s][1][pos[s]:pos[s] + F]), "%s slot %d (entry %d)" % (tag, s, lives[s][1])
            lives[s][2] += F
        for s in fresh:
            one = api.Batch(api.default_control(**menu[lives[s][1]]), nstreams=1, max_frames=F)
            assert device_call(one, np.ascontiguousarray(w[s][0][:F * 1152].reshape(1, -1)), F)[0][0] == got[s]
            alone = one.get_stream_state(0)
            one.close()
            mine = b.get_stream_state(s)
            assert mine != alone or lives[s][1] == 0, "slot %d: the class index word should differ" % s
            assert blob_diff(mine, alone, True) == "", "%s slot %d: its blob is not a new %s stream's" % (tag, s, "mono" if lives[s][1] else "stereo")

    def assign(idx, entry):
        b.assign_streams(idx, [entry] * len(idx))
        for s in idx:
            lives[s] = [lives[s][0] + 100, entry, 0]
        assert [b.stream_channels(s) for s in range(4)] == [1 if e else 2 for _, e, _ in lives]

    call("call 0")
    call("call 1")
    assign([0, 2], 1)
    call("call 2 (slots 0, 2 mono)", fresh=[0, 2])
    call("call 3")
    assign([0], 0)
    call("call 4 (slot 0 stereo again)", fresh=[0])
    call("call 5")
    b.close()


def test_optional_outputs_of_pipelined_submits(k6_build):
    """three submit_f32_device calls with two sets of output buffers in turn and one wait: rows, packets, frame counters,
    per-frame CRCs and the dense image of every call (the first call's rows from its image: the third call has its row
    set) and the ledger equal what the host rules derive from the oracle's frames.  The mono file in slot 1 and the
    stereo file in slot 4 end inside the second call."""
    import torch
    A = api
    F, NC, PK = 4, 3, 2048
    w = [want_f32(700 + i, key(kw)) for i, kw in enumerate(ENTRIES)]
    pcm, frames = [x for x, _ in w], [list(f) for _, f in w]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    b = mixed_batch()
    stride, cap = b.out_stride(F), b.dense_bound(F)
    ncalls = [20, 5, 20, 20, 5, 20]
    b.ledger_begin(list(range(S)), ncalls, stream=st)
    recs = [A.ledger_open(n, 1, 0, 0) for n in ncalls]

    # rows and byte counts alternate between two sets, so call 2 overwrites call 0's; the optional outputs are per call
    sets = [CallBufs(b, F, counters=True, crc=True, packets=PK, image=Image(S, cap, guard=0)) for _ in range(NC)]
    d_pcm = [torch.from_numpy(rows_of(pcm, [F * c] * S, [F] * S, F, True)).to(dev) for c in range(NC)]
    torch.cuda.synchronize()
    for c in range(NC):
        sets[c].set_on(b)
        b.submit_device(d_pcm[c].data_ptr(), F, sets[c & 1].ptr, stride, sets[c & 1].nb.data_ptr(), st, f32=True)
    b.wait(st)
    torch.cuda.synchronize()
    assert b.status() == 0
    # what the host derives from the oracle's frames, call by call: rows, byte counts, counters, CRCs and the records
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
        if c == 0:      # (its rows are gone: the image holds them)
            got_bs = [dense[off[s]:off[s] + nb[s]].tobytes() for s in range(S)]
        else:
            g_rows, g_nb = sets[c & 1].rows()
            assert g_nb.tolist() == nb.tolist(), tag
            got_bs = [g_rows[s, :g_nb[s]].tobytes() for s in range(S)]
        check_call(frames, F * c, F, got_bs, *o.packets(), 0, tag)
        assert (o.host()[3] == crc).all(), tag + ": per-frame CRCs"
    got = b.ledger_read(list(range(S)))
    for s in range(S):
        assert got[s].tobytes() == recs[s].tobytes(), "the record of slot %d differs from hx_ledger_update's" % s
    assert [bool(r.ended) for r in got] == [s in (1, 4) for s in range(S)]
    b.close()


@pytest.mark.parametrize("which", [1, 0], ids=["mono", "stereo"])
def test_blobs_move_between_a_mixed_and_a_uniform_batch(which, k6_build):
    """stream `which` of the mixed batch after one call continues in a uniform batch of its control, and a stream saved
    from that uniform batch after one call continues in slot `which` of a new mixed batch"""
    pcm, want = six(True)
    kw = ENTRIES[which]
    uni = lambda: api.Batch(api.default_control(**kw), nstreams=1, max_frames=4)
    own = lambda f0: np.ascontiguousarray(pcm[which][f0 * 1152:(f0 + 4) * 1152].reshape(1, -1))
    m = mixed_batch()
    assert m.encode_host(rows_of(pcm, [0] * S, [4] * S, 4, True))[which] == joined(want[which], 0, 4)
    blob = m.get_stream_state(which)
    m.close()
    u = uni()
    u.set_stream_state(0, blob)
    assert u.encode_host(own(4))[0] == joined(want[which], 4, 4), "mixed -> uniform"
    assert u.status() == 0
    u.close()
    u = uni()
    assert u.encode_host(own(0))[0] == joined(want[which], 0, 4)
    blob = u.get_stream_state(0)
    u.close()
    m = mixed_batch()
    m.set_stream_state(which, blob)
    pos = [4 if s == which else 0 for s in range(S)]
    got = m.encode_host(rows_of(pcm, pos, [4] * S, 4, True))
    assert m.status() == 0
    for s in range(S):
        assert got[s] == joined(want[s], pos[s], 4), "uniform -> mixed: stream %d" % s
    m.close()


@pytest.mark.one_k6_build
def test_multi_over_two_blocks(k6_build):
    """five streams of channel counts [2, 1, 1, 2, 1] in blocks of three and two on one device: the boundary falls between
    a mono and a stereo row; one call, an assign that crosses both blocks, another call"""
    menu = [dict(bitrate=64), dict(bitrate=64, mode=3)]
    cfg = [0, 1, 1, 0, 1]
    m = api.Multi.mixed(controls(menu), 5, cfg=cfg, max_frames=3, devices=[0, 0])
    assert m.ndevices() == 2 and [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    assert m.pcm_channels() == 2 and [m.stream_channels(i) for i in range(5)] == [2, 1, 1, 2, 1]
    w = [want_f32(900 + i, key(menu[c])) for i, c in enumerate(cfg)]
    got = m.encode_host(rows_of([x for x, _ in w], [0] * 5, [3] * 5, 3, True))
    assert m.status() == 0
    for s in range(5):
        assert got[s] == b"".join(f.bs for f in w[s][1][:3]), "first call, stream %d" % s
    m.assign_streams([2, 3], [0, 1])
    assert [m.stream_channels(i) for i in range(5)] == [2, 1, 2, 1, 1]
    pos = [3, 3, 0, 0, 3]
    for s, c in ((2, 0), (3, 1)):
        w[s] = want_f32(950 + s, key(menu[c]))
    got = m.encode_host(rows_of([x for x, _ in w], pos, [3] * 5, 3, True))
    assert m.status() == 0
    for s in range(5):
        assert got[s] == b"".join(f.bs for f in w[s][1][pos[s]:pos[s] + 3]), "second call, stream %d" % s
    m.close()


# ---- converting batches ----

@pytest.mark.parametrize("counts", [None, [[3, 1, 2, 0], [2, 3, 0, 3]]], ids=["uniform", "per_stream_counts"])
def test_converting_mixed_batch(counts, k6_build):
    """stereo s16 44.1 kHz, mono u8 32 -> 44.1 kHz, stereo s24 48 -> 44.1 kHz summed to mono, mono f32 44.1 kHz: the
    converted PCM (the "srcpcm" tap) is hx_src_convert's bit for bit, each stream's calls contiguous at the start of a row
    pitched for two channels, and the rows are the oracle's for that PCM under the control src_encode_control derives"""
    A = api
    F = 3
    streams = [Stream(44100, 16, 0, seed=21, seconds=1.0), Stream(32000, 8, 0, channels=1, mpeg_select=44100, seed=22, seconds=1.0),
               Stream(48000, 24, 0, mono_convert=1, mpeg_select=44100, seed=23, seconds=1.0), Stream(44100, 32, 1, channels=1, seed=24, seconds=1.0)]
    n = len(streams)
    b = A.SrcBatch.mixed([s.ec for s in streams], [s.src for s in streams], n, cfg=list(range(n)), max_frames=F)
    assert b.pcm_channels() == 2 and [b.stream_channels(i) for i in range(n)] == [2, 1, 1, 1]
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
        tap = b.debug_read("srcpcm", np.float32, n * F * 1152 * 2).reshape(n, F * 1152 * 2)
        for i in range(n):
            y, ub, tch = conv[i]
            at = "call %d stream %d (%d calls)" % (c, i, cnt[i])
            wantpcm = y[done[i] * 1152:(done[i] + cnt[i]) * 1152].reshape(-1)
            assert np.array_equal(tap[i, :len(wantpcm)].view(np.uint32), wantpcm.view(np.uint32)), at + ": converted PCM"
            assert res[i] == b"".join(f.bs for f in frames[i][done[i]:done[i] + cnt[i]]), at + ": bitstream"
            assert int(used[i]) == sum(ub[done[i]:done[i] + cnt[i]]), at + ": input bytes used"
            done[i] += cnt[i]
            pos[i] += int(used[i])
    b.close()


# ---- the command line ----

@pytest.mark.one_k6_build
@pytest.mark.parametrize("flags", [[], ["-A32000", "-B64"]], ids=["fp32_frames", "converting"])
@pytest.mark.parametrize("slots", [[], ["-slots2"]], ids=["batch", "slots2"])
def test_cli_batch_of_mono_and_stereo_files(tmp_path, flags, slots, k6_build):
    """hmp3amd -batch [-slots2] on five files of either channel count, 5 to 130 frames: every output is the file's
    single-file run and, where the reference binary is built, the reference's"""
    # (name, rate, channels, write_wav's format: False s16, True f32, 8 / 24 integer widths, frames)
    files = [("a", 44100, 2, False, 130), ("b", 44100, 1, False, 5), ("c", 48000, 2, 24, 37), ("d", 48000, 1, True, 61), ("e", 32000, 1, 8, 18)]
    pairs = []
    for k, (name, sr, ch, fmt, frames) in enumerate(files):
        nsamp = frames * 1152 * (sr // 100 if flags else 320) // 320 - 301 * k - 7
        x = synth.stream_pcm(60 + k, nsamp // 1152 + 1, sr=sr, rho=RHOS[k % 4], bursts=True)[:nsamp]
        write_wav(str(tmp_path / (name + ".wav")), x if ch == 2 else np.ascontiguousarray(x[:, 0]), sr, fmt)
        pairs.append((name, str(tmp_path / (name + ".wav")), str(tmp_path / (name + ".batch.mp3"))))
    batch_vs_single_vs_reference(pairs, flags, slots, floor=1000)
