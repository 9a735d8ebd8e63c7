"""The file ledger on a real MI355X (include/hmp3_amd.h, "file ledger"; k_ledger in hmp3_amd/csrc/hx_ledger.hip): per stream
one record that says where the stream's file ends, which bytes of that call belong to it, their MusicCRC and the Xing seek
points, updated on the GPU behind every call.

Every comparison is equality, bytewise on whole records.  The expected record is hx_ledger_update on the host over the same
call's own frame counters, CRCs and byte counts read back from the device (tests/test_ledger_host.py holds that function to
the loop it restates).  A twin batch without a ledger takes the same calls and must give identical rows, byte counts,
counters and CRCs.  The ledger does not depend on the build of the rate-loop kernel: the tests run once (one_k6_build).

hx_xing keeps 512 seek points, so its table is first halved at the 512th sampled call and again at the 1024th: the
seek-point test runs files of 1030 calls."""
import ctypes as C

import numpy as np
import pytest

import ledger_cases as H
from gpu_support import CallBufs, cur_stream, dev, run_cli, sync, write_wav
from hmp3_amd import api, synth
from ledger_cases import DRAIN, NEVER, RESTART, SITS_OUT, SMALL_NCALLS, block, small_batch, small_counts, small_pcm, small_restart_pcm
from output_checks import same_outputs
from src_cases import Stream, make_batch

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


def ledger_bufs(b, nf, odd=False):
    """every output buffer of one device call: rows, byte counts, frame counters (odd: starting 4 bytes past an 8-byte
    boundary), per-frame CRCs"""
    return CallBufs(b, nf, counters=True, odd=odd, crc=True)


class Run:
    """a batch with a ledger and its twin without, fed the same plain device calls; `want` are the host's records"""

    def __init__(self, make, full, odd=False):
        self.b, self.t, self.full, self.odd = make(), make(), full, odd
        self.S = self.b.n
        self.want = [api.Ledger() for _ in range(self.S)]
        self.given = [0] * self.S
        self.ends, self.frozen, self.calls = [], 0, 0

    def begin(self, idx, ncalls, head_bytes=0, flags=0, fpc=1):
        self.b.ledger_begin(idx, ncalls, head_bytes, flags, stream=cur_stream())
        per_slot = [[v] * len(idx) if np.isscalar(v) else list(v) for v in (ncalls, head_bytes, flags)]
        for e, s in enumerate(idx):
            self.want[s] = api.ledger_open(per_slot[0][e], fpc, per_slot[1][e], per_slot[2][e])

    def host_update(self, counts, nb, st, cr):
        for s, n in enumerate(counts):
            was_live = self.want[s].open and not self.want[s].ended
            self.frozen += bool(self.want[s].ended and n > 0)
            if api.ledger_update(self.want[s], st[s, :n], cr[s, :n], nb[s]):
                self.ends.append((self.want[s].fed - 1 - self.given[s], n))
            assert not (was_live and n > 0 and self.want[s].call_bytes > nb[s])
            self.given[s] += n

    def records(self):
        return [r.tobytes() for r in self.b.ledger_read(list(range(self.S)))]

    def check_records(self, tag):
        got = self.records()
        for s in range(self.S):
            assert got[s] == self.want[s].tobytes(), "%s: the record of slot %d differs from hx_ledger_update's (fed %d, ended %d)" % (
                tag, s, self.want[s].fed, self.want[s].ended)
        return got

    def step(self, counts):
        """one plain device call under per-stream counts on both batches -> the ledger batch's (rows, nb, stats, crc)"""
        import torch
        nf = max(counts)
        d_pcm = torch.from_numpy(block(self.full, self.given, counts, nf)).to(dev())
        sync()
        outs = []
        for h in (self.b, self.t):
            o = ledger_bufs(h, nf, self.odd)
            o.set_on(h)
            h.frame_counts(counts)
            h.encode_device(d_pcm.data_ptr(), nf, o.ptr, o.stride, o.nb.data_ptr(), cur_stream(), f32=True)
            outs.append(o)
        sync()
        got, twin = outs[0].host(), outs[1].host()
        tag = "call %d" % self.calls
        same_outputs(got, twin, counts, tag)
        self.host_update(counts, *got[1:])
        self.check_records(tag)
        self.calls += 1
        return got

    def close(self):
        assert self.b.status() == 0 and self.t.status() == 0
        self.b.close()
        self.t.close()


def test_small_shape_every_kind_of_end():
    """9 streams, CBR-128 stereo 44.1 kHz, plain device calls of 8 frames under counts min(8, ncalls + 32 - fed): files of 1, 7,
    8, 9, 16, 20 and 15 calls followed by silence.  After every call every record equals the host's.  The ends include one on
    the first and one on the last frame of a call; ended slots go on taking silence with their records frozen but for
    call_bytes = 0; the slot that is never begun stays all zero; a begun slot that sits a call out is unchanged across it"""
    r = Run(small_batch, small_pcm())
    begun = [s for s in range(r.S) if s != NEVER]
    r.begin(begun, [SMALL_NCALLS[s] for s in begun])
    before = None
    while True:
        counts = small_counts(r.given, SMALL_NCALLS, r.calls)
        if not any(counts):
            break
        if r.calls == 1:
            before = r.records()[SITS_OUT]
        r.step(counts)
        if r.calls == 2:
            rec = r.want[SITS_OUT]
            assert r.records()[SITS_OUT] == before and rec.open and not rec.ended and rec.fed == 8
    final = r.records()
    assert final[NEVER] == bytes(C.sizeof(api.Ledger))
    assert all(r.want[s].ended for s in begun)
    assert [r.want[s].call_bytes for s in begun] == [0] * len(begun) and r.frozen >= len(begun)
    assert any(f == 0 for f, n in r.ends), "no file's drain ended on the first frame of a call: %s" % r.ends
    assert any(f == n - 1 for f, n in r.ends), "no file's drain ended on the last frame of a call: %s" % r.ends
    assert len(r.ends) == len(begun) and r.calls >= 7
    r.close()


def test_seek_points_through_two_halvings():
    """4 streams x 17 calls of 64 frames, VBR (the byte positions vary), files of 1030 calls with seek points and the tag
    frame's size from hx_xing_header: the table is halved at the 512th and the 1024th call.  The tag frame built from the
    record equals the tag frame of the host's replay of the counters"""
    S, nf, ncalls = 4, 64, 1030
    base = synth.stream_pcm(6200, ncalls, bursts=True).astype(np.float32)
    full = [np.roll(base, 1152 * 7 * s, axis=0) * (1.0, 0.5, 0.25, 0.8)[s] for s in range(S)]
    r = Run(lambda: api.Batch(api.default_control(), nstreams=S, max_frames=nf), full)
    x = api.lib().hx_xing_create()
    _, head = H.tag_frame(x, 1)
    api.lib().hx_xing_destroy(x)
    r.begin(list(range(S)), ncalls, head_bytes=head, flags=1)
    hist = [[] for _ in range(S)]
    data = [b""] * S
    for c in range(17):
        rows, nb, st, cr = r.step([nf] * S)
        for s in range(S):
            hist[s].append(st[s])
            data[s] += rows[s, :nb[s]].tobytes()
    assert len({len(d) for d in data}) == S
    for s in range(S):
        rec = r.want[s]
        assert rec.ended and rec.every == 4 and 256 <= rec.npt < 512

        class Hist:
            pass
        f = Hist()
        st = np.concatenate(hist[s])
        f.ncalls, f.fpc, f.expected, f.samples = ncalls, 1, ncalls, ncalls * 1152 - 77
        f.fr, f.by = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64)
        f.end = rec.fed - 1
        f.data = np.frombuffer(data[s], np.uint8)
        f.crc_of = lambda a, b, d=f.data: int(api.lib().hx_xing_update_crc(0, d[a:b].tobytes(), b - a))
        tag, frames, nbytes, crc, halvings, n = H.replay(f)
        assert halvings == 2 and n == head
        got = r.b.ledger_read([s])[0]
        assert (got.frames, got.bytes, got.crc) == (frames, nbytes, crc)
        assert H.record_tag(got, 1, f.samples) == tag, "stream %d" % s
    r.close()


def test_files_equal_the_single_file_loops(tmp_path):
    """three WAVs, 44.1 kHz 16-bit, of 5, 40 and 130 frames with -X2 through a batch with the ledger: tag frame from the
    record + the call_bytes of every call + hx_xing_update_info equals, byte for byte, what `hmp3amd in.wav out.mp3 -X2`
    writes for the file"""
    A, L = api, api.lib()
    frames = (5, 40, 130)
    S, CH = len(frames), 48
    ec, used, head = A.default_control(samprate=44100), A.EControl(), A.MpegHead()
    assert L.hx_control_info(C.byref(ec), C.byref(used), C.byref(head)) == 1
    wavs, full, ncalls, samples = [], [], [], []
    for i, nfr in enumerate(frames):
        pcm = synth.stream_pcm(6300 + i, nfr, bursts=True)[:nfr * 1152 - 311 * i]
        wavs.append(str(tmp_path / ("in%d.wav" % i)))
        write_wav(wavs[-1], pcm, 44100, False)
        # the single-file loop's calls: one per 1152 sample frames while 1153 are left of audio ++ 4 x 1153 frames of zeros
        size = len(pcm) * 4 + 4 * 1153 * 4
        ncalls.append((size - 1153 * 4) // 4608 + 1)
        samples.append(len(pcm))
        full.append(pcm.astype(np.float32))
    x = L.hx_xing_create()
    tags, vbr_scale = [], used.vbr_mnr if used.vbr_flag else -1
    for s in range(S):
        buf = (C.c_ubyte * 2048)()
        n = L.hx_xing_header(x, used.samprate, head.mode, used.cr_bit, used.original, 0x4F, 0, 0, vbr_scale, None, buf, None, None, used.bitrate * 2)
        assert n > 0
        tags.append((buf, n))
    r = Run(lambda: A.Batch(ec, nstreams=S, max_frames=CH), full)
    r.begin(list(range(S)), ncalls, head_bytes=[n for _, n in tags], flags=1)
    audio = [b""] * S
    while True:
        counts = [0 if r.want[s].ended else max(0, min(CH, ncalls[s] + DRAIN - r.given[s])) for s in range(S)]
        if not any(counts):
            break
        rows, nb, st, cr = r.step(counts)
        for s in range(S):
            if counts[s]:
                audio[s] += rows[s, :r.want[s].call_bytes].tobytes()
    recs = r.b.ledger_read(list(range(S)))
    r.close()
    for s in range(S):
        rec, (buf, n) = recs[s], tags[s]
        assert rec.ended and rec.bytes == len(audio[s])
        L.hx_xing_header(x, used.samprate, head.mode, used.cr_bit, used.original, 0x4F, 0, 0, vbr_scale, None, buf, None, None, used.bitrate * 2)
        A.xing_load_points(x, rec)
        assert L.hx_xing_update_info(x, rec.frames, n + rec.bytes, vbr_scale, None, buf, None, None, samples[s], n + rec.bytes, used.freq_limit,
                                     44100, used.samprate, rec.crc) == 1
        out = str(tmp_path / ("single%d.mp3" % s))
        run_cli([wavs[s], out, "-X2"])
        assert bytes(buf[:n]) + audio[s] == open(out, "rb").read(), "file %d (%d frames)" % (s, frames[s])
    L.hx_xing_destroy(x)


# ---- kinds of batch ----
def run_files(r, ncalls, call, fpc=1):
    """files of ncalls[s] calls through r in calls of `call` frames under counts, until all have ended"""
    r.begin(list(range(r.S)), ncalls, fpc=fpc)
    while True:
        counts = [0 if r.want[s].ended else max(0, min(call, ncalls[s] + DRAIN - r.given[s])) for s in range(r.S)]
        if not any(counts):
            break
        r.step(counts)
    assert all(w.ended for w in r.want) and len(r.ends) == r.S
    r.close()


def test_mpeg2_batch():
    """22.05 kHz: two frames per call, the drain ends when the frame counter reaches 2 x ncalls"""
    ncalls = [3, 10, 17]
    full = [synth.stream_pcm(6400 + i, nc, sr=22050, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Run(lambda: api.Batch(api.default_control(samprate=22050), nstreams=3, max_frames=8), full)
    run_files(r, ncalls, 8, fpc=2)
    assert all(w.frames_per_call == 2 and w.frames >= 2 * nc for w, nc in zip(r.want, ncalls))


def test_mono_batch():
    """... with the frame-counter buffers 4 bytes past an 8-byte boundary: k_ledger reads the pairs in halves"""
    ncalls = [2, 9, 16, 21]
    full = [synth.stream_pcm(6500 + i, nc, bursts=True)[:, :1].astype(np.float32) for i, nc in enumerate(ncalls)]
    run_files(Run(lambda: api.Batch(api.default_control(mode=3), nstreams=4, max_frames=16), full, odd=True), ncalls, 16)


def test_converting_batch_through_the_host_call():
    """48 kHz 24-bit sources encoded at 44.1 kHz through hx_batch_encode_src_counts_host with stats and crc: files of 5, 9 and
    14 converter calls, whose drain calls read a region of zero bytes through frame_off"""
    A = api
    streams = [Stream(48000, 24, 0, mpeg_select=44100, seed=95 + i, seconds=0.6) for i in range(3)]
    S, nf, ncalls = 3, 8, [5, 9, 14]
    b, t = make_batch(streams, nf), make_batch(streams, nf)
    b.ledger_begin(list(range(S)), ncalls)
    want = [A.ledger_open(nc) for nc in ncalls]
    row_data, zero = b.in_stride(nf), b.in_stride(1)
    pos, given, ended_in = [0] * S, [0] * S, 0
    while True:
        counts = [0 if want[s].ended else max(0, min(nf, ncalls[s] + DRAIN - given[s])) for s in range(S)]
        if not any(counts):
            break
        rows_in = np.zeros((S, row_data + zero), np.uint8)
        off = np.full((S, nf), row_data, np.int64)
        for s in range(S):
            chunk = np.frombuffer(streams[s].data[pos[s]:pos[s] + row_data], np.uint8)
            rows_in[s, :len(chunk)] = chunk
            take = max(0, min(counts[s], ncalls[s] - given[s]))         # calls on the file's input; the rest read zeros
            if take:
                nb_in, _ = b.schedule(s, take)
                off[s, :take] = np.concatenate([[0], np.cumsum(nb_in)[:-1]])
                pos[s] += int(nb_in.sum())
        res, used, st, cr = b.encode_src_counts_host(rows_in, nf, counts, frame_off=off, stats=True, crc=True)
        tres, tused, tst, tcr = t.encode_src_counts_host(rows_in, nf, counts, frame_off=off, stats=True, crc=True)
        assert res == tres and (st == tst).all() and (cr == tcr).all() and used.tolist() == tused.tolist()
        for s in range(S):
            ended_in += A.ledger_update(want[s], st[s, :counts[s]], cr[s, :counts[s]], len(res[s]))
            given[s] += counts[s]
        got = b.ledger_read(list(range(S)))
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    assert ended_in == S and all(w.ended and w.bytes > 0 for w in want)
    assert b.status() == 0 and t.status() == 0
    b.close()
    t.close()


def test_multi_on_one_device():
    """hx_multi_ledger_begin / _read over three blocks of device 0 (4 streams: uneven blocks), host calls with stats and crc
    under hx_multi_frame_counts; a slot listed twice or out of range is refused for all blocks"""
    A = api
    ncalls, nf = [3, 8, 13, 6], 8
    full = [synth.stream_pcm(6600 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    ec = A.default_control(bitrate=64)
    m, t = (A.Multi(ec, nstreams=4, max_frames=nf, devices=[0, 0, 0]) for _ in range(2))
    order = [2, 0, 3, 1]
    with pytest.raises(RuntimeError, match="listed twice"):
        m.ledger_begin([0, 3, 0], 5)
    with pytest.raises(RuntimeError, match="out of range"):
        m.ledger_begin([0, 4], 5)
    with pytest.raises(RuntimeError, match="ncalls < 1"):
        m.ledger_begin([0, 3], [5, 0])
    assert [g.tobytes() for g in m.ledger_read(order)] == [bytes(C.sizeof(A.Ledger))] * 4
    m.ledger_begin(order, [ncalls[s] for s in order])
    want = [A.ledger_open(nc) for nc in ncalls]
    given = [0] * 4
    while True:
        counts = [0 if want[s].ended else max(0, min(nf, ncalls[s] + DRAIN - given[s])) for s in range(4)]
        if not any(counts):
            break
        blk = block(full, given, counts, nf)
        m.frame_counts(counts)
        t.frame_counts(counts)
        res, st, cr = m.encode_host(blk, stats=True, crc=True)
        tres, tst, tcr = t.encode_host(blk, stats=True, crc=True)
        assert res == tres and (st == tst).all() and (cr == tcr).all()
        for s in range(4):
            A.ledger_update(want[s], st[s, :counts[s]], cr[s, :counts[s]], len(res[s]))
            given[s] += counts[s]
        got = m.ledger_read(order)
        assert [g.tobytes() for g in got] == [want[s].tobytes() for s in order]
    assert all(w.ended for w in want) and m.status() == 0 and t.status() == 0
    m.close()
    t.close()


def small_plain_with_restart():
    """the small shape by plain calls, with slot RESTART (its file of 7 calls ended in call 0) given a new file of 6 calls -
    hx_batch_ledger_begin + hx_batch_reset_streams - between calls 2 and 3 -> the records after the last call"""
    r = Run(small_batch, small_pcm())
    begun = [s for s in range(r.S) if s != NEVER]
    ncalls = list(SMALL_NCALLS)
    r.begin(begun, [ncalls[s] for s in begun])
    while True:
        if r.calls == 3:
            assert r.want[RESTART].ended
            r.begin([RESTART], 6)
            r.b.reset_streams([RESTART], stream=cur_stream())
            r.t.reset_streams([RESTART], stream=cur_stream())
            ncalls[RESTART], r.given[RESTART], r.full[RESTART] = 6, 0, small_restart_pcm()
        counts = small_counts(r.given, ncalls, r.calls)
        if not any(counts):
            break
        r.step(counts)
    final = r.records()
    assert r.want[RESTART].ended and r.want[RESTART].ncalls == 6 and len(r.ends) == len(begun) + 1
    r.close()
    return final


def test_pipelined_submits_advance_the_records_in_call_order():
    """the small shape through hx_batch_submit_f32_device with two sets of row / counter / CRC buffers in turn and no wait
    between submits, one hx_batch_ledger_begin + hx_batch_reset_streams between two submits for a slot whose file has ended:
    the records after hx_batch_wait equal the plain-call run's"""
    import torch
    want = small_plain_with_restart()
    b, full = small_batch(), small_pcm()
    begun = [s for s in range(b.n) if s != NEVER]
    ncalls, given = list(SMALL_NCALLS), [0] * b.n
    b.ledger_begin(begun, [ncalls[s] for s in begun], stream=cur_stream())
    sets, keep, call = [ledger_bufs(b, 8), ledger_bufs(b, 8)], [], 0
    while True:
        if call == 3:
            b.ledger_begin([RESTART], 6, stream=cur_stream())
            b.reset_streams([RESTART], stream=cur_stream())
            ncalls[RESTART], given[RESTART], full[RESTART] = 6, 0, small_restart_pcm()
        counts = small_counts(given, ncalls, call)
        if not any(counts):
            break
        keep.append(torch.from_numpy(block(full, given, counts, 8)).to(dev()))
        sync()          # (the upload is done; the previous submit's packing is still deferred - it goes out with the next submit)
        o = sets[call & 1]
        o.set_on(b)
        b.frame_counts(counts)
        b.submit_device(keep[-1].data_ptr(), 8, o.ptr, o.stride, o.nb.data_ptr(), cur_stream(), f32=True)
        given = [g + c for g, c in zip(given, counts)]
        call += 1
    b.wait(cur_stream())
    sync()
    got = [r.tobytes() for r in b.ledger_read(list(range(b.n)))]
    assert b.status() == 0
    b.close()
    for s in range(len(got)):
        assert got[s] == want[s], "slot %d" % s


def test_refusals_leave_batch_and_records_as_they_were():
    """a call that feeds an open record without a CRC buffer or without counters, ncalls = 0, a slot listed twice or out of
    range, a misaligned d_out: each -1 with a message before anything runs, the records unchanged, and the next well-formed
    call correct.  A call that feeds no live record needs neither buffer, and a batch that never began a ledger takes calls
    without counters as before"""
    import torch
    A, L = api, api.lib()
    ncalls = [4, 11, 6]
    full = [synth.stream_pcm(6700 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Run(lambda: A.Batch(A.default_control(bitrate=64), nstreams=3, max_frames=8), full)
    o = ledger_bufs(r.t, 8)
    d_pcm = torch.from_numpy(block(full, [0] * 3, [8] * 3, 8)).to(dev())
    sync()
    o.set_on(r.t, stats=False, crc=False)       # (the twin never begins a ledger: no counters needed)
    r.t.encode_device(d_pcm.data_ptr(), 8, o.ptr, o.stride, o.nb.data_ptr(), cur_stream(), f32=True)
    sync()
    r.t.reset_streams([0, 1, 2], stream=cur_stream())
    r.begin([0, 1], ncalls[:2])
    r.step([8, 8, 8])
    before = r.records()
    o = ledger_bufs(r.b, 8)
    for stats, crc in ((True, False), (False, False)):
        o.set_on(r.b, stats, crc)
        r.b.frame_counts(None)
        for fn in (L.hx_batch_encode_f32_device, L.hx_batch_submit_f32_device):
            assert fn(r.b.h, d_pcm.data_ptr(), 8, o.ptr, o.stride, o.nb.data_ptr(), cur_stream()) == -1
            assert "ledger record" in A.last_error() and "stream 1" in A.last_error()
    blk = np.zeros((3, 8 * 1152, 2), np.float32)
    out, nb = np.zeros((3, r.b.out_stride(8)), np.uint8), np.zeros(3, np.int32)
    assert L.hx_batch_encode_f32_host(r.b.h, blk.ctypes.data, 8, out.ctypes.data, out.shape[1], nb.ctypes.data) == -1 and "ledger record" in A.last_error()
    for idx, nc, what in (([0, 2], [5, 0], "ncalls < 1"), ([2, 0, 2], 5, "listed twice"), ([0, 3], 5, "out of range"), ([-1], 5, "out of range")):
        with pytest.raises(RuntimeError, match=what):
            r.b.ledger_begin(idx, nc)
    with pytest.raises(RuntimeError, match="head_bytes < 0"):
        r.b.ledger_begin([2], 5, head_bytes=-1)
    d_out = torch.zeros(3 * C.sizeof(A.Ledger) + 32, dtype=torch.uint8, device=dev())
    base = d_out.data_ptr() + (-d_out.data_ptr()) % 16
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        r.b.ledger_read_device([0, 1, 2], base + 8, stream=cur_stream())
    with pytest.raises(RuntimeError, match="listed twice"):
        r.b.ledger_read([1, 1])
    sync()
    assert r.b.status() == 0 and (o.rows()[1] == -1).all() and r.records() == before
    r.b.ledger_read_device([2, 0, 1], base, stream=cur_stream())
    sync()
    img = d_out.cpu().numpy()[base - d_out.data_ptr():][:3 * C.sizeof(A.Ledger)].tobytes()
    assert img == before[2] + before[0] + before[1]
    # slot 0's file (4 calls) has ended and a read has shown it: a call that feeds slots 0 and 2 only needs no counters
    assert r.want[0].ended and not r.want[1].ended
    o.set_on(r.b, False, False)
    r.b.frame_counts([8, 0, 8])
    r.b.encode_device(d_pcm.data_ptr(), 8, o.ptr, o.stride, o.nb.data_ptr(), cur_stream(), f32=True)
    sync()
    o2 = ledger_bufs(r.t, 8)
    o2.set_on(r.t, False, False)
    r.t.frame_counts([8, 0, 8])
    r.t.encode_device(d_pcm.data_ptr(), 8, o2.ptr, o2.stride, o2.nb.data_ptr(), cur_stream(), f32=True)
    sync()
    after = r.records()
    frozen = A.Ledger.from_buffer_copy(before[0])
    frozen.call_bytes = 0
    assert after == [frozen.tobytes(), before[1], before[2]]
    r.want[0].call_bytes = 0
    r.given[0] += 8
    r.given[2] += 8
    while not r.want[1].ended:
        r.step([0, 8, 0])
    r.close()
