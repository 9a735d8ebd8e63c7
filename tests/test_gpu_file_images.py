"""File images on a real MI355X (include/hmp3_amd.h, "file images"; k_file_append / k_ledger_brief in
hmp3_amd/csrc/hx_fileimg.hip): behind every call's ledger update the bytes the ledger gave to a file are put behind the
file's bytes so far in the slot's image on the GPU, and the host fetches a file once.

Every comparison is byte equality.  The expected image is built on the host from a twin batch without images that takes the
same calls through plain device calls: per slot a model of the whole image, cap bytes of a guard pattern, into which the
model writes rows[s, :call_bytes] at head_bytes + the file's bytes so far, call_bytes from hx_ledger_update
(tests/test_ledger_host.py pins that function).  The device image is pre-filled with the same pattern through
hx_batch_file_image_ptr, so after every call image == model says at once that the file's bytes are there and that no byte in
front of head_bytes, behind the file's end or at or beyond cap has changed (a restarted slot keeps the old file's bytes
behind the new one's end: the model does too).  The twin's rows, counts, counters, CRCs and records must equal the image
batch's.  Nothing here depends on the build of the rate-loop kernel: the tests run once (one_k6_build)."""
import numpy as np
import pytest

import file_image_cases as K
from file_image_cases import CHUNK, PAT
from file_image_support import Files, file_bufs, image_of, prefill, vbr_small
from gpu_support import cur_stream, dev, sync
from hmp3_amd import api, synth
from ledger_cases import DRAIN, small_pcm, small_restart_pcm
from src_cases import Stream, make_batch

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]


# ---- 1: the small shape ----
def test_small_shape():
    """the ledger test's small shape (tests/file_image_cases.py), VBR: every slot its own head_bytes; slot NEVER never begun,
    slot SITS_OUT sits call 1 out, slot ONE_FRAME takes one frame of call 0 (a fed live stream with a piece of 0 bytes), slot
    RESTART gets a second file between calls 2 and 3 - its length returns to 0 and the new file overwrites from its head, the
    old file's bytes staying behind it.  Ended files' images stay as they are through the later calls of silence.
    Nine slots cannot hold sixteen different head_bytes: the heads are chosen so that the shape's 17 pieces start at 14 of the
    16 residues mod 16 (asserted here, and predicted on the CPU by tests/test_file_images_abi.py); that pieces start at all
    16 is asserted where there are pieces enough, in test_small_pieces"""
    r = Files(vbr_small, small_pcm(), 9000)
    ended_image = {}
    for step in K.schedule():
        if step[0] == "begin":
            r.begin(*step[1:])
        elif step[0] == "restart":
            s = step[1]
            assert r.want[s].ended and r.length[s] > 0
            old = r.model[s].copy()
            r.begin([s], [K.RESTART_NCALLS], [K.RESTART_HEAD])
            for h in (r.b, r.t):
                h.reset_streams([s], stream=cur_stream())
            r.full[s], r.given[s] = small_restart_pcm(), 0
            r.check("restart")
            assert r.b.ledger_poll()[s].image_bytes == 0 and (image_of(r.b, s) == old).all()
            ended_image.pop(s, None)
        else:
            r.step(step[1], nf=8)
            for s in range(r.S):
                if r.want[s].ended:
                    img = image_of(r.b, s).tobytes()
                    assert ended_image.setdefault(s, img) == img, "slot %d's image changed after its file's end" % s
    p = r.pieces
    assert any(q["live"] and 0 < q["cb"] < q["nb"] for q in p), "no file ends inside a call's bytes"
    assert any(q["live"] and q["cb"] == 0 for q in p), "no fed live stream had a piece of 0 bytes"
    assert len({q["at"] % 16 for q in p if q["cb"]}) >= 14      # (17 pieces; all 16 residues: test_small_pieces)
    assert not any(q["s"] == K.NEVER for q in p) and (r.model[K.NEVER] == PAT).all()
    assert all(r.want[s].ended for s in range(r.S) if s != K.NEVER) and len(ended_image) == r.S - 1
    assert (r.model[K.RESTART][K.RESTART_HEAD:K.RESTART_HEAD + r.length[K.RESTART]] != PAT).any()
    r.close()


# ---- 2: misaligned rows ----
@pytest.mark.parametrize("shift,extra", [(1, 0), (5, 3), (15, 1)])
def test_misaligned_rows(shift, extra):
    """d_out 1, 5 and 15 bytes past a 16-byte boundary, and an odd out_stride: the rows start at every misalignment"""
    ncalls = [2, 5, 9, 3]
    full = [synth.stream_pcm(7100 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Files(lambda: api.Batch(api.default_control(), nstreams=4, max_frames=4), full, 6000, shift=shift, extra=extra)
    r.begin([0, 1, 2, 3], ncalls, [3, 0, 8, 13])
    r.run(ncalls, 4)
    assert sum(q["cb"] > 0 for q in r.pieces) >= 5 and {q["at"] % 16 for q in r.pieces if q["cb"]} > {0} and all(w.ended for w in r.want)
    r.close()


# ---- 3: small pieces ----
def test_small_pieces():
    """calls of one frame: pieces of 0 bytes and of a few hundred, most vectors partial; the pieces start at every residue"""
    ncalls = [30, 34, 38]
    full = [synth.stream_pcm(7200 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Files(lambda: api.Batch(api.default_control(), nstreams=3, max_frames=1), full, 16000)
    r.begin([0, 1, 2], ncalls, [7, 0, 2])
    while not all(w.ended for w in r.want):
        r.step([1, 1, 1], check=r.calls % 8 == 0)
    r.check("end")
    sizes = [q["cb"] for q in r.pieces if q["live"]]
    assert 0 in sizes and max(sizes) < 1500 and {q["at"] % 16 for q in r.pieces if q["cb"]} == set(range(16))
    r.close()


# ---- 4: chunk edges ----
def test_chunk_edges():
    """one stream at 320 kbit/s in calls of so many frames that a piece spans three of the kernel's chunks, starting off a
    16-byte boundary: the second call's piece starts wherever the first one's ended"""
    nf = 2 * CHUNK // 1044 + 2
    full = [synth.stream_pcm(7300, 2 * nf, bursts=True).astype(np.float32)]
    r = Files(lambda: api.Batch(api.default_control(bitrate=160), nstreams=1, max_frames=nf), full, 3 * nf * 1100)
    r.begin([0], [2 * nf], [5])
    r.run([2 * nf], nf)
    big = [q for q in r.pieces if q["cb"] + q["at"] % 16 > 2 * CHUNK]
    assert len(big) >= 2 and big[0]["at"] == 5 and r.want[0].ended
    r.close()


# ---- 5: overflow ----
def test_overflow():
    """cap such that slot 1's file overflows in the middle of a call: nothing at or beyond cap changes (the model is cap bytes;
    a guard behind every image is checked by the neighbours' models and, for the last, by the allocation's rounding to 16),
    image_bytes stops at cap - head, status bit 64 is set, the other slots' files are complete, and the batch stays usable:
    slot 1 gets a shorter file that fits"""
    ncalls, heads = [4, 11, 6], [9, 6, 0]
    full = [synth.stream_pcm(7400 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    make = lambda: api.Batch(api.default_control(), nstreams=3, max_frames=8)
    scout = Files(make, full, 20000)            # the same calls with room for everything: where slot 1's second piece lies
    scout.begin([0, 1, 2], ncalls, heads)
    scout.run(ncalls, 8, check=False)
    second = [q for q in scout.pieces if q["s"] == 1 and q["cb"]][1]
    cap = second["at"] + second["cb"] // 2 + 1
    scout.close()
    r = Files(make, full, cap)
    r.begin([0, 1, 2], ncalls, heads)
    r.run(ncalls, 8)
    cut = [q for q in r.pieces if q["cut"]]
    assert cut and all(q["s"] == 1 for q in cut) and cut[0]["at"] < cap < cut[0]["at"] + cut[0]["cb"], "the file does not overflow inside a call"
    assert r.length[1] == cap - heads[1] < r.want[1].bytes and r.b.ledger_poll()[1].image_bytes == cap - heads[1]
    assert all(r.length[s] == r.want[s].bytes for s in (0, 2)) and r.b.status() == 64
    assert r.b.file_fetch(1, cap, fill=1) == bytes([1]) * heads[1] + r.model[1][heads[1]:].tobytes()
    r.begin([1], [2], [3])
    for h in (r.b, r.t):
        h.reset_streams([1], stream=cur_stream())
    r.full[1], r.given[1] = synth.stream_pcm(7410, 2, bursts=True).astype(np.float32), 0
    r.run([0, 2, 0], 8)
    assert r.want[1].ended and r.length[1] == r.want[1].bytes > 0
    r.close(status=64)


# ---- 6: mixed kinds ----
def test_mixed_kinds():
    """a create_any batch: MPEG-1 stereo, MPEG-2 (two frames per block) and a mono entry, in rows pitched for two channels"""
    A = api
    menu = [dict(), dict(samprate=22050), dict(mode=3, samprate=48000)]
    ncalls = [6, 9, 4]
    full = [synth.stream_pcm(7500, 6, bursts=True), synth.stream_pcm(7501, 9, sr=22050, bursts=True), synth.stream_pcm(7502, 4, sr=48000, bursts=True)[:, :1]]
    full = [x.astype(np.float32) for x in full]
    r = Files(lambda: A.Batch.any([A.default_control(**kw) for kw in menu], 3, cfg=[0, 1, 2], max_frames=4), full, 8000)
    assert [r.t.stream_frames_per_block(s) for s in range(3)] == [1, 2, 1] and [r.t.stream_channels(s) for s in range(3)] == [2, 2, 1]
    r.begin([0, 1, 2], ncalls, [1, 14, 6])
    r.run(ncalls, 4)
    assert all(w.ended and w.bytes > 0 for w in r.want)
    r.close()


# ---- 7: pipelined submits ----
def test_pipelined_submits():
    """three hx_batch_submit_f32_device calls with two sets of buffers in turn, no wait between them, then hx_batch_wait: the
    images, lengths and records equal those of the twin's plain calls"""
    ncalls = [3, 40, 9, 14]
    full = [synth.stream_pcm(7600 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Files(lambda: api.Batch(api.default_control(), nstreams=4, max_frames=8), full, 12000)
    r.begin([0, 1, 2, 3], ncalls, [4, 11, 0, 15])
    sets, keep = [file_bufs(r.b, 8), file_bufs(r.b, 8, shift=7)], []
    for c in range(3):
        counts = [8, 8, 0 if c == 1 else 8, 5]
        feed = lambda blk, counts, nf: keep.append(r.device_call(r.b, blk, counts, nf, submit=True, out=sets[c & 1])) and None
        r.step(counts, nf=8, feed=feed, check=False)
    r.b.wait(cur_stream())
    sync()
    r.check("after the wait")
    assert r.want[0].ended and not r.want[1].ended and sum(q["cb"] > 0 for q in r.pieces) >= 8
    r.close()


# ---- 8: the host calls that bring nothing down ----
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_host_files_calls_under_counts_and_segments(f32):
    """hx_batch_encode_{s16,f32}_host_files under per-stream counts, every second call fed as one packed PCM image
    (hx_batch_pcm_segments): images, polls and fetches equal the device-call twin's; fetch leaves dst[0, head) untouched"""
    ncalls = [2, 7, 12, 5]
    full = [synth.stream_pcm(7700 + i, nc, bursts=True) for i, nc in enumerate(ncalls)]
    full = [x.astype(np.float32) if f32 else x.astype(np.int16) for x in full]
    r = Files(lambda: api.Batch(api.default_control(), nstreams=4, max_frames=8), full, 9000, f32=f32)
    r.begin([0, 1, 2, 3], ncalls, [2, 0, 13, 8])

    def feed(blk, counts, nf):
        r.b.frame_counts(counts)
        if r.calls & 1:
            off, total = r.b.packed_layout(nf, f32=f32)
            image = np.concatenate([blk[s, :counts[s] * 1152 * 2] for s in range(r.S)])
            assert image.nbytes == total
            r.b.pcm_segments(off, total)
            assert r.b.encode_host_files_image(image, nf) == 0
            r.b.pcm_segments(None)
        else:
            assert r.b.encode_host_files(blk) == 0
    call = 0
    while not all(w.ended for w in r.want):
        counts = [0 if r.want[s].ended else (3 if (s + call) % 3 == 0 else 8) for s in range(r.S)]
        r.step(counts, nf=8, feed=feed)
        call += 1
    assert r.calls >= 3
    r.close()


@pytest.mark.parametrize("multi", [False, True], ids=["batch", "multi"])
def test_converting_host_files_call(multi):
    """hx_batch_encode_src_files_host - and hx_multi_encode_src_files_host over two blocks of device 0, whose images are
    seen through the fetch - with counts and frame_off against hx_batch_encode_src_counts_host with stats and crc on a twin:
    48 kHz 24-bit sources encoded at 44.1 kHz, files of 5, 9 and 14 converter calls"""
    A = api
    streams = [Stream(48000, 24, 0, mpeg_select=44100, seed=95 + i, seconds=0.6) for i in range(3)]
    S, nf, ncalls, heads, cap = 3, 8, [5, 9, 14], [0, 7, 12], 12000
    t = make_batch(streams, nf)
    b = A.SrcMulti([s.ec for s in streams], [s.src for s in streams], max_frames=nf, devices=[0, 0]) if multi else make_batch(streams, nf)
    b.file_images(cap)
    if not multi:
        prefill(b)
    for h in (b, t):
        h.ledger_begin(list(range(S)), ncalls, heads)
    want = [A.ledger_open(nc, 1, h, 0) for nc, h in zip(ncalls, heads)]
    model = [np.full(cap, PAT, np.uint8) for _ in range(S)]
    row_data, zero = b.in_stride(nf), b.in_stride(1)
    pos, given = [0] * S, [0] * S
    while True:
        counts = [0 if want[s].ended else max(0, min(nf, ncalls[s] + DRAIN - given[s])) for s in range(S)]
        if not any(counts):
            break
        rows_in = np.zeros((S, row_data + zero), np.uint8)
        off = np.full((S, nf), row_data, np.int64)
        for s in range(S):
            chunk = np.frombuffer(streams[s].data[pos[s]:pos[s] + row_data], np.uint8)
            rows_in[s, :len(chunk)] = chunk
            take = max(0, min(counts[s], ncalls[s] - given[s]))
            if take:
                nb_in, _ = t.schedule(s, take)
                off[s, :take] = np.concatenate([[0], np.cumsum(nb_in)[:-1]])
                pos[s] += int(nb_in.sum())
        status, used = b.encode_src_files_host(rows_in, nf, counts, frame_off=off)
        tres, tused, tst, tcr = t.encode_src_counts_host(rows_in, nf, counts, frame_off=off, stats=True, crc=True)
        assert status == 0 and used.tolist() == tused.tolist()
        for s in range(S):
            A.ledger_update(want[s], tst[s, :counts[s]], tcr[s, :counts[s]], len(tres[s]))
            if counts[s]:
                at = heads[s] + want[s].bytes - want[s].call_bytes
                model[s][at:at + want[s].call_bytes] = np.frombuffer(tres[s][:want[s].call_bytes], np.uint8)
            given[s] += counts[s]
        polls, recs = b.ledger_poll(), t.ledger_read(list(range(S)))
        for s in range(S):
            assert recs[s].tobytes() == want[s].tobytes() and polls[s].tobytes() == A.ledger_brief(want[s], want[s].bytes).tobytes()
            if not multi:
                assert (image_of(b, s) == model[s]).all(), "slot %d's image" % s
            assert b.file_fetch(s, heads[s] + want[s].bytes, fill=9) == bytes([9]) * heads[s] + model[s][heads[s]:heads[s] + want[s].bytes].tobytes()
    assert all(w.ended and w.bytes > 0 for w in want) and b.status() == 0 and t.status() == 0
    for s in range(S):
        assert b.file_fetch(s, cap, fill=9) == bytes([9]) * heads[s] + model[s][heads[s]:heads[s] + want[s].bytes].tobytes()
    b.close()
    t.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_multi_in_two_blocks_on_one_device(f32):
    """hx_multi_file_images / _ledger_poll / _file_fetch / _encode_{s16,f32}_host_files over two blocks of device 0 (5
    streams: uneven blocks) under hx_multi_frame_counts, against a one-batch twin's device calls"""
    A = api
    ncalls, heads = [3, 8, 13, 6, 2], [5, 0, 9, 14, 3]
    full = [synth.stream_pcm(7800 + i, nc, bursts=True).astype(np.float32 if f32 else np.int16) for i, nc in enumerate(ncalls)]
    ec = A.default_control()
    r = Files(lambda: A.Batch(ec, nstreams=5, max_frames=8), full, 9000, f32=f32, make_b=lambda: A.Multi(ec, nstreams=5, max_frames=8, devices=[0, 0]))
    with pytest.raises(RuntimeError, match="out of range"):
        r.b.file_fetch(5, 100)
    r.begin(list(range(5)), ncalls, heads)
    with pytest.raises(RuntimeError, match="stream 0 has a live ledger record"):
        r.b.file_images(4000)

    def feed(blk, counts, nf):
        r.b.frame_counts(counts)
        assert r.b.encode_host_files(blk) == 0
    r.run(ncalls, 8, feed=feed, read=False)
    recs = r.b.ledger_read(list(range(5)))
    assert [x.tobytes() for x in recs] == [w.tobytes() for w in r.want] and all(w.ended for w in r.want)
    r.close()


# ---- 9: the poll ----
def test_poll_teaches_the_host_which_records_ended():
    """the poll equals hx_ledger_brief of the full read for every slot (Files.check, after every call of every test here); and
    like a read it tells the host that a record has ended: a call that feeds only that slot, without counters and CRCs, is
    refused before the poll and taken after it"""
    import torch
    A, L = api, api.lib()
    ncalls = [1, 12]
    full = [synth.stream_pcm(7900 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Files(lambda: A.Batch(A.default_control(), nstreams=2, max_frames=8), full, 9000)
    r.begin([0, 1], ncalls, [0, 0])
    r.step([8, 8], check=False)
    assert r.want[0].ended and not r.want[1].ended
    o = file_bufs(r.b, 8)
    o.set_on(r.b, stats=False, crc=False)
    r.b.frame_counts([8, 0])
    d_pcm = torch.zeros((2, 8 * 1152, 2), dtype=torch.float32, device=dev())
    sync()
    call = lambda: L.hx_batch_encode_f32_device(r.b.h, d_pcm.data_ptr(), 8, o.ptr, o.stride, o.nb.data_ptr(), cur_stream())
    assert call() == -1 and "stream 0 has an open ledger record" in A.last_error()
    polls = r.b.ledger_poll()
    assert polls[0].ended == 1 and polls[1].ended == 0
    assert call() == 0
    sync()
    assert r.t.ledger_read([0])[0].ended == 1
    # (the twin takes the same call, so that the two go on alike; slot 0's record is frozen but for call_bytes = 0)
    o2 = file_bufs(r.t, 8)
    o2.set_on(r.t, stats=False, crc=False)
    r.t.frame_counts([8, 0])
    assert L.hx_batch_encode_f32_device(r.t.h, d_pcm.data_ptr(), 8, o2.ptr, o2.stride, o2.nb.data_ptr(), cur_stream()) == 0
    sync()
    r.want[0].call_bytes = 0
    r.given[0] += 8
    r.check("after the call without counters")
    r.close()


# ---- 10: refusals ----
def test_refusals_leave_the_batch_as_it_was():
    """hx_batch_file_images while a record is live or with a negative cap; *_host_files without a ledger or without images; a
    fetch into too small a dst; a misaligned d_out for poll_device: each -1 with a message, images, lengths and records
    unchanged, and the next well-formed call correct"""
    import torch
    A, L = api, api.lib()
    ncalls = [4, 11]
    full = [synth.stream_pcm(8000 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    blk = np.zeros((2, 8 * 1152 * 2), np.float32)
    plain = A.Batch(A.default_control(), nstreams=2, max_frames=8)
    assert L.hx_batch_encode_f32_host_files(plain.h, blk.ctypes.data, 8) == -1 and "needs a file ledger" in A.last_error()
    plain.ledger_begin([0], [3])
    assert L.hx_batch_encode_f32_host_files(plain.h, blk.ctypes.data, 8) == -1 and "needs file images" in A.last_error()
    assert L.hx_batch_encode_s16_host_files(plain.h, blk.ctypes.data, 8) == -1 and "needs file images" in A.last_error()
    buf = np.zeros(64, np.uint8)
    assert L.hx_batch_file_fetch(plain.h, 0, buf.ctypes.data, 64) == -1 and "file images are off" in A.last_error()
    assert plain.file_image_cap() == 0 and plain.file_image_ptr(0) is None and plain.status() == 0
    plain.close()

    r = Files(lambda: A.Batch(A.default_control(), nstreams=2, max_frames=8), full, 7000)
    with pytest.raises(RuntimeError, match="cap < 0"):
        r.b.file_images(-1)
    r.begin([0, 1], ncalls, [6, 1])
    r.step([8, 8])
    before = [image_of(r.b, s).tobytes() for s in range(2)], [p.tobytes() for p in r.b.ledger_poll()]
    for cap in (0, 5000):
        with pytest.raises(RuntimeError, match="stream 1 has a live ledger record"):
            r.b.file_images(cap)
    assert r.b.file_image_cap() == 7000
    need = r.head[1] + r.length[1]
    small = np.full(need, 0x11, np.uint8)
    assert L.hx_batch_file_fetch(r.b.h, 1, small.ctypes.data, need - 1) == -1 and "do not fit dst_cap" in A.last_error() and (small == 0x11).all()
    assert L.hx_batch_file_fetch(r.b.h, 2, small.ctypes.data, need) == -1 and L.hx_batch_file_fetch(r.b.h, 1, None, need) == -1
    d_out = torch.zeros(2 * 32 + 32, dtype=torch.uint8, device=dev())
    base = d_out.data_ptr() + (-d_out.data_ptr()) % 16
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        r.b.ledger_poll_device(base + 8, stream=cur_stream())
    assert L.hx_batch_encode_f32_host_files(r.b.h, None, 8) == -1 and L.hx_batch_encode_f32_host_files(r.b.h, blk.ctypes.data, 9) == -1
    sync()
    assert ([image_of(r.b, s).tobytes() for s in range(2)], [p.tobytes() for p in r.b.ledger_poll()]) == before and r.b.status() == 0
    r.b.ledger_poll_device(base, stream=cur_stream())
    sync()
    assert d_out.cpu().numpy()[base - d_out.data_ptr():][:64].tobytes() == b"".join(before[1])
    r.run(ncalls, 8)
    assert all(w.ended for w in r.want)
    # between files the images may be switched: off, and on again with another cap - the records begun before have no image
    r.b.file_images(0)
    assert r.b.file_image_cap() == 0 and r.b.file_image_ptr(0) is None
    r.b.file_images(3000)
    assert r.b.file_image_cap() == 3000 and [p.image_bytes for p in r.b.ledger_poll()] == [0, 0]
    assert r.b.status() == 0 and r.t.status() == 0
    r.b.close()
    r.t.close()


def test_refused_allocation_leaves_the_batch_usable():
    """a cap the device cannot hold (2^45 bytes per slot: hipMalloc refuses it at once): -1, hx_batch_file_image_cap and
    hx_batch_file_image_ptr unchanged - on a batch that has images and on one that has none - status 0, and the next
    hx_batch_ledger_begin and the calls behind it run and fill the images that stood; the same for hx_multi_file_images in
    two blocks of device 0, which then takes images that fit, a begin and a call"""
    A, L = api, api.lib()
    HUGE = 1 << 45
    ncalls = [4, 7]
    full = [synth.stream_pcm(8100 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    make = lambda: A.Batch(A.default_control(), nstreams=2, max_frames=8)
    fresh = make()
    for cap in (HUGE, (1 << 63) - 1, (1 << 63) - 16):
        with pytest.raises(RuntimeError, match="do not fit"):
            fresh.file_images(cap)
        assert fresh.file_image_cap() == 0 and fresh.file_image_ptr(0) is None
    fresh.ledger_begin([0, 1], ncalls)            # (the launch behind a refused allocation: it must not find that error)
    assert fresh.status() == 0 and [p.open for p in fresh.ledger_poll()] == [1, 1]
    fresh.close()
    r = Files(make, full, 7000)
    ptrs = [r.b.file_image_ptr(s) for s in range(2)]
    with pytest.raises(RuntimeError, match="do not fit"):
        r.b.file_images(HUGE)
    assert r.b.file_image_cap() == 7000 and [r.b.file_image_ptr(s) for s in range(2)] == ptrs and r.b.status() == 0
    r.begin([0, 1], ncalls, [3, 10])
    r.run(ncalls, 8)
    assert all(w.ended and n > 0 for w, n in zip(r.want, r.length))
    r.close()
    r = Files(make, full, 7000, make_b=lambda: A.Multi(A.default_control(), nstreams=2, max_frames=8, devices=[0, 0]))
    with pytest.raises(RuntimeError, match="do not fit"):
        r.b.file_images(HUGE)
    assert [int(L.hx_batch_file_image_cap(r.b.batch(k))) for k in range(2)] == [7000, 7000]
    r.begin([0, 1], ncalls, [3, 10])

    def feed(blk, counts, nf):
        r.b.frame_counts(counts)
        assert r.b.encode_host_files(blk) == 0
    r.run(ncalls, 8, feed=feed)
    assert all(w.ended and n > 0 for w, n in zip(r.want, r.length))
    r.close()
