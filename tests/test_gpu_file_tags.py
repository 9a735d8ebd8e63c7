"""The tag frame of a finished file built on a real MI355X (include/hmp3_amd.h, "finished files"; k_file_tag in
hmp3_amd/csrc/hx_fileimg.hip): hx_batch_file_tags writes into the head room of a slot's file image exactly the bytes
hx_file_tag_build gives for the slot's record - the project's own host function, which tests/test_file_tags_abi.py holds to the
three hx_xing_* calls.  Every comparison is byte equality.

One hx_batch_create_any batch of seven slots (tests/file_tag_cases.py) is run once, in calls of 8 frames under per-stream
counts through the host calls that bring nothing down; the tags are built in the middle of the run and after its end, and the
tests share the ended batch.  Around every hx_batch_file_tags call the images, the length words and the records are read
whole: the listed heads are the host function's, everything else is bit-identical.  Nothing here depends on the build of the
rate-loop kernel: the tests run once (one_k6_build)."""
import ctypes as C

import numpy as np
import pytest

import file_tag_cases as K
from file_image_cases import PAT, rows_block
from file_image_support import Files, file_bufs, image_of, prefill
from gpu_support import cur_stream, hip, sync
from hmp3_amd import api, synth

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
CAP = 112004            # slot LONG's file is about 99 000 bytes; not a multiple of 16: the pitch is larger
S = len(K.SLOTS)


def heads():
    return [K.slot_head(api, s) for s in range(S)]


def snapshot(b):
    """(every slot's image, the briefs - with them the length words - and the records)"""
    return [image_of(b, s) for s in range(b.n)], [p.tobytes() for p in b.ledger_poll()], b.ledger_read(list(range(b.n)))


def tags_checked(b, idx, tags, head, what):
    """hx_batch_file_tags on the list, the state read whole before and behind it: the listed heads equal hx_file_tag_build of
    the slot's record, and nothing else has changed -> the heads of all slots"""
    img0, polls0, recs0 = snapshot(b)
    b.file_tags(idx, tags, stream=cur_stream())
    sync()
    img1, polls1, recs1 = snapshot(b)
    assert polls1 == polls0 and [r.tobytes() for r in recs1] == [r.tobytes() for r in recs0], what + ": a record or a length word changed"
    for s in range(b.n):
        h = head[s]
        assert (img1[s][h:] == img0[s][h:]).all(), "%s: slot %d: a byte at or beyond head_bytes %d changed" % (what, s, h)
        if s in idx:
            want = api.file_tag_build(recs0[s], tags[idx.index(s)])
            assert len(want) == h, "%s: slot %d: the host builds %d bytes for a head of %d" % (what, s, len(want), h)
            bad = np.flatnonzero(img1[s][:h] != np.frombuffer(want, np.uint8))
            assert not len(bad), "%s: slot %d: the head differs from hx_file_tag_build at byte %d of %d (%d differ)" % (what, s, bad[0], h, len(bad))
        else:
            assert (img1[s][:h] == img0[s][:h]).all(), "%s: the head of slot %d, which was not listed, changed" % (what, s)
    return [img1[s][:head[s]].tobytes() for s in range(b.n)]


class Shape:
    """the seven-slot batch, run to the end; what was seen on the way"""

    def __init__(self):
        A = api
        self.head = heads()
        self.b = A.Batch.any([K.control_of(A, s) for s in range(S)], S, cfg=list(range(S)), max_frames=K.CALL)
        b = self.b
        assert [b.stream_frames_per_block(s) for s in range(S)] == [1, 1, 1, 2, 2, 1, 1] and [b.stream_channels(s) for s in range(S)] == [c["ch"] for c in K.SLOTS]
        b.file_images(CAP)
        prefill(b)
        b.ledger_begin(list(range(S)), [c["ncalls"] for c in K.SLOTS], self.head, [K.slot_flags(s) for s in range(S)], stream=cur_stream())
        full = [K.slot_pcm(synth, s) for s in range(S)]
        given, call, P = [0] * S, 0, b.pcm_channels()
        self.true_tags = [K.slot_tag(A, s) for s in range(S)]
        self.mid = None
        while True:
            counts = K.counts_at(given)
            if not any(counts):
                break
            b.frame_counts(counts)
            assert b.encode_host_files(rows_block(full, given, counts, K.CALL, P, np.float32)) == 0
            given = [g + n for g, n in zip(given, counts)]
            if call == K.MID_CALL:
                self.mid_run()
            call += 1
        self.calls = call
        self.recs = b.ledger_read(list(range(S)))

    def mid_run(self):
        """live records: first two slots alone - the other heads still hold the pattern - then all"""
        b = self.b
        recs = b.ledger_read(list(range(S)))
        live = [s for s in range(S) if not recs[s].ended]
        assert len(live) >= 3 and K.LONG in live and any(r.ended for r in recs)
        two = [K.LONG, 1]
        got = tags_checked(b, two, [self.true_tags[s] for s in two], self.head, "mid-run, two slots")
        for s in range(S):
            if s not in two:
                assert got[s] == bytes([PAT]) * self.head[s], "slot %d's head no longer holds the pattern" % s
        got = tags_checked(b, list(range(S)), self.true_tags, self.head, "mid-run, all slots")
        self.mid = dict(live=live, heads=got, frames=[r.frames for r in recs])


@pytest.fixture(scope="module")
def shape():
    sh = Shape()
    yield sh
    assert sh.b.status() == 0
    sh.b.close()


def test_tags_of_live_and_ended_records(shape):
    """mid-run (checked inside the run: Shape.mid_run) and after the end: each head equals hx_file_tag_build of the record read
    at that moment; the long file's table has halved, the CBR file below 64 kbit/s holds points but its frame no TOC, the
    untagged slot has no head and nothing written"""
    A = api
    assert shape.mid and len(shape.mid["live"]) >= 3
    assert all(r.ended for r in shape.recs) and shape.recs[K.LONG].every == 2 and shape.recs[K.LONG].npt >= 256
    assert shape.recs[K.COUNTS_ONLY].npt == 0 and shape.recs[K.NO_TOC_CBR].npt > 0 and shape.head[K.UNTAGGED] == 0
    end = tags_checked(shape.b, list(range(S)), shape.true_tags, shape.head, "after the end")
    for s in shape.mid["live"]:
        assert end[s] != shape.mid["heads"][s], "slot %d: the tag of the live record equals the finished file's" % s
    side = 17
    assert end[K.NO_TOC_CBR][4 + side:4 + side + 4] == b"Info" and end[K.NO_TOC_CBR][4 + side + 7] & 4 == 0
    assert end[0][4 + 32:4 + 32 + 4] == b"Xing" and end[0][4 + 32 + 7] & 4 and b"LAMEH5.24" in end[0]
    assert b"LAME" not in end[K.COUNTS_ONLY] and end[K.UNTAGGED] == b""
    assert any(end[K.LONG][4 + 17 + 16:4 + 17 + 116]) and end[K.LONG] == A.file_tag_build(shape.recs[K.LONG], shape.true_tags[K.LONG])


def test_parameter_grid_rebuilds_the_whole_head(shape):
    """on the ended records: samples_audio in {0, 1, true, true + 10 x 1152} x in_samplerate in {0, 44100, 48000, 96000,
    samprate / 2} - both sides of the trimming compare, the wrapped one included (tests/file_tag_cases.py), the LAME fields
    skipped for 0 - each call the whole head rebuilt: a head built with other parameters leaves no byte behind (the file
    with counts only has no LAME fields, but its frame count is trimmed all the same)"""
    A = api
    grids = [K.grid(A, s) for s in range(S)]
    seen = [set() for _ in range(S)]
    for g in range(len(grids[0])):
        tags = [grids[s][g] for s in range(S)]
        got = tags_checked(shape.b, list(range(S)), tags, shape.head, "grid %d" % g)
        for s in range(S):
            seen[s].add(got[s])
    assert len(seen[0]) >= 8 and len(seen[K.LONG]) >= 8 and len(seen[K.COUNTS_ONLY]) >= 2 and seen[K.UNTAGGED] == {b""}


def test_one_slot_lists_and_the_all_slots_list_give_the_same_heads(shape):
    A = api
    every = tags_checked(shape.b, list(range(S)), shape.true_tags, shape.head, "all slots")
    other = [K.slot_tag(A, s, 1, 48000) for s in range(S)]
    scrambled = tags_checked(shape.b, list(range(S)), other, shape.head, "other parameters")
    assert scrambled[0] != every[0]
    for s in reversed(range(S)):
        got = tags_checked(shape.b, [s], [shape.true_tags[s]], shape.head, "slot %d alone" % s)
        assert got[s] == every[s]
    assert [image_of(shape.b, s)[:shape.head[s]].tobytes() for s in range(S)] == every
    assert shape.b.file_tags([], []) is None        # (n = 0: nothing launched)


def test_refusals_leave_batch_and_images_as_they_were(shape):
    """a tag of another size than the slot's head room, a duplicate, an index out of range, a null tag array, a call under
    stream capture - on the shared batch, whose images, length words and records stay bit-identical; images off and a slot
    never begun (or begun before the images were switched on) on batches of their own"""
    import torch
    A, L, b = api, api.lib(), shape.b
    img0, polls0, recs0 = snapshot(b)
    with pytest.raises(RuntimeError, match=r"entry 1: the tag frame takes \d+ bytes, slot 1's record was begun with head_bytes \d+"):
        b.file_tags([0, 1], [shape.true_tags[0], shape.true_tags[0]])
    with pytest.raises(RuntimeError, match="entry 0: the tag frame takes 0 bytes"):
        b.file_tags([3], [A.FileTag()])
    with pytest.raises(RuntimeError, match="entry 1: slot 2 is listed twice"):
        b.file_tags([2, 2], [shape.true_tags[2]] * 2)
    with pytest.raises(RuntimeError, match="entry 0: slot 7 out of range"):
        b.file_tags([S], [shape.true_tags[0]])
    idx = (C.c_int * 1)(0)
    assert L.hx_batch_file_tags(b.h, idx, None, 1, None) == -1 and "tags is null" in A.last_error()
    assert L.hx_batch_file_tags(b.h, None, None, 1, None) == -1 and L.hx_batch_file_tags(b.h, idx, None, -1, None) == -1
    # under stream capture
    h = hip()
    h.hipStreamBeginCapture.argtypes, h.hipStreamEndCapture.argtypes, h.hipGraphDestroy.argtypes = [C.c_void_p, C.c_int], [C.c_void_p, C.c_void_p], [C.c_void_p]
    q = torch.cuda.Stream()
    tag = (A.FileTag * 1)(shape.true_tags[0])
    assert h.hipStreamBeginCapture(q.cuda_stream, 2) == 0          # (2: relaxed - other threads' and unrelated calls stay legal)
    rc, why = L.hx_batch_file_tags(b.h, idx, tag, 1, q.cuda_stream), A.last_error()
    graph = C.c_void_p()
    assert h.hipStreamEndCapture(q.cuda_stream, C.byref(graph)) == 0
    if graph.value:
        h.hipGraphDestroy(graph)
    assert rc == -1 and "not made under stream capture" in why
    sync()
    img1, polls1, recs1 = snapshot(b)
    assert polls1 == polls0 and [r.tobytes() for r in recs1] == [r.tobytes() for r in recs0] and all((x == y).all() for x, y in zip(img0, img1))
    assert b.status() == 0
    tags_checked(b, [0], [shape.true_tags[0]], shape.head, "behind the refusals")
    # images off; a slot never begun; a slot begun before the images were on
    t0, size = shape.true_tags[0], shape.head[0]
    p = A.Batch(A.default_control(), nstreams=3, max_frames=8)
    p.ledger_begin([0], [4], [size], [1])
    with pytest.raises(RuntimeError, match="file images are off"):
        p.file_tags([0], [t0])
    assert p.ledger_poll()[0].open == 1
    p.ledger_read([0])
    # (the record is live: images cannot be switched on under it - a batch of its own for the rest)
    p.close()
    p = A.Batch(A.default_control(), nstreams=3, max_frames=8)
    p.file_images(4096)
    prefill(p)
    p.ledger_begin([0], [4], [size], [1], stream=cur_stream())
    with pytest.raises(RuntimeError, match="entry 1: slot 1's record was not begun with an image"):
        p.file_tags([0, 1], [t0, t0])
    sync()
    assert all((image_of(p, s) == PAT).all() for s in range(3))
    p.file_tags([0], [t0], stream=cur_stream())
    sync()
    assert image_of(p, 0)[:size].tobytes() == A.file_tag_build(p.ledger_read([0])[0], t0) and (image_of(p, 0)[size:] == PAT).all()
    assert p.status() == 0
    p.close()


def test_behind_a_pipelined_submit_the_tag_reflects_that_submits_update():
    """two hx_batch_submit_f32_device calls, no wait, then hx_batch_file_tags on the same stream: the deferred packing - and
    the ledger update that travels with it - goes out first, so the head is the tag of the record behind both submits"""
    A = api
    ncalls = [30, 25]
    full = [synth.stream_pcm(9200 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    tags = [K.tag_of(A, A.default_control(), 2, 3, nc * 1152 - K.TAIL) for nc in ncalls]
    size = A.file_tag_bytes(tags[0])
    r = Files(lambda: A.Batch(A.default_control(), nstreams=2, max_frames=8), full, 20000)
    r.begin([0, 1], ncalls, [size, size])
    sets, keep = [file_bufs(r.b, 8), file_bufs(r.b, 8, shift=7)], []
    for c in range(2):
        feed = lambda blk, counts, nf: keep.append(r.device_call(r.b, blk, counts, nf, submit=True, out=sets[c & 1])) and None
        r.step([8, 8], nf=8, feed=feed, check=False)
    r.b.file_tags([0, 1], tags, stream=cur_stream())
    r.b.wait(cur_stream())
    sync()
    recs = r.b.ledger_read([0, 1])
    for s in range(2):
        assert recs[s].tobytes() == r.want[s].tobytes() and recs[s].fed == 16 and recs[s].frames > 8
        want = A.file_tag_build(recs[s], tags[s])
        assert len(want) == size and image_of(r.b, s)[:size].tobytes() == want, "slot %d: the head is not the tag of the record behind the submits" % s
        r.model[s][:size] = np.frombuffer(want, np.uint8)
    r.check("behind the tags")
    r.close()
