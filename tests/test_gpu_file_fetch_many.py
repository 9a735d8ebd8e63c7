"""Many finished files fetched at once on a real MI355X (include/hmp3_amd.h, "finished files"; k_file_off / k_file_gather in
hmp3_amd/csrc/hx_fileimg.hip): hx_batch_file_fetch_many and hx_batch_file_gather_device bring the images of any list of
slots together as one dense image - segment e the slot's head room and audio bytes, at the rounded sums, zeros between.

The reference is the project's own per-file fetch, hx_batch_file_fetch, which tests/test_gpu_file_images.py holds to the host's
model of the images; every comparison is byte equality.  The shapes are tests/file_image_cases.py's small one and, for the
kernel's chunk edges, test_chunk_edges' stream at 320 kbit/s.  The tests run once (one_k6_build)."""
import ctypes as C

import numpy as np
import pytest

import file_image_cases as K
import file_tag_cases as T
from file_image_cases import CHUNK, PAT, rows_block
from file_image_support import Files, file_bufs, image_of, prefill, vbr_small
from gpu_support import cur_stream, dev, sync
from hmp3_amd import api, synth
from ledger_cases import small_pcm, small_restart_pcm

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
SENT = 0x6B


def r16(n):
    return (n + 15) & ~15


def fetch_checked(b, idx, what, cap_extra=40):
    """fetch_many of the list against file_fetch of each slot, with the head room as the image holds it: the segments, the
    offsets as rounded sums, zero padding, the sentinel beyond off[n] -> the lengths"""
    want = []
    for s in idx:
        # (hx_batch_file_fetch leaves the head room to the caller: what differs between two fills is the head room, and there
        # the reference is the image itself)
        w, w2 = b.file_fetch(s, b.file_image_cap(), fill=PAT), b.file_fetch(s, b.file_image_cap(), fill=PAT ^ 0xFF)
        head = sum(x != y for x, y in zip(w, w2))
        assert w[head:] == w2[head:]
        want.append(image_of(b, s)[:head].tobytes() + w[head:])
    total = sum(r16(len(w)) for w in want)
    buf, off, r = b.file_fetch_many(idx, total + cap_extra, fill=SENT)
    assert r == total and off.tolist() == np.concatenate([[0], np.cumsum([r16(len(w)) for w in want])]).tolist(), what + ": the offsets"
    for e, s in enumerate(idx):
        seg = buf[off[e]:off[e + 1]]
        assert seg[:len(want[e])].tobytes() == want[e], "%s: segment %d (slot %d, %d bytes) differs from hx_batch_file_fetch" % (what, e, s, len(want[e]))
        assert not seg[len(want[e]):].any(), "%s: segment %d's padding is not zero" % (what, e)
    assert (buf[total:] == SENT).all(), what + ": a byte beyond off[n] was written"
    return [len(w) for w in want]


def run_small(upto=None):
    """the small shape of the file-image tests on a Files pair, to its end or until `upto` calls are made"""
    r = Files(vbr_small, small_pcm(), 9000)
    for step in K.schedule():
        if step[0] == "begin":
            r.begin(*step[1:])
        elif step[0] == "restart":
            r.begin([step[1]], [K.RESTART_NCALLS], [K.RESTART_HEAD])
            for h in (r.b, r.t):
                h.reset_streams([step[1]], stream=cur_stream())
            r.full[step[1]], r.given[step[1]] = small_restart_pcm(), 0
        else:
            r.step(step[1], nf=8, check=False)
            if upto and r.calls == upto:
                break
    return r


def test_small_shape_all_slots_a_subset_and_the_live_state():
    """in the middle of the run (live records: the segments are what the device holds then) and after the last call: all
    slots, and a shuffled subset; slot NEVER and - with head_bytes 0 - the slot that was fed one frame before its file has a
    byte give empty segments; a list of one; the empty list"""
    A, L = api, api.lib()
    r = run_small(upto=2)
    S = r.S
    live = [s for s in range(S) if r.want[s].open and not r.want[s].ended]
    assert len(live) >= 3
    lens = fetch_checked(r.b, list(range(S)), "mid-run")
    assert lens[K.NEVER] == 0 and any(lens[s] > 16 for s in live)
    r.close()
    r = run_small()
    assert all(r.want[s].ended for s in range(S) if s != K.NEVER)
    lens = fetch_checked(r.b, list(range(S)), "all slots")
    assert lens[K.NEVER] == 0 and lens == [r.head[s] + r.length[s] for s in range(S)] and {n % 16 for n in lens} > {0}
    order = [5, K.NEVER, 0, 8, 2, 6]
    fetch_checked(r.b, order, "a shuffled subset")
    fetch_checked(r.b, [4], "one slot")
    fetch_checked(r.b, [K.NEVER], "the empty slot alone")
    # a new file in a slot with head_bytes 0, not fed yet: an empty segment between two files
    r.begin([0], [3], [0])
    sync()
    lens = fetch_checked(r.b, [2, 0, 5], "an unfed file with head_bytes 0")
    assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0
    # the empty list: 0, nothing written but off[0]
    off = np.full(1, -1, np.int64)
    assert L.hx_batch_file_fetch_many(r.b.h, None, 0, None, 0, off.ctypes.data) == 0 and off[0] == 0
    assert L.hx_batch_file_fetch_many(r.b.h, None, 0, None, 0, None) == 0
    assert L.hx_batch_file_gather_device(r.b.h, None, 0, None, 0, None, cur_stream()) == 0
    assert r.b.status() == 0
    r.b.close()
    r.t.close()


def chunk_edge_batch():
    """four slots with the same stream at 320 kbit/s (test_chunk_edges' means), files of 12 calls: run once with head_bytes 0
    to learn the files' size B, then begun again with the heads that make the segments 16 KB - 1, 16 KB, 16 KB + 1 and
    2 x 16 KB + 5 long"""
    A = api
    nc, nf = 12, 8
    pcm = synth.stream_pcm(7300, nc, bursts=True).astype(np.float32)
    b = A.Batch(A.default_control(bitrate=160), nstreams=4, max_frames=nf)
    b.file_images(3 * CHUNK)
    prefill(b)

    def run(heads):
        b.reset_streams([0, 1, 2, 3], stream=cur_stream())
        b.ledger_begin([0, 1, 2, 3], [nc] * 4, heads, stream=cur_stream())
        given = 0
        while not all(p.ended for p in b.ledger_poll()):
            n = max(0, min(nf, nc + 32 - given))
            assert n > 0
            b.frame_counts([n] * 4)
            assert b.encode_host_files(rows_block([pcm] * 4, [given] * 4, [n] * 4, nf, 2, np.float32)) == 0
            given += n
        return [p.image_bytes for p in b.ledger_poll()]
    B = run([0, 0, 0, 0])
    assert len(set(B)) == 1 and 8000 < B[0] < CHUNK - 1
    want = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
    heads = [w - B[0] for w in want]
    assert run(heads) == B
    return b, want


def test_chunk_edges_and_a_dst_cap_one_byte_short():
    """segments of 16 KB - 1, 16 KB, 16 KB + 1 and 2 x 16 KB + 5 bytes, in every order of first slot; dst_cap one byte short:
    -1, dst untouched, the offsets filled in"""
    A, L = api, api.lib()
    b, want = chunk_edge_batch()
    for first in range(4):
        idx = [(first + k) % 4 for k in range(4)]
        assert fetch_checked(b, idx, "from slot %d" % first) == [want[s] for s in idx]
    total = sum(r16(w) for w in want)
    idx = (C.c_int * 4)(0, 1, 2, 3)
    dst, off = np.full(total, SENT, np.uint8), np.full(5, -1, np.int64)
    assert L.hx_batch_file_fetch_many(b.h, idx, 4, dst.ctypes.data, total - 1, off.ctypes.data) == -1 and "do not fit dst_cap" in A.last_error()
    assert (dst == SENT).all() and off[4] == total
    assert L.hx_batch_file_fetch_many(b.h, idx, 4, dst.ctypes.data, total, off.ctypes.data) == total and (dst[:16] != SENT).any()
    assert b.status() == 0
    b.close()


def test_device_form_against_the_host_form():
    """hx_batch_file_gather_device into device memory: image and offsets equal the host form's; with a short dst_cap the
    offsets are complete, the segments that fit in whole are written, the others are not, nothing at or beyond dst_cap is, and
    status bit 16 is set; a misaligned d_dst or d_off and the list errors are refused"""
    import torch
    A, L = api, api.lib()
    b, want = chunk_edge_batch()
    idx = [2, 0, 3, 1]
    total = sum(r16(w) for w in want)
    host, hoff, _ = b.file_fetch_many(idx, total)
    d = torch.full((total + 64,), SENT, dtype=torch.uint8, device=dev())
    base = d.data_ptr() + (-d.data_ptr()) % 16
    at = base - d.data_ptr()
    d_off = torch.full((5,), -1, dtype=torch.int64, device=dev())
    sync()
    b.file_gather_device(idx, base, total, d_off.data_ptr(), stream=cur_stream())
    sync()
    got = d.cpu().numpy()
    assert d_off.cpu().numpy().tolist() == hoff.tolist() and (got[at:at + total] == host[:total]).all() and (got[at + total:] == SENT).all() and (got[:at] == SENT).all()
    assert b.status() == 0
    # refusals
    with pytest.raises(RuntimeError, match="d_dst must be 16-byte aligned"):
        b.file_gather_device(idx, base + 4, total, d_off.data_ptr(), stream=cur_stream())
    with pytest.raises(RuntimeError, match="d_off must be 8-byte aligned"):
        b.file_gather_device(idx, base, total, d_off.data_ptr() + 4, stream=cur_stream())
    with pytest.raises(RuntimeError, match="listed twice"):
        b.file_gather_device([1, 1], base, total, d_off.data_ptr(), stream=cur_stream())
    with pytest.raises(RuntimeError, match="out of range"):
        b.file_fetch_many([4], total)
    sync()
    assert (d.cpu().numpy() == got).all() and b.status() == 0
    # a dst_cap that holds the first two segments and half of the third
    d.fill_(SENT)
    d_off.fill_(-1)
    cap = int(hoff[2]) + 4096
    sync()
    b.file_gather_device(idx, base, cap, d_off.data_ptr(), stream=cur_stream())
    sync()
    got = d.cpu().numpy()
    assert d_off.cpu().numpy().tolist() == hoff.tolist()
    assert (got[at:at + hoff[2]] == host[:hoff[2]]).all() and (got[at + hoff[2]:] == SENT).all()
    assert b.status() == 16
    # ... that the fourth would fit behind the second does not matter: it lies beyond dst_cap
    b.close()
    # images off
    p = A.Batch(A.default_control(), nstreams=2, max_frames=8)
    with pytest.raises(RuntimeError, match="file images are off"):
        p.file_fetch_many([0], 64)
    with pytest.raises(RuntimeError, match="file images are off"):
        p.file_gather_device([0], base, 64, d_off.data_ptr(), stream=cur_stream())
    p.close()


def test_multi_in_two_blocks_against_the_one_batch_twin():
    """hx_multi_file_tags and hx_multi_file_fetch_many over two blocks of device 0 (5 streams: uneven blocks), with a list that
    crosses the blocks out of order, against a one-batch twin that takes the same calls: the same image, the same offsets"""
    A, L = api, api.lib()
    ncalls = [3, 8, 13, 6, 2]
    full = [synth.stream_pcm(9300 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    ec = A.default_control()
    tags = [T.tag_of(A, ec, 2, 3, nc * 1152) for nc in ncalls]
    size = A.file_tag_bytes(tags[0])
    m, b = A.Multi(ec, nstreams=5, max_frames=8, devices=[0, 0]), A.Batch(ec, nstreams=5, max_frames=8)
    for h in (m, b):
        h.file_images(9000)
        h.ledger_begin(list(range(5)), ncalls, [size] * 5, [1] * 5)
    given = [0] * 5
    while not all(p.ended for p in b.ledger_poll()):
        counts = [max(0, min(8, nc + 32 - g)) for nc, g in zip(ncalls, given)]
        blk = rows_block(full, given, counts, 8, 2, np.float32)
        for h in (m, b):
            h.frame_counts(counts)
            assert h.encode_host_files(blk) == 0
        given = [g + n for g, n in zip(given, counts)]
    assert all(p.ended for p in m.ledger_poll())
    idx = [4, 0, 3, 1, 2]
    with pytest.raises(RuntimeError, match="entry 2: slot 5 out of range"):
        m.file_tags([0, 1, 5], tags[:3])
    with pytest.raises(RuntimeError, match="entry 3: slot 4 is listed twice"):
        m.file_fetch_many([4, 0, 3, 4], 64)
    bad = A.FileTag.from_buffer_copy(tags[1])
    bad.kbps, bad.vbr_scale = 128, -1
    assert A.file_tag_bytes(bad) != size
    with pytest.raises(RuntimeError, match="entry 3: the tag frame takes"):
        m.file_tags(idx, [tags[4], tags[0], tags[3], bad, tags[2]])
    m.file_tags(idx, [tags[s] for s in idx])
    b.file_tags(idx, [tags[s] for s in idx])
    recs = b.ledger_read(list(range(5)))
    assert [r.tobytes() for r in m.ledger_read(list(range(5)))] == [r.tobytes() for r in recs]
    lens = [size + r.bytes for r in recs]
    total = sum(r16(lens[s]) for s in idx)
    for lst in (idx, [3, 1], [2], list(range(5))):
        one, off1, r1 = b.file_fetch_many(lst, total + 32, fill=SENT)
        two, off2, r2 = m.file_fetch_many(lst, total + 32, fill=SENT)
        assert r1 == r2 == sum(r16(lens[s]) for s in lst) and off1.tolist() == off2.tolist() and (one == two).all(), lst
        for e, s in enumerate(lst):
            assert one[off1[e]:off1[e] + size].tobytes() == A.file_tag_build(recs[s], tags[s]) and off1[e + 1] - off1[e] == r16(lens[s])
    dst, off = np.full(total, SENT, np.uint8), np.full(6, -1, np.int64)
    arr = (C.c_int * 5)(*idx)
    assert L.hx_multi_file_fetch_many(m.h, arr, 5, dst.ctypes.data, total - 1, off.ctypes.data) == -1 and (dst == SENT).all() and off[5] == total
    assert L.hx_multi_file_fetch_many(m.h, None, 0, None, 0, off.ctypes.data) == 0 and off[0] == 0
    assert m.status() == 0 and b.status() == 0
    m.close()
    b.close()


def test_behind_a_pipelined_submit_with_deferred_packing():
    """three hx_batch_submit_f32_device calls, no wait: the fetch of many drains, the deferred packing - and with it the last
    append - first, so the segments hold the bytes of all three calls (the host's model of the images)"""
    ncalls = [3, 40, 9, 14]
    full = [synth.stream_pcm(7600 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(ncalls)]
    r = Files(lambda: api.Batch(api.default_control(), nstreams=4, max_frames=8), full, 12000)
    r.begin([0, 1, 2, 3], ncalls, [4, 11, 0, 15])
    sets, keep = [file_bufs(r.b, 8), file_bufs(r.b, 8, shift=7)], []
    for c in range(3):
        feed = lambda blk, counts, nf: keep.append(r.device_call(r.b, blk, counts, nf, submit=True, out=sets[c & 1])) and None
        r.step([8, 8, 0 if c == 1 else 8, 5], nf=8, feed=feed, check=False)
    idx = [3, 1, 0, 2]
    lens = [r.head[s] + r.length[s] for s in idx]
    total = sum(r16(n) for n in lens)
    buf, off, got = r.b.file_fetch_many(idx, total, fill=SENT)
    assert got == total and min(lens) > 500
    for e, s in enumerate(idx):
        assert buf[off[e]:off[e] + lens[e]].tobytes() == r.model[s][:lens[e]].tobytes(), "slot %d's segment lacks bytes of the submits" % s
        assert not buf[off[e] + lens[e]:off[e + 1]].any()
    r.b.wait(cur_stream())
    sync()
    r.check("after the wait")
    r.close()
