"""Dense output on a real MI355X (include/hmp3_amd.h, "dense output"): a call's bitstreams gathered back to back behind its
packing (k_dense_off, k_dense_gather in hmp3_amd/csrc/hx_pack.hip), through the device calls, the pipelined submits, the
host calls that move only the image, a converting batch and an MPEG-2 batch.

Every comparison is equality.  The contract, with nb = out_bytes: off = [0, cumsum(round_up(nb, 16))]; segment i is the first
nb[i] bytes of row i; the bytes up to off[i + 1] are zero; the rows and nb are what a twin batch without dense output
writes.  Images are prefilled with 0xA5, so a byte a call must not write stays recognisable."""
import numpy as np
import pytest

from dense_cases import RATES, mixed_controls, mixed_pcm
from gpu_support import FILL, CallBufs, Image, Pinned, cur_stream, cut, dev, oracle_bytes, sync
import gpu_support as G
from hmp3_amd import api, synth
from output_checks import check_image, closed_form, round16
from src_cases import Stream, make_batch

pytestmark = pytest.mark.gpu
GUARD = 4096            # (gpu_support.Image's guard region behind the image)


def device_call(b, blk, nf, image, shift=0, extra=0, submit=False):
    """one fp32 device call into fresh row buffers, dense on when `image` is given (not waited for)"""
    return G.device_call(b, blk, nf, CallBufs(b, nf, shift=shift, extra=extra, image=image).set_on(b), submit=submit)


def run_twins(controls, pcm, calls, shift=0, extra=0, caps=None, tag=""):
    """the same plain device calls on two batches, one with dense output (caps[c]: the image's capacity, default the bound),
    one without: rows and byte counts identical, every image checked -> (per call: rows, nb, dense, off), the dense batch"""
    maxF = max(calls)
    bd, bt = api.Batch(controls, max_frames=maxF), api.Batch(controls, max_frames=maxF)
    res, f0 = [], 0
    for c, nf in enumerate(calls):
        cap = bd.dense_bound(nf) if caps is None or caps[c] is None else caps[c]
        img = Image(bd.n, cap)
        rd = device_call(bd, cut(pcm, f0, nf), nf, img, shift, extra)
        rt = device_call(bt, cut(pcm, f0, nf), nf, None, shift, extra)
        sync()
        (rows, nb), (trows, tnb) = rd.host(), rt.host()
        assert nb.tolist() == tnb.tolist() and (rows == trows).all(), "%s call %d: rows / byte counts differ from the twin batch's" % (tag, c)
        dense, off = img.host()
        check_image(rows, nb, dense, off, cap, tag="%s call %d" % (tag, c))
        res.append((rows, nb, dense, off))
        f0 += nf
    assert bt.status() == 0
    bt.close()
    return res, bd


def test_image_equals_rows_and_offsets_equal_the_closed_form():
    """1100 streams (more than one 1024-lane round of the offsets scan, many wave boundaries) of three rates, VBR-50: a
    first call of one frame, in which no stream emits anything (empty segments, the image untouched), then three frames;
    the first streams' segments against the oracle"""
    S = 1100
    pcm = mixed_pcm(S, 4, 3000)
    res, b = run_twins(mixed_controls(S), pcm, [1, 3], tag="1100 streams")
    assert b.status() == 0
    b.close()
    (_, nb0, dense0, off0), (_, nb1, dense1, off1) = res
    assert not nb0.any() and not off0.any() and (dense0 == FILL).all()
    assert nb1.min() > 0 and len(set(nb1.tolist())) > 8 and (nb1 % 16 != 0).any()
    for s in range(6):
        assert dense1[off1[s]:off1[s] + nb1[s]].tobytes() == oracle_bytes(dict(samprate=RATES[s % 3]), pcm[s].astype(np.int16), 4), "stream %d" % s


@pytest.mark.parametrize("shift,extra", [(0, 0), (4, 7), (1, 7)], ids=["aligned", "dword_aligned_odd_stride", "byte_aligned_odd_stride"])
def test_rows_without_alignment(shift, extra):
    """70 streams, rows of every alignment: 16-byte aligned ones (the gather's vector loads), a first row 4 and 1 byte past
    a boundary with out_stride = hx_batch_out_stride + 7 (every misalignment in turn: the funnelled path)"""
    S = 70
    res, b = run_twins(mixed_controls(S), mixed_pcm(S, 8, 3100), [4, 4], shift, extra, tag="shift %d" % shift)
    assert b.status() == 0
    b.close()
    assert all(nb.min() > 0 for _, nb, _, _ in res)


def test_capacity():
    """an image of half the needed size: status bit 16, complete offsets, the segments that fit in whole, and not a byte from
    the first one that does not up to the end of a guard region behind dense_cap; dense_cap = hx_batch_dense_bound: status
    0; a d_dense that is not 16-byte aligned is refused and the batch goes on encoding"""
    S, F = 70, 4
    controls, pcm = mixed_controls(S), mixed_pcm(S, 8, 3100)
    full, b = run_twins(controls, pcm, [F], tag="bound")
    assert b.status() == 0
    img = Image(S, b.dense_bound(F))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        b.dense_buffers(img.ptr + 4, img.cap - 16, img.off.data_ptr())
    r = device_call(b, cut(pcm, F, F), F, img)
    sync()
    assert b.status() == 0 and r.host()[1].min() > 0
    check_image(*r.host(), *img.host(), img.cap, tag="after the refusal")
    b.close()
    size = int(full[0][3][S])
    cap = (size // 2) & ~15
    assert 0 < cap < size
    half, b = run_twins(controls, pcm, [F], caps=[cap], tag="half")
    assert b.status() == 16
    b.close()
    rows, nb, dense, off = half[0]
    assert off.tolist() == full[0][3].tolist()
    fits = int(np.searchsorted(off, cap, side="right")) - 1
    assert 0 < fits < S and off[fits] <= cap < off[fits + 1]
    assert (dense[off[fits]:] == FILL).all() and len(dense) == cap + GUARD
    assert dense[:off[fits]].tobytes() == full[0][2][:off[fits]].tobytes()


def plain_rows(controls, pcm, calls):
    """(rows, nb) of plain device calls on a batch without dense output"""
    b = api.Batch(controls, max_frames=max(calls))
    out, f0 = [], 0
    for nf in calls:
        r = device_call(b, cut(pcm, f0, nf), nf, None)
        sync()
        out.append(r.host())
        f0 += nf
    assert b.status() == 0
    b.close()
    return out


@pytest.mark.parametrize("nsets,calls,last", [(2, (5, 5, 5, 5), "scratch"), (4, (5, 5, 5, 5), "off"), (3, (1, 7, 2), "scratch")],
                         ids=["two_sets_in_turn_then_scratch", "own_sets_then_off", "ragged_1_7_2"])
def test_pipelined_device_submits(nsets, calls, last):
    """hx_batch_submit_f32_device with dense output, then hx_batch_wait: a submit's image kernels go out with its deferred
    packing - behind the next submit's stream walk, or at the wait - and write the buffers set at the submit, whatever is
    set afterwards: dense output is switched off behind one submit and, behind the last one, either off or to a poisoned
    scratch image that must stay untouched.  Row and image sets alternate; with two sets the last two calls survive and are
    checked, with a set per call all of them."""
    S = 37
    controls, pcm = mixed_controls(S), mixed_pcm(S, sum(calls), 3200)
    want = plain_rows(controls, pcm, calls)
    b = api.Batch(controls, max_frames=max(calls))
    bound = b.dense_bound(max(calls))
    images = [Image(S, bound) for _ in range(nsets)]
    rows = [CallBufs(b, max(calls)) for _ in range(nsets)]
    scratch = Image(S, bound, fill=0x5A)
    import torch
    d_pcm, f0 = [], 0
    for nf in calls:
        d_pcm.append(torch.from_numpy(cut(pcm, f0, nf)).to(dev()))
        f0 += nf
    sync()
    for c, nf in enumerate(calls):
        images[c % nsets].set_on(b)
        r = rows[c % nsets]
        b.submit_device(d_pcm[c].data_ptr(), nf, r.ptr, r.stride, r.nb.data_ptr(), cur_stream(), f32=True)
        if c == 1:
            b.dense_buffers(None, 0, None)      # behind submit 1, whose packing is still to come
    if last == "off":
        b.dense_buffers(None, 0, None)
    else:
        scratch.set_on(b)
    b.wait(cur_stream())
    sync()
    assert b.status() == 0
    b.close()
    for c in range(max(0, len(calls) - nsets), len(calls)):
        (r, nb), (dense, off) = rows[c % nsets].host(), images[c % nsets].host()
        wr, wnb = want[c]
        assert nb.tolist() == wnb.tolist(), "submit %d" % c
        assert closed_form(nb).tolist() == off.tolist(), "submit %d: offsets" % c
        for s in range(S):
            assert r[s, :nb[s]].tobytes() == wr[s, :nb[s]].tobytes(), "submit %d stream %d: row" % (c, s)
            assert dense[off[s]:off[s] + nb[s]].tobytes() == wr[s, :nb[s]].tobytes(), "submit %d stream %d: segment" % (c, s)
            assert not dense[off[s] + nb[s]:off[s + 1]].any(), "submit %d stream %d: padding" % (c, s)
        if nsets >= len(calls):     # (a set used once: nothing behind the image either)
            assert (dense[off[S]:] == FILL).all(), "submit %d" % c
    sdense, soff = scratch.host()
    assert (sdense == 0x5A).all() and (soff == -1).all()
    assert sum(int(want[c][1].sum()) for c in range(len(calls))) > 0


def check_host_image(want, nb, dense, off, tag):
    """a host call's image against the list of bitstreams a row call of a twin batch returned"""
    S = len(want)
    assert nb.tolist() == [len(w) for w in want], tag
    assert off.tolist() == closed_form(nb).tolist(), tag + ": offsets"
    for s in range(S):
        assert dense[off[s]:off[s] + nb[s]].tobytes() == want[s], "%s stream %d" % (tag, s)
        assert not dense[off[s] + nb[s]:off[s + 1]].any(), "%s stream %d: padding" % (tag, s)
    assert (dense[off[S]:] == FILL).all(), tag + ": bytes written behind the image"


def test_synchronous_host_calls_return_the_image_of_the_row_calls():
    """hx_batch_encode_f32_host_dense on pageable memory, two calls, against hx_batch_encode_f32_host of a twin batch; the
    second call through Batch.encode_host_dense; a capacity of half the image returns the segments that fit"""
    S, F = 37, 6
    controls, pcm = mixed_controls(S), mixed_pcm(S, 2 * F, 3300)
    t = api.Batch(controls, max_frames=F)
    want = [t.encode_host(cut(pcm, c * F, F)) for c in range(2)]
    t.close()
    b = api.Batch(controls, max_frames=F)
    cap = b.dense_bound(F)
    assert cap == S * round16(b.out_stride(F))
    dense, off, nb = np.full(cap + GUARD, FILL, np.uint8), np.full(S + 1, -1, np.int64), np.full(S, -1, np.int32)
    blk = cut(pcm, 0, F)
    assert api.lib().hx_batch_encode_f32_host_dense(b.h, blk.ctypes.data, F, dense.ctypes.data, cap, off.ctypes.data, nb.ctypes.data) == 0, api.last_error()
    check_host_image(want[0], nb, dense, off, "call 0")
    got, off1 = b.encode_host_dense(cut(pcm, F, F))
    assert got == want[1] and off1.tolist() == closed_form([len(w) for w in want[1]]).tolist()
    assert b.status() == 0 and sum(len(w) for w in want[1]) > 0
    b.close()
    b = api.Batch(controls, max_frames=F)
    b.encode_host_dense(cut(pcm, 0, F))
    half = (int(off1[S]) // 2) & ~15
    got, off2 = b.encode_host_dense(cut(pcm, F, F), dense_cap=half)
    assert off2.tolist() == off1.tolist() and b.status() == 16
    fits = int(np.searchsorted(off2, half, side="right")) - 1
    assert 0 < fits < S and got[:fits] == want[1][:fits] and all(g is None for g in got[fits:])
    b.close()


def test_device_image_set_once_holds_across_a_host_call_that_returns_the_image():
    """The setter is sticky, and a host call that returns the image takes it for itself only: device dense buffers set once,
    then a device call, hx_batch_encode_f32_host_dense and a device call (3 streams, VBR-50, 2 frames each), the image and
    offsets prefilled again before each without a word to the batch.  The device calls' image equals their rows, which are
    a twin batch's; the host call returns the twin's bitstreams and leaves the device image and offsets as prefilled."""
    S, nf = 3, 2
    controls, pcm = mixed_controls(S), mixed_pcm(S, 3 * nf, 3500)
    t = api.Batch(controls, max_frames=nf)
    want = [t.encode_host(cut(pcm, c * nf, nf)) for c in range(3)]
    assert t.status() == 0 and sum(len(w) for ws in want for w in ws) > 0
    t.close()
    b = api.Batch(controls, max_frames=nf)
    img = Image(S, b.dense_bound(nf))
    img.set_on(b)
    for c in range(3):
        blk = cut(pcm, c * nf, nf)
        if c > 0:
            img.prefill()
        if c == 1:
            got, off = b.encode_host_dense(blk)
            assert got == want[c] and off.tolist() == closed_form([len(w) for w in want[c]]).tolist()
            dense, d_off = img.host()
            assert (dense == FILL).all() and (d_off == -1).all(), "the host call wrote the caller's device image"
        else:
            r = device_call(b, blk, nf, None)
            sync()
            rows, nb = r.host()
            assert [rows[s, :nb[s]].tobytes() for s in range(S)] == want[c], "call %d: rows differ from the twin batch's" % c
            check_image(rows, nb, *img.host(), img.cap, tag="call %d" % c)
        assert b.status() == 0
    b.close()


def test_pipelined_host_calls_write_the_image_into_page_locked_memory():
    """hx_batch_submit_s16_host_dense three times (two sets of hx_pinned_alloc buffers in turn: the last two calls survive),
    then hx_batch_wait_host, against hx_batch_submit_s16_host of a twin batch; before them a submit with a pageable image,
    refused with a message, after which the batch works"""
    S, F, calls = 37, 6, 3
    controls = mixed_controls(S)
    pcm = mixed_pcm(S, calls * F, 3300).astype(np.int16)
    t = api.Batch(controls, max_frames=F)
    stride = t.out_stride(F)
    t_out = [np.zeros((S, stride), np.uint8) for _ in range(calls)]
    t_nb = [np.zeros(S, np.int32) for _ in range(calls)]
    blks = [cut(pcm, c * F, F) for c in range(calls)]
    for c in range(calls):
        t.submit_host(blks[c].ctypes.data, F, t_out[c].ctypes.data, stride, t_nb[c].ctypes.data)
    t.wait_host()
    assert t.status() == 0
    t.close()
    want = [[t_out[c][s, :t_nb[c][s]].tobytes() for s in range(S)] for c in range(calls)]
    b = api.Batch(controls, max_frames=F)
    cap = b.dense_bound(F)
    pin = Pinned()
    try:
        dense = [pin.array(cap + GUARD, np.uint8, FILL) for _ in range(2)]
        off = [pin.array(S + 1, np.int64, -1) for _ in range(2)]
        nb = [pin.array(S, np.int32, -1) for _ in range(calls)]
        h_pcm = [pin.array(blks[c].size, np.int16, 0) for c in range(calls)]
        for c in range(calls):
            h_pcm[c][:] = blks[c].reshape(-1)
        pageable = np.full(cap, FILL, np.uint8)
        with pytest.raises(RuntimeError, match="page-locked"):
            b.submit_host_dense(h_pcm[0].ctypes.data, F, pageable.ctypes.data, cap, off[0].ctypes.data, nb[0].ctypes.data)
        with pytest.raises(RuntimeError, match="page-locked"):
            b.submit_host_dense(h_pcm[0].ctypes.data, F, dense[0].ctypes.data, cap, np.zeros(S + 1, np.int64).ctypes.data, nb[0].ctypes.data)
        assert (pageable == FILL).all() and (off[0] == -1).all()
        for c in range(calls):
            b.submit_host_dense(h_pcm[c].ctypes.data, F, dense[c & 1].ctypes.data, cap, off[c & 1].ctypes.data, nb[c].ctypes.data)
        b.wait_host()
        assert b.status() == 0
        assert nb[0].tolist() == [len(w) for w in want[0]]
        check_host_image(want[2], nb[2], dense[0][:int(off[0][S])], off[0], "submit 2")     # (set 0 held call 0's longer or shorter image before)
        check_host_image(want[1], nb[1], dense[1], off[1], "submit 1")
        assert (dense[0][max(closed_form(nb[0])[S], off[0][S]):] == FILL).all()
        assert sum(len(w) for w in want[2]) > 0
    finally:
        b.close()
        pin.free()


def test_converting_batch_image_equals_its_rows():
    """hx_batch_encode_src_device (48 kHz 24-bit sources encoded at 44.1 kHz) with dense output: the image of what the
    converting call wrote into its rows"""
    import torch
    streams = [Stream(48000, 24, 0, mpeg_select=44100, seed=81 + i, seconds=1.0) for i in range(5)]
    S, nf = len(streams), 4
    b = make_batch(streams, nf)
    pos, total = [0] * S, 0
    for c in range(2):
        in_stride = b.in_stride(nf)
        rows_in = np.zeros((S, in_stride), np.uint8)
        for i, s in enumerate(streams):
            chunk = np.frombuffer(s.data[pos[i]:pos[i] + in_stride], np.uint8)
            rows_in[i, :len(chunk)] = chunk
        d_in = torch.from_numpy(rows_in).to(dev())
        r, img = CallBufs(b, nf), Image(S, b.dense_bound(nf))
        used = np.zeros(S, np.int64)
        sync()
        img.set_on(b)
        assert api.lib().hx_batch_encode_src_device(b.h, d_in.data_ptr(), in_stride, None, nf, r.ptr, r.stride, r.nb.data_ptr(), used.ctypes.data, cur_stream()) == 0, api.last_error()
        sync()
        assert b.status() == 0
        (rows, nb), (dense, off) = r.host(), img.host()
        check_image(rows, nb, dense, off, img.cap, tag="converting call %d" % c)
        total += int(nb.sum())
        for i in range(S):
            pos[i] += int(used[i])
    assert total > 0
    b.close()


def test_mpeg2_image_equals_rows():
    """an MPEG-2 batch (22.05 kHz): every input frame yields two frames, and the byte counts cover both"""
    S, F = 9, 4
    a = api
    pcm = np.stack([synth.stream_pcm(3400 + i, 2 * F, sr=22050, rho=(0.7, 0.0, 1.0, 0.3)[i % 4], bursts=True) for i in range(S)]).astype(np.float32)
    res, b = run_twins([a.default_control(samprate=22050) for _ in range(S)], pcm, [F, F], tag="mpeg2")
    assert b.status() == 0
    b.close()
    assert res[1][1].min() > 0
