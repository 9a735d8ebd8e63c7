"""Converting batches under per-stream frame counts (hx_batch_encode_src_counts_*, hx_multi_encode_src_counts_host) on the GPU.

A converting call's counts come with the call: stream i makes the first counts[i] of the call's nframes converter and encoder
calls, 0 = it sits the call out.  Every expected value comes from outside the batch under test: the reference's
MP3_audio_encode loop on the same source (Stream.reference, compared where oracle/_ref is built) and this library's
per-frame encoder (Stream.per_frame, always), each over the stream's total number of calls.

k_src keeps a stream's call count and carried samples in two copies that change roles with every launch, for the whole
batch; a stream without a call in a launch has to copy them across.  Two idle calls in a row, and one frame after an idle
call, are the sequences that read a stale copy otherwise: the count tables below hold both for every converter case."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import skip_unless_host_libm_is_the_restated_one
from gpu_support import FILL, GOLD, GOLDEN_CLI as M, CallBufs, Image, batch_vs_single_vs_reference, cur_stream, dev, host_crc, run_cli, states, sync
from hmp3_amd import api, synth
from oracle import oracle as O
from output_checks import check_crc, check_dense, check_idle_rows
from src_cases import Stream, make_batch, make_rows, ref_converted

pytestmark = pytest.mark.gpu
FORMATS = [(8, 0), (16, 0), (24, 0), (32, 0), (32, 1)]
# (source rate, encode rate) -> the converter's case (hx_src.cpp hx_src_init): 0 copy, 1 exact 1:2, 2 linear up-sampling,
# 3 one polyphase bank (48000 -> 32000: 2 x 19 taps of memory), 4 two stages with carried intermediate samples
# (44100 -> 32000: 320 x 17 taps, 48000 -> 44100: 147 x 13 taps, both beyond one bank's 780)
PAIRS = [(44100, 44100), (22050, 44100), (32000, 44100), (48000, 32000), (44100, 32000), (48000, 44100)]
# four calls of 3 frames; stream i takes row i % 4.  Between them the rows hold a 0 between two non-zero calls, two 0s in
# a row (behind a call and from the start), a 1 after a 0 and a full 3; the four case-4 streams of a batch (streams 8 - 11)
# take one row each
TABLE = [[3, 0, 1, 2], [2, 0, 0, 1], [0, 0, 3, 1], [1, 3, 0, 2]]
HAVE_REF = O.ref() is not None


def mk(source, bits, is_float, **kw):
    s = Stream(source, bits, is_float, seconds=2.0, **kw)
    s.key = (source, bits, is_float) + tuple(sorted(kw.items()))
    return s


_expected = {}


def expect(s, total, offsets=None):
    """(bytes, input position) of the stream after `total` calls: the per-frame encoder's (without offsets), equal to the
    reference's loop where that is built; computed once per stream and total"""
    k = (s.key, total, None if offsets is None else tuple(int(o) for o in offsets))
    if k not in _expected:
        want = None
        if offsets is None:
            want = s.per_frame(total)
        if HAVE_REF:
            r = s.reference(total, offsets=offsets)
            assert want is None or want == r, "the per-frame encoder and the reference disagree on %r" % (s.key,)
            want = r
        _expected[k] = want
    return _expected[k]


def layout_streams(layout):
    """twelve streams: every pair twice - stereo in two formats, or a mono source and a stereo one summed to mono"""
    out = []
    for k, (src, tgt) in enumerate(PAIRS):
        for j in range(2):
            bits, fl = FORMATS[(2 * k + j) % 5]
            kw = dict(mpeg_select=tgt, seed=500 + 2 * k + j, noise=(k + j) % 2 == 0)
            if layout == "mono":
                kw.update(dict(channels=1) if j == 0 else dict(mono_convert=1))
            s = mk(src, bits, fl, **kw)
            s.target = tgt
            out.append(s)
    return out


def raw_call(b, rows, nf, counts, off=None, stats=True, crc=True, fn=None, n=None):
    """the C call into prefilled arrays of the caller's -> (return value, rows, out_bytes, in_used, stats, crc)"""
    A = api
    n = b.n if n is None else n
    fn = fn or A.lib().hx_batch_encode_src_counts_host
    stride = int(A.lib().hx_multi_out_stride(b.h, nf)) if fn.__name__.startswith("hx_multi") else b.out_stride(nf)
    out, nb, used = np.full((n, stride), FILL, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int64)
    st, cr = np.full((n, nf, 2), -1, np.int32), np.full((n, nf), 0xBEEF, np.uint16)
    carr = None if counts is None else (C.c_int * n)(*counts)
    o = None if off is None else np.ascontiguousarray(off, np.int64)
    rc = fn(b.h, rows.ctypes.data, rows.shape[1], None if o is None else o.ctypes.data, nf, carr, out.ctypes.data, stride, nb.ctypes.data,
            used.ctypes.data, st.ctypes.data if stats else None, cr.ctypes.data if crc else None)
    return int(rc), out, nb, used, st, cr


def untouched(out, nb, used, st, cr):
    return (out == FILL).all() and (nb == -7).all() and (used == -7).all() and (st == -1).all() and (cr == 0xBEEF).all()


def check_totals(streams, outs, pos, done):
    for i, s in enumerate(streams):
        want, end = expect(s, done[i])
        assert outs[i] == want, "stream %d %r: bytes after %d calls" % (i, s.key, done[i])
        assert pos[i] == end, "stream %d %r: input position after %d calls" % (i, s.key, done[i])


@pytest.mark.parametrize("layout", ["stereo", "mono"])
def test_uneven_calls_equal_each_streams_own_run(layout, k6_build):
    """twelve streams, one pair per converter case 0 - 4 (case 4 twice) in two formats or layouts, four calls of 3 frames
    under TABLE: per stream the concatenated rows and the final input position are the reference's and the per-frame
    encoder's over the stream's total, the "srcpcm" tap's frames f < n are the reference converter's bit for bit, and the
    status is 0 after every call"""
    streams = layout_streams(layout)
    S, nf, nch = len(streams), 3, 2 if layout == "stereo" else 1
    b = make_batch(streams, nf)
    pos, done, outs = [0] * S, [0] * S, [b""] * S
    conv = [ref_converted(s, s.target, 8) for s in streams] if HAVE_REF else None
    for c in range(4):
        counts = [TABLE[i % 4][c] for i in range(S)]
        res, used = b.encode_src_counts_host(make_rows(b, streams, pos, nf, counts), nf, counts)
        assert b.status() == 0
        pcm = b.debug_read("srcpcm", np.float32, S * nf * 1152 * nch).reshape(S, nf * 1152, nch)
        for i, n in enumerate(counts):
            if conv is not None:
                want = conv[i][done[i] * 1152:(done[i] + n) * 1152]
                assert np.array_equal(pcm[i, :n * 1152].view(np.uint32), want.view(np.uint32)), "call %d stream %d: converted PCM" % (c, i)
            if n == 0:
                assert res[i] == b"" and used[i] == 0, "call %d: idle stream %d" % (c, i)
            outs[i] += res[i]
            pos[i] += int(used[i])
            done[i] += n
    check_totals(streams, outs, pos, done)
    b.close()


def test_an_idle_stream_is_untouched_and_garbage_is_never_read(k6_build):
    """three calls of 4 frames on two batches of the same ten streams: one with zeros, one with 0xFF (NaN as fp32) over every
    row byte beyond what the stream's n calls read and over the whole rows of n = 0 streams.  The n = 0 streams' checkpoints
    are the same bytes before and after, their rows are not written, out_bytes and in_used are 0, their counters repeat the
    ones they entered with and their CRCs are 0; every stream's bytes equal the zero-filled run's and the per-frame encoder's"""
    streams = layout_streams("stereo")[2:]
    S, nf = len(streams), 4
    table = [[0, 4, 1, 0, 2, 0, 3, 1, 0, 4], [0, 0, 2, 1, 4, 0, 0, 3, 1, 0], [2, 1, 0, 0, 3, 1, 4, 0, 0, 2]]
    bz, bg = make_batch(streams, nf), make_batch(streams, nf)
    pos, done, outs = [0] * S, [0] * S, [b""] * S
    entered = [(0, 0)] * S
    for c, counts in enumerate(table):
        rcz, outz, nbz, usedz, stz, crz = raw_call(bz, make_rows(bz, streams, pos, nf, counts, garbage=0), nf, counts)
        before = states(bg, single=True)
        rc, out, nb, used, st, cr = raw_call(bg, make_rows(bg, streams, pos, nf, counts, garbage=0xFF), nf, counts)
        assert rcz == 0 and rc == 0 and bz.status() == 0 and bg.status() == 0
        after = states(bg, single=True)
        for i, n in enumerate(counts):
            at = "call %d stream %d (count %d)" % (c, i, n)
            if n == 0:
                assert after[i] == before[i], at + ": checkpoint changed"
                assert nb[i] == 0 and used[i] == 0 and (out[i] == FILL).all(), at + ": outputs of an idle stream"
                assert all(tuple(st[i, f]) == entered[i] for f in range(nf)), at + ": counters"
                assert (cr[i] == 0).all(), at + ": CRC of no bytes"
            assert nb[i] == nbz[i] and out[i, :nb[i]].tobytes() == outz[i, :nbz[i]].tobytes() and used[i] == usedz[i], at + ": garbage reached the output"
            assert (st[i] == stz[i]).all() and (cr[i] == crz[i]).all(), at
            assert all(tuple(st[i, f]) == tuple(st[i, max(n, 1) - 1]) for f in range(n, nf)), at + ": counters behind the count"
            entered[i] = tuple(int(v) for v in st[i, nf - 1])
            outs[i] += out[i, :nb[i]].tobytes()
            pos[i] += int(used[i])
            done[i] += n
    check_totals(streams, outs, pos, done)
    bz.close()
    bg.close()


def test_frame_offsets_under_counts(k6_build):
    """two calls of 3 frames with an offset per call that revisits input (back to 0) and skips it, rows starting at the
    sources' first byte; the entries f >= n are -1 and far beyond in_stride and are ignored.  Against the reference's loop
    fed the same pointers (where it is built; the per-frame encoder takes no pointers)"""
    streams = [layout_streams("stereo")[i] for i in (0, 3, 5, 6, 8, 9, 10, 11)]
    S, nf = len(streams), 3
    b = make_batch(streams, nf)
    table = [[3, 0, 1, 2, 3, 1, 0, 2], [1, 2, 0, 3, 2, 1, 3, 0]]
    offs_of = [[] for _ in range(S)]
    outs, last = [b""] * S, [0] * S
    rows = make_rows(b, streams, [0] * S, nf, None, extra=65536)
    for c, counts in enumerate(table):
        off = np.empty((S, nf), np.int64)
        for i, s in enumerate(streams):
            for f in range(nf):
                k = len(offs_of[i])
                if f < counts[i]:
                    off[i, f] = s.fb * (0 if k % 3 == 1 else 700 * k + 3)
                    offs_of[i].append(int(off[i, f]))
                else:
                    off[i, f] = -1 if f % 2 else 10 * rows.shape[1]
        rc, out, nb, used, st, cr = raw_call(b, rows, nf, counts, off=off)
        assert rc == 0, api.last_error()
        assert b.status() == 0
        for i, n in enumerate(counts):
            outs[i] += out[i, :nb[i]].tobytes()
            if n:
                last[i] = int(used[i])
            else:
                assert used[i] == 0 and nb[i] == 0
    if not HAVE_REF:
        pytest.skip("oracle/_ref not built: no reference for calls with pointers of their own")
    for i, s in enumerate(streams):
        s.data = bytes(rows[i])
        want, end = s.reference(len(offs_of[i]), offsets=offs_of[i])
        assert outs[i] == want and last[i] == end, "stream %d %r" % (i, s.key)
    b.close()


def test_optional_outputs_of_a_converting_call_under_counts(k6_build):
    """one call of 4 frames under counts on one batch and a uniform one on another: device call with packet, counter, CRC
    and dense buffers, host call with stats and crc.  Entries f < n equal the uniform call's; behind the count the counters
    repeat the end-of-call values, packet sizes are {0, 0} and no packet byte is written, crc[i][f] is the host CRC of row
    i's e[f] bytes, and the dense image follows out_bytes"""
    import torch
    streams = [layout_streams("stereo")[i] for i in (1, 2, 4, 7, 8, 11)]
    S, nf = len(streams), 4
    counts = [2, 0, 4, 1, 3, 0]
    bu, bc = make_batch(streams, nf), make_batch(streams, nf)
    rows = make_rows(bu, streams, [0] * S, nf, None)
    d_rows = torch.from_numpy(rows).to(dev())
    q = cur_stream()
    res = []
    for b, cn in ((bu, None), (bc, counts)):
        o = CallBufs(b, nf, rows_fill=FILL, counters=True, crc=True, packets=4096, image=Image(b.n, b.dense_bound(nf), guard=0)).set_on(b)
        used = b.encode_src_counts_device(d_rows.data_ptr(), rows.shape[1], nf, cn, o.ptr, o.stride, o.nb.data_ptr(), stream=q)
        sync()
        assert b.status() == 0
        check_crc(o)
        check_dense(o)
        res.append((o, used))
    (ou, usedu), (oc, usedc) = res
    check_idle_rows(oc, counts)
    (ru, nbu), (rc_, nbc) = ou.rows(), oc.rows()
    (pku, pkbu, stu), (pkc, pkbc, stc) = ou.packets(), oc.packets()
    for i, n in enumerate(counts):
        at = "stream %d (count %d)" % (i, n)
        assert (stc[i, :n] == stu[i, :n]).all() and (pkbc[i, :n] == pkbu[i, :n]).all() and (pkc[i, :n] == pku[i, :n]).all(), at
        assert rc_[i, :nbc[i]].tobytes() == ru[i, :nbc[i]].tobytes() and nbc[i] <= nbu[i], at + ": the row is a prefix of the uniform call's"
        for f in range(n, nf):
            assert tuple(stc[i, f]) == (tuple(stc[i, n - 1]) if n else (0, 0)), at + ": counters behind the count"
            assert tuple(pkbc[i, f]) == (0, 0) and (pkc[i, f] == FILL).all(), at + ": packets behind the count"
        assert usedc[i] == sum(int(v) for v in make_used(streams[i], n)), at + ": in_used"
    # the host call on two fresh batches: stats and crc
    hu, hc = make_batch(streams, nf), make_batch(streams, nf)
    _, outu, nbu, _, stu, cru = raw_call(hu, rows, nf, None)
    rc, outc, nbc, _, stc, crc = raw_call(hc, rows, nf, counts)
    assert rc == 0 and hc.status() == 0
    for i, n in enumerate(counts):
        assert (stc[i, :n] == stu[i, :n]).all() and (crc[i, :n] == cru[i, :n]).all(), i
        for f in range(nf):
            e = int(nbc[i]) - ((int(stc[i, -1, 1]) - int(stc[i, f, 1])) & 0xFFFFFFFF)
            assert 0 <= e <= nbc[i] and crc[i, f] == host_crc(outc[i, :e]), "host call stream %d frame %d: CRC" % (i, f)
            if f >= n:
                assert tuple(stc[i, f]) == (tuple(stc[i, n - 1]) if n else (0, 0)) and e == nbc[i]
    for b in (bu, bc, hu, hc):
        b.close()


def make_used(s, n):
    """input bytes the stream's first n calls consume, from the host converter's schedule"""
    A = api
    L = A.lib()
    h = L.hx_src_create()
    cut = C.c_int(0)
    tch = 1 if (s.channels == 1 or s.mono_convert) else 2
    assert L.hx_src_init(h, s.source, s.channels, s.bits, s.is_float, s.target, tch, C.byref(cut)) > 0
    nb = np.zeros(max(n, 1), np.int64)
    L.hx_src_schedule(h, 0, n, nb.ctypes.data)
    L.hx_src_destroy(h)
    return nb[:n]


def test_refusals_leave_the_batch_usable(k6_build):
    """counts of -1 and nframes + 1, a row too short for a stream's n calls and crc without stats are refused (-1), the count
    refusals naming the stream; a row too short only for nframes calls is accepted.  After each refusal the prefilled outputs
    are untouched, every checkpoint and schedule() are as before, and the calls that follow match the reference"""
    A = api
    streams = [layout_streams("stereo")[i] for i in (9, 6, 2)]     # (stream 0: 8 bytes per sample frame, the widest rows)
    S, nf = len(streams), 3
    b = make_batch(streams, nf)
    pos, done, outs = [0] * S, [0] * S, [b""] * S

    def valid(counts, rows=None):
        rc, out, nb, used, _, _ = raw_call(b, make_rows(b, streams, pos, nf, counts) if rows is None else rows, nf, counts)
        assert rc == 0 and b.status() == 0, A.last_error()
        for i, n in enumerate(counts):
            outs[i] += out[i, :nb[i]].tobytes()
            pos[i] += int(used[i])
            done[i] += n

    valid([1, 0, 2])
    # a row that holds one call of every stream: too short for nframes calls, and for the two calls of stream 0
    short = b.schedule(0, 1)[1]
    assert max(b.schedule(i, 1)[1] for i in range(S)) == short < b.schedule(0, 2)[1]
    full = make_rows(b, streams, pos, nf, None)
    refused = [(full, [2, -1, 2], True, "stream 1"), (full, [2, 2, nf + 1], True, "stream 2"),
               (np.ascontiguousarray(full[:, :short]), [2, 1, 1], True, "stream 0"), (full, [1, 1, 1], False, "")]
    for rows, counts, stats, who in refused:
        before, sched = states(b, single=True), [b.schedule(i, nf)[0].tolist() for i in range(S)]
        rc, *o = raw_call(b, rows, nf, counts, stats=stats)
        assert rc == -1 and who in A.last_error(), (counts, A.last_error())
        assert untouched(*o), "a refused call wrote an output"
        assert states(b, single=True) == before and [b.schedule(i, nf)[0].tolist() for i in range(S)] == sched
    with pytest.raises(TypeError):
        b.encode_src_counts_host(full, nf, [1, 1, 1], crc=True)
    with pytest.raises(RuntimeError, match="stream 2"):
        b.encode_src_counts_host(full, nf, [0, 0, 7])
    valid([1, 1, 1], rows=np.ascontiguousarray(full[:, :short]))
    valid([0, 3, 1])
    check_totals(streams, outs, pos, done)
    b.close()


@pytest.mark.one_k6_build
@pytest.mark.parametrize("kind", ["mpeg2", "intensity"])
def test_mpeg2_target_and_first_generation_allocator_under_counts(kind, k6_build):
    """11025 -> 22050 (exact 1:2) and 48000 -> 24000 (one bank) streams, an MPEG-2 call yielding two frames per converter
    call: mono and summed-to-mono at 64 kbit/s, or stereo at 16 kbit/s, which is packet_cases.A1's intensity-stereo control of
    the first-generation allocator at 22.05 kHz (its streams go through libm in the reference: skipped where the host's
    differs from the restated one)"""
    if kind == "intensity":
        skip_unless_host_libm_is_the_restated_one()
        streams = [mk(11025, 16, 0, mpeg_select=22050, seed=601, bitrate=16), mk(48000, 24, 0, mpeg_select=24000, seed=602, bitrate=16),
                   mk(11025, 8, 0, mpeg_select=22050, seed=603, bitrate=16, noise=True), mk(48000, 32, 1, mpeg_select=24000, seed=604, bitrate=16)]
    else:
        streams = [mk(11025, 16, 0, channels=1, mpeg_select=22050, seed=611), mk(48000, 24, 0, mono_convert=1, mpeg_select=24000, seed=612),
                   mk(11025, 32, 1, mono_convert=1, mpeg_select=22050, seed=613, noise=True), mk(48000, 8, 0, channels=1, mpeg_select=24000, seed=614)]
    S, nf = len(streams), 3
    b = make_batch(streams, nf)
    pos, done, outs = [0] * S, [0] * S, [b""] * S
    for c in range(4):
        counts = [TABLE[i][c] for i in range(S)]
        res, used = b.encode_src_counts_host(make_rows(b, streams, pos, nf, counts, garbage=0xFF), nf, counts)
        assert b.status() == 0
        for i, n in enumerate(counts):
            outs[i] += res[i]
            pos[i] += int(used[i])
            done[i] += n
    check_totals(streams, outs, pos, done)
    b.close()


@pytest.mark.one_k6_build
def test_multi_over_two_blocks_on_one_device(k6_build):
    """hx_multi_encode_src_counts_host: five streams in blocks of 3 + 2 on device 0, three calls with zeros among the counts,
    bytes per stream as in the first test; a count out of range in the second block refuses the call for all streams before a
    block starts, names the stream by its number over all blocks and moves none"""
    A = api
    L = A.lib()
    streams = [layout_streams("stereo")[i] for i in (3, 8, 5, 10, 0)]
    S, nf = len(streams), 3
    m = A.SrcMulti([s.ec for s in streams], [s.src for s in streams], max_frames=nf, devices=[0, 0])
    assert [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    fn = L.hx_multi_encode_src_counts_host
    pos, done, outs = [0] * S, [0] * S, [b""] * S

    def rows_for():
        stride = m.in_stride(nf)
        rows = np.zeros((S, stride), np.uint8)
        for i, s in enumerate(streams):
            rows[i] = np.frombuffer(s.data[pos[i]:pos[i] + stride], np.uint8)
        return rows

    def multi_states():
        blobs = []
        for k in range(2):
            h, (_, first, count) = L.hx_multi_batch(m.h, k), m.shard(k)
            for i in range(count):
                buf = (C.c_ubyte * int(L.hx_batch_stream_state_bytes(h)))()
                assert L.hx_batch_get_stream_state(h, i, buf) == 0
                blobs.append(bytes(buf))
        return blobs

    for c, counts in enumerate([[3, 0, 1, 0, 2], [0, 0, 2, 1, 3], [1, 2, 0, 0, 1]]):
        if c == 2:
            before = multi_states()
            bad = list(counts)
            bad[3] = nf + 1
            rc, *o = raw_call(m, rows_for(), nf, bad, fn=fn, n=S)
            assert rc == -1 and A.last_error().startswith("stream 3: frame count %d " % (nf + 1)), A.last_error()
            assert untouched(*o) and multi_states() == before
        res, used, st, cr = m.encode_src_counts_host(rows_for(), nf, counts, stats=True, crc=True)
        assert m.status() == 0
        for i, n in enumerate(counts):
            assert cr[i, nf - 1] == host_crc(res[i]), "call %d stream %d: CRC of the call's row" % (c, i)
            outs[i] += res[i]
            pos[i] += int(used[i])
            done[i] += n
    check_totals(streams, outs, pos, done)
    m.close()


# ---- the command line: -batch takes files at any rate and -A (hmp3_amd/cli/hmp3amd.cpp, the converting route) ----

SRC_CASES = ["cli_src_11k_to_22k_s16", "cli_src_8k_to_16k_u8_mono", "cli_src_32k_to_44k_f32", "cli_src_48k_to_24k_s24", "cli_src_44k_to_32k_s16",
             "cli_src_44k_to_22k_downmix", "cli_src_44k_to_16k_f32_nopad", "cli_src_48k_to_22k_s24_nopad", "cli_src_24k_to_22k_s32_nopad"]


@pytest.mark.one_k6_build
@pytest.mark.parametrize("name", SRC_CASES)
def test_cli_batch_of_one_converting_file_equals_the_reference_cli(name, tmp_path, k6_build):
    """`hmp3amd -batch in.wav out.mp3 <flags>` on each sample-rate-conversion case of the whole-file goldens: the file the
    reference's command line wrote (tests/golden/<name>.mp3), tag frame, TOC and MusicCRC included"""
    seed, nsamp, sr, as_float, bursts, flags = M.CASES[name]
    wav, mp3 = str(tmp_path / "in.wav"), str(tmp_path / "out.mp3")
    M.write_wav(wav, M.case_pcm(name), sr, as_float, M.CONTAINER.get(name))
    run_cli(["-batch", wav, mp3] + flags)
    assert open(mp3, "rb").read() == open(os.path.join(GOLD, name + ".mp3"), "rb").read()


@pytest.mark.one_k6_build
def test_cli_batch_of_converting_files_of_different_lengths(tmp_path, k6_build):
    """one `-batch -A32000 -B64` run of three stereo files - 48 kHz s24, 44.1 kHz s16, 32 kHz f32, of 5, 40 and 130 output
    frames, so two of them end inside the first call of 96 frames - writes the files of the three single-file runs byte for
    byte, and the reference binary's where it is built"""
    flags = ["-A32000", "-B64"]
    files = []
    for i, (sr, fmt, frames) in enumerate([(48000, 24, 5), (44100, False, 40), (32000, True, 130)]):
        nsamp = frames * 1152 * sr // 32000 - 301 * i - 7
        pcm = synth.stream_pcm(9500 + i, nsamp // 1152 + 1, sr=sr, rho=0.5, bursts=i != 1)[:nsamp]
        wav = str(tmp_path / ("in%d.wav" % i))
        M.write_wav(wav, pcm, sr, fmt)
        files.append(("file %d" % i, wav, str(tmp_path / ("batch%d.mp3" % i))))
    batch_vs_single_vs_reference(files, flags)
