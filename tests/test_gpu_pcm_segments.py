"""PCM segments (hx_batch_pcm_segments, hx_multi_pcm_segments, k_pcm_spread) on a real MI355X: a call's input as one image
whose segments the GPU spreads into the rows the front end reads.

Every comparison is equality against a twin batch of the same controls, made the same way and fed rows built from the same
samples: the rows' used parts, out_bytes, and the optional outputs where named.  PCM comes from hmp3_amd.synth.  Whatever of
an image or a row belongs to no stream is a poison - 0x7FFF (int16) or a quiet NaN (fp32): nothing may depend on it.  Device
calls write into zeroed rows, so the streams' checkpoints can be compared across the two batches as well (behind host calls
they are not: a stream's ring of pending main data keeps the bytes that lie behind its frames in the call's row, and a host
call's rows are device staging that nobody zeroes).
k_pcm_spread's chunk is 16 KB (HX_PCM_CHUNK), the size the chunk-edge test's segments are chosen for."""
import functools

import numpy as np
import pytest

import gpu_support as G
from gpu_support import CallBufs, Pinned, controls, states, sync
from hmp3_amd import api, synth

pytestmark = pytest.mark.gpu
POISON = {np.dtype(np.int16): 0x7FFF, np.dtype(np.float32): np.nan}
FILL = 0xA5
STEREO, MONO = dict(bitrate=64), dict(bitrate=64, mode=3)


@functools.lru_cache(maxsize=None)
def signal(seed, ch, F, f32, sr=44100):
    """stream `seed`'s samples as its row holds them, [F, 1152 * ch] (interleaved for ch = 2): int16, or float32 at int16 scale
    with non-integral samples; computed once, shared, never changed"""
    x = synth.stream_pcm(seed, F, sr=sr, rho=(0.7, 0.0, 1.0, 0.3)[seed % 4], bursts=True)
    x = x if ch == 2 else x[:, seed & 1]
    if f32:
        x = x.astype(np.float32) + np.random.default_rng(seed).uniform(-0.49, 0.49, x.shape).astype(np.float32)
    x = np.ascontiguousarray(x).reshape(F, 1152 * ch)
    x.setflags(write=False)
    return x


class Feed:
    """the streams' signals and how far each has come; take(counts) -> every stream's next samples, flat, in row order"""

    def __init__(self, channels, F, dtype, seed=900, sr=None):
        self.dtype = np.dtype(dtype)
        self.sig = [signal(seed + i, ch, F, self.dtype == np.float32, *( (sr[i],) if sr else ())) for i, ch in enumerate(channels)]
        self.pos = [0] * len(channels)

    def take(self, counts):
        parts = []
        for s, n in enumerate(counts):
            assert self.pos[s] + n <= len(self.sig[s]), "the test's signal is too short"
            parts.append(self.sig[s][self.pos[s]:self.pos[s] + n].reshape(-1))
            self.pos[s] += n
        return parts


def rows_of(parts, nf, P, dtype):
    """the twin's input [S, nf * 1152 * P]: every stream's samples at the start of its row, poison behind them"""
    blk = np.full((len(parts), nf * 1152 * P), POISON[np.dtype(dtype)], dtype)
    for s, p in enumerate(parts):
        blk[s, :len(p)] = p
    return blk


def image_of(parts, off, total, dtype):
    """the image of `total` bytes: part i at byte off[i] (parts written in order: an overlap keeps the later one), poison elsewhere"""
    item = np.dtype(dtype).itemsize
    assert total % item == 0
    img = np.full(total // item, POISON[np.dtype(dtype)], dtype)
    for p, o in zip(parts, off):
        assert o % item == 0 and o + p.nbytes <= total
        img[o // item:o // item + len(p)] = p
    return img


def spaced(parts, residues, dtype, descending=False):
    """offsets that leave a gap in front of every segment and start segment i `residues[i]` bytes past a 16-byte boundary
    (descending: the first stream's segment last in the image) -> (off int64 [S], total)"""
    order = range(len(parts) - 1, -1, -1) if descending else range(len(parts))
    off, at = np.zeros(len(parts), dtype=np.int64), 0
    for i in order:
        off[i] = at + 48 + residues[i]
        at = (off[i] + parts[i].nbytes + 15) // 16 * 16
    return off, int(at + 64)


def call(b, pcm, nf, shift=0, submit=False):
    """one device call - or submit - on the null stream: the PCM `shift` elements past a 16-byte boundary, zeroed rows"""
    return G.device_call(b, pcm, nf, CallBufs(b, nf), submit=submit, stream=None, shift=shift)


def result(o):
    sync()
    return o.bitstreams()


def device_call(b, pcm, nf, shift=0):
    r = result(call(b, pcm, nf, shift))
    assert b.status() == 0
    return r


def host_crc_call(b, pcm, nf):
    """hx_batch_encode_f32_host_crc into prefilled host buffers -> (return code, rows, out_bytes, stats, crc)"""
    stride = b.out_stride(nf)
    out, nb = np.full((b.n, stride), FILL, np.uint8), np.full(b.n, -1, np.int32)
    st, cr = np.full((b.n, nf, 2), -1, np.int32), np.full((b.n, nf), 0xFFFF, np.uint16)
    pcm = np.ascontiguousarray(pcm, dtype=np.float32)
    rc = api.lib().hx_batch_encode_f32_host_crc(b.h, pcm.ctypes.data, nf, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data, cr.ctypes.data)
    return rc, out, nb, st, cr


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_tight_layout_of_a_uniform_batch_equals_rows_call_after_call(f32):
    """6 stereo 44.1 kHz CBR-128 streams, three device calls of 3 frames fed the tight image: rows and byte counts of every
    call equal the twin's - from the second call on that also holds the PCM history k_msscan carries to the spread rows - and
    so does every stream's checkpoint at the end"""
    a = api
    dtype, S, nf = (np.float32 if f32 else np.int16), 6, 3
    b, t = (a.Batch(a.default_control(**STEREO), nstreams=S, max_frames=nf) for _ in range(2))
    feed = Feed([2] * S, 9, dtype)
    off, total = b.packed_layout(nf, f32)
    assert list(off) == [i * nf * 2304 * (4 if f32 else 2) for i in range(S + 1)]
    b.pcm_segments(off, total)
    for c in range(3):
        parts = feed.take([nf] * S)
        got = device_call(b, image_of(parts, off, total, dtype), nf)
        want = device_call(t, rows_of(parts, nf, 2, dtype), nf)
        assert all(len(w) > 0 for w in want) or c == 0
        assert got == want, "call %d" % c
    assert states(b) == states(t)
    b.close(), t.close()


def test_counts_and_channels_through_the_host_crc_call():
    """the command line's call: a mixed batch of 8 slots alternating stereo and mono under per-stream counts, fed the tight
    fp32 image through hx_batch_encode_f32_host_crc - rows, out_bytes, frame counters and CRCs equal the twin's, and the host
    rows of the streams that sit a call out are untouched"""
    a = api
    S, nf, ch = 8, 3, [2, 1] * 4
    b, t = (a.Batch.mixed(controls([STEREO, MONO]), S, cfg=[0, 1] * 4, max_frames=nf) for _ in range(2))
    feed = Feed(ch, 8, np.float32)
    for c, counts in enumerate([[3, 0, 1, 2, 3, 1, 0, 2], [0, 3, 2, 0, 1, 3, 3, 1]]):
        parts = feed.take(counts)
        for x in (b, t):
            x.frame_counts(counts)
        off, total = b.packed_layout(nf, True)
        assert total == sum(p.nbytes for p in parts) and list(off) == list(a.packed_layout(nf, ch, counts, True)[0])
        b.pcm_segments(off, total)
        rc, out, nb, st, cr = host_crc_call(b, image_of(parts, off, total, np.float32), nf)
        assert rc == 0 and b.status() == 0, a.last_error()
        rc, wout, wnb, wst, wcr = host_crc_call(t, rows_of(parts, nf, 2, np.float32), nf)
        assert rc == 0 and t.status() == 0, a.last_error()
        assert (nb == wnb).all() and (st == wst).all() and (cr == wcr).all(), "call %d" % c
        for s, n in enumerate(counts):
            assert out[s, :nb[s]].tobytes() == wout[s, :wnb[s]].tobytes(), "call %d stream %d" % (c, s)
            if n == 0:
                assert nb[s] == 0 and (out[s] == FILL).all(), "call %d: stream %d sat the call out and its host row was written" % (c, s)
        assert nb.sum() > 0
    # (no checkpoint comparison here: a stream's ring of pending main data keeps whatever bytes lie behind its frames in the
    # call's row, and a host call's rows are the batch's own device staging, which nobody zeroes)
    b.close(), t.close()


@pytest.mark.parametrize("shift", [0, 1], ids=["base_aligned", "base_one_sample_on"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_every_alignment_residue_of_a_segment_start(f32, shift):
    """8 streams whose segments start 0, 2, .. 14 bytes (int16; fp32: 0, 4, 8, 12 twice) past a 16-byte boundary of the image,
    with poisoned gaps between them - and once more with the device image's base itself one sample past a 16-byte boundary,
    which moves every residue on: aligned loads, every word residue of the funnel and, for int16, the half-word ones"""
    a = api
    dtype, S, nf = (np.float32 if f32 else np.int16), 8, 2
    b, t = (a.Batch(a.default_control(**STEREO), nstreams=S, max_frames=nf) for _ in range(2))
    parts = Feed([2] * S, nf, dtype, seed=920).take([nf] * S)
    off, total = spaced(parts, [(4 if f32 else 2) * i % 16 for i in range(S)], dtype)
    assert sorted(set(int(o) % 16 for o in off)) == ([0, 4, 8, 12] if f32 else [0, 2, 4, 6, 8, 10, 12, 14])
    b.pcm_segments(off, total)
    got = device_call(b, image_of(parts, off, total, dtype), nf, shift)
    assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf)
    assert states(b) == states(t)
    b.close(), t.close()


def test_chunk_edges_of_the_spread():
    """a max_frames = 32 int16 batch whose segments are 2304 B (one mono frame: less than a 16 KB chunk), 16128 B (7 mono
    frames: just under one), 18432 B (4 stereo frames: just over) and 147456 B (32 stereo frames: exactly nine chunks)"""
    a = api
    nf, ch, counts = 32, [1, 1, 2, 2], [1, 7, 4, 32]
    b, t = (a.Batch.mixed(controls([STEREO, MONO]), 4, cfg=[1, 1, 0, 0], max_frames=nf) for _ in range(2))
    parts = Feed(ch, 32, np.int16, seed=930).take(counts)
    assert [p.nbytes for p in parts] == [2304, 16128, 18432, 147456]
    for x in (b, t):
        x.frame_counts(counts)
    off, total = b.packed_layout(nf)
    b.pcm_segments(off, total)
    got = device_call(b, image_of(parts, off, total, np.int16), nf)
    assert got == device_call(t, rows_of(parts, nf, 2, np.int16), nf)
    assert states(b) == states(t)
    rows = b.debug_read("pcmrows", np.int16, 4 * nf * 2304).reshape(4, -1)
    for s, p in enumerate(parts):
        assert (rows[s, :len(p)] == p).all(), "stream %d: the spread row" % s
    b.close(), t.close()


def test_no_store_lands_behind_a_segment_or_in_another_row():
    """the "pcmrows" tap: call A at full counts, then call B with smaller counts and other samples - every row holds B's
    segment in its first len_i bytes and, from there to its end, exactly what call A left there; the row of a stream that
    sits B out is A's whole"""
    a = api
    S, nf, ch = 6, 3, [2, 1, 2, 1, 2, 1]
    b = a.Batch.mixed(controls([STEREO, MONO]), S, cfg=[0, 1] * 3, max_frames=nf)
    feed = Feed(ch, 6, np.int16, seed=940)

    def call(counts):
        parts = feed.take(counts)
        b.frame_counts(counts)
        off, total = spaced(parts, [2 * i for i in range(S)], np.int16)
        b.pcm_segments(off, total)
        device_call(b, image_of(parts, off, total, np.int16), nf)
        return parts, b.debug_read("pcmrows", np.int16, S * nf * 2304).reshape(S, -1).copy()

    pa, ra = call([nf] * S)
    for s in range(S):
        assert (ra[s, :len(pa[s])] == pa[s]).all(), "call A stream %d" % s
    pb, rb = call([1, 2, 0, 0, 2, 1])
    for s in range(S):
        assert (rb[s, :len(pb[s])] == pb[s]).all(), "call B stream %d: its segment" % s
        assert (rb[s, len(pb[s]):] == ra[s, len(pb[s]):]).all(), "call B stream %d: bytes stored behind its segment" % s
    assert len(pb[2]) == 0 and (rb[2] == ra[2]).all()
    b.close()


def test_gaps_descending_order_and_a_shared_segment():
    """segments in descending order with poisoned gaps between them, and two slots of the same control reading one segment:
    they emit identical rows, and all equal the twin's"""
    a = api
    S, nf = 4, 3
    b, t = (a.Batch(a.default_control(**STEREO), nstreams=S, max_frames=nf) for _ in range(2))
    parts = Feed([2] * S, nf, np.float32, seed=950).take([nf] * S)
    parts[3] = parts[2]
    off, total = spaced(parts[:3], [0, 4, 8], np.float32, descending=True)
    assert off[0] > off[1] > off[2]
    off = np.append(off, off[2])
    b.pcm_segments(off, total)
    got = device_call(b, image_of(parts[:3], off[:3], total, np.float32), nf)
    assert got == device_call(t, rows_of(parts, nf, 2, np.float32), nf)
    assert got[2] == got[3] and len(got[2]) > 0 and got[0] != got[1]
    b.close(), t.close()


PIN = Pinned()         # (kept until the module's teardown releases it)
pinned = PIN.copy


@pytest.fixture(scope="module", autouse=True)
def _release_pinned():
    yield
    PIN.free()


SUBMITS = [[3, 1, 0, 2, 3, 2], [1, 3, 2, 0, 1, 3], [2, 0, 3, 3, 0, 1]]


def test_segments_travel_with_their_submit():
    """three hx_batch_submit_f32_host calls and a wait, then three hx_batch_submit_s16_device calls and a wait: every submit
    under other counts and offsets, the setters called between the submits while the earlier ones are in flight - the rows
    of all six equal the twin's, which makes the same submits fed rows"""
    import torch
    a = api
    S, nf, ch = 6, 3, [2, 1] * 3
    b, t = (a.Batch.mixed(controls([STEREO, MONO]), S, cfg=[0, 1] * 3, max_frames=nf) for _ in range(2))
    stride = b.out_stride(nf)
    feed = Feed(ch, 9, np.float32, seed=960)
    got, want = [], []
    for c, counts in enumerate(SUBMITS):
        parts = feed.take(counts)
        off, total = spaced(parts, [4 * ((i + c) % 4) for i in range(S)], np.float32, descending=c == 1)
        for x, pcm, res in ((b, image_of(parts, off, total, np.float32), got), (t, rows_of(parts, nf, 2, np.float32), want)):
            x.frame_counts(counts)
            if x is b:
                x.pcm_segments(off, total)
            pcm, out, nb = pinned(pcm), pinned(np.zeros((S, stride), np.uint8)), pinned(np.full(S, -1, np.int32))
            x.submit_host(pcm.ctypes.data, nf, out.ctypes.data, stride, nb.ctypes.data, f32=True)
            res.append((out, nb))
    b.pcm_segments(np.zeros(S, np.int64), 0)        # (what is set after a submit does not reach it)
    b.wait_host(), t.wait_host()
    for c, counts in enumerate(SUBMITS):
        (out, nb), (wout, wnb) = got[c], want[c]
        assert (nb == wnb).all() and nb.sum() > 0, "host submit %d" % c
        assert all(out[s, :nb[s]].tobytes() == wout[s, :nb[s]].tobytes() for s in range(S)), "host submit %d" % c
    feed16 = Feed(ch, 9, np.int16, seed=970)
    got, want = [], []
    for c, counts in enumerate(SUBMITS[::-1]):
        parts = feed16.take(counts)
        off, total = spaced(parts, [2 * ((i + 3 * c) % 8) for i in range(S)], np.int16, descending=c == 2)
        b.frame_counts(counts), t.frame_counts(counts)
        b.pcm_segments(off, total)
        got.append(call(b, image_of(parts, off, total, np.int16), nf, submit=True))
        want.append(call(t, rows_of(parts, nf, 2, np.int16), nf, submit=True))
    b.pcm_segments(None)
    b.wait(None), t.wait(None)
    torch.cuda.synchronize()
    for c in range(3):
        r = result(got[c])
        assert r == result(want[c]) and sum(len(x) for x in r) > 0, "device submit %d" % c
    assert b.status() == 0 and t.status() == 0      # (checkpoints: not compared behind host submits, see above)
    b.close(), t.close()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_the_dc_blocker_reads_the_spread_rows(f32):
    """a batch with filter_select = 1 streams (k_dcfilter in front of the polyphase), under counts, two calls"""
    a = api
    dtype, nf, counts = (np.float32 if f32 else np.int16), 3, [[3, 1, 2, 0], [1, 3, 0, 2]]
    menu = [dict(bitrate=64, filter_select=1), STEREO, dict(bitrate=64, filter_select=1), STEREO]
    b, t = (a.Batch(controls(menu), max_frames=nf) for _ in range(2))
    feed = Feed([2] * 4, 6, dtype, seed=980)
    for c in counts:
        parts = feed.take(c)
        b.frame_counts(c), t.frame_counts(c)
        off, total = spaced(parts, [6, 0, 12, 8] if not f32 else [4, 0, 12, 8], dtype)
        b.pcm_segments(off, total)
        got = device_call(b, image_of(parts, off, total, dtype), nf)
        assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf)
    assert states(b) == states(t)
    b.close(), t.close()


@pytest.mark.one_k6_build
def test_a_batch_of_an_mpeg1_and_an_mpeg2_entry():
    """hx_batch_create_any with an MPEG-1 and an MPEG-2 entry (two frames per block there), one of them mono, under counts"""
    a = api
    nf, menu, cfg = 3, [STEREO, dict(bitrate=32, samprate=22050), dict(bitrate=32, samprate=22050, mode=3)], [0, 1, 2, 1, 0]
    b, t = (a.Batch.any(controls(menu), 5, cfg=cfg, max_frames=nf) for _ in range(2))
    ch = [b.stream_channels(i) for i in range(5)]
    assert ch == [2, 2, 1, 2, 2] and b.stream_frames_per_block(1) == 2
    feed = Feed(ch, 6, np.int16, seed=990, sr=[menu[k].get("samprate", 44100) for k in cfg])
    for c in ([2, 3, 1, 0, 3], [3, 0, 2, 3, 1]):
        parts = feed.take(c)
        b.frame_counts(c), t.frame_counts(c)
        off, total = b.packed_layout(nf)
        b.pcm_segments(off, total)
        got = device_call(b, image_of(parts, off, total, np.int16), nf)
        assert got == device_call(t, rows_of(parts, nf, 2, np.int16), nf)
    assert states(b) == states(t)
    b.close(), t.close()


def test_multi_blocks_read_one_image():
    """hx_multi_pcm_segments: 5 streams of a mixed menu in two blocks (3 + 2) on device 0; the offsets address the caller's
    one image, each block copies its own span, and every block's result equals the twin's"""
    a = api
    nf, cfg = 3, [0, 1, 1, 0, 1]
    m, t = (a.Multi.mixed(controls([STEREO, MONO]), 5, cfg=cfg, max_frames=nf, devices=[0, 0]) for _ in range(2))
    assert [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    ch = [m.stream_channels(i) for i in range(5)]
    feed = Feed(ch, 6, np.float32, seed=1000)
    for c, counts in enumerate([[3, 0, 2, 1, 3], [0, 3, 1, 2, 0]]):
        parts = feed.take(counts)
        m.frame_counts(counts), t.frame_counts(counts)
        if c == 0:
            off, total = m.packed_layout(nf, True)
        else:
            off, total = spaced(parts, [4, 8, 0, 12, 4], np.float32, descending=True)
        m.pcm_segments(off, total)
        got = m.encode_host_image(image_of(parts, off, total, np.float32), nf, stats=True, crc=True)
        want = t.encode_host(rows_of(parts, nf, 2, np.float32), stats=True, crc=True)
        assert m.status() == 0 and got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), "call %d" % c
        assert sum(len(x) for x in got[0]) > 0
    # a segment of the second block's that ends beyond the image: refused for both blocks, named by the caller's number
    parts = feed.take([1] * 5)
    m.frame_counts([1] * 5), t.frame_counts([1] * 5)
    off, total = m.packed_layout(nf, True)
    m.pcm_segments(off, total - 4)
    with pytest.raises(RuntimeError, match="stream 4: PCM segment"):
        m.encode_host_image(image_of(parts, off, total, np.float32), nf)
    m.pcm_segments(None)
    assert m.encode_host(rows_of(parts, nf, 2, np.float32)) == t.encode_host(rows_of(parts, nf, 2, np.float32))
    m.close(), t.close()


def test_refusals_name_the_stream_and_leave_the_batch_usable():
    """an offset that is no multiple of the sample size, a segment that ends beyond in_bytes and a negative offset are each
    refused with the stream's number, by the device and by the host call; the offset of a stream that takes no frame is not
    looked at; after every refusal the batch encodes the twin's bytes, and pcm_segments(None) restores rows"""
    a = api
    S, nf = 4, 2
    b, t = (a.Batch(a.default_control(**STEREO), nstreams=S, max_frames=nf) for _ in range(2))
    feed = Feed([2] * S, 8, np.float32, seed=1010)
    good, total = b.packed_layout(nf, True)
    cases = [(2, int(good[2]) + 2, total, "no multiple"), (3, int(good[3]), total - 4, "ends beyond in_bytes"), (1, -4, total, "is negative")]
    for s, o, nbytes, what in cases:
        off = good.copy()
        off[s] = o
        b.pcm_segments(off, nbytes)
        junk = np.zeros(total // 4, np.float32)
        before = states(b)
        with pytest.raises(RuntimeError, match="stream %d: PCM segment" % s) as e:
            device_call(b, junk, nf)
        assert what in str(e.value)
        with pytest.raises(RuntimeError, match="stream %d: PCM segment" % s):
            b.encode_host_image(junk, nf)
        assert states(b) == before, "a refused call moved a stream"
        # the same offset under a count of 0 for that stream is not looked at
        counts = [nf] * S
        counts[s] = 0
        parts = feed.take(counts)
        b.frame_counts(counts), t.frame_counts(counts)
        b.pcm_segments(off, total)
        assert device_call(b, image_of([p for p in parts if len(p)], [x for x, p in zip(off, parts) if len(p)], total, np.float32), nf) == \
            device_call(t, rows_of(parts, nf, 2, np.float32), nf), what
        b.frame_counts(None), t.frame_counts(None)
    b.pcm_segments(None)
    parts = feed.take([nf] * S)
    assert device_call(b, rows_of(parts, nf, 2, np.float32), nf) == device_call(t, rows_of(parts, nf, 2, np.float32), nf)
    assert states(b) == states(t)
    b.close(), t.close()


@pytest.mark.one_k6_build
def test_a_converting_batch_takes_no_segments():
    a = api
    sb = a.SrcBatch(a.default_control(bitrate=64, samprate=48000), a.Source(16, 0, 0, 0), nstreams=2, max_frames=2)
    with pytest.raises(RuntimeError, match="converting batch"):
        sb.pcm_segments([0, 4608], 9216)
    sb.close()
