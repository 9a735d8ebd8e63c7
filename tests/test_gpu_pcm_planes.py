"""PCM planes (hx_batch_pcm_planes, hx_multi_pcm_planes, k_pcm_planes) on a real MI355X: a call's input as one image of
channel planes that the GPU interleaves into the rows the front end reads.

Every comparison is equality against a twin batch of the same controls, made the same way and fed rows built from the same
samples - the route that exists: the rows' used parts, out_bytes, and the "pcmrows" tap by bit pattern.  Samples, images and
the twin's rows come from tests/pcm_planes_cases.py; whatever belongs to no plane is a poison.  Device calls write into zeroed
rows, so the streams' checkpoints can be compared across the two batches (behind host calls they are not: a host call's rows
are device staging that nobody zeroes).  The planes have nothing to do with the stream walk's build: the module runs once.
k_pcm_planes' chunk is 16 KB (HX_PCM_CHUNK), the size the chunk-edge test's rows are chosen for."""
import numpy as np
import pytest

import gpu_support as G
from gpu_support import CallBufs, Pinned, controls, states, sync
from hmp3_amd import api
from pcm_planes_cases import Feed, image_of, row_of, rows_of, spaced

pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
FILL = 0xA5
STEREO, MONO = dict(bitrate=64), dict(bitrate=64, mode=3)
S16, F32 = np.int16, np.float32
DT = pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def tap(b, dtype, S, nf, P=2):
    """the "pcmrows" tap after a call of nf frames: [S, nf * 1152 * P] samples"""
    return b.debug_read("pcmrows", dtype, S * nf * 1152 * P).reshape(S, -1).copy()


def tap_holds(rows, parts, what=""):
    for s, part in enumerate(parts):
        r = row_of(part) if part else np.zeros(0, rows.dtype)
        assert (bits(rows[s, :len(r)]) == bits(r)).all(), "%s stream %d: the interleaved row" % (what, s)


def host_crc_call(b, pcm, nf):
    """hx_batch_encode_f32_host_crc into prefilled host buffers -> (return code, rows, out_bytes, stats, crc)"""
    stride = b.out_stride(nf)
    out, nb = np.full((b.n, stride), FILL, np.uint8), np.full(b.n, -1, np.int32)
    st, cr = np.full((b.n, nf, 2), -1, np.int32), np.full((b.n, nf), 0xFFFF, np.uint16)
    pcm = np.ascontiguousarray(pcm, dtype=np.float32)
    rc = api.lib().hx_batch_encode_f32_host_crc(b.h, pcm.ctypes.data, nf, out.ctypes.data, stride, nb.ctypes.data, st.ctypes.data, cr.ctypes.data)
    return rc, out, nb, st, cr


def pair(menu=None, S=None, cfg=None, nf=2, make=None):
    """the batch under test and its twin"""
    a = api
    if make:
        return make(), make()
    if cfg is None:
        return tuple(a.Batch(a.default_control(**(menu or STEREO)), nstreams=S, max_frames=nf) for _ in range(2))
    return tuple(a.Batch.mixed(controls(menu), S, cfg=cfg, max_frames=nf) for _ in range(2))


# ---- 1. the tight [S, C, T] image ----

@DT
def test_tight_s_c_t_image_equals_rows_call_after_call(f32):
    """4 stereo streams, three device calls of 2 frames fed the tight planar image (planar_layout; chan_stride NULL): rows and
    byte counts of every call and the checkpoints at the end equal the twin's"""
    dtype, S, nf = (F32 if f32 else S16), 4, 2
    b, t = pair(S=S, nf=nf)
    feed = Feed([2] * S, 6, dtype)
    off, stride, total = api.planar_layout(nf, [2] * S, None, f32)
    assert list(stride) == [nf * 1152 * (4 if f32 else 2)] * S and total == S * 2 * stride[0]
    b.pcm_planes(off, None, total)
    for c in range(3):
        parts = feed.take([nf] * S)
        got = device_call(b, image_of(parts, off, stride, total, dtype), nf)
        want = device_call(t, rows_of(parts, nf, 2, dtype), nf)
        assert got == want, "call %d" % c
    assert sum(len(w) for w in want) > 0
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 2. every pair of plane residues ----

@DT
def test_every_pair_of_plane_residues(f32):
    """one stream per pair (start of plane 0, start of plane 1) modulo 16 - 8 x 8 for int16, 4 x 4 for fp32 -, one frame,
    poisoned gaps, the device image's base itself one sample (2 or 4 bytes) past a 16-byte boundary"""
    dtype, item = (F32 if f32 else S16), (4 if f32 else 2)
    res = list(range(0, 16, item))
    pairs = [(r0, r1) for r0 in res for r1 in res]
    S, nf = len(pairs), 1
    assert S == (16 if f32 else 64)
    b, t = pair(S=S, nf=nf)
    parts = Feed([2] * S, nf, dtype, seed=1920).take([nf] * S)
    off, stride, total = spaced(parts, [p[0] for p in pairs], [p[1] for p in pairs], dtype)
    assert sorted(set((int(o) % 16, int(o + d) % 16) for o, d in zip(off, stride))) == sorted(pairs)
    b.pcm_planes(off, stride, total)
    got = device_call(b, image_of(parts, off, stride, total, dtype), nf, shift=1)
    tap_holds(tap(b, dtype, S, nf), parts)
    assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf)
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 3. chunk edges ----

@DT
def test_chunk_edges(f32):
    """the smallest rows that cross 16 KB, 18432 bytes each: a stereo stream at 4 (int16) / 2 (fp32) frames and a mono stream
    under planes at 8 / 4 frames, beside a stream of one frame; unaligned planes; the tap compared whole up to len_s"""
    dtype, nf = (F32 if f32 else S16), (4 if f32 else 8)
    counts, ch = [nf // 2, nf, 1, 1], [2, 1, 2, 1]
    b, t = pair([STEREO, MONO], 4, [0, 1, 0, 1], nf)
    parts = Feed(ch, nf, dtype, seed=1930).take(counts)
    assert [row_of(p).nbytes for p in parts] == [18432, 18432, 2304 * (4 if f32 else 2), 1152 * (4 if f32 else 2)]
    for x in (b, t):
        x.frame_counts(counts)
    off, stride, total = spaced(parts, [4, 12, 0, 8], [8, 0, 4, 0], dtype)
    b.pcm_planes(off, stride, total)
    got = device_call(b, image_of(parts, off, stride, total, dtype), nf)
    tap_holds(tap(b, dtype, 4, nf), parts)
    assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf)
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 4. no store behind len_s or in another row ----

@DT
def test_no_store_lands_behind_len_s_or_in_another_row(f32):
    """call A at full counts, then call B with smaller counts and other samples: every row holds B's samples in its first
    len_s bytes and, from there to its end, exactly what call A left there"""
    dtype, S, nf, ch = (F32 if f32 else S16), 6, 3, [2, 1, 2, 1, 2, 1]
    b = api.Batch.mixed(controls([STEREO, MONO]), S, cfg=[0, 1] * 3, max_frames=nf)
    feed = Feed(ch, 6, dtype, seed=1940)
    item = 4 if f32 else 2

    def one(counts):
        parts = feed.take(counts)
        b.frame_counts(counts)
        off, stride, total = spaced(parts, [item * i % 16 for i in range(S)], [item * (i + 3) % 16 for i in range(S)], dtype)
        b.pcm_planes(off, stride, total)
        device_call(b, image_of(parts, off, stride, total, dtype), nf)
        return parts, tap(b, dtype, S, nf)

    pa, ra = one([nf] * S)
    tap_holds(ra, pa, "call A")
    pb, rb = one([1, 2, 0, 0, 2, 1])
    tap_holds(rb, pb, "call B")
    for s in range(S):
        n = len(row_of(pb[s]))
        assert (bits(rb[s, n:]) == bits(ra[s, n:])).all(), "call B stream %d: bytes stored behind len_s" % s
    assert len(pb[2][0]) == 0 and (bits(rb[2]) == bits(ra[2])).all()
    b.close()


# ---- 5. strides ----

@DT
def test_c_s_t_negative_zero_and_shared_strides(f32):
    """four layouts of one image family, each against the twin fed the interleaved rows: [C, S, T] (a stream's planes S planes
    apart); a negative stride with plane 1 in front of plane 0; stride 0, which is rows with L = R; two streams sharing both
    planes"""
    dtype, item, S, nf = (F32 if f32 else S16), (4 if f32 else 2), 4, 2
    b, t = pair(S=S, nf=nf)
    feed = Feed([2] * S, 8, dtype, seed=1950)
    plen = nf * 1152 * item
    # [C, S, T]
    parts = feed.take([nf] * S)
    off, stride, total = np.arange(S, dtype=np.int64) * plen, np.full(S, S * plen, np.int64), 2 * S * plen
    b.pcm_planes(off, stride, total)
    assert device_call(b, image_of(parts, off, stride, total, dtype), nf) == device_call(t, rows_of(parts, nf, 2, dtype), nf), "[C, S, T]"
    # plane 1 in front of plane 0
    parts = feed.take([nf] * S)
    off, stride, total = spaced(parts, [0, item, 8, 12], [item, 0, 12, 8], dtype, swap=range(S))
    assert (stride < 0).all()
    b.pcm_planes(off, stride, total)
    assert device_call(b, image_of(parts, off, stride, total, dtype), nf) == device_call(t, rows_of(parts, nf, 2, dtype), nf), "negative stride"
    # stride 0: both channels read plane 0
    parts = feed.take([nf] * S)
    off, stride, total = np.arange(S, dtype=np.int64) * (plen + 16) + item, np.zeros(S, np.int64), S * (plen + 16) + 16
    b.pcm_planes(off, stride, total)
    got = device_call(b, image_of([p[:1] for p in parts], off, stride, total, dtype), nf)
    assert got == device_call(t, rows_of([[p[0], p[0]] for p in parts], nf, 2, dtype), nf), "stride 0"
    # streams 2 and 3 read stream 1's planes (streams 0 and 1 so far in step: same control, but their own histories)
    parts = feed.take([nf] * S)
    parts[2] = parts[3] = parts[1]
    off, stride, total = spaced(parts[:2], [item, 8], [12, 0], dtype)
    off, stride = np.append(off, [off[1]] * 2), np.append(stride, [stride[1]] * 2)
    b.pcm_planes(off, stride, total)
    got = device_call(b, image_of(parts[:2], off, stride, total, dtype), nf)
    assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf) and sum(len(x) for x in got) > 0, "shared planes"
    assert states(b) == states(t)
    b.close(), t.close()


def test_a_mono_stride_and_a_sitting_streams_offset_are_not_looked_at():
    """a mono stream whose chan_stride would put a second plane far outside the image, and a stream with count 0 whose
    offset and stride are wild: the call is made and equals the twin's"""
    S, nf, ch, counts = 4, 2, [2, 1, 2, 1], [2, 2, 0, 1]
    b, t = pair([STEREO, MONO], S, [0, 1, 0, 1], nf)
    parts = Feed(ch, nf, S16, seed=1960).take(counts)
    for x in (b, t):
        x.frame_counts(counts)
    off, stride, total = spaced(parts, [2, 6, 0, 10], [14, 0, 0, 0], S16)
    stride[1], stride[3], off[2], stride[2] = -(1 << 40), (1 << 50) + 1, -(1 << 45) + 1, 1 << 55
    b.pcm_planes(off, stride, total)
    got = device_call(b, image_of(parts, off, stride * np.array([1, 0, 0, 0]), total, S16), nf)
    assert got == device_call(t, rows_of(parts, nf, 2, S16), nf) and got[2] == b""
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 6. a mixed batch under counts through the host *_crc call ----

def test_mixed_batch_under_counts_through_the_host_crc_call():
    """8 slots alternating stereo and mono under per-stream counts, fp32 planes in descending order with gaps through
    hx_batch_encode_f32_host_crc (the span copy): rows, out_bytes, frame counters and CRCs equal the twin's"""
    S, nf, ch = 8, 3, [2, 1] * 4
    b, t = pair([STEREO, MONO], S, [0, 1] * 4, nf)
    feed = Feed(ch, 8, F32, seed=1970)
    for c, counts in enumerate([[3, 0, 1, 2, 3, 1, 0, 2], [0, 3, 2, 0, 1, 3, 3, 1]]):
        parts = feed.take(counts)
        for x in (b, t):
            x.frame_counts(counts)
        off, stride, total = spaced(parts, [4 * (i + c) % 16 for i in range(S)], [4 * (3 * i + 1) % 16 for i in range(S)], F32, descending=True,
                                    swap=(0, 4) if c else ())
        live = [i for i in range(S) if counts[i]]
        assert all(off[i] > off[j] for i, j in zip(live, live[1:]))
        b.pcm_planes(off, stride, total)
        rc, out, nb, st, cr = host_crc_call(b, image_of(parts, off, stride, total, F32), nf)
        assert rc == 0 and b.status() == 0, api.last_error()
        rc, wout, wnb, wst, wcr = host_crc_call(t, rows_of(parts, nf, 2, F32), nf)
        assert rc == 0 and t.status() == 0, api.last_error()
        assert (nb == wnb).all() and (st == wst).all() and (cr == wcr).all(), "call %d" % c
        for s, n in enumerate(counts):
            assert out[s, :nb[s]].tobytes() == wout[s, :wnb[s]].tobytes(), "call %d stream %d" % (c, s)
            if n == 0:
                assert nb[s] == 0 and (out[s] == FILL).all()
        assert nb.sum() > 0
        tap_holds(tap(b, F32, S, nf), parts, "call %d" % c)
    b.close(), t.close()


# ---- 7. unit scale ----

def test_unit_scale_equals_the_scaled_rows_and_a_converting_batch():
    """fp32 planes in [-1, 1) under unit_scale: the bytes equal the twin fed np.float32(x) * np.float32(32768) as rows, and a
    converting batch (32-bit float source at the encoder's rate, no mono convert) fed the same unit-scale samples interleaved"""
    a = api
    S, nf = 3, 2
    b, t = pair(S=S, nf=nf)
    conv = a.SrcBatch(a.default_control(**STEREO), a.Source(32, 1, 0, 0), nstreams=S, max_frames=nf)
    rng = np.random.default_rng(1980)
    parts = Feed([2] * S, nf, F32, seed=1980).take([nf] * S)
    # unit-scale samples that do not all come back as they were at int16 scale: a random last bit here and there
    unit = [[(p / np.float32(32768)) * (np.float32(1) + rng.integers(0, 2, len(p)).astype(np.float32) * np.float32(2.0 ** -23)) for p in part] for part in parts]
    assert all(p.dtype == np.float32 and np.abs(p).max() < 1 for part in unit for p in part)
    scaled = [[np.float32(1) * p * np.float32(32768) for p in part] for part in unit]
    off, stride, total = spaced(unit, [4, 0, 12], [8, 12, 0], F32)
    b.pcm_planes(off, stride, total, unit_scale=True)
    got = device_call(b, image_of(unit, off, stride, total, F32), nf)
    tap_holds(tap(b, F32, S, nf), scaled)
    assert got == device_call(t, rows_of(scaled, nf, 2, F32), nf) and sum(len(x) for x in got) > 0
    assert states(b) == states(t)
    rows = np.zeros((S, conv.in_stride(nf)), np.uint8)
    for s, part in enumerate(unit):
        r = row_of(part).view(np.uint8)
        rows[s, :len(r)] = r
    want, used = conv.encode_src_host(rows, nf)
    assert list(used) == [nf * 1152 * 2 * 4] * S and conv.status() == 0
    assert got == want, "the converting batch's bytes"
    b.close(), t.close(), conv.close()


def test_unit_scale_by_bit_pattern():
    """the tap after a unit-scale call whose planes hold -0.0, subnormal inputs (1e-42, 1e-39, 2^-141, 2^-149: kept, not
    flushed), +-2^-126, +-65535 (2^16 x full scale, the top of the range the encoder is held over) and ordinary values: every
    row sample is the one IEEE product x * 32768.0f; and the same planes with unit_scale = 0 arrive unchanged.
    The largest float, whose product is an infinity, is not fed to a whole call: the next test holds it through the row
    kernel alone, and says why."""
    S, nf = 2, 1
    b = api.Batch(api.default_control(**STEREO), nstreams=S, max_frames=nf)
    special = np.array([-0.0, 0.0, 1e-42, -1e-42, 1e-39, -1e-39, 65535.0, -65535.0, 2.0 ** -126, -2.0 ** -126,
                        2.0 ** -141, 2.0 ** -149, 0.999999, -1.0, 1.0 / 3, 3e-5], np.float32)
    assert (np.abs(special[2:6]) < np.finfo(np.float32).tiny).all() and (special[2:6] != 0).all(), "the test's subnormals were flushed on the host"
    rng = np.random.default_rng(1990)
    parts = [[np.resize(np.roll(special, s + 3 * c), 1152) * np.float32(1) for c in range(2)] for s in range(S)]
    for s in range(S):
        parts[s][1][500:] = rng.uniform(-1, 1, 652).astype(np.float32)
    scaled = [[p * np.float32(32768) for p in part] for part in parts]
    assert (bits(scaled[0][0]) == 0x80000000).any() and np.isfinite(scaled[0][0]).all() and (scaled[0][0] == np.float32(2.0 ** -134)).any()
    off, stride, total = spaced(parts, [4, 8], [12, 0], F32)
    img = image_of(parts, off, stride, total, F32)
    for unit, want in ((True, scaled), (False, parts)):
        b.pcm_planes(off, stride, total, unit_scale=unit)
        call(b, img, nf)
        sync()
        tap_holds(tap(b, F32, S, nf), want, "unit_scale = %d" % unit)
    b.close()


def test_unit_scale_overflow_by_bit_pattern_through_the_row_kernel_alone():
    """the largest float, +-2^113 (the smallest magnitudes whose product overflows) and their lower neighbours under
    unit_scale, in a stereo and in a mono stream: every row sample is numpy's float32 product by bit pattern - +-infinity
    for the first two.  The rows are made by hx_batch_debug_pcm_rows, the call's checks, layout upload and row kernel with
    nothing behind them, and read with the "pcmrows" tap; no stream moves, and the batch then encodes what its twin does.
    Why not a whole call: one infinite sample is outside what the encoder behind the row kernel defines, and the CPU
    restatement shows what that means - oracle.OracleEncoder.encode_f32 fed one infinite sample in a stream dies of a
    segmentation fault in quant_opt (oracle/hxo_alloc.c, the reference's l3math.c:675-694): the spectrum is NaN, (int) of
    it is INT_MIN, the index is clamped from above only, and hxo_quant_off[INT_MIN] is read.  The stream walk restates that
    arithmetic (trade_dual in hx_alloc2.inc clamps the same index from above only), so on the GPU such a call reads out
    of bounds; it is not made."""
    S, nf = 2, 1
    b, t = pair([STEREO, MONO], S, [0, 1], nf)
    big = np.float32(np.finfo(np.float32).max)
    edge = np.float32(2.0 ** 113)
    special = np.array([big, -big, edge, -edge, np.nextafter(edge, np.float32(0)), -np.nextafter(edge, np.float32(0)), 1e-42, -0.0, 0.5, -1.0], np.float32)
    parts = [[np.resize(np.roll(special, c), 1152) for c in range(2)], [np.resize(np.roll(special, 5), 1152)]]
    with np.errstate(over="ignore"):
        scaled = [[p * np.float32(32768) for p in part] for part in parts]
    assert (bits(scaled[0][0]) == 0x7F800000).sum() >= 200 and (bits(scaled[1][0]) == 0xFF800000).sum() >= 200
    assert np.isfinite(np.nextafter(edge, np.float32(0)) * np.float32(32768))
    off, stride, total = spaced(parts, [4, 8], [12, 0], F32)
    img = image_of(parts, off, stride, total, F32)
    import torch
    d = torch.zeros(img.size + 4, dtype=torch.float32, device=G.dev())
    d[1:1 + img.size] = torch.from_numpy(img).to(G.dev())                   # (the image's base 4 bytes past a 16-byte boundary)
    before = states(b)
    with pytest.raises(RuntimeError, match="segments or PCM planes in force"):
        b.debug_pcm_rows(d.data_ptr() + 4, nf, f32=True)
    for unit, want in ((True, scaled), (False, parts)):
        b.pcm_planes(off, stride, total, unit_scale=unit)
        b.debug_pcm_rows(d.data_ptr() + 4, nf, f32=True)
        sync()
        tap_holds(tap(b, F32, S, nf), want, "unit_scale = %d" % unit)
    assert b.status() == 0 and states(b) == before, "the row kernel alone moved a stream"
    b.pcm_planes(None)
    rows = rows_of(Feed([2, 1], nf, F32, seed=1995).take([nf] * S), nf, 2, F32)
    assert device_call(b, rows, nf) == device_call(t, rows, nf)
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 8. planes travel with their submit ----

PIN = Pinned()         # (kept until the module's teardown releases it)
pinned = PIN.copy


@pytest.fixture(scope="module", autouse=True)
def _release_pinned():
    yield
    PIN.free()


SUBMITS = [[3, 1, 0, 2, 3, 2], [1, 3, 2, 0, 1, 3], [2, 0, 3, 3, 0, 1]]


def test_planes_travel_with_their_submit():
    """three hx_batch_submit_f32_host calls and a wait, then three hx_batch_submit_s16_device calls and a wait: every submit
    under other counts, offsets and strides, the setters called between the submits while the earlier ones are in flight -
    the rows of all six equal the twin's, which makes the same submits fed rows"""
    import torch
    S, nf, ch = 6, 3, [2, 1] * 3
    b, t = pair([STEREO, MONO], S, [0, 1] * 3, nf)
    stride_out = b.out_stride(nf)
    feed = Feed(ch, 9, F32, seed=2000)
    got, want = [], []
    for c, counts in enumerate(SUBMITS):
        parts = feed.take(counts)
        off, stride, total = spaced(parts, [4 * ((i + c) % 4) for i in range(S)], [4 * ((i + 2 * c + 1) % 4) for i in range(S)], F32, descending=c == 1,
                                    swap=(0, 2) if c == 2 else ())
        for x, pcm, res in ((b, image_of(parts, off, stride, total, F32), got), (t, rows_of(parts, nf, 2, F32), want)):
            x.frame_counts(counts)
            if x is b:
                x.pcm_planes(off, stride, total)
            pcm, out, nb = pinned(pcm), pinned(np.zeros((S, stride_out), np.uint8)), pinned(np.full(S, -1, np.int32))
            x.submit_host(pcm.ctypes.data, nf, out.ctypes.data, stride_out, nb.ctypes.data, f32=True)
            res.append((out, nb))
    b.pcm_planes(np.zeros(S, np.int64), np.zeros(S, np.int64), 0)        # (what is set after a submit does not reach it)
    b.wait_host(), t.wait_host()
    for c, counts in enumerate(SUBMITS):
        (out, nb), (wout, wnb) = got[c], want[c]
        assert (nb == wnb).all() and nb.sum() > 0, "host submit %d" % c
        assert all(out[s, :nb[s]].tobytes() == wout[s, :nb[s]].tobytes() for s in range(S)), "host submit %d" % c
    feed16 = Feed(ch, 9, S16, seed=2010)
    got, want = [], []
    for c, counts in enumerate(SUBMITS[::-1]):
        parts = feed16.take(counts)
        off, stride, total = spaced(parts, [2 * ((i + 3 * c) % 8) for i in range(S)], [2 * ((5 * i + c) % 8) for i in range(S)], S16, descending=c == 2)
        b.frame_counts(counts), t.frame_counts(counts)
        b.pcm_planes(off, stride, total)
        got.append(call(b, image_of(parts, off, stride, total, S16), nf, submit=True))
        want.append(call(t, rows_of(parts, nf, 2, S16), nf, submit=True))
    b.pcm_planes(None)
    b.wait(None), t.wait(None)
    torch.cuda.synchronize()
    for c in range(3):
        r = result(got[c])
        assert r == result(want[c]) and sum(len(x) for x in r) > 0, "device submit %d" % c
    assert b.status() == 0 and t.status() == 0
    b.close(), t.close()


# ---- 9. the DC blocker, and a batch of an MPEG-1 and an MPEG-2 entry ----

@DT
def test_the_dc_blocker_reads_the_interleaved_rows(f32):
    """a batch with filter_select = 1 streams (k_dcfilter in front of the polyphase), under counts, two calls"""
    dtype, item, nf, counts = (F32 if f32 else S16), (4 if f32 else 2), 3, [[3, 1, 2, 0], [1, 3, 0, 2]]
    menu = [dict(bitrate=64, filter_select=1), STEREO, dict(bitrate=64, filter_select=1), STEREO]
    b, t = (api.Batch(controls(menu), max_frames=nf) for _ in range(2))
    feed = Feed([2] * 4, 6, dtype, seed=2020)
    for c in counts:
        parts = feed.take(c)
        b.frame_counts(c), t.frame_counts(c)
        off, stride, total = spaced(parts, [item, 0, 12, 8], [8, item, 0, 12], dtype)
        b.pcm_planes(off, stride, total)
        got = device_call(b, image_of(parts, off, stride, total, dtype), nf)
        assert got == device_call(t, rows_of(parts, nf, 2, dtype), nf)
    assert states(b) == states(t)
    b.close(), t.close()


def test_a_batch_of_an_mpeg1_and_an_mpeg2_entry():
    """hx_batch_create_any with an MPEG-1 and an MPEG-2 entry (two frames per block there), one of them mono, under counts,
    fed the tight planar layout of the counts in force"""
    a = api
    nf, menu, cfg = 3, [STEREO, dict(bitrate=32, samprate=22050), dict(bitrate=32, samprate=22050, mode=3)], [0, 1, 2, 1, 0]
    b, t = (a.Batch.any(controls(menu), 5, cfg=cfg, max_frames=nf) for _ in range(2))
    ch = [b.stream_channels(i) for i in range(5)]
    assert ch == [2, 2, 1, 2, 2] and b.stream_frames_per_block(1) == 2
    feed = Feed(ch, 6, S16, seed=2030, sr=[menu[k].get("samprate", 44100) for k in cfg])
    for c in ([2, 3, 1, 0, 3], [3, 0, 2, 3, 1]):
        parts = feed.take(c)
        b.frame_counts(c), t.frame_counts(c)
        off, stride, total = a.planar_layout(nf, ch, c)
        b.pcm_planes(off, None, total)
        got = device_call(b, image_of(parts, off, stride, total, S16), nf)
        assert got == device_call(t, rows_of(parts, nf, 2, S16), nf)
    assert states(b) == states(t)
    b.close(), t.close()


# ---- 10. hx_multi ----

def test_multi_blocks_read_one_image():
    """hx_multi_pcm_planes: 5 streams of a mixed menu in two blocks (3 + 2) on device 0; offsets and strides address the
    caller's one image, each block copies its own span, and every block's result equals the twin's; a plane of the second
    block's that ends beyond the image is refused for both blocks and named by the caller's stream number"""
    a = api
    nf, cfg = 3, [0, 1, 1, 0, 1]
    m, t = (a.Multi.mixed(controls([STEREO, MONO]), 5, cfg=cfg, max_frames=nf, devices=[0, 0]) for _ in range(2))
    assert [m.shard(k)[1:] for k in range(2)] == [(0, 3), (3, 2)]
    ch = [m.stream_channels(i) for i in range(5)]
    feed = Feed(ch, 7, F32, seed=2040)
    for c, counts in enumerate([[3, 0, 2, 1, 3], [0, 3, 1, 2, 0]]):
        parts = feed.take(counts)
        m.frame_counts(counts), t.frame_counts(counts)
        if c == 0:
            off, stride, total = a.planar_layout(nf, ch, counts, True)
            m.pcm_planes(off, None, total)
        else:
            off, stride, total = spaced(parts, [4, 8, 0, 12, 4], [0, 0, 0, 8, 0], F32, descending=True, swap=(3,))
            m.pcm_planes(off, stride, total)
        got = m.encode_host_image(image_of(parts, off, stride, total, F32), nf, stats=True, crc=True)
        want = t.encode_host(rows_of(parts, nf, 2, F32), stats=True, crc=True)
        assert m.status() == 0 and got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), "call %d" % c
        assert sum(len(x) for x in got[0]) > 0
    parts = feed.take([1] * 5)
    m.frame_counts([1] * 5), t.frame_counts([1] * 5)
    off, stride, total = a.planar_layout(nf, ch, [1] * 5, True)
    m.pcm_planes(off, stride, total - 4)
    with pytest.raises(RuntimeError, match="stream 4 channel 0: PCM plane"):
        m.encode_host_image(image_of(parts, off, stride, total, F32), nf)
    m.pcm_planes(None)
    assert m.encode_host(rows_of(parts, nf, 2, F32)) == t.encode_host(rows_of(parts, nf, 2, F32))
    m.close(), t.close()


# ---- 11. refusals ----

def test_refusals_name_stream_and_channel_and_leave_the_batch_usable():
    """an offset that is no multiple of the sample size, a plane that starts below 0 through a negative stride, a plane that
    ends beyond in_bytes: each refused with stream and channel, by the device and by the host call, nothing moved; unit_scale
    = 2 refused by the setter, which changes nothing; an s16 call under unit_scale = 1 refused by name; after every refusal
    the batch encodes the twin's bytes"""
    S, nf = 4, 2
    b, t = pair(S=S, nf=nf)
    feed = Feed([2] * S, 16, F32, seed=2050)
    good, gstride, total = api.planar_layout(nf, [2] * S, None, True)
    plen = int(gstride[0])

    def ok():
        parts = feed.take([nf] * S)
        b.pcm_planes(good, gstride, total)
        assert device_call(b, image_of(parts, good, gstride, total, F32), nf) == device_call(t, rows_of(parts, nf, 2, F32), nf)

    cases = [(2, 0, int(good[2]) + 2, plen, total, "no multiple"), (1, 1, int(good[1]), plen + 2, total, "no multiple"),
             (0, 1, plen - 4, -plen, total, "starts below 0"), (3, 1, int(good[3]), plen, total - 4, "ends beyond in_bytes"),
             (3, 0, total, -plen, total, "ends beyond in_bytes")]
    junk = np.zeros(total // 4, np.float32)
    for s, c, o, d, nbytes, what in cases:
        off, stride = good[:S].copy(), gstride.copy()
        off[s], stride[s] = o, d
        b.pcm_planes(off, stride, nbytes)
        before = states(b)
        with pytest.raises(RuntimeError, match="stream %d channel %d: PCM plane" % (s, c)) as e:
            device_call(b, junk, nf)
        assert what in str(e.value)
        with pytest.raises(RuntimeError, match="stream %d channel %d: PCM plane" % (s, c)):
            b.encode_host_image(junk, nf)
        assert states(b) == before, "a refused call moved a stream"
        ok()
    # the setter: unit_scale = 2 changes nothing - the planes of the last ok() stay, at int16 scale
    with pytest.raises(RuntimeError, match="unit_scale"):
        b.pcm_planes(good + 4, gstride, total + 4, unit_scale=2)
    parts = feed.take([nf] * S)
    assert device_call(b, image_of(parts, good, gstride, total, F32), nf) == device_call(t, rows_of(parts, nf, 2, F32), nf)
    # an s16 call under unit_scale = 1
    b.pcm_planes(good // 2, gstride // 2, total // 2, unit_scale=True)
    before = states(b)
    with pytest.raises(RuntimeError, match="s16 call under PCM planes with unit_scale"):
        device_call(b, np.zeros(total // 4, np.int16), nf)
    assert states(b) == before
    ok()
    assert states(b) == states(t)
    b.close(), t.close()


def test_planes_and_segments_replace_each_other():
    """planes set and then segments set give segments' behaviour, the reverse planes'; either setter with a null off gives
    rows back"""
    S, nf = 3, 2
    b, t = pair(S=S, nf=nf)
    feed = Feed([2] * S, 12, S16, seed=2060)
    poff, pstride, total = api.planar_layout(nf, [2] * S)
    soff, stotal = b.packed_layout(nf)
    assert stotal == total

    def seg_image(parts):
        return np.concatenate([row_of(p) for p in parts])

    def step(set_up, image):
        parts = feed.take([nf] * S)
        set_up()
        assert device_call(b, image(parts), nf) == device_call(t, rows_of(parts, nf, 2, S16), nf)

    planes = lambda parts: image_of(parts, poff, pstride, total, S16)
    rows = lambda parts: rows_of(parts, nf, 2, S16)
    step(lambda: (b.pcm_planes(poff, pstride, total), b.pcm_segments(soff, stotal)), seg_image)
    step(lambda: (b.pcm_segments(soff, stotal), b.pcm_planes(poff, pstride, total)), planes)
    step(lambda: b.pcm_segments(None), rows)
    step(lambda: (b.pcm_segments(soff, stotal), b.pcm_planes(None)), rows)
    step(lambda: b.pcm_planes(poff, None, total), planes)
    assert states(b) == states(t)
    b.close(), t.close()


def test_a_converting_batch_takes_no_planes():
    a = api
    sb = a.SrcBatch(a.default_control(bitrate=64, samprate=48000), a.Source(16, 0, 0, 0), nstreams=2, max_frames=2)
    with pytest.raises(RuntimeError, match="converting batch"):
        sb.pcm_planes([0, 4608], [2304, 2304], 9216)
    sb.close()


# ---- 12. Batch.encode_tensor ----

def test_encode_tensor():
    """a device [S, 2, T] float32 tensor in [-1, 1) gives the bytes of the twin fed interleaved int16-scale rows; so do a
    [C, S, T] tensor permuted to [S, C, T], a host tensor (the host call), and an int16 device tensor; a tensor whose last
    dimension has another stride than 1 is refused"""
    import torch
    S, nf = 3, 2
    b, t = pair(S=S, nf=nf)
    feed = Feed([2] * S, 10, F32, seed=2070)

    def tensors(parts, dtype):
        w = np.stack([np.stack(p) for p in parts])                      # [S, 2, T] at int16 scale
        return w, (torch.from_numpy(w / np.float32(32768)) if dtype == F32 else torch.from_numpy(w.astype(np.int16)))

    def on_device(w):
        o = CallBufs(b, nf)
        b.encode_tensor(w, o.ptr, o.stride, o.nb.data_ptr(), None)
        r = result(o)
        assert b.status() == 0
        return r

    parts = feed.take([nf] * S)
    w, x = tensors(parts, F32)
    assert x.dtype == torch.float32 and float(x.abs().max()) < 1
    assert on_device(x.to(G.dev())) == device_call(t, rows_of(parts, nf, 2, F32), nf), "[S, C, T]"
    parts = feed.take([nf] * S)
    w, x = tensors(parts, F32)
    cst = x.permute(1, 0, 2).contiguous().to(G.dev())                   # [C, S, T] in memory
    view = cst.permute(1, 0, 2)
    assert view.stride() == (nf * 1152, S * nf * 1152, 1) and view.data_ptr() == cst.data_ptr()
    assert on_device(view) == device_call(t, rows_of(parts, nf, 2, F32), nf), "[C, S, T] permuted"
    parts = feed.take([nf] * S)
    w, x = tensors(parts, F32)
    assert b.encode_tensor(x) == device_call(t, rows_of(parts, nf, 2, F32), nf), "host tensor"
    parts = feed.take([nf] * S)
    w, x = tensors(parts, S16)
    ints = [[p.astype(np.int16) for p in part] for part in parts]
    assert on_device(x.to(G.dev())) == device_call(t, rows_of(ints, nf, 2, S16), nf), "int16 tensor"
    # refusals come before the planes are set: the batch, switched back to rows, still takes rows afterwards
    b.pcm_planes(None)
    with pytest.raises(ValueError, match="stride 1"):
        b.encode_tensor(torch.zeros(S, nf * 1152, 2).permute(0, 2, 1))
    with pytest.raises(ValueError, match="d_out_ptr"):
        b.encode_tensor(torch.zeros(S, 2, nf * 1152, device=G.dev()))
    with pytest.raises(ValueError, match="channel"):
        b.encode_tensor(torch.zeros(S, nf * 1152))
    with pytest.raises(ValueError, match="max_frames"):
        b.encode_tensor(torch.zeros(S, 2, (nf + 1) * 1152))
    parts = feed.take([nf] * S)
    assert device_call(b, rows_of(parts, nf, 2, F32), nf) == device_call(t, rows_of(parts, nf, 2, F32), nf), "rows after refused tensors"
    b.close(), t.close()
    m = api.Batch(api.default_control(**MONO), nstreams=2, max_frames=nf)
    with pytest.raises(ValueError, match="channel"):
        m.encode_tensor(torch.zeros(2, 2, nf * 1152))
    m.close()
