"""Converting batches (hx_batch_create_src) on the GPU: sources in any format and at any rate the converter takes,
converted by k_src (hmp3_amd/csrc/hx_src.hip) and encoded in one call.

The converted PCM (the "srcpcm" tap) is compared with the reference's own Csrc bit for bit, and every stream's bytes and
in_used with the reference's MP3_audio_encode loop on the same source (oracle/_ref/libhmp3ref.so) and with this library's
per-frame MP3_audio_encode.  MPEG-1 tests run on both stream-walk builds, MPEG-2 ones once (one_k6_build)."""
import ctypes as C

import numpy as np
import pytest

from hmp3_amd import api
from oracle import oracle as O
from src_cases import Stream, make_batch, ref_converted, run, source_signal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(O.ref() is None, reason="oracle/_ref not built")]

FORMATS = [(8, 0), (16, 0), (24, 0), (32, 0), (32, 1)]
# (source rate, encode rate): every case of the converter towards MPEG-1 and towards MPEG-2 rates
PAIRS1 = [(44100, 44100), (22050, 44100), (32000, 44100), (48000, 32000), (44100, 32000), (48000, 44100)]
PAIRS2 = [(16000, 16000), (8000, 16000), (11025, 16000), (22050, 24000), (48000, 24000), (44100, 24000), (32000, 22050)]


def stage_streams(pairs, layout):
    out = []
    for k, (src, tgt) in enumerate(pairs):
        for j, (bits, fl) in enumerate(FORMATS):
            ch, mono = {"stereo": (2, 0), "mono": (1, 0), "downmix": (2, 1)}[layout]
            s = Stream(src, bits, fl, ch, mpeg_select=tgt, mono_convert=mono, seed=100 * k + j, seconds=4.0, noise=(j % 2 == 0))
            s.target = tgt
            out.append(s)
    return out


@pytest.mark.one_k6_build
@pytest.mark.parametrize("pairs", ["mpeg1", "mpeg2"])
@pytest.mark.parametrize("layout", ["stereo", "mono", "downmix"])
def test_srcpcm_tap_equals_the_reference_converter(pairs, layout, k6_build):
    """k_src's output is the reference's Csrc output bit for bit: every case x layout x format, calls of 1, 5 and 37
    frames in sequence (a one-frame call reads and writes the carried intermediate samples in one launch)"""
    streams = stage_streams(PAIRS1 if pairs == "mpeg1" else PAIRS2, layout)
    b = make_batch(streams, 37)
    _, _, pcm = run(b, streams, [1, 5, 37], taps=True)
    got = np.concatenate(pcm, axis=1)
    for i, s in enumerate(streams):
        want = ref_converted(s, s.target, 43)
        g = got[i][:, :want.shape[1]]
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (s.source, s.target, s.bits, s.is_float, layout,
                                                                         int(np.argmax(np.any(g != want, axis=1))))
    b.close()


def range_streams(layout):
    """float sources (at the +-1 scale: k_src multiplies by 32768) far outside it: samples up to 16.0, and at 1e-41, which
    float32 holds as a subnormal; rate pairs without conversion, down and up"""
    out = []
    for k, (src, tgt) in enumerate([(44100, 44100), (48000, 44100), (22050, 44100)]):
        for scale in (16.0, 1e-41):
            ch, mono = {"stereo": (2, 0), "downmix": (2, 1)}[layout]
            s = Stream(src, 32, 1, ch, mpeg_select=tgt, mono_convert=mono, seed=900 + k, seconds=1.0)
            x = source_signal(900 + k, src, ch) * scale
            x[5::97] = scale                    # the level itself, exactly
            s.data = x.astype("<f4").tobytes() + bytes(1 << 18)
            s.target, s.scale = tgt, scale
            out.append(s)
    return out


@pytest.mark.one_k6_build
@pytest.mark.parametrize("layout", ["stereo", "downmix"])
def test_srcpcm_tap_on_float_sources_outside_the_unit_range(layout, k6_build):
    """k_src on float sources at 16 x full scale and at 1e-41 (subnormal in the source, 3.3e-37 once scaled; the filter's
    products of it are subnormal again): the converted PCM equals the reference's Csrc bit for bit over calls of 1, 5 and
    12 frames, zero signs included, and the streams' bytes equal the reference's MP3_audio_encode loop"""
    streams = range_streams(layout)
    raw = [np.frombuffer(s.data[:4 * 2 * s.source], "<f4") for s in streams]
    assert all(float(np.abs(r).max()) == 16.0 for r in raw[0::2])
    assert all(0 < float(np.abs(r).max()) < 2.0 ** -126 and np.count_nonzero(r) > 40000 for r in raw[1::2])
    b = make_batch(streams, 12)
    outs, _, pcm = run(b, streams, [1, 5, 12], taps=True)
    got = np.concatenate(pcm, axis=1)
    for i, s in enumerate(streams):
        want = ref_converted(s, s.target, 18)
        g = got[i][:, :want.shape[1]]
        assert np.count_nonzero(want) > 10000
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (s.source, s.target, s.scale, layout,
                                                                         int(np.argmax(np.any(g.view(np.uint32) != want.view(np.uint32), axis=1))))
        assert outs[i] == s.reference(18)[0], (s.source, s.target, s.scale, layout)
    b.close()


def mixed_stereo():
    return [Stream(48000, 24, 0, mpeg_select=44100, seed=1), Stream(32000, 32, 1, mpeg_select=44100, seed=2),
            Stream(22050, 16, 0, mpeg_select=44100, seed=3), Stream(44100, 8, 0, seed=4),
            Stream(48000, 32, 0, mpeg_select=32000, seed=5), Stream(44100, 16, 0, mpeg_select=32000, seed=6)]


def mixed_mono():
    return [Stream(48000, 16, 0, channels=1, mpeg_select=44100, seed=7), Stream(44100, 24, 0, mono_convert=1, mpeg_select=32000, seed=8),
            Stream(32000, 8, 0, channels=1, mpeg_select=44100, seed=9), Stream(48000, 32, 1, mono_convert=1, seed=10),
            Stream(22050, 16, 0, mono_convert=1, mpeg_select=44100, seed=11)]


def mixed_mpeg2():
    return [Stream(48000, 16, 0, mono_convert=1, mpeg_select=24000, seed=12), Stream(44100, 24, 0, mono_convert=1, mpeg_select=22050, seed=13),
            Stream(11025, 16, 0, channels=1, mpeg_select=22050, seed=14), Stream(8000, 8, 0, channels=1, mpeg_select=16000, seed=15)]


def check_against_reference(streams, nframes, calls):
    b = make_batch(streams, max(calls))
    outs, pos, _ = run(b, streams, calls)
    for i, s in enumerate(streams):
        want, used = s.reference(nframes)
        assert outs[i] == want, "stream %d differs from the reference's MP3_audio_encode loop" % i
        assert pos[i] == used
        mine, used2 = s.per_frame(nframes)
        assert outs[i] == mine and pos[i] == used2, "stream %d differs from the per-frame encoder" % i
    b.close()


def test_mixed_stereo_batch_equals_the_reference_loop(k6_build):
    check_against_reference(mixed_stereo(), 64, [64])


def test_mixed_mono_batch_equals_the_reference_loop(k6_build):
    check_against_reference(mixed_mono(), 64, [64])


@pytest.mark.one_k6_build
def test_mpeg2_converting_batch_equals_the_reference_loop(k6_build):
    check_against_reference(mixed_mpeg2(), 48, [48])


def test_ragged_calls_with_dc_filter_equal_one_call(k6_build):
    """calls of 1, 7 and 40 frames give what one call of 48 gives, the DC filter (after the converter) on some streams"""
    def streams():
        st = mixed_stereo()
        for s in st[::2]:
            s.ec.filter_select = 1
        return st
    a, b = streams(), streams()
    ba, bb = make_batch(a, 48), make_batch(b, 48)
    oa, pa, _ = run(ba, a, [48])
    ob, pb, _ = run(bb, b, [1, 7, 40])
    assert oa == ob and pa == pb
    want, _ = a[0].reference(48)
    assert oa[0] == want


def test_checkpoint_of_a_converting_stream_resumes_elsewhere(k6_build):
    """a case-4 stream saved mid-way continues in another slot of another batch (another max_frames) byte for byte;
    blobs do not cross between converting and plain batches; reset_stream restarts the converter"""
    A = api
    L = A.lib()
    s = Stream(48000, 24, 0, mpeg_select=44100, seed=21)
    other = Stream(44100, 16, 0, mpeg_select=32000, seed=22)
    b1 = make_batch([s, other], 16)
    o1, p1, _ = run(b1, [s, other], [9])
    blob = b1.get_stream_state(0)
    o1b, _, _ = run(b1, [s, other], [13], pos=list(p1))
    b2 = make_batch([other, other, s], 32)
    b2.set_stream_state(2, blob)
    o2, _, _ = run(b2, [other, other, s], [5, 8], pos=[0, 0, p1[0]])
    assert o2[2] == o1b[0]
    want, _ = s.reference(22)
    assert o1[0] + o1b[0] == want
    # a plain batch's blob and a converting batch's blob are refused by the other kind
    plain = A.Batch(A.default_control(bitrate=64), nstreams=1, max_frames=4)
    pb = plain.get_stream_state(0)
    buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
    assert L.hx_batch_set_stream_state(plain.h, 0, buf) != 0
    buf2 = (C.c_ubyte * len(blob)).from_buffer_copy(pb + bytes(len(blob) - len(pb)))
    assert L.hx_batch_set_stream_state(b2.h, 0, buf2) != 0
    # reset: the slot starts over, converter included
    b1.reset_stream(0)
    o3, _, _ = run(b1, [s, other], [9], pos=[0, p1[1] + 0])
    assert o3[0] == o1[0]


def test_pointer_switch_to_zero_bytes_equals_the_reference(k6_build):
    """calls whose input jumps to a region of zero bytes right after real audio (the command line's drain calls) equal the
    reference's loop fed the same pointers: the carried case-4 samples are formed ones, not input (u8: zero bytes are
    full-scale negative)"""
    for s in (Stream(48000, 16, 0, mpeg_select=32000, seed=31), Stream(44100, 16, 0, mpeg_select=32000, seed=32),
              Stream(48000, 8, 0, mpeg_select=44100, seed=33)):
        b = make_batch([s], 24)
        nf = 24
        stride = b.in_stride(nf) + 65536
        nb, _ = b.schedule(0, 12)
        zero_at = stride - 32768
        offs = np.concatenate([np.concatenate([[0], np.cumsum(nb)[:-1]]), np.full(nf - 12, zero_at)]).astype(np.int64)
        row = np.zeros((1, stride), np.uint8)
        real = np.frombuffer(s.data[:zero_at], np.uint8)
        row[0, :len(real)] = real
        row[0, zero_at:] = 0
        res, used = b.encode_src_host(row, nf, frame_off=offs[None, :])
        s.data = bytes(row[0])
        want, end = s.reference(nf, offsets=offs)
        assert res[0] == want and int(used[0]) == end
        b.close()


def test_misuse_is_refused_and_leaves_the_batch_usable(k6_build):
    A = api
    L = A.lib()
    streams = mixed_stereo()[:3]
    b = make_batch(streams, 8)
    stride = b.in_stride(8)
    rows = np.zeros((3, stride), np.uint8)
    out = np.zeros((3, b.out_stride(8)), np.uint8)
    nb = np.zeros(3, np.int32)
    used = np.zeros(3, np.int64)
    short = np.zeros((3, 1000), np.uint8)
    assert L.hx_batch_encode_src_host(b.h, short.ctypes.data, 1000, None, 8, out.ctypes.data, out.shape[1], nb.ctypes.data, used.ctypes.data, None) != 0
    assert "in_stride" in A.last_error()
    offs = np.full((3, 8), stride - 10, np.int64)
    assert L.hx_batch_encode_src_host(b.h, rows.ctypes.data, stride, offs.ctypes.data, 8, out.ctypes.data, out.shape[1], nb.ctypes.data, used.ctypes.data, None) != 0
    assert L.hx_batch_encode_src_host(b.h, rows.ctypes.data, stride, None, 9, out.ctypes.data, out.shape[1], nb.ctypes.data, used.ctypes.data, None) != 0
    # still usable, and nothing advanced: the next call is the stream's first
    o, _, _ = run(b, streams, [8])
    want, _ = streams[0].reference(8)
    assert o[0] == want
    b.close()
    bad = mixed_stereo()[:2]
    bad[1].src.bits = 12
    with pytest.raises(RuntimeError, match="stream 1"):
        make_batch(bad, 4)


def test_several_devices_equal_the_reference_loop(k6_build):
    """hx_multi_create_src: the streams in blocks over every device present, each block a converting batch"""
    A = api
    streams = mixed_stereo()
    m = A.SrcMulti([s.ec for s in streams], [s.src for s in streams], max_frames=24)
    stride = m.in_stride(24)
    rows = np.zeros((len(streams), stride), np.uint8)
    for i, s in enumerate(streams):
        rows[i] = np.frombuffer(s.data[:stride], np.uint8)
    res, used = m.encode_src_host(rows, 24)
    assert m.status() == 0
    for i, s in enumerate(streams):
        want, end = s.reference(24)
        assert res[i] == want and int(used[i]) == end, i
    m.close()


def test_plain_pcm_calls_are_refused_on_a_converting_batch(k6_build):
    A = api
    L = A.lib()
    streams = mixed_stereo()[:2]
    b = make_batch(streams, 4)
    pcm = np.zeros((2, 4 * 1152, 2), np.float32)
    out = np.zeros((2, b.out_stride(4)), np.uint8)
    nb = np.zeros(2, np.int32)
    assert L.hx_batch_encode_f32_host(b.h, pcm.ctypes.data, 4, out.ctypes.data, out.shape[1], nb.ctypes.data) != 0
    assert "hx_batch_encode_src" in A.last_error()
    assert L.hx_batch_encode_s16_host(b.h, pcm.astype(np.int16).ctypes.data, 4, out.ctypes.data, out.shape[1], nb.ctypes.data) != 0
    o, _, _ = run(b, streams, [4])
    want, _ = streams[0].reference(4)
    assert o[0] == want
    b.close()


def test_phase_beyond_32_bits_equals_the_stepped_converter(k6_build):
    """a stream resumed at call 14000 of a 32 -> 44.1 kHz converter (output index x bank step beyond 2^32) converts what the
    host converter stepped through 14000 calls converts: the kernel's phase is 64-bit"""
    A = api
    L = A.lib()
    s = Stream(32000, 16, 0, mpeg_select=44100, seed=41)
    b = make_batch([s], 4)
    calls = 14000
    blob = bytearray(b.get_stream_state(0))
    carry = 2 * 192 * 4
    blob[len(blob) - carry - 8:len(blob) - carry] = np.int64(calls).tobytes()     # the converter's call count
    b.set_stream_state(0, bytes(blob))
    h = L.hx_src_create()
    cut = C.c_int(0)
    assert L.hx_src_init(h, 32000, 2, 16, 0, 44100, 2, C.byref(cut)) > 0
    zeros = (C.c_ubyte * (1152 * 4 * 2))()
    y = np.zeros(2304, np.float32)
    for _ in range(calls):
        L.hx_src_convert(h, zeros, y.ctypes.data, None)
    _, _, pcm = run(b, [s], [1, 3], taps=True)
    got = np.concatenate(pcm, axis=1)[0]
    buf = (C.c_ubyte * len(s.data)).from_buffer_copy(s.data)
    pos, want = 0, []
    for _ in range(4):
        pos += L.hx_src_convert(h, C.byref(buf, pos), y.ctypes.data, None)
        want.append(y.reshape(1152, 2).copy())
    want = np.concatenate(want)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    L.hx_src_destroy(h)
    b.close()
