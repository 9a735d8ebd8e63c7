"""PCM planes as an ABI (host only, no GPU): the three exports of include/hmp3_amd.h's "PCM planes" section are declared,
exported and bound, hx_pcm_planar_layout - pure host code - is held to hand-computed layouts, the setters refuse a null
handle, and encode_tensor's stride derivation (api.tensor_planes, a pure function on shapes and strides) is held to the
layouts of the tensors it is meant for."""
import ctypes as C

import numpy as np
import pytest

P, I, LL = C.c_void_p, C.c_int, C.c_longlong
WANT = {
    "hx_pcm_planar_layout": ("long long", ["int", "int", "const int *", "const int *", "int", "long long *", "long long *"], LL, [I, I, P, P, I, P, P]),
    "hx_batch_pcm_planes": ("int", ["hx_batch *", "const long long *", "const long long *", "long long", "int"], I, [P, P, P, LL, I]),
    "hx_multi_pcm_planes": ("int", ["hx_multi *", "const long long *", "const long long *", "long long", "int"], I, [P, P, P, LL, I]),
    # (the test tap that runs the row kernel of a call alone)
    "hx_batch_debug_pcm_rows": ("int", ["hx_batch *", "const void *", "int", "int", "void *"], I, [P, P, I, I, P]),
}


@pytest.mark.parametrize("name", list(WANT))
def test_prototype_is_declared_exported_and_bound(name):
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert name in protos, "include/hmp3_amd.h does not declare " + name
    ret, params, restype, argtypes = WANT[name]
    assert protos[name][1] == ret and protos[name][2] == params
    f = getattr(api.lib(), name)            # (raises AttributeError if the library does not export it)
    assert f.restype is restype
    assert list(f.argtypes) == argtypes


def test_python_offers_the_calls():
    from hmp3_amd import api
    assert callable(api.planar_layout) and callable(api.tensor_planes)
    for cls in (api.Batch, api.Multi):
        assert callable(getattr(cls, "pcm_planes")), cls.__name__
    assert callable(api.Batch.encode_tensor) and callable(api.Batch.debug_pcm_rows)


def layout(nstreams, nframes, nfr, channels, sample_bytes, off="own", stride="own"):
    """hx_pcm_planar_layout through ctypes -> (return value, the offsets it wrote, the strides it wrote)"""
    from hmp3_amd import api
    arr = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
    o = (C.c_longlong * (nstreams + 1))(*([-7] * (nstreams + 1)))
    d = (C.c_longlong * max(nstreams, 1))(*([-7] * max(nstreams, 1)))
    r = api.lib().hx_pcm_planar_layout(nstreams, nframes, arr(nfr), arr(channels), sample_bytes, o if off == "own" else off, d if stride == "own" else stride)
    return int(r), list(o), list(d)[:nstreams]


COUNTS, CHANNELS = [2, 0, 1, 3], [2, 1, 1, 2]


def test_planar_layout_by_hand():
    """uniform: 3 stereo streams of 2 frames, int16 - planes of 4608 bytes, two per stream"""
    assert layout(3, 2, None, [2, 2, 2], 2) == (27648, [0, 9216, 18432, 27648], [4608] * 3)
    # mixed mono / stereo, 3 frames each: planes of 6912 bytes; the image is the packed layout's size
    assert layout(4, 3, None, CHANNELS, 2) == (41472, [0, 13824, 20736, 27648, 41472], [6912] * 4)
    # counts [2, 0, 1, 3] of 3 frames: planes of 4608, 0, 2304 and 6912 bytes (int16), twice that in fp32
    assert layout(4, 3, COUNTS, CHANNELS, 2) == (25344, [0, 9216, 9216, 11520, 25344], [4608, 0, 2304, 6912])
    assert layout(4, 3, COUNTS, CHANNELS, 4) == (50688, [0, 18432, 18432, 23040, 50688], [9216, 0, 4608, 13824])
    assert layout(0, 3, None, [], 2)[0] == 0


def test_every_tight_plane_is_16_byte_aligned():
    rng = np.random.default_rng(6)
    for sample_bytes in (2, 4):
        nfr, ch = [int(v) for v in rng.integers(0, 8, 40)], [int(v) for v in rng.integers(1, 3, 40)]
        r, off, stride = layout(40, 7, nfr, ch, sample_bytes)
        assert r == off[-1] == sum(n * 1152 * c * sample_bytes for n, c in zip(nfr, ch))
        assert all(o % 16 == 0 for o in off) and all(d % 2304 == 0 for d in stride)
        assert stride == [n * 1152 * sample_bytes for n in nfr]


@pytest.mark.parametrize("bad", [
    dict(off=None), dict(stride=None), dict(channels=None), dict(channels=[2, 1, 3, 2]), dict(channels=[2, 0, 1, 2]), dict(sample_bytes=3),
    dict(sample_bytes=8), dict(sample_bytes=0), dict(nfr=[2, 0, 4, 3]), dict(nfr=[2, -1, 1, 3])],
    ids=["null_off", "null_stride", "null_channels", "three_channels", "no_channel", "three_byte_samples", "eight_byte_samples", "no_sample_size",
         "count_beyond_nframes", "negative_count"])
def test_planar_layout_refuses_bad_arguments(bad):
    kw = dict(nfr=COUNTS, channels=CHANNELS, sample_bytes=2)
    kw.update(bad)
    r, off, stride = layout(4, 3, kw["nfr"], kw["channels"], kw["sample_bytes"], **{k: None for k in ("off", "stride") if k in bad})
    assert r == -1 and off == [-7] * 5 and stride == [-7] * 4, "a refused layout wrote something"
    from hmp3_amd import api
    assert api.lib().hx_pcm_planar_layout(-1, 3, None, (C.c_int * 1)(2), 2, (C.c_longlong * 1)(), (C.c_longlong * 1)()) == -1
    assert api.lib().hx_pcm_planar_layout(1, -1, None, (C.c_int * 1)(2), 2, (C.c_longlong * 2)(), (C.c_longlong * 1)()) == -1


def test_python_planar_layout():
    from hmp3_amd import api
    off, stride, total = api.planar_layout(3, CHANNELS, COUNTS)
    assert off.dtype == np.int64 and list(off) == [0, 9216, 9216, 11520, 25344] and list(stride) == [4608, 0, 2304, 6912] and total == 25344
    assert api.planar_layout(3, CHANNELS, f32=True)[2] == 82944
    with pytest.raises(ValueError):
        api.planar_layout(3, [2, 3])


def test_setters_refuse_a_null_handle():
    from hmp3_amd import api
    L = api.lib()
    off, stride = (C.c_longlong * 2)(0, 4608), (C.c_longlong * 2)(2304, 2304)
    assert L.hx_batch_pcm_planes(None, off, stride, 9216, 0) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_pcm_planes(None, None, None, 0, 0) == -1
    assert L.hx_multi_pcm_planes(None, off, stride, 9216, 1) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_pcm_planes(None, None, None, 0, 0) == -1
    assert L.hx_batch_debug_pcm_rows(None, off, 1, 1, None) == -1 and "null batch" in api.last_error()


# ---- encode_tensor's stride derivation: shapes and strides (in elements) as torch reports them ----
T = 2304


def planes(shape, strides, item=4):
    from hmp3_amd import api
    off, stride, nbytes, first = api.tensor_planes(shape, strides, item)
    assert off.dtype == np.int64 and stride.dtype == np.int64
    return list(off), list(stride), nbytes, first


def test_a_contiguous_s_c_t_tensor():
    assert planes((3, 2, T), (2 * T, T, 1)) == ([0, 8 * T, 16 * T], [4 * T] * 3, 24 * T, 0)
    assert planes((3, 2, T), (2 * T, T, 1), 2) == ([0, 4 * T, 8 * T], [2 * T] * 3, 12 * T, 0)


def test_a_c_s_t_tensor_permuted_to_s_c_t():
    """torch.empty(2, 3, T).permute(1, 0, 2): strides (T, 3 T, 1) - a stream's planes lie 3 T samples apart"""
    assert planes((3, 2, T), (T, 3 * T, 1)) == ([0, 4 * T, 8 * T], [12 * T] * 3, 24 * T, 0)


def test_a_time_sliced_view():
    """w[:, :, 1152:3456] of a [3, 2, 4608] tensor: strides stay (9216, 4608, 1); the image is what the view spans, from its
    own first element (the caller's pointer is the view's data_ptr)"""
    assert planes((3, 2, T), (9216, 4608, 1)) == ([0, 4 * 9216, 8 * 9216], [4 * 4608] * 3, 4 * (2 * 9216 + 4608 + T), 0)


def test_expand_along_the_channel_is_stride_zero():
    """torch.empty(3, 1, T).expand(3, 2, T): channel stride 0 - both channels read one plane"""
    assert planes((3, 2, T), (T, 0, 1)) == ([0, 4 * T, 8 * T], [0] * 3, 12 * T, 0)


def test_a_mono_s_t_tensor_and_negative_strides():
    assert planes((3, T), (T, 1), 2) == ([0, 2 * T, 4 * T], [0] * 3, 6 * T, 0)
    # (torch has no negative strides; the function is plain arithmetic and numbers the image from its lowest element)
    assert planes((2, 2, T), (2 * T, -T, 1)) == ([4 * T, 12 * T], [-4 * T] * 2, 16 * T, -T)


@pytest.mark.parametrize("shape, strides, what", [
    ((3, 2, T), (2 * T, 1, 2), "stride 1"), ((3, 2, T), (4 * T, 2 * T, 2), "stride 1"), ((3, T), (1, 3), "stride 1"),
    ((3, 2, 1000), (2000, 1000, 1), "multiple of 1152"), ((3, 2, 0), (0, 0, 1), "multiple of 1152"), ((3, 3, T), (3 * T, T, 1), "1 or 2 channels"),
    ((T,), (1,), "dimensional"), ((1, 3, 2, T), (6 * T, 2 * T, T, 1), "dimensional")],
    ids=["time_major", "every_other_sample", "mono_transposed", "ragged_time", "no_time", "three_channels", "one_dimension", "four_dimensions"])
def test_tensor_planes_refuses(shape, strides, what):
    from hmp3_amd import api
    with pytest.raises(ValueError, match=what):
        api.tensor_planes(shape, strides, 4)
