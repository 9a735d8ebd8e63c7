"""PCM segments as an ABI (host only, no GPU): the three exports of include/hmp3_amd.h's "PCM segments" section are declared,
exported and bound, hx_pcm_packed_layout - pure host code - is held to hand-computed layouts, and the setters refuse a null
handle."""
import ctypes as C

import numpy as np
import pytest

P, I, LL = C.c_void_p, C.c_int, C.c_longlong
WANT = {
    "hx_pcm_packed_layout": ("long long", ["int", "int", "const int *", "const int *", "int", "long long *"], LL, [I, I, P, P, I, P]),
    "hx_batch_pcm_segments": ("int", ["hx_batch *", "const long long *", "long long"], I, [P, P, LL]),
    "hx_multi_pcm_segments": ("int", ["hx_multi *", "const long long *", "long long"], I, [P, P, LL]),
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
    assert callable(api.packed_layout)
    for cls in (api.Batch, api.Multi):
        for m in ("pcm_segments", "packed_layout", "encode_host_image"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert callable(api.Batch.encode_host_dense_image)


def layout(nstreams, nframes, nfr, channels, sample_bytes, off="own"):
    """hx_pcm_packed_layout through ctypes -> (return value, the offsets it wrote)"""
    from hmp3_amd import api
    arr = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
    out = (C.c_longlong * (nstreams + 1))(*([-7] * (nstreams + 1)))
    r = api.lib().hx_pcm_packed_layout(nstreams, nframes, arr(nfr), arr(channels), sample_bytes, out if off == "own" else off)
    return int(r), list(out)


COUNTS, CHANNELS = [2, 0, 1, 3], [2, 1, 1, 2]


def test_packed_layout_by_hand():
    """counts [2, 0, 1, 3] of 3 frames, channels [2, 1, 1, 2]: int16 segments of 2 * 4608, 0, 2304 and 3 * 4608 bytes"""
    assert layout(4, 3, COUNTS, CHANNELS, 2) == (25344, [0, 9216, 9216, 11520, 25344])
    # no counts: every stream takes the 3 frames - 13824, 6912, 6912, 13824 bytes
    assert layout(4, 3, None, CHANNELS, 2) == (41472, [0, 13824, 20736, 27648, 41472])
    # fp32: twice the int16 layouts
    assert layout(4, 3, COUNTS, CHANNELS, 4) == (50688, [0, 18432, 18432, 23040, 50688])
    assert layout(4, 3, None, CHANNELS, 4) == (82944, [0, 27648, 41472, 55296, 82944])


def test_every_tight_offset_is_16_byte_aligned():
    rng = np.random.default_rng(5)
    for sample_bytes in (2, 4):
        nfr, ch = [int(v) for v in rng.integers(0, 8, 40)], [int(v) for v in rng.integers(1, 3, 40)]
        r, off = layout(40, 7, nfr, ch, sample_bytes)
        assert r == off[-1] == sum(n * 1152 * c * sample_bytes for n, c in zip(nfr, ch)) and all(o % 16 == 0 for o in off)


@pytest.mark.parametrize("bad", [
    dict(off=None), dict(channels=None), dict(channels=[2, 1, 3, 2]), dict(channels=[2, 0, 1, 2]), dict(sample_bytes=3), dict(sample_bytes=8),
    dict(sample_bytes=0), dict(nfr=[2, 0, 4, 3]), dict(nfr=[2, -1, 1, 3])],
    ids=["null_off", "null_channels", "three_channels", "no_channel", "three_byte_samples", "eight_byte_samples", "no_sample_size",
         "count_beyond_nframes", "negative_count"])
def test_packed_layout_refuses_bad_arguments(bad):
    kw = dict(nfr=COUNTS, channels=CHANNELS, sample_bytes=2)
    kw.update(bad)
    r, off = layout(4, 3, kw["nfr"], kw["channels"], kw["sample_bytes"], **({"off": None} if "off" in bad else {}))
    assert r == -1 and off == [-7] * 5, "a refused layout wrote offsets"


def test_python_packed_layout():
    from hmp3_amd import api
    off, total = api.packed_layout(3, CHANNELS, COUNTS)
    assert off.dtype == np.int64 and list(off) == [0, 9216, 9216, 11520, 25344] and total == 25344
    assert api.packed_layout(3, CHANNELS, f32=True)[1] == 82944
    with pytest.raises(ValueError):
        api.packed_layout(3, [2, 3])


def test_setters_refuse_a_null_handle():
    from hmp3_amd import api
    L = api.lib()
    off = (C.c_longlong * 2)(0, 4608)
    assert L.hx_batch_pcm_segments(None, off, 9216) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_pcm_segments(None, None, 0) == -1
    assert L.hx_multi_pcm_segments(None, off, 9216) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_pcm_segments(None, None, 0) == -1
