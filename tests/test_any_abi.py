"""One batch for every stream kind as an ABI (host only, no GPU): the three exports of include/hmp3_amd.h's "one batch for
every stream kind" section are declared, exported and bound, and create validates the menu before it looks at a device - a
menu of both MPEG versions and both allocator generations passes hx_batch_create_any / hx_multi_create_any and is refused
for the missing device alone, while hx_batch_create_mixed keeps refusing it by name."""
import ctypes as C

import pytest

P, I = C.c_void_p, C.c_int
WANT = {
    "hx_batch_create_any": ("hx_batch *", ["int", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P, [I, I, P, I, P, P, I]),
    "hx_multi_create_any": ("hx_multi *", ["int", "const int *", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P,
                            [I, P, I, P, I, P, P, I]),
    "hx_batch_stream_frames_per_block": ("int", ["const hx_batch *", "int"], I, [P, I]),
}
# stereo 44.1 kHz CBR-64 (kind 0), 22.05 kHz CBR-32 (kind 1), dual channel (kind 2), mono 16 kHz CBR-32 (kind 1)
MENU = [dict(bitrate=64), dict(bitrate=32, samprate=22050), dict(bitrate=64, mode=2), dict(bitrate=32, mode=3, samprate=16000)]


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


def test_python_classes_offer_the_calls():
    from hmp3_amd import api
    for cls in (api.Batch, api.SrcBatch, api.Multi, api.SrcMulti):
        for m in ("any", "stream_frames_per_block"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_accessor_and_creates_refuse_bad_arguments():
    from hmp3_amd import api
    L = api.lib()
    assert L.hx_batch_stream_frames_per_block(None, 0) == -1
    ec = api.default_control(bitrate=64)
    assert not L.hx_batch_create_any(0, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()
    assert not L.hx_multi_create_any(0, None, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()


def create(fn, menu):
    """-> hx_last_error of a create over `menu` on this GPU-less machine (the handle, if one came back, is released)"""
    from hmp3_amd import api
    L = api.lib()
    ecs = (api.EControl * len(menu))(*[api.default_control(**kw) for kw in menu])
    if fn.startswith("hx_multi"):
        h = getattr(L, fn)(1, None, 4, ecs, len(menu), None, None, 4)
        if h:
            L.hx_multi_destroy(h)
            return ""
    else:
        h = getattr(L, fn)(0, 4, ecs, len(menu), None, None, 4)
        if h:
            L.hx_batch_destroy(h)
            return ""
    return api.last_error()


@pytest.mark.parametrize("fn", ["hx_batch_create_any", "hx_multi_create_any"])
def test_a_menu_of_every_kind_passes_entry_validation(fn):
    """what refuses it here is the missing device (with a device: nothing)"""
    from hmp3_amd import api
    err = create(fn, MENU)
    assert not err.startswith("menu entry"), err
    if api.lib().hx_device_count() == 0:
        assert err.startswith("no HIP device available"), err


def test_the_same_menu_stays_refused_by_the_mixed_create():
    assert create("hx_batch_create_mixed", MENU).startswith("menu entry 1: MPEG-1 and MPEG-2")
