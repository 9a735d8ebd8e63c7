"""Slot configurations as an ABI (host only, no GPU): the six prototypes of the menu calls are in include/hmp3_amd.h, the
library exports them, and hmp3_amd.api binds them with the argument types the header declares."""
import ctypes as C

import pytest

P, I = C.c_void_p, C.c_int
# name -> (return type, parameter types as the header spells them, ctypes restype, ctypes argtypes)
WANT = {
    "hx_batch_create_menu": ("hx_batch *", ["int", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P, [I, I, P, I, P, P, I]),
    "hx_multi_create_menu": ("hx_multi *", ["int", "const int *", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P,
                             [I, P, I, P, I, P, P, I]),
    "hx_batch_nconfigs": ("int", ["const hx_batch *"], I, [P]),
    "hx_batch_stream_config": ("int", ["const hx_batch *", "int"], I, [P, I]),
    "hx_batch_assign_streams": ("int", ["hx_batch *", "const int *", "const int *", "int", "void *"], I, [P, P, P, I, P]),
    "hx_multi_assign_streams": ("int", ["hx_multi *", "const int *", "const int *", "int"], I, [P, P, P, I]),
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


def test_python_classes_offer_the_calls():
    from hmp3_amd import api
    for cls in (api.Batch, api.SrcBatch, api.Multi, api.SrcMulti):
        for m in ("menu", "assign_streams", "nconfigs", "stream_config"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_the_create_calls_keep_their_signatures():
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert protos["hx_batch_create"][2] == ["int", "int", "const HX_E_CONTROL *", "int", "int"]
    assert protos["hx_batch_create_src"][2] == ["int", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "int", "int"]
    assert protos["hx_batch_reset_streams"][2] == ["hx_batch *", "const int *", "int", "void *"]


def test_calls_refuse_bad_arguments_without_a_device():
    from hmp3_amd import api
    L = api.lib()
    one = (C.c_int * 1)(0)
    ec = api.default_control(bitrate=64)
    assert L.hx_batch_nconfigs(None) == 0 and L.hx_batch_stream_config(None, 0) == -1
    assert L.hx_batch_assign_streams(None, one, one, 1, None) == -1 and "null batch" in api.last_error()
    assert L.hx_multi_assign_streams(None, one, one, 1) == -1 and "null handle" in api.last_error()
    assert not L.hx_batch_create_menu(0, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()
    assert not L.hx_batch_create_menu(0, 2, None, 1, None, None, 4) and "bad arguments" in api.last_error()
    bad = (C.c_int * 2)(0, 1)
    assert not L.hx_batch_create_menu(0, 2, C.byref(ec), 1, None, bad, 4) and "stream 1: configuration 1 out of range" in api.last_error()
    assert not L.hx_multi_create_menu(0, None, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()


def test_a_source_the_converter_rejects_names_its_menu_entry():
    """the converter's part of create runs on the host, before a device is looked for"""
    from hmp3_amd import api
    L = api.lib()
    ecs = (api.EControl * 2)(api.default_control(bitrate=64), api.default_control(bitrate=64))
    srcs = (api.Source * 2)(api.Source(16, 0, 0, 0), api.Source(12, 0, 0, 0))       # (12-bit samples: no such source format)
    assert not L.hx_batch_create_menu(0, 3, ecs, 2, srcs, None, 4)
    assert api.last_error().startswith("menu entry 1: "), api.last_error()
