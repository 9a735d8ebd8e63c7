"""The slot operations on many streams as an ABI (host only, no GPU): the six prototypes are in include/hmp3_amd.h, the
library exports them, and hmp3_amd.api binds them with the argument types the header declares."""
import ctypes as C

import pytest

P, LL, I = C.c_void_p, C.c_longlong, C.c_int
# name -> (return type, parameter types as the header spells them, ctypes argtypes)
WANT = {
    "hx_batch_stream_states_stride": ("long long", ["const hx_batch *"], [P]),
    "hx_batch_reset_streams": ("int", ["hx_batch *", "const int *", "int", "void *"], [P, P, I, P]),
    "hx_batch_get_stream_states_device": ("int", ["hx_batch *", "const int *", "int", "void *", "long long", "void *"], [P, P, I, P, LL, P]),
    "hx_batch_set_stream_states_device": ("int", ["hx_batch *", "const int *", "int", "const void *", "long long", "void *"], [P, P, I, P, LL, P]),
    "hx_batch_get_stream_states": ("int", ["hx_batch *", "const int *", "int", "void *", "long long"], [P, P, I, P, LL]),
    "hx_batch_set_stream_states": ("int", ["hx_batch *", "const int *", "int", "const void *", "long long"], [P, P, I, P, LL]),
}


@pytest.mark.parametrize("name", list(WANT))
def test_prototype_is_declared_exported_and_bound(name):
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert name in protos, "include/hmp3_amd.h does not declare " + name
    ret, params, argtypes = WANT[name]
    assert protos[name][1] == ret and protos[name][2] == params
    f = getattr(api.lib(), name)            # (raises AttributeError if the library does not export it)
    assert f.restype is (C.c_longlong if ret == "long long" else C.c_int)
    assert list(f.argtypes) == argtypes


def test_python_classes_offer_the_calls():
    from hmp3_amd import api
    for cls in (api.Batch, api.SrcBatch):
        for m in ("reset_streams", "get_stream_states", "set_stream_states", "get_stream_states_device", "set_stream_states_device"):
            assert callable(getattr(cls, m))


def test_single_slot_calls_keep_their_signatures():
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert protos["hx_batch_reset_stream"][2] == ["hx_batch *", "int"]
    assert protos["hx_batch_get_stream_state"][2] == ["hx_batch *", "int", "void *"]
    assert protos["hx_batch_set_stream_state"][2] == ["hx_batch *", "int", "const void *"]


def test_calls_refuse_a_null_batch_without_a_device():
    from hmp3_amd import api
    L = api.lib()
    one = (C.c_int * 1)(0)
    assert L.hx_batch_stream_states_stride(None) == 0
    assert L.hx_batch_reset_streams(None, one, 1, None) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_get_stream_states(None, one, 1, None, 16) == -1
    assert L.hx_batch_set_stream_states_device(None, one, 1, None, 16, None) == -1
