"""Decoded PCM as an ABI (host only, no GPU): the three exports of include/hmp3_amd.h's "decoded PCM" section are declared,
exported and bound, the setter and the host call refuse a null handle, the delay is the documented constant and the Python
methods exist."""
import ctypes as C

import pytest

P, I, LL = C.c_void_p, C.c_int, C.c_longlong
WANT = {
    "hx_batch_recon_buffer": ("int", ["hx_batch *", "float *"], I, [P, P]),
    "hx_batch_encode_f32_host_recon": ("int", ["hx_batch *", "const float *", "int", "unsigned char *", "long long", "int *", "float *"], I, [P, P, I, P, LL, P, P]),
    "hx_recon_delay": ("int", [], I, []),
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
    assert callable(api.recon_delay)
    for m in ("recon_buffer", "encode_host_recon"):
        assert callable(getattr(api.Batch, m)), m


def test_the_delay_is_the_documented_constant():
    """include/hmp3_amd.h states D = 2209 = the tag's encoder delay of 1680 and the decoder's 529; tests/test_recon_cases.py
    finds the same number as the lag of the decoder's output against the input"""
    from hmp3_amd import api
    assert api.recon_delay() == 2209 == 1680 + 529
    assert "hx_recon_delay() = 2209" in open(api.HEADER).read()


def test_setters_refuse_a_null_handle():
    from hmp3_amd import api
    L = api.lib()
    buf = (C.c_float * 4)()
    assert L.hx_batch_recon_buffer(None, buf) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_recon_buffer(None, None) == -1
    out, nb = (C.c_ubyte * 16)(), (C.c_int * 1)()
    assert L.hx_batch_encode_f32_host_recon(None, buf, 1, out, 16, nb, buf) == -1 and "null batch" in api.last_error()
