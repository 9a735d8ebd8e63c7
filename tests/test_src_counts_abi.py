"""The converting calls under per-stream frame counts as an ABI (host only, no GPU): the three prototypes are in
include/hmp3_amd.h, the library exports them, and hmp3_amd.api binds them with the argument types the header declares."""
import ctypes as C

import pytest

NAMES = ["hx_batch_encode_src_counts_device", "hx_batch_encode_src_counts_host", "hx_multi_encode_src_counts_host"]
P, LL, I = C.c_void_p, C.c_longlong, C.c_int
# (handle, in, in_stride, frame_off, nframes, nfr, out, out_stride, out_bytes, in_used, ...)
COMMON = [P, P, LL, P, I, P, P, LL, P, P]
WANT = {NAMES[0]: COMMON + [P],             # ... stream
        NAMES[1]: COMMON + [P, P],          # ... stats, crc
        NAMES[2]: COMMON + [P, P]}


@pytest.mark.parametrize("name", NAMES)
def test_prototype_is_declared_exported_and_bound(name):
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert name in protos, "include/hmp3_amd.h does not declare " + name
    _, ret, params = protos[name]
    assert ret == "int"
    assert params[5] == "const int *" and params[3] == "const long long *" and params[9] == "long long *"
    if name != NAMES[0]:
        assert params[-2:] == ["int *", "unsigned short *"]
    f = getattr(api.lib(), name)            # (raises AttributeError if the library does not export it)
    assert f.restype is C.c_int
    assert list(f.argtypes) == WANT[name]


def test_existing_converting_calls_keep_their_signatures():
    from hmp3_amd import api
    protos = {p[0]: p for p in api.PROTOTYPES}
    assert len(protos["hx_batch_encode_src_device"][2]) == 10
    assert len(protos["hx_batch_encode_src_host"][2]) == 10 and len(protos["hx_multi_encode_src_host"][2]) == 10
