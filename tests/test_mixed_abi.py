"""Mixed batches as an ABI (host only, no GPU): the four exports of include/hmp3_amd.h's "mixed batches" section are declared,
exported and bound, and create validates the menu before it looks at a device - entries that differ in channel count pass
hx_batch_create_mixed and nothing else, MPEG-1 beside MPEG-2 rates and the first-generation allocator stay refused by name."""
import ctypes as C

import pytest

P, I = C.c_void_p, C.c_int
WANT = {
    "hx_batch_create_mixed": ("hx_batch *", ["int", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P, [I, I, P, I, P, P, I]),
    "hx_multi_create_mixed": ("hx_multi *", ["int", "const int *", "int", "const HX_E_CONTROL *", "int", "const HX_SOURCE *", "const int *", "int"], P,
                              [I, P, I, P, I, P, P, I]),
    "hx_batch_pcm_channels": ("int", ["const hx_batch *"], I, [P]),
    "hx_batch_stream_channels": ("int", ["const hx_batch *", "int"], I, [P, I]),
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
        for m in ("mixed", "pcm_channels", "stream_channels"):
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_accessors_refuse_a_null_batch():
    from hmp3_amd import api
    L = api.lib()
    assert L.hx_batch_pcm_channels(None) == 0 and L.hx_batch_stream_channels(None, 0) == -1
    ec = api.default_control(bitrate=64)
    assert not L.hx_batch_create_mixed(0, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()
    assert not L.hx_multi_create_mixed(0, None, 2, C.byref(ec), 0, None, None, 4) and "bad arguments" in api.last_error()


def create(fn, menu, sources=None):
    """-> hx_last_error of a create over `menu` on this GPU-less machine (the handle, if one came back, is released)"""
    from hmp3_amd import api
    L = api.lib()
    ecs = (api.EControl * len(menu))(*[api.default_control(**kw) for kw in menu])
    srcs = (api.Source * len(menu))(*sources) if sources else None
    h = getattr(L, fn)(0, 3, ecs, len(menu), srcs, None, 4)
    if h:
        L.hx_batch_destroy(h)
        return ""
    return api.last_error()


def test_mpeg1_beside_mpeg2_rates_stays_refused():
    assert create("hx_batch_create_mixed", [dict(bitrate=64), dict(bitrate=32, samprate=22050)]).startswith("menu entry 1: MPEG-1 and MPEG-2")


def test_dual_channel_beside_the_others_stays_refused():
    assert create("hx_batch_create_mixed", [dict(bitrate=64), dict(bitrate=64, mode=2)]).startswith("menu entry 1: intensity-stereo / dual-channel")


def test_stereo_and_mono_entries_pass_the_menu_check_of_the_mixed_create_only():
    menu = [dict(bitrate=64), dict(bitrate=64, mode=3)]
    assert not create("hx_batch_create_mixed", menu).startswith("menu entry")
    assert create("hx_batch_create_menu", menu).startswith("menu entry 1: mono and stereo")


def test_a_converting_menu_of_both_output_channel_counts_passes_entry_validation():
    """a mono source, a stereo source, and a stereo source summed to mono"""
    from hmp3_amd import api
    menu = [dict(bitrate=64, mode=3, samprate=32000), dict(bitrate=64), dict(bitrate=64, samprate=48000)]
    sources = [api.Source(8, 0, 0, 0), api.Source(16, 0, 0, 0), api.Source(24, 0, 0, 1)]
    assert not create("hx_batch_create_mixed", menu, sources).startswith("menu entry")
    assert create("hx_batch_create_menu", menu, sources).startswith("menu entry 1: mono and stereo")
