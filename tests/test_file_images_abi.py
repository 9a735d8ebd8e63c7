"""File images as an ABI (host only, no GPU): every export of include/hmp3_amd.h's "file images" section is declared,
exported and bound; HX_LEDGER_BRIEF is 32 bytes; hx_ledger_brief - pure host code, the reference for k_ledger_brief - is held
to records driven through hx_ledger_update; the calls refuse what they can refuse without a device.  And the inputs of the
GPU tests (tests/file_image_cases.py) reach, by the CPU oracle, the edges they exist for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, LL, U = C.c_void_p, C.c_int, C.c_longlong, C.c_uint
B, M, UC = "hx_batch *", "hx_multi *", "unsigned char *"
WANT = {
    "hx_ledger_brief": ("void", ["const HX_LEDGER *", "unsigned", "HX_LEDGER_BRIEF *"], None, [P, U, P]),
    "hx_batch_file_images": ("int", [B, "long long"], I, [P, LL]),
    "hx_batch_file_image_cap": ("long long", ["const hx_batch *"], LL, [P]),
    "hx_batch_file_image_ptr": (UC, [B, "int"], P, [P, I]),
    "hx_batch_ledger_poll": ("int", [B, "HX_LEDGER_BRIEF *"], I, [P, P]),
    "hx_batch_ledger_poll_device": ("int", [B, "HX_LEDGER_BRIEF *", "void *"], I, [P, P, P]),
    "hx_batch_file_fetch": ("long long", [B, "int", UC, "long long"], LL, [P, I, P, LL]),
    "hx_batch_encode_s16_host_files": ("int", [B, "const int16_t *", "int"], I, [P, P, I]),
    "hx_batch_encode_f32_host_files": ("int", [B, "const float *", "int"], I, [P, P, I]),
    "hx_batch_encode_src_files_host": ("int", [B, "const unsigned char *", "long long", "const long long *", "int", "const int *", "long long *"],
                                       I, [P, P, LL, P, I, P, P]),
    "hx_multi_file_images": ("int", [M, "long long"], I, [P, LL]),
    "hx_multi_ledger_poll": ("int", [M, "HX_LEDGER_BRIEF *"], I, [P, P]),
    "hx_multi_file_fetch": ("long long", [M, "int", UC, "long long"], LL, [P, I, P, LL]),
    "hx_multi_encode_s16_host_files": ("int", [M, "const int16_t *", "int"], I, [P, P, I]),
    "hx_multi_encode_f32_host_files": ("int", [M, "const float *", "int"], I, [P, P, I]),
    "hx_multi_encode_src_files_host": ("int", [M, "const unsigned char *", "long long", "const long long *", "int", "const int *", "long long *"],
                                       I, [P, P, LL, P, I, P, P]),
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
    assert callable(api.ledger_brief)
    for cls in (api.Batch, api.Multi):
        for m in ("file_images", "ledger_poll", "file_fetch", "encode_host_files", "encode_host_files_image"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    for m in ("file_image_cap", "file_image_ptr", "ledger_poll_device"):
        assert callable(getattr(api.Batch, m))
    assert callable(api.SrcBatch.encode_src_files_host) and callable(api.SrcMulti.encode_src_files_host)


def test_brief_is_32_bytes_in_the_header_and_in_python(tmp_path):
    """sizeof and the offsets of HX_LEDGER_BRIEF as the C compiler lays the header's struct out, against the ctypes mirror"""
    from hmp3_amd import api
    fields = [f[0] for f in api.LedgerBrief._fields_]
    assert fields == ["open", "ended", "fed", "frames", "bytes", "crc", "call_bytes", "image_bytes"]
    src = tmp_path / "brief.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmp3_amd.h"\nint main(void) { printf("%zu", sizeof(HX_LEDGER_BRIEF));\n' +
                   "".join('printf(" %%zu", offsetof(HX_LEDGER_BRIEF, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "brief")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [32] + [4 * k for k in range(8)]
    assert C.sizeof(api.LedgerBrief) == 32 and [getattr(api.LedgerBrief, f).offset for f in fields] == got[1:]


def by_hand(rec, image_bytes):
    return np.array([rec.open, rec.ended, rec.fed, rec.frames, rec.bytes, rec.crc, rec.call_bytes, image_bytes], np.int64).astype(np.uint32).tobytes()


def test_brief_of_records_driven_through_update():
    """synthetic counters: a closed record; an open one before its first call; across calls of 3 frames of a file of 7 calls
    whose drain ends on the second frame of a call (a mid-call end: call_bytes < out_bytes); the ended record after a further
    call (call_bytes = 0); and image_bytes below the record's bytes, as after an overflow - it is passed through, never taken
    from the record"""
    from hmp3_amd import api
    closed = api.Ledger()
    assert api.ledger_brief(closed, 0).tobytes() == bytes(32)
    assert api.ledger_brief(closed, 77).tobytes() == by_hand(closed, 77)
    rec = api.ledger_open(7, 1, 13, 1)
    assert api.ledger_brief(rec, 0).tobytes() == by_hand(rec, 0) and api.ledger_brief(rec, 0).open == 1
    rng = np.random.default_rng(11)
    fr, by, seen = 0, 0, []
    for call in range(5):
        st = np.zeros((3, 2), np.int32)
        for f in range(3):
            fed = call * 3 + f
            fr = max(0, fed + 1 - 2)        # the encoder runs two frames behind: frame 7 comes out at fed = 8, the 3rd call's last
            fr += int(fed == 7)             # ... one early: the drain ends at fed = 7, the second frame of call 2
            by += int(rng.integers(100, 900)) if fr else 0
            st[f] = fr, by
        nb = int(st[2, 1] - (seen[-1][1] if seen else 0))
        was = rec.ended
        ended = api.ledger_update(rec, st, rng.integers(0, 65536, 3).astype(np.uint16), nb)
        seen.append((fr, int(st[2, 1])))
        for img in (rec.bytes, max(0, rec.bytes - 5), 0):
            b = api.ledger_brief(rec, img)
            assert b.tobytes() == by_hand(rec, img) and b.image_bytes == img
        if ended:
            assert call == 2 and 0 < rec.call_bytes < nb and rec.fed == 8, (call, rec.call_bytes, nb)
        if was:
            assert rec.call_bytes == 0 and api.ledger_brief(rec, rec.bytes).ended == 1
    assert rec.ended
    # null arguments: nothing is written, nothing is read
    out = api.LedgerBrief(1, 2, 3, 4, 5, 6, 7, 8)
    api.lib().hx_ledger_brief(None, 9, C.byref(out))
    assert out.tobytes() == by_hand(api.Ledger(open=1, ended=2, fed=3, frames=4, bytes=5, crc=6, call_bytes=7), 8)
    api.lib().hx_ledger_brief(C.byref(rec), 9, None)


def test_refusals_that_need_no_device():
    from hmp3_amd import api
    L = api.lib()
    buf = (C.c_ubyte * 64)()
    assert L.hx_batch_file_images(None, 4096) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_file_images(None, -1) == -1
    assert L.hx_batch_file_image_cap(None) == 0 and L.hx_batch_file_image_ptr(None, 0) is None
    assert L.hx_batch_ledger_poll(None, buf) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_ledger_poll_device(None, buf, None) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_file_fetch(None, 0, buf, 64) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_encode_s16_host_files(None, buf, 1) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_encode_f32_host_files(None, buf, 1) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_encode_src_files_host(None, buf, 64, None, 1, None, None) == -1 and "null batch" in api.last_error()
    assert L.hx_multi_file_images(None, 4096) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_ledger_poll(None, buf) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_file_fetch(None, 0, buf, 64) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_encode_s16_host_files(None, buf, 1) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_encode_f32_host_files(None, buf, 1) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_encode_src_files_host(None, buf, 64, None, 1, None, None) == -1 and "null handle" in api.last_error()


def test_header_documents_the_contract():
    text = open(os.path.join(ROOT, "include", "hmp3_amd.h")).read()
    at = text.index("---- file images:")
    section = text[at:text.index("---- host placement", at)]
    assert text.index("---- file ledger:") < at and "Not covered:" in section and "status bit 64" in section
    assert "64 = a file did not fit its image" in text


def test_small_shape_reaches_its_edges_by_the_oracle():
    """the GPU test's small shape through the CPU oracle: a file ends with 0 < call_bytes < out_bytes; a fed live stream gets a
    piece of 0 bytes; the pieces start at 14 of the 16 residues mod 16; the restarted slot gets pieces of both files"""
    import file_image_cases as K
    from hmp3_amd import api
    from oracle import oracle as O
    pieces = K.oracle_pieces(api, O)
    assert any(live and 0 < cb < nb for s, c, n, nb, cb, live, res in pieces), "no file ends inside a call's bytes"
    assert any(live and cb == 0 and n > 0 for s, c, n, nb, cb, live, res in pieces), "no fed live stream has a piece of 0 bytes"
    assert len({res for s, c, n, nb, cb, live, res in pieces if cb > 0}) >= 14
    mine = [c for s, c, n, nb, cb, live, res in pieces if s == K.RESTART and cb > 0]
    assert min(mine) < K.RESTART_AT <= max(mine)
    assert not any(s == K.NEVER for s, *_ in pieces)
