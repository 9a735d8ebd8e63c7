"""Finished files as an ABI (host only, no GPU): every export of include/hmp3_amd.h's "finished files" part is declared,
exported and bound; HX_FILE_TAG is 48 bytes; hx_file_tag_build - pure host code, the reference for k_file_tag - equals the three
hx_xing_* calls it stands for, byte for byte, on records driven through hx_ledger_update and over the parameter grid of the GPU
test, and leaves the record alone; the calls refuse what they can refuse without a device.  And the GPU test's shape
(tests/file_tag_cases.py) reaches, by the CPU oracle, the edges it exists for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import file_tag_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, LL = C.c_void_p, C.c_int, C.c_longlong
B, M, UC = "hx_batch *", "hx_multi *", "unsigned char *"
WANT = {
    "hx_file_tag_bytes": ("int", ["const HX_FILE_TAG *"], I, [P]),
    "hx_file_tag_build": ("int", ["const HX_LEDGER *", "const HX_FILE_TAG *", UC, "int"], I, [P, P, P, I]),
    "hx_batch_file_tags": ("int", [B, "const int *", "const HX_FILE_TAG *", "int", "void *"], I, [P, P, P, I, P]),
    "hx_batch_file_fetch_many": ("long long", [B, "const int *", "int", UC, "long long", "long long *"], LL, [P, P, I, P, LL, P]),
    "hx_batch_file_gather_device": ("int", [B, "const int *", "int", UC, "long long", "long long *", "void *"], I, [P, P, I, P, LL, P, P]),
    "hx_multi_file_tags": ("int", [M, "const int *", "const HX_FILE_TAG *", "int"], I, [P, P, P, I]),
    "hx_multi_file_fetch_many": ("long long", [M, "const int *", "int", UC, "long long", "long long *"], LL, [P, P, I, P, LL, P]),
}
FIELDS = ["samprate", "h_mode", "cr_bit", "original_bit", "flags", "kbps", "vbr_scale", "lowpass", "in_samplerate", "reserved", "samples_audio"]


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
    assert callable(api.file_tag_bytes) and callable(api.file_tag_build)
    for cls in (api.Batch, api.Multi):
        for m in ("file_tags", "file_fetch_many"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert callable(api.Batch.file_gather_device)


def test_tag_is_48_bytes_in_the_header_and_in_python(tmp_path):
    """sizeof and the offsets of HX_FILE_TAG as the C compiler lays the header's struct out, against the ctypes mirror"""
    from hmp3_amd import api
    assert [f[0] for f in api.FileTag._fields_] == FIELDS
    src = tmp_path / "tag.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmp3_amd.h"\nint main(void) { printf("%zu", sizeof(HX_FILE_TAG));\n' +
                   "".join('printf(" %%zu", offsetof(HX_FILE_TAG, %s));\n' % f for f in FIELDS) + "return 0; }\n")
    exe = str(tmp_path / "tag")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [48] + [4 * k for k in range(10)] + [40]
    assert C.sizeof(api.FileTag) == 48 and [getattr(api.FileTag, f).offset for f in FIELDS] == got[1:]


def host_records(api):
    """records through hx_ledger_update: short and long files, one whose 512-point table has halved once (every == 2), one
    without seek points, one with repeated points (calls that emit no frame), one ended with 0 frames, MPEG-2 (two frames a
    call), and a live one before its first call"""
    recs = {
        "short": K.drive(api, 5, seed=1),
        "mid": K.drive(api, 60, seed=2),
        "halved": K.drive(api, 530, seed=3),
        "no points": K.drive(api, 9, flags=0, seed=4),
        "repeated": K.drive(api, 12, stall=5, seed=5),
        "0 frames": K.drive(api, 3, fpc=0, seed=6),
        "two frames a call": K.drive(api, 21, fpc=2, seed=7),
        "not fed": api.ledger_open(4, 1, 0, 1),
    }
    assert recs["halved"].every == 2 and 256 <= recs["halved"].npt < 512
    assert recs["no points"].npt == 0
    pts = np.ctypeslib.as_array(recs["repeated"].pt)[:recs["repeated"].npt]
    assert (pts[1:, 0] == pts[:-1, 0]).any() and (np.diff(pts[:, 0]) >= 0).all()
    assert recs["0 frames"].ended and recs["0 frames"].frames == 0
    return recs


def test_build_equals_the_three_xing_calls_and_leaves_the_record():
    """every record x every slot's tag x the parameter grid: the bytes, the size, and the record bytewise unchanged"""
    from hmp3_amd import api
    recs = host_records(api)
    fired = set()
    n = 0
    for name, rec in recs.items():
        for s, c in enumerate(K.SLOTS):
            for tag in [K.slot_tag(api, s)] + K.grid(api, s):
                size = api.file_tag_bytes(tag)
                rec.head_bytes = size       # (the file's record is begun with its tag's size)
                before = rec.tobytes()
                want, hsize = K.three_calls(api, rec, tag)
                assert size == hsize and (size > 0) == bool(c["xing"]), (name, s)
                got = api.file_tag_build(rec, tag)
                assert got == want and len(got) == size, "%s, slot %d: hx_file_tag_build differs from the three calls" % (name, s)
                assert rec.tobytes() == before, "%s, slot %d: the record changed" % (name, s)
                if size and tag.samples_audio:
                    spf = 1152 if tag.samprate >= 32000 else 576
                    fired.add((K.trim_fires(rec.frames, spf, tag.samples_audio, tag.in_samplerate, tag.samprate)[0], tag.samples_audio > rec.frames * spf))
                n += 1
    assert n == len(recs) * len(K.SLOTS) * 21
    # both sides of the trimming compare, the wrapped one among them: it fired with the audio shorter and with it longer than
    # the frames, and it did not fire
    assert {(True, False), (True, True), (False, False)} <= fired, fired


def test_build_refuses_what_the_header_says():
    from hmp3_amd import api
    L = api.lib()
    tag = K.slot_tag(api, 0)
    size = api.file_tag_bytes(tag)
    rec = K.drive(api, 7, head=size)
    buf = (C.c_ubyte * 2048)(*([0x5A] * 2048))
    assert L.hx_file_tag_build(C.byref(rec), C.byref(tag), buf, 2048) == size and bytes(buf[size:size + 8]) == bytes([0x5A]) * 8
    for bad in ("head", "cap", "npt", "every"):
        r = api.Ledger.from_buffer_copy(rec)
        cap = 2048
        if bad == "head":
            r.head_bytes = size + 1
        elif bad == "cap":
            cap = size - 1
        elif bad == "npt":
            r.npt = 512
        else:
            r.every = 0
        buf = (C.c_ubyte * 2048)(*([0x5A] * 2048))
        assert L.hx_file_tag_build(C.byref(r), C.byref(tag), buf, cap) == 0 and bytes(buf) == bytes([0x5A]) * 2048, bad
    assert L.hx_file_tag_build(None, C.byref(tag), buf, 2048) == 0 and L.hx_file_tag_build(C.byref(rec), None, buf, 2048) == 0
    assert L.hx_file_tag_build(C.byref(rec), C.byref(tag), None, 2048) == 0 and L.hx_file_tag_bytes(None) == 0
    # no tag: size 0, nothing built
    none = K.slot_tag(api, K.UNTAGGED)
    assert api.file_tag_bytes(none) == 0 and api.file_tag_build(api.ledger_open(3, 1, 0, 0), none) == b""
    # a sample rate MPEG audio does not have
    odd = K.slot_tag(api, 0)
    odd.samprate = 11025
    assert api.file_tag_bytes(odd) == 0


def test_tag_bytes_equals_xing_header_over_rates_and_bitrates():
    from hmp3_amd import api
    L = api.lib()
    x = L.hx_xing_create()
    buf = (C.c_ubyte * 2048)()
    sizes = set()
    for sr in (16000, 22050, 24000, 32000, 44100, 48000, 8000):
        for mode in (0, 3):
            for vbr in (-1, 50):
                for kbps in (0, 8, 32, 48, 56, 64, 128, 160, 320, 77):
                    for flags in (0x4F, 0x0B, 0x7F, 0):
                        t = api.FileTag(sr, mode, 1, 1, flags, kbps, vbr, 16000, sr, 0, 1000)
                        want = L.hx_xing_header(x, sr, mode, 1, 1, flags, 0, 0, vbr, None, buf, None, None, kbps)
                        assert api.file_tag_bytes(t) == want
                        sizes.add(want)
    L.hx_xing_destroy(x)
    assert 0 in sizes and max(sizes) == 1440 and len(sizes) > 20


def test_refusals_that_need_no_device():
    from hmp3_amd import api
    L = api.lib()
    buf, idx, tag = (C.c_ubyte * 64)(), (C.c_int * 1)(0), api.FileTag()
    off = (C.c_longlong * 2)()
    assert L.hx_batch_file_tags(None, idx, C.byref(tag), 1, None) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_file_fetch_many(None, idx, 1, buf, 64, off) == -1 and "null batch" in api.last_error()
    assert L.hx_batch_file_gather_device(None, idx, 1, buf, 64, off, None) == -1 and "null batch" in api.last_error()
    assert L.hx_multi_file_tags(None, idx, C.byref(tag), 1) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_file_fetch_many(None, idx, 1, buf, 64, off) == -1 and "null handle" in api.last_error()
    assert L.hx_multi_file_tags(None, None, C.byref(tag), 1) == -1 and L.hx_multi_file_fetch_many(None, None, 1, buf, 64, off) == -1


def test_header_documents_the_contract():
    text = open(os.path.join(ROOT, "include", "hmp3_amd.h")).read()
    at = text.index("---- file images:")
    section = text[at:text.index("---- host placement", at)]
    assert "---- finished files:" in section and "only k_file_tag writes them, when asked" in section and "no kernel ever writes them" not in text
    not_covered = section[section.index("Not covered:"):]
    assert "building the tag" not in section
    for what in ("pipelined host", "checkpoint blob", "hx_enc_*", "page-locked"):
        assert what in not_covered[not_covered.rindex("Not covered:"):], what
    assert "also the image of hx_batch_file_gather_device" in text


def test_gpu_shape_reaches_its_edges_by_the_oracle():
    """the GPU test's seven slots through the CPU oracle and hx_ledger_update: slot LONG's table has halved once; the slot with
    counts only holds no points; a record holds repeated points (a call that emitted no frame); the CBR slot below 64 kbit/s holds points while its frame has no
    TOC; the tag sizes differ; behind call MID_CALL three files are live and others have ended; and with the files' true lengths the trimming rule does
    not fire while the grid's other lengths make it fire from both sides"""
    from hmp3_amd import api, synth
    from oracle import oracle as O
    mid = K.oracle_records(api, O, synth, stop=K.MID_CALL)
    end = K.oracle_records(api, O, synth)
    assert all(r.ended for r in end) and sum(not r.ended for r in mid) >= 3 and any(r.ended for r in mid)
    assert end[K.LONG].every == 2 and end[K.LONG].npt >= 256 and all(end[s].every == 1 for s in range(len(end)) if s != K.LONG)
    assert end[K.COUNTS_ONLY].npt == 0 and end[K.UNTAGGED].npt == 0 and end[K.UNTAGGED].head_bytes == 0
    assert end[K.MPEG2].frames_per_call == 2
    repeats = [int((np.diff(np.ctypeslib.as_array(r.pt)[:r.npt, 0]) == 0).sum()) if r.npt > 1 else 0 for r in end]
    assert any(repeats), "no record holds repeated seek points"
    cbr = K.slot_tag(api, K.NO_TOC_CBR)
    assert end[K.NO_TOC_CBR].npt > 0 and cbr.flags & 4 and cbr.vbr_scale == -1 and cbr.kbps == 48
    frame = api.file_tag_build(end[K.NO_TOC_CBR], cbr)
    assert frame[4 + 17:4 + 17 + 4] == b"Info" and frame[4 + 17 + 7] & 4 == 0 and len(frame) == api.file_tag_bytes(cbr)
    heads = [K.slot_head(api, s) for s in range(len(K.SLOTS))]
    assert heads[K.UNTAGGED] == 0 and len(set(heads)) >= 5 and {h % 16 for h in heads if h} > {0}, heads
    ones = 0
    for s, r in enumerate(end):
        if not K.SLOTS[s]["xing"] & 2:
            continue
        spf = 1152 if r.frames_per_call == 1 else 576
        true = K.true_samples(s)
        sr = K.slot_tag(api, s).samprate
        fires, d = K.trim_fires(r.frames, spf, true, sr, sr)
        assert not fires and K.TAIL - 1680 <= d <= K.TAIL - 1680 + spf, (s, d)       # (an MPEG-2 drain may end one frame late)
        ones += K.trim_fires(r.frames, spf, 1, sr, sr)[0]
        fires, d = K.trim_fires(r.frames, spf, true + 10 * 1152, sr, sr)
        assert fires and d > (1 << 63), (s, d)
    assert ones >= 3, "samples_audio = 1 makes the rule fire for the files of more than 5 calls"
