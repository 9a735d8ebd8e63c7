"""The inputs the file-ledger tests share (tests/test_gpu_ledger.py, tests/file_image_cases.py and the file-image, fetch and
tag suites behind it) and the host loop a ledger record restates (tests/test_ledger_host.py holds hx_ledger_update to it; the
GPU suite replays a device run's counters through it).  No GPU."""
import ctypes as C

import numpy as np

from hmp3_amd import api, synth

DRAIN = 32              # frames of silence a file may take behind its input

# ---- the small shape: files of 1 .. 20 calls in calls of 8 frames ----
# slots 0 - 5: the files; slot 6: a file of 15 calls, whose drain ends on the first frame of a call (the others' ends include
# one on the last frame of a call); slot 7 is never begun; slot 8 is begun and sits call 1 out
SMALL_NCALLS = [1, 7, 8, 9, 16, 20, 15, 5, 12]
NEVER, SITS_OUT, RESTART = 7, 8, 1


def small_pcm():
    return [synth.stream_pcm(6100 + i, nc, bursts=True).astype(np.float32) for i, nc in enumerate(SMALL_NCALLS)]


def small_restart_pcm():
    return synth.stream_pcm(6190, 6, bursts=True).astype(np.float32)


def small_batch():
    return api.Batch(api.default_control(bitrate=64), nstreams=len(SMALL_NCALLS), max_frames=8)


def small_counts(given, ncalls, call):
    c = [max(0, min(8, nc + DRAIN - g)) for nc, g in zip(ncalls, given)]
    if call == 1:
        c[SITS_OUT] = 0
    return c


def block(full, given, counts, nf):
    """the call's PCM [S, nf * 1152, ch]: stream s's next counts[s] frames of full[s], silence behind its end"""
    ch = full[0].shape[1]
    blk = np.zeros((len(full), nf * 1152, ch), np.float32)
    for s, n in enumerate(counts):
        part = full[s][given[s] * 1152:(given[s] + n) * 1152]
        blk[s, :len(part)] = part
    return blk


# ---- the loop a record restates: the command-line tool's Tagger::after_call per input call, its scan for the frame at which
# the drain ends and its MusicCRC, on hx_xing_toc, hx_xing_update_crc and hx_xing_update_info ----
HEAD_FLAGS = 1 | 2 | 8 | 4 | 0x40       # what `-X2` asks for: frames, bytes, scale, TOC, LAME info
VBR_SCALE = 50                          # a VBR file: the tag keeps its TOC at every bitrate


def tag_frame(x, fpc):
    """a new tag frame through hx_xing_header (which also empties x's seek points) -> (buffer, its size)"""
    buf = (C.c_ubyte * 2048)()
    n = api.lib().hx_xing_header(x, 44100 if fpc == 1 else 22050, 1, 1, 1, HEAD_FLAGS, 0, 0, VBR_SCALE, None, buf, None, None, 128)
    assert n > 0
    return buf, n


def finish(x, buf, n, fpc, frames, nbytes, crc, samples):
    sr = 44100 if fpc == 1 else 22050
    assert api.lib().hx_xing_update_info(x, frames, n + nbytes, VBR_SCALE, None, buf, None, None, samples, n + nbytes, 16000, sr, sr, crc) == 1
    return bytes(buf[:n])


def replay(f):
    """Tagger::after_call + job_write over an encode history f (ncalls, fpc, expected, samples, fr, by, end, crc_of)
    -> (tag frame, frames, bytes, crc, halvings of the seek table, the tag frame's size)"""
    L = api.lib()
    x = L.hx_xing_create()
    buf, n = tag_frame(x, f.fpc)
    counter, every, halvings = 0, 1, 0
    for u in range(f.ncalls):
        counter -= 1
        if counter <= 0:
            counter = L.hx_xing_toc(x, int(f.fr[u]) + 1, int(f.by[u]) + n)
            halvings += counter != every
            every = counter
    u = f.ncalls
    while u < len(f.fr) and f.fr[u - 1] < f.expected:
        u += 1
    assert f.fr[u - 1] >= f.expected and u - 1 == f.end
    frames, nbytes = int(f.fr[u - 1]), int(f.by[u - 1])
    crc = f.crc_of(0, nbytes)
    tag = finish(x, buf, n, f.fpc, frames, nbytes, crc, f.samples)
    L.hx_xing_destroy(x)
    return tag, frames, nbytes, crc, halvings, n


def record_tag(rec, fpc, samples):
    """the finished tag frame from a record alone: hx_xing_header, hx_xing_load_points, hx_xing_update_info"""
    L = api.lib()
    x = L.hx_xing_create()
    buf, n = tag_frame(x, fpc)
    assert n == rec.head_bytes
    api.xing_load_points(x, rec)
    tag = finish(x, buf, n, fpc, rec.frames, rec.bytes, rec.crc, samples)
    L.hx_xing_destroy(x)
    return tag
