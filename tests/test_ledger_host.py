"""The file ledger's record on the host (include/hmp3_amd.h, HX_LEDGER; hmp3_amd/csrc/hx_xhead.cpp): hx_ledger_open,
hx_ledger_update and hx_xing_load_points against the loop they restate - the command-line tool's Tagger::after_call per input
call, its scan for the frame at which the drain ends and its MusicCRC - written out here in Python on hx_xing_toc,
hx_xing_update_crc and hx_xing_update_info (tests/test_xing_tag.py pins those to the reference).  No GPU.

hx_xing keeps 512 seek points (the reference's table, xhead.c:71), so the table is halved after 512, 1024 and 2048 sampled
calls: the random files have 1 - 1000 calls (none or one halving), and two fixed longer ones reach two and three."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hmp3_amd import api
from ledger_cases import record_tag, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class File:
    """a random encode history: per frame fed (input calls, then drain calls of silence) the stream's frames / bytes out so
    far, and the bytes themselves.  The encoder runs `lag` frames behind its input; the drain goes on for `after` frames
    past the one at which it ends"""

    def __init__(self, rng, ncalls, fpc, lag0=None, after=5):
        self.ncalls, self.fpc, self.expected = ncalls, fpc, ncalls * fpc
        fr, lag = [], int(rng.integers(0, 3 * fpc + 1)) if lag0 is None else lag0
        while not fr or not (len(fr) >= ncalls and fr[-1] >= self.expected):
            if lag0 is None and rng.random() < 0.1:
                lag = int(rng.integers(0, 3 * fpc + 1))
            fr.append(max(fr[-1] if fr else 0, (len(fr) + 1) * fpc - lag))
        self.end = len(fr) - 1                      # the frame fed at which the drain ends
        for _ in range(after):
            fr.append(fr[-1] + int(rng.integers(0, fpc + 1)))
        sizes = rng.integers(96, 1200, fr[-1] + 1)
        cum = np.concatenate([[0], np.cumsum(sizes)])
        self.fr = np.array(fr, np.int64)
        self.by = cum[self.fr]
        self.data = rng.integers(0, 256, int(self.by[-1]), dtype=np.uint8)
        self.samples = ncalls * 1152 - int(rng.integers(0, 1152))

    def crc_of(self, a, b, seed=0):
        d = self.data[a:b]
        return int(api.lib().hx_xing_update_crc(seed, d.ctypes.data, len(d)))


def through_ledger(f, cuts, head_bytes):
    """the same history as calls [cuts[k], cuts[k + 1]) of hx_ledger_update (equal cuts: a call of n = 0) -> (record, where
    the end fell: (f, n) of the call that ended the file)"""
    rec = api.ledger_open(f.ncalls, f.fpc, head_bytes, 1)
    ended_at = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        before = rec.tobytes()
        st = np.stack([f.fr[a:b], f.by[a:b]], axis=1).astype(np.int32)
        by0 = int(f.by[a - 1]) if a else 0
        nb = int(f.by[b - 1]) - by0 if b > a else 0
        crc, run = np.zeros(b - a, np.uint16), 0
        for k in range(b - a):
            run = f.crc_of(int(f.by[a + k - 1]) if a + k else 0, int(f.by[a + k]), run)
            crc[k] = run
        was_ended = bool(rec.ended)
        ended = api.ledger_update(rec, st, crc, nb)
        if b == a:
            assert rec.tobytes() == before and not ended, "a call of n = 0 changed the record"
        elif was_ended:
            assert not ended and rec.call_bytes == 0
            rec2 = api.Ledger.from_buffer_copy(before)
            rec2.call_bytes = 0
            assert rec.tobytes() == rec2.tobytes(), "a call after the end changed more than call_bytes"
        elif ended:
            assert a <= f.end < b and rec.fed == f.end + 1 and rec.call_bytes == int(f.by[f.end]) - by0
            ended_at = (f.end - a, b - a)
        else:
            assert rec.fed == b and rec.call_bytes == nb and not rec.ended
    return rec, ended_at


def random_cuts(rng, total, force=None, end=None):
    """call boundaries 0 = c0 <= c1 <= ... = total, some calls empty; force "first" / "last": the frame `end` is the first /
    the last of its call"""
    cuts = {0, total}
    at = 0
    while at < total:
        at = min(total, at + int(rng.integers(1, 97)))
        cuts.add(at)
    if force == "first":
        cuts.add(end)
    if force == "last":
        cuts.add(end + 1)
    cuts = sorted(cuts)
    out = []
    for c in cuts:
        out.append(c)
        if rng.random() < 0.15:
            out.append(c)           # an n = 0 call
    return out


def run_case(rng, ncalls, fpc, lag0=None, force=None):
    f = File(rng, ncalls, fpc, lag0)
    tag, frames, nbytes, crc, halvings, n = replay(f)
    cuts = random_cuts(rng, len(f.fr), force, f.end)
    rec, ended_at = through_ledger(f, cuts, n)
    assert rec.ended and ended_at is not None
    assert (rec.frames, rec.bytes, rec.crc) == (frames, nbytes, crc), (ncalls, fpc)
    assert any(rec.pad0) + any(rec.pad1) == 0
    assert record_tag(rec, fpc, f.samples) == tag, (ncalls, fpc)
    return {"first": ended_at[0] == 0, "last": ended_at[0] == ended_at[1] - 1, "no_drain": f.end == ncalls - 1, "halvings": halvings}


def test_update_against_the_loop_it_restates():
    """seeded random files of 1 - 1000 calls, 1 and 2 frames per call, cut into calls of 0 - 96 frames that go on past the
    end, and two longer files: the tag frame and (frames, bytes, crc) from the record equal the replayed loop's.  Every kind
    of end and 0, 1, 2 and 3 halvings of the seek table must have occurred"""
    rng = np.random.default_rng(20251)
    seen = []
    sizes = [1, 2, 3, 7, 8, 9, 95, 96, 97, 511, 512, 513, 1000] + [int(v) for v in rng.integers(1, 1001, 35)]
    for i, ncalls in enumerate(sizes):
        fpc = 1 + (i & 1)
        seen.append(run_case(rng, ncalls, fpc, lag0=0 if i % 5 == 0 else None, force=(None, "first", "last")[i % 3]))
    seen.append(run_case(rng, 1100, 1))         # halvings at 512 and 1024 sampled calls
    seen.append(run_case(rng, 2100, 2))         # ... and at 2048
    assert any(s["first"] for s in seen), "no file ended at f = 0 of a call"
    assert any(s["last"] for s in seen), "no file ended at f = n - 1 of a call"
    assert any(s["no_drain"] for s in seen), "no file ended at u = ncalls - 1"
    assert any(not s["no_drain"] for s in seen)
    assert {s["halvings"] for s in seen} >= {0, 1, 2, 3}, sorted({s["halvings"] for s in seen})


def test_closed_record_is_left_alone():
    """a record that is not open is bytewise unchanged by a call; so is an open one by a call of n = 0"""
    rec = api.Ledger()
    st, crc = np.array([[5, 2000], [6, 2400]], np.int32), np.array([1, 2], np.uint16)
    assert not api.ledger_update(rec, st, crc, 2400) and rec.tobytes() == bytes(C.sizeof(api.Ledger))
    rec = api.ledger_open(4, 1, 417, 1)
    before = rec.tobytes()
    assert not api.ledger_update(rec, st[:0], crc[:0], 0) and rec.tobytes() == before
    assert rec.open == 1 and rec.every == 1 and rec.ncalls == 4 and rec.head_bytes == 417 and rec.flags == 1


def test_record_without_seek_points_keeps_none():
    """flags = 0: the end, the bytes and the CRC as with seek points, and no point is stored"""
    rng = np.random.default_rng(7)
    f = File(rng, 40, 1)
    rec = api.ledger_open(f.ncalls, 1, 0, 0)
    st = np.stack([f.fr, f.by], axis=1).astype(np.int32)
    crc, run = np.zeros(len(f.fr), np.uint16), 0
    for k in range(len(f.fr)):
        run = f.crc_of(int(f.by[k - 1]) if k else 0, int(f.by[k]), run)
        crc[k] = run
    assert api.ledger_update(rec, st, crc, int(f.by[-1]))
    assert (rec.frames, rec.bytes, rec.crc, rec.fed) == (int(f.fr[f.end]), int(f.by[f.end]), f.crc_of(0, int(f.by[f.end])), f.end + 1)
    assert rec.npt == 0 and rec.toc_counter == 0 and not np.ctypeslib.as_array(rec.pt).any()


def test_layout_is_the_headers(tmp_path):
    """sizeof(HX_LEDGER) is a multiple of 16, and the ctypes mirrors have the size and the field offsets a C compiler gives
    the header's structs"""
    exe = str(tmp_path / "ledger_layout_check")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "ledger_layout_check.c")])
    mirrors = {"HX_LEDGER": api.Ledger, "HX_LEDGER_OPEN": api.LedgerOpen}
    fields = {name: 0 for name in mirrors}
    for line in subprocess.check_output([exe], text=True).splitlines():
        what, a, *b = line.split()
        if what == "sizeof":
            assert C.sizeof(mirrors[a]) == int(b[0]), line
        elif what == "HX_LEDGER_POINTS":
            assert api.LEDGER_POINTS == int(a)
        else:
            struct, field = what.split(".")
            d = getattr(mirrors[struct], field)
            assert (d.offset, d.size) == (int(a), int(b[0])), line
            fields[struct] += 1
    assert fields == {name: len(m._fields_) for name, m in mirrors.items()}
    assert C.sizeof(api.Ledger) % 16 == 0
