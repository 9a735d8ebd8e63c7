"""The device side of the file-image suites (tests/test_gpu_file_images.py, tests/test_gpu_file_fetch_many.py,
tests/test_gpu_file_tags.py): reading and prefilling a batch's file images through the HIP runtime, and Files, a batch with
file images and its twin without that are fed the same calls while the host keeps a model of every image
(tests/file_image_cases.py holds the shapes)."""
import numpy as np

import file_image_cases as K
import gpu_support as G
from file_image_cases import PAT, rows_block
from gpu_support import CallBufs, cur_stream, hip, sync
from hmp3_amd import api
from ledger_cases import DRAIN
from output_checks import same_outputs


def pitch_of(b):
    """the bytes from one slot's image to the next: cap rounded up to 16 (the header's allocation rule)"""
    return (b.file_image_cap() + 15) & ~15


def image_of(b, s):
    """slot s's image, cap bytes; the bytes from cap to the next slot's image must hold the guard pattern"""
    out = np.zeros(pitch_of(b), np.uint8)
    assert hip().hipMemcpy(out.ctypes.data, b.file_image_ptr(s), len(out), 2) == 0
    assert (out[b.file_image_cap():] == PAT).all(), "slot %d: a byte at or beyond cap was written" % s
    return out[:b.file_image_cap()]


def prefill(b):
    for s in range(b.n):
        assert b.file_image_ptr(s) == b.file_image_ptr(0) + s * pitch_of(b) and b.file_image_ptr(s) % 16 == 0
    assert hip().hipMemset(b.file_image_ptr(0), PAT, b.n * pitch_of(b)) == 0
    sync()


def file_bufs(b, nf, shift=0, extra=0):
    """the ledger suite's buffers - rows, byte counts, counters, per-frame CRCs - with the first row `shift` bytes past a
    16-byte boundary and `extra` bytes added to the stride"""
    return CallBufs(b, nf, shift=shift, extra=extra, counters=True, crc=True)


class Files:
    """a batch with file images (b: a Batch, or a Multi when `multi`) and its twin t without, both with a ledger; `want` the
    host's records, `model` the host's images"""

    def __init__(self, make, full, cap, f32=True, shift=0, extra=0, make_b=None, prefilled=True):
        self.t, self.b = make(), (make_b or make)()
        self.full, self.cap, self.f32, self.shift, self.extra = list(full), cap, f32, shift, extra
        self.S, self.P = self.t.n, self.t.pcm_channels()
        self.b.file_images(cap)
        self.direct = prefilled and hasattr(self.b, "file_image_ptr")
        if self.direct:
            assert self.b.file_image_cap() == cap
            prefill(self.b)
        self.want = [api.Ledger() for _ in range(self.S)]
        self.model = [np.full(cap, PAT, np.uint8) for _ in range(self.S)]
        self.head, self.has, self.length = [0] * self.S, [False] * self.S, [0] * self.S
        self.given, self.calls, self.pieces, self.status = [0] * self.S, 0, [], 0

    def begin(self, idx, ncalls, heads):
        fpc = [self.t.stream_frames_per_block(s) for s in idx]
        for h in (self.b, self.t):
            h.ledger_begin(idx, ncalls, heads, **({} if isinstance(h, api.Multi) else {"stream": cur_stream()}))
        for e, s in enumerate(idx):
            self.want[s] = api.ledger_open(ncalls[e], fpc[e], heads[e], 0)
            self.head[s], self.has[s], self.length[s] = heads[e], True, 0

    def block(self, counts, nf):
        return rows_block(self.full, self.given, counts, nf, self.P, np.float32 if self.f32 else np.int16)

    def device_call(self, h, blk, counts, nf, shift=0, extra=0, submit=False, out=None):
        h.frame_counts(counts)
        return G.device_call(h, blk, nf, (out or file_bufs(h, nf, shift, extra)).set_on(h), submit=submit, f32=self.f32)

    def host_update(self, counts, rows, nb, st, cr):
        """the twin's outputs of one call into the host's records and images"""
        for s, n in enumerate(counts):
            live = bool(self.want[s].open and not self.want[s].ended)
            api.ledger_update(self.want[s], st[s, :n], cr[s, :n], nb[s])
            w = self.want[s]
            if n and w.open and self.has[s]:
                at = self.head[s] + w.bytes - w.call_bytes
                piece = rows[s, :w.call_bytes]
                fit = max(0, min(len(piece), self.cap - at))
                self.model[s][at:at + fit] = piece[:fit]
                self.length[s] = max(0, min(w.bytes, self.cap - self.head[s]))
                if fit < len(piece):
                    self.status |= 64
                self.pieces.append(dict(s=s, n=n, nb=int(nb[s]), cb=int(w.call_bytes), live=live, at=at, cut=fit < len(piece)))
            self.given[s] += n

    def check(self, tag, read=True):
        polls = self.b.ledger_poll()
        if read:
            recs = self.b.ledger_read(list(range(self.S)))
            trecs = self.t.ledger_read(list(range(self.S)))
        for s in range(self.S):
            assert polls[s].tobytes() == api.ledger_brief(self.want[s], self.length[s]).tobytes(), "%s: slot %d's brief (image_bytes %d, want %d)" % (
                tag, s, polls[s].image_bytes, self.length[s])
            if read:
                assert recs[s].tobytes() == self.want[s].tobytes() == trecs[s].tobytes(), "%s: slot %d's record" % (tag, s)
                assert polls[s].tobytes() == api.ledger_brief(recs[s], polls[s].image_bytes).tobytes()
            if self.direct:
                got = image_of(self.b, s)
                bad = np.flatnonzero(got != self.model[s])
                assert not len(bad), "%s: slot %d's image differs from the model at byte %d (head %d, length %d, cap %d; %d bytes differ)" % (
                    tag, s, bad[0], self.head[s], self.length[s], self.cap, len(bad))
            if self.has[s] and self.head[s] + self.length[s] <= self.cap + 64:
                got = self.b.file_fetch(s, self.head[s] + self.length[s], fill=0x3C)
                assert got == bytes([0x3C]) * self.head[s] + self.model[s][self.head[s]:self.head[s] + self.length[s]].tobytes(), "%s: fetch of slot %d" % (tag, s)

    def step(self, counts, nf=None, feed=None, check=True, read=True):
        """one call on both: the twin by a plain device call, the image batch the same way or through feed(blk, counts, nf)"""
        nf = nf or max(counts)
        blk = self.block(counts, nf)
        tw = self.device_call(self.t, blk, counts, nf)
        got = self.device_call(self.b, blk, counts, nf, self.shift, self.extra) if feed is None else feed(blk, counts, nf)
        sync()
        tag = "call %d" % self.calls
        twin = tw.host()
        if got is not None:
            same_outputs(got.host(), twin, counts, tag)
        self.host_update(counts, *twin)
        self.calls += 1
        if check:
            self.check(tag, read)
        return twin

    def run(self, ncalls, call, stop=None, **kw):
        """calls of `call` frames under counts until every begun file has ended"""
        while True:
            counts = [0 if (not self.want[s].open or self.want[s].ended) else max(0, min(call, ncalls[s] + DRAIN - self.given[s])) for s in range(self.S)]
            if not any(counts) or (stop and self.calls >= stop):
                break
            self.step(counts, nf=call, **kw)

    def close(self, status=None):
        assert self.b.status() == (self.status if status is None else status) and self.t.status() == 0
        self.b.close()
        self.t.close()


def vbr_small():
    return api.Batch(api.default_control(), nstreams=len(K.SMALL_NCALLS), max_frames=8)
