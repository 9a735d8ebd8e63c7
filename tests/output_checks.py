"""What a call's optional outputs must equal, where more than one GPU suite asserts it: the dense image against the rows
(tests/test_gpu_dense.py's contract), the per-frame CRCs from the call's own counters (tests/test_gpu_crc.py's), packets, sizes
and counters against the oracle's frames (tests/test_gpu_packets.py's), and the three checks of a call under per-stream counts
(tests/test_gpu_frame_counts.py's).  Host arrays in, assertions out; the buffers come as arguments (gpu_support.CallBufs)."""
import numpy as np

from gpu_support import FILL, host_crc


def round16(n):
    return (np.asarray(n, dtype=np.int64) + 15) & ~15


def closed_form(nb):
    return np.concatenate([[0], np.cumsum(round16(nb))]).astype(np.int64)


def check_image(rows, nb, dense, off, cap, fill=FILL, tag=""):
    """the contract: closed-form offsets; every segment that fits below cap equals its row and its padding is zero; from the
    first segment that does not fit (or the image's end) to the end of the guard region nothing was written"""
    S = len(nb)
    assert (nb >= 0).all(), tag
    assert off.tolist() == closed_form(nb).tolist(), tag + ": offsets"
    fits = int(np.searchsorted(off, cap, side="right")) - 1         # segments 0 .. fits - 1 end at or below cap
    want = np.zeros(int(off[fits]), dtype=np.uint8)
    for i in range(fits):
        want[off[i]:off[i] + nb[i]] = rows[i, :nb[i]]
    bad = np.nonzero(dense[:len(want)] != want)[0]
    assert bad.size == 0, "%s: image differs from the rows at byte %d (stream %d)" % (tag, bad[0], np.searchsorted(off, bad[0], side="right") - 1)
    assert (dense[len(want):] == fill).all(), tag + ": bytes written behind the last segment that fits"
    return fits


def emitted(nb, stats):
    """e[s][f]: the call's bytes of row s after input frame f, in unsigned arithmetic"""
    by = stats[:, :, 1].astype(np.int64)
    return (nb.astype(np.int64)[:, None] - ((by[:, -1:] - by) & 0xFFFFFFFF)) & 0xFFFFFFFF


def expected_crc(rows, nb, stats):
    """the host's CRC of every prefix rows[s][:e[s][f]] (e does not decrease with f: one chained pass per row)"""
    e = emitted(nb, stats)
    want = np.zeros(e.shape, np.uint16)
    for s in range(len(nb)):
        run, at = 0, 0
        assert (np.diff(e[s]) >= 0).all() and e[s, -1] == nb[s]
        for f in range(e.shape[1]):
            run = host_crc(rows[s, at:e[s, f]], run)
            at = int(e[s, f])
            want[s, f] = run
    return want, e


def check_call(want, f0, nf, bs, pk, pkb, stats, lsf, tag=""):
    """one call's outputs against the oracle's frames f0 .. f0 + nf of every stream (want[s]: [packet_cases.Frame])"""
    for s in range(len(want)):
        assert bs[s] == b"".join(w.bs for w in want[s][f0:f0 + nf]), "%s stream %d: bitstream" % (tag, s)
        for f in range(nf):
            w = want[s][f0 + f]
            at = "%s stream %d frame %d + %d" % (tag, s, f0, f)
            n0, n1 = w.sizes
            assert n0 > 0 and (n1 > 0) == bool(lsf), at         # (the expectation itself: one packet, or the MPEG-2 call's two)
            assert tuple(pkb[s, f]) == (n0, n1), at + ": packet sizes"
            assert pk[s, f, :n0 + n1].tobytes() == w.packet, at + ": packet"
            assert (pk[s, f, n0 + n1:] == FILL).all(), at + ": bytes written behind the packet"
            assert tuple(stats[s, f]) == (w.frames_out, w.bytes_out), at + ": frames / bytes emitted so far"


def same_outputs(a, b, counts, tag):
    """rows (their used part), byte counts, counters and CRCs of two calls' buffers are identical (the file ledger's twins)"""
    (rows, nb, st, cr), (trows, tnb, tst, tcr) = a, b
    assert nb.tolist() == tnb.tolist() and (st == tst).all() and (cr == tcr).all(), tag + ": byte counts / counters / CRCs differ from the twin batch's"
    for s in range(len(nb)):
        if counts[s]:
            assert rows[s, :nb[s]].tobytes() == trows[s, :nb[s]].tobytes(), "%s: row %d differs from the twin batch's" % (tag, s)


def check_idle_rows(bufs, counts):
    """a stream that takes no frame: byte count 0, and its row (prefilled with FILL) is not written"""
    o, n = bufs.rows()
    for s in range(len(n)):
        if counts[s] == 0:
            assert n[s] == 0 and (o[s] == FILL).all(), "stream %d took no frame and its row was written" % s


def check_crc(bufs):
    """d_crc[s][f] = CRC of the row's first e[f] bytes, e[f] from the call's own counters (the header's formula)"""
    o, n, st, crc = bufs.host()
    for s in range(len(n)):
        for f in range(bufs.nf):
            e = int(n[s]) - ((int(st[s, -1, 1]) - int(st[s, f, 1])) & 0xFFFFFFFF)
            assert 0 <= e <= n[s]
            assert crc[s, f] == host_crc(o[s, :e]), "stream %d frame %d: CRC" % (s, f)


def check_dense(bufs):
    o, n = bufs.rows()
    img, off = bufs.image.host()
    assert off[0] == 0 and (np.diff(off) == (n.astype(np.int64) + 15) // 16 * 16).all()
    for s in range(len(n)):
        assert img[off[s]:off[s] + n[s]].tobytes() == o[s, :n[s]].tobytes(), "stream %d: dense segment" % s
