"""The cases of tests/test_gpu_pack.py and tests/test_pack_cases.py: frames constructed for the bit packer (k_pack,
hmp3_amd/csrc/hx_pack.hip), as plain records made from seeds and rules, and what follows from the records and the oracle's
code tables alone - each segment's bit length, the frame's place in its slots, the sequence of put sizes the reference's
writer would see.  Nothing here is taken from an encoder run.

A segment:  {"fields": 40 entries in transmission order, None or (value, length) - a negative value is a field the
             first-generation allocator can leave (bit 15 of the record's field) -, "not_null", "pairs": (n0, n1, n2),
             "tables": (t0, t1, t2), "c1", "quads", "ix": 576 magnitudes, "sign": 576 sign bits}
A frame:    {"segs": its segments in wave order - MPEG-1 stereo: granule 0 left, right, granule 1 left, right; MPEG-1 mono:
             granule 0, 1; MPEG-2 stereo: left, right; MPEG-2 mono: one -, "mf": the capacity of the frame's own slot,
             "stuff": zero bytes behind the main data (bytes - raw_bytes), "packet": also goes to the packet buffer,
             "huff_bits_off": added to segment 0's huff_bits (the status test)}
A stream:   {"cls": a key of CLASSES, "frames", "pending": capacities of the slots pending from earlier calls,
             "main_bytes0": bytes in use in the first of them, "ghosts": frame positions behind the stream's count that
             carry a record all the same (it must not be packed)}
A list:     {"streams"}: what one hx_debug_pack call gets.
"""
import ctypes as C
import functools
import random

import numpy as np

from oracle import oracle as O

CLASSES = {     # name: control, MPEG-2 (one granule per frame), channels, side information bytes
    "m1s": dict(kw=dict(), lsf=0, nchan=2, side=32),
    "m1m": dict(kw=dict(mode=3), lsf=0, nchan=1, side=17),
    "m2s": dict(kw=dict(samprate=22050), lsf=1, nchan=2, side=17),
    "m2m": dict(kw=dict(samprate=22050, mode=3), lsf=1, nchan=1, side=9),
}
SLOTS_EXTRA = 40        # HX_SLOTS_EXTRA
SGN_WORDS = 20          # HX_SGN_WORDS
GRID_CAP = 8 * 256 * 8  # the largest grid the runtime launches k_pack with
LIST_NAMES = ("codewords", "widest_pair", "pair_counts", "quad_counts", "regions", "fields", "negative_fields", "length",
              "slots", "classes", "grid_stride")


def segs_per_frame(cls):
    c = CLASSES[cls]
    return c["nchan"] * (1 if c["lsf"] else 2)


# ---- the ctypes mirrors of hx_types.h (sizes: hx_debug_host_table "sizeof_pack_records") ----
class SegOut(C.Structure):
    _fields_ = [("start_bit", C.c_int), ("huff_bits", C.c_int), ("nreg01", C.c_uint), ("nreg2_quads", C.c_uint), ("tabs", C.c_uint),
                ("not_null", C.c_int), ("sf", C.c_ushort * 40), ("pad_", C.c_ubyte * 8)]


class Slot(C.Structure):
    _fields_ = [("off", C.c_int), ("mf", C.c_int)]


class FrameOut(C.Structure):
    _fields_ = [("bytes", C.c_int), ("raw_bytes", C.c_int), ("first_slot", C.c_int), ("main_bytes", C.c_int), ("packet_off", C.c_longlong),
                ("pad_", C.c_int * 2), ("near", Slot * 4)]


# ---- building segments ----
def mk_seg(fields=(), pairs=(), split=None, tables=(0, 0, 0), quads=(), c1=0, not_null=1, tail_signs=0):
    """pairs: (x, y, sign of x, sign of y); split: pairs per region (default: all in region 0); quads: ((v0, v1, v2, v3),
    (s0, s1, s2, s3)); tail_signs: the sign bit of every line behind the coded ones (the lines' signs come from the
    spectrum, whatever a line quantises to)"""
    split = (len(pairs), 0, 0) if split is None else tuple(split)
    assert sum(split) == len(pairs)
    ix = [0] * 576
    sign = [tail_signs] * 576
    for i, (x, y, sx, sy) in enumerate(pairs):
        ix[2 * i], ix[2 * i + 1], sign[2 * i], sign[2 * i + 1] = x, y, sx, sy
    for i, (v, s) in enumerate(quads):
        j = 2 * len(pairs) + 4 * i
        ix[j:j + 4], sign[j:j + 4] = v, s
    return {"fields": (list(fields) + [None] * 40)[:40], "not_null": not_null, "pairs": split, "tables": tuple(tables), "c1": c1,
            "quads": len(quads), "ix": ix, "sign": sign}


def pad_fields(nbits, first=()):
    """fields of 4 bits (and one shorter) that add nbits to `first`"""
    f = list(first)
    while nbits > 0:
        n = min(nbits, 4)
        f.append(((5 * len(f) + 3) % (1 << n), n))
        nbits -= n
    assert len(f) <= 40
    return f


def table_max(tabs, t):
    return 15 + (1 << tabs["linbits"][t]) - 1 if t >= 16 else tabs["dim"][t] - 1


def pair_bits(tabs, t, x, y):
    if tabs["dim"][t] == 0:
        return 0
    lin = tabs["linbits"][t]
    return tabs["len"][t, min(x, 15), min(y, 15)] + (lin if x >= 15 else 0) + (lin if y >= 15 else 0) + (x != 0) + (y != 0)


def region_tables(seg):
    n0, n1, n2 = seg["pairs"]
    return [seg["tables"][0]] * n0 + [seg["tables"][1]] * n1 + [seg["tables"][2]] * n2


def seg_puts(tabs, seg):
    """the sizes of the segment's puts in the reference writer's order, each with what it is: ("field", j), ("code", pair),
    ("lin", pair), ("sign", pair), ("quad", q), ("qsign", q)"""
    puts = [(n, ("field", j)) for j, f in enumerate(seg["fields"]) if f is not None for n in [f[1]]]
    if not seg["not_null"]:
        return puts
    ix = seg["ix"]
    for i, t in enumerate(region_tables(seg)):
        if tabs["dim"][t] == 0:
            continue
        x, y, lin = ix[2 * i], ix[2 * i + 1], tabs["linbits"][t]
        puts.append((tabs["len"][t, min(x, 15), min(y, 15)], ("code", i)))
        if x >= 15 and t >= 16:
            puts.append((lin, ("lin", i)))
        if x:
            puts.append((1, ("sign", i)))
        if y >= 15 and t >= 16:
            puts.append((lin, ("lin", i)))
        if y:
            puts.append((1, ("sign", i)))
    q0 = 2 * sum(seg["pairs"])
    for q in range(seg["quads"]):
        v = ix[q0 + 4 * q:q0 + 4 * q + 4]
        puts.append((4 if seg["c1"] else tabs["quada"][8 * v[0] + 4 * v[1] + 2 * v[2] + v[3]][1], ("quad", q)))
        puts += [(1, ("qsign", q))] * sum(v)
    return puts


_bits, _valid = {}, {}


def seg_bits(tabs, seg):
    """(kept per segment object: a list may use one segment in thousands of frames; a segment is not changed once made)"""
    k = id(seg)
    if k not in _bits or _bits[k][0] is not seg:
        _bits[k] = (seg, sum(n for n, _ in seg_puts(tabs, seg)))
    return _bits[k][1]


def field_bits(seg):
    return sum(f[1] for f in seg["fields"] if f is not None)


def frame_fills(tabs, segs):
    """the bits in the reference writer's 32-bit buffer in front of each negative field of the frame, after the flush that
    field's own size may cause: the fill unmasked_writer_fixup replays"""
    fills, P = [], 0
    for seg in segs:
        for n, (kind, j) in seg_puts(tabs, seg):
            if 32 - P < n:          # (l3pack.c, L3_outbits: whole bytes leave until 24 bits are free)
                while P > 8:
                    P -= 8
            if kind == "field" and seg["fields"][j][0] < 0:
                fills.append(P)
            P += n
    return fills


def long_pair_offsets(tabs, segs):
    """start offsets (mod 32) in the frame's main data of the pairs longer than 32 bits"""
    offs, pos = [], 0
    for seg in segs:
        p = pos + field_bits(seg)
        if seg["not_null"]:
            for i, t in enumerate(region_tables(seg)):
                n = pair_bits(tabs, t, seg["ix"][2 * i], seg["ix"][2 * i + 1])
                if n > 32:
                    offs.append(p % 32)
                p += n
        pos += seg_bits(tabs, seg)
    return offs


# ---- the validator: a case must be something the stream walk can emit ----
def validate_seg(tabs, seg):
    if _valid.get(id(seg)) is seg:
        return
    _valid[id(seg)] = seg
    n0, n1, n2 = seg["pairs"]
    npairs, nq, ix = n0 + n1 + n2, seg["quads"], seg["ix"]
    assert len(seg["fields"]) == 40 and len(ix) == 576 and len(seg["sign"]) == 576
    assert seg["not_null"] in (0, 1) and seg["c1"] in (0, 1) and all(s in (0, 1) for s in seg["sign"])
    for f in seg["fields"]:
        if f is not None:
            v, n = f
            assert 0 <= n <= 5 and (n, v) != (0, 0) and (0 <= v < (1 << n) if v >= 0 else v >= -128), f
    assert 2 * npairs + 4 * nq <= 576 and npairs <= 288
    for i, t in enumerate(region_tables(seg)):
        assert 0 <= t < 32 and t not in (4, 14), t
        x, y = ix[2 * i], ix[2 * i + 1]
        top = max(table_max(tabs, t), 0)        # (x, y < dim below table 16 - table 0: all-zero pairs -, the escape range from 16 on)
        assert 0 <= x <= top and 0 <= y <= top, (t, x, y)
    assert all(v in (0, 1) for v in ix[2 * npairs:2 * npairs + 4 * nq]), "quads hold 0 / 1 only"
    assert all(v == 0 for v in ix[2 * npairs + 4 * nq:]), "lines behind the coded ones are zero"
    assert seg_bits(tabs, seg) <= 4095


def stream_layout(tabs, stream, frame_bits=None):
    """where each frame's main data goes: the stream's slots [(off, mf)], the row bytes they take, and per frame
    {"first_slot", "main_bytes", "raw", "bytes", "runs": [(row offset, count)], "span": slots from first_slot to the last one
    written}.  The walk's rule: a frame gets a slot of its own behind the pending ones, its main data goes on where the frame
    before ended and never beyond its own slot; full slots retire."""
    hdr = 4 + CLASSES[stream["cls"]]["side"]
    pending = list(stream.get("pending", ()))
    caps = pending + [fr["mf"] for fr in stream["frames"]]
    offs, o = [], 0
    for c in caps:
        offs.append(o)
        o += hdr + c
    p0, mb, recs = 0, stream.get("main_bytes0", 0), []
    assert mb == 0 or mb < caps[0]
    for i, fr in enumerate(stream["frames"]):
        own = len(pending) + i
        bits = sum(seg_bits(tabs, s) for s in fr["segs"]) if frame_bits is None else frame_bits[i]
        raw = (bits + 7) // 8
        nbytes = raw + fr.get("stuff", 0)
        assert p0 <= own and sum(caps[p0:own + 1]) - mb >= nbytes, "slot capacities sum to at least the frame's bytes"
        rec = {"first_slot": p0, "main_bytes": mb, "raw": raw, "bytes": nbytes, "runs": [], "span": 1 if nbytes else 0}
        q, k, left = mb, p0, nbytes
        while left > 0:
            if q >= caps[k]:
                q -= caps[k]
                k += 1
                continue
            take = min(left, caps[k] - q)
            rec["runs"].append((offs[k] + hdr + q, take))
            rec["span"] = k - p0 + 1
            left -= take
            q += take
        mb += nbytes
        while p0 <= own and mb >= caps[p0]:
            mb -= caps[p0]
            p0 += 1
        recs.append(rec)
    return list(zip(offs, caps)), o, recs


def list_shape(lst):
    """(F, NG, frame stride, per-stream counts or None) of a list's call: F is the largest count, an MPEG-2 stream's frames
    come two to a count, and with an MPEG-2 class in play every stream has NG frame positions, else F"""
    any_lsf = any(CLASSES[s["cls"]]["lsf"] for s in lst["streams"])
    per = [(2 if CLASSES[s["cls"]]["lsf"] else 1) for s in lst["streams"]]
    assert all(len(s["frames"]) % p == 0 for s, p in zip(lst["streams"], per))
    counts = [len(s["frames"]) // p for s, p in zip(lst["streams"], per)]
    F = max(counts)
    fps = 2 * F if any_lsf else F
    assert all(len(s["frames"]) + s.get("ghosts", 0) <= fps for s in lst["streams"])
    return F, 2 * F, fps, (None if all(c == F for c in counts) else counts)


def validate(tabs, lst):
    F, NG, fps, counts = list_shape(lst)
    for st in lst["streams"]:
        assert len(st.get("pending", ())) <= SLOTS_EXTRA
        for fr in st["frames"]:
            assert len(fr["segs"]) == segs_per_frame(st["cls"])
            for seg in fr["segs"]:
                validate_seg(tabs, seg)
            assert sum(seg_bits(tabs, s) for s in fr["segs"]) <= 640 * 32
        slots, used, recs = stream_layout(tabs, st)
        assert len(slots) <= fps + SLOTS_EXTRA
        for rec in recs:
            assert all(0 <= a and a + n <= used for a, n in rec["runs"]), "offsets lie inside the row"


# ---- what hx_debug_pack takes, and what it must leave ----
def _frame_key(fr):
    return id(fr["segs"])


_WEIGHTS = (1 << np.arange(32, dtype=np.uint64)).astype(np.uint32)
_records = {}


def seg_record(seg):
    """the segment as (HxSegOut without its position and bit count, lines as int16, sign words); kept per segment object"""
    k = id(seg)
    if k not in _records or _records[k][0] is not seg:
        so = SegOut()
        so.nreg01, so.nreg2_quads = seg["pairs"][0] | seg["pairs"][1] << 16, seg["pairs"][2] | seg["quads"] << 16
        so.tabs = seg["tables"][0] | seg["tables"][1] << 8 | seg["tables"][2] << 16 | seg["c1"] << 24
        so.not_null = seg["not_null"]
        for j, fl in enumerate(seg["fields"]):
            so.sf[j] = 0 if fl is None else (fl[1] << 8) | (fl[0] & 255) | (0x8000 if fl[0] < 0 else 0)
        _records[k] = (seg, so, np.asarray(seg["ix"], np.int16), np.asarray(seg["sign"], np.uint32).reshape(18, 32) @ _WEIGHTS)
    return _records[k][1:]


def build(tabs, lst):
    """the arrays of one hx_debug_pack call and the rows / packet buffer it must leave: a dict of numpy / ctypes arrays -
    cls, nfr (or None), seg, ixq, sgn, frm, slots, rows, packet (pre-filled with 0xA5), want_rows, want_packet - and S, NG,
    fps, out_stride, classes (the names, in class order).  The main data comes from the oracle's writer (hxo_pack_frame).
    A ghost record is a copy of the stream's first frame with a slot of its own behind the stream's real ones."""
    F, NG, fps, counts = list_shape(lst)
    S = len(lst["streams"])
    classes = sorted({st["cls"] for st in lst["streams"]})
    seg = (SegOut * (S * NG * 2))()
    ixq = np.zeros((S, NG, 2, 576), np.int16)
    sgn = np.zeros((S, NG, 2, SGN_WORDS), np.uint32)
    frm = (FrameOut * (S * fps))()
    slots = (Slot * (S * (fps + SLOTS_EXTRA)))()
    packed, lays, stride, npacket = {}, [], 0, 0
    for st in lst["streams"]:
        datas = []
        for fr in st["frames"]:
            k = _frame_key(fr)
            if k not in packed:
                packed[k] = O.pack_frame(fr["segs"])
            datas.append(packed[k])
        ghosts = st.get("ghosts", 0) if st["frames"] else 0
        frames = st["frames"] + ([dict(st["frames"][0], stuff=0, packet=False)] * ghosts if ghosts else [])
        datas = datas + datas[:1] * ghosts
        lay = stream_layout(tabs, dict(st, frames=frames), [sum(d[1]) for d in datas])
        lays.append((lay, frames, datas))
        stride = max(stride, lay[1])
        npacket += sum(len(d[0]) + 24 for fr, d in zip(frames, datas) if fr.get("packet"))
    stride = (stride + 64 + 15) // 16 * 16
    rows = np.full((S, stride), 0xA5, np.uint8)
    packet = np.full(npacket + 40, 0xA5, np.uint8)
    want_rows, want_packet = rows.copy(), packet.copy()
    pk = 8
    for s, (st, (lay, frames, datas)) in enumerate(zip(lst["streams"], lays)):
        c = CLASSES[st["cls"]]
        for j, (off, mf) in enumerate(lay[0]):
            slots[s * (fps + SLOTS_EXTRA) + j].off, slots[s * (fps + SLOTS_EXTRA) + j].mf = off, mf
        for f, (rec, fr, (data, bits)) in enumerate(zip(lay[2], frames, datas)):
            fo = frm[s * fps + f]
            fo.bytes, fo.raw_bytes, fo.first_slot, fo.main_bytes, fo.packet_off = rec["bytes"], rec["raw"], rec["first_slot"], rec["main_bytes"], -1
            if f < len(st["frames"]):
                body = np.frombuffer(data + bytes(rec["bytes"] - rec["raw"]), np.uint8)
                at = 0
                for a, n in rec["runs"]:
                    want_rows[s, a:a + n] = body[at:at + n]
                    at += n
                if fr.get("packet"):
                    fo.packet_off = pk
                    want_packet[pk:pk + len(data)] = np.frombuffer(data, np.uint8)
                    pk += len(data) + 24
            start = 0
            for w, sg in enumerate(fr["segs"]):
                g, ch = (f, w) if c["lsf"] else (2 * f + w // c["nchan"], w % c["nchan"])
                if g < NG:      # (an MPEG-1 stream's positions behind the first half of its row have no granules)
                    so, ix, words = seg_record(sg)
                    i = (s * NG + g) * 2 + ch
                    seg[i] = so
                    seg[i].start_bit, seg[i].huff_bits = start, bits[w] - field_bits(sg) + (fr.get("huff_bits_off", 0) if w == 0 else 0)
                    ixq[s, g, ch] = ix
                    sgn[s, g, ch, :18] = words
                start += bits[w]
    cls = np.array([classes.index(st["cls"]) for st in lst["streams"]], np.int32)
    return dict(S=S, NG=NG, fps=fps, out_stride=stride, classes=classes, cls=cls, nfr=None if counts is None else np.array(counts, np.int32),
                seg=seg, ixq=ixq, sgn=sgn, frm=frm, slots=slots, rows=rows, packet=packet, want_rows=want_rows, want_packet=want_packet)


# ---- the lists ----
def _signs(i):
    return (i & 1, (i >> 1) & 1)        # all four combinations over four pair positions


def _all_pairs(tabs, t, rng, xs=range(16)):
    """every (x, y) of table t with x in xs; at 15 from table 16 on the escape values 15, 16, the table's maximum and random
    ones in turn"""
    dim, top, pairs, e = tabs["dim"][t], table_max(tabs, t), [], 0
    for x in xs:
        if x >= dim:
            break
        for y in range(dim):
            v = []
            for c in (x, y):
                if t >= 16 and c == 15:
                    c = (15, 16, top, rng.randint(15, top))[e % 4]
                    e += 1
                v.append(c)
            pairs.append((v[0], v[1]) + _signs(len(pairs)))
    return pairs


def _in_region(pairs, r, t):
    """all pairs in region r on table t, the other two regions empty"""
    split = [0, 0, 0]
    split[r] = len(pairs)
    tables = [t if k == r else (1, 5, 24)[k] for k in range(3)]      # (an empty region's table is not looked at)
    return dict(pairs=pairs, split=split, tables=tables)


def _frames(cls, segs, mf=None, **kw):
    """segments dealt to frames of class cls (the last one filled up with empty segments), each in a slot of its own"""
    n = segs_per_frame(cls)
    segs = list(segs) + [mk_seg(not_null=0)] * (-len(segs) % n)
    return [dict(segs=segs[i:i + n], mf=mf if mf is not None else 4 * 512 + 8, **kw) for i in range(0, len(segs), n)]


def _even(cls, frames):
    """an MPEG-2 stream's frames come in twos (a 1152-sample block is two frames)"""
    if CLASSES[cls]["lsf"] and len(frames) % 2:
        frames = frames + [dict(segs=[mk_seg(not_null=0)] * segs_per_frame(cls), mf=16)]
    return frames


def _stream(cls, frames, **kw):
    return dict(cls=cls, frames=_even(cls, frames), **kw)


def _random_pairs(tabs, rng, t, n, big=False):
    top = max(table_max(tabs, t), 0)
    return [((rng.randint(0, top) if big or rng.random() < 0.5 else rng.randint(0, min(top, 3))),
             rng.randint(0, top) if big else rng.randint(0, min(top, 2)), rng.randint(0, 1), rng.randint(0, 1)) for _ in range(n)]


def _random_quads(rng, n, first=0):
    """n quads whose patterns run through all 16; signs random, on the zero lines too"""
    return [(tuple(((first + q) % 16 >> (3 - k)) & 1 for k in range(4)), tuple(rng.randint(0, 1) for _ in range(4))) for q in range(n)]


def _seg_of_bits(tabs, rng, target, t=23):
    """a segment of exactly `target` bits: pairs of an escape table with large values, then fields for the rest"""
    pairs, bits = [], 0
    while True:
        p = _random_pairs(tabs, rng, t, 1, big=True)[0]
        n = pair_bits(tabs, t, p[0], p[1])
        if bits + n > target - 8 or len(pairs) == 288:
            break
        pairs.append(p)
        bits += n
    assert target - bits <= 160
    return mk_seg(fields=pad_fields(target - bits), pairs=pairs, tables=(t, t, t), split=(len(pairs) // 3, len(pairs) // 3, len(pairs) - 2 * (len(pairs) // 3)))


def _codewords(tabs):
    rng, segs, k = random.Random(101), [], 0
    for t in range(1, 32):
        if t in (4, 14):
            continue
        for xs in ((range(16),) if t < 16 and t != 13 and t != 15 else (range(0, 8), range(8, 16))):
            pairs = _all_pairs(tabs, t, rng, xs)
            if tabs["dim"][t] <= 4:     # (few pairs of two non-zero values: the table four times over, the signs moved on by one each time)
                pairs = [p[:2] + _signs(i + r) for r in range(4) for i, p in enumerate(pairs)]
            segs.append(mk_seg(**_in_region(pairs, k % 3, t), tail_signs=k & 1))
            k += 1
    return dict(streams=[_stream("m1s", _frames("m1s", segs))])


def _widest_pair(tabs):
    # the longest code word among the (15, 15) entries of the two tables with 13 linbits, both escapes at the maximum
    t = max((23, 31), key=lambda t: tabs["len"][t, 15, 15])
    top, frames, pos = table_max(tabs, t), [], 0
    for o in range(32):
        if o % 4 == 0:
            frames.append(dict(segs=[], mf=512))
            pos = 0
        sg = mk_seg(fields=pad_fields((o - pos) % 32), pairs=[(top, top, 1, 1)], tables=(t, 0, 0))
        pos += seg_bits(tabs, sg)
        frames[-1]["segs"].append(sg)
    return dict(streams=[_stream("m1s", frames)])


def _pair_counts(tabs):
    rng, segs = random.Random(202), []
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 192, 256, 287, 288):
        a = rng.randint(0, n)
        b = rng.randint(0, n - a)
        t3 = [rng.choice((1, 2, 3, 5, 6, 7, 8, 9)) for _ in range(3)]
        pairs = sum((_random_pairs(tabs, rng, t, c) for t, c in zip(t3, (a, b, n - a - b))), [])
        segs.append(mk_seg(fields=pad_fields(rng.randint(0, 9)), pairs=pairs, split=(a, b, n - a - b), tables=t3,
                           quads=_random_quads(rng, min(3, (576 - 2 * n) // 4)), c1=n & 1, tail_signs=1))
    return dict(streams=[_stream("m1s", _frames("m1s", segs))])


def _quad_counts(tabs):
    rng, segs = random.Random(303), []
    for nq in (0, 1, 63, 64, 65, 128, 143, 144):
        for npairs in (0, 1, 15):       # (an odd pair count: a quad's sign bits straddle two words where 2 * pairs + 4 * q is 30 mod 32)
            if 2 * npairs + 4 * nq > 576:
                continue
            for c1 in (0, 1):
                segs.append(mk_seg(pairs=_random_pairs(tabs, rng, 7, npairs), tables=(7, 0, 0), quads=_random_quads(rng, nq, first=len(segs)),
                                   c1=c1, tail_signs=1))
    return dict(streams=[_stream("m1s", _frames("m1s", segs[:len(segs) // 2])), _stream("m2s", _frames("m2s", segs[len(segs) // 2:]))])


def _regions(tabs):
    rng, segs = random.Random(404), []
    P = lambda t, n: _random_pairs(tabs, rng, t, n)
    for split, t3 in (((0, 9, 7), (0, 7, 24)), ((9, 0, 7), (5, 13, 24)), ((9, 7, 0), (5, 24, 31)), ((0, 0, 11), (1, 1, 15)), ((11, 0, 0), (16, 0, 0)),
                      ((0, 11, 0), (0, 10, 0)), ((8, 6, 10), (5, 0, 24)), ((6, 70, 6), (2, 0, 3)), ((5, 6, 7), (12, 12, 12)), ((70, 70, 70), (9, 9, 9))):
        pairs = sum((P(t, n) if n else [] for t, n in zip(t3, split)), [])
        segs.append(mk_seg(pairs=pairs, split=split, tables=t3,quads=_random_quads(rng, 5), tail_signs=1))
    return dict(streams=[_stream("m1s", _frames("m1s", segs))])


def _fields(tabs):
    rng = random.Random(505)
    some = _random_pairs(tabs, rng, 8, 20)

    def full(maxlen, gaps=()):
        return [None if j in gaps else (lambda n: (rng.randrange(1 << n), n))(1 + (j + rng.randint(0, 1)) % maxlen) for j in range(40)]
    m1 = [mk_seg(fields=full(4), pairs=some, tables=(8, 0, 0)), mk_seg(fields=full(4, gaps=(0, 7, 8, 21, 39)), pairs=some, tables=(8, 0, 0)),
          mk_seg(fields=full(4, gaps=range(1, 40, 2)), not_null=0), mk_seg(pairs=some, tables=(8, 0, 0)),
          mk_seg(fields=[(0, 1), (0, 4), None, (15, 4), (1, 1)], not_null=0), mk_seg(fields=[None] * 39 + [(5, 3)], pairs=some, tables=(8, 0, 0)),
          mk_seg(not_null=0), mk_seg(fields=full(3), quads=_random_quads(rng, 4))]
    m2 = [mk_seg(fields=full(5), pairs=some, tables=(8, 0, 0)), mk_seg(fields=full(5, gaps=(3, 4, 5, 30)), not_null=0),
          mk_seg(fields=[(31, 5)] * 40, pairs=some, tables=(8, 0, 0)), mk_seg(pairs=some, tables=(8, 0, 0))]
    return dict(streams=[_stream("m1s", _frames("m1s", m1)), _stream("m2s", _frames("m2s", m2)), _stream("m2m", _frames("m2m", m2))])


NEGATIVE = (-1, -2, -3, -4, -17, -43, -86, -128)


def _negative_fields(tabs):
    rng = random.Random(606)
    neg = lambda n: (rng.choice(NEGATIVE), n)
    some = lambda n, t=10: dict(pairs=_random_pairs(tabs, rng, t, n), tables=(t, 0, 0))
    # MPEG-2 mono, one segment per frame: fields of k bits in all, then a negative field of no length - the buffer holds k bits
    # in front of it, k = 0 (the frame's first put) .. 32 -, then one with a length, then Huffman data over the stray bits' place
    m2m = [mk_seg(fields=pad_fields(k) + [neg(0), neg(1 + k % 4)], **some(6)) for k in range(33)]
    # a negative field whose own size does not fit: directly after a flush
    m2m += [mk_seg(fields=pad_fields(k) + [neg(32 - k + 1 + j) if 32 - k + 1 + j <= 5 else neg(5)], **some(4)) for k in (28, 29, 30, 31, 32) for j in (0, 1)]
    # MPEG-1 stereo: one in each of the four segments in turn behind Huffman data of other segments, two in one frame, one in
    # every segment, fields behind escapes and quads
    quiet = lambda: mk_seg(fields=pad_fields(rng.randint(0, 30)), quads=_random_quads(rng, rng.randint(0, 9)), c1=rng.randint(0, 1), **some(rng.randint(0, 40), rng.choice((10, 13, 24))))
    loud = lambda extra=0: mk_seg(fields=pad_fields(rng.randint(0, 11)) + [neg(rng.randint(0, 4)) for _ in range(1 + extra)] + pad_fields(rng.randint(0, 7))[:3],
                                  quads=_random_quads(rng, rng.randint(0, 9)), **some(rng.randint(0, 40), rng.choice((7, 15, 16, 29))))
    m1s = []
    for w in range(4):
        m1s.append(dict(segs=[loud() if k == w else quiet() for k in range(4)], mf=2048))
    m1s.append(dict(segs=[loud(), quiet(), quiet(), loud()], mf=2048))
    m1s.append(dict(segs=[loud(2), loud(), loud(1), loud()], mf=2048))
    m1s.append(dict(segs=[mk_seg(fields=[neg(3)], not_null=0), quiet(), mk_seg(fields=[neg(0)], **some(3)), quiet()], mf=2048))
    m1m = [dict(segs=[quiet(), loud()], mf=1024), dict(segs=[loud(), loud(3)], mf=1024)]
    return dict(streams=[_stream("m2m", _frames("m2m", m2m, mf=64)), _stream("m1s", m1s), _stream("m1m", m1m)])


def _length(tabs):
    rng = random.Random(707)
    # the largest raw main data of an MPEG-1 frame: 320 kbit/s at 32 kHz is 1440 bytes, less 36 of header and side
    # information, plus the 511 bytes main_data_begin can reach back
    most = 8 * (1440 - 36 + 511)
    big = [_seg_of_bits(tabs, rng, most // 4, t) for t in (23, 31, 22, 30)]
    frames = [dict(segs=[_seg_of_bits(tabs, rng, 4095), mk_seg(not_null=0), _seg_of_bits(tabs, rng, 4095, 31), mk_seg(fields=[(1, 1)], not_null=0)], mf=1100),
              dict(segs=big, mf=2000)]
    return dict(streams=[_stream("m1s", frames)])


def _slots(tabs):
    rng = random.Random(808)

    def fr(nbits, cls="m1s", **kw):
        n = segs_per_frame(cls)
        return dict(segs=[_seg_of_bits(tabs, rng, nbits // n, rng.choice((16, 20, 24, 27))) for _ in range(n)], **kw)
    return dict(streams=[
        # each frame in its own slot: bytes == raw_bytes, and stuffing up to the slot's size
        _stream("m1s", [fr(800, mf=100), fr(803, mf=140, stuff=39), fr(400, mf=50, packet=True), fr(408, mf=51)]),
        # main_bytes > 0 in the first slot; two slots; four
        _stream("m1s", [fr(1200, mf=200), fr(800, mf=40, stuff=1), fr(808, mf=150, packet=True)], pending=(60,), main_bytes0=17),
        _stream("m1m", [fr(1000, "m1m", mf=300), fr(1960, "m1m", mf=12)], pending=(31, 29, 33), main_bytes0=30),
        # five slots: the walk beyond the four near ones; a zero-capacity slot before the fourth and behind it; twelve slots
        _stream("m1s", [fr(1000, mf=90), fr(704, mf=160, stuff=5)], pending=(40, 11, 13, 17)),
        _stream("m2s", [fr(1500, "m2s", mf=100), fr(96, "m2s", mf=30)], pending=(20, 9, 0, 14, 12, 0, 0, 15, 30, 7, 21), main_bytes0=3),
        _stream("m1s", [fr(1500, mf=100, packet=True)], pending=(20, 0, 0, 0, 0, 0, 14, 12, 1, 15, 30, 7, 21), main_bytes0=19),
    ])


def _classes(tabs):
    rng = random.Random(909)

    def fr(cls, **kw):
        return dict(segs=[mk_seg(fields=pad_fields(rng.randint(0, 20)), quads=_random_quads(rng, rng.randint(0, 20)), c1=rng.randint(0, 1), tail_signs=1,
                                 pairs=_random_pairs(tabs, rng, 11, rng.randint(0, 60)), tables=(11, 0, 0)) for _ in range(segs_per_frame(cls))], mf=rng.randint(700, 720), **kw)
    # a call of F = 3 with an MPEG-2 class in play: the frame stride is NG = 6; the MPEG-1 streams use the first three positions
    # of their rows, the counts cut one stream of each version short, and every position left over carries a record
    return dict(streams=[
        _stream("m1s", [fr("m1s") for _ in range(3)], ghosts=3),
        _stream("m2s", [fr("m2s") for _ in range(6)]),
        _stream("m1m", [fr("m1m", packet=True) for _ in range(2)], ghosts=4, pending=(45,), main_bytes0=5),
        _stream("m2m", [fr("m2m") for _ in range(4)], ghosts=2),
        _stream("m2s", [fr("m2s") for _ in range(2)], ghosts=4),
        _stream("m1s", [], ghosts=0),
    ])


def _grid_stride(tabs):
    rng = random.Random(1010)
    kinds = [[mk_seg(fields=pad_fields(rng.randint(0, 9)), pairs=_random_pairs(tabs, rng, t, rng.randint(1, 4)), tables=(t, 0, 0),
                     quads=_random_quads(rng, k % 3, first=k), c1=k & 1)] for k, t in enumerate((1, 7, 13, 16, 24, 5, 10))]
    assert all(seg_bits(tabs, k[0]) <= 8 * 24 for k in kinds)
    n = GRID_CAP + 616          # more frame positions than the launch has workgroups
    return dict(streams=[dict(cls="m2m", frames=[dict(segs=kinds[i % 7], mf=24 + i % 3) for i in range(n)])])


def _status(tabs):
    """a correct frame, the same with segment 0's huff_bits off by one, and the correct one again"""
    lst = _pair_counts(tabs)
    fr = lst["streams"][0]["frames"][1]
    return dict(streams=[_stream("m1s", [fr, dict(fr, huff_bits_off=1), fr])])


_MAKERS = dict(codewords=_codewords, widest_pair=_widest_pair, pair_counts=_pair_counts, quad_counts=_quad_counts, regions=_regions, fields=_fields,
               negative_fields=_negative_fields, length=_length, slots=_slots, classes=_classes, grid_stride=_grid_stride, status=_status)


@functools.lru_cache(maxsize=None)
def tables():
    return O.huff_tables()


@functools.lru_cache(maxsize=None)
def case_list(name):
    return _MAKERS[name](tables())


def debug_pack(b, device=0):
    """hx_debug_pack on what build() made: (return value, status word); b["rows"] and b["packet"] are written in place"""
    from hmp3_amd import api
    ecs = (api.EControl * len(b["classes"]))(*[api.default_control(**CLASSES[c]["kw"]) for c in b["classes"]])
    status = C.c_int(-1)
    rc = api.lib().hx_debug_pack(device, ecs, len(b["classes"]), b["cls"].ctypes.data, b["S"], b["NG"], b["fps"],
                                 None if b["nfr"] is None else b["nfr"].ctypes.data, b["seg"], b["ixq"].ctypes.data, b["sgn"].ctypes.data,
                                 b["frm"], b["slots"], b["rows"].ctypes.data, b["out_stride"], b["packet"].ctypes.data, b["packet"].nbytes,
                                 C.byref(status))
    return rc, status.value
