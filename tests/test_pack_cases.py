"""The constructed frames of tests/pack_cases.py on the CPU: every case is something the stream walk can emit; the oracle's
writer (hxo_pack_frame) equals the reference's own (ref_pack_frame: L3_outbits / L3_pack_huff) on every one of them; the
oracle's pair lengths and the library's host code tables reproduce the reference's writer entry by entry; and the cases
reach what tests/test_gpu_pack.py is there for - conditions computed from the cases and the oracle's tables alone, so that
an edit of the cases cannot thin them unnoticed.  hx_debug_pack's refusals need no GPU either: they come before any launch."""
import ctypes as C

import numpy as np
import pytest

import pack_cases as P
from oracle import oracle as O
from hmp3_amd import api

ALL_LISTS = P.LIST_NAMES + ("status",)


def need_ref():
    if O.ref() is None:
        pytest.skip("oracle/_ref not built")


def host_table(name, dtype, n, **kw):
    a = np.zeros(n, dtype)
    assert api.lib().hx_debug_host_table(C.byref(api.default_control(**kw)), name.encode(), a.ctypes.data, a.nbytes) == a.nbytes, name
    return a


def all_frames(names=ALL_LISTS):
    for name in names:
        for st in P.case_list(name)["streams"]:
            for fr in st["frames"]:
                yield name, st, fr


def test_the_mirrors_have_the_librarys_sizes_and_the_classes_its_parameters():
    v = host_table("sizeof_pack_records", np.int32, 5)
    assert [int(x) for x in v] == [C.sizeof(P.SegOut), C.sizeof(P.FrameOut), C.sizeof(P.Slot), P.SLOTS_EXTRA, P.SGN_WORDS]
    for name, c in P.CLASSES.items():
        got = [int(host_table(n, np.int32, 1, **c["kw"])[0]) for n in ("side_bytes", "nchan", "h_id")]
        assert got == [c["side"], c["nchan"], 0 if c["lsf"] else 1], name


@pytest.mark.parametrize("name", ALL_LISTS)
def test_every_case_is_something_the_stream_walk_can_emit(name):
    P.validate(P.tables(), P.case_list(name))


@pytest.mark.parametrize("name", ALL_LISTS)
def test_oracle_writer_equals_reference_writer(name):
    need_ref()
    tabs, seen = P.tables(), set()
    for st in P.case_list(name)["streams"]:
        for fr in st["frames"]:
            if id(fr["segs"]) in seen:
                continue
            seen.add(id(fr["segs"]))
            got, want = O.pack_frame(fr["segs"]), O.pack_frame(fr["segs"], use_ref=True)
            assert got[1] == want[1] == [P.seg_bits(tabs, s) for s in fr["segs"]]
            assert got[0] == want[0]
            assert len(got[0]) == (sum(got[1]) + 7) // 8


def test_the_harness_and_the_direct_calls_are_one_reference_writer():
    """a reference build from before ref_pack_frame is driven through its exported writer functions (oracle.py): both ways
    give the same bytes and lengths"""
    need_ref()
    if not O.ref_has_pack_frame():
        pytest.skip("oracle/_ref was built before the harness had ref_pack_frame: only the direct calls exist")
    for _, _, fr in all_frames(("negative_fields", "codewords", "quad_counts", "length")):
        assert O.pack_frame(fr["segs"], use_ref=True, harness=True) == O.pack_frame(fr["segs"], use_ref=True, harness=False)


def legal_pairs(tabs):
    """every (t, x, y) clamped to 15, and from table 16 on the escape extremes"""
    for t in O.HUFF_TABLES:
        if t == 0:
            continue
        for x in range(tabs["dim"][t]):
            for y in range(tabs["dim"][t]):
                yield t, x, y
        if t >= 16:
            top = P.table_max(tabs, t)
            for x, y in ((top, top), (top, 0), (0, top), (16, top), (top, 15), (15, 14), (14, 16)):
                yield t, x, y


def test_oracle_pair_lengths_equal_what_the_reference_writer_produces():
    need_ref()
    tabs = P.tables()
    for t, x, y in legal_pairs(tabs):
        for sx, sy in ((0, 0), (1, 1)):
            data, bits = O.pack_frame([P.mk_seg(pairs=[(x, y, sx, sy)], tables=(t, 0, 0))], use_ref=True)
            assert bits == [O.huff_pair_len(t, x, y)] == [P.pair_bits(tabs, t, x, y)], (t, x, y)


def as_bytes(value, nbits):
    return (value << (-nbits % 8)).to_bytes((nbits + 7) // 8, "big")


def test_host_code_tables_reproduce_the_reference_writer_on_every_pair_and_quad():
    """the tables k_pack stages (HxGlobalTabs), addressed the way it addresses them"""
    need_ref()
    code, hlen = host_table("huff_code", np.uint16, 1408), host_table("huff_len", np.uint8, 1408)
    off, dim, lin = host_table("huff_off", np.uint16, 32), host_table("huff_dim", np.uint8, 32), host_table("huff_lin", np.uint8, 32)
    qcode, qlen = host_table("quada_code", np.uint8, 16), host_table("quada_len", np.uint8, 16)
    for t, x, y in legal_pairs(P.tables()):
        d, l = (16, int(lin[t])) if t >= 16 else (int(dim[t]), 0)
        o = int(off[t]) + min(x, 15) * d + min(y, 15)
        for sx, sy in ((0, 1), (1, 0)):
            v, n = int(code[o]), int(hlen[o])
            if x >= 15 and l:
                v, n = (v << l) | (x - 15), n + l
            if x:
                v, n = (v << 1) | sx, n + 1
            if y >= 15 and l:
                v, n = (v << l) | (y - 15), n + l
            if y:
                v, n = (v << 1) | sy, n + 1
            want = O.pack_frame([P.mk_seg(pairs=[(x, y, sx, sy)], tables=(t, 0, 0))], use_ref=True)
            assert (as_bytes(v, n), [n]) == want, (t, x, y)
    for c1 in (0, 1):
        for pat in range(16):
            q = tuple((pat >> (3 - k)) & 1 for k in range(4))
            for s in ((0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 1, 1)):
                v, n = (pat ^ 15, 4) if c1 else (int(qcode[pat]), int(qlen[pat]))
                for k in range(4):
                    if q[k]:
                        v, n = (v << 1) | s[k], n + 1
                want = O.pack_frame([P.mk_seg(quads=[(q, s)], c1=c1)], use_ref=True)
                assert (as_bytes(v, n), [n]) == want, (c1, pat)


# ---- the coverage conditions ----
def test_every_code_word_of_every_table_is_emitted():
    tabs, seen = P.tables(), set()
    for _, _, fr in all_frames():
        for seg in fr["segs"]:
            if seg["not_null"]:
                for i, t in enumerate(P.region_tables(seg)):
                    seen.add((t, min(seg["ix"][2 * i], 15), min(seg["ix"][2 * i + 1], 15)))
    missing = [k for k in tabs["len"] if k[0] in O.HUFF_TABLES and k not in seen]
    assert not missing, missing[:20]
    # the escape values at 15: the smallest two, the table's largest and others, in both positions
    for t in range(16, 32):
        top = P.table_max(tabs, t)
        for pos in (0, 1):
            vals = {seg["ix"][2 * i + pos] for _, _, fr in all_frames(("codewords",)) for seg in fr["segs"]
                    for i, tt in enumerate(P.region_tables(seg)) if tt == t and seg["ix"][2 * i + pos] >= 15}
            assert {15, 16, top} <= vals and (len(vals) > 3 or top < 30), (t, pos, sorted(vals))
    # signs: all four combinations of a pair of two non-zero values, per table
    for t in O.HUFF_TABLES[1:]:
        combos = {(seg["sign"][2 * i], seg["sign"][2 * i + 1]) for _, _, fr in all_frames(("codewords",)) for seg in fr["segs"]
                  for i, tt in enumerate(P.region_tables(seg)) if tt == t and seg["ix"][2 * i] and seg["ix"][2 * i + 1]}
        assert len(combos) == 4, (t, combos)
    # each table is met in region 0, 1 and 2 somewhere
    regions = {r for _, _, fr in all_frames(("codewords",)) for seg in fr["segs"] for r in range(3) if seg["pairs"][r]}
    assert regions == {0, 1, 2}


def test_every_quad_pattern_is_emitted_under_both_count1_tables_and_a_sign_word_is_straddled():
    seen, straddle = set(), set()
    for _, _, fr in all_frames():
        for seg in fr["segs"]:
            q0 = 2 * sum(seg["pairs"])
            for q in range(seg["quads"] if seg["not_null"] else 0):
                v = seg["ix"][q0 + 4 * q:q0 + 4 * q + 4]
                seen.add((seg["c1"], tuple(v)))
                if (q0 + 4 * q) % 32 == 30 and any(v) and len(set(seg["sign"][q0 + 4 * q:q0 + 4 * q + 4])) == 2:
                    straddle.add((seg["c1"], tuple(v[:2]) != (0, 0), tuple(v[2:]) != (0, 0)))
    assert len(seen) == 32
    assert {(0, True, True), (1, True, True)} <= straddle      # coded values on both sides of the word boundary, signs that differ


def test_pair_and_quad_counts_at_the_lane_structures_edges():
    pairs = {sum(seg["pairs"]) for _, _, fr in all_frames(("pair_counts",)) for seg in fr["segs"] if seg["not_null"]}
    assert {0, 1, 63, 64, 65, 127, 128, 129, 192, 256, 287, 288} <= pairs
    quads = {(seg["quads"], sum(seg["pairs"]) % 2) for _, _, fr in all_frames(("quad_counts",)) for seg in fr["segs"] if seg["not_null"]}
    assert {(n, 0) for n in (0, 1, 63, 64, 65, 128, 143, 144)} | {(n, 1) for n in (0, 1, 63, 64, 65, 128, 143)} <= quads


def test_a_long_pair_starts_at_every_bit_offset():
    tabs = P.tables()
    offs = {o for _, _, fr in all_frames(("widest_pair",)) for o in P.long_pair_offsets(tabs, fr["segs"])}
    assert offs == set(range(32))
    # The format has one pair longer than 32 bits: table 23's (15, 15) with both escapes, 36 bits.  The part of it that
    # put_bits64 writes first, its top 36 - 32 bits, lies inside the 8-bit code word 00000011 and is zero whatever the values
    # and signs are: no record the stream walk can emit tells a wrong high part from a right one, only a wrong low part or a
    # wrong position (which the 32 offsets above hold).
    longer = {(t, x, y) for (t, x, y) in tabs["len"] if t in O.HUFF_TABLES and P.pair_bits(tabs, t, P.table_max(tabs, t) if x == 15 else x, P.table_max(tabs, t) if y == 15 else y) > 32}
    assert longer == {(23, 15, 15)} and (tabs["len"][23, 15, 15], tabs["code"][23, 15, 15]) == (8, 3)
    widest = max(P.pair_bits(tabs, t, P.table_max(tabs, t), P.table_max(tabs, t)) for t in (23, 31))
    assert {P.seg_bits(tabs, s) - P.field_bits(s) for _, _, fr in all_frames(("widest_pair",)) for s in fr["segs"]} == {widest} and widest > 32


def test_every_replayed_fill_occurs_in_front_of_a_negative_field():
    tabs, fills, where, per_frame, flushed = P.tables(), set(), set(), [], 0
    for _, st, fr in all_frames(("negative_fields",)):
        f = P.frame_fills(tabs, fr["segs"])
        fills |= set(f)
        per_frame.append(len(f))
        where |= {(st["cls"], w) for w, seg in enumerate(fr["segs"]) if any(fl is not None and fl[0] < 0 for fl in seg["fields"])}
        # a field that does not fit what is left of the buffer: the fill in front of it is what the flush left
        P_ = 0
        for seg in fr["segs"]:
            for n, (kind, j) in P.seg_puts(tabs, seg):
                fl = 32 - P_ < n
                if fl:
                    while P_ > 8:
                        P_ -= 8
                flushed += fl and kind == "field" and seg["fields"][j][0] < 0
                P_ += n
    assert set(range(0, 33)) <= fills       # 0: the frame's first put
    assert {("m1s", w) for w in range(4)} <= where and ("m1m", 1) in where and ("m2m", 0) in where
    assert max(per_frame) >= 2 and flushed >= 5
    # zero-length negative fields (a group whose only values are negative has length 0) and ones with a length
    lens = {fl[1] for _, _, fr in all_frames(("negative_fields",)) for seg in fr["segs"] for fl in seg["fields"] if fl is not None and fl[0] < 0}
    assert {0, 1, 2, 3, 4, 5} <= lens


def test_the_slot_spans_reach_beyond_the_four_near_slots():
    tabs, spans, facts = P.tables(), set(), set()
    for name in ("slots", "classes", "grid_stride"):
        for st in P.case_list(name)["streams"]:
            slots, _, recs = P.stream_layout(tabs, st)
            for i, (fr, rec) in enumerate(zip(st["frames"], recs)):
                spans.add(rec["span"])
                k0, k1 = rec["first_slot"], rec["first_slot"] + rec["span"]
                facts |= {("main_bytes", rec["main_bytes"] > 0), ("stuffing", rec["bytes"] > rec["raw"]), ("packet", bool(fr.get("packet"))),
                          ("own_slot", rec["span"] == 1 and k0 == len(st.get("pending", ())) + i)}
                facts |= {("zero_capacity_near", k) for k in range(k0 + 1, min(k0 + 4, k1 - 1)) if slots[k][1] == 0}
                facts |= {("zero_capacity_far", True) for k in range(k0 + 4, k1 - 1) if slots[k][1] == 0}
    assert {1, 2, 4, 5} <= spans and max(spans) >= 12
    assert {("main_bytes", True), ("main_bytes", False), ("stuffing", True), ("stuffing", False), ("packet", True), ("packet", False),
            ("own_slot", True), ("zero_capacity_far", True)} <= facts
    assert any(f[0] == "zero_capacity_near" for f in facts)


def test_lengths_classes_and_the_grid_stride_list():
    tabs = P.tables()
    bits = [[P.seg_bits(tabs, s) for s in fr["segs"]] for _, _, fr in all_frames(("length",))]
    assert any(4095 in b for b in bits)
    most = 1440 - 36 + 511      # bytes: 320 kbit/s at 32 kHz, less header and side information, plus the reservoir
    assert any(most - 2 <= (sum(b) + 7) // 8 <= most for b in bits)
    lst = P.case_list("classes")
    F, NG, fps, counts = P.list_shape(lst)
    assert fps == NG and counts is not None and {st["cls"] for st in lst["streams"]} == set(P.CLASSES)
    assert any(not P.CLASSES[st["cls"]]["lsf"] and len(st["frames"]) == F and st.get("ghosts") for st in lst["streams"])    # an MPEG-1 stream whose row is NG records long
    assert any(len(st["frames"]) < (2 if P.CLASSES[st["cls"]]["lsf"] else 1) * F for st in lst["streams"]) and 0 in counts     # counts that cut a stream short
    F, NG, fps, counts = P.list_shape(P.case_list("grid_stride"))
    assert fps > P.GRID_CAP and len(P.case_list("grid_stride")["streams"]) == 1
    assert {st["cls"] for name in P.LIST_NAMES for st in P.case_list(name)["streams"]} == set(P.CLASSES)


# ---- hx_debug_pack refuses what the stream walk cannot emit, before anything is launched ----
def refused(b):
    rows = b["rows"].copy()
    rc, status = P.debug_pack(b)
    assert rc == -1 and status == -1 and np.array_equal(rows, b["rows"])
    return api.lib().hx_last_error().decode()


def small():
    return P.build(P.tables(), P.case_list("status"))


def test_a_value_above_its_tables_range_is_refused():
    b = small()
    b["ixq"][0, 0, 0, 3] = 8        # table dimension 8 at the most: 0 .. 7
    assert "above its table's range" in refused(b)
    b = small()
    b["ixq"][0, 1, 1, 2 * 129 + 4] = 2      # a count1 value
    assert "neither 0 nor 1" in refused(b)


def test_records_that_would_leave_a_buffer_are_refused():
    b = small()
    b["seg"][1].start_bit += 1
    assert "start_bit" in refused(b)
    b = small()
    b["seg"][0].tabs = (b["seg"][0].tabs & ~0xFF) | 4
    assert "does not have" in refused(b)
    b = small()
    b["seg"][2].nreg2_quads |= 145 << 16
    assert "576 lines" in refused(b)
    b = small()
    b["seg"][0].sf[0] = (9 << 8) | 1
    assert "longer than 5 bits" in refused(b)
    b = small()
    b["slots"][0].off = b["out_stride"] - 40
    assert "outside the row" in refused(b)
    b = small()
    b["slots"][0].mf = 10
    b["slots"][1].mf = b["slots"][2].mf = 10
    assert "less than the frame's bytes" in refused(b)
    b = small()
    b["frm"][0].raw_bytes -= 1
    assert "raw_bytes" in refused(b)
    b = small()
    b["frm"][0].packet_off = b["packet"].nbytes - 3
    assert "packet" in refused(b)
    b = small()
    b["frm"][0].first_slot = b["fps"] + P.SLOTS_EXTRA
    assert "first_slot" in refused(b)
    b = small()
    b["cls"][0] = 1
    assert "class" in refused(b)
