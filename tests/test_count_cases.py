"""What the records of tests/count_cases.py reach, asserted from the oracle's outputs (not from how the records were built), for
the band tables of all six sample rates; and the oracle held to the reference's own functions - CBitAllo::subdivide2 /
subdivide2BT13 with output_subdivide2, CBitAlloShort::subdivide2, vect_quant / vect_quantB / vect_quantB2 - by == on every
output of every record.  Nothing here needs a GPU: hx_debug_count's refusals come before any launch."""
import numpy as np
import pytest

import count_cases as K
from hmp3_amd import api
from oracle import oracle as O

ALL_RATES = K.RATES["mpeg1"] + K.RATES["mpeg2"]


def tmax(v):
    return K.candidates(int(v))[1]


def channel0(sr):
    """per record of the count set: (rule, block type, ncb, lines, maxima the counter sees, its ten outputs), channel 0"""
    R = K.count_long(sr)
    _, _, out, _ = K.expected("count", sr, False)
    for r in range(R.n):
        ncb = int(R.hdr[r, 2])
        mx = R.ixmax[r, 0].copy()
        mx[ncb:] = 0
        yield R.rules[r], int(R.hdr[r, 0]), ncb, R.ix[r].reshape(-1), mx, [int(v) for v in out[r, :10]]


def initial_regions(bt, cb2):
    if bt != 0:
        return 8, 8
    cb0 = max(K.REG0[cb2], 1)
    return cb0, min(max(cb0 + K.REG1[cb2], cb0 + 1), cb0 + 8)


@pytest.mark.parametrize("sr", ALL_RATES)
def test_classes_edges_regions_and_shrink_branches_are_reached(sr):
    seen_class, seen_value, seen_cb2, shrink1, shrink0, raw_cb2 = set(), set(), set(), set(), set(), set()
    for rule, bt, ncb, ix, mx, (t0, t1, t2, c1, cb0, cb1, cb2, nbig, nquads, bits) in channel0(sr):
        i0, i1 = initial_regions(bt, cb2)
        r = [int(mx[:i0].max(initial=0)), int(mx[i0:i1].max(initial=0)), int(mx[i1:cb2].max(initial=0))]
        for q in ((0, 1, 2) if bt == 0 else (0, 2)):
            seen_class.add((bt, ncb, q, K.value_class(r[q])))
            seen_value.add((bt, ncb, q, r[q]))
        seen_cb2.add((bt, ncb, cb2))
        above1 = np.flatnonzero(mx > 1)
        raw_cb2.add((bt, "below" if (above1[-1] + 1 if len(above1) else 0) < 8 else ("above" if above1[-1] + 1 > 8 else "at")))
        if bt != 0:
            assert (cb0, cb1) == (8, 8)
            continue
        c0t, c1t, c2t = tmax(r[0]), tmax(r[1]), tmax(r[2])
        if not c2t < c1t:
            shrink1.add("not taken")
            assert cb1 == i1
        elif i1 > i0 + 2:
            found = [j for j in range(i1 - 1, i0, -1) if mx[j] > c2t]
            assert cb1 == (found[0] + 1 if found else i0 + 1), rule
            shrink1.add("none" if not found else ("top" if found[0] == i1 - 1 else ("bottom" if found[0] == i0 + 1 else "inside")))
        if not c1t < c0t:
            shrink0.add("not taken")
            assert cb0 == i0
        else:
            n = max(cb1 - 8, 1)
            if not i0 - 1 > n:
                shrink0.add("guard holds it")
                assert cb0 == i0
            else:
                found = [j for j in range(i0 - 1, n, -1) if mx[j] > c1t]
                assert cb0 == (found[0] + 1 if found else n + 1), rule
                shrink0.add("none" if not found else ("top" if found[0] == i0 - 1 else ("bottom" if found[0] == n + 1 else "inside")))
    for ncb in (21, 22):
        for bt in (0, 1, 3):
            for q in ((0, 1, 2) if bt == 0 else (0, 2)):
                # (region 2 ends with the last band above 1: where it is not empty its maximum is at least 2)
                classes = set(range(19)) - ({1} if q == 2 else set())
                assert {c for b, n, qq, c in seen_class if (b, n, qq) == (bt, ncb, q)} >= classes, (bt, ncb, q)
                assert {v for b, n, qq, v in seen_value if (b, n, qq) == (bt, ncb, q)} >= set(K.EDGES) - ({1} if q == 2 else set()), (bt, ncb, q)
            assert {c for b, n, c in seen_cb2 if (b, n) == (bt, ncb)} >= set(range(2 if bt == 0 else 8, ncb + 1)), (bt, ncb)
    assert shrink1 >= {"not taken", "top", "bottom", "none"}, shrink1
    assert shrink0 >= {"not taken", "guard holds it", "top", "bottom", "none"}, shrink0
    assert raw_cb2 >= {(1, "below"), (1, "above"), (3, "below"), (3, "above")}


@pytest.mark.parametrize("sr", ALL_RATES)
def test_ties_follow_the_reference_rule(sr):
    """`<` between the first two candidates, `<=` for the third and fourth, `<` between the two count1 tables"""
    sb = K.tables(sr).startBand_l
    seen = set()
    for rule, bt, ncb, ix, mx, (t0, t1, t2, c1, cb0, cb1, cb2, nbig, nquads, bits) in channel0(sr):
        if rule.startswith("tie "):
            region = int(rule.split("region=")[1])
            a, b = (0, int(sb[cb0])) if region == 0 else (int(sb[cb0]), min(int(sb[cb1]), nbig))
            cands, _ = K.candidates(int(mx[:cb0].max() if region == 0 else mx[cb0:cb1].max()))
            s = K.region_sums(cands, ix[a:b])
            picked = (t0, t1)[region]
            best = s[0] if s[0] < s[1] else s[1]
            if len(cands) == 2 and s[0] == s[1]:
                seen.add("two")
                assert picked == cands[1], rule
            elif len(cands) == 4:
                if s[2] == best and s[3] == best:
                    seen.add("both")
                    assert picked == cands[3], rule
                elif s[2] == best and s[3] > best:
                    seen.add("t2")
                    assert picked == cands[2], rule
                elif s[3] == best and s[2] > best:
                    seen.add("t3")
                    assert picked == cands[3], rule
        if nquads > 0:
            q = ix[nbig:nbig + 4 * nquads].reshape(-1, 4)
            qa = sum(K.quada_len(int(8 * v[0] + 4 * v[1] + 2 * v[2] + v[3])) + int(v.sum()) for v in q)
            qb = sum(4 + int(v.sum()) for v in q)
            if qa == qb:
                seen.add("count1 bt=%d" % bt)
                assert c1 == 1, rule
    assert seen >= {"two", "t2", "t3", "both", "count1 bt=0", "count1 bt=1", "count1 bt=3"}, seen


@pytest.mark.parametrize("sr", ALL_RATES)
def test_where_the_big_values_end_and_the_lane_boundaries(sr):
    t = K.tables(sr)
    sb = [int(v) for v in t.startBand_l]
    seen = set()
    for rule, bt, ncb, ix, mx, (t0, t1, t2, c1, cb0, cb1, cb2, nbig, nquads, bits) in channel0(sr):
        both_sides = lambda e: e >= 2 and ix[e - 2:e].any() and ix[e:e + 2].any()
        if rule.startswith(("zeros", "single_one")):
            # nothing above 1: the first bands stay big values, and the quadruple count comes out of the band widths alone
            assert nbig == sb[2 if bt == 0 else 8] and bits == (0 if rule.startswith("zeros") else bits)
            raw = (sb[1 if bt == 0 else 7] + 4 - nbig) >> 2
            assert nquads == (raw if bt == 0 else max(raw, 0)), rule
            seen.add(("nothing", bt, "negative" if raw < 0 else "not negative"))
        seen.add(("nbig", bt, nbig)) if both_sides(nbig) or nbig in (sb[2], sb[8], 576) else None
        if nbig > 0 and nbig % 128 == 0 and both_sides(nbig):
            seen.add(("nbig on a 64-pair step", nbig))
        n0, n1 = sb[cb0], sb[cb1]
        if bt == 0 and n0 < n1 <= nbig:
            for name, e in (("n0", n0), ("n1", n1)):
                if e < nbig and both_sides(e):
                    seen.add((name, "both sides"))
                    if e % 128 == 0:
                        seen.add((name, "on a 64-pair step"))
        lo2, hi2, lo3 = sb[cb2 - 1], sb[cb2], sb[max(cb2, int(np.flatnonzero(mx > 0)[-1]) + 1 if mx.any() else cb2) - 1]
        if mx[cb2 - 1] > 1 and ix[lo2:hi2].max() <= 1:
            seen.add(("maximum above the lines", "big", bt))
        cb3 = max(cb2, int(np.flatnonzero(mx > 0)[-1]) + 1 if mx.any() else 0)
        if cb3 > cb2 and mx[cb3 - 1] > 0 and not ix[sb[cb3 - 1]:sb[cb3]].any():
            seen.add(("maximum above the lines", "count1", bt))
        if nbig + 4 * max(nquads, 0) > 576:
            seen.add(("past line 575", bt))
    for bt in (0, 1, 3):
        assert ("nbig", bt, sb[2 if bt == 0 else 8]) in seen and ("nbig", bt, 574) in seen and ("nbig", bt, 576) in seen
        assert ("maximum above the lines", "big", bt) in seen and ("maximum above the lines", "count1", bt) in seen
        assert ("past line 575", bt) in seen
        assert ("nothing", bt, "negative") in seen or bt == 0
    # (block type 0 keeps two bands: negative where band 1 is wider than four lines, the MPEG-2 tables)
    assert (("nothing", 0, "negative") in seen) == (sb[2] - sb[1] > 4)
    assert {n for k, n in [s for s in seen if s[0] == "nbig on a 64-pair step"]} == {128, 256, 384, 512}
    assert ("n0", "both sides") in seen and ("n1", "both sides") in seen
    # (region boundaries are band starts: one on a 64-pair step exists only where the rate's table has a band start there)
    for name, bands in (("n0", range(1, 8)), ("n1", range(2, 16))):
        if any(sb[b] % 128 == 0 for b in bands):
            assert (name, "on a 64-pair step") in seen


def test_a_negative_quadruple_count_is_reached_at_block_type_0():
    assert any((sb[2] - sb[1]) > 4 for sb in (K.tables(sr).startBand_l for sr in K.RATES["mpeg2"]))


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_largest_sums_fit_the_packed_accumulators(sr):
    """a granule of 8206 throughout: each candidate's length over a region is what one half of a packed 32-bit sum holds"""
    sb = K.tables(sr).startBand_l
    n = 0
    for rule, bt, ncb, ix, mx, (t0, t1, t2, c1, cb0, cb1, cb2, nbig, nquads, bits) in channel0(sr):
        if not rule.startswith("all_8206"):
            continue
        n += 1
        assert nbig == 576 and nquads == 0 and cb2 == 22 and (ix[:576] == 8206).all()
        worst = 0
        for a, b in ((0, int(sb[cb0])), (int(sb[cb0]), int(sb[cb1])), (int(sb[cb1]), 576)):
            if b > a:
                worst = max(worst, max(K.region_sums(K.candidates(8206)[0], ix[a:b])))
        assert bits < worst * 3 and worst < 65536 // 2, (worst, bits)        # a factor of two to spare
        assert max(K.pair_len(t, 8206, 8206) for t in K.candidates(8206)[0]) * 5 < 65536     # a lane's five pairs
    assert n == 6


@pytest.mark.parametrize("sr", ALL_RATES)
def test_channels_side_by_side(sr):
    R = K.count_long(sr)
    _, _, out, sums = K.expected("count", sr, False)
    rules = list(R.rules)
    for bt in (0, 1, 3):
        rows = [rules.index("beside k=%d bt=%d" % (k, bt)) for k in (1, 2, 3)]
        assert all(np.array_equal(out[rows[0], :10], out[r, :10]) for r in rows) and len({tuple(out[r, 10:20]) for r in rows}) == 3
        assert len({int(R.hdr[r, 3]) for r in rows}) == 3 and all(sums[r] == out[r, 9] + out[r, 19] for r in rows)
        s = rules.index("swapped bt=%d" % bt)
        assert R.hdr[s, 2] != R.hdr[s, 3] and np.array_equal(out[s, 10:20], out[rows[0], :10])
        m = rules.index("mono bt=%d" % bt)
        assert R.hdr[m, 1] == 1 and not out[m, 10:20].any() and sums[m] == out[m, 9] and np.array_equal(out[m, :10], out[rows[0], :10])
        # channel 0's last quadruple on lines 576 and 577: it counts channel 1's lines 0 and 1
        for last in (574, 575):
            b = {l: out[rules.index("over_read ch1=%s last=%d bt=%d" % (l, last, bt))] for l in ("00", "10", "01", "11")}
            assert all(v[7] + 4 * v[8] == 578 for v in b.values())
            assert all(np.array_equal(v[:9], b["00"][:9]) or v[3] != b["00"][3] for v in b.values())
            assert b["00"][9] < b["10"][9] < b["11"][9] and b["00"][9] < b["01"][9] < b["11"][9]       # (every 1 costs its sign bit at the least)
    assert sum(r.startswith("random") for r in rules) == 3 * K.RANDOM_PER_BT
    assert R.unfused.sum() == 24 and not R.slim.any()


@pytest.mark.parametrize("sr", [K.RATES["mpeg1"][0], K.RATES["mpeg2"][0]])
def test_every_rounding_threshold_of_every_gain_step(sr):
    """for each gain step and rule, two neighbouring floats that quantise to n - 1 and to n, for every n of the targets: the
    floats are the records' own, the values the oracle's"""
    t = K.tables(sr)
    want = set(n for n in K.THRESHOLD_TARGETS if n > 0)

    def steps(u, q):
        o = np.argsort(u)
        u, q = u[o].astype(np.int64), q[o].astype(np.int64)
        at = np.flatnonzero((np.diff(u) == 1) & (np.diff(q) == 1))
        return set(int(v) for v in q[at + 1])

    R = K.quant_long(sr)
    ix, _, _, _ = K.expected("quant_count", sr, False)
    seen = {}
    for r in range(R.n):
        if R.rules[r].startswith("thresholds"):
            for c in range(2):
                g, opt = int(R.gsf[r, c, 0]), int(R.hdr[r, 4])
                n = int(np.flatnonzero(R.x34[r, c].view(np.uint32))[-1]) + 1
                seen[opt, g] = steps(R.x34[r, c, :n].view(np.uint32), ix[r].reshape(2, 576)[c, :n])
                u = R.x34[r, c, :n + 1].view(np.uint32)
                assert (u == 0).any() and ((u > 0) & (u < 0x800000)).any(), "zero and subnormal magnitudes"
                assert ix[r].reshape(2, 576)[c, :n].max() == 8206
    assert set(seen) == {(opt, g) for opt in (0, 1) for g in range(128)}
    assert all(s >= want for s in seen.values()), [k for k, s in seen.items() if not s >= want][:4]
    # short blocks: plain, and the table rule with its first offset at -0.30
    S = K.short_quant(sr)
    sx, _, _, _ = K.expected("short", sr, False)
    seen = {}
    for r in range(S.n):
        if S.rules[r].startswith("short_thresholds"):
            for k in range(6):
                u = S.x34[r].reshape(6, 192)[k].view(np.uint32)
                if u.any():
                    key = (int(S.hdr[r, 4]), int(S.gsf[r].reshape(6, 16)[k, 0]))
                    seen.setdefault(key, [[], []])
                    n = int(np.flatnonzero(u)[-1]) + 1
                    seen[key][0].append(u[:n])
                    seen[key][1].append(sx[r].reshape(6, 192)[k, :n])
    assert set(seen) == {(opt, g) for opt in (0, 1) for g in range(128)}
    for key, (u, q) in seen.items():
        assert steps(np.concatenate(u), np.concatenate(q)) >= want, key
    # the three rules differ where they should: the first offset, and the table's offsets beyond it
    x = np.float32(0.5) / np.float32(t.quant_lines(0, np.ones(1, np.float32), 8)[0] or 1)
    probe = np.linspace(0.05, 3.0, 600, dtype=np.float32)
    q = [t.quant_lines(rule, probe, 8) for rule in (0, 1, 2)]
    assert (q[0] != q[1]).any() and (q[1] != q[2]).any() and x > 0


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_quantising_records_reach_the_line_buffer_rules(sr):
    R = K.quant_long(sr)
    sb = K.tables(sr).startBand_l
    plain = K.expected("quant_count", sr, False)
    slim = K.expected("quant_count", sr, True)
    seen = set()
    for r in range(R.n):
        opt, nchan = int(R.hdr[r, 4]), int(R.hdr[r, 1])
        for c in range(nchan):
            nsf, nl = int(R.hdr[r, 6 + c]), int(R.hdr[r, 8 + c])
            assert nl == sb[nsf]
            past_in, past_slim = R.ix[r, c, nl:], slim[0][r].reshape(2, 576)[c, nl:]
            if R.slim[r] and past_in.any():
                assert not (opt & 2) and not past_slim.any()
                seen.add("written as zero")
            elif opt & 2 and past_in.any():
                assert np.array_equal(past_in, past_slim) and np.array_equal(past_in, plain[0][r].reshape(2, 576)[c, nl:])
                seen.add("left alone")
            if nsf < 22 and R.ixmax[r, c, nsf:].any() and not (R.hdr[r, 5] and c == 0):
                assert np.array_equal(R.ixmax[r, c, nsf:], slim[1][r].reshape(2, 22)[c, nsf:])
                seen.add("maxima kept")
        if R.hdr[r, 5]:
            assert R.ixmax[r, 0, 21] > 0 and plain[1][r].reshape(2, 22)[0, 21] == 0
            seen.add("zero21")
        if not R.slim[r]:
            assert all(np.array_equal(a[r], b[r]) for a, b in zip(plain[:3], slim[:3]))
        seen.add(("opt", opt, int(R.hdr[r, 0]), nchan))
    assert seen >= {"written as zero", "left alone", "maxima kept", "zero21"}
    assert {s[1:] for s in seen if s[0] == "opt"} >= {(o, bt, 2) for o in (0, 1, 3) for bt in (0, 1, 3)} | {(o, 0, 1) for o in (0, 1, 3)}
    over = [r for r in range(R.n) if R.unfused[r]]
    assert len(over) == 3 and all(plain[2][r, 7] + 4 * plain[2][r, 8] == 578 for r in over)
    assert len({int(plain[2][r, 9]) for r in over}) >= 2        # channel 1's quantised lines 0 and 1 are counted


@pytest.mark.parametrize("sr", ALL_RATES)
def test_short_records_reach_classes_and_ties(sr):
    S = K.short_count(sr)
    t = K.tables(sr)
    _, _, out, _ = K.expected("short_count", sr, False)
    classes, ties = set(), set()
    for r in range(S.n):
        for c in range(int(S.hdr[r, 1])):
            mx = S.ixmax[r, c].reshape(3, 16)[:, :t.nsfs]
            o = out[r, 10 * c:10 * c + 10]
            assert o[4] == 3 and 3 <= o[5] <= o[6] <= t.nsfs and o[7] == t.startBand_s[o[5]]
            classes.add((0, K.value_class(int(mx[:, :3].max()))))
            classes.add((1, K.value_class(int(mx[:, 3:o[5]].max(initial=0)))))
        if S.rules[r].startswith("short_tie"):
            n0 = int(t.startBand_s[3])
            cands, _ = K.candidates(int(S.ixmax[r, 0].reshape(3, 16)[:, :3].max()))
            s = K.region_sums(cands, S.ix[r, 0].reshape(3, 192)[:, :n0].reshape(-1))
            best = s[0] if s[0] < s[1] else s[1]
            if len(cands) == 2:
                kind, pick = ("two", cands[1]) if s[0] == s[1] else ("", out[r, 0])
            elif s[2] == best == s[3]:
                kind, pick = "both", cands[3]
            elif s[2] == best < s[3]:
                kind, pick = "t2", cands[2]
            elif s[3] == best < s[2]:
                kind, pick = "t3", cands[3]
            else:
                kind, pick = "", out[r, 0]
            ties.add(kind)
            assert out[r, 0] == pick, S.rules[r]
    assert {c for q, c in classes if q == 0} == set(range(19)) and {c for q, c in classes if q == 1} >= set(range(19)) - {1}
    assert ties >= {"two", "t2", "t3", "both"}
    assert any(S.hdr[r, 1] == 1 for r in range(S.n))


# ---- the oracle against the reference's own functions, on every record ----

@pytest.mark.skipif(not O.ref_has_count_records(), reason="oracle/_ref is not built (or predates the quantise-and-count entries of its harness)")
@pytest.mark.parametrize("mode", ["count", "quant_count", "short", "short_count"])
@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_oracle_is_the_reference_on_every_record(sr, mode):
    R = K.records(mode, sr)
    t = K.tables(sr, True)
    lines, maxima, out, sums = K.expected(mode, sr, False)
    rl, rm, rout, rsums = K.expected(mode, sr, False, True)
    short = mode.startswith("short")
    for r in range(R.n):
        where = "record %d (%s)" % (r, R.rules[r])
        assert sums[r] == rsums[r], "%s: the sum is %d, the reference's %d" % (where, sums[r], rsums[r])
        for c in range(int(R.hdr[r, 1])):
            if short:
                for k, name in enumerate(O.COUNT_OUT):
                    assert out[r, 10 * c + k] == rout[r, 10 * c + k], "%s channel %d: %s is %d, the reference's %d" % (where, c, name, out[r, 10 * c + k], rout[r, 10 * c + k])
                assert np.array_equal(maxima[r].reshape(2, 3, 16)[c, :, :t.nsfs], rm[r].reshape(2, 3, 16)[c, :, :t.nsfs]), where
            else:
                assert out[r, 10 * c + 9] == rout[r, 12 * c], "%s channel %d: bits is %d, the reference's %d" % (where, c, out[r, 10 * c + 9], rout[r, 12 * c])
                gr = O.count_out_to_gr(t, out[r, 10 * c:10 * c + 10])
                for k, name in enumerate(O.COUNT_GR):
                    assert gr[k] == rout[r, 12 * c + 1 + k], "%s channel %d: %s is %d, the reference's %d" % (where, c, name, gr[k], rout[r, 12 * c + 1 + k])
                assert np.array_equal(maxima[r].reshape(2, 22)[c], rm[r].reshape(2, 22)[c]), where
            assert np.array_equal(lines[r].reshape(2, 576)[c], rl[r].reshape(2, 576)[c]), where


@pytest.mark.skipif(not O.ref_has_count_records(), reason="oracle/_ref is not built (or predates the quantise-and-count entries of its harness)")
def test_the_oracles_quantisers_are_the_references_at_every_threshold():
    for sr in (K.RATES["mpeg1"][0], K.RATES["mpeg2"][0]):
        t = K.tables(sr, True)
        for rule in (0, 1, 2):
            for g in range(128):
                u = K.threshold_lines(sr, rule, g).view(np.float32)
                assert np.array_equal(t.quant_lines(rule, u, g), t.quant_lines(rule, u, g, use_ref=True)), (sr, rule, g)


# ---- hx_debug_count refuses what the walk cannot hand over, before anything is launched ----

def refused(unit, mode, a, sr=K.RATES["mpeg1"][0]):
    quant = mode in ("quant_count", "quant_then_count", "short")
    ec = api.default_control(samprate=sr, **K.UNITS[unit][1])
    rc, ix, mx, out = api.debug_count(ec, unit, mode, a["hdr"], a["ix"], a["ixmax"], a["x34"] if quant else None, a["gsf"] if quant else None)
    assert rc == -1 and not out.any() and np.array_equal(ix.reshape(a["ix"].shape), a["ix"])
    return api.last_error()


def some(mode, rule, sr=K.RATES["mpeg1"][0]):
    R = K.records(mode, sr)
    r = next(i for i in range(R.n) if R.rules[i].startswith(rule))
    return R.pick(np.array([0, r]))


def test_values_outside_the_counters_tables_are_refused():
    a = some("count", "random k=1 ")
    a["ix"][1, 0, 3] = 8207
    assert "record 1 channel 0: a line outside" in refused("k_alloc", "count", a)
    a = some("count", "random k=1 ")
    a["ix"][1, 1, 5] = -1
    assert "record 1 channel 1: a line outside" in refused("k_alloc1", "count", a)
    a = some("count", "cb2=9 bt=0 ncb=22")
    a["ix"][1, 0, 0] = a["ixmax"][1, 0, 0] + 1
    assert "above its band's maximum" in refused("k_alloc_slim", "count", a)
    a = some("count", "nbig=128 tail=2 bt=0")
    a["ix"][1, 0, 130], a["ixmax"][1, 0] = 2, np.maximum(a["ixmax"][1, 0], 2)
    a["ixmax"][1, 0, 14:] = 0       # (the band of line 130 stays behind the last band above 1 ... by its maximum alone)
    a["ix"][1, 0, 134:] = 0
    msg = refused("k_alloc", "count", a)
    assert "above its band's maximum" in msg or "value above 1" in msg
    a = some("count", "random k=1 ")
    a["hdr"][1, 0] = 2
    assert "block type" in refused("k_alloc", "count", a)
    a["hdr"][1, 0], a["hdr"][1, 2] = 0, 23
    assert "ncb" in refused("k_alloc", "count", a)
    a["hdr"][1, 2], a["hdr"][1, 12] = 22, 1
    assert "spare" in refused("k_alloc", "count", a)


def test_a_last_quadruple_past_line_575_is_taken_from_channel_0_of_two_unfused_only():
    a = some("count", "over_read ch1=11 last=575 bt=0")
    a["ix"][1], a["ixmax"][1] = a["ix"][1, ::-1].copy(), a["ixmax"][1, ::-1].copy()
    assert "record 1 channel 1: the last count1 quadruple reaches past line 575" in refused("k_alloc", "count", a)
    a = some("count", "over_read ch1=00 last=574 bt=3")
    a["hdr"][1, 1], a["hdr"][1, 3] = 1, 0
    assert "past line 575" in refused("k_alloc_slim", "count", a)
    a = some("count", "over_read ch1=11 last=575 bt=0")
    a["ix"][1, 1, 1], a["ixmax"][1, 1, 0] = 2, 2
    assert "value above 1" in refused("k_alloc", "count", a)
    a = some("quant_count", "over_read_quant ch1=01")
    assert "the walk goes unfused there" in refused("k_alloc", "quant_count", a)


def test_quantising_records_the_walk_cannot_hand_over_are_refused():
    sb = K.tables(K.RATES["mpeg1"][0]).startBand_l
    rule = "random_quant k=4 "
    a = some("quant_count", rule)
    a["hdr"][1, 8] -= 2
    assert "nbmax" in refused("k_alloc", "quant_count", a)
    a = some("quant_count", rule)
    a["gsf"][1, 1, 3] = 128
    assert "gain step" in refused("k_alloc", "quant_then_count", a)
    for bad in (np.float32(-1.0), np.float32(np.inf), np.float32(np.nan), np.float32(3.0e38)):
        a = some("quant_count", rule)
        a["x34"][1, 0, 2] = bad
        assert "not a finite magnitude, or that quantises above 8206" in refused("k_alloc_slim", "quant_count", a)
    a = some("quant_count", "thresholds opt=1 gsf=40,41")
    n = int(np.flatnonzero(a["x34"][1, 0])[-1])
    a["x34"][1, 0, n] = a["x34"][1, 0, n] * np.float32(1.001)
    assert "quantises above 8206" in refused("k_alloc", "quant_count", a)      # (the largest float of the record quantises to 8206)
    R = K.quant_long(K.RATES["mpeg1"][0])
    r = int(np.flatnonzero(R.slim)[0])
    a = R.pick(np.array([0, r]))
    assert "at or past nbmax is not zero" in refused("k_alloc", "quant_count", a)
    a = some("quant_count", rule)
    a["hdr"][1, 4] = 2
    assert "opt" in refused("k_alloc", "quant_count", a)
    a = some("short", "short_random k=1")
    a["gsf"][1, 0, 5] = -1
    assert "gain step" in refused("k_alloc", "short", a)
    a = some("short_count", "short_random k=1")
    a["ix"][1, 0, 0] = a["ixmax"][1, 0, 0] + 1
    assert "above its band's maximum" in refused("k_alloc", "short_count", a)
    a["hdr"][1, 4] = 1
    assert "opt" in refused("k_alloc", "short_count", a)


def test_a_unit_takes_the_controls_it_walks_and_calls_are_bounded():
    a = some("count", "random k=1 ")
    ec1, ec2 = api.default_control(samprate=44100, bitrate=64), api.default_control(samprate=22050, bitrate=64)
    eca = api.default_control(samprate=44100, bitrate=64, nsbstereo=8)
    for ec, unit in ((ec1, "k_alloc_lsf"), (ec2, "k_alloc"), (ec1, "k_alloc1"), (eca, "k_alloc_slim"), (ec2, "k_alloc1_lsf")):
        assert api.debug_count(ec, unit, "count", a["hdr"], a["ix"], a["ixmax"])[0] == -1 and "does not run streams of this control" in api.last_error()
    assert api.debug_count(ec1, "k_pack", "count", a["hdr"], a["ix"], a["ixmax"])[0] == -1 and "no stream-walk unit" in api.last_error()
    L = api.lib()
    import ctypes as C
    z = np.zeros(16, np.int32)
    assert L.hx_debug_count(0, C.byref(ec1), b"k_alloc", 0, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, z.ctypes.data) == -1
    assert L.hx_debug_count(0, C.byref(ec1), b"k_alloc", 0, 16385, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, z.ctypes.data) == -1 and "16384" in api.last_error()
    assert L.hx_debug_count(0, C.byref(ec1), b"k_alloc", 5, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, z.ctypes.data) == -1
    assert L.hx_debug_count(0, C.byref(ec1), b"k_alloc", 1, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, z.ctypes.data) == -1 and "null" in api.last_error()
