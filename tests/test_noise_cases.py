"""What the constructed granules of tests/noise_cases.py reach, asserted on the CPU from the oracle's outputs and path counters,
and the oracle held to the reference's own noise_seek_actual (ifnc_noise_actual, decrease_noise, increase_noise) and inverse_sf2
on every record by ==.  The restatement of the device's summation order must arrive at the oracle's outputs too - it adds the
fall-back band strictly, as the device does - and never sees a certificate pass a band whose lane sum lies in another bucket
than the strict sum.  The host's rules for a record are checked here as well: a refusal needs no GPU."""
import os

import numpy as np
import pytest

import noise_cases as K
from hmp3_amd import api
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "hmp3_amd", "libhmp3amd.so")), reason="hmp3_amd/libhmp3amd.so not built (hmp3_amd/build.sh)")
ALL_RATES = K.RATES["mpeg1"] + K.RATES["mpeg2"]


def band_words(out):
    return out[:, :176].reshape(-1, 2, 22, 4)


@pytest.mark.skipif(not O.ref_has_noise_records(), reason="oracle/_ref not built, or built before the harness had ref_seek_record")
@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_oracle_is_the_reference_on_every_record(sr):
    for mode in K.MODES:
        R = K.records(mode, sr)
        tabs = O.CountTables(O.default_control(samprate=sr, **K.CONTROL), use_ref=True)
        want = band_words(O.noise_records(tabs, mode, R.hdr, R.xr, R.band, x34=R.x34, ix=R.ix, use_ref=True))
        got = band_words(K.reference(mode, sr)[0])
        for k, name in enumerate(("gsf", "Noise", "NTadjust") if mode == "seek" else ("sf",)):
            bad = np.argwhere(got[..., k] != want[..., k])
            assert not len(bad), "%s %d Hz record %d (%s: %s) channel %d band %d: %s is %d, the reference's %d" % (
                mode, sr, bad[0][0], R.lists[bad[0][0]], R.rules[bad[0][0]], bad[0][1], bad[0][2], name, got[tuple(bad[0]) + (k,)], want[tuple(bad[0]) + (k,)])


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_restatement_arrives_at_the_oracles_outputs(sr):
    for mode in K.MODES:
        R = K.records(mode, sr)
        want, res, forced = K.reference(mode, sr)
        for r in (res, forced):
            got = np.zeros_like(want)
            g = band_words(got)
            if mode == "seek":
                g[..., 0], g[..., 1], g[..., 2], g[..., 3] = r["gsf"].reshape(-1, 2, 22), r["Noise"].reshape(-1, 2, 22), r["NTadjust"].reshape(-1, 2, 22), -1
            else:
                g[..., 0], g[..., 1] = r["sf"].reshape(-1, 2, 22), np.where(r["sel"].reshape(-1, 2, 22), 1, -1)
            assert K.first_difference(R, np.arange(R.n), got, want) is None, K.first_difference(R, np.arange(R.n), got, want)
        if mode == "seek":
            assert np.array_equal(forced["nstrict"], res["sweeps"].reshape(-1, 2).sum(axis=1)) and np.array_equal(forced["big"], res["big"])


def test_every_unit_runs_a_hundred_records_of_every_mode_and_rate():
    for unit, family in K.UNITS.items():
        for sr in K.RATES[family]:
            for mode in K.MODES:
                R = K.records(mode, sr)
                keep = K.runs(unit, R)
                assert len(keep) >= 100
                assert len(keep) == R.n or unit in K.LEFT_OUT
                assert set(R.lists) == set(K.LISTS[mode])


def trace(T, a, r, c, b):
    """the search of one band step by step through the oracle's noise_actual (bitallo3.cpp:1164-1288 written out) ->
    (kind as noise_cases.seek names it, dn of the first measurement, [(step, noise)])"""
    sl = slice(T.start[b], T.start[b] + T.width[b])
    NT, Noise0, s = (int(a["band"][r, c, b, k]) for k in range(3))
    N = lambda g: O.noise_band(T.o, a["x34"][r, c, sl], a["xr"][r, c, sl], g, int(T.logcbw[b]))
    if Noise0 <= NT:
        return 0, None, []
    steps = [(s, N(s))]
    dn = steps[0][1] - NT
    kind = 1
    if dn > 100:
        kind, t = 4, s - 1
        for _ in range(min(t, 20)):
            steps.append((t, N(t)))
            if steps[-1][1] <= NT:
                kind = 2
                break
            t -= 1
    elif dn < -100:
        kind, t = 5, s
        for _ in range(20):
            t += 1
            steps.append((t, N(t)))
            if steps[-1][1] >= NT:
                kind = 3
                break
    return kind, dn, steps


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_walk_list_puts_bands_into_every_state_of_the_search(sr):
    R = K.records("seek", sr)
    T = R.T
    want, res, _ = K.reference("seek", sr)
    rows = R.rows("walk")
    a = R.pick(np.arange(R.n))
    out = band_words(want)
    kinds = res["kind"].reshape(-1, 2, 22)
    # no certificate fails on this list: the expected count of strict fall-backs is zero
    assert not res["nstrict"][rows].any() and not res["differs"].reshape(-1, 2, 22)[rows].any()
    seen = set()
    ties, longest = {"tie down": 0, "tie up": 0}, {}
    for r in rows:
        rule = R.rules[r]
        if " | " not in rule or ":" in rule or rule.split(" | ")[0] != rule.split(" | ")[1]:
            continue
        rule = rule.split(" | ")[0]
        seen.add(rule)
        for c in range(2):
            for b in range(T.nb):
                kind, dn, steps = trace(T, a, r, c, b)
                assert kind == kinds[r, c, b], "the restatement's search ends another way than the oracle's"
                ad = [abs(n - int(a["band"][r, c, b, 0])) for _, n in steps]
                if steps:
                    best = steps[ad.index(min(ad))]         # (the first of equals)
                    assert (out[r, c, b, 0], out[r, c, b, 1]) == best
                    assert out[r, c, b, 2] == a["band"][r, c, b, 4] + (dn >> 3)
                if rule == "unmeasured":
                    assert kind == 0 and out[r, c, b, 0] == a["band"][r, c, b, 3] + 5 and out[r, c, b, 1] == a["band"][r, c, b, 1]
                elif rule in ("dn=100", "dn=-100"):
                    assert kind == 1 and dn == int(rule[3:]) and len(steps) == 1
                elif rule == "dn=101":
                    assert dn == 101 and kind in (2, 4) and len(steps) > 1 and steps[1][0] == steps[0][0] - 1
                elif rule == "dn=-101":
                    assert dn == -101 and kind in (3, 5) and len(steps) > 1 and steps[1][0] == steps[0][0] + 1
                elif rule == "down to target":
                    assert kind == 2 and 2 <= len(steps) <= 20      # (noise is not monotone in the step: a walk may stop before the step the target was read at)
                    longest[rule] = max(longest.get(rule, 0), len(steps))
                elif rule == "down 20 steps":
                    assert kind == 4 and len(steps) == 21 and steps[-1][0] == steps[0][0] - 20
                elif rule.startswith("start "):
                    assert kind == 4 and dn > 100 and steps[0][0] == int(rule[6:]) and len(steps) == int(rule[6:])      # niter = 0, 1, 2
                elif rule == "up to target":
                    assert kind == 3 and 2 <= len(steps) <= 20
                    longest[rule] = max(longest.get(rule, 0), len(steps))
                elif rule == "up 20 steps":
                    assert kind == 5 and len(steps) == 21 and steps[-1][0] == steps[0][0] + 20
                elif rule == "dn=-5" or (rule.startswith("tie") and ad.count(min(ad)) < 2):
                    assert dn == -5 and kind == 1 and out[r, c, b, 2] == a["band"][r, c, b, 4] - 1      # (-5 >> 3 is -1; -5 / 8 is 0)
                else:
                    assert ad.count(min(ad)) == 2 and ad.index(min(ad)) == len(ad) - 2 and kind == (2 if rule == "tie down" else 3)
                    ties[rule] += 1
    assert seen == set(K.WALK_RULES) and min(ties.values()) >= 3 and min(longest.values()) >= 12, (ties, longest)
    by = lambda tag: [r for r in rows if R.rules[r].startswith(tag)]
    assert all(a["hdr"][r, 1] != a["hdr"][r, 2] for r in by("nsf differ")) and len(by("nsf differ")) == 2
    for r in by("mono"):
        assert a["hdr"][r, 0] == 1 and not a["hdr"][r, [2, 4]].any() and (out[r, 1, :, 3] == -1).all() and not out[r, 1, :, 1].any()
    assert len(by("mono")) == 3
    sweeps = res["sweeps"].reshape(-1, 2)
    assert [tuple(sweeps[r]) for r in by("channel 1 goes on")] == [(1, 21)] and [tuple(sweeps[r]) for r in by("channel 0 goes on")] == [(21, 0)]
    beside = by("beside")
    assert len(beside) == 3 and all(np.array_equal(out[beside[0], 0], out[r, 0]) for r in beside) and len({out[r, 1].tobytes() for r in beside}) == 3


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_layout_list_measures_every_band_alone_and_all_together(sr):
    R = K.records("seek", sr)
    T = R.T
    want, res, _ = K.reference("seek", sr)
    rows = R.rows("layout")
    measured = res["measured"].reshape(-1, 2, 22)
    alone = {(c, b) for r in rows for c in range(2) for b in range(T.nb) if measured[r, c, b] and measured[r, c].astype(bool).sum() == 1}
    assert alone == {(c, b) for c in range(2) for b in range(T.nb)}
    full = [r for r in rows if R.rules[r] == "every band"]
    assert len(full) >= 4 and all(measured[r, :, :T.nb].all() and (R.xr[r, :, 575] != 0).all() and (R.x34[r, :, 575] != 0).all() for r in full)
    used = int((T.l_cnt > 0).sum())
    if sr == 32000:
        assert (T.W, used) == (10, 64)          # every lane holds a run
    # a pattern in the lines behind the measured bands changes nothing
    out = band_words(want)
    pairs = [(r, r + 1) for r in rows if R.rules[r].endswith("zeros behind")]
    assert len(pairs) == 4
    for z, s in pairs:
        assert R.rules[s].endswith("sentinel behind") and (R.xr[s] == K.SENTINEL).any() and not np.array_equal(R.xr[z], R.xr[s])
        assert np.array_equal(out[z], out[s]) and np.array_equal(res["sweeps"].reshape(-1, 2)[z], res["sweeps"].reshape(-1, 2)[s])


def test_the_address_clamp_of_the_pair_loops_is_beyond_the_six_band_tables():
    """min(q.start + k, 574) in sweep_load / isf2_run guards the pairs an unrolled loop reads past the class's run width: a run
    would have to start at line 568 or later.  Without -HF at most 21 bands are measured and the last run of the widest table
    (32 kHz) starts at line 548, so no record of these lists - and no stream of these classes - reaches the clamp; this test
    says so, and fails when a table moves far enough for the lists to need such a record"""
    assert max(int(K.tables(sr).l_start[K.tables(sr).l_cnt > 0].max()) for sr in ALL_RATES) == 548


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_edge_lists_hold_bands_whose_lane_sum_is_in_another_bucket(sr):
    """minimum counts per band table, and the fall-backs the restatement predicts for them"""
    for mode, edge, worst in (("seek", "bucket_edge", "worst_case"), ("isf2", "ratio_edge", "ratio_worst_case")):
        R = K.records(mode, sr)
        want, res, _ = K.reference(mode, sr)
        differs = res["differs"].reshape(-1, 2, 22) > 0
        assert differs[R.rows(edge)].sum() >= 32 and differs[R.rows(worst)].sum() >= 8
        # every band of these records lies on a boundary: both channels of every record fall back, once (one sweep)
        assert (res["nstrict"][R.rows(edge)] == 2).all() and (res["nstrict"][R.rows(worst)] == 2).all()
        if mode == "seek":
            assert (res["sweeps"][np.repeat(2 * R.rows(edge), 2) + np.tile([0, 1], len(R.rows(edge)))] == 1).all()
            widths = {int(R.T.width[b]) for r in R.rows(worst) for c in range(2) for b in range(R.T.nb) if differs[r, c, b]}
            assert max(widths) == R.T.width[:R.T.nb].max()          # up to the widest band of the table


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_double_table_list_reaches_the_double_table_and_a_strict_sum_behind_it(sr):
    R = K.records("seek", sr)
    want, res, _ = K.reference("seek", sr)
    rows = R.rows("double_table")
    reach = want[:, 178:181]
    values = [r for r in rows if R.rules[r].startswith("values to")]
    assert len(values) == 18 and all(reach[r, 0] > 0 and res["big"][r] > 0 for r in values)
    for r in values:
        top = int(R.rules[r].split()[2])
        assert reach[r, 2] >= top and (reach[r, 1] > 0) == (reach[r, 2] >= 16384)
    assert sum(reach[r, 1] > 0 for r in values) >= 6 and {R.rules[r].split(" in ")[1] for r in values} == {"one band", "several bands"}
    strict = res["strict"].reshape(-1, 2)
    big = lambda r: res["big"][r]
    loud = [r for r in rows if R.rules[r] == "edges beside a loud band"]
    # the loud channel's one sweep is a double-table pass with bands on a boundary: the strict sum finds the terms stored
    assert len(loud) == 4 and all(big(r) == 1 and strict[r, r & 1] == 1 and reach[r, 0] > 0 for r in [x for x in loud])
    behind = [r for r in rows if R.rules[r].startswith("a strict band in the plain sweeps")]
    sweeps = res["sweeps"].reshape(-1, 2)
    # one double-table pass per channel, then twenty plain sweeps every one of which adds a band strictly
    assert len(behind) == 4 and all(big(r) == 2 and (sweeps[r] == 21).all() and (strict[r] >= 20).all() for r in behind)


@pytest.mark.parametrize("sr", ALL_RATES)
def test_the_select_list_refines_what_it_names(sr):
    R = K.records("isf2", sr)
    want, res, _ = K.reference("isf2", sr)
    rows = R.rows("select")
    reach, out = want[:, 178:181], band_words(want)
    side = [r for r in rows if R.rules[r].startswith("maxima")]
    for r in side:
        m = R.band[r, :, :R.T.nb, 3]
        assert set(m.reshape(-1)) == {0, 1, 2, 3, 8191}
        assert np.array_equal(out[r, :, :R.T.nb, 1] == 1, (m == 1) | (m == 2)) and (out[r, :, R.T.nb:, 1] == -1).all()
        keep = out[r, :, :, 1] != 1
        assert np.array_equal(out[r][keep][:, 0], R.band[r][keep][:, 2])         # a band that is not refined keeps its scalefactor
    assert {tuple(R.hdr[r, 7:9]) for r in side} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert min(R.hdr[r, 5:7].min() for r in side) <= 5 and max(R.hdr[r, 5:7].max() for r in side) >= 250
    for k in range(3):          # inside the limits, above up, below lo: each all over a record
        rs = [r for r in rows if R.rules[r] == "every band refined, clamp %d" % k]
        assert len(rs) >= 10
        if k == 0:
            assert not reach[rs, 1:].any() and (reach[rs, 0] == 2 * R.T.nb).all()
        else:
            assert reach[rs, k].sum() > 0.8 * reach[rs, 0].sum()
    none = [r for r in rows if R.rules[r] == "no band refined"]
    assert len(none) == 4 and not reach[none].any() and (out[none][..., 1] == -1).all() and not res["nstrict"][none].any()
    mono = [r for r in rows if R.rules[r] == "mono"]
    assert len(mono) == 8 and reach[mono, 0].all() and (R.hdr[mono, 0] == 1).all() and (out[mono][:, 1, :, 1] == -1).all()


def test_the_host_refuses_a_record_by_the_rule_of_the_field():
    """nothing is launched for a refused call (there is no GPU here to launch on): the message names record, channel, band and field"""
    sr = 44100
    for mode, cases in (("seek", [("hdr", (1, 0), 3, "record 1: nchan"), ("hdr", (1, 9), 1, "record 1: the short-block band count"), ("hdr", (1, 10), 1, "record 1: the -HF count"),
                                  ("hdr", (0, 1), 22, "record 0 channel 0: nsf"), ("hdr", (0, 4), 2, "record 0 channel 1: nbmax"), ("hdr", (2, 5), 1, "record 2 channel 0: G"),
                                  ("xr", (3, 1, 17), np.inf, "record 3 channel 1 band"), ("x34", (3, 0, 5), -1.0, "record 3 channel 0 band"), ("x34", (3, 0, 5), np.nan, ": x34"),
                                  ("x34max", (2, 1, 6), 0.5, "record 2 channel 1 band 6: x34max"), ("band", (2, 1, 3, 2), 108, "record 2 channel 1 band 3: gsf"),
                                  ("band", (2, 0, 3, 2), -1, "band 3: gsf"), ("band", (0, 0, 0, 0), 1 << 21, "band 0: NT"), ("band", (0, 0, 1, 1), -(1 << 21), "band 1: Noise0"),
                                  ("band", (0, 1, 2, 4), 1 << 21, "band 2: NTadjust"), ("band", (0, 1, 2, 3), 128, "band 2: gzero"), ("band", (0, 1, 2, 6), 1, "a spare band word")]),
                        ("isf2", [("ix", (4, 1, 30), 9000, "record 4 channel 1 band"), ("band", (5, 0, 4, 3), 9, "record 5 channel 0 band 4: ixmax"),
                                  ("band", (5, 0, 4, 0), 0, "band 4: up"), ("band", (5, 0, 4, 1), 256, "band 4: lo"), ("band", (5, 0, 4, 2), -1, "band 4: sf"),
                                  ("hdr", (2, 5), 256, "record 2 channel 0: G"), ("hdr", (2, 8), 2, "record 2 channel 1: scale"), ("xr", (3, 1, 17), np.nan, ": xr")])):
        R = K.records(mode, sr)
        for key, at, value, text in cases:
            a = R.pick(np.arange(8))
            if key == "band" and at[3] == 0 and mode == "isf2":
                a["band"][at[:3] + (1,)] = 1        # (up below lo)
            a[key][at] = value
            rc, out = api.debug_seek(R.T.ec, "k_alloc", mode, a["hdr"], a["xr"], a["band"], x34=a["x34"] if mode == "seek" else None,
                                     x34max=a["x34max"] if mode == "seek" else None, ix=a["ix"] if mode == "isf2" else None)
            assert rc == -1 and text in api.last_error() and not out.any(), (key, at, value, api.last_error())
    R = K.records("seek", sr)
    a = R.pick(np.arange(2))
    args = (a["hdr"], a["xr"], a["band"])
    kw = dict(x34=a["x34"], x34max=a["x34max"])
    assert api.debug_seek(R.T.ec, "k_alloc_lsf", "seek", *args, **kw)[0] == -1 and "does not run" in api.last_error()
    assert api.debug_seek(api.default_control(samprate=sr, bitrate=64, nsbstereo=8), "k_alloc1", "seek", *args, **kw)[0] == -1 and "first-generation" in api.last_error()
    assert api.debug_seek(R.T.ec, "k_alloc", "seek", *args, x34=a["x34"])[0] == -1 and "null buffer" in api.last_error()
