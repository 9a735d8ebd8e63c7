"""The constructed granules of tests/recon_granule_cases.py bite, shown without a GPU: the lists reach what they are there
for; an error of one part in 4096 in any single entry of any table of the decoded-PCM kernels would push some compared value
past twice its bound; a float32 restatement of the kernels' operation order stays within the bound everywhere, and eight
literal mutants of it each leave it; hx_debug_recon refuses one record per rule of its host check, before any launch.
tests/test_gpu_recon_granules.py runs the same lists through the kernels."""
import numpy as np
import pytest

import mp3_decode as D
import recon_granule_cases as R
from hmp3_amd import api

LISTS = [n for n in R.LIST_NAMES]


def all_launches():
    return [(name, i, L, ref) for name in LISTS for i, (L, ref) in enumerate(zip(R.case_list(name), R.references(name)))]


# ---- the lists reach what they say ----
def test_layouts_and_band_tables_are_the_hosts():
    lay = R.layouts()
    assert lay["sgn_words"] == 20 and lay["state"] == 1152 + 2 * 15 * 32
    for cls in ("s44", "s48", "s32"):
        c = R.CLASSES[cls]
        assert np.array_equal(np.cumsum(R.host_table("nBand_l_iso", np.int32, 22, **c["kw"])), D.SFB_LONG[c["rate"]][1:])
        assert np.array_equal(np.cumsum(R.host_table("nBand_s", np.int32, 13, **c["kw"])), D.SFB_SHORT[c["rate"]][1:])
    for name in LISTS:
        for L in R.case_list(name):
            assert L.S <= 10 and L.NG <= 16
            for s in range(L.S):
                assert all(b in R.SUCC[a] for a, b in zip(L.bt[s], L.bt[s][1:]))


def test_every_magnitude_is_reached_alone_in_its_subband():
    seen, gains = set(), set()
    for L in R.case_list("pow43"):
        assert not L.state.any() and not L.bt.any() and not L.ms.any()
        for s, g, ch in L.units():
            nz = np.flatnonzero(L.ix[s, g, ch])
            if g % 2 == 0 or g == L.NG - 1:     # the neighbours, and no case without a granule behind it
                assert not nz.size
                continue
            assert (nz % 18 == 8).all()
            seen |= set(int(v) for v in L.ix[s, g, ch, 8::18])
            gains.add(int(L.gg[s, g, ch]))
    assert seen == set(range(R.MAX_MAG + 1))
    assert {0, 255} <= gains and {(g - 210) & 3 for g in gains} == {0, 1, 2, 3} and len({(g - 210) >> 2 for g in gains}) >= 6
    signs = np.concatenate([L.sign[:, 1::2].reshape(-1) for L in R.case_list("pow43")])
    assert 0.4 < signs.mean() < 0.6


def test_every_band_of_every_rate_is_reached_at_its_first_and_last_line():
    rates = set()
    for L in R.case_list("exponent_long"):
        rate = L.rate(0)
        rates.add(rate)
        bl, combos = D.SFB_LONG[rate], set()
        for s, g, ch in L.units():
            if g == 0:
                nz = set(np.flatnonzero(L.ix[s, g, ch]))
                assert nz == {bl[b] for b in range(22)} | {bl[b + 1] - 1 for b in range(22)} and L.bt[s, g] == 0
                v = L.sfl[s, g, ch]
                kind = 0 if not v.any() else 1 if v[:21].max() == 1 else 2
                assert kind < 2 or (list(v[:11]) == [15] * 11 and list(v[11:21]) == [7] * 10 and v[21] == 0)
                combos.add((int(L.scale[s, g, ch]), int(L.pre[s, g, ch]), kind))
        assert len(combos) == 12
    assert rates == {44100, 48000, 32000}
    rates = set()
    for L in R.case_list("exponent_short"):
        rate = L.rate(0)
        rates.add(rate)
        ss, scales, gains = D.SFB_SHORT[rate], set(), set()
        for s, g, ch in L.units():
            if g == 0:
                want = set()
                for b in range(13):
                    wd = ss[b + 1] - ss[b]
                    want |= {3 * ss[b] + w * wd for w in range(3)} | {3 * ss[b] + w * wd + wd - 1 for w in range(3)}
                assert set(np.flatnonzero(L.ix[s, g, ch])) == want and L.bt[s, g] == 2
                assert len(set(L.sbg[s, g, ch])) == 3 and all(len(set(L.sfs[s, g, ch, b])) == 3 for b in range(12))
                assert L.sfs[s, g, ch, :6].max() <= 15 and L.sfs[s, g, ch, 6:].max() <= 7
                scales.add(int(L.scale[s, g, ch]))
                gains.add(tuple(L.sbg[s, g, ch]))
        assert scales == {0, 1} and gains == {(7, 0, 3), (3, 7, 0), (0, 3, 7)}
    assert rates == {44100, 48000, 32000}


def test_every_transition_stands_inside_a_frame_at_a_frame_boundary_and_across_the_carried_state():
    (L,) = R.case_list("transforms")
    inside = {(int(L.bt[s, g - 1]), int(L.bt[s, g])) for s in range(L.S) for g in range(1, L.NG, 2)}
    boundary = {(int(L.bt[s, g - 1]), int(L.bt[s, g])) for s in range(L.S) for g in range(2, L.NG, 2)}
    assert inside == boundary == set(R.TRANSITIONS) and len(R.TRANSITIONS) == 7
    (P,) = R.case_list("split")
    assert {(int(P.bt[s, P.NG // 2 - 1]), int(P.bt[s, P.NG // 2])) for s in range(P.S)} == set(R.TRANSITIONS)
    assert {P.nchan(s) for s in range(P.S)} == {1, 2}
    # one line at a time, at every position of an even and an odd subband on the long types and of every window of a short block
    seen = set()
    for s, g, ch in L.units():
        (j,) = np.flatnonzero(L.ix[s, g, ch])
        bt = int(L.bt[s, g])
        if bt == 2:
            _, w, at = R.line_maps(44100, True)
            seen.add((2, int(at[j]) // 18, int(w[j]), int(at[j]) % 6))
        else:
            seen.add((bt, j // 18, j % 18))
    for sb in R.TRANSFORM_SB:
        assert {(bt, sb, k) for bt in (0, 1, 3) for k in range(18)} | {(2, sb, w, k) for w in range(3) for k in range(6)} <= seen
    assert R.TRANSFORM_SB[0] % 2 == 0 and R.TRANSFORM_SB[1] % 2 == 1


def test_signs_ranges_kinds_and_the_rest_are_reached():
    flips = set()
    for L in R.case_list("signs"):
        for s, g, ch in L.units():
            if g == 0:
                sg = L.sign[s, g, ch]
                c = int(sg.sum() > 288)
                (j,) = np.flatnonzero(sg != c)
                flips.add((int(j), c))
                assert L.ix[s, g, ch].all()
    assert flips == {(j, c) for j in [0, 575] + [32 * k - 1 for k in range(1, 18)] + [32 * k for k in range(1, 18)] for c in (0, 1)}
    (L,) = R.case_list("coded_range")
    got = {(L.ncoded(s, 0, 0), int(L.nn[s, 0, 0])) for s in range(L.S)}
    assert {(0, 1), (2, 1), (4, 1), (574, 1), (576, 1), (0, 0)} <= got
    assert any(2 * L.bv[s, 0, 0] + 4 * L.nq[s, 0, 0] > 576 for s in range(L.S))
    for s in range(L.S):
        n = L.ncoded(s, 0, 0)
        assert (L.ix[s, 0, 0, n:] == 0x7FFF).all() and (L.ix[s, 0, 1, n:] < 0).all() and L.ix[s, 0, 0, :n].all() and L.sign[s, 0, :, n:].all()
    (L,) = R.case_list("ms")
    assert L.ms[0].all() and L.ix[0].all() and not L.ix[1, :, 1].any() and L.ms[1].all() and np.array_equal(L.ix[2, :, 0], L.ix[2, :, 1]) and L.ms[2].all()
    assert list(L.ms[3]) == [1, 0] and list(L.ms[4]) == [0, 1] and L.nchan(5) == 1 and L.ms[5].all()
    (L,) = R.case_list("alias")
    lines = {(int(L.bt[s, g]), int(j)) for s, g, ch in L.units() for j in np.flatnonzero(L.ix[s, g, ch])}
    assert lines == {(bt, 18 * sb + d) for bt in range(4) for sb in (1, 16, 31) for d in range(-8, 8)}
    lay, slots = R.layouts(), set()
    for L in R.case_list("synthesis"):
        assert not L.ix.any() and L.state[:, :lay["tail"]].all()
        for s in range(L.S):
            for ch in range(2):
                h = L.state[s, lay["tail"]:].reshape(2, 15, 32)[ch]
                ((slot, sb),) = np.argwhere(h)
                slots.add((ch, int(sb), int(slot)))
    assert {(sb, slot) for _, sb, slot in slots} == {(sb, slot) for sb in range(32) for slot in range(15)} and len(slots) == 480
    (L,) = R.case_list("counts_and_kinds")
    assert {(L.nchan(s), L.frames(s)) for s in range(L.S)} >= {(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)} and L.NG == 4
    assert R.bits(L.fill) == R.bits(R.SENTINEL) and (R.bits(L.state[1]) == R.bits(R.SENTINEL)).all()
    units = sum(len(L.units()) for L in R.case_list("random"))
    assert units >= 300
    fields = [np.concatenate([getattr(L, a).reshape(-1) for L in R.case_list("random")]) for a in ("gg", "sbg", "sfl", "sfs", "bv", "bt")]
    assert [(int(f.min()), int(f.max())) for f in fields] == [(0, 255), (0, 7), (0, 15), (0, 15), (0, 288), (0, 3)]


# ---- the float32 restatement stays within the bound, and the mutants leave it ----
def test_the_float32_restatement_of_the_kernels_stays_within_the_bound():
    worst = {}
    for name, i, L, ref in all_launches():
        r = R.check(name, i, L, ref, *R.restate(L))
        worst[name] = [max(a, b) for a, b in zip(worst.get(name, [0.0, 0.0]), r)]
    for name in LISTS:
        print("%-18s largest error / bound: hybrid tap %.3f, output %.3f" % (name, worst[name][0], worst[name][1]))
    print("all lists: hybrid tap %.3f, output %.3f" % (max(w[0] for w in worst.values()), max(w[1] for w in worst.values())))
    assert max(max(w) for w in worst.values()) <= 1.0
    # ... and the bound is no formality: the restatement's error is a fair share of it
    assert max(w[0] for w in worst.values()) > 0.05 and max(w[1] for w in worst.values()) > 0.02


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_a_literal_mutant_of_the_restatement_leaves_the_bound(mutant):
    name = R.MUTANTS[mutant]
    caught = []
    for i, (L, ref) in enumerate(zip(R.case_list(name), R.references(name))):
        try:
            R.check(name, i, L, ref, *R.restate(L, mutant))
        except AssertionError as e:
            caught.append(str(e))
    assert caught, "%s passes the whole list %s" % (mutant, name)
    print("%s: caught on list %s by %d of %d launches; the first: %s" % (mutant, name, len(caught), len(R.case_list(name)), caught[0]))


def test_the_split_list_restated_in_halves_gives_the_same_bits():
    (L,) = R.case_list("split")
    state, hyb, out = R.restate(L)
    s1, h1, o1 = R.restate(L.half(0))
    s2, h2, o2 = R.restate(L.half(1, s1))
    n = L.row // 2
    assert np.array_equal(R.bits(state), R.bits(s2)) and np.array_equal(R.bits(hyb), R.bits(np.concatenate([h1, h2], axis=1)))
    for s in range(L.S):
        m = n * L.nchan(s) // 2
        assert np.array_equal(R.bits(out[s, :2 * m]), R.bits(np.concatenate([o1[s, :m], o2[s, :m]])))


# ---- each table entry would be caught ----
PART = 2.0 ** -12       # the relative error of a single entry that must show
HALF_STEP = 1.0 - 2.0 ** -0.5       # what a pretab entry off by one takes off a line at the least (scalefac_scale 0)


def reach():
    """{table: per entry, the largest over every compared value of every list of
    |the value's float64 terms that pass through the entry| * 2^-12 / (2 * the value's bound)}"""
    T = {k: np.asarray(v, dtype=np.float64) for k, v in R.device_tables().items()}
    best = {"cos36": np.zeros((36, 18)), "cos12": np.zeros((12, 6)), "win": np.zeros((4, 36)), "cs": np.zeros(8), "ca": np.zeros(8),
            "synth": np.zeros((32, 64)), "dwin": np.zeros(512), "pow43": np.zeros(R.MAX_MAG + 1), "pow2q": np.zeros(4),
            "pretab": np.zeros((3, 21))}
    lay = R.layouts()
    H = lay["hist"]
    for name, i, L, ref in all_launches():
        parts = {}
        R.restate(L, dtype=np.float64, parts=parts)
        S, NG = L.S, L.NG
        written = np.zeros((S, NG, 2), dtype=bool)
        for s in range(S):
            written[s, :2 * L.frames(s), :L.nchan(s)] = True
        with np.errstate(divide="ignore"):
            bh = 1.0 / (2.0 * (R.gamma(R.K_HYB) * ref["hyb_mag"] + R.FLOOR_HYB)).transpose(0, 1, 2, 4, 3)     # [S][NG][2][32][18]
            bo = 1.0 / (2.0 * (R.gamma(R.K_OUT) * ref["out_mag"] + R.FLOOR_OUT))
        bh = bh * written[..., None, None]
        # a granule's 36 transform outputs land in its own 18 slots and the next granule's
        b36 = np.concatenate([bh, np.concatenate([bh[:, 1:], np.zeros_like(bh[:, :1])], axis=1)], axis=-1) * written[..., None, None] * PART
        long_, short = (L.bt != 2)[:, :, None, None, None], (L.bt == 2)[:, :, None, None, None]
        win = T["win"][L.bt][:, :, None, None, :]       # [S][NG][1][1][36]
        X, x, full = parts["alias"], parts["lines"], parts["full"]
        up = lambda a, axes: a.max(axis=axes)
        # cos36[i][k]: the term X[sb][k] cos36[i][k] win[i];  win[bt][i]: the whole windowed sum
        t = np.abs(X[..., None, :] * T["cos36"] * win[..., None]) * (b36 * long_)[..., None]
        best["cos36"] = np.maximum(best["cos36"], up(t, (0, 1, 2, 3)))
        t = np.abs(full) * b36
        for bt in range(4):
            sel = L.bt == bt
            if sel.any() and bt != 2:
                best["win"][bt] = np.maximum(best["win"][bt], up(t[sel], (0, 1, 2)))
        for w in range(3):      # cos12[j][k], win[2][j]: window w's term of output 6 + 6 w + j
            t = X[..., 6 * w:6 * w + 6][..., None, :] * T["cos12"] * T["win"][2, :12, None]        # [..][32][12][6]
            b = (b36 * short)[..., 6 + 6 * w:18 + 6 * w]
            best["cos12"] = np.maximum(best["cos12"], up(np.abs(t) * b[..., None], (0, 1, 2, 3)))
            best["win"][2, :12] = np.maximum(best["win"][2, :12], up(np.abs(t.sum(axis=-1)) * b, (0, 1, 2, 3)))
        # cs[k], ca[k]: both butterflies a subband's lines stand in (boundary sb at lines k, boundary sb + 1 at lines 17 - k)
        z = np.zeros_like(x[..., :1, :8])
        hi, lo = np.concatenate([z, x[..., 1:, :8]], axis=-2), np.concatenate([x[..., :31, :9:-1], z], axis=-2)
        prev_lo, next_hi = np.concatenate([z, x[..., :31, :9:-1]], axis=-2), np.concatenate([x[..., 1:, :8], z], axis=-2)
        c_hi, c_lo = T["cos36"][:, :8], T["cos36"][:, :9:-1]        # [36][8]: cos36[i][k], cos36[i][17 - k]
        wb = (win * b36 * long_)[..., None]
        t = T["cs"] * (hi[..., None, :] * c_hi + lo[..., None, :] * c_lo)
        best["cs"] = np.maximum(best["cs"], up(np.abs(t) * wb, (0, 1, 2, 3, 4)))
        t = T["ca"] * (prev_lo[..., None, :] * c_hi - next_hi[..., None, :] * c_lo)
        best["ca"] = np.maximum(best["ca"], up(np.abs(t) * wb, (0, 1, 2, 3, 4)))
        if name == "pow43":     # a subband's 36 outputs are the one line's: its pow43 entry and its pow2q residue
            t = up(np.abs(full) * b36, (4,))        # [S][NG][2][32]
            mags = L.ix[..., 8::18].astype(np.int64)
            np.maximum.at(best["pow43"], mags.reshape(-1), t.reshape(-1))
            res = np.broadcast_to(((L.gg - 210) & 3)[..., None], mags.shape)
            np.maximum.at(best["pow2q"], res.reshape(-1), t.reshape(-1))
        if name == "exponent_long":     # a pretab entry off by one: a band's lines under preflag, through their own subband
            bl = D.SFB_LONG[L.rate(0)]
            for b in range(21):
                for j in (bl[b], bl[b + 1] - 1):
                    sb, l = j // 18, j % 18
                    c = T["cs"][l] if (l < 8 and sb >= 1) else T["cs"][17 - l] if (l >= 10 and sb <= 30) else 1.0
                    t = np.abs(x[..., sb, l, None] * c * T["cos36"][:, l] * T["win"][0]) * b36[..., sb, :] / PART * HALF_STEP
                    t = t * (L.pre == 1)[..., None]
                    r = R.RATES.index(L.rate(0))
                    best["pretab"][r, b] = max(best["pretab"][r, b], t.max())
        # the synthesis: dwin[64 k + j] through v[t - 2 k][j], dwin[64 k + 32 + j] through v[t - 2 k - 1][32 + j]; synth[sb][n] through
        # the eight taps of its half
        M = T["synth"]      # [sb][n]
        for s in range(S):
            nf, nch = L.frames(s), L.nchan(s)
            for ch in range(nch if nf else 0):
                hist = L.state[s, lay["tail"]:].reshape(2, H, 32)[ch].astype(np.float64)
                seq = np.concatenate([hist, ref["hyb"][s, :2 * nf, ch].reshape(-1, 32)])
                nt = 36 * nf
                b = bo[s, :nt * 32 * nch].reshape(nt, 32, nch)[:, :, ch] * PART        # [t][j]
                tt = H + np.arange(nt)[:, None] - 2 * np.arange(8)[None, :]             # [t][k]
                h0, h1 = seq[tt], seq[tt - 1]                                           # [t][k][sb]
                d0, d1 = T["dwin"].reshape(8, 64)[:, :32], T["dwin"].reshape(8, 64)[:, 32:]      # [k][j]
                v0, v1 = h0 @ M[:, :32], h1 @ M[:, 32:]                                 # [t][k][j]
                best["dwin"].reshape(8, 64)[:, :32] = np.maximum(best["dwin"].reshape(8, 64)[:, :32], (np.abs(v0 * d0) * b[:, None, :]).max(axis=0))
                best["dwin"].reshape(8, 64)[:, 32:] = np.maximum(best["dwin"].reshape(8, 64)[:, 32:], (np.abs(v1 * d1) * b[:, None, :]).max(axis=0))
                c0 = np.einsum("kj,tks->tjs", d0, h0) * M[:, :32].T * b[:, :, None]     # [t][j][sb]
                c1 = np.einsum("kj,tks->tjs", d1, h1) * M[:, 32:].T * b[:, :, None]
                best["synth"][:, :32] = np.maximum(best["synth"][:, :32], np.abs(c0).max(axis=0).T)
                best["synth"][:, 32:] = np.maximum(best["synth"][:, 32:], np.abs(c1).max(axis=0).T)
    return best, T


def test_an_error_of_one_part_in_4096_in_any_table_entry_would_be_caught():
    """for each entry of pow2q, cs, ca, cos36, cos12, the four windows, the 32 x 64 matrix and the 512 taps as hx_recon_tabs
    builds them, of pow43 up to 8206 (through the pow43 list) and - off by one - of pretab: some compared value's terms through
    that entry, times 2^-12, exceed twice the value's bound.  An entry that is zero has no part in 4096: win[1][30 ..], win[2]
    [12 ..], win[3][.. 5], pow43[0], dwin[0], and column 48 of the matrix, whose closed form is cos of odd multiples of
    pi / 2 (the table holds 1e-16s there)."""
    best, T = reach()
    for name in ("pow2q", "cs", "ca", "cos36", "cos12", "win", "synth", "dwin"):
        live = np.abs(T[name]) > 1e-12
        print("%-6s %5d entries, %d zero; the least reach %.3g" % (name, live.size, (~live).sum(), best[name][live].min()))
        assert (best[name][live] > 1.0).all(), (name, np.argwhere(live & (best[name] <= 1.0))[:8], best[name][live].min())
    assert (~(np.abs(T["win"]) > 1e-12)).sum() == 6 + 24 + 6 and (~(np.abs(T["synth"]) > 1e-12)).sum() == 32 and (np.abs(T["dwin"]) > 1e-12).sum() == 511
    print("pow43  least reach %.3g; pretab %.3g" % (best["pow43"][1:].min(), best["pretab"].min()))
    assert (best["pow43"][1:] > 1.0).all(), np.flatnonzero(best["pow43"][1:] <= 1.0)[:8] + 1
    assert (best["pretab"] > 1.0).all(), np.argwhere(best["pretab"] <= 1.0)


# ---- hx_debug_recon refuses what the stream walk cannot hand over, before anything is launched ----
def small():
    L = R.Launch(["s44", "m44"], 4)
    L.set_types(0, [0, 1, 2, 3])
    L.ix[:] = 3
    return L


def rec_edit(field, value, f=0, g=0, ch=0, s=0):
    def edit(a):
        if field == "ms":
            a["rec"]["ms"][s, f] = value
        elif field == "sf":
            a["rec"]["sf"][s, f, g, ch, value[0]] = value[1]
        elif isinstance(value, tuple):
            a["rec"]["gr"][field][s, f, g, ch, value[0]] = value[1]
        else:
            a["rec"]["gr"][field][s, f, g, ch] = value
    return edit


def seg_field(j, value, g=2):
    def edit(a):
        a["seg"]["sf"][0, g, 0, j] = value
    return edit


def arr_edit(name, index, value):
    def edit(a):
        a[name][index] = value
    return edit


REFUSALS = [
    ("block_type outside", rec_edit("block_type", 4), "stream 0 granule 0 channel 0"),
    ("block_type differs", rec_edit("block_type", 0, g=1, ch=1), "stream 0 granule 1 channel 1"),
    ("cannot follow", lambda a: [rec_edit("block_type", 0, f=1, g=0, ch=c)(a) for c in (0, 1)], "stream 0 granule 2"),
    ("mixed_block_flag", rec_edit("mixed_block_flag", 1, f=1, g=1), "stream 0 granule 3 channel 0"),
    ("global_gain", rec_edit("global_gain", 256), "granule 0"),
    ("global_gain", rec_edit("global_gain", -1, s=1), "stream 1"),
    ("subblock_gain", rec_edit("subblock_gain", (2, 8)), "granule 0"),
    ("sf: a long scalefactor", rec_edit("sf", (10, 16)), "granule 0"),
    ("sf: a long scalefactor", rec_edit("sf", (11, 8)), "granule 0"),
    ("sf: a long scalefactor", rec_edit("sf", (21, 1)), "granule 0"),
    ("sf: a long scalefactor", rec_edit("sf", (3, -1)), "granule 0"),
    ("short scalefactor field above", seg_field(17, (4 << 8) | 16), "granule 2"),
    ("short scalefactor field above", seg_field(18, (4 << 8) | 8), "granule 2"),
    ("negative short scalefactor", seg_field(5, 0x8000 | (4 << 8) | 255), "granule 2"),
    ("ixq: a magnitude", arr_edit("ixq", (0, 1, 1, 575), 8207), "stream 0 granule 1 channel 1"),
    ("ixq: a magnitude", arr_edit("ixq", (1, 0, 0, 0), -1), "stream 1 granule 0 channel 0"),
    ("big_values", rec_edit("big_values", 289), "granule 0"),
    ("aux_nquads", rec_edit("aux_nquads", -1), "granule 0"),
    ("ms is neither", rec_edit("ms", 2, f=1), "stream 0 granule 2"),
    ("state: a tail", arr_edit("state", (0, 600), np.inf), "stream 0"),
    ("state: a carried slot", arr_edit("state", (1, 1152 + 5), np.nan), "stream 1"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0].split(":")[0].replace(" ", "_") + str(i) for i, r in enumerate(REFUSALS)])
def test_the_host_check_refuses_one_record_per_rule(k):
    what, edit, where = REFUSALS[k]
    L = small()
    a = R.device_arrays(L)
    edit(a)
    rc, state, hyb, out = R.debug_recon(L, **a)
    assert rc == -1 and what in api.last_error() and where in api.last_error(), api.last_error()
    assert not hyb.any() and not out.any()


def test_the_host_check_refuses_counts_rows_kinds_and_looks_at_nothing_no_kernel_reads():
    L = small()
    L.nfr = np.array([3, 0], dtype=np.int32)
    assert R.debug_recon(L)[0] == -1 and "frame count 3 out of range" in api.last_error()
    L.nfr = None
    a = R.device_arrays(L)
    assert R.debug_recon(L, out=a["out"][:, :2 * 1152 * 2 - 1])[0] == -1 and "row is shorter" in api.last_error()
    for kw, word in ((dict(samprate=22050), "class 1 (22050 Hz, mode 1) is an MPEG-2 rate"), (dict(bitrate=64, nsbstereo=8), "first-generation")):
        assert R.debug_recon(L, ecs=[api.default_control(), api.default_control(**kw)], cls=np.array([0, 0], dtype=np.int32))[0] == -1
        assert word in api.last_error(), api.last_error()
    # behind a stream's count, in a mono stream's second channel and from the coded range on anything goes: with no device
    # here the call gets as far as looking for one
    L = small()
    L.nfr = np.array([1, 2], dtype=np.int32)
    L.bv[:] = 100
    a = R.device_arrays(L)
    a["ixq"][:, :, :, 200:] = -5
    a["rec"]["gr"]["global_gain"][0, 1] = 999
    a["rec"]["gr"]["block_type"][1, :, :, 1] = 7
    a["state"][1, 576:1152] = np.nan
    rc = R.debug_recon(L, **a)[0]
    assert rc == 0 or "no HIP device" in api.last_error() or "gfx950" in api.last_error(), api.last_error()
