"""CPU side of the allocator path census (tests/alloc_path_cases.py; tests/test_gpu_alloc_paths.py compares the same inputs on
the GPU): the oracle alone runs the committed cases, and every case must reach every entry it claims with two frames to
follow; the claims and the UNREACHED table together are the whole census, and UNREACHED may hold nothing that is known to be
reachable or that too little search stands behind.  Prints the census table (python -m pytest -s)."""
import re

import pytest

import alloc_path_cases as K
from oracle import oracle as O

MPEG1 = ["m1_long", "m1_short", "m1_mono", "m1_hf"]
# pairs known to be reachable: never in UNREACHED.  At MPEG-1 and at MPEG-2 rates ...
BOTH = ["L_inc_stepback", "L_lim_max", "L_inc_cap", "L_dec_cap", "L_inc_ms", "L_inc_lr", "L_dec_ms", "L_dec_lr"]
# ... and at MPEG-1 rates alone
M1_ONLY = ["L_lim_p23_one", "L_inc_hf", "H_count1_a", "H_count1_b"] + ["H_tab%d" % t for t in O.HUFF_TABLES]
MIN_SEARCHED = 200000       # inputs of the kind behind an entry that has no proof of deadness
# ... of which at least this many with the feature of the control the entry cannot be reached without (K.NEEDS): every
# feature is one side of a choice of at most four in the tool's draw (mode 0 / 1 / 2 / 3, hf_flag 0 .. 3, CBR / VBR / VBR
# with a limit), so an even draw gives it a quarter of the kind's inputs
MIN_FEATURED = MIN_SEARCHED // 4


def claimed():
    """{(entry, kind): [cases that claim it]} from the committed claims (test_case_reaches_what_it_claims holds each case to them)"""
    out = {}
    for name, (kind, seed, kw, sig) in K.CASES.items():
        for e in K.CLAIMS[name]:
            out.setdefault((e, kind), []).append(name)
    return out


def test_counter_names_are_those_of_the_library():
    assert len(O.path_counts()) == len(O.PATH_NAMES) == len(set(O.PATH_NAMES))
    assert len(O.HUFF_TABLES) == 30


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_reaches_what_it_claims(name):
    """the committed claims of the case, counted on the oracle now: each with TAIL frames to follow its first hit"""
    kind, seed, kw, sig = K.CASES[name]
    assert K.kind_of(kw) == kind
    assert len(sig["gains"]) >= K.FRAMES and K.FRAMES <= 12
    assert K.CLAIMS[name] and set(K.CLAIMS[name]) <= set(K.ENTRIES[kind])
    got = K.claims(kind, K.case_hits(name))
    assert set(K.CLAIMS[name]) <= set(got), sorted(set(K.CLAIMS[name]) - set(got))


def test_batches_are_small():
    b = K.batches()
    assert all(len(v) <= 8 for v in b.values())
    assert {n.split("_")[0] + "_" + n.split("_")[1] for n in b} == set(K.KINDS)
    assert sorted(n for v in b.values() for n in v) == sorted(K.CASES)
    for v in b.values():
        assert len({K.CASES[n][0] for n in v}) == 1 and len({K.CASES[n][2].get("mode") == 3 for n in v}) == 1


def test_census_is_complete_and_disjoint():
    c = claimed()
    census = set(K.CENSUS)
    print("\n%-22s %s" % ("entry", " ".join("%-9s" % k for k in K.KINDS)))
    for e in O.PATH_NAMES:
        if any((e, k) in census for k in K.KINDS):
            cell = lambda k: "-" if (e, k) not in census else c[(e, k)][0][len(k) + 1:] if (e, k) in c else "UNREACHED"
            print("%-22s %s" % (e, " ".join("%-9s" % cell(k) for k in K.KINDS)))
    for key, why in K.UNREACHED.items():
        print("UNREACHED %-22s %-9s %s" % (key + (why,)))
    assert set(c) <= census
    assert set(K.UNREACHED) <= census
    assert not set(c) & set(K.UNREACHED), sorted(set(c) & set(K.UNREACHED))
    assert set(c) | set(K.UNREACHED) == census, sorted(census - set(c) - set(K.UNREACHED))


def test_unreached_hides_no_known_path():
    m1 = [k for k in MPEG1 if k != "m1_short"]
    for e in BOTH:
        assert not any((e, k) in K.UNREACHED for k in ("m1_long", "m2_long")), e
    for e in M1_ONLY:
        assert (e, "m1_long") not in K.UNREACHED or any((e, k) in claimed() for k in m1), e
    assert ("L_inc_hf", "m1_hf") not in K.UNREACHED
    assert ("L_inc_hf", "m1_mono") not in K.UNREACHED      # -HF stays in force on one channel (mp3enc.cpp:326-340 clears it for mode 2 only)


def test_unreached_has_a_proof_or_the_search_behind_it():
    """An UNREACHED pair carries a proof from the reference's code or at least MIN_SEARCHED inputs of its kind (the tables'
    own count of the inputs tried: tools/alloc_path_search.py --extend searches on behind the pairs that have too few)"""
    for (e, kind), why in K.UNREACHED.items():
        if why.startswith("dead: ") or why.startswith("too long: "):
            assert re.search(r"\w+\.(cpp|c|h):\d+", why), (e, kind, why)      # the reference's file and lines
            continue
        m = re.match(r"searched: (\d+) inputs of the kind, seeds (\d+) \.\. (\d+)( and \d+ \.\. \d+)*$", why)
        assert m, (e, kind, why)
        assert int(m.group(1)) == K.SEARCHED["inputs"][kind]
        assert int(m.group(1)) >= MIN_SEARCHED, (e, kind, why)
        need = K.needs(e)
        if need is not None:        # ... and the search drew controls that can take the path at all
            assert K.SEARCHED["features"][kind].get(need, 0) >= MIN_FEATURED, (e, kind, need, K.SEARCHED["features"][kind])


def test_every_kind_was_searched_with_every_feature_it_admits():
    """the draw leaves no combination out: -HF on one channel, VBR with short blocks at MPEG-2 rates, ..."""
    f = K.SEARCHED["features"]
    assert f["m1_mono"].get("hf", 0) > 0 and f["m1_hf"].get("switching", 0) > 0 and f["m1_mono"].get("switching", 0) > 0
    for kind in ("m1_long", "m1_short", "m1_mono", "m1_hf", "m2_long", "m2_short"):
        assert all(f[kind].get(x, 0) > 0 for x in ("cbr", "vbr", "vbr_limit")), (kind, f[kind])
    for kind in ("m1_long", "m1_short", "m1_hf", "m2_long", "m2_short"):
        assert f[kind].get("joint", 0) > 0 and f[kind]["stereo"] > f[kind]["joint"], (kind, f[kind])
