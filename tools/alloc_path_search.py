#!/usr/bin/env python3
"""CPU-only random search for inputs that reach the entries of the allocator path census (tests/alloc_path_cases.py) on the
oracle: random controls and small random signals from a fixed seed range, one process per usable CPU.  For every
(entry, kind) of the census it prints the number of inputs that reach it and the first seeds that do; --emit writes
tests/alloc_path_data.py: a greedy cover of the census by cases, the UNREACHED table with the effort spent, and the counts.

A hit is minimised by construction: every input is FRAMES (10) frames long and an entry counts as reached only where its
first hit leaves TAIL (2) frames after it, so the state the path leaves behind is part of what a case compares.

    python tools/alloc_path_search.py --seeds 0 600000 --emit       (not a test; never run on the GPU machine)
    python tools/alloc_path_search.py --extend --need 200000        more inputs of the kinds that still have unreached pairs
    python tools/alloc_path_search.py --more 10000000 10700000      a range of the free draw (draw_free), merged into the tables
    python tools/alloc_path_search.py --features                    recount SEARCHED's features and the cases' CLAIMS

Every input is 10 frames; hits are not shortened further (a batch may have 12)."""
import argparse
import concurrent.futures
import multiprocessing as mp
import os
import pickle
import pprint
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np      # noqa: E402

KEEP = 6                # seeds kept per (entry, kind), with everything else those inputs reach
BR_M1 = [24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160]                 # per channel, stereo: twice a legal total
BR_M1_MONO = [32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BR_M2 = [8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80]
BR_M2_MONO = [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
LEVELS = [0.0, 0.0, 0.001, 0.01, 0.05, 0.2, 0.5, 1.0, 1.0]
# what a seed draws first: the family of controls (so that every kind gets its share of the inputs)
FAMILIES = ["m1_long", "m1_short", "m1_mono", "m1_hf", "m2_long", "m2_short", "a1_m1", "a1_m2"]


FREE = 10000000          # seeds from here on draw every field of the control on its own (draw_free)


def draw_signal(r, pick, mono):
    gains = []
    g = (pick(LEVELS), pick(LEVELS))
    for _ in range(12):
        if r.random() < 0.45:
            g = (pick(LEVELS), pick(LEVELS))
        gains.append(g)
    fmt = pick(["s16", "s16", "f32"])
    sig = dict(gains=gains, tone=float(pick([0.0025, 0.01, 0.037, 0.11, 0.23, 0.41])),
               layout=pick(["independent", "correlated", "antiphase", "left", "right", "same"]),
               fmt=fmt, scale=1.0 if fmt == "s16" else float(pick([1.0 / 16, 1.0, 16.0, 4096.0])))
    if mono:
        sig["mono"] = True
    return sig


def draw_free(seed):
    """(control, signal) of a seed >= FREE: sample rate, mode, nsbstereo, CBR / VBR / vbr_br_limit, hf_flag + freq_limit and
    short_block_threshold each drawn on its own, whatever the others are (so -HF meets mono, VBR meets short blocks at every
    rate, ...); MPEG-1 rates and -HF get the larger share, being where the kinds with unreached pairs are"""
    r = np.random.Generator(np.random.PCG64(0x5EA7C4 + int(seed)))
    pick = lambda seq: seq[int(r.integers(len(seq)))]
    kw = dict(samprate=pick([44100, 48000, 44100, 48000, 32000, 22050, 24000, 16000]), mode=pick([0, 1, 1, 3, 3, 2]))
    mpeg1, mono = kw["samprate"] >= 32000, kw["mode"] == 3
    if kw["mode"] == 1 and r.random() < 0.2:
        kw["nsbstereo"] = pick([4, 8, 12, 16])
    if r.random() < 0.6:
        kw.update(hf_flag=pick([1, 2, 3]), freq_limit=pick([16000, 19000, 21000, 24000]))
    if kw["mode"] == 2 or r.random() < 0.6:
        kw["bitrate"] = pick((BR_M1_MONO if mono else BR_M1) if mpeg1 else (BR_M2_MONO if mono else BR_M2))
    else:
        kw["vbr_mnr"] = pick([0, 20, 50, 80, 100, 120, 150])
        if r.random() < 0.5:
            kw["vbr_br_limit"] = pick([32, 48, 64, 96, 128, 160] if mpeg1 else [8, 16, 24, 32, 48, 80])
    t = pick([0, 700, 99999, 99999])
    if t != 700:
        kw["short_block_threshold"] = t
    return kw, draw_signal(r, pick, mono)


def draw(seed):
    """(control, signal) of a seed; seeds below FREE (the family draw; from FREE on see draw_free): every sample rate, CBR / VBR / vbr_br_limit, modes 0 .. 3, nsbstereo, -HF with a
    frequency limit, short_block_threshold 0 / default / 99999; per-frame gains on noise, tone and silence, correlated /
    anti-phase / hard-panned channels, 16-bit and float scales up to 4096 x full scale"""
    if seed >= FREE:
        return draw_free(seed)
    r = np.random.Generator(np.random.PCG64(0x5EA7C4 + int(seed)))
    pick = lambda seq: seq[int(r.integers(len(seq)))]
    fam = FAMILIES[int(seed) % len(FAMILIES)]
    mpeg1 = fam.startswith("m1") or fam == "a1_m1"
    kw = dict(samprate=pick([44100, 48000, 32000] if mpeg1 else [22050, 24000, 16000]))
    if fam.startswith("a1"):
        kw["mode"] = pick([1, 2])
        if kw["mode"] == 1:
            kw["nsbstereo"] = pick([4, 8, 12, 16])
    elif fam == "m1_mono":
        kw["mode"] = 3
    elif fam == "m1_hf":
        kw.update(mode=pick([0, 1]), samprate=pick([44100, 48000]), hf_flag=pick([1, 2, 3]), freq_limit=pick([16000, 19000, 21000, 24000]))
    else:
        kw["mode"] = pick([0, 1, 1, 3]) if fam.startswith("m2") else pick([0, 1, 1])
    mono = kw["mode"] == 3
    cbr = fam.startswith("a1") or r.random() < 0.6
    if cbr:
        kw["bitrate"] = pick((BR_M1_MONO if mono else BR_M1) if mpeg1 else (BR_M2_MONO if mono else BR_M2))
        if fam == "m1_hf":
            kw["bitrate"] = pick([96, 112, 128, 160])
    else:
        kw["vbr_mnr"] = pick([0, 20, 50, 80, 100, 120, 150]) if fam != "m1_hf" else pick([80, 100, 120, 150])
        if r.random() < 0.5:
            kw["vbr_br_limit"] = pick([32, 48, 64, 96, 128, 160] if mpeg1 else [8, 16, 24, 32, 48, 80])
    if fam in ("m1_long", "m2_long") or (fam in ("m1_mono", "m1_hf") and r.random() < 0.7):
        kw["short_block_threshold"] = 99999
    elif fam in ("m1_short", "m2_short") and r.random() < 0.4:
        kw["short_block_threshold"] = 0
    gains = []
    g = (pick(LEVELS), pick(LEVELS))
    for _ in range(12):
        if r.random() < 0.45:
            g = (pick(LEVELS), pick(LEVELS))
        gains.append(g)
    fmt = pick(["s16", "s16", "f32"])
    sig = dict(gains=gains, tone=float(pick([0.0025, 0.01, 0.037, 0.11, 0.23, 0.41])),
               layout=pick(["independent", "correlated", "antiphase", "left", "right", "same"]),
               fmt=fmt, scale=1.0 if fmt == "s16" else float(pick([1.0 / 16, 1.0, 16.0, 4096.0])))
    if mono:
        sig["mono"] = True
    return kw, sig


def _one(K, seed, dry=False):
    """(kind, entries claimed) of a seed, run in a forked child: an input on which the oracle's own assertions end the process
    (the reference would write past its buffers there) is reported as aborted, not searched"""
    kw, sig = draw(seed)
    kind, feats = K.kind_and_features(kw)
    if kind is None:
        return None, [], []
    if dry:
        return kind, [], feats
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.close(r)
        devnull = os.open(os.devnull, os.O_WRONLY)
        os.dup2(devnull, 2)
        got = K.claims(kind, K.first_hits(kw, K.case_pcm(seed, sig)))
        os.write(w, pickle.dumps(got))
        os._exit(0)
    os.close(w)
    data = b""
    while True:
        blk = os.read(r, 65536)
        if not blk:
            break
        data += blk
    os.close(r)
    _, status = os.waitpid(pid, 0)
    if status != 0:
        return "aborted", [], []
    return kind, pickle.loads(data), feats


def _chunk(job):
    """-> (first seed, tried, count, keep); tried counts inputs per kind and, as "kind:feature", those with a feature"""
    import alloc_path_cases as K
    seeds, dry = job
    tried = {k: 0 for k in K.KINDS + ["aborted"]}
    count, keep = {}, {}
    for seed in seeds:
        kind, got, feats = _one(K, seed, dry)
        if kind is None:
            continue
        tried[kind] += 1
        for f in feats:
            tried[kind + ":" + f] = tried.get(kind + ":" + f, 0) + 1
        if kind == "aborted":
            keep.setdefault(("aborted", "aborted"), []).append((seed, []))
        for e in got:
            key = (e, kind)
            count[key] = count.get(key, 0) + 1
            if len(keep.setdefault(key, [])) < KEEP:
                keep[key].append((seed, got))
    return seeds[0], tried, count, keep


def search(ranges, procs, step=500, dry=False):
    """ranges: range objects of seeds (picklable), searched in chunks of `step` seeds; dry: draw and classify only"""
    import alloc_path_cases as K
    tried = {k: 0 for k in K.KINDS + ["aborted"]}
    count, keep = {}, {}
    jobs = [(r[a:a + step], dry) for r in ranges for a in range(0, len(r), step)]
    t0 = time.time()
    # (an executor, not a Pool: a worker that dies ends the search with BrokenProcessPool instead of hanging it)
    with concurrent.futures.ProcessPoolExecutor(procs, mp_context=mp.get_context("spawn")) as pool:
        for _, tr, cn, kp in sorted(pool.map(_chunk, jobs)):
            for k, v in tr.items():
                tried[k] = tried.get(k, 0) + v
            for k, v in cn.items():
                count[k] = count.get(k, 0) + v
            for k, v in kp.items():
                keep[k] = sorted(keep.get(k, []) + v)[:None if k[0] == "aborted" else KEEP]
    print("searched %d seeds in %.0f s on %d processes" % (sum(len(r) for r in ranges), time.time() - t0, procs))
    return tried, count, keep


def cover(K, keep, pairs=None, first=None):
    """greedy: per kind, the kept seeds that claim the most entries not yet claimed (pairs: only these (entry, kind) pairs;
    first: per kind the number the first new case takes)"""
    cases = {}
    for kind in K.KINDS:
        want = {e for e in K.ENTRIES[kind] if (e, kind) in keep and (pairs is None or (e, kind) in pairs)}
        cand = {}
        for e in want:
            for seed, got in keep[(e, kind)]:
                cand[seed] = set(got)
        i = 0 if first is None else first[kind]
        while want:
            seed = max(sorted(cand), key=lambda s: len(cand[s] & want))
            assert cand[seed] & want
            want -= cand[seed]
            kw, sig = draw(seed)
            cases["%s_%02d" % (kind, i)] = (kind, seed, kw, sig)
            i += 1
    return cases


def write_tables(K, path, how, cases, unreached, searched, count):
    with open(path, "w") as f:
        f.write('"""The tables of tests/alloc_path_cases.py, written by tools/alloc_path_search.py %s; the DEAD table of\n'
                'alloc_path_cases.py replaces a "searched" reason by a proof where there is one."""\n' % how)
        f.write("CASES = " + pprint.pformat(cases, width=150, sort_dicts=False) + "\n\n")
        claims = {n: K.claims(c[0], K.first_hits(c[2], K.case_pcm(c[1], c[3]))) for n, c in cases.items()}
        f.write("# what each case reaches with %d frames to follow, on the oracle, when the tables were written\nCLAIMS = " % K.TAIL
                + pprint.pformat(claims, width=150, sort_dicts=False) + "\n\n")
        f.write("UNREACHED = " + pprint.pformat(unreached, width=150, sort_dicts=False) + "\n\n")
        f.write("SEARCHED = " + pprint.pformat(searched, width=150, sort_dicts=False) + "\n\n")
        f.write("# inputs of the search that reach each pair (with %d frames after the hit)\nCOUNTS = " % K.TAIL
                + pprint.pformat({k: count[k] for k in K.CENSUS if k in count}, width=150, sort_dicts=False) + "\n")
    print("wrote %d cases, %d unreached pairs" % (len(cases), len(unreached)))


def extend(K, a, procs):
    """More search behind the pairs the committed tables leave unreached without a proof: past the seed range already
    searched, only the seeds of those pairs' kinds are drawn (seed % 8 picks the family), as many as bring the kind to
    --need inputs at the share of its seeds the encoder accepted so far.  The committed cases stay; a pair reached now
    gets a new case."""
    import alloc_path_data as D
    lo = D.SEARCHED["seeds"][1]
    tried = dict(D.SEARCHED["inputs"])
    kinds = sorted({k for (e, k), why in K.UNREACHED.items() if why.startswith("searched")}, key=K.KINDS.index)
    ranges, last = [], {}
    ext = {k: list(v) for k, v in D.SEARCHED.get("extended", {}).items()}      # kind: [first, last, step] of earlier extensions
    for k in kinds:
        fam = FAMILIES.index(k)
        first = ext[k][1] + 8 if k in ext else lo + (fam - lo) % 8
        drawn = lo / 8.0 + (first - lo) / 8.0                                   # seeds of the family drawn so far
        n = int((a.need - tried[k]) / (tried[k] / drawn) * 1.05) + 1 if tried[k] < a.need else 0
        if n > 0:
            ranges.append(range(first, first + 8 * n, 8))
            ext[k] = [ext[k][0] if k in ext else first, ranges[-1][-1], 8]
        if k in ext:
            last[k] = ext[k][1]
    merge(K, a, D, ranges, procs, dict(extended=ext))


def reason(searched, kind):
    r = "searched: %d inputs of the kind, seeds %d .. %d" % (searched["inputs"][kind], searched["seeds"][0],
                                                             searched.get("extended", {}).get(kind, [0, searched["seeds"][1] - 1])[1])
    return r + "".join(" and %d .. %d" % (lo, hi - 1) for lo, hi in searched.get("free", []))


def merge(K, a, D, ranges, procs, update):
    """search `ranges` and merge into the committed tables D: counts add up, the cases stay, a pair reached for the first
    time gets a new case; `update` goes into SEARCHED"""
    tr, cn, keep = search(ranges, procs)
    print("inputs per kind in this search:", {k: v for k, v in tr.items() if ":" not in k})
    print("inputs that end the oracle by one of its assertions (not searched):", [s for s, _ in keep.pop(("aborted", "aborted"), [])])
    searched = dict(D.SEARCHED)
    searched.update(update)
    searched["inputs"] = {k: D.SEARCHED["inputs"].get(k, 0) + tr.get(k, 0) for k in list(D.SEARCHED["inputs"]) + [k for k in tr if ":" not in k and k not in D.SEARCHED["inputs"]]}
    feats = {k: dict(v) for k, v in D.SEARCHED.get("features", {}).items()}
    for k, v in tr.items():
        if ":" in k:
            kind, f = k.split(":")
            feats.setdefault(kind, {})[f] = feats.get(kind, {}).get(f, 0) + v
    searched["features"] = feats
    census = set(K.CENSUS)
    count = dict(D.COUNTS)
    fresh = {key for key in cn if key not in count and key in census}
    for key, v in cn.items():
        if key in census:
            count[key] = count.get(key, 0) + v
    print("pairs reached now that were not:", sorted(fresh))
    cases = dict(D.CASES)
    cases.update(cover(K, keep, fresh, {k: sum(1 for c in D.CASES.values() if c[0] == k) for k in K.KINDS}))
    unreached = {(e, k): reason(searched, k) for e, k in K.CENSUS if (e, k) not in count}
    write_tables(K, a.out, "(--seeds A B --emit, then --extend and --more: the ranges are in SEARCHED)", cases, unreached, searched, count)


def features_only(K, a, procs):
    """fill SEARCHED["features"] for the ranges already searched: draws and classifies every seed again, runs no input"""
    import alloc_path_data as D
    S = D.SEARCHED
    ranges = [range(*S["seeds"])] + [range(f, l + 1, st) for f, l, st in S.get("extended", {}).values()] + [range(lo, hi) for lo, hi in S.get("free", [])]
    tr, _, _ = search(ranges, procs, dry=True)
    for k in K.KINDS:
        assert tr[k] + (0 if k else 0) >= 0
    feats = {}
    for k, v in tr.items():
        if ":" in k:
            kind, f = k.split(":")
            feats.setdefault(kind, {})[f] = v
    print("inputs per kind as classified again:", {k: v for k, v in tr.items() if ":" not in k})
    searched = dict(S, features=feats)
    write_tables(K, a.out, "(--seeds A B --emit, then --extend and --more: the ranges are in SEARCHED)", D.CASES, D.UNREACHED, searched, D.COUNTS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", nargs=2, type=int, default=[0, 40000])
    ap.add_argument("--procs", type=int, default=0)
    ap.add_argument("--emit", action="store_true", help="write tests/alloc_path_data.py")
    ap.add_argument("--extend", action="store_true", help="search on behind the unreached pairs of tests/alloc_path_data.py and rewrite it")
    ap.add_argument("--more", nargs=2, type=int, help="search a range of free-draw seeds (>= 10000000) and merge it into the tables")
    ap.add_argument("--features", action="store_true", help="recount SEARCHED's features over the ranges already searched")
    ap.add_argument("--need", type=int, default=200000, help="--extend: inputs of a kind to reach")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "alloc_path_data.py"), help="where --emit / --extend write")
    a = ap.parse_args()
    import alloc_path_cases as K
    from oracle_pool import usable_cpus
    if a.extend:
        return extend(K, a, a.procs or usable_cpus())
    if a.features:
        return features_only(K, a, a.procs or usable_cpus())
    if a.more:
        import alloc_path_data as D
        assert a.more[0] >= FREE
        return merge(K, a, D, [range(*a.more)], a.procs or usable_cpus(), dict(free=D.SEARCHED.get("free", []) + [list(a.more)]))
    tried, count, keep = search([range(a.seeds[0], a.seeds[1])], a.procs or usable_cpus())
    print("inputs per kind:", tried)
    print("inputs that end the oracle by one of its assertions (not searched):", [s for s, _ in keep.pop(("aborted", "aborted"), [])])
    for e, kind in K.CENSUS:
        n = count.get((e, kind), 0)
        print("%-22s %-9s %7d  %s" % (e, kind, n, [s for s, _ in keep.get((e, kind), [])][:KEEP]))
    if a.emit:
        unreached = {(e, k): "searched: %d inputs of the kind, seeds %d .. %d" % (tried[k], a.seeds[0], a.seeds[1] - 1)
                     for e, k in K.CENSUS if (e, k) not in count}
        write_tables(K, a.out, "--seeds %d %d --emit" % tuple(a.seeds), cover(K, keep), unreached,
                     dict(seeds=list(a.seeds), inputs=tried), count)


if __name__ == "__main__":
    main()
