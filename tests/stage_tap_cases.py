"""The cases of tests/test_gpu_stage_taps.py: configurations, shapes, call plans and inputs, and what the oracle alone says
about them (block types, call-boundary transitions, branches of the pre-echo clamp).  The seeds and burst positions below
were picked by a CPU-only search over the oracle (random positions, judged by trace() below) so that the cases reach the
branches tests/test_stage_tap_cases.py asserts; a case whose inputs stop reaching one is replaced, not relaxed."""
import functools

import numpy as np

from hmp3_amd import synth
from oracle import oracle as O
from stage_taps import preecho_branches

RHOS = [0.7, 0.0, 1.0, 0.3]

CONFIGS = {     # name: (control, what the oracle taps on that path - TapBatch's `taps`)
    "vbr50_sw": (dict(), "full"),
    "cbr128_lr_sw": (dict(bitrate=64, mode=0), "full"),
    "mono_vbr50": (dict(mode=3), "lines"),
    "lsf_cbr64_22k": (dict(bitrate=32, samprate=22050), "lines"),
    "lsf_mono_vbr_16k": (dict(samprate=16000, mode=3), "lines"),
    "thr0_all_short": (dict(short_block_threshold=0), "full"),
    "thr100_mostly_short": (dict(short_block_threshold=100), "full"),
    "a1_intensity": (dict(bitrate=64, nsbstereo=8), "lines"),
    "a1_dual_lsf": (dict(bitrate=32, samprate=22050, mode=2), "lines"),
    "hf_48k_sw": (dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000), "full"),
}

# per-stream frame counts of the uneven calls (S = 6, at most 3 frames a call), cycled until every stream has its frames
UNEVEN = [[3, 0, 1, 2, 0, 3], [1, 2, 3, 0, 3, 1], [0, 3, 2, 1, 2, 0], [2, 1, 0, 3, 1, 2]]

# name: (configuration, S, frames per stream, plan, first seed, per stream the sample positions of its noise bursts)
#   plan "frames": calls of one frame; "one": one call; "counts": the UNEVEN table
CASES = {
    "frame_by_frame_vbr50_sw": ("vbr50_sw", 5, 24, "frames", 4100,
        [(23041,), (13614, 21187), (6917, 9545), (8068, 10290, 20199), (7811,)]),
    "frame_by_frame_cbr128_lr_sw": ("cbr128_lr_sw", 5, 24, "frames", 4200,
        [(3420, 5803, 19117), (5064, 6929), (8330,), (11145,), (11327, 16246)]),
    "frame_by_frame_mono_vbr50": ("mono_vbr50", 5, 24, "frames", 4300,
        [(5563, 8045), (4667,), (14481, 22382, 23020), (2539, 4780), (18525, 21769, 22462)]),
    "frame_by_frame_lsf_cbr64_22k": ("lsf_cbr64_22k", 5, 24, "frames", 4400,
        [(15431, 17252), (2461, 12178, 13012), (2533, 19119, 19924), (6107, 24188), (23847,)]),
    "frame_by_frame_lsf_mono_vbr_16k": ("lsf_mono_vbr_16k", 5, 24, "frames", 4500,
        [(2376, 4874, 16657), (6612, 9335), (12615, 18189, 20978), (14099,), (18930,)]),
    "one_call_vbr50_sw": ("vbr50_sw", 3, 23, "one", 4600,
        [(6329, 8524), (6089, 8585, 7368), (9046, 18362)]),
    "one_call_cbr128_lr_sw": ("cbr128_lr_sw", 3, 23, "one", 4700,
        [(11719, 14222, 16211), (14622,), (14519,)]),
    "one_call_mono_vbr50": ("mono_vbr50", 3, 23, "one", 4800,
        [(11982,), (8800, 11544), (6498, 9402)]),
    "one_call_lsf_cbr64_22k": ("lsf_cbr64_22k", 3, 23, "one", 4900,
        [(4343, 8552, 21631), (5237,), (10452,)]),
    "one_call_lsf_mono_vbr_16k": ("lsf_mono_vbr_16k", 3, 23, "one", 5000,
        [(11031, 14100, 17480), (8798, 11842), (15857, 17923)]),
    "uneven_counts_vbr50_sw": ("vbr50_sw", 6, 12, "counts", 5100,
        [(8163,), (8849,), (9529,), (9475,), (6579, 9940), (8322,)]),
    "thr0_all_short": ("thr0_all_short", 3, 8, "frames", 5200,
        [(), (), ()]),
    "thr100_mostly_short": ("thr100_mostly_short", 3, 8, "frames", 5300,
        [(5661,), (4376,), (3128, 4867)]),
    "a1_intensity": ("a1_intensity", 2, 12, "one", 5400,
        [(7643,), (9783,)]),
    "a1_dual_lsf": ("a1_dual_lsf", 2, 12, "one", 5500,
        [(4959,), (2948,)]),
    "hf_48k_sw": ("hf_48k_sw", 3, 12, "one", 5600,
        [(3332,), (4647,), (9700, 11324)]),
}

# the legal block-type transitions (previous granule's type, this granule's): all of them must be met at call boundaries
TRANSITIONS = {(0, 0), (0, 1), (1, 2), (2, 2), (2, 3), (3, 0), (3, 1)}


def control(name):
    return CONFIGS[CASES[name][0]][0]


def taps(name):
    return CONFIGS[CASES[name][0]][1]


def stream_pcm(seed, nframes, sr, rho, bursts):
    """int16 [nframes * 1152, 2]: synth.stream_pcm at 0.6 full scale plus a decaying white burst (2000 samples, both
    channels, independent) at every sample position of `bursts`"""
    x = synth.stream_pcm(seed, nframes, sr=sr, rho=rho, bursts=False).astype(np.float64) * (0.6 / 32767.0)
    rng = np.random.Generator(np.random.PCG64(0x5A17 + 7919 * int(seed)))
    env = np.exp(-np.arange(2000) / 200.0)
    for p in bursts:
        n = min(2000, x.shape[0] - p)
        x[p:p + n] += 0.35 * env[:n, None] * rng.standard_normal((n, 2))
    return np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)


def case_pcm(name, bursts=None):
    """the case's input: int16 [S, F * 1152, 2], or [S, F * 1152] for a mono configuration"""
    cfg, S, F, _, seed0, pos = CASES[name]
    kw = CONFIGS[cfg][0]
    pos = pos if bursts is None else bursts
    pcm = np.stack([stream_pcm(seed0 + i, F, kw.get("samprate", 44100), RHOS[i % 4], pos[i]) for i in range(S)])
    return pcm[:, :, 0].copy() if kw.get("mode") == 3 else pcm


def plan(name):
    """the calls of the case: a list of per-stream frame counts"""
    _, S, F, how, _, _ = CASES[name]
    if how == "frames":
        return [[1] * S for _ in range(F)]
    if how == "one":
        return [[F] * S]
    done, calls = [0] * S, []
    while min(done) < F:
        row = [min(n, F - d) for n, d in zip(UNEVEN[len(calls) % len(UNEVEN)], done)]
        if max(row) > 0:
            calls.append(row)
        else:       # (every stream the row serves is through: serve the others)
            calls.append([min(1, F - d) for d in done])
        done = [d + n for d, n in zip(done, calls[-1])]
    return calls


def trace(name, pcm=None):
    """What the oracle alone says about the case: bt [S][2 F] block types; boundaries, the (type before, type after) pairs at
    the calls' starts; short [S] short granules per stream; and over the long granules that follow a long one and are no
    stop block: taken / floor, how many have the pre-echo clamp taken / held by the 0.1 * thr floor in some partition, and
    first_taken, those with the clamp taken that are a call's first granule."""
    cfg, S, F, _, _, _ = CASES[name]
    kw = CONFIGS[cfg][0]
    pcm = case_pcm(name) if pcm is None else pcm
    nch = 1 if kw.get("mode") == 3 else 2
    starts = [set() for _ in range(S)]      # frames of a stream at which a call begins
    done = [0] * S
    for row in plan(name):
        for s, n in enumerate(row):
            if n:
                starts[s].add(done[s])
                done[s] += n
    assert done == [F] * S
    out = dict(bt=[], boundaries=set(), short=[], taken=0, floor=0, first_taken=0)
    for s in range(S):
        enc = O.OracleEncoder(O.default_control(**kw))
        d = O.oracle_enable_debug(enc)
        bts, last = [], None
        for f in range(F):
            enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152])
            ot = np.array(d.thr).reshape(2, 2, 64)[:, :nch]
            for igr in range(2):
                bt = int(d.block_type[igr])
                if igr == 0 and f in starts[s] and f > 0:
                    out["boundaries"].add((bts[-1], bt))
                if bt == 2:
                    last = None
                else:
                    if bt != 3 and last is not None:
                        tk, fl = preecho_branches(ot[igr], np.float32(2.0) * last)
                        out["taken"] += tk > 0
                        out["floor"] += fl > 0
                        out["first_taken"] += tk > 0 and igr == 0 and f in starts[s]
                    last = ot[igr].copy()
                bts.append(bt)
        out["bt"].append(bts)
        out["short"].append(bts.count(2))
    return out


@functools.lru_cache(maxsize=None)
def case_trace(name):
    """trace() of the committed inputs, computed once per process"""
    return trace(name)
