"""The allocator path census: which branches of the rate control, the Huffman pick and the frame driver the oracle takes on
small committed inputs, per kernel kind (tests/test_alloc_path_cases.py asserts it on the CPU, tests/test_gpu_alloc_paths.py
compares the same inputs on the GPU).  The inputs are seeds, controls and signal parameters, found by the CPU-only search
tools/alloc_path_search.py over the oracle's path counters (oracle/hxo_int.h, HXO_PATHS) and regenerated here: no PCM files.
A case whose input stops reaching an entry it claims is replaced by a new search, not relaxed.

A KIND is the kernel a stream runs on together with the variant of it the control selects:
    m1_long     k_alloc / k_alloc_slim, stereo, long blocks only (short_block_threshold 99999), no -HF
    m1_short    the same with block switching on (the short allocator and the start / stop blocks)
    m1_mono     the same kernels with one channel: no helper channel, no M/S
    m1_hf       the same kernels with -HF in force (band 21 coded)
    m2_long     k_alloc_lsf, long blocks only
    m2_short    k_alloc_lsf with block switching on
    a1_m1       k_alloc1: intensity stereo or dual channel at MPEG-1 rates (first-generation allocator)
    a1_m2       k_alloc1_lsf: the same at MPEG-2 rates
ENTRIES says which counters are accounted for in which kinds: an (entry, kind) pair of the census is either claimed by a
case of CASES or listed in UNREACHED with its reason."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from stage_taps import TapBatch

KINDS = ["m1_long", "m1_short", "m1_mono", "m1_hf", "m2_long", "m2_short", "a1_m1", "a1_m2"]
FRAMES = 10             # frames per case (at most 12): the search judges a hit by the frame it first shows at
TAIL = 2                # at least this many frames follow the frame in which a case first takes a path it claims

_P = O.PATH_NAMES
_LONG = [n for n in _P if n.startswith("L_") and n not in ("L_bt1_adjust", "L_bt3_adjust", "L_short_mnr0_cbr", "L_short_mnr0_vbr")]
_SWITCH = ["L_bt1_adjust", "L_bt3_adjust", "L_short_mnr0_cbr", "L_short_mnr0_vbr"] + [n for n in _P if n.startswith("S_")]
_A1 = [n for n in _P if n.startswith("A_")]
_HUFF = [n for n in _P if n.startswith("H_") and not n.startswith("H_tab")] + ["H_tab%d" % t for t in O.HUFF_TABLES]
_DRIVER_M1 = [n for n in _P if n.startswith("D_") and not n.startswith("D_lsf")]     # (the MPEG-2 driver is a function of its own)
_DRIVER_M2 = [n for n in _P if n.startswith("D_") and n not in ("D_scfsi_shared", "D_no_frame_out", "D_two_frames_out")]
ENTRIES = {
    "m1_long": _LONG + _HUFF + _DRIVER_M1,
    "m1_short": _SWITCH,
    "m1_mono": _LONG,
    "m1_hf": _LONG,
    "m2_long": _LONG + _HUFF + _DRIVER_M2,
    "m2_short": _SWITCH,
    "a1_m1": _A1,
    "a1_m2": _A1,
}
CENSUS = [(e, k) for k in KINDS for e in ENTRIES[k]]


def kind_of(kw):
    """the kind of a control, or None where the encoder refuses it"""
    return kind_and_features(kw)[0]


# what an entry needs of the control beyond its kind; the search must have drawn such controls (SEARCHED["features"])
FEATURES = ["hf", "cbr", "vbr", "vbr_limit", "stereo", "joint", "switching"]
NEEDS = {"L_inc_hf": "hf", "L_lim_p23_both": "stereo", "L_inc_ms": "joint", "L_dec_ms": "joint", "D_ms_frame": "joint",
         "L_fb_": "cbr", "L_short_mnr0_cbr": "cbr", "L_short_mnr0_vbr": "vbr", "D_cbr_": "cbr", "D_vbr_limit_cut": "vbr_limit",
         "D_vbr_": "vbr", "D_lsf_vbr_": "vbr", "S_": "switching", "L_bt": "switching"}


def needs(entry):
    """the feature of the control an entry cannot be reached without, or None"""
    for k in sorted(NEEDS, key=len, reverse=True):
        if entry.startswith(k):
            return NEEDS[k]
    return None


def kind_and_features(kw):
    """(kind, [features]) of a control as hxo_init resolves it (hxo_stream_kind), or (None, []) where the encoder refuses
    it.  Features: "hf" -HF in force, "cbr" / "vbr", "vbr_limit" a vbr_br_limit given, "stereo" two channels, "joint" mode 1
    (M/S allowed), "switching" short blocks allowed"""
    enc = O.OracleEncoder(O.default_control(**kw))
    if not enc.ok():
        return None, []
    v = int(O.lib().hxo_stream_kind(enc.h))
    vbr = "bitrate" not in kw and kw.get("mode") != 2
    feats = [f for f, on in (("hf", v & 8), ("cbr", not vbr), ("vbr", vbr), ("vbr_limit", vbr and "vbr_br_limit" in kw),
                             ("stereo", not v & 4), ("joint", kw.get("mode", 1) == 1),
                             ("switching", kw.get("short_block_threshold", 700) < 99999)) if on]
    return _kind(kw, v), feats


def _kind(kw, v):
    mpeg1, a1, mono, hf = v & 1, v & 2, v & 4, v & 8
    if a1:
        return "a1_m1" if mpeg1 else "a1_m2"
    switching = kw.get("short_block_threshold", 700) < 99999
    if not mpeg1:
        return "m2_short" if switching else "m2_long"
    return "m1_mono" if mono else "m1_hf" if hf else "m1_short" if switching else "m1_long"


def case_pcm(seed, sig, frames=FRAMES):
    """float32 [frames * 1152, 2] (mono: [frames * 1152]) in 16-bit units: per frame a gain on white noise and one on a tone
    (sig["gains"]: (noise, tone) as fractions of full scale, (0, 0) is silence), laid out over the channels by sig["layout"],
    times sig["scale"]; sig["fmt"] "s16" rounds and clips to 16 bits (then scale is 1)"""
    n = frames * 1152
    rng = np.random.Generator(np.random.PCG64(0xA110C + int(seed)))
    t = np.arange(n)
    gn = np.repeat(np.array([g[0] for g in sig["gains"]], dtype=np.float64)[:frames], 1152)
    gt = np.repeat(np.array([g[1] for g in sig["gains"]], dtype=np.float64)[:frames], 1152)
    tone = np.sin(2.0 * np.pi * sig["tone"] * t)
    a = gn * rng.uniform(-1.0, 1.0, n) + gt * tone
    b = gn * rng.uniform(-1.0, 1.0, n) + gt * np.sin(2.0 * np.pi * sig["tone"] * 1.31 * t + 0.7)
    lay = sig["layout"]
    x = {"independent": (a, b), "correlated": (a, 0.9 * a + 0.1 * b), "antiphase": (a, -a), "left": (a, 0.0 * a),
         "right": (0.0 * a, a), "same": (a, a)}[lay]
    x = np.stack(x, axis=1) * 32767.0
    if sig["fmt"] == "s16":
        x = np.clip(np.round(x), -32768, 32767)
    else:
        x = x * sig["scale"]
    x = x.astype(np.float32)
    return np.ascontiguousarray(x[:, 0]) if sig.get("mono") else x


def first_hits(kw, pcm, frames=FRAMES):
    """{entry: the frame at which the oracle first counts it} over one stream"""
    enc = O.OracleEncoder(O.default_control(**kw))
    assert enc.ok(), kw
    counts = np.ctypeslib.as_array((C.c_longlong * len(O.PATH_NAMES)).in_dll(O.lib(), "hxo_path_counts"))
    hit = {}
    before = counts.copy()
    for f in range(frames):
        enc.encode_f32(pcm[f * 1152:(f + 1) * 1152])
        for i in np.flatnonzero(counts != before):
            hit.setdefault(O.PATH_NAMES[i], f)
        before[:] = counts
    return hit


def claims(kind, hit, frames=FRAMES):
    """the entries of the kind's census a stream with these first hits may claim: TAIL frames follow the hit"""
    return sorted(e for e in ENTRIES[kind] if e in hit and hit[e] <= frames - 1 - TAIL)


# ---- the committed tables (tests/alloc_path_data.py, written by tools/alloc_path_search.py --emit) ----
# CASES: name -> (kind, seed, control, signal).  SEARCHED: the seed range tried and the inputs of each kind in it.
# UNREACHED: (entry, kind) -> "searched: N inputs of the kind, seeds A .. B"; where the reference's code shows a pair dead,
# DEAD below gives the proof instead ("dead: ..."), or says that the path needs more frames than a case may have ("too long: ...").
from alloc_path_data import CASES, CLAIMS, SEARCHED, UNREACHED as _SEARCHED_UNREACHED      # noqa: E402

_NO_MS = "dead: a one-channel stream is coded by encode_singleB, which hands the allocator ms_flag 0 (mp3enc.cpp:1675-1749)"
DEAD = {
    ("L_inc_ms", "m1_mono"): _NO_MS,
    ("L_dec_ms", "m1_mono"): _NO_MS,
    ("L_lim_p23_both", "m1_mono"): "dead: limit_bits tests huff_bits of nchan = 1 channels (bitallo3.cpp:2749-2773); the second never exceeds the cap",
    ("L_inc_hf", "m1_long"): "dead: the kind is the one with hf_flag 0 after init (mp3enc.cpp:326-340); with it set the stream is of kind m1_hf",
    ("L_inc_hf", "m2_long"): "dead: below 44100 Hz init clears hf_flag (mp3enc.cpp:339-340), so no MPEG-2 stream codes band 21",
    # no input of a case's length gets there, however many are tried (a case is at most 12 calls = 24 MPEG-2 frames)
    ("D_lsf_vbr_span25", "m2_long"): "too long: needs more than 24 frames pending (mp3enc.cpp:2337-2479, side_dp > 24), so 25 frames coded and "
                                     "none sent; a case of 12 calls has 24",
    ("D_lsf_vbr_span16", "m2_long"): "too long: needs more than 15 frames pending (mp3enc.cpp:2337-2479, side_dp > 15), so not before the 17th "
                                     "frame = call 9 and with no frame sent until then; two calls must follow, and a case here has 10",
}
UNREACHED = {k: DEAD.get(k, v) for k, v in _SEARCHED_UNREACHED.items()}
assert all(k in _SEARCHED_UNREACHED for k in DEAD), "a pair with a proof of deadness was reached by the search"


def batches():
    """{batch name: [case names]}: the cases of a kind, one-channel streams apart from the others (a batch's PCM has one
    shape), at most 8 streams a batch: "m2_long", "m2_long_b", "m2_long_mono", ..."""
    out = {}
    for kind in KINDS:
        for tag, mono in (("", False), ("_mono", True)):
            names = [n for n in CASES if CASES[n][0] == kind and (CASES[n][2].get("mode") == 3) == mono and not (mono and kind == "m1_mono")]
            if kind == "m1_mono" and not mono:
                names = [n for n in CASES if CASES[n][0] == kind]
            for i in range(0, len(names), 8):
                out[kind + tag + ("" if i == 0 else "_" + "bcdefgh"[i // 8 - 1])] = names[i:i + 8]
    return out


def batch_input(batch):
    """(controls, float32 PCM [S, FRAMES * 1152, 2] or [S, FRAMES * 1152]) of a batch"""
    names = batches()[batch]
    return [CASES[n][2] for n in names], np.stack([case_pcm(CASES[n][1], CASES[n][3]) for n in names])


def run_batch(api, batch, frames_per_call):
    """the batch through the C ABI in calls of frames_per_call frames, every frame compared with the oracle (tests/stage_taps.py,
    TapBatch) -> the TapBatch, closed"""
    kws, pcm = batch_input(batch)
    full = batch.startswith("m1_") and "mono" not in batch
    tb = TapBatch(api, kws, len(kws), frames_per_call, "full" if full else "lines", alloc_state=True)
    for f in range(0, FRAMES, frames_per_call):
        tb.call(pcm[:, f * 1152:(f + frames_per_call) * 1152])
    tb.close()
    assert tb.frames == [FRAMES] * len(kws) and all(len(g) > 0 for g in tb.got)
    return tb


@functools.lru_cache(maxsize=None)
def case_hits(name):
    """first_hits of a committed case, computed once per process"""
    kind, seed, kw, sig = CASES[name]
    return first_hits(kw, case_pcm(seed, sig))
