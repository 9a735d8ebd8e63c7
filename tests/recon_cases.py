"""The inputs of the decoded-PCM tests: CPU_CASES, on which tests/test_recon_cases.py pins the decoder of tests/mp3_decode.py
against the oracle, and GPU_CASES, whose batches tests/test_gpu_recon.py compares with that decoder.

The CPU cases start from inputs the other suites already drive the allocator into its corners with (tests/stage_tap_cases.py,
tests/alloc_path_cases.py): what each reaches of the decoder - block types, M/S switching, scfsi, scalefac_scale, preflag,
subblock_gain, both count1 tables, linbits, an all-zero granule, mono - is asserted from the parsed side information by
the test, per case in REACHES; a case whose input stops reaching an entry is replaced, not relaxed."""
import functools

import numpy as np

from hmp3_amd import synth
from oracle import oracle as O

DRAIN_CAP = 40          # zero blocks fed behind the signal, at the most, until every signal frame is out
SNR_CASE = "cbr128_tones"


def _stage(name, stream):
    import stage_tap_cases as ST
    return dict(ST.control(name)), ST.case_pcm(name)[stream]


def _path(name):
    import alloc_path_cases as AP
    _, seed, kw, sig = AP.CASES[name]
    return dict(kw), AP.case_pcm(seed, sig)


# name: () -> (control, PCM of one stream: int16 or float32 at int16 scale, [n * 1152, 2] or [n * 1152] for mono)
CPU_CASES = {
    "cbr128_tones": lambda: (dict(bitrate=64), synth.stream_pcm(0, 10, rho=0.5)),
    "vbr50_switching_ms": lambda: _stage("frame_by_frame_vbr50_sw", 1),
    "hf_preflag_subblock_gain": lambda: _path("m1_hf_02"),
    "hf_48k_switching": lambda: _stage("hf_48k_sw", 1),
    "mono_vbr50_switching": lambda: _stage("one_call_mono_vbr50", 1),
    "mono_preflag": lambda: _path("m1_mono_02"),
    "mono_32k_cbr64": lambda: (dict(bitrate=64, samprate=32000, mode=3), synth.stream_pcm(3, 6, sr=32000)[:, 0].copy()),
    "silence": lambda: (dict(), np.zeros((4 * 1152, 2), np.int16)),
}
# what the parsed side information of each case's signal frames must show (features() below)
REACHES = {
    "cbr128_tones": {"bt0", "count1_a", "count1_b", "linbits", "scfsi"},
    "vbr50_switching_ms": {"bt0", "bt1", "bt2", "bt3", "ms_both_ways", "scfsi", "scalefac_scale", "subblock_gain", "count1_a", "count1_b", "linbits"},
    "hf_preflag_subblock_gain": {"bt0", "bt1", "bt2", "bt3", "preflag", "scalefac_scale", "subblock_gain", "linbits"},
    "hf_48k_switching": {"bt0", "bt1", "bt2", "bt3", "ms_both_ways", "subblock_gain"},
    "mono_vbr50_switching": {"mono", "bt0", "bt1", "bt2", "bt3", "subblock_gain"},
    "mono_preflag": {"mono", "preflag", "scalefac_scale"},
    "mono_32k_cbr64": {"mono", "bt0"},
    "silence": {"zero_granule"},
}
EVERYTHING = {"bt0", "bt1", "bt2", "bt3", "ms_both_ways", "scfsi", "scalefac_scale", "preflag", "subblock_gain", "count1_a", "count1_b",
              "linbits", "zero_granule", "mono"}


def features(frames):
    """what the parsed side information of these frames shows of the decoder's paths"""
    s, ms = set(), set()
    for info in frames:
        ms.add(info["ms"])
        if info["nch"] == 1:
            s.add("mono")
        if any(any(c) for c in info["scfsi"]):
            s.add("scfsi")
        for g in range(2):
            for q in info["gr"][g]:
                s.add("bt%d" % q["block_type"])
                for key in ("scalefac_scale", "preflag"):
                    if q[key]:
                        s.add(key)
                if any(q["subblock_gain"]):
                    s.add("subblock_gain")
                if q["nquads"]:
                    s.add("count1_b" if q["count1table_select"] else "count1_a")
                if q["linbits_used"]:
                    s.add("linbits")
                if q["part2_3_length"] == 0 and not q["ix"].any():
                    s.add("zero_granule")
    if ms == {0, 1}:
        s.add("ms_both_ways")
    return s


def encode_fn(enc, pcm):
    return enc.encode_f32 if pcm.dtype == np.float32 else enc.encode_s16


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The case through the oracle, one call per block, then zero blocks until every signal frame is out (at most DRAIN_CAP;
    more is a failure) -> (control, pcm, the bytes, per signal call the oracle's taps (ix, signx, gr, ms, scfsi), the calls
    made, the oracle's frame count after them).  A call codes one frame and the reservoir may hold its bytes back, so the
    frame count trails the calls and never passes them."""
    kw, pcm = CPU_CASES[name]()
    enc = O.OracleEncoder(O.default_control(**kw))
    assert enc.ok(), kw
    d = O.oracle_enable_debug(enc)
    F, fn = len(pcm) // 1152, encode_fn(enc, pcm)
    out, taps = [], []
    for f in range(F):
        out.append(fn(pcm[f * 1152:(f + 1) * 1152]))
        assert enc.frames_out() <= f + 1
        taps.append((np.array(d.ix).reshape(2, 2, 576), np.array(d.signx).reshape(2, 2, 576), np.array(d.gr).reshape(2, 2, 27), int(d.ms), list(d.scfsi)))
    calls, zero = F, np.zeros_like(pcm[:1152])
    while enc.frames_out() < F:
        assert calls < F + DRAIN_CAP, "%s: %d zero blocks did not bring the signal's frames out" % (name, DRAIN_CAP)
        out.append(fn(zero))
        calls += 1
        assert enc.frames_out() <= calls
    return kw, pcm, b"".join(out), taps, calls, enc.frames_out()


# ---- the GPU tests' batches: synth.stream_pcm at 0.95 full scale or below, float32 at int16 scale ----
def gpu_pcm(seed, nframes, sr=44100, rho=0.7, bursts=False, mono=False, scale=1.0):
    x = synth.stream_pcm(seed, nframes, sr=sr, rho=rho, bursts=bursts).astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(x[:, 0]) if mono else x


def _bursty(seed, nframes, sr):
    """synth's tones at 0.6 of its scale plus decaying noise bursts every 3000 samples: block switching within a few frames"""
    x = synth.stream_pcm(seed, nframes, sr=sr, rho=0.3).astype(np.float64) * 0.6
    rng = np.random.Generator(np.random.PCG64(0xB0057 + seed))
    env = np.exp(-np.arange(1500) / 150.0)
    for p in range(1700 + 131 * seed, len(x) - 1500, 3000):
        x[p:p + 1500] += 0.3 * 32767.0 * env[:, None] * rng.standard_normal((1500, 2))
    assert np.abs(x).max() <= 0.95 * 32767.0 + 1.0
    return x.astype(np.float32)


_BT = {"bt0", "bt1", "bt2", "bt3"}
CBR128_REACHES = _BT | {"ms_both_ways", "scalefac_scale", "scfsi", "linbits", "count1_a", "count1_b", "zero_granule"}
VBR48_REACHES = _BT | {"ms_both_ways", "subblock_gain", "linbits", "count1_a", "count1_b"}
MONO32_REACHES = _BT | {"mono", "subblock_gain"}
MIXED_REACHES = {"mono", "ms_both_ways", "scalefac_scale"}
HF_REACHES = {"preflag", "scalefac_scale", "bt2", "subblock_gain"}
def _path_scaled(name, seed_offset, nframes):
    """the signal of a case of tests/alloc_path_cases.py (another seed of it: seed_offset), brought to 0.9 full scale and
    followed by zero frames up to nframes"""
    import alloc_path_cases as AP
    _, seed, _, sig = AP.CASES[name]
    x = AP.case_pcm(seed + seed_offset, sig).astype(np.float64)
    x *= 0.9 * 32767.0 / np.abs(x).max()
    out = np.zeros((nframes * 1152,) + x.shape[1:], np.float32)
    out[:len(x)] = x
    return out


F_GPU = 12
# name: (how the batch is made, controls, per stream () -> PCM, what the streams' signal frames together must show of the
# decoder's paths - asserted from the side information parsed out of the GPU's bytes, features()); the last stream of every
# stereo batch is digital silence.  hf_preflag: no synth signal tried reached preflag, so this case takes the tone-and-noise
# steps of the allocator census's m1_hf_02 (its control too), scaled from 4096 x full scale down to 0.9
GPU_CASES = {
    "cbr128_joint_rho": ("one", dict(bitrate=64), [lambda r=r, i=i: gpu_pcm(20 + i, F_GPU, rho=r) for i, r in enumerate((0.0, 0.5, 1.0))] +
                         [lambda: np.zeros((F_GPU * 1152, 2), np.float32)], CBR128_REACHES),
    "vbr_48k_bursts": ("one", dict(samprate=48000, short_block_threshold=100), [lambda i=i: _bursty(30 + i, F_GPU, 48000) for i in range(3)] +
                       [lambda: np.zeros((F_GPU * 1152, 2), np.float32)], VBR48_REACHES),
    "mono_32k": ("one", dict(samprate=32000, mode=3, bitrate=64), [lambda i=i: gpu_pcm(40 + i, F_GPU, sr=32000, mono=True) for i in range(3)], MONO32_REACHES),
    "mixed_mono_stereo": ("mixed", [dict(mode=3), dict()], [lambda: gpu_pcm(50, F_GPU, mono=True), lambda: gpu_pcm(51, F_GPU, rho=0.4),
                                                            lambda: gpu_pcm(52, F_GPU, mono=True, scale=0.5)], MIXED_REACHES),
    "hf_preflag": ("one", dict(samprate=44100, mode=1, hf_flag=3, freq_limit=24000, bitrate=112),
                   [lambda i=i: _path_scaled("m1_hf_02", i, F_GPU) for i in range(2)] + [lambda: np.zeros((F_GPU * 1152, 2), np.float32)], HF_REACHES),
}
MIXED_CFG = [0, 1, 0]
