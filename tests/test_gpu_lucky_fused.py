"""big_lucky_noise forms each candidate's noise where it is summed: one lane per entry (candidate, channel, band) of the work
list computes the entry's terms and adds them in line order, entries dealt alternately to the two waves of a stereo stream,
64 (mono) or 128 per round (hx_alloc.hip, lucky_eval).  Byte identity against the CPU oracle on batches of 8 streams x 32
frames in two calls of 16, CBR-128 and long blocks unless said otherwise: the three MPEG-1 rates, one MPEG-2 rate (bands of up
to 24 lines: the longest loop), mono (one wave takes every entry), -HF VBR, a subband limit of 4 at 48 kHz (the lines past
the coded range stay zero with nothing wiping them: the bit count and the bytes depend on it) and loud near-mono material
(a band quantises beyond the 256-entry table: the out-of-line evaluator with the double table) - each with the certified
band sums and with the strict ones, on k_alloc and on k_alloc_slim.

The debug tap lucky_rounds (entries summed, rounds beyond a wave's first, the longest list of a pass) says which shapes of
list a batch really ran.  Its bounds come from a count on the CPU oracle over exactly these seeds and frames (a copy of
hxo_alloc.c with a counter in big_lucky_noise; per measuring granule the entries of its first pass at twelve / at six
candidates per band and pass, the two builds' limits):
    case         granules   longest list   lists above 64   lists above 128
    44.1 kHz        496      131 / 108       378 / 346          3 / 0
    48 kHz          496      117 / 102       403 / 365          0 / 0
    32 kHz          496      133 / 113       378 / 352          3 / 0
    22.05 kHz       496      186 / 139       474 / 472         99 / 10
    48 kHz mono     496       77 / 70          2 / 1            0 / 0
    -HF VBR         496      144 / 114       479 / 453          5 / 0
    nsb_limit 4     496      135 / 108       220 / 186          2 / 0
    loud (F = 40)   624      123 / 78        304 / 210          0 / 0
A stereo stream's wave takes a second round above 128 entries, a mono stream's above 64: the 44.1 and 32 kHz batches reach
it on the twelve-candidate build only (k_alloc_slim's lists end at 108 and 113 entries there), the mono batch on both.
Run with: python -m pytest tests -m gpu"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from hmp3_amd import api, synth

pytestmark = pytest.mark.gpu
S, F, CALL = 8, 32, 16                                      # streams (seeds 0 .. 7 of synth.stream_pcm), frames, frames per call
BASE = dict(bitrate=64, short_block_threshold=99999)        # CBR-128, long blocks
CASES = {
    "44k": dict(BASE),
    "48k": dict(BASE, samprate=48000),
    "32k": dict(BASE, samprate=32000),
    "lsf_22k": dict(BASE, samprate=22050),
    "48k_mono": dict(BASE, samprate=48000, mode=3),
    "48k_vbr_hf": dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000, short_block_threshold=99999),
    "48k_nsb4": dict(BASE, samprate=48000, nsb_limit=4),
}
# cases whose lists pass a wave's first round (CPU count above): on the twelve-candidate build / on both builds
SECOND_ROUND_FAT = ("44k", "32k")
SECOND_ROUND_BOTH = ("48k_mono",)
LOUD_S, LOUD_F = 8, 40                                      # the batch of test_gpu_parity's loud near-mono case


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the batch's PCM, the oracle's bytes per stream): computed once per case, shared by the builds and both kinds of band sums"""
    kw = CASES[name]
    pcm = np.stack([synth.stream_pcm(s, F, kw.get("samprate", 44100)) for s in range(S)])
    if kw.get("mode") == 3:
        pcm = np.ascontiguousarray(pcm[:, :, 0])
    want = []
    for s in range(S):
        enc = O.OracleEncoder(O.default_control(**kw))
        want.append(b"".join(enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152]) for f in range(F)))
    return pcm, want


@functools.lru_cache(maxsize=None)
def loud_reference():
    pcm = np.stack([synth.stream_pcm(8100 + s, LOUD_F, sr=44100, rho=1.0, bursts=False) for s in range(LOUD_S)])
    want = []
    for s in range(LOUD_S):
        enc = O.OracleEncoder(O.default_control(**BASE))
        want.append(b"".join(enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152]) for f in range(LOUD_F)))
    return pcm, want


def encode(kw, pcm, nstreams, call):
    """the batch in two calls; (bytes per stream, the lucky_rounds words, double-table passes, the build that ran)"""
    b = api.Batch(api.default_control(**kw), nstreams=nstreams, max_frames=max(call, pcm.shape[1] // 1152 - call))
    got = b.encode_host(pcm[:, :call * 1152])
    got2 = b.encode_host(pcm[:, call * 1152:])
    assert b.status() == 0
    rounds = [int(v) for v in b.debug_read("lucky_rounds", np.int32, 3)]
    big = int(b.debug_read("big_sweeps", np.int32, 1)[0])
    variant = b.k6_variant()
    b.close()
    return [got[s] + got2[s] for s in range(nstreams)], rounds, big, variant


@pytest.mark.parametrize("strict", [0, 1], ids=["certified", "strict"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_byte_identical_to_oracle(name, strict, k6_build, monkeypatch):
    # (a batch reads the variable when it is created)
    monkeypatch.setenv("HMP3AMD_EXACT_SUMS", str(strict))
    pcm, want = reference(name)
    got, (entries, extra_rounds, longest), big, variant = encode(CASES[name], pcm, S, CALL)
    print("%s strict %d build %s (variant %d): %d entries summed, %d rounds beyond a wave's first, longest list %d"
          % (name, strict, k6_build, variant, entries, extra_rounds, longest))
    for s in range(S):
        assert got[s] == want[s], "stream %d" % s
    assert entries > 0, "big_lucky_noise did not run"
    twelve = variant == 0       # k_alloc / k_alloc_lsf: twelve candidates per band and pass (MPEG-2 batches ignore the build switch)
    if CASES[name].get("mode") != 3:
        assert longest > 64, "no list longer than one round of a single wave"
    if name in SECOND_ROUND_BOTH or (name in SECOND_ROUND_FAT and twelve):
        assert extra_rounds > 0, "no wave took a second round"


@pytest.mark.parametrize("strict", [0, 1], ids=["certified", "strict"])
def test_loud_near_mono_material_takes_the_out_of_line_evaluator(strict, k6_build, monkeypatch):
    """L = R at full scale: bands of the mid channel quantise beyond the 256-entry table at big_lucky's low gain steps, and
    the pass goes to the evaluator that fetches the double table (it books itself in the double-table counter, as the gain
    search's passes do)."""
    monkeypatch.setenv("HMP3AMD_EXACT_SUMS", str(strict))
    pcm, want = loud_reference()
    got, (entries, extra_rounds, longest), big, variant = encode(BASE, pcm, LOUD_S, LOUD_F // 2)
    print("loud strict %d build %s: %d entries, %d extra rounds, longest list %d, double-table passes %d" % (strict, k6_build, entries, extra_rounds, longest, big))
    for s in range(LOUD_S):
        assert got[s] == want[s], "stream %d" % s
    assert entries > 0 and longest > 64
    assert big > 0, "the case does not reach the table's end"
