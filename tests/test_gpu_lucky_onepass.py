"""big_lucky_noise of the 256-register stream walks (k_alloc, k_alloc_lsf) measures up to twelve candidates per band in one
pass: the terms run on from the term buffer into the quantised lines, which are dead until the quantiser runs, and what a
pass left past the coded range is zero again before it does (hx_alloc.hip).  Byte identity against the CPU oracle on
batches of 8 streams x 32 frames, CBR-128 and long blocks unless said otherwise: the three MPEG-1 rates (K = 12, 12, 11), one
MPEG-2 rate (its own band tables and K), mono (no helper wave), -HF VBR (band 21's lines lie past the coded range) and a
subband limit of 4 at 48 kHz (72 coded lines: nearly every line the terms reach is past the coded range) - each with the
certified band sums and with the strict ones.  The device's counter says which passes the 44.1 kHz batch really took.
Run with: python -m pytest tests -m gpu"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from hmp3_amd import api, synth

# (k_alloc / k_alloc_lsf only: the low-footprint build keeps its six candidates per pass and does not count)
pytestmark = [pytest.mark.gpu, pytest.mark.one_k6_build]
S, F, CALL = 8, 32, 16                                      # streams (seeds 0x484D5033 + 0 .. 7), frames, frames per call
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


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the batch's PCM, the oracle's bytes per stream): computed once per case, shared by both kinds of band sums"""
    kw = CASES[name]
    pcm = np.stack([synth.stream_pcm(s, F, kw.get("samprate", 44100)) for s in range(S)])
    if kw.get("mode") == 3:
        pcm = np.ascontiguousarray(pcm[:, :, 0])
    want = []
    for s in range(S):
        enc = O.OracleEncoder(O.default_control(**kw))
        want.append(b"".join(enc.encode_s16(pcm[s, f * 1152:(f + 1) * 1152]) for f in range(F)))
    return pcm, want


def encode(kw, pcm):
    """the batch in two calls on the 256-register build; (bytes per stream, the big_lucky counters)"""
    b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=CALL)
    got = b.encode_host(pcm[:, :CALL * 1152])
    got2 = b.encode_host(pcm[:, CALL * 1152:])
    assert b.status() == 0
    assert b.k6_variant() == 0, "the case is meant for k_alloc / k_alloc_lsf"
    lucky = [int(v) for v in b.debug_read("lucky", np.int32, 3)]
    b.close()
    return [got[s] + got2[s] for s in range(S)], lucky


@pytest.mark.parametrize("strict", [0, 1], ids=["certified", "strict"])
@pytest.mark.parametrize("name", list(CASES))
def test_one_pass_byte_identical_to_oracle(name, strict, monkeypatch):
    # (a batch reads the variable when it is created)
    monkeypatch.setenv("HMP3AMD_EXACT_SUMS", str(strict))
    pcm, want = reference(name)
    got, (granules, passes, wide) = encode(CASES[name], pcm)
    print("%s strict %d: big_lucky measured %d granules in %d passes (%.2f per granule), %d with more than six candidates in a pass"
          % (name, strict, granules, passes, passes / max(granules, 1), wide))
    for s in range(S):
        assert got[s] == want[s], "stream %d" % s
    assert granules > 0 and passes >= granules, "big_lucky_noise did not run"
    assert wide > 0, "no pass reached beyond the term buffer"


def test_all_three_kinds_of_granule_at_44k():
    """Six or fewer candidates per band (the pass stays inside the term buffer), seven to twelve in one pass (it reaches
    into the lines, no second pass), and more than twelve (a second pass): the 44.1 kHz batch has granules of each kind.
    Every granule with a second pass is a wide one, so wide - (passes - granules) bounds the one-pass wide granules from
    below.  On the CPU, over twelve seeds x 128 frames of the same family, the shares are 19 %, 74 % and 6.7 %: 1.07 passes per
    granule with twelve candidates per pass, 1.88 with six.  The bound on the passes, 1.25 per granule, lies between the two:
    more than three times the CPU count's share of second passes, and out of reach of a pass of six."""
    pcm, want = reference("44k")
    got, (granules, passes, wide) = encode(CASES["44k"], pcm)
    print("44k: granules %d, passes %d (%.3f per granule), wide %d" % (granules, passes, passes / max(granules, 1), wide))
    assert got == want
    assert granules - wide > 0, "no granule with six or fewer candidates"
    assert passes > granules, "no granule took a second pass"
    assert wide - (passes - granules) > 0, "no granule with seven to twelve candidates in one pass"
    assert passes <= 1.25 * granules, "passes per granule far from the CPU count's 1.07"
