"""Stage-by-stage comparison of the HIP pipeline against the oracle on a real GPU, from the command line.
Usage: python tests/gpu_check.py [nstreams] [nframes] [config]
The comparison is tests/stage_taps.py (TapBatch), the one the GPU tests use: every stage by bit pattern, long and short
granules alike.  Prints the first stage / stream / frame where the two differ (everything is expected to be bit-exact).
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from hmp3_amd import api, synth
from stage_taps import TapBatch

CONFIGS = {
    "cbr128": dict(bitrate=64, short_block_threshold=99999),
    "cbr128lr": dict(bitrate=64, mode=0, short_block_threshold=99999),
    "vbr50": dict(short_block_threshold=99999),
    "cbr192": dict(bitrate=96, short_block_threshold=99999),
    "vbr100hf": dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000, short_block_threshold=99999),
    "cbr128_32k": dict(bitrate=64, samprate=32000, short_block_threshold=99999),
    # block switching on (default threshold 700) with bursts in the signal
    "cbr128_sw": dict(bitrate=64),
    "cbr128lr_sw": dict(bitrate=64, mode=0),
    "vbr50_sw": dict(),
    "vbr100hf_sw": dict(samprate=48000, vbr_mnr=100, hf_flag=3, freq_limit=19000),
    "cbr128_thr100": dict(bitrate=64, short_block_threshold=100),
}


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    cfg = sys.argv[3] if len(sys.argv) > 3 else "cbr128"
    kw = CONFIGS[cfg]
    sr = kw.get("samprate", 44100)
    rhos = [0.7, 0.0, 1.0, 0.3]
    bursts = kw.get('short_block_threshold', 700) < 99999
    seeds = list(range(S))
    if "GC_KW" in os.environ:       # an arbitrary case: GC_KW='{"bitrate": 160, ...}' GC_SEEDS=395960 GC_RHO=0.7 GC_BURSTS=1 (stereo)
        import json
        kw = json.loads(os.environ["GC_KW"])
        sr = kw.get("samprate", 44100)
        seeds = [int(x) for x in os.environ.get("GC_SEEDS", "0").split(",")]
        S = len(seeds)
        rhos = [float(os.environ.get("GC_RHO", "0.7"))] * 4
        bursts = bool(int(os.environ.get("GC_BURSTS", "0")))
    pcm = np.stack([synth.stream_pcm(seeds[i], F, sr=sr, rho=rhos[i % 4], bursts=bursts) for i in range(S)])
    full = kw.get("mode", 1) in (0, 1) and sr >= 32000 and "nsbstereo" not in kw    # the path on which the oracle taps everything
    t0 = time.time()
    tb = TapBatch(api, kw, S, F, "full" if full else "lines")
    ok = True
    try:
        tb.call(pcm if kw.get("mode") != 3 else pcm[:, :, 0])
    except AssertionError as e:
        ok = False
        print("first mismatch (stage, stream, frame, granule, channel ...):", e)
    print("compared in %.3fs: block types %s, %d short granules, %d long granules through k_prep's comparison"
          % (time.time() - t0, sorted(tb.seen_bt), sum(tb.short_granules), tb.prep_granules))
    tb.close()
    print("RESULT", "PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
