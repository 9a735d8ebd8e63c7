"""The batches of the stream walk's line-loop test (tests/test_gpu_line_loops.py), and their encode in two calls: what the test
and the fresh child process it starts under HMP3AMD_EXACT_SUMS both run."""
import numpy as np

from hmp3_amd import api, synth

F, CALL = 24, 12                                            # frames per stream, given as two calls of 12
STREAMS = [(seed, rho) for seed in (0, 1, 2) for rho in (0.7, 1.0)]
BASE = dict(bitrate=64, short_block_threshold=99999)        # CBR-128, long blocks
BATCHES = {
    "44k": dict(BASE),
    "48k": dict(BASE, samprate=48000),
    "32k": dict(BASE, samprate=32000),
    "lsf_22k": dict(BASE, samprate=22050),
    "lsf_24k": dict(BASE, samprate=24000),
    "lsf_16k": dict(BASE, samprate=16000),
    "44k_freq8000": dict(BASE, freq_limit=8000),
    "48k_nsb4": dict(BASE, samprate=48000, nsb_limit=4),
}


def batch_pcm(kw, mono=False):
    sr = kw.get("samprate", 44100)
    pcm = np.stack([synth.stream_pcm(seed, F, sr, rho) for seed, rho in STREAMS])
    return np.ascontiguousarray(pcm[:1, :, 0]) if mono else pcm


def encode_two_calls(kw, pcm):
    b = api.Batch(api.default_control(**kw), nstreams=pcm.shape[0], max_frames=CALL)
    got = b.encode_host(pcm[:, :CALL * 1152])
    got2 = b.encode_host(pcm[:, CALL * 1152:])
    assert b.status() == 0
    b.close()
    return [got[s] + got2[s] for s in range(pcm.shape[0])]
