"""The mixed-rate batches the dense-output and MusicCRC suites share (tests/test_gpu_dense.py, tests/test_gpu_crc.py): streams at
32, 44.1 and 48 kHz in turn, VBR-50 by default, so that the streams' byte counts differ.  One generated signal per shape,
shared and read-only."""
import functools

import numpy as np

from hmp3_amd import api, synth

RATES = (32000, 44100, 48000)


@functools.lru_cache(maxsize=None)
def mixed_pcm(S, F, first, unique=66):
    """fp32 PCM [S, F * 1152, 2] at int16 values, stream i at RATES[i % 3]; beyond `unique` distinct streams the rest are
    time-rotated copies of their class (generation stays cheap at S = 1100)"""
    base = [synth.stream_pcm(first + i, F, sr=RATES[i % 3], rho=(0.7, 0.0, 1.0, 0.3)[i % 4], bursts=True) for i in range(min(S, unique))]
    out = np.empty((S, F * 1152, 2), dtype=np.float32)
    for i in range(S):
        out[i] = base[i] if i < unique else np.roll(base[i % unique], 1152 * (i // unique) // 2 + 97 * (i // unique), axis=0)
    out.setflags(write=False)
    return out


def mixed_controls(S, **kw):
    """VBR-50 by default: the streams' byte counts differ"""
    return [api.default_control(samprate=RATES[i % 3], **kw) for i in range(S)]
