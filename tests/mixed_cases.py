"""What the mixed-batch suites share (tests/test_gpu_mixed.py: mono and stereo in one batch; tests/test_gpu_any.py: every stream
kind in one batch): one signal per (seed, control) with the oracle's frames for it, computed once and read-only, the rows of
a call pitched for two channels, and where two checkpoint blobs differ.  No GPU."""
import functools

import numpy as np

import packet_cases as PC
from hmp3_amd import synth
from oracle import oracle as O

RHOS = [0.7, 0.0, 1.0, 0.3]


def mono(kw):
    return kw.get("mode") == 3


def key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def signal(seed, kw_items, rho=None):
    """int16 [22 * 1152(, 2)] at the control's rate, a burst in frame 5 or 6 (32 kHz: 1) ([n] for a mono control)"""
    kw = dict(kw_items)
    x = synth.stream_pcm(seed, 30, sr=kw.get("samprate", 44100), rho=RHOS[seed % 4] if rho is None else rho, bursts=True)[8 * 1152:]
    x = np.ascontiguousarray(x[:, seed & 1] if mono(kw) else x)
    x.setflags(write=False)
    return x


def as_f32(x, seed):
    """the signal as float32 at int16 scale with non-integral samples"""
    return x.astype(np.float32) + np.random.default_rng(seed).uniform(-0.49, 0.49, x.shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def want_f32(seed, kw_items, rho=None):
    """-> (float32 signal, the oracle's [PC.Frame] for it): computed once, shared, never changed"""
    x = as_f32(signal(seed, kw_items, rho), seed)
    x.setflags(write=False)
    return x, tuple(PC.oracle_frames(dict(kw_items), x))


@functools.lru_cache(maxsize=None)
def want_s16(seed, kw_items):
    x = signal(seed, kw_items)
    enc = O.OracleEncoder(O.default_control(**dict(kw_items)))
    return x, tuple(enc.encode_s16(x[f * 1152:(f + 1) * 1152]) for f in range(len(x) // 1152))


def streams_of(entries, f32, seed):
    """the streams of a menu, stream i on seed + i: (signals, the oracle's bytes per frame)"""
    if f32:
        w = [want_f32(seed + i, key(kw)) for i, kw in enumerate(entries)]
        return [x for x, _ in w], [[fr.bs for fr in frames] for _, frames in w]
    w = [want_s16(seed + i, key(kw)) for i, kw in enumerate(entries)]
    return [x for x, _ in w], [list(frames) for _, frames in w]


def rows_of(pcm, pos, counts, nf, f32):
    """the call's PCM [S, nf * 1152 * 2]: stream s's next counts[s] frames from frame pos[s] at the start of its row -
    interleaved for a stereo stream, contiguous for a mono one - and 0x7FFF / NaN everywhere else"""
    blk = np.full((len(pcm), nf * 1152 * 2), np.nan if f32 else 0x7FFF, np.float32 if f32 else np.int16)
    for s, n in enumerate(counts):
        part = pcm[s][pos[s] * 1152:(pos[s] + n) * 1152].reshape(-1)
        assert len(part) == n * 1152 * pcm[s].ndim
        blk[s, :len(part)] = part
    return blk


def joined(frames, f0, n):
    return b"".join(frames[f0:f0 + n])


def blob_diff(a, b, skip_class=False):
    """where two checkpoint blobs differ, as byte ranges of the blob ("" = nowhere); skip_class: but for the class index, the
    first word of the stream record behind the 24-byte header - the numbering of the batch the blob was saved from"""
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if len(x) != len(y):
        return "sizes %d and %d" % (len(x), len(y))
    d = x != y
    if skip_class:
        d[24:28] = False
    at = np.nonzero(d)[0]
    if at.size == 0:
        return ""
    cuts = np.nonzero(np.diff(at) > 1)[0]
    runs = list(zip(at[np.r_[0, cuts + 1]].tolist(), at[np.r_[cuts, at.size - 1]].tolist()))
    return "%d bytes differ, in [first, last] %s" % (at.size, runs[:12])
