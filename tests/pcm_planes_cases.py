"""What the PCM planes' tests share (tests/test_gpu_pcm_planes.py): the streams' samples as channel planes, plane images with a
poison between the planes, and the twin's rows built from the same samples.  A plain module beside the tests; it imports no
test module.

A stream's "part" of a call is the list of its channel planes, each n * 1152 samples (an empty list's planes are empty for a
stream that sits the call out).  Whatever of an image or a row belongs to no plane is a poison - 0x7FFF (int16) or a quiet NaN
(fp32): nothing may depend on it."""
import functools

import numpy as np

from hmp3_amd import synth

POISON = {np.dtype(np.int16): 0x7FFF, np.dtype(np.float32): np.nan}


@functools.lru_cache(maxsize=None)
def planes_of(seed, ch, F, f32, sr=44100):
    """stream `seed`'s ch channel planes, each [F * 1152]: int16, or float32 at int16 scale with non-integral samples;
    computed once, shared, never changed"""
    x = synth.stream_pcm(seed, F, sr=sr, rho=(0.7, 0.0, 1.0, 0.3)[seed % 4], bursts=True)
    x = x if ch == 2 else x[:, seed & 1:(seed & 1) + 1]
    if f32:
        x = x.astype(np.float32) + np.random.default_rng(seed).uniform(-0.49, 0.49, x.shape).astype(np.float32)
    out = tuple(np.ascontiguousarray(x[:, c]) for c in range(ch))
    for p in out:
        p.setflags(write=False)
    return out


class Feed:
    """the streams' planes and how far each has come; take(counts) -> every stream's next samples as a list of planes"""

    def __init__(self, channels, F, dtype, seed=1900, sr=None):
        self.dtype = np.dtype(dtype)
        self.sig = [planes_of(seed + i, ch, F, self.dtype == np.float32, *((sr[i],) if sr else ())) for i, ch in enumerate(channels)]
        self.pos = [0] * len(channels)

    def take(self, counts):
        parts = []
        for s, n in enumerate(counts):
            assert (self.pos[s] + n) * 1152 <= len(self.sig[s][0]), "the test's signal is too short"
            parts.append([p[self.pos[s] * 1152:(self.pos[s] + n) * 1152] for p in self.sig[s]])
            self.pos[s] += n
        return parts


def row_of(part):
    """a stream's samples in the order its row holds them: interleaved for two planes"""
    return part[0] if len(part) == 1 else np.stack(part, axis=1).reshape(-1)


def rows_of(parts, nf, P, dtype):
    """the twin's input [S, nf * 1152 * P]: every stream's samples at the start of its row, poison behind them"""
    blk = np.full((len(parts), nf * 1152 * P), POISON[np.dtype(dtype)], dtype)
    for s, part in enumerate(parts):
        r = row_of(part)
        blk[s, :len(r)] = r
    return blk


def image_of(parts, off, stride, total, dtype):
    """the image of `total` bytes: channel c of part i at byte off[i] + c * stride[i] (written in order: an overlap keeps the
    later plane), poison elsewhere; a stream whose planes are empty is not placed (its offset may be wild)"""
    item = np.dtype(dtype).itemsize
    assert total % item == 0
    img = np.full(total // item, POISON[np.dtype(dtype)], dtype)
    for i, part in enumerate(parts):
        for c, p in enumerate(part):
            if len(p) == 0:
                continue
            o = int(off[i]) + c * int(stride[i])
            assert o % item == 0 and 0 <= o and o + p.nbytes <= total, (i, c, o)
            img[o // item:o // item + len(p)] = p
    return img


def spaced(parts, res0, res1, dtype, descending=False, swap=()):
    """a layout with a poisoned gap in front of every plane: plane 0 of stream i starts res0[i] bytes past a 16-byte boundary,
    plane 1 res1[i] bytes past one (descending: the first stream's planes last in the image; swap: streams whose plane 1 lies
    in front of their plane 0, a negative stride) -> (off int64 [S], stride int64 [S], total)"""
    S = len(parts)
    order = range(S - 1, -1, -1) if descending else range(S)
    off, stride, at = np.zeros(S, np.int64), np.zeros(S, np.int64), 0
    for i in order:
        start = [0, 0]
        for c in ((1, 0) if i in swap else (0, 1)):
            if c >= len(parts[i]):
                continue
            start[c] = at + 48 + (res0, res1)[c][i]
            at = (start[c] + parts[i][c].nbytes + 15) // 16 * 16
        off[i] = start[0]
        stride[i] = start[1] - start[0] if len(parts[i]) == 2 else 0
    return off, stride, int(at + 64)
