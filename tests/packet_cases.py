"""What the packet / frame-counter tests share (test infrastructure): the controls, the fp32 input with non-integral samples,
and the per-frame expectation from the oracle's L3_audio_encode_Packet restatement.  tests/test_gpu_packets.py compares the
batched calls' optional outputs with it, tests/test_oracle_vs_ref.py pins it to the real reference for the same controls."""
import ctypes as C

import numpy as np

from oracle import oracle as O
from hmp3_amd import synth

RHOS = [0.7, 0.0, 1.0, 0.3]

# MPEG-1 rates, the stream walk k_alloc / k_alloc_slim: one packet per call
MPEG1 = [
    dict(bitrate=64),
    dict(vbr_mnr=60),
    dict(bitrate=64, mode=0),
    dict(bitrate=160),
    dict(vbr_mnr=150, hf_flag=3, freq_limit=22000, samprate=48000),
    dict(bitrate=64, mode=3),       # mono: 21 bytes of header and side info
    dict(mode=3),
]
# MPEG-2 rates (k_alloc_lsf): two single-granule packets per call, back to back
MPEG2 = [
    dict(bitrate=32, samprate=22050),
    dict(samprate=24000, vbr_mnr=80),
    dict(bitrate=32, samprate=16000, mode=3),
    dict(samprate=16000, mode=3),
]
# the first-generation allocator (k_alloc1 / k_alloc1_lsf): dual channel, intensity stereo
A1 = [
    dict(bitrate=64, mode=2),
    dict(bitrate=64, nsbstereo=8),
    dict(bitrate=16, samprate=22050),
    dict(bitrate=16, samprate=16000, mode=2),
    dict(bitrate=8, samprate=16000),
]


def case_id(kw):
    return "-".join("%s%s" % (k[:4], v) for k, v in kw.items())


def packet_pcm(seed, S, F, kw, noise_seed=5, bursts=lambda i: i % 2 == 0):
    """float32 [S, F * 1152, 2] ([S, F * 1152] for a mono control) at int16 scale, samples non-integral"""
    sr = kw.get("samprate", 44100)
    pcm = np.stack([synth.stream_pcm(seed + i, F, sr, rho=RHOS[i % 4], bursts=bool(bursts(i))) for i in range(S)]).astype(np.float32)
    pcm += np.random.default_rng(noise_seed).uniform(-0.49, 0.49, pcm.shape).astype(np.float32)
    if kw.get("mode") == 3:
        pcm = np.ascontiguousarray(pcm[:, :, 0])
    return pcm


class Frame:
    """what one L3_audio_encode_Packet call of one stream returns, and the stream's counters behind it"""
    __slots__ = ("bs", "packet", "sizes", "frames_out", "bytes_out")

    def __init__(self, bs, packet, sizes, frames_out, bytes_out):
        self.bs, self.packet, self.sizes, self.frames_out, self.bytes_out = bs, packet, sizes, frames_out, bytes_out


def oracle_control(ec):
    """a control dict, or an E_CONTROL structure of the library's binding, as the oracle's"""
    if isinstance(ec, dict):
        return O.default_control(**ec)
    oc = O.Control()
    assert C.sizeof(oc) == C.sizeof(ec)
    C.memmove(C.byref(oc), C.byref(ec), C.sizeof(oc))
    return oc


def oracle_frames(ec, pcm):
    """one stream, pcm float32 [F * 1152(, 2)] -> [Frame] * F from one OracleEncoder fed frame by frame"""
    enc = O.OracleEncoder(oracle_control(ec))
    assert enc.ok()
    out = []
    for f in range(len(pcm) // 1152):
        bs, pk = enc.encode_packet(pcm[f * 1152:(f + 1) * 1152])
        out.append(Frame(bs, pk, tuple(enc.packet_sizes), enc.frames_out(), enc.bytes_out()))
    return out
