"""Converting batches at config-2 shape (1024 streams x 256 frames per call, CBR-128 stereo): the converting call
(hx_batch_encode_src_device: k_src in front of the fp32 path) against the same batch fed the pre-converted fp32
(hx_batch_encode_f32_device), alternated call by call in one process, and the host converter (hx_src_convert) on 16
threads for the same sources.  One JSON line per configuration.  k_src's own time: run this under
rocprofv3 --kernel-trace --stats (a separate run; the wall times here are not taken under the profiler).
  python tools/bench_src.py [--streams 1024] [--frames 256] [--steps 6] [--host-frames 2000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, source rate, bits, is_float, encode rate)
CONFIGS = [("48k_s24_to_44k1", 48000, 24, 0, 44100), ("44k1_s16_to_32k", 44100, 16, 0, 32000), ("44k1_f32_same_rate", 44100, 32, 1, 44100)]


def source_rows(rng, S, stride, bits, is_float):
    """[S][stride] bytes of a noisy tone in the source format (row i: stream i's next input)"""
    n = stride // (2 * bits // 8) + 1
    t = np.arange(n)[:, None]
    x = 0.3 * np.sin(2 * np.pi * 440.0 * t / 44100.0) + 0.02 * rng.standard_normal((n, 2))
    x = x.reshape(-1)
    if is_float:
        b = x.astype("<f4").tobytes()
    elif bits == 16:
        b = (x * 32767).astype("<i2").tobytes()
    else:
        v = (x * 2147483647.0).astype("<i4").view(np.uint8).reshape(-1, 4)
        b = (v if bits == 32 else v[:, 1:]).tobytes()
    row = np.frombuffer(b[:stride], np.uint8)
    return np.broadcast_to(row, (S, stride)).copy()


def host_rate(source, bits, is_float, target, frames, threads=16):
    """frames/s of hx_src_convert on `threads` threads, each converting its own stream"""
    from hmp3_amd import api
    L = api.lib()
    fb = 2 * bits // 8
    per = 1152 * (source // target + 2) * fb
    data = (C.c_ubyte * (per * 4))()

    def work(_):
        h = L.hx_src_create()
        cut = C.c_int(0)
        L.hx_src_init(h, source, 2, bits, is_float, target, 2, C.byref(cut))
        y = np.zeros(2304, np.float32)
        for _ in range(frames):
            L.hx_src_convert(h, data, y.ctypes.data, None)
        L.hx_src_destroy(h)

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(work, range(threads)))
        dt = time.perf_counter() - t0
    return threads * frames / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--host-frames", type=int, default=2000)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    from hmp3_amd import api
    S, F = args.streams, args.frames
    rng = np.random.default_rng(1)
    for name, source, bits, is_float, target in CONFIGS:
        if args.only and args.only != name:
            continue
        ec = api.default_control(bitrate=64)
        ec.samprate = source
        src = api.Source(bits, is_float, target, 0)
        sb = api.SrcBatch(ec, src, nstreams=S, max_frames=F)
        ec2, _ = api.src_encode_control(ec, src)
        fb_ = api.Batch(ec2, nstreams=S, max_frames=F)
        in_stride = sb.in_stride(F)
        d_in = torch.from_numpy(source_rows(rng, S, in_stride, bits, is_float)).cuda()
        stride = sb.out_stride(F)
        d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
        d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
        used = np.zeros(S, np.int64)
        q = torch.cuda.current_stream().cuda_stream
        L = api.lib()

        def conv():
            if L.hx_batch_encode_src_device(sb.h, d_in.data_ptr(), in_stride, None, F, d_out.data_ptr(), stride, d_nb.data_ptr(), used.ctypes.data, q) != 0:
                raise RuntimeError(api.last_error())
        # the fp32 the converter made, fed to the plain batch (each call re-encodes the same converted block)
        conv()
        torch.cuda.synchronize()
        pcm = torch.from_numpy(sb.debug_read("srcpcm", np.float32, S * F * 1152 * 2).reshape(S, F * 1152, 2)).cuda()

        def plain():
            if L.hx_batch_encode_f32_device(fb_.h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
                raise RuntimeError(api.last_error())
        for fn in (conv, plain):            # warm-up
            fn()
        torch.cuda.synchronize()
        tc, tp = [], []
        for _ in range(args.steps):
            for fn, acc in ((conv, tc), (plain, tp)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append(time.perf_counter() - t0)
        assert sb.status() == 0 and fb_.status() == 0
        ms_c, ms_p = 1e3 * float(np.median(tc)), 1e3 * float(np.median(tp))
        in_bytes = S * in_stride
        gpu_rate = S * F / (ms_c / 1e3)
        hrate = host_rate(source, bits, is_float, target, args.host_frames) if args.host_frames > 0 else None
        print(json.dumps({"config": name, "streams": S, "frames": F, "ms_converting_call": round(ms_c, 3), "ms_f32_call": round(ms_p, 3),
                          "ratio": round(ms_c / ms_p, 4), "gpu_frames_per_s": round(gpu_rate), "host_src_frames_per_s_16_threads": None if hrate is None else round(hrate),
                          "gpu_over_host": None if hrate is None else round(gpu_rate / hrate, 1), "input_bytes_per_call": in_bytes,
                          "output_bytes_per_call": S * F * 1152 * 2 * 4, "calls": args.steps}), flush=True)
        sb.close()
        fb_.close()
        del d_in, pcm, d_out


if __name__ == "__main__":
    main()
