"""PCM planes (hx_batch_pcm_planes) against the two ways a caller has without them, alternated call by call in one process,
medians over the calls.  Config-2 shape (1024 stereo streams x 256 frames, CBR-128, long blocks only), the input a float32
waveform tensor [streams, 2, time] in [-1, 1) on the device:
  (a) planes      the call under planes with unit_scale: k_pcm_planes interleaves and scales into the batch's row buffer;
  (b) torch       the same tensor interleaved and scaled by torch, (w * 32768).transpose(1, 2).contiguous(), inside the timed
                  region, then fed as rows;
  (c) rows        a rows call on a buffer interleaved and scaled beforehand: what neither costs.
(a) - (c) is what the planes cost, (b) - (c) what the framework's copy costs; both with the spread of the runs.  Nothing is
gated.  With --only WAY the process makes calls of one way alone, for a kernel trace of its own; there "segments" is a way
too: (c)'s buffer fed as the tight image of PCM segments, so that k_pcm_spread moves the bytes k_pcm_planes moves.  One JSON line.
  python tools/bench_pcm_planes.py [--streams 1024] [--frames 256] [--steps 8] [--only planes|torch|rows|segments] [--out profiles/pcm_planes_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WAYS = ("planes", "torch", "rows")


def ms(x):
    return round(1e3 * float(x), 3)


def spread(t):
    """median, lowest and highest of a way's runs, in ms"""
    return {"median": ms(np.median(t)), "min": ms(min(t)), "max": ms(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--only", default="", choices=("",) + WAYS + ("segments",))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 6 and not args.only:
        ap.error("--steps: medians of at least 6 calls")
    import torch
    from hmp3_amd import api, synth
    L = api.lib()
    S, F = args.streams, args.frames
    b = api.Batch(api.default_control(bitrate=64, short_block_threshold=99999), nstreams=S, max_frames=F)
    src = torch.from_numpy(synth.batch_pcm(S, F, unique=16)).cuda()                    # int16 [S, F * 1152, 2]
    w = (src.to(torch.float32) / 32768).transpose(1, 2).contiguous()                    # the waveform [S, 2, T] in [-1, 1)
    rows = (w * 32768).transpose(1, 2).contiguous()                                     # (c)'s buffer, made once
    del src
    off, chan_stride, total, first = api.tensor_planes(w.shape, w.stride(), 4)
    assert first == 0 and total == w.numel() * 4
    stride = b.out_stride(F)
    d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
    q = torch.cuda.current_stream().cuda_stream

    def call(way):
        if way == "planes":
            b.pcm_planes(off, chan_stride, total, unit_scale=True)
        elif way == "segments":
            b.pcm_segments(*b.packed_layout(F, True))
        else:
            b.pcm_planes(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pcm = w if way == "planes" else rows if way in ("rows", "segments") else (w * 32768).transpose(1, 2).contiguous()
        if L.hx_batch_encode_f32_device(b.h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ways = (args.only,) if args.only else WAYS
    for x in ways:          # (warm-up)
        call(x)
    t = {x: [] for x in ways}
    for _ in range(args.steps):
        for x in ways:
            t[x].append(call(x))
    assert b.status() == 0
    b.close()
    res = {"what": "PCM planes against torch's interleave-and-scale and against rows made beforehand, alternated call by call on one box; "
                   "fp32 unit-scale [streams, 2, time] on the device, ms per call",
           "build_id": api.build_id(), "streams": S, "frames": F, "calls": args.steps, "pcm_bytes": int(total),
           "ms": {x: spread(t[x]) for x in ways}, "ms_each": {x: [ms(v) for v in t[x]] for x in ways}}
    if not args.only:
        d = lambda x: [u - v for u, v in zip(t[x], t["rows"])]
        res["planes_minus_rows_ms"] = dict(spread(d("planes")), of_medians=round(res["ms"]["planes"]["median"] - res["ms"]["rows"]["median"], 3))
        res["torch_minus_rows_ms"] = dict(spread(d("torch")), of_medians=round(res["ms"]["torch"]["median"] - res["ms"]["rows"]["median"], 3))
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
