"""PCM segments (hx_batch_pcm_segments) against rows, alternated call by call in one process, medians over the calls.
1. Host-fed: one mixed batch (P = 2, every second stream mono) under counts cycling over {frames, frames / 2, 0}, through
   hx_batch_encode_s16_host from page-locked memory - once fed rows [streams][frames * 1152 * 2], once the tight image
   (hx_pcm_packed_layout) of the same samples: the call time and the PCM bytes that crossed the link, each way.
2. Device calls with uniform stereo streams, where segments save nothing: the same device buffer read as rows and as the
   tight image (with uniform streams the two layouts coincide), so the difference is what k_pcm_spread's extra pass costs.
Both are reported, neither is gated.  One JSON line.
  python tools/bench_pcm_segments.py [--streams 1024] [--frames 256] [--steps 8] [--out profiles/pcm_segments.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pinned(api, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = api.lib().hx_pinned_alloc(max(n, 16))
    if not p:
        raise MemoryError("hx_pinned_alloc(%d)" % n)
    return p, np.frombuffer((C.c_ubyte * n).from_address(p), dtype=dtype).reshape(shape)


def median_ms(t):
    return round(1e3 * float(np.median(t)), 3)


def host_fed(api, synth, S, F, steps):
    import torch
    L = api.lib()
    ch = [2 if s % 2 == 0 else 1 for s in range(S)]
    counts = [(F, F // 2, 0)[s % 3] for s in range(S)]
    b = api.Batch.mixed([api.default_control(bitrate=64), api.default_control(bitrate=64, mode=3)], S, cfg=[s % 2 for s in range(S)], max_frames=F)
    src = synth.batch_pcm(S, F, unique=16)
    off, total = api.packed_layout(F, ch, counts)
    held = []
    p, rows = pinned(api, (S, F * 1152 * 2), np.int16)
    held.append(p)
    p, image = pinned(api, (max(total // 2, 8),), np.int16)
    held.append(p)
    rows[...] = 0
    for s in range(S):
        x = (src[s] if ch[s] == 2 else src[s, :, 0])[:counts[s] * 1152].reshape(-1)
        rows[s, :len(x)] = x
        image[off[s] // 2:off[s] // 2 + len(x)] = x
    stride = b.out_stride(F)
    out, nb = np.zeros((S, stride), np.uint8), np.zeros(S, np.int32)
    b.frame_counts(counts)

    def call(way):
        b.pcm_segments(off if way == "image" else None, total)
        pcm = image if way == "image" else rows
        t0 = time.perf_counter()
        if L.hx_batch_encode_s16_host(b.h, pcm.ctypes.data, F, out.ctypes.data, stride, nb.ctypes.data) != 0:
            raise RuntimeError(api.last_error())
        return time.perf_counter() - t0
    ways = ("rows", "image")
    for w in ways:
        call(w)
    t = {w: [] for w in ways}
    for _ in range(steps):
        for w in ways:
            t[w].append(call(w))
    assert b.status() == 0
    b.close()
    torch.cuda.synchronize()
    for p in held:
        L.hx_pinned_free(p)
    frames = sum(counts)
    return {"streams": S, "frames": F, "calls": steps, "frames_encoded_per_call": frames,
            "link_bytes_rows": int(rows.nbytes), "link_bytes_image": int(total),
            "ms_rows": median_ms(t["rows"]), "ms_image": median_ms(t["image"]),
            "ms_each_rows": [round(1e3 * x, 3) for x in t["rows"]], "ms_each_image": [round(1e3 * x, 3) for x in t["image"]]}


def device_uniform(api, synth, S, F, steps):
    import torch
    L = api.lib()
    b = api.Batch(api.default_control(bitrate=64), nstreams=S, max_frames=F)
    pcm = torch.from_numpy(synth.batch_pcm(S, F, unique=16)).cuda()
    off, total = b.packed_layout(F)
    assert total == pcm.numel() * 2
    stride = b.out_stride(F)
    d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
    q = torch.cuda.current_stream().cuda_stream

    def call(way):
        b.pcm_segments(off if way == "segments" else None, total)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if L.hx_batch_encode_s16_device(b.h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    ways = ("rows", "segments")
    for w in ways:
        call(w)
    t = {w: [] for w in ways}
    for _ in range(steps):
        for w in ways:
            t[w].append(call(w))
    assert b.status() == 0
    b.close()
    return {"streams": S, "frames": F, "calls": steps, "pcm_bytes": int(total),
            "ms_rows": median_ms(t["rows"]), "ms_segments": median_ms(t["segments"]),
            "ms_spread": round(median_ms(t["segments"]) - median_ms(t["rows"]), 3),
            "ms_each_rows": [round(1e3 * x, 3) for x in t["rows"]], "ms_each_segments": [round(1e3 * x, 3) for x in t["segments"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.steps < 6:
        ap.error("--steps: medians of at least 6 calls")
    from hmp3_amd import api, synth
    res = {"what": "PCM segments against rows, alternated call by call on one box, medians; int16 PCM",
           "build_id": api.build_id(),
           "host_fed_mixed_counts": host_fed(api, synth, args.streams, args.frames, args.steps),
           "device_uniform": device_uniform(api, synth, args.streams, args.frames, args.steps)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
