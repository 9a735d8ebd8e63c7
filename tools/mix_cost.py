"""What mixing kinds in one batch costs: one batch of N kind-0 (44.1 kHz CBR stereo) plus N kind-1 (22.05 kHz CBR stereo) streams
(hx_batch_create_any, slots interleaved) against two uniform batches of N streams each run back to back, on the same PCM,
fp32 device calls of F frames, alternated call by call in one process; medians.  A batch of several kinds walks its streams
in one launch per kind, one after the other on one stream, so every kind adds a launch tail in which the chip drains.  Two
uniform batches run back to back have the same two tails, so this comparison does NOT measure the tail: the difference of
the two stream-walk times is what k_order_kinds and the spans cost, and the difference of the call times what one front end
and one packing instead of two save.  The tail's own size would take a walk that holds both kinds at once, which does not
exist.  One JSON line.
  python tools/mix_cost.py [--streams 512] [--frames 64] [--steps 9] [--out profiles/mix_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=512, help="streams per kind")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from hmp3_amd import api, synth
    N, F = args.streams, args.frames
    L = api.lib()
    menu = [api.default_control(bitrate=64), api.default_control(bitrate=32, samprate=22050)]
    mixed = api.Batch.any(menu, 2 * N, cfg=[s & 1 for s in range(2 * N)], max_frames=F)
    parts = [api.Batch(menu[k], nstreams=N, max_frames=F) for k in range(2)]
    host = synth.batch_pcm(2 * N, F, unique=16).astype(np.float32)
    pcm = torch.from_numpy(host).cuda()
    pcm_k = [torch.from_numpy(np.ascontiguousarray(host[k::2])).cuda() for k in range(2)]      # the same rows, per kind
    q = torch.cuda.current_stream().cuda_stream

    def buffers(b):
        stride = b.out_stride(F)
        return stride, torch.zeros((b.n, stride), dtype=torch.uint8, device="cuda"), torch.zeros(b.n, dtype=torch.int32, device="cuda")
    out_m, out_k = buffers(mixed), [buffers(b) for b in parts]

    def call(b, x, o):
        if L.hx_batch_encode_f32_device(b.h, x.data_ptr(), F, o[1].data_ptr(), o[0], o[2].data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())

    def run_mixed():
        t0 = time.perf_counter()
        call(mixed, pcm, out_m)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, mixed.alloc_kernel_ms()[0]

    def run_parts():
        t0 = time.perf_counter()
        for k in range(2):
            call(parts[k], pcm_k[k], out_k[k])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(b.alloc_kernel_ms()[0] for b in parts)
    for _ in range(2):          # warm-up (the second call's launch order is the first call's durations)
        run_mixed()
        run_parts()
    t = {"mixed": [], "parts": []}
    for _ in range(args.steps):
        t["mixed"].append(run_mixed())
        t["parts"].append(run_parts())
    assert mixed.status() == 0 and all(b.status() == 0 for b in parts)
    # the same streams, the same bytes
    nb_m, nb_k = out_m[2].cpu().numpy(), [o[2].cpu().numpy() for o in out_k]
    assert all((nb_m[k::2] == nb_k[k]).all() for k in range(2)), "the mixed batch's byte counts differ from the uniform batches'"
    med = lambda v, i: round(float(np.median([x[i] for x in t[v]])) * (1e3 if i == 0 else 1), 3)
    res = {"streams_per_kind": N, "frames": F, "calls": args.steps, "build_id": api.build_id(),
           "mixed_k6_variant": mixed.k6_variant(), "parts_k6_variant": parts[0].k6_variant(),
           "ms_call_mixed": med("mixed", 0), "ms_call_two_batches": med("parts", 0),
           "ms_walk_mixed": med("mixed", 1), "ms_walk_two_batches": med("parts", 1),
           "ms_call_each_mixed": [round(1e3 * x[0], 3) for x in t["mixed"]], "ms_call_each_two_batches": [round(1e3 * x[0], 3) for x in t["parts"]]}
    res["ms_walk_difference"] = round(res["ms_walk_mixed"] - res["ms_walk_two_batches"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    mixed.close()
    for b in parts:
        b.close()


if __name__ == "__main__":
    main()
