"""The decoded-PCM output at config-2 shape (1024 streams x 256 frames per call, CBR-128 long blocks, fp32 device calls):
a call with a recon buffer (k_recon_hybrid, k_recon_synth, k_recon_carry behind the packing, and the stream walk writing a
frame record per frame) against the same call without, alternated call by call on one batch in one process.  One JSON line:
the step's and the stream walk's milliseconds off and on, and the bytes the recon kernels need to move per call - lines
read, recon written, the hybrid scratch written once and read 51 / 36 times (a frame's synthesis reads its own 36 time
slots and the 15 before them) - against the step's added time.
  python tools/bench_recon.py [--streams 1024] [--frames 256] [--steps 8]
The kernels' own times: run this under rocprofv3 --kernel-trace --stats (a separate run; the wall times here are not
taken under the profiler) and read the k_recon_* rows with tools/kstats.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    args = ap.parse_args()
    import torch
    from hmp3_amd import api, synth
    S, F = args.streams, args.frames
    L = api.lib()
    b = api.Batch(api.default_control(bitrate=64, short_block_threshold=99999), nstreams=S, max_frames=F)
    pcm = torch.from_numpy(synth.batch_pcm(S, F, unique=16).astype(np.float32)).cuda()
    stride = b.out_stride(F)
    d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_recon = torch.zeros((S, F * 1152 * 2), dtype=torch.float32, device="cuda")
    q = torch.cuda.current_stream().cuda_stream

    def call(on):
        b.recon_buffer(d_recon.data_ptr() if on else None)
        if L.hx_batch_encode_f32_device(b.h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())
    for on in (True, False):        # warm-up (the first switch-on allocates)
        call(on)
    torch.cuda.synchronize()
    b.alloc_kernel_ms()
    t, walk = {True: [], False: []}, {True: [], False: []}
    for _ in range(args.steps):
        for on in (True, False):
            t0 = time.perf_counter()
            call(on)
            torch.cuda.synchronize()
            t[on].append(time.perf_counter() - t0)
            walk[on].append(b.alloc_kernel_ms()[0])
    assert b.status() == 0
    G = S * 2 * F       # granules per call
    moved = {"lines_read": G * 2 * 576 * 2, "recon_written": G * 2 * 576 * 4, "scratch_written": G * 2 * 576 * 4, "scratch_read": S * F * 2 * 51 * 32 * 4}
    ms = {on: 1e3 * float(np.median(t[on])) for on in t}
    res = {"streams": S, "frames": F, "calls": args.steps, "build_id": api.build_id(),
           "ms_step_off": round(ms[False], 3), "ms_step_on": round(ms[True], 3), "ratio": round(ms[True] / ms[False], 4),
           "ms_step_off_all": [round(1e3 * v, 2) for v in t[False]], "ms_step_on_all": [round(1e3 * v, 2) for v in t[True]],
           "ms_walk_off": round(float(np.median(walk[False])), 3), "ms_walk_on": round(float(np.median(walk[True])), 3),
           "bytes_moved": moved, "GB_moved": round(sum(moved.values()) / 1e9, 2),
           "GB_per_s_over_added_time": round(sum(moved.values()) / 1e9 / max((ms[True] - ms[False]) / 1e3, 1e-9), 1),
           "recon_nonzero": bool(d_recon[:4].any().item())}
    print(json.dumps(res), flush=True)
    b.close()


if __name__ == "__main__":
    main()
