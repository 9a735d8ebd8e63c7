"""The MusicCRC output at config-2 shape (1024 streams x 256 frames per call, CBR-128 stereo, fp32 device calls): a call
with frame counters and a CRC buffer (k_crc behind the packing) against the same call with frame counters only, alternated
call by call on one batch in one process; then hx_xing_update_crc on one core over the same call's bytes, which is what
the CRC output takes off the host.  One JSON line.
  python tools/bench_crc.py [--streams 1024] [--frames 256] [--steps 8] [--host-crc 1] [--dense 0]
--crc 0: counters-only calls alone (a library picked through HMP3AMD_LIB that predates the CRC output: the parent build).
--dense 1: dense output on in every call, so that k_dense_gather (which reads the same bytes) runs next to k_crc.
k_crc's own time: run this under rocprofv3 --kernel-trace --stats (a separate run; the wall times here are not taken
under the profiler)."""
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
    ap.add_argument("--crc", type=int, default=1)
    ap.add_argument("--dense", type=int, default=0)
    ap.add_argument("--host-crc", type=int, default=1)
    args = ap.parse_args()
    import torch
    from hmp3_amd import api, synth
    S, F = args.streams, args.frames
    L = api.lib()
    b = api.Batch(api.default_control(bitrate=64), nstreams=S, max_frames=F)
    pcm = torch.from_numpy(synth.batch_pcm(S, F, unique=16).astype(np.float32)).cuda()
    stride = b.out_stride(F)
    d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros((S, F, 2), dtype=torch.int32, device="cuda")
    d_crc = torch.zeros((S, F), dtype=torch.int16, device="cuda")
    q = torch.cuda.current_stream().cuda_stream
    b.frame_stats_buffer(d_stats.data_ptr())
    if args.dense:
        d_dense = torch.zeros(b.dense_bound(F), dtype=torch.uint8, device="cuda")
        d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
        b.dense_buffers(d_dense.data_ptr(), d_dense.numel(), d_off.data_ptr())

    def call(with_crc):
        if args.crc:
            b.crc_buffer(d_crc.data_ptr() if with_crc else None)
        if L.hx_batch_encode_f32_device(b.h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())
    variants = (True, False) if args.crc else (False,)
    for v in variants:          # warm-up
        call(v)
    torch.cuda.synchronize()
    t = {v: [] for v in variants}
    for _ in range(args.steps):
        for v in variants:
            t0 = time.perf_counter()
            call(v)
            torch.cuda.synchronize()
            t[v].append(time.perf_counter() - t0)
    assert b.status() == 0
    nb = d_nb.cpu().numpy()
    res = {"streams": S, "frames": F, "calls": args.steps, "build_id": api.build_id(), "dense": args.dense, "bytes_per_call": int(nb.sum()),
           "ms_counters_only": round(1e3 * float(np.median(t[False])), 3)}
    if args.crc:
        res["ms_counters_and_crc"] = round(1e3 * float(np.median(t[True])), 3)
        res["ratio"] = round(res["ms_counters_and_crc"] / res["ms_counters_only"], 4)
    if args.crc and args.host_crc:
        # the last call was a counters-only one: run one with the CRC so that buffer and rows belong together
        call(True)
        torch.cuda.synchronize()
        rows, nb, crc = d_out.cpu().numpy(), d_nb.cpu().numpy(), d_crc.cpu().numpy().view(np.uint16)
        t0 = time.perf_counter()
        host = [int(L.hx_xing_update_crc(0, rows[s].ctypes.data, int(nb[s]))) for s in range(S)]
        res["ms_host_crc_one_core"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["host_crc_MB_per_s"] = round(float(nb.sum()) / 1e6 / (res["ms_host_crc_one_core"] / 1e3), 1)
        res["host_over_step"] = round(res["ms_host_crc_one_core"] / res["ms_counters_only"], 1)
        assert host == crc[:, -1].tolist(), "k_crc differs from hx_xing_update_crc"
    print(json.dumps(res), flush=True)
    b.close()


if __name__ == "__main__":
    main()
