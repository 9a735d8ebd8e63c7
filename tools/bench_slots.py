"""Slot operations on a config-3-shaped batch (4096 streams, max_frames 256, int16 PCM in device memory), one MI355X:
  a. all slots reset / saved / restored: the new call (host time until it returns, device time between two events on its
     stream; the host-blob calls: wall time) against a loop of the existing single-slot call in the same library;
  b. the three kernels alone: bytes moved over the device time of (a);
  c. pipelined submits of --frames frames with --share of the slots reset between every two submits: step time with
     hx_batch_reset_streams, with the loop of hx_batch_reset_stream, and with no resets.
The batch is created over a menu of two entries that cost the same to encode (they differ in the copyright bit), every slot on
the first: the "assign" rows hand all slots (a), or the share of (c), the other entry with hx_batch_assign_streams - the
reset kernel with another class in its entries - next to the reset rows of the same run.
Every comparison is alternated --rounds times in one process on one batch.  One JSON document to --out (and stdout).
  python tools/bench_slots.py [--streams 4096] [--max-frames 256] [--frames 64] [--steps 8] [--share 0.05] [--rounds 2]
(d, the regression check of the encode path, is bench.py itself run on this build and on the parent's library through
HMP3AMD_LIB, alternated: see DESIGN.md section 7.)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--max-frames", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from hmp3_amd import api, synth
    S, F = args.streams, args.frames
    L = api.lib()
    b = api.Batch.menu([api.default_control(bitrate=64), api.default_control(bitrate=64, cr_bit=1)], S, max_frames=args.max_frames)
    dev = torch.device("cuda:0")
    q = torch.cuda.current_stream().cuda_stream
    pcm = torch.from_numpy(synth.batch_pcm(S, F, unique=16)).to(dev)
    ostride = b.out_stride(F)
    d_out = [torch.zeros((S, ostride), dtype=torch.uint8, device=dev) for _ in range(2)]
    d_nb = [torch.zeros(S, dtype=torch.int32, device=dev) for _ in range(2)]
    need, stride = int(L.hx_batch_stream_state_bytes(b.h)), b.states_stride()
    d_blobs = torch.zeros(S * stride, dtype=torch.uint8, device=dev)
    h_blobs = np.zeros(S * stride, dtype=np.uint8)
    one = (C.c_ubyte * need)()
    everything = (C.c_int * S)(*range(S))
    entry = [(C.c_int * S)(*([k] * S)) for k in range(2)]
    cur = np.zeros(S, dtype=np.int32)       # the entry each slot runs

    def submit(k):
        b.submit_device(pcm.data_ptr(), F, d_out[k & 1].data_ptr(), ostride, d_nb[k & 1].data_ptr(), q)

    # something in every slot's state
    submit(0); submit(1); b.wait(q)
    torch.cuda.synchronize()
    assert b.status() == 0

    def timed_device(fn):
        """(host ms until the call returns, device ms between two events around it)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        if fn() != 0:
            raise RuntimeError(api.last_error())
        host = time.perf_counter() - t0
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * host, e0.elapsed_time(e1)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def loop(fn):
        def run():
            for i in range(S):
                if fn(i) != 0:
                    raise RuntimeError(api.last_error())
        return run

    def check(rc):
        if rc != 0:
            raise RuntimeError(api.last_error())

    a = {k: [] for k in ("get_device", "get_host_ms", "get_loop_ms", "set_device", "set_host_ms", "set_loop_ms", "reset_device", "reset_loop_ms", "assign_device", "assign_back_device")}
    for _ in range(args.rounds + 1):        # (the first round warms up: staging, device staging of the host calls)
        a["get_device"].append(timed_device(lambda: L.hx_batch_get_stream_states_device(b.h, everything, S, d_blobs.data_ptr(), stride, q)))
        a["get_host_ms"].append(wall(lambda: check(L.hx_batch_get_stream_states(b.h, everything, S, h_blobs.ctypes.data, stride))))
        a["get_loop_ms"].append(wall(loop(lambda i: L.hx_batch_get_stream_state(b.h, i, one))))
        a["set_device"].append(timed_device(lambda: L.hx_batch_set_stream_states_device(b.h, everything, S, d_blobs.data_ptr(), stride, q)))
        a["set_host_ms"].append(wall(lambda: check(L.hx_batch_set_stream_states(b.h, everything, S, h_blobs.ctypes.data, stride))))
        C.memmove(one, h_blobs.ctypes.data, need)     # (slot 0's blob: every slot has the same configuration)
        a["set_loop_ms"].append(wall(loop(lambda i: L.hx_batch_set_stream_state(b.h, i, one))))
        a["reset_device"].append(timed_device(lambda: L.hx_batch_reset_streams(b.h, everything, S, q)))
        a["reset_loop_ms"].append(wall(loop(lambda i: L.hx_batch_reset_stream(b.h, i))))
        a["assign_device"].append(timed_device(lambda: L.hx_batch_assign_streams(b.h, everything, entry[1], S, q)))
        a["assign_back_device"].append(timed_device(lambda: L.hx_batch_assign_streams(b.h, everything, entry[0], S, q)))
    assert b.status() == 0
    res = {"streams": S, "max_frames": args.max_frames, "build_id": api.build_id(), "blob_bytes": need, "blob_stride": stride, "rounds": args.rounds, "all_slots": {}}
    for k, v in a.items():
        v = v[1:]
        if k.endswith("_device"):
            res["all_slots"][k[:-7] + "_new_host_ms"] = [round(x[0], 3) for x in v]
            res["all_slots"][k[:-7] + "_new_device_ms"] = [round(x[1], 3) for x in v]
        else:
            res["all_slots"][k] = [round(x, 2) for x in v]
    # b. bytes the kernels move over the device time above (which also holds the 64 KB list upload): read + written for the
    # gather and the scatter; for the reset the bytes written only - what it reads is one HxStream per class, out of cache
    moved = {"get": S * (need + stride), "set": S * 2 * need, "reset": S * (need - 24)}
    res["kernels"] = {k: {"bytes_moved": moved[k], "device_ms": min(res["all_slots"][k + "_new_device_ms"]),
                          "TB_per_s": round(moved[k] / 1e9 / min(res["all_slots"][k + "_new_device_ms"]), 3)} for k in moved}

    # c. pipelined submits with a share of the slots recycled between every two
    nrec = max(1, int(round(S * args.share)))
    rng = np.random.default_rng(1)

    def steps(variant):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            submit(k)
            if variant != "none" and k + 1 < args.steps:
                idx = rng.choice(S, nrec, replace=False).astype(np.int32)
                if variant == "new":
                    check(L.hx_batch_reset_streams(b.h, idx.ctypes.data, nrec, q))
                elif variant == "assign":
                    cfg = (1 - cur[idx]).astype(np.int32)
                    check(L.hx_batch_assign_streams(b.h, idx.ctypes.data, cfg.ctypes.data, nrec, q))
                    cur[idx] = cfg
                else:
                    for i in idx:
                        check(L.hx_batch_reset_stream(b.h, int(i)))
        b.wait(q)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    steps("none")
    c = {v: [] for v in ("none", "new", "loop", "assign")}
    for _ in range(args.rounds):
        for v in c:
            c[v].append(round(steps(v), 3))
    assert b.status() == 0
    res["pipelined"] = {"frames": F, "steps": args.steps, "slots_reset_between_submits": nrec, "step_ms_no_resets": c["none"],
                        "step_ms_reset_streams": c["new"], "step_ms_loop_of_reset_stream": c["loop"],
                        "step_ms_assign_streams": c["assign"]}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    b.close()


if __name__ == "__main__":
    main()
