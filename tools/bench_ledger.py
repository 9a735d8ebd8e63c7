"""The file ledger at config-2 shape (1024 streams x 256 frames per call, CBR-128 stereo, fp32 device calls): a call with
frame counters and a CRC buffer on a batch without a ledger against the same call on a twin batch with every record open
(k_ledger behind k_crc; files long enough never to end, seek points on, so every call stores points and the table is
halved on the way), alternated call by call in one process; then hx_ledger_update on one core over the same call's
counters - the per-frame host loop (Tagger::after_call and the scan for the end) that the ledger takes off the host - and
the time to read all records.  One JSON line.
  python tools/bench_ledger.py [--streams 1024] [--frames 256] [--steps 8] [--out profiles/ledger_bench.json]
--ledger 0: the plain calls alone (a library picked through HMP3AMD_LIB that predates the ledger: the parent build).
k_ledger's own time: run this under rocprofv3 --kernel-trace --stats (a separate run; the wall times here are not taken
under the profiler)."""
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
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--ledger", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from hmp3_amd import api, synth
    S, F = args.streams, args.frames
    L = api.lib()
    variants = ("plain", "ledger") if args.ledger else ("plain",)
    batch = {v: api.Batch(api.default_control(bitrate=64), nstreams=S, max_frames=F) for v in variants}
    pcm = torch.from_numpy(synth.batch_pcm(S, F, unique=16).astype(np.float32)).cuda()
    stride = batch["plain"].out_stride(F)
    d_out = torch.zeros((S, stride), dtype=torch.uint8, device="cuda")
    d_nb = torch.zeros(S, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros((S, F, 2), dtype=torch.int32, device="cuda")
    d_crc = torch.zeros((S, F), dtype=torch.int16, device="cuda")
    q = torch.cuda.current_stream().cuda_stream
    for b in batch.values():
        b.frame_stats_buffer(d_stats.data_ptr())
        b.crc_buffer(d_crc.data_ptr())
    want = None
    if args.ledger:
        batch["ledger"].ledger_begin(range(S), 1 << 24, head_bytes=417, flags=1, stream=q)
        want = [api.ledger_open(1 << 24, 1, 417, 1) for _ in range(S)]
    t_host = []

    def encode(v):
        if L.hx_batch_encode_f32_device(batch[v].h, pcm.data_ptr(), F, d_out.data_ptr(), stride, d_nb.data_ptr(), q) != 0:
            raise RuntimeError(api.last_error())
        torch.cuda.synchronize()

    def host_update():
        """the host's records keep step with the device's: the same update on one core over the call just made -> seconds"""
        st, cr, nb = d_stats.cpu().numpy(), d_crc.cpu().numpy().view(np.uint16), d_nb.cpu().numpy()
        t0 = time.perf_counter()
        for s in range(S):
            L.hx_ledger_update(C.byref(want[s]), st[s].ctypes.data, cr[s].ctypes.data, F, int(nb[s]))
        return time.perf_counter() - t0
    for v in variants:          # warm-up
        encode(v)
        if v == "ledger":
            host_update()
    t = {v: [] for v in variants}
    for _ in range(args.steps):
        for v in variants:
            t0 = time.perf_counter()
            encode(v)
            t[v].append(time.perf_counter() - t0)
            if v == "ledger":
                t_host.append(host_update())
    for b in batch.values():
        assert b.status() == 0
    res = {"streams": S, "frames": F, "calls": args.steps, "build_id": api.build_id(),
           "ms_counters_and_crc": round(1e3 * float(np.median(t["plain"])), 3), "ms_each_plain": [round(1e3 * x, 3) for x in t["plain"]]}
    if args.ledger:
        res["ms_with_open_records"] = round(1e3 * float(np.median(t["ledger"])), 3)
        res["ms_each_ledger"] = [round(1e3 * x, 3) for x in t["ledger"]]
        res["ratio"] = round(res["ms_with_open_records"] / res["ms_counters_and_crc"], 4)
        res["ms_host_update_one_core"] = round(1e3 * float(np.median(t_host)), 2)
        res["host_frames_per_s"] = round(S * F / float(np.median(t_host)))
        res["host_over_step"] = round(res["ms_host_update_one_core"] / res["ms_counters_and_crc"], 3)
        t0 = time.perf_counter()
        got = batch["ledger"].ledger_read(range(S))
        res["ms_read_all_records"] = round(1e3 * (time.perf_counter() - t0), 2)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], "k_ledger differs from hx_ledger_update"
        res["seek_points"], res["every"], res["fed"] = int(got[0].npt), int(got[0].every), int(got[0].fed)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for b in batch.values():
        b.close()


if __name__ == "__main__":
    main()
