"""Per-stream phase profile of k_alloc on the bench's own signal set (1024 distinct streams): where the slowest streams
spend their time.  Library built with HX_EXTRA=-DHX_PROFILE."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from hmp3_amd import api
import prof_slots
S, F = 1024, int(os.environ.get("PF", "256"))
dev = torch.device("cuda:0")
CFG = int(os.environ.get("PF_CFG", "2"))         # 2: CBR-128 long blocks; 3: VBR-50 with block switching (1024 of its streams)
w = bench.workload(CFG)
kw, sr = w["classes"][0]
rho_list = [float(os.environ["PF_RHO"])] if "PF_RHO" in os.environ else w["rho"]     # PF_RHO=1.0: the loud near-mono case
pcm = bench.synth_batch_gpu(torch, np, S, F, [sr] * S, [rho_list[i % len(rho_list)] for i in range(S)], w["bursts"], dev)
st = torch.cuda.current_stream().cuda_stream
b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=F)
b.debug_enable(True)
stride = b.out_stride(F)
out = torch.empty((S, stride), dtype=torch.uint8, device=dev); nb = torch.zeros((S,), dtype=torch.int32, device=dev)
for c in range(3):
    b.encode_device(pcm.data_ptr(), F, out.data_ptr(), stride, nb.data_ptr(), st)
torch.cuda.synchronize()
prof = b.debug_read("prof", np.uint64, S * 64).reshape(S, 64).astype(np.float64)
names = prof_slots.slots()
T = prof_slots.slot("total")
order = np.argsort(prof[:, T])
top = order[-10:]
print("streams by kernel total (k cycles per frame): min %.0f  mean %.0f  p95 %.0f  p99 %.0f  max %.0f" % tuple(x / F / 1e3 for x in (
    prof[:, T].min(), prof[:, T].mean(), np.percentile(prof[:, T], 95), np.percentile(prof[:, T], 99), prof[:, T].max())))
print("%-16s %10s %10s   slowest streams: %s" % ("per frame", "mean", "slowest10", " ".join(str(int(s)) for s in top[::-1])))
for k in sorted(names):
    print("%-16s %10.0f %10.0f   %s" % (names[k], prof[:, k].mean() / F, prof[top, k].mean() / F, " ".join("%6.0f" % (prof[s, k] / F) for s in top[::-1][:6])))
