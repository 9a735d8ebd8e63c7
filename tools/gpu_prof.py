"""Phase profile of k_alloc (library must be built with HX_EXTRA=-DHX_PROFILE hmp3_amd/build.sh)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hmp3_amd import api, synth
import prof_slots
S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
F = int(sys.argv[2]) if len(sys.argv) > 2 else 32
import json
kw = json.loads(os.environ["PROF_KW"]) if "PROF_KW" in os.environ else dict(bitrate=64, short_block_threshold=99999)
pcm = synth.batch_pcm(S, F, unique=16, bursts=bool(int(os.environ.get("PROF_BURSTS", "0"))), rho=float(os.environ.get("PROF_RHO", "0.7")))
b = api.Batch(api.default_control(**kw), nstreams=S, max_frames=F)
b.debug_enable(True)
b.encode_host(pcm)
b.encode_host(pcm)
prof = b.debug_read("prof", np.uint64, S * 64).reshape(S, 64).astype(np.float64)
names = prof_slots.slots()
T = prof_slots.slot("total")
tot = prof[:, T].mean()
print("mean cycles per frame (clock64 ticks), S=%d F=%d" % (S, F))
for k in sorted(names):
    v = prof[:, k].mean() / F
    print("  %-16s %10.0f  %5.1f%%" % (names[k], v, 100 * prof[:, k].mean() / tot))
print("  kernel ticks/frame %.0f" % (tot / F))
ms, n = b.alloc_kernel_ms()
print("k_alloc ms %.3f (%d calls)" % (ms, n))
t = prof[:, T] / F
print("per-stream kernel ticks/frame: min %.0f  mean %.0f  p95 %.0f  max %.0f" % (t.min(), t.mean(), np.percentile(t, 95), t.max()))
