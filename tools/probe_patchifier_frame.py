"""The Patchifier's per-frame call (one 480 x 640 frame under autocast fp16, M = 96): host and wall time per call, launches and GPU time per
call, and the call replayed from a captured graph.

    python tools/probe_patchifier_frame.py [topk | multi | nms]        # the evaluation selection mode on the 2 x 2 grid (default topk)
    DEVO_PATCHIFIER_SELECT=0 python tools/probe_patchifier_frame.py multi   # the same with the selection as the torch composition
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from devo_amd.patchifier import Patchifier
MODE = sys.argv[1] if len(sys.argv) > 1 else "topk"
dev = torch.device("cuda", 0)
torch.manual_seed(0)
pf = Patchifier().to(dev).eval()
images = torch.randn(1, 1, 5, 480, 640, device=dev)
def run():
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return pf(images, 96, scorer_eval_mode=MODE)
for _ in range(5): run()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20): run()
th = time.perf_counter() - t0
torch.cuda.synchronize()
ta = time.perf_counter() - t0
print(f"eager ({MODE}): host {th/20*1e3:.3f} ms, wall {ta/20*1e3:.3f} ms")
from torch.profiler import profile, ProfilerActivity
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    for _ in range(5): run()
    torch.cuda.synchronize()
tot = 0; n = 0; names = {}
for ev in prof.events():
    if "cuda" in str(getattr(ev, "device_type", "")).lower():
        d = float(getattr(ev, "device_time", 0.0) or 0.0); tot += d; n += 1
        names[ev.name[:70]] = names.get(ev.name[:70], 0) + d
print(f"kernels per call {n/5:.0f}, GPU busy per call {tot/5/1e3:.3f} ms")
for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:14]:
    print(f"  {v/5:8.1f} us  {k}")
# graph capture
try:
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
        with torch.cuda.graph(g, stream=s):
            out = run()
    torch.cuda.current_stream().wait_stream(s)
    g.replay(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20): g.replay()
    torch.cuda.synchronize()
    print(f"graph replay: {(time.perf_counter()-t0)/20*1e3:.3f} ms")
except Exception as ex:
    print("graph capture failed:", type(ex).__name__, str(ex)[:300])
