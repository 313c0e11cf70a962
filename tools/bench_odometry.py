"""Milliseconds per steady-state frame of the online tracker on a synthetic sequence at 480 x 640, M = 96 (config defaults otherwise,
MIXED_PRECISION on): odometry.DEVO against tests/odometry_ref.py's ReferenceTracker — devo/devo.py's control flow in eager torch over the
package's drop-in entry points, today's way of running a sequence.

    python tools/bench_odometry.py                     # -> the table of profiles/odometry.txt
    python tools/bench_odometry.py --frames 60 --repeats 5

One network (seeded random weights, the two-row output layers scaled by 0.05 so that the adjustment stays in its basin) and one sequence (a
sparse texture sliding under the camera) for both; every probe is accepted (scale 1e-3), so frame 8 initialises and every later frame is a
steady-state frame: input, Patchifier, frame store, rings, window edges, one update, the keyframe test.  A run tracks the whole sequence
with a fresh tracker; the steady-state frames are timed from the host as ONE window between two device synchronisations (wall time, what a
user waits for), divided by their number.  The two trackers alternate, run after run; the first run of each is warm-up (code objects,
MIOpen's choices, the Patchifier's captured graph); the figure is the median over the remaining runs, with the spread next to it."""
import argparse
import json
import os
import sys
import time
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from devo_amd import odometry                                            # noqa: E402
from devo_amd.training import TrainNet                                   # noqa: E402
from odometry_ref import ReferenceTracker                                # noqa: E402

DEV = "cuda"
H, W, BINS, M, STEP, INIT = 480, 640, 5, 96, 3, 8


def sequence(frames, density=0.3, seed=5):
    g = torch.Generator().manual_seed(seed)
    tex = torch.randn(BINS, H + frames, W + STEP * frames, generator=g)
    tex = tex * (torch.rand(tex.shape, generator=g) < density)
    K = torch.tensor([320.0, 320.0, W / 2, H / 2], device=DEV)
    return [(tex[:, i // 2:i // 2 + H, STEP * i:STEP * i + W].contiguous().to(DEV), K, 1e4 * i) for i in range(frames)]


def one_run(make, seq, thresh):
    """-> (ms per steady-state frame, n at the end)."""
    t = make(odometry.Config(PATCHES_PER_FRAME=M, KEYFRAME_THRESH=thresh))
    t0 = None
    for i, (v, K, ts) in enumerate(seq):
        if t.is_initialized and t0 is None:
            torch.cuda.synchronize()
            t0, first = time.perf_counter(), i
        torch.manual_seed(i)
        t(ts, v, K, scale=1e-3)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (len(seq) - first), t.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=4, help="timed runs per tracker (one more, the first, is warm-up)")
    a = ap.parse_args()
    torch.manual_seed(0)
    net = TrainNet(p=3, dim=384).to(DEV).eval()
    with torch.no_grad():
        for p in net.update.parameters():
            if p.dim() == 2 and p.shape[0] == 2:
                p.mul_(0.05)
    seq = sequence(a.frames)
    makers = {"odometry.DEVO": lambda cfg: odometry.DEVO(cfg, net, ht=H, wd=W), "ReferenceTracker": lambda cfg: ReferenceTracker(cfg, net, ht=H, wd=W)}
    print(f"# python tools/bench_odometry.py  ({torch.cuda.get_device_name(0)}; {H} x {W}, M = {M}, fp16 rings; {a.frames} frames, the {a.frames - INIT} after "
          f"initialisation timed as one window of host wall time closed by a device synchronisation; {a.repeats} alternating runs after one warm-up run each)")
    print(f"{'keyframes':>10} {'tracker':>17} {'n':>4} {'median ms/frame':>16} {'min':>8} {'max':>8}")
    rows = []
    for branch, thresh in (("removed", 1e9), ("kept", 0.0)):
        times = {k: [] for k in makers}
        ends = {}
        for r in range(a.repeats + 1):
            for name, make in makers.items():
                ms, ends[name] = one_run(make, seq, thresh)
                if r:
                    times[name].append(ms)
        for name in makers:
            t = torch.tensor(times[name], dtype=torch.float64)
            rows.append({"keyframes": branch, "tracker": name, "n": ends[name], "median_ms": float(t.median()), "min_ms": float(t.min()), "max_ms": float(t.max()), "runs": times[name]})
            print(f"{branch:>10} {name:>17} {ends[name]:>4} {rows[-1]['median_ms']:>16.3f} {rows[-1]['min_ms']:>8.3f} {rows[-1]['max_ms']:>8.3f}", flush=True)
        print(f"{'':>10} {'ratio':>17} {'':>4} {rows[-1]['median_ms'] / rows[-2]['median_ms']:>15.2f}x")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
