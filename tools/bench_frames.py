"""Cost of the per-frame state calls of devo_amd.frames against the reference's own eager sequences on the same GPU.

    python tools/bench_frames.py                 # the table of profiles/frame_state.txt

(a) eager:  the reference's lines (devo/devo.py:487-488, :502-520; :342-344; :179-196) composed from devo_amd.lietorch,
            devo_amd.projective_ops and torch.median — what a user of the state machine runs without devo_amd.frames;
(b) frames: devo_amd.frames.begin_frame / point_cloud / Trajectory.complete.
Shapes: begin_frame at M = 96, n = 22; point_cloud at M = 96 with n = 22 and n = 1000; complete at counter = 5000 with every second
frame removed.  A call is timed from the host with a device synchronisation in front and behind; warm-up calls first, then the median
and the spread (p90 - p10) over the timed repeats.  Launches per call are counted with torch.profiler over one call (kernels only)."""
import argparse
import json
import os
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import synth, frames                                      # noqa: E402
from devo_amd import projective_ops as pops                             # noqa: E402
from devo_amd import lietorch                                           # noqa: E402
from devo_amd.lietorch import SE3                                       # noqa: E402

DEV = "cuda"
M, P, H, W, RES, DAMPING = 96, 3, 120, 160, 4.0, 0.5


def measure(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    t = torch.tensor(times, dtype=torch.float64)
    q = lambda p: float(torch.quantile(t, p))
    return {"min_us": float(t.min()), "median_us": q(0.5), "spread_us": q(0.9) - q(0.1)}


def launches(fn):
    """Kernels of one call, counted by torch.profiler in a pass of its own (-1: the profiler is not available here)."""
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")))
    except Exception as e:                                              # noqa: BLE001
        print(f"# launches not counted: {type(e).__name__}: {e}", file=sys.stderr)
        return -1


def state(n):
    nbuf = n + 2
    poses = synth.make_poses(nbuf, 11, trans_step=0.01, rot_step=0.002)[0].contiguous().to(DEV)
    patches = synth.make_patches(nbuf, M, H, W, seed=11)[0].view(nbuf, M, 3, P, P).contiguous().to(DEV)
    intr = synth.make_intrinsics(nbuf, H, W)[0].contiguous().to(DEV)
    tstamps = torch.arange(nbuf, dtype=torch.int64, device=DEV)
    return poses, patches, intr, tstamps


def bench_begin(n, repeats, warmup):
    poses, patches, intr, tstamps = state(n)
    new = synth.make_patches(1, M, H, W, seed=12)[0].to(DEV)
    K = torch.tensor([320.0, 320.0, 320.0, 240.0], device=DEV)

    def eager():                                                        # devo.py:487-488, :502-520
        tstamps[n] = 77
        intr[n] = K / RES
        P1, P2 = SE3(poses[n - 1]), SE3(poses[n - 2])
        xi = DAMPING * (P1 * P2.inv()).log()
        poses[n] = (SE3.exp(xi) * P1).data
        p = new.clone()
        p[:, :, 2] = torch.rand_like(p[:, :, 2, 0, 0, None, None])
        p[:, :, 2] = torch.median(patches[n - 3:n, :, 2])
        patches[n] = p

    ours = lambda: frames.begin_frame(poses, patches, intr, tstamps, n, new, K, 77, RES, damping=DAMPING)
    return {"call": "begin_frame", "shape": f"M={M} n={n}", "eager": measure(eager, repeats, warmup), "frames": measure(ours, repeats, warmup),
            "eager_launches": launches(eager), "frames_launches": launches(ours)}


def bench_points(n, repeats, warmup):
    poses, patches, intr, _ = state(n)
    m = n * M
    ix = torch.arange((n + 2) * M, device=DEV) // M
    out = torch.zeros((n + 2) * M, 3, device=DEV)
    Pv, Qv, Kv = poses[None], patches.view(1, -1, 3, P, P), intr[None]

    def eager():                                                        # devo.py:342-344
        pts = pops.point_cloud(SE3(Pv), Qv[:, :m], Kv, ix[:m])
        pts = (pts[..., 1, 1, :3] / pts[..., 1, 1, 3:]).reshape(-1, 3)
        out[:len(pts)] = pts[:]

    ours = lambda: frames.point_cloud(poses, patches, intr, ix, m, out)
    return {"call": "point_cloud", "shape": f"M={M} n={n}", "eager": measure(eager, repeats, warmup), "frames": measure(ours, repeats, warmup),
            "eager_launches": launches(eager), "frames_launches": launches(ours)}


def bench_complete(counter, repeats, warmup):
    kf = list(range(0, counter, 2))                                     # every second frame removed: frame t hangs on t - 1
    n = len(kf)
    poses = synth.make_poses(n, 13, trans_step=0.01, rot_step=0.002)[0].contiguous().to(DEV)
    tstamps = torch.tensor(kf, dtype=torch.int64, device=DEV)
    rel = synth.make_poses(counter, 14, trans_step=1e-5, rot_step=1e-6)[0].contiguous().to(DEV)
    tr = frames.Trajectory(counter, DEV)
    odd = torch.arange(1, counter, 2, device=DEV)
    tr.parent[odd] = odd - 1
    tr.rel.copy_(rel)
    delta = {t: (t - 1, rel[t]) for t in range(1, counter, 2)}          # the reference's dict of device tensors
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))

    def eager():                                                        # devo.py:179-196
        traj = {}
        for i in range(n):
            traj[tstamps[i].item()] = poses[i]

        def get_pose(t):
            if t in traj:
                return SE3(traj[t])
            t0, dP = delta[t]
            return SE3(dP) * get_pose(t0)

        ps = lietorch.stack([get_pose(t) for t in range(counter)], dim=0)
        return ps.inv().data

    ours = lambda: tr.complete(poses, tstamps, n, counter)
    reps = max(3, repeats // 20)                                        # the eager walk takes seconds
    return {"call": "complete", "shape": f"counter={counter} every 2nd removed", "eager": measure(eager, reps, 1), "frames": measure(ours, repeats, warmup),
            "eager_launches": launches(eager), "frames_launches": launches(ours), "eager_repeats": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--counter", type=int, default=5000)
    a = ap.parse_args()
    rows = [bench_begin(22, a.repeats, a.warmup), bench_points(22, a.repeats, a.warmup), bench_points(1000, a.repeats, a.warmup),
            bench_complete(a.counter, a.repeats, a.warmup)]
    print(f"# python tools/bench_frames.py  ({torch.cuda.get_device_name(0)}; medians and p90 - p10 over {a.repeats} repeats after {a.warmup} warm-up calls "
          f"(the eager complete: {rows[-1]['eager_repeats']} repeats); us per call, host wall time between two device synchronisations; launches: kernels of one call)")
    print(f"{'call':>12} {'shape':>34} {'impl':>7} {'launches':>8} {'min':>11} {'median':>11} {'p90-p10':>10}")
    for r in rows:
        for impl in ("eager", "frames"):
            t = r[impl]
            print(f"{r['call']:>12} {r['shape']:>34} {impl:>7} {r[impl + '_launches']:>8} {t['min_us']:>11.1f} {t['median_us']:>11.1f} {t['spread_us']:>10.1f}")
        ratio = r["eager"]["median_us"] / r["frames"]["median_us"]
        print(f"{'':>12} {'':>34} {'ratio':>7} {'':>8} {'':>11} {ratio:>10.2f}x" + ("   (frames is SLOWER than the eager sequence here)" if ratio < 1 else ""))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
