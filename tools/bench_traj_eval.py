"""Trajectory evaluation per call: devo_amd.evaluation (one launch, csrc/traj_eval.hip) against the same computation composed in torch on
the GPU and in numpy on the host.

    python tools/bench_traj_eval.py                              # the table of profiles/traj_eval.txt
    python tools/bench_traj_eval.py --out profiles/traj_eval.txt

Shapes: B = 60 pairs of N = 2 000 poses (a validation run: scenes x trials) and B = 1 pair of N = 100 000 (one long trajectory, one
workgroup); fp32 poses, int64 stamps, nearest association, Sim(3) alignment.  The two compositions compute the association (a sorted
search; the brute-force argmin of tests/traj_eval_ref.py is quadratic), the alignment (an SVD of the 3 x 3 covariance with the reflection
correction) and rmse / mean / median / std / min / max of the errors, pair after pair — not the rotation and RPE columns, which the kernel
computes in the same launch.  `kernel` includes the status read-back of check=True; `kernel nocheck` leaves it out.  A batch of --calls
calls is timed on the host clock until the device has finished; batches of the paths alternate after a warm-up batch each; medians over
the batches with the p90 - p10 spread.  Launches per call: GPU activities (kernels and copies) the profiler records over 3 calls."""
import argparse
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from devo_amd import evaluation as E                                   # noqa: E402


def scene(B, N, seed):
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 40.0, N)
    gt = np.stack([np.cos(s) * (1 + 0.1 * s), np.sin(s), 0.2 * s, 0 * s, 0 * s, 0 * s, 1 + 0 * s], 1)
    t = 50_000 * np.arange(N, dtype=np.int64)
    pairs = []
    for _ in range(B):
        est = gt.copy()
        est[:, :3] = est[:, :3] * 0.5 + 0.01 * rng.standard_normal((N, 3)) + 1.0
        pairs.append((est.astype(np.float32), t + rng.integers(-2000, 2001, N), gt.astype(np.float32), t))
    return pairs


def host_pair(est, est_t, gt, gt_t, max_diff):
    j = np.clip(np.searchsorted(est_t, gt_t), 1, len(est_t) - 1)
    j = np.where(np.abs(est_t[j - 1] - gt_t) <= np.abs(est_t[j] - gt_t), j - 1, j)
    keep = np.abs(est_t[j] - gt_t) <= max_diff
    x, y = est[j[keep], :3].astype(np.float64), gt[keep, :3].astype(np.float64)
    mx, my = x.mean(0), y.mean(0)
    U, D, Vt = np.linalg.svd((y - my).T @ (x - mx) / len(x))
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    c = np.trace(np.diag(D) @ S) / ((x - mx) ** 2).sum(1).mean()
    e = np.linalg.norm(y - (c * x @ R.T + (my - c * R @ mx)), axis=1)
    return np.sqrt((e * e).mean()), e.mean(), np.median(e), e.std(), e.min(), e.max()


def torch_pair(est, est_t, gt, gt_t, max_diff):
    j = torch.searchsorted(est_t, gt_t).clamp(1, len(est_t) - 1)
    j = torch.where((est_t[j - 1] - gt_t).abs() <= (est_t[j] - gt_t).abs(), j - 1, j)
    keep = (est_t[j] - gt_t).abs() <= max_diff
    x, y = est[j[keep], :3].double(), gt[keep, :3].double()
    mx, my = x.mean(0), y.mean(0)
    U, D, Vt = torch.linalg.svd((y - my).T @ (x - mx) / len(x))
    S = torch.ones(3, dtype=torch.float64, device=est.device)
    S[2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    R = (U * S) @ Vt
    c = (D * S).sum() / ((x - mx) ** 2).sum(1).mean()
    e = (y - (c * x @ R.T + (my - c * R @ mx))).norm(dim=1)
    return torch.stack([(e * e).mean().sqrt(), e.mean(), torch.quantile(e, 0.5), e.std(unbiased=False), e.min(), e.max()])


def batch(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def launches(fn, calls=3):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if "cuda" in str(getattr(ev, "device_type", "")).lower()) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="calls per timed batch")
    ap.add_argument("--repeats", type=int, default=7, help="alternating batches per path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_traj_eval needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    lines = [f"# python tools/bench_traj_eval.py  ({torch.cuda.get_device_name(0)}; fp32 poses, int64 stamps, nearest, sim3; ms per call over batches of {a.calls} calls, "
             f"batches of the paths alternating after one warm-up batch each; median (p90 - p10) of {a.repeats} batches)",
             f"{'B':>3} {'N':>7} {'path':>15} {'launches':>9} {'ms per call':>18}"]
    for B, N in ((60, 2000), (1, 100_000)):
        pairs = scene(B, N, seed=B)
        devp = [[torch.from_numpy(x).to(dev) for x in p] for p in pairs]
        packed = [torch.cat([p[k] for p in devp]) for k in range(4)]
        off = [N * b for b in range(B + 1)]
        md = 10_000
        paths = {"kernel": lambda: E.evaluate(*packed, max_diff=md, offsets=(off, off)),
                 "kernel nocheck": lambda: E.evaluate(*packed, max_diff=md, offsets=(off, off), check=False),
                 "torch on GPU": lambda: torch.stack([torch_pair(*p, md) for p in devp]).cpu(),
                 "numpy on host": lambda: [host_pair(*p, md) for p in pairs]}
        got, want = paths["kernel"]().stats[:, 1:7].cpu().numpy(), np.array(paths["numpy on host"]())
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), np.abs(got - want).max()
        assert np.abs(paths["torch on GPU"]().numpy() - want).max() <= 1e-9 * np.abs(want).max()
        times = {k: [] for k in paths}
        for r in range(1 + a.repeats):
            for name, fn in paths.items():
                ms = batch(fn, a.calls)
                if r >= 1:
                    times[name].append(ms)
        for name, fn in paths.items():
            n_l = launches(fn) if name != "numpy on host" else 0.0
            v = times[name]
            lines.append(f"{B:>3} {N:>7} {name:>15} {n_l:>9.1f} {q(v, 0.5):>9.3f} ({q(v, 0.9) - q(v, 0.1):>6.3f})")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
