"""Relative pose error per call: devo_amd.evaluation.relative_errors (three launches, csrc/traj_rel.hip) against the same statistics composed
in torch on the GPU and in numpy on the host.

    python tools/bench_traj_rel.py                              # the table at the head of profiles/traj_rel.txt
    python tools/bench_traj_rel.py --out FILE

Shapes: B = 60 pairs of N = 2 000 poses (a validation run: scenes x trials) and B = 1 pair of N = 100 000 (one long trajectory: one
workgroup prepares it, five evaluate it); fp32 poses, int64 stamps, nearest association, the Umeyama scale, unit "m" along the ground truth,
end "reach", the five relative deltas 0.1 .. 0.5.  The two compositions are one function over torch or numpy, pair after pair: the
association and the end of every sub-trajectory by sorted searches (the brute-force scans of tests/traj_rel_ref.py are quadratic and do not
fit at N = 100 000), the scale by an SVD of the 3 x 3 covariance, the index by a cumulative sum, the errors by batched quaternion
arithmetic, then n / rmse / mean / median / std / min / max of both errors per delta.  `kernel` includes the status read-back of check=True;
`kernel nocheck` leaves it out.  A batch of --calls calls is timed on the host clock until the device has finished; batches of the paths
alternate after a warm-up batch each; medians over the batches with the p90 - p10 spread.  Launches per call: GPU activities (kernels and
copies) the profiler records over 3 calls."""
import argparse
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from devo_amd import evaluation as E                                   # noqa: E402

FRACTIONS = (0.1, 0.2, 0.3, 0.4, 0.5)


def scene(B, N, seed):
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, 40.0, N)
    half = 0.5 * (0.3 * s)                                           # a steady turn about z
    gt = np.stack([np.cos(s) * (1 + 0.1 * s), np.sin(s), 0.2 * s, 0 * s, 0 * s, np.sin(half), np.cos(half)], 1)
    t = 50_000 * np.arange(N, dtype=np.int64)
    pairs = []
    for _ in range(B):
        est = gt.copy()
        est[:, :3] = est[:, :3] * 0.5 + 0.01 * rng.standard_normal((N, 3)) + 1.0
        est[:, 3:5] += 0.01 * rng.standard_normal((N, 2))
        pairs.append((est.astype(np.float32), t + rng.integers(-2000, 2001, N), gt.astype(np.float32), t))
    return pairs


def qmul(xp, a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return xp.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot_inv(xp, q, v):
    """R(q)^T v"""
    cross = lambda a, b: xp.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                   a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    u, w = -q[..., :3], q[..., 3:]
    c = cross(u, v)
    return v + 2.0 * (w * c + cross(u, c))


def compose(xp, est, est_t, gt, gt_t, max_diff):
    tor = xp is torch
    f64 = (lambda a: a.double()) if tor else (lambda a: a.astype(np.float64))
    where = (lambda m: torch.nonzero(m).squeeze(1)) if tor else (lambda m: np.nonzero(m)[0])
    sort = (lambda a: a.sort().values) if tor else np.sort
    norm = lambda a: xp.sqrt((a * a).sum(-1))
    j = xp.searchsorted(est_t, gt_t).clip(1, len(est_t) - 1)
    j = xp.where(abs(est_t[j - 1] - gt_t) <= abs(est_t[j] - gt_t), j - 1, j)
    keep = abs(est_t[j] - gt_t) <= max_diff
    P, Q = f64(est[j[keep]]), f64(gt[keep])
    x, y, n = P[:, :3], Q[:, :3], len(P)
    mx, my = x.mean(0), y.mean(0)
    U, D, Vt = xp.linalg.svd((y - my).T @ (x - mx) / n)
    c = (D[0] + D[1] + D[2] * xp.sign(xp.linalg.det(U) * xp.linalg.det(Vt))) / ((x - mx) ** 2).sum(1).mean()
    conj = xp.asarray([-1.0, -1.0, -1.0, 1.0]) if not tor else torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=torch.float64, device=est.device)
    qx, qy = P[:, 3:] / norm(P[:, 3:])[:, None], Q[:, 3:] / norm(Q[:, 3:])[:, None]
    u = xp.cumsum(norm(y[1:] - y[:-1]), 0)
    u = xp.concatenate([0 * u[:1], u]) if not tor else torch.cat([0 * u[:1], u])
    rows = []
    for f in FRACTIONS:
        delta = f * (u[-1] - u[0])
        end = xp.searchsorted(u, u + delta)
        i = where(end < n)
        e = end[i]
        ta, qa = c * qrot_inv(xp, qx[i], x[e] - x[i]), qmul(xp, qx[i] * conj, qx[e])
        tb, qb = qrot_inv(xp, qy[i], y[e] - y[i]), qmul(xp, qy[i] * conj, qy[e])
        qe = qmul(xp, qa * conj, qb)
        te, re = norm(qrot_inv(xp, qa, tb - ta)), 2.0 * xp.arctan2(norm(qe[:, :3]), abs(qe[:, 3])) * (180.0 / np.pi)
        row = [0 * delta + len(i)]
        for v in (te, re):
            s, m = sort(v), len(v)
            mean = v.mean()
            row += [xp.sqrt((v * v).mean()), mean, 0.5 * (s[(m - 1) // 2] + s[m // 2]), xp.sqrt(((v - mean) ** 2).mean()), s[0], s[-1]]
        rows.append(xp.stack(row))
    return xp.stack(rows)


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
    ap.add_argument("--calls", type=int, default=3, help="calls per timed batch")
    ap.add_argument("--repeats", type=int, default=5, help="alternating batches per path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_traj_rel needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    lines = [f"# python tools/bench_traj_rel.py  ({torch.cuda.get_device_name(0)}; fp32 poses, int64 stamps, nearest, sim3 scale, unit m along gt, reach, "
             f"5 relative deltas; ms per call over batches of {a.calls} calls, batches of the paths alternating after one warm-up batch each; "
             f"median (p90 - p10) of {a.repeats} batches)",
             f"{'B':>3} {'N':>7} {'path':>15} {'launches':>9} {'ms per call':>18}"]
    for B, N in ((60, 2000), (1, 100_000)):
        pairs = scene(B, N, seed=B)
        devp = [[torch.from_numpy(x).to(dev) for x in p] for p in pairs]
        packed = [torch.cat([p[k] for p in devp]) for k in range(4)]
        off = [N * b for b in range(B + 1)]
        md = 10_000
        kw = dict(deltas=FRACTIONS, unit="m", relative=True, max_diff=md, offsets=(off, off))
        paths = {"kernel": lambda: E.relative_errors(*packed, **kw),
                 "kernel nocheck": lambda: E.relative_errors(*packed, check=False, **kw),
                 "torch on GPU": lambda: torch.stack([compose(torch, *p, md) for p in devp]).cpu(),
                 "numpy on host": lambda: np.stack([compose(np, *p, md) for p in pairs])}
        got, want = paths["kernel"]().stats[:, :, :13].cpu().numpy(), paths["numpy on host"]()
        assert np.array_equal(got[:, :, 0], want[:, :, 0]) and np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), np.abs(got - want).max()
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
