#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Writes tests/golden/rpe_scene.npz: the reference's scripts/evaluate_rpe.py:evaluate_trajectory(gt, est, 0, True, delta, unit, 0.0, 1.0) on a
seeded synthetic scene — 400 ground-truth poses at 100 Hz, 70 estimated poses at every fifth-or-so ground-truth stamp with a jitter below
half the ground-truth interval, position noise of about 1 % of the scene and rotation noise of 0.03 .. 0.06 rad per pose — for the units
"s" and "f" (the script's "m" and "rad" branches call `dict_keys.sort` and do not run under Python 3).  Recorded: the inputs, and per
(unit, delta) the script's rows (stamp_est_0, stamp_est_1, stamp_gt_0, stamp_gt_1, trans, rot in rad).  The seed is the first for which
every relative rotation error the script reports is above 1e-2 rad (its angle is an arccos of a trace, well conditioned only there), every
estimated stamp has exactly one nearest ground-truth stamp and no end-point decision is a tie.  Data only: inputs and recorded results."""
import importlib.util
import os
import sys
import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden import REF                          # noqa: E402
import traj_eval_ref as T                           # noqa: E402

N_GT, N_EST, DT = 400, 70, 0.01
CASES = (("s", 0.25), ("s", 0.5), ("s", 1.0), ("f", 1.0), ("f", 5.0), ("f", 10.0))


def scene(seed):
    rng = np.random.default_rng(seed)
    gt = T.spiral(N_GT)
    gt_t = DT * np.arange(N_GT)
    keep = 10 + 5 * np.arange(N_EST) + rng.integers(0, 3, N_EST)     # every fifth-or-so stamp, inside the ground truth's range
    est_t = gt_t[keep] + rng.uniform(-0.4, 0.4, N_EST) * DT
    est = gt[keep].copy()
    est[:, :3] += 0.02 * rng.standard_normal((N_EST, 3))            # about 1 % of the scene's 2 m extent
    for k in range(N_EST):
        v = rng.standard_normal(3)
        v *= rng.uniform(0.03, 0.06) / np.linalg.norm(v)
        dq = np.concatenate([np.sin(np.linalg.norm(v) / 2) * v / np.linalg.norm(v), [np.cos(np.linalg.norm(v) / 2)]])
        est[k, 3:] = T.qmul(est[k, 3:], dq)
    return est, est_t, gt, gt_t


def main():
    spec = importlib.util.spec_from_file_location("evaluate_rpe", os.path.join(REF, "scripts", "evaluate_rpe.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    for seed in range(100):
        est, est_t, gt, gt_t = scene(seed)
        traj_gt = {float(t): S.transform44([t] + list(p)) for t, p in zip(gt_t, gt)}
        traj_est = {float(t): S.transform44([t] + list(p)) for t, p in zip(est_t, est)}
        if len(traj_est) != N_EST or np.any(np.diff(est_t) <= 0):
            continue
        out = dict(est=est, est_t=est_t, gt=gt, gt_t=gt_t, units=np.array([u for u, _ in CASES]), deltas=np.array([d for _, d in CASES]), seed=seed)
        ok = True
        for k, (unit, delta) in enumerate(CASES):
            rows = np.array(S.evaluate_trajectory(traj_gt, traj_est, 0, True, delta, unit, 0.0, 1.0), np.float64)
            ok = ok and rows[:, 5].min() > 1e-2
            out[f"rows_{k}"] = rows
        d = np.abs(gt_t[None, :] - est_t[:, None])
        d.sort(1)
        ok = ok and (d[:, 1] - d[:, 0]).min() > 1e-6                # one nearest ground-truth stamp each
        if ok:
            break
    else:
        raise SystemExit("no seed gives a well-conditioned scene")
    path = os.path.join(ROOT, "tests", "golden", "rpe_scene.npz")
    np.savez_compressed(path, **out)
    print(path, "seed", seed, {f"{u} {d:g}": len(out[f"rows_{k}"]) for k, (u, d) in enumerate(CASES)}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
