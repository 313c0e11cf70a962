#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference and oracle/).

Writes tests/golden/frame_state_f64.npz: the per-frame state of the reference's state machine (devo/devo.py:502-512 the motion model,
:342-344 the centre-pixel point cloud, :179-196 and :276-280 the relative-pose log and terminate()) evaluated with the REFERENCE's own
`devo.lietorch.SE3` class and `devo.projective_ops.point_cloud` on CPU in fp64, over tools/gen_golden.py's shims (the group VALUES
come from oracle/lie.py's backend; what the fixture pins is the reference's composition of them).  devo/devo.py itself cannot be
imported without a GPU, so its few lines are driven here as written, `get_pose` recursively.  Data only: inputs and expected outputs."""
import math
import os
import sys
import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden import install_shims                # noqa: E402
from devo_amd import synth                          # noqa: E402


def rot_pose(axis, angle, t):
    axis = torch.tensor(axis, dtype=torch.float64)
    axis = axis / axis.norm()
    return torch.cat([torch.tensor(t, dtype=torch.float64), math.sin(angle / 2) * axis, torch.tensor([math.cos(angle / 2)], dtype=torch.float64)])


def main():
    install_shims()
    from devo import projective_ops as pops
    from devo import lietorch
    from devo.lietorch import SE3
    dt = torch.float64
    out = {}

    # ---- the motion model (devo.py:504-509) for four pairs (P1 = poses[n-1], P2 = poses[n-2])
    sp = synth.make_poses(9, 21, trans_step=0.05, rot_step=0.01, dtype=dt)[0]
    P1 = torch.stack([sp[8], sp[3], rot_pose((0.3, -1.0, 0.2), 0.5, (0.2, -0.1, 0.4)), sp[1]])
    P2 = torch.stack([sp[7], sp[3], rot_pose((0.3, -1.0, 0.2), 0.0, (0.0, 0.0, 0.0)), sp[0]])      # pair 1: identical poses; pair 2: a 0.5 rad step
    damping = 0.5
    pred = []
    for a, b in zip(P1, P2):
        A, B = SE3(a[None]), SE3(b[None])
        xi = damping * (A * B.inv()).log()
        pred.append((SE3.exp(xi) * A).data[0])
    out.update(mm_P1=P1.numpy(), mm_P2=P2.numpy(), mm_damping=damping, mm_pred=torch.stack(pred).numpy())

    # ---- the point cloud behind every update (devo.py:342-344), (n 5, M 7)
    n, M, H, W = 5, 7, 48, 64
    poses = synth.make_poses(n, 22, dtype=dt)
    patches, _ = synth.make_patches(n, M, H, W, seed=22, dtype=dt)
    intr = synth.make_intrinsics(n, H, W, dtype=dt)
    ix = torch.arange(n * M) // M
    m = n * M
    points = pops.point_cloud(SE3(poses), patches[:, :m], intr, ix[:m])
    points = (points[..., 1, 1, :3] / points[..., 1, 1, 3:]).reshape(-1, 3)
    out.update(pc_poses=poses.numpy(), pc_patches=patches.numpy(), pc_intrinsics=intr.numpy(), pc_ix=ix.numpy(), pc_points=points.numpy())

    # ---- a 12-frame trajectory: frames 4 and 5 removed one after the other (5 chains to 4, 4 to 3), frame 9 removed, frame 1 skipped by the
    # motion probe (devo.py:534); keyframes 0, 2, 3, 6, 7, 8, 10, 11.  delta and traj as devo.py:276-280 and :189-191 fill them.
    counter = 12
    full = synth.make_poses(counter, 23, trans_step=0.07, rot_step=0.03, dtype=dt)[0]
    delta, alive = {}, list(range(counter))
    delta[1] = (0, SE3.Identity(1, dtype=dt).data[0])
    alive.remove(1)
    for t1 in (5, 4, 9):                                                 # removal order: 5 first (parent 4), then 4 (parent 3)
        k = alive.index(t1)
        t0 = alive[k - 1]
        delta[t1] = (t0, (SE3(full[t1]) * SE3(full[t0]).inv()).data)
        alive.remove(t1)
    traj = {t: full[t] for t in alive}

    def get_pose(t):                                                     # devo.py:179-184
        if t in traj:
            return SE3(traj[t])
        t0, dP = delta[t]
        return SE3(dP) * get_pose(t0)

    done = lietorch.stack([get_pose(t) for t in range(counter)], dim=0).inv().data
    log_t = sorted(delta)
    out.update(tr_counter=counter, tr_kf_tstamps=np.array(alive, dtype=np.int64), tr_kf_poses=torch.stack([full[t] for t in alive]).numpy(),
               tr_log_t=np.array(log_t, dtype=np.int64), tr_log_parent=np.array([delta[t][0] for t in log_t], dtype=np.int64),
               tr_log_rel=torch.stack([delta[t][1].reshape(7) for t in log_t]).numpy(), tr_poses_all=full.numpy(), tr_out=done.reshape(counter, 7).numpy())
    path = os.path.join(ROOT, "tests", "golden", "frame_state_f64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
