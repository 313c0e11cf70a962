"""Plain-torch fp64 restatement of the per-frame state of the reference's state machine that devo_amd.frames moves to the GPU
(devo/devo.py:502-512 the motion model, :515-520 the depth initialisation, :487-488 intrinsics and timestamp, :342-344 the centre-pixel
point cloud, :276-280 / :534 the relative-pose log, :179-196 get_pose / terminate), built on oracle/se3.py: test infrastructure, the
yardstick of tests/test_gpu_frames.py, pinned to the reference's own classes by tests/golden/frame_state_f64.npz
(tools/gen_golden_frames.py).  The trajectory is completed ITERATIVELY in increasing t — every parent is an earlier frame — so no
recursion limit bounds the depth of a chain."""
import torch
from oracle import se3

IDENTITY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def motion_model(P1, P2, damping=0.5, model="DAMPED_LINEAR"):
    """devo.py:502-512: P1 = poses[n-1], P2 = poses[n-2], [7] or [B, 7] -> poses[n]."""
    if model != "DAMPED_LINEAR":
        return P1.clone()                                                # :511-512
    a, b = P1.reshape(-1, 7), P2.reshape(-1, 7)
    xi = damping * se3.logm(se3.mul(a, se3.inv(b)))                      # :507
    return se3.mul(se3.expm(xi), a).reshape(P1.shape)                    # :508


def lower_median(x):
    """torch.median of a flattened tensor (devo.py:517): the value of rank (count - 1) // 2 in ascending order."""
    v = x.reshape(-1).sort().values
    return v[(v.numel() - 1) // 2]


def begin_frame(poses, patches, intrinsics, tstamps, n, new_patches, new_intrinsics, counter, res, motion_model_name="DAMPED_LINEAR", damping=0.5,
                depth="median"):
    """devo.py:487-488, :502-520 on CPU tensors of any floating dtype, in place: poses [N, 7], patches [N, M, 3, P, P], intrinsics [N, 4],
    tstamps [N]; new_patches [1, M, 3, P, P]."""
    tstamps[n] = counter                                                 # :487
    intrinsics[n] = new_intrinsics / res                                 # :488
    if n > 1:
        poses[n] = motion_model(poses[n - 1], poses[n - 2], damping, motion_model_name)
    new = new_patches.reshape(patches.shape[1:]).clone()
    if isinstance(depth, str):
        new[:, 2] = torch.median(patches[n - 3:n, :, 2])                 # :517-518
    else:
        new[:, 2] = depth.reshape(-1, 1, 1)                              # :515
    patches[n] = new                                                     # :520


def point_cloud(poses, patches, intrinsics, ix, m):
    """devo.py:342-344: poses [1, n, 7], patches [1, Np, 3, P, P], intrinsics [1, n, 4], ix [>= m] -> [m, 3], the centre pixel only."""
    c = patches.shape[-1] // 2
    f = ix[:m]
    x, y, d = patches[0, :m, 0, c, c], patches[0, :m, 1, c, c], patches[0, :m, 2, c, c]
    fx, fy, cx, cy = intrinsics[0, f].unbind(-1)
    X0 = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(d), d], -1)       # projective_ops.py:19-29
    X = se3.act4(se3.inv(poses[0, f]), X0)                               # projective_ops.py:107-109
    return X[:, :3] / X[:, 3:]                                           # devo.py:343


class RefTrajectory:
    def __init__(self):
        self.delta = {}

    def record_removed(self, poses, tstamps, k):                         # devo.py:276-280
        t0, t1 = int(tstamps[k - 1]), int(tstamps[k])
        self.delta[t1] = (t0, se3.mul(poses[k][None], se3.inv(poses[k - 1][None]))[0])

    def record_skipped(self, t, t0, dtype=torch.float64):                # devo.py:534
        self.delta[int(t)] = (int(t0), torch.tensor(IDENTITY, dtype=dtype))

    def complete(self, poses, tstamps, n, counter):
        """devo.py:179-196: get_pose for t = 0 .. counter - 1 in increasing t (a parent is an earlier frame, so its pose is there), then
        the inverse of all.  KeyError for a frame that is neither a keyframe nor in the log, as the reference's dict lookup."""
        traj = {int(tstamps[i]): poses[i] for i in range(n)}             # :189-191
        out = []
        for t in range(counter):
            if t in traj:                                                # :180-181
                out.append(traj[t])
                continue
            t0, dP = self.delta[t]                                       # :183
            if not 0 <= t0 < t:
                raise KeyError(t)
            out.append(se3.mul(dP[None], out[t0][None])[0])              # :184
        return se3.inv(torch.stack(out))                                 # :195-196
