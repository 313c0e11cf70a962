"""A plain numpy fp64 restatement of devo_amd.evaluation (csrc/traj_eval.hip), written for clarity: brute-force argmin association,
np.linalg.svd, np.median / np.std.  It is the oracle of tests/test_gpu_traj_eval.py and is itself checked by tests/test_traj_eval_cpu.py
against closed forms, Horn's quaternion-eigenvector solution and scipy's Slerp.  Nothing here imports the package.

TOLERANCES.  Both sides of the GPU comparison are fp64, so the bound is measured, not chosen: `evaluate(..., formulation="horn")` computes
the same row by a second formulation (Horn 1987: the rotation as the dominant eigenvector of a 4 x 4 matrix; every sum taken in reversed
order; rotation angles and relative poses through rotation / homogeneous matrices instead of quaternion products).  tests/test_traj_eval_cpu.py runs both over exactly the cases of the GPU test's first group (`cases()`: N in SIZES x three
alignments x fp32 / fp64 poses x int64 / fp64 stamps) and asserts that the largest disagreement per column stays within the figures
recorded here; the GPU test allows 16 x the recorded figure (a different reduction tree, Jacobi against LAPACK).
  REL: the largest relative disagreement |a - b| / |a| per column over the noisy cases (every column is far from zero there).
  ABS: the largest absolute disagreement of the error columns over the exact-recovery cases (errors ~ 0), as a fraction of the RMS extent
       of the ground truth about its mean.
Measured (this file's cases, numpy 1.x / LAPACK): see REL and ABS below; the recorded figures are the measured maxima rounded up to one
digit.
"""
import numpy as np

COLUMNS = ("n", "rmse", "mean", "median", "std", "min", "max", "sse", "rot_rmse_deg", "rot_mean_deg", "path_length", "mpe", "scale", "rpe_trans_rmse",
           "rpe_rot_rmse_deg", "rpe_terms")
NO_MATCH, TOO_FEW, DEGENERATE, UNSORTED = 1, 2, 4, 8
RANK_RULE = 1e-10
SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1025)

# measured by tests/test_traj_eval_cpu.py::test_recorded_tolerances (it prints the maxima with -s); see the module docstring
REL = {"rmse": 6e-15, "mean": 8e-15, "median": 2e-13, "std": 2e-14, "min": 3e-12, "max": 5e-14, "sse": 2e-14, "rot_rmse_deg": 2e-14, "rot_mean_deg": 2e-14, "path_length": 5e-16, "mpe": 8e-15, "scale": 7e-16, "rpe_trans_rmse": 7e-15, "rpe_rot_rmse_deg": 2e-15, "transform": 2e-15}
ABS = 2e-14
GPU_FACTOR = 16.0


# ---------------------------------------------------------------------------------------------------------------- rotations
def quat_to_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_to_quat(R):
    """xyzw, w >= 0: the dominant eigenvector of the symmetric 4 x 4 form of R (independent of the kernel's branch formula)"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[3] >= 0 else -q


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def angle_deg(q):
    return np.degrees(2.0 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3])))


def matrix_angle_deg(R):
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return np.degrees(np.arctan2(0.5 * np.linalg.norm(a), 0.5 * (np.trace(R) - 1.0)))


def slerp(q0, q1, alpha):
    """along the shorter arc; identical neighbours give q0"""
    d = float(np.dot(q0, q1))
    if d < 0:
        q1, d = -q1, -d
    v = q1 - d * q0
    s = np.linalg.norm(v)
    if s <= 1e-12:
        return q0
    th = alpha * np.arctan2(s, d)
    q = np.cos(th) * q0 + np.sin(th) * v / s
    return q / np.linalg.norm(q)


# ---------------------------------------------------------------------------------------------------------------- association
def associate_nearest(est_t, gt_t, max_diff):
    """-> (short_is_est, matched [n_short]: the long index or -1)"""
    short_is_est = len(est_t) < len(gt_t)
    short, long = (est_t, gt_t) if short_is_est else (gt_t, est_t)
    matched = np.full(len(short), -1, np.int64)
    for i, s in enumerate(short):
        if len(long):
            d = np.abs(long - s)
            j = int(np.argmin(d))                                    # the first minimum: the lowest index on a tie, the leftmost of equal stamps
            if d[j] <= max_diff:
                matched[i] = j
    return short_is_est, matched


def interpolate_gt(est_t, gt, gt_t):
    """-> (matched [Ne]: the lower bracket or -1, poses [Ne, 7] of the interpolated ground truth, NaN outside its range)"""
    matched = np.full(len(est_t), -1, np.int64)
    poses = np.full((len(est_t), 7), np.nan)
    if len(gt_t) == 0:
        return matched, poses
    for i, s in enumerate(est_t):
        if s < gt_t[0] or s > gt_t[-1]:
            continue
        hit = np.nonzero(gt_t == s)[0]
        if len(hit):
            j = int(hit[0])
            matched[i], poses[i, :3], poses[i, 3:] = j, gt[j, :3], gt[j, 3:] / np.linalg.norm(gt[j, 3:])
            continue
        j = int(np.nonzero(gt_t < s)[0][-1])
        alpha = (s - gt_t[j]) / (gt_t[j + 1] - gt_t[j])
        matched[i] = j
        poses[i, :3] = gt[j, :3] + alpha * (gt[j + 1, :3] - gt[j, :3])
        poses[i, 3:] = slerp(gt[j, 3:] / np.linalg.norm(gt[j, 3:]), gt[j + 1, 3:] / np.linalg.norm(gt[j + 1, 3:]), alpha)
    return matched, poses


# ---------------------------------------------------------------------------------------------------------------- alignment
def umeyama(x, y, align):
    """the estimate's positions x [n, 3] onto y [n, 3] -> (c, R, t) or None when degenerate (Umeyama 1991)"""
    n = len(x)
    if n < 3:
        return None
    mx, my = x.mean(0), y.mean(0)
    var_x = ((x - mx) ** 2).sum(1).mean()
    cov = (y - my).T @ (x - mx) / n
    U, D, Vt = np.linalg.svd(cov)
    if not D[1] > RANK_RULE * D[0]:
        return None
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0])
    R = U @ S @ Vt
    c = float(np.trace(np.diag(D) @ S) / var_x) if align == "sim3" else 1.0
    return c, R, my - c * R @ mx


def horn(x, y, align):
    """the second formulation (Horn 1987): the rotation is the eigenvector of the largest eigenvalue of the 4 x 4 matrix N built from
    M = sum x' y'^T; the scale is the least-squares one for that rotation.  Sums in reversed order."""
    n = len(x)
    if n < 3:
        return None
    mx, my = x[::-1].sum(0) / n, y[::-1].sum(0) / n
    xc, yc = (x - mx)[::-1], (y - my)[::-1]
    M = xc.T @ yc
    if not np.linalg.svd(M, compute_uv=False)[1] > RANK_RULE * np.linalg.svd(M, compute_uv=False)[0]:
        return None
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = M.ravel()
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, v = np.linalg.eigh(N)
    qw, qx, qy, qz = v[:, -1]
    R = quat_to_matrix(np.array([qx, qy, qz, qw]))
    c = float((yc * (xc @ R.T)).sum() / (xc * xc).sum()) if align == "sim3" else 1.0
    return c, R, my - c * R @ mx


# ---------------------------------------------------------------------------------------------------------------- the evaluation
def evaluate(est, est_t, gt, gt_t, max_diff=0.0, align="sim3", association="nearest", rpe_delta=0, formulation="umeyama"):
    """One pair -> dict(stats [16] (COLUMNS), transform [8] = (c, t, q_xyzw of R), status, short_is_est, matched [n_short] (long index or
    -1), errors [n_short] (NaN where unmatched), R).  A flagged pair has NaN in every column but n and in its transform."""
    est, gt = np.asarray(est, np.float64), np.asarray(gt, np.float64)
    est_t, gt_t = np.asarray(est_t).astype(np.float64), np.asarray(gt_t).astype(np.float64)
    rev = (lambda v: v[::-1]) if formulation == "horn" else (lambda v: v)
    out = dict(stats=np.full(16, np.nan), transform=np.full(8, np.nan), status=0, R=None)
    out["stats"][0] = 0
    interp = association == "interpolate"
    out["short_is_est"] = short_is_est = interp or len(est) < len(gt)
    n_short = len(est) if short_is_est else len(gt)
    out["matched"], out["errors"] = np.full(n_short, -1, np.int64), np.full(n_short, np.nan)
    long_t = gt_t if short_is_est else est_t
    if np.any(np.diff(long_t) < 0):
        out["status"] = UNSORTED
        return out
    if interp:
        matched, gt_at = interpolate_gt(est_t, gt, gt_t)
    else:
        _, matched = associate_nearest(est_t, gt_t, max_diff)
    out["matched"] = matched
    short = np.nonzero(matched >= 0)[0]
    n = len(short)
    out["stats"][0] = n
    if n == 0:
        out["status"] = NO_MATCH
        return out
    long = matched[short]
    if interp:
        P, Q = est[short], gt_at[short]
    elif short_is_est:
        P, Q = est[short], gt[long]
    else:
        P, Q = est[long], gt[short]
    P, Q = P.copy(), Q.copy()
    P[:, 3:] /= np.linalg.norm(P[:, 3:], axis=1, keepdims=True)
    Q[:, 3:] /= np.linalg.norm(Q[:, 3:], axis=1, keepdims=True)
    x, y = P[:, :3], Q[:, :3]
    if align == "none":
        c, R, t = 1.0, np.eye(3), np.zeros(3)
    else:
        if n < 3:
            out["status"] = TOO_FEW
            return out
        sol = (horn if formulation == "horn" else umeyama)(x, y, align)
        if sol is None:
            out["status"] = DEGENERATE
            return out
        c, R, t = sol
    e = np.linalg.norm(y - (c * x @ R.T + t), axis=1)
    qR = matrix_to_quat(R)
    if formulation == "horn":                                        # rotation matrices instead of quaternion products
        ang = np.array([matrix_angle_deg(quat_to_matrix(Q[k, 3:]).T @ R @ quat_to_matrix(P[k, 3:])) for k in range(n)])
    else:
        ang = np.array([angle_deg(qmul(qconj(Q[k, 3:]), qmul(qR, P[k, 3:]))) for k in range(n)])
    path = float(rev(np.linalg.norm(np.diff(gt[:, :3], axis=0), axis=1)).sum())
    s = out["stats"]
    mean = rev(e).sum() / n
    s[1], s[2], s[3], s[5], s[6], s[7] = np.sqrt(rev(e * e).sum() / n), mean, np.median(e), e.min(), e.max(), rev(e * e).sum()
    s[4] = np.std(e) if formulation != "horn" else np.sqrt(rev((e - mean) ** 2).sum() / n)
    s[8], s[9], s[10], s[11], s[12] = np.sqrt(rev(ang * ang).sum() / n), rev(ang).sum() / n, path, 100.0 * mean / path, c
    d = int(rpe_delta)
    s[15] = 0
    if 0 < d < n:
        tt, aa = [], []
        for k in range(n - d if formulation != "horn" else 0):
            Rp, Rq = quat_to_matrix(P[k, 3:]), quat_to_matrix(Q[k, 3:])
            tp, qp = Rp.T @ (c * (x[k + d] - x[k])), qmul(qconj(P[k, 3:]), P[k + d, 3:])          # P_k^-1 P_k+d
            tq, qq = Rq.T @ (y[k + d] - y[k]), qmul(qconj(Q[k, 3:]), Q[k + d, 3:])                # Q_k^-1 Q_k+d
            te = quat_to_matrix(qq).T @ (tp - tq)
            tt.append(te @ te)
            aa.append(angle_deg(qmul(qconj(qq), qp)) ** 2)
        if formulation == "horn":                                    # homogeneous 4 x 4 matrices instead of quaternion / vector pairs
            def hom(pose, scale):
                M = np.eye(4)
                M[:3, :3], M[:3, 3] = quat_to_matrix(pose[3:]), scale * pose[:3]
                return M
            for k in range(n - d):
                E = np.linalg.inv(np.linalg.inv(hom(Q[k], 1.0)) @ hom(Q[k + d], 1.0)) @ (np.linalg.inv(hom(P[k], c)) @ hom(P[k + d], c))
                tt.append(E[:3, 3] @ E[:3, 3])
                aa.append(matrix_angle_deg(E[:3, :3]) ** 2)
        s[13], s[14], s[15] = np.sqrt(rev(np.array(tt)).sum() / (n - d)), np.sqrt(rev(np.array(aa)).sum() / (n - d)), n - d
    out["transform"] = np.concatenate([[c], t, qR])
    out["errors"][short] = e
    out["R"] = R
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def spiral(n, planar=False, span=7.0):
    """the ground truth of the tests: positions (cos s (1 + 0.1 s), sin s, 0.2 s) (z = 0 when planar), smoothly turning orientations"""
    s = np.linspace(0.0, span, n)                                    # (no multiple of pi: four poses are not coplanar)
    pos = np.stack([np.cos(s) * (1 + 0.1 * s), np.sin(s), np.zeros(n) if planar else 0.2 * s], 1)
    rv = np.stack([0.3 * np.sin(s), 0.2 * s, 0.1 * np.cos(s)], 1)
    th = np.linalg.norm(rv, axis=1, keepdims=True)
    th = np.where(th < 1e-12, 1e-12, th)
    q = np.concatenate([np.sin(th / 2) * rv / th, np.cos(th / 2)], 1)
    return np.concatenate([pos, q], 1)


SIM3 = (1.7, np.array([0.4, -0.3, 0.25, 0.82]) / np.linalg.norm([0.4, -0.3, 0.25, 0.82]), np.array([0.5, -2.0, 1.0]))   # c, q_xyzw, t


def image_of(gt, noise, seed):
    """an estimate whose Sim(3) image under SIM3 is the ground truth, plus Gaussian noise of `noise` on positions (and 2 `noise` rad on the
    orientations)"""
    c, q, t = SIM3
    R = quat_to_matrix(q)
    rng = np.random.default_rng(seed)
    n = len(gt)
    pos = (gt[:, :3] - t) @ R / c + noise * rng.standard_normal((n, 3))
    quat = np.empty((n, 4))
    for k in range(n):
        dv = noise * rng.standard_normal(3)
        dq = np.concatenate([dv, [1.0]])
        quat[k] = qmul(qmul(qconj(q), gt[k, 3:]), dq / np.linalg.norm(dq))
    return np.concatenate([pos, quat], 1)


def stamps(n, kind, jitter=0, seed=0):
    """int64: microseconds from an epoch-sized origin, 50 ms apart; fp64: seconds.  jitter (microseconds) moves every stamp by a seeded amount."""
    t = 1_700_000_000_000_000 + 50_000 * np.arange(n, dtype=np.int64)
    if jitter:
        t = t + np.random.default_rng(seed).integers(-jitter, jitter + 1, n)
    return t if kind == "int64" else (t - 1_700_000_000_000_000).astype(np.float64) * 1e-6


def case(n, pose_dtype, stamp_kind, noise=0.01):
    """one case of the GPU test's first group -> (est, est_t, gt, gt_t, max_diff): Ne = Ng = n, the estimate's stamps jittered by <= 2 ms"""
    gt = spiral(n)
    est = image_of(gt, noise, seed=n)
    if pose_dtype == "float32":
        gt, est = gt.astype(np.float32), est.astype(np.float32)
    max_diff = 10_000 if stamp_kind == "int64" else 0.010
    return est, stamps(n, stamp_kind, jitter=2000, seed=n + 1), gt, stamps(n, stamp_kind), max_diff


def cases():
    for n in SIZES:
        for align in ("none", "se3", "sim3"):
            for pose_dtype in ("float32", "float64"):
                for stamp_kind in ("int64", "float64"):
                    yield n, align, pose_dtype, stamp_kind


def extent(gt):
    p = np.asarray(gt, np.float64)[:, :3]
    return float(np.sqrt(((p - p.mean(0)) ** 2).sum(1).mean()))
