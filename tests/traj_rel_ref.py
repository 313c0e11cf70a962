"""A plain numpy restatement of devo_amd.evaluation.relative_errors (csrc/traj_rel.hip), written for clarity: association and the Umeyama
scale from tests/traj_eval_ref.py, `np.cumsum` for the index, a linear scan / `np.argmin` for the end of every sub-trajectory, rotation
matrices for the relative motions, `np.median` / `np.std`.  It is the oracle of tests/test_gpu_traj_rel.py and is itself checked by
tests/test_traj_rel_cpu.py against results recorded from the reference's scripts/evaluate_rpe.py (tests/golden/rpe_scene.npz; units "s" and
"f" only: that script's "m" and "rad" branches do not run under Python 3, so for those units this restatement is the only oracle).  Nothing
here imports the package.

The stages for one pair (the text of the feature, not the reference's script):
  1. association, exactly traj_eval_ref's -> n matches (x_k, y_k, s_k) in short order, s_k the estimate's stamp;
  2. the scale c: "sim3" (Umeyama over the matches, three matches needed) or a given number (two matches suffice, no alignment);
  3. the index u_k: "f" k; "s" s_k; "m" the cumulative path length, "rad" / "deg" the cumulative rotation angle between consecutive
     matches, along the ground truth's matched poses or the estimate's (with "est" and "m": times c);  relative=True: every delta is a
     fraction of u_{n-1} - u_0;
  4. the end of the sub-trajectory that starts at i: "reach" the first j > i with u_j - u_i >= delta; "closest" the j whose u_j is nearest
     to u_i + delta (the lowest index on a tie), the pair dropped when j = n - 1;
  5. E = (c . (X_i^-1 X_j))^-1 (Y_i^-1 Y_j), c multiplying the translation of the estimate's relative motion: |t_E| and the angle of R_E in
     degrees as 2 atan2(|q_v|, |q_w|);
  6. per delta: COLUMNS.

TOLERANCES.  `relative(..., dtype=np.longdouble)` runs stages 3 - 6 (and the normalisation of the quaternions) in extended precision; stages
1 and 2 (index decisions; an SVD) stay fp64 in both.  tests/test_traj_rel_cpu.py::test_recorded_tolerances runs both over every case of the
GPU test's first group and records the largest relative gap |a - b| / |a| per column group; TOL below are those figures rounded up to two
digits, and the GPU test allows GPU_FACTOR = 8 times them.  Measured on x86-64 (80-bit long double), numpy 1.x.
"""
import numpy as np

import traj_eval_ref as T

COLUMNS = ("n", "trans_rmse", "trans_mean", "trans_median", "trans_std", "trans_min", "trans_max", "rot_rmse_deg", "rot_mean_deg", "rot_median_deg",
           "rot_std_deg", "rot_min_deg", "rot_max_deg", "delta", "span_mean", "scale")
GROUPS = {"trans": (1, 2, 3, 4, 5, 6), "rot": (7, 8, 9, 10, 11, 12), "index": (13, 14)}
NO_PAIR = 128
UNITS = ("f", "s", "m", "rad", "deg")
SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1000)
FRACTIONS = (0.1, 0.2, 0.3, 0.4, 0.5)                              # RPG's sub-trajectory lengths, as fractions of the whole
MARGIN = 1e-9                                                      # of the index range: every end-point decision of a test case must be this clear

# measured by tests/test_traj_rel_cpu.py::test_recorded_tolerances (it prints the maxima with -s); see the module docstring
TOL = {"trans": 1.7e-13, "rot": 1.1e-13, "index": 1.6e-15}    # measured 1.660e-13, 1.007e-13, 1.537e-15
GPU_FACTOR = 8.0
# Under "closest" a sub-trajectory can end where it starts (j = i): E is then the identity up to rounding, |t_E| is exactly 0 on every side and
# the angle is whatever rounding leaves of q_i^-1 q_i, nothing a relative bound can hold.  A product of three or four unit quaternions carries
# at most ~8 eps of absolute error per component, so such an angle is below 2 sqrt(3) 8 eps rad = 3.5e-13 degrees (test_gpu_traj_eval.py's
# ROT_ABS_DEG = 1e-12): two rotation figures that are both below this floor agree, in the measurement above and in the GPU comparison alike.
FLOOR = {"trans": 0.0, "rot": 1e-12, "index": 0.0}


def gap(want, got, group):
    """the relative disagreement of two figures of a column group (0 when both are below the group's floor)"""
    want, got = float(want), float(got)
    if abs(want) <= FLOOR[group] and abs(got) <= FLOOR[group]:
        return 0.0
    return abs(want - got) / abs(want) if want != 0 else abs(got)


# ---------------------------------------------------------------------------------------------------------------- small algebra, any dtype
def _matrix(q):
    """[..., 4] xyzw -> [..., 3, 3]"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one = q.dtype.type(1)
    rows = [[one - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), one - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), one - 2 * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def _qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def _qconj(q):
    return q * np.array([-1, -1, -1, 1], dtype=q.dtype)


def _angle_rad(q):
    return 2 * np.arctan2(np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2]), np.abs(q[..., 3]))


def _deg(a, dtype):
    return a * (dtype(180) / (np.pi if dtype is np.float64 else dtype("3.14159265358979323846264338327950288")))


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _tmul(R, v):
    """R^T v, batched"""
    return (R * v[..., :, None]).sum(-2)


# ---------------------------------------------------------------------------------------------------------------- the matches
def matches(est, est_t, gt, gt_t, max_diff, association, align):
    """stages 1 and 2 in fp64 through traj_eval_ref -> (status, P [n, 7], Q [n, 7], s [n], c or None): the estimate's and the ground truth's
    matched poses (quaternions as given, not normalised), the estimate's matched stamps, the Umeyama scale when align is "sim3" """
    est, gt = np.asarray(est, np.float64), np.asarray(gt, np.float64)
    est_t, gt_t = np.asarray(est_t).astype(np.float64), np.asarray(gt_t).astype(np.float64)
    base = T.evaluate(est, est_t, gt, gt_t, max_diff=max_diff, align=align, association=association)
    if base["status"]:
        return base["status"], None, None, None, None
    matched = base["matched"]
    short = np.nonzero(matched >= 0)[0]
    long = matched[short]
    if association == "interpolate":
        P, Q, s = est[short], T.interpolate_gt(est_t, gt, gt_t)[1][short], est_t[short]
    elif base["short_is_est"]:
        P, Q, s = est[short], gt[long], est_t[short]
    else:
        P, Q, s = est[long], gt[short], est_t[long]
    return 0, P, Q, s, (float(base["stats"][12]) if align == "sim3" else None)


def index_of(P, Q, s, c, unit, along, dtype):
    """stage 3: u [n], non-decreasing (not checked here).  P, Q: normalised, in `dtype` """
    n = len(P)
    if unit == "f":
        return np.arange(n).astype(dtype)
    if unit == "s":
        return s.astype(dtype)
    A = P if along == "est" else Q
    if unit == "m":
        inc = _norm(A[1:, :3] - A[:-1, :3])
        if along == "est":
            inc = dtype(c) * inc
    else:
        inc = _angle_rad(_qmul(_qconj(A[:-1, 3:]), A[1:, 3:]))
        if unit == "deg":
            inc = _deg(inc, dtype)
    return np.concatenate([np.zeros(1, dtype), np.cumsum(inc, dtype=dtype)])


def ends_of(u, delta, end):
    """stage 4 for every start -> (j [n] or -1, margins [n]: how far the nearest other outcome of each decision is, in the index's unit).
    Equal values of u never count as another outcome: both rules name the lowest index among them, which needs no arithmetic."""
    n = len(u)
    rows, k = np.arange(n), np.arange(n)[None, :]
    if end == "reach":
        over = u[None, :] - u[:, None] - delta                       # [i, k]: (u_k - u_i) - delta, the subtraction the rule makes first
        ok = (u[None, :] - u[:, None] >= delta) & (k > rows[:, None])
        j = np.where(ok.any(1), ok.argmax(1), -1)                    # the first
        last = np.where(j >= 0, j, n - 1)                            # (none: the decision was about the last match)
        margin = np.abs(over[rows, last]).astype(np.float64)
        before = (j >= 0) & (j - 1 > rows)
        margin[before] = np.minimum(margin[before], np.abs(over[rows[before], j[before] - 1]).astype(np.float64))
        margin[(j < 0) & (rows == n - 1)] = np.inf
        return j, margin
    dist = np.abs(u[None, :] - (u[:, None] + delta))
    j = dist.argmin(1)                                               # the first minimum: the lowest index on a tie
    others = np.where(u[None, :] != u[j][:, None], dist, np.inf)
    margin = (others.min(1) - dist[rows, j]).astype(np.float64)
    return np.where(j != n - 1, j, -1), margin


def error_of(P, Q, i, j, c, dtype, reverse=False):
    """stage 5 for index arrays i, j -> (|t_E|, the angle of R_E in degrees), one each per pair.  reverse=True swaps i and j: E of the motion from j back to i, which is what
    scripts/evaluate_rpe.py computes (its ominus(b, a) is b^-1 a); the angle is the same, |t_E| is not."""
    if reverse:
        i, j = j, i
    Rxi, Ryi = _matrix(P[i, 3:]), _matrix(Q[i, 3:])
    ta, Ra = dtype(c) * _tmul(Rxi, P[j, :3] - P[i, :3]), np.swapaxes(Rxi, -1, -2) @ _matrix(P[j, 3:])       # c . (X_i^-1 X_j)
    tb = _tmul(Ryi, Q[j, :3] - Q[i, :3])                                                                  # Y_i^-1 Y_j
    te = _tmul(Ra, tb - ta)
    qe = _qmul(_qconj(_qmul(_qconj(P[i, 3:]), P[j, 3:])), _qmul(_qconj(Q[i, 3:]), Q[j, 3:]))
    return _norm(te), _deg(_angle_rad(qe), dtype)


def relative(est, est_t, gt, gt_t, deltas, unit="m", relative=False, along="gt", end="reach", scale="sim3", max_diff=0.0, association="nearest",
             dtype=np.float64, reverse=False):
    """One pair -> dict(stats [D, 16] (COLUMNS), status [D], errors [D, Ne, 2], ends [D, Ne] (rows per match number, NaN / -1 elsewhere),
    margins [D, n], u [n], n).  A flagged row has n = 0 and NaN elsewhere."""
    deltas = [float(d) for d in np.atleast_1d(deltas)]
    D, ne = len(deltas), len(est)
    out = dict(stats=np.full((D, 16), np.nan, dtype), status=np.zeros(D, np.int64), errors=np.full((D, ne, 2), np.nan, dtype), ends=np.full((D, ne), -1, np.int64),
               margins=None, u=None, n=0)
    out["stats"][:, 0] = 0

    def flagged(bits):
        out["status"][:] = bits
        return out
    status, P, Q, s, c = matches(est, est_t, gt, gt_t, max_diff, association, "sim3" if isinstance(scale, str) else "none")
    if status:
        return flagged(status)
    n = len(P)
    if n < 2:
        return flagged(T.TOO_FEW)
    if not isinstance(scale, str):
        c = float(scale)
    P, Q = P.astype(dtype), Q.astype(dtype)
    for A in (P, Q):
        A[:, 3:] /= np.sqrt((A[:, 3:] * A[:, 3:]).sum(1, keepdims=True))
    u = index_of(P, Q, s, c, unit, along, dtype)
    if np.any(np.diff(u) < 0):
        return flagged(T.UNSORTED)
    out["u"], out["n"], out["margins"] = u, n, np.full((D, n), np.inf)
    for d, delta in enumerate(deltas):
        if relative and unit in ("f", "s"):      # the index is exact in fp64 here: the fp64 product IS the delta (in a wider format 0.2 * 255 is not 51, and a tie would flip)
            delta = dtype(np.float64(delta) * (np.float64(u[-1]) - np.float64(u[0])))
        else:
            delta = dtype(delta) * (u[-1] - u[0]) if relative else dtype(delta)
        ends, out["margins"][d] = ends_of(u, delta, end)
        i = np.nonzero(ends >= 0)[0]
        m = len(i)
        if not m:
            out["status"][d] = NO_PAIR
            continue
        j = ends[i]
        te, re = error_of(P, Q, i, j, c, dtype, reverse)
        span = u[j] - u[i]
        out["errors"][d, i, 0], out["errors"][d, i, 1], out["ends"][d, :n] = te, re, ends
        row = out["stats"][d]
        row[0] = m
        row[1:7] = np.sqrt((te * te).sum() / m), te.sum() / m, np.median(te), np.std(te), te.min(), te.max()
        row[7:13] = np.sqrt((re * re).sum() / m), re.sum() / m, np.median(re), np.std(re), re.min(), re.max()
        row[13], row[14], row[15] = delta, span.sum() / m, c
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
def case(n, pose_dtype="float64", stamp_kind="int64"):
    """traj_eval_ref's case: Ne = Ng = n (the ground truth is the short trajectory), every pose matched"""
    return T.case(n, pose_dtype, stamp_kind)


def sparse_case(n_gt, every, seed, pose_dtype="float64", stamp_kind="int64"):
    """an estimate at every `every`-th ground-truth stamp, jittered by <= 2 ms (the estimate is the short trajectory) -> as `case` """
    gt = T.spiral(n_gt)
    keep = np.arange(0, n_gt, every)
    est = T.image_of(gt, 0.01, seed=seed)[keep]
    gt_t = T.stamps(n_gt, stamp_kind)
    jit = np.random.default_rng(seed + 1).integers(-2000, 2001, len(keep))
    est_t = gt_t[keep] + (jit if stamp_kind == "int64" else jit * 1e-6)
    if pose_dtype == "float32":
        gt, est = gt.astype(np.float32), est.astype(np.float32)
    return est, est_t, gt, gt_t, (10_000 if stamp_kind == "int64" else 0.010)


COMBOS = (("float64", "int64"), ("float32", "float64"))             # pose dtype, stamp kind


def cases():
    """the GPU test's first group: every size x unit x end rule x along x (fp64 poses with int64 stamps, fp32 poses with fp64 stamps), five
    relative deltas each"""
    for n in SIZES:
        for unit in UNITS:
            for end in ("reach", "closest"):
                for along in ("gt", "est"):
                    for pose_dtype, stamp_kind in COMBOS:
                        yield n, unit, end, along, pose_dtype, stamp_kind


def extent(poses):
    return float(np.abs(np.asarray(poses, np.float64)[:, :3]).max())
