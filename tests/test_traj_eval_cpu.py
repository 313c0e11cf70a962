"""tests/traj_eval_ref.py — the numpy restatement of devo_amd.evaluation that the GPU test compares against — checked on the CPU against
closed forms, Horn's quaternion-eigenvector solution and scipy's Slerp; the tolerances the GPU test uses are measured here; the header,
the ctypes table and the compiled binding must declare the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

import traj_eval_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_COLUMNS = [c for c in T.COLUMNS if c in T.REL]


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("n", [3, 4, 65, 257])
def test_a_known_sim3_image_is_recovered(n):
    gt = T.spiral(n)
    est = T.image_of(gt, 0.0, seed=1)
    t = T.stamps(n, "int64")
    c0, q0, t0 = T.SIM3
    r = T.evaluate(est, t, gt, t, align="sim3")
    assert r["status"] == 0 and r["stats"][0] == n
    ext = T.extent(gt)
    assert abs(r["transform"][0] - c0) < 1e-13 * c0
    assert np.abs(r["R"] - T.quat_to_matrix(q0)).max() < 1e-13 and abs(np.linalg.det(r["R"]) - 1) < 1e-13
    assert np.abs(r["transform"][1:4] - t0).max() < 1e-13 * ext * 10
    assert abs(abs(np.dot(r["transform"][4:], q0)) - 1) < 1e-13
    assert r["stats"][6] < 1e-13 * ext * 10                          # the largest error
    assert r["stats"][8] < 1e-5                                      # the rotations agree as well (degrees; atan2 of a 1e-16 vector part)
    # se3 cannot undo the scale: the error is that of the best rigid fit, well above zero
    assert T.evaluate(est, t, gt, t, align="se3")["stats"][1] > 0.1 * ext


def test_a_constant_offset_without_alignment():
    gt = T.spiral(64)
    est = gt.copy()
    est[:, :3] += np.array([3.0, -4.0, 12.0])
    t = T.stamps(64, "float64")
    r = T.evaluate(est, t, gt, t, align="none", rpe_delta=1)
    s = dict(zip(T.COLUMNS, r["stats"]))
    for k in ("rmse", "mean", "median", "min", "max"):
        assert abs(s[k] - 13.0) < 1e-13 * 13
    assert s["std"] < 1e-13 and abs(s["sse"] - 64 * 169.0) < 1e-10 and s["scale"] == 1.0
    assert s["rot_rmse_deg"] < 1e-6 and s["rpe_trans_rmse"] < 1e-13 and s["rpe_terms"] == 63
    assert np.array_equal(r["transform"], [1, 0, 0, 0, 0, 0, 0, 1])
    path = np.linalg.norm(np.diff(gt[:, :3], axis=0), axis=1).sum()
    assert abs(s["path_length"] - path) < 1e-13 * path and abs(s["mpe"] - 1300.0 / path) < 1e-12


def test_a_mirrored_estimate_gets_a_proper_rotation():
    """the uncorrected U V^T would be a reflection with error ~ 0; the corrected rotation leaves the error of the best proper fit"""
    gt = T.spiral(4)
    est = gt.copy()
    est[:, 2] *= -1
    t = T.stamps(4, "int64")
    r = T.evaluate(est, t, gt, t, align="sim3")
    assert r["status"] == 0 and abs(np.linalg.det(r["R"]) - 1) < 1e-12 and r["stats"][1] > 0.05
    h = T.evaluate(est, t, gt, t, align="sim3", formulation="horn")
    assert abs(h["stats"][1] - r["stats"][1]) < 1e-12 and np.abs(h["R"] - r["R"]).max() < 1e-12
    x, y = est[:, :3] - est[:, :3].mean(0), gt[:, :3] - gt[:, :3].mean(0)
    U, D, Vt = np.linalg.svd(y.T @ x)
    assert np.linalg.det(U @ Vt) < 0 and np.abs(y - D.sum() / (x * x).sum() * x @ (U @ Vt).T).max() < 1e-14   # the reflection fits exactly


def test_planar_is_valid_and_collinear_is_degenerate():
    gt = T.spiral(65, planar=True)
    est = T.image_of(gt, 0.01, seed=3)
    est[:, :3] = (gt[:, :3] - T.SIM3[2]) @ T.quat_to_matrix(T.SIM3[1]) / T.SIM3[0]      # exactly planar in its own frame
    t = T.stamps(65, "int64")
    r = T.evaluate(est, t, gt, t)
    assert r["status"] == 0 and r["stats"][6] < 1e-13 and abs(np.linalg.det(r["R"]) - 1) < 1e-13
    line = gt.copy()
    line[:, :3] = np.arange(65)[:, None] * np.array([1.0, 2.0, -1.0])
    r = T.evaluate(line, t, line, t)
    assert r["status"] == T.DEGENERATE and r["stats"][0] == 65 and np.isnan(r["stats"][1:]).all() and np.isnan(r["transform"]).all()
    assert T.evaluate(gt[:2], t[:2], gt[:2], t[:2])["status"] == T.TOO_FEW


def test_the_valid_scenes_are_far_from_the_rank_rule():
    for n in T.SIZES:
        for planar in (False, True):
            p = T.spiral(n, planar)[:, :3]
            d = np.linalg.svd((p - p.mean(0)).T @ (p - p.mean(0)), compute_uv=False)
            assert d[1] / d[0] >= 1e-3, (n, planar, d)


# ------------------------------------------------------------------------------------------------ association
def test_nearest_association_rules():
    gt_t = np.array([0, 10, 10, 20, 30, 40], np.int64)
    est_t = np.array([5, 10, 26, 33, 100], np.int64)
    short_is_est, m = T.associate_nearest(est_t, gt_t, 4)
    assert short_is_est and m.tolist() == [-1, 1, 4, 4, -1]          # 5 is 5 away; 10 takes the leftmost 10; 26 -> 30; 33 -> 30 (shared); 100: none
    assert T.associate_nearest(est_t, gt_t, 5)[1].tolist() == [0, 1, 4, 4, -1]      # halfway between 0 and 10: the lower index; distance = max_diff is kept
    assert not T.associate_nearest(gt_t, gt_t, 0)[0]                 # equal length: the ground truth is the short one
    assert not T.associate_nearest(gt_t, est_t, 4)[0]
    p = T.spiral(6)
    assert T.evaluate(p, gt_t[::-1].copy(), p[:5], est_t, 4)["status"] == T.UNSORTED
    assert T.evaluate(p[:5], est_t + 1000, p, gt_t, 4)["status"] == T.NO_MATCH


def test_interpolation_against_scipy_slerp():
    st = pytest.importorskip("scipy.spatial.transform")
    gt = T.spiral(12)
    gt[5, 3:] *= -1                                                  # a neighbour of opposite sign: the same rotation
    gt[8] = gt[7]                                                    # identical neighbours
    gt_t = np.arange(12, dtype=np.float64) * 0.5
    est_t = np.array([-0.1, 0.0, 0.2, 2.25, 2.5, 2.8, 3.7, 5.5, 5.6, 6.0], np.float64)
    est = T.spiral(10)
    m, poses = T.interpolate_gt(est_t, gt, gt_t)
    assert m.tolist() == [-1, 0, 0, 4, 5, 5, 7, 11, -1, -1] and np.isnan(poses[0]).all()
    inside = m >= 0
    ref_q = st.Slerp(gt_t, st.Rotation.from_quat(gt[:, 3:]))(est_t[inside]).as_quat()
    ref_p = np.stack([np.interp(est_t[inside], gt_t, gt[:, k]) for k in range(3)], 1)
    assert np.abs(poses[inside, :3] - ref_p).max() < 1e-14
    dots = np.abs((poses[inside, 3:] * ref_q).sum(1))
    assert np.abs(dots - 1).max() < 1e-14
    assert np.array_equal(poses[4, :3], gt[5, :3]) and np.array_equal(poses[7], gt[11])     # a stamp on a ground-truth stamp: that pose
    r = T.evaluate(est, est_t, gt, gt_t, association="interpolate", align="se3")
    assert r["status"] == 0 and r["stats"][0] == 7 and r["short_is_est"]


# ------------------------------------------------------------------------------------------------ the measured tolerances
def _disagreement(a, b):
    out = {}
    for k, name in enumerate(T.COLUMNS):
        if name in T.REL and np.isfinite(a["stats"][k]):
            out[name] = abs(a["stats"][k] - b["stats"][k]) / abs(a["stats"][k]) if a["stats"][k] != 0 else abs(b["stats"][k])
    qa, qb = a["transform"][4:], b["transform"][4:]
    tb = np.concatenate([b["transform"][:4], qb if np.dot(qa, qb) >= 0 else -qb])
    ta = a["transform"]
    out["transform"] = max(abs(ta[0] - tb[0]) / abs(ta[0]), np.abs(ta[1:4] - tb[1:4]).max() / max(np.abs(ta[1:4]).max(), 1.0), np.abs(ta[4:] - tb[4:]).max())
    return out


def test_recorded_tolerances():
    """Umeyama / SVD against Horn / eigenvector with reversed sums over exactly the cases of the GPU test's first group: the largest
    disagreement per column must stay within the figures recorded in traj_eval_ref.py (REL, relative, noisy cases; ABS, absolute over the
    RMS extent, exact-recovery cases).  Run with -s to see the measured maxima."""
    worst, worst_abs = {k: 0.0 for k in T.REL}, 0.0
    for n, align, pose_dtype, stamp_kind in T.cases():
        est, est_t, gt, gt_t, max_diff = T.case(n, pose_dtype, stamp_kind)
        kw = dict(max_diff=max_diff, align=align, rpe_delta=1)
        a, b = T.evaluate(est, est_t, gt, gt_t, **kw), T.evaluate(est, est_t, gt, gt_t, formulation="horn", **kw)
        assert a["status"] == b["status"] == 0 and a["stats"][0] == n
        for k, v in _disagreement(a, b).items():
            worst[k] = max(worst[k], v)
        if align == "sim3" and pose_dtype == "float64":
            est = T.image_of(np.asarray(gt, np.float64), 0.0, seed=n)
            a, b = T.evaluate(est, est_t, gt, gt_t, **kw), T.evaluate(est, est_t, gt, gt_t, formulation="horn", **kw)
            for col in (1, 2, 3, 4, 5, 6, 13):
                worst_abs = max(worst_abs, abs(a["stats"][col] - b["stats"][col]) / T.extent(gt))
            worst_abs = max(worst_abs, np.sqrt(abs(a["stats"][7] - b["stats"][7])) / T.extent(gt))
    print("\nmeasured REL:", {k: float(f"{v:.2g}") for k, v in worst.items()}, "ABS:", float(f"{worst_abs:.2g}"))
    for k, v in worst.items():
        assert v <= T.REL[k], (k, v, T.REL[k])
    assert worst_abs <= T.ABS, (worst_abs, T.ABS)


# ------------------------------------------------------------------------------------------------ the layers
def test_the_entry_points_are_declared_everywhere():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bdevo_traj_eval\s*\(", txt) and re.search(r"\bdevo_traj_eval_workspace_bytes\s*\(", txt)
    assert re.search(r"#define\s+DEVO_ABI_VERSION\s+9\b", txt)
    from devo_amd import _lib, build
    assert {"devo_traj_eval", "devo_traj_eval_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "traj_eval.hip" in build.SOURCES
    build.build_lib(verbose=False)
    lib = _lib.lib()
    nearest, interp = lib.devo_traj_eval_workspace_bytes(1000, 0), lib.devo_traj_eval_workspace_bytes(1000, 1)
    assert nearest >= 1000 * 16 and interp >= nearest + 1000 * 56
    build.build_binding(verbose=False)
    from devo_amd import _C
    assert callable(_C.evaluation.traj_eval) and _C.evaluation.workspace_bytes(1000, 1) == interp and _C.evaluation.COLS == len(T.COLUMNS)
    assert hasattr(torch.ops.devo_hip, "traj_eval")
    from devo_amd import evaluation as E
    assert E.COLUMNS == T.COLUMNS and _C.evaluation.MAX_MATCHES == E.MAX_MATCHES


def test_cpu_tensors_are_refused_and_arguments_checked():
    from devo_amd import evaluation as E
    p, t = torch.from_numpy(T.spiral(8)), torch.arange(8)
    with pytest.raises(RuntimeError, match="GPU"):
        E.evaluate(p, t, p, t, max_diff=0)
    with pytest.raises(RuntimeError, match="GPU"):
        E.ate(p, p, t)
    with pytest.raises(ValueError, match="align"):
        E.evaluate(p, t, p, t, max_diff=0, align="affine")
    with pytest.raises(ValueError, match="association"):
        E.evaluate(p, t, p, t, max_diff=0, association="spline")
    with pytest.raises(ValueError, match="2\\^53"):
        E.evaluate(T.spiral(8), np.arange(8) + (1 << 53), T.spiral(8), np.arange(8), max_diff=0)


def test_summary_is_compute_median_results():
    from devo_amd import evaluation as E
    res = {"a": [0.5, 0.2, 0.9], "b": [1.5, 0.4], "c": [0.3]}
    s = E.summary(res, "ds")
    everything = np.array([0.5, 0.2, 0.9, 1.5, 0.4, 0.3])
    assert s["ds/a"] == 0.5 and s["ds/b"] == pytest.approx(0.95) and s["ds/c"] == 0.3
    assert s["AUC"] == pytest.approx(np.maximum(1 - everything, 0).mean()) and s["AVG"] == pytest.approx(np.mean([0.5, 0.95, 0.3]) / 100)
    assert set(E.summary(res)) == {"a", "b", "c", "AUC", "AVG"}
