"""tests/traj_rel_ref.py — the numpy restatement of devo_amd.evaluation.relative_errors that the GPU test compares against — checked on
the CPU: against rows recorded from the reference's scripts/evaluate_rpe.py (tests/golden/rpe_scene.npz, written by tools/gen_golden_rpe.py;
units "s" and "f" only: the script's "m" and "rad" branches do not run under Python 3, so for "m", "rad" and "deg" the restatement is the only
oracle), against itself in extended precision (the recorded tolerances), on the clearness of every end-point decision of the GPU test's
cases, and on deliberate ties.  Then the layers (header, tables, sources, bindings) and the refusals that need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

import traj_eval_ref as T
import traj_rel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the golden scene
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "rpe_scene.npz"))
    cases = [(str(u), float(d), g[f"rows_{k}"]) for k, (u, d) in enumerate(zip(g["units"], g["deltas"]))]
    return g["est"], g["est_t"], g["gt"], g["gt_t"], 2.0 * float(np.median(np.diff(g["gt_t"]))), cases     # (the script's twice-median ground-truth interval)


GOLDEN_ROT_RAD = 1e-12      # the script's angle is arccos((tr - 1) / 2): at angles >= 1e-2 rad (asserted) a rounding of eps in the trace moves it by eps / sin(angle) <= 2.3e-14
GOLDEN_TRANS_REL = 1e-13    # |t_E| of the script: 4 x 4 inverses and products of poses of extent ~2, errors ~ 0.05: ~100 eps of absolute rounding, 4e-13 relative at worst


def test_the_golden_scene_is_well_posed():
    est, est_t, gt, gt_t, max_diff, cases = golden()
    assert len(gt) == 400 and len(est) == 70 and np.all(np.diff(gt_t) > 0) and np.all(np.diff(est_t) > 0)
    d = np.sort(np.abs(gt_t[None, :] - est_t[:, None]), 1)
    assert (d[:, 1] - d[:, 0]).min() > 1e-6, "an estimated stamp with two nearest ground-truth stamps"
    assert d[:, 0].max() < 0.5 * np.median(np.diff(gt_t)) < max_diff
    for unit, delta, rows in cases:
        o = R.relative(est, est_t, gt, gt_t, [delta], unit=unit, along="est", end="closest", scale=1.0, max_diff=max_diff)
        assert o["n"] == 70 and o["margins"].min() > 0, (unit, delta, "an end-point decision is a tie")
        assert rows[:, 5].min() > 1e-2, "a rotation error where the script's arccos is ill conditioned"


def test_restatement_against_the_reference_script():
    """Pair selection (the starts and ends by their stamps, the j = n - 1 rule, the count) must be exact and the rotation error must agree.
    The script forms its relative motions from the END pose: ominus(traj[j], traj[i]) = X_j^-1 X_i, so what it reports is
    E(j, i) = (c . (X_j^-1 X_i))^-1 (Y_j^-1 Y_i): the same angle as E(i, j) of the feature's text, another |t_E| (the error seen from the end
    frame; on this scene they differ by up to 80 %).  The restatement's `reverse=True` computes E(j, i) by the same code with i and j swapped:
    that must reproduce the script's translation, which checks the scale, the inverse and the product; the forward value is what the package
    computes (stage 5 of the text, and `evaluate`'s rpe columns)."""
    est, est_t, gt, gt_t, max_diff, cases = golden()
    for unit, delta, rows in cases:
        fwd = R.relative(est, est_t, gt, gt_t, [delta], unit=unit, along="est", end="closest", scale=1.0, max_diff=max_diff)
        rev = R.relative(est, est_t, gt, gt_t, [delta], unit=unit, along="est", end="closest", scale=1.0, max_diff=max_diff, reverse=True)
        i = np.nonzero(fwd["ends"][0] >= 0)[0]
        j = fwd["ends"][0][i]
        assert len(i) == len(rows) == fwd["stats"][0, 0], (unit, delta, len(i), len(rows))
        assert np.array_equal(est_t[i], rows[:, 0]) and np.array_equal(est_t[j], rows[:, 1]), (unit, delta, "pair selection")
        assert np.array_equal(rev["ends"], fwd["ends"])
        for o in (fwd, rev):
            assert np.abs(np.radians(o["errors"][0, i, 1]) - rows[:, 5]).max() <= GOLDEN_ROT_RAD, (unit, delta, "rotation")
        gap = np.abs(rev["errors"][0, i, 0] - rows[:, 4]) / rows[:, 4]
        print(unit, delta, len(rows), "pairs; translation gap", gap.max(), "rotation gap (rad)", np.abs(np.radians(fwd["errors"][0, i, 1]) - rows[:, 5]).max())
        assert gap.max() <= GOLDEN_TRANS_REL, (unit, delta, "translation", gap.max())
        assert fwd["stats"][0, 2] == pytest.approx(fwd["errors"][0, i, 0].mean(), rel=1e-14) and fwd["stats"][0, 13] == delta and fwd["stats"][0, 15] == 1.0


# ------------------------------------------------------------------------------------------------ tolerances and margins
def test_recorded_tolerances():
    """fp64 against long double over exactly the cases of the GPU test's first group: the largest relative gap per column group must stay
    within the figures recorded in traj_rel_ref.py (TOL; `gap` and FLOOR there say what counts).  Run with -s to see the measured maxima."""
    worst = {k: 0.0 for k in R.GROUPS}
    for n, unit, end, along, pose_dtype, stamp_kind in R.cases():
        est, est_t, gt, gt_t, max_diff = R.case(n, pose_dtype, stamp_kind)
        kw = dict(unit=unit, relative=True, along=along, end=end, max_diff=max_diff)
        a, b = R.relative(est, est_t, gt, gt_t, R.FRACTIONS, **kw), R.relative(est, est_t, gt, gt_t, R.FRACTIONS, dtype=np.longdouble, **kw)
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["ends"], b["ends"]) and np.array_equal(a["stats"][:, 0], b["stats"][:, 0])
        for d in range(len(R.FRACTIONS)):
            if a["status"][d]:
                continue
            for group, cols in R.GROUPS.items():
                for col in cols:
                    worst[group] = max(worst[group], R.gap(b["stats"][d, col], a["stats"][d, col], group))
            for k, group in enumerate(("trans", "rot")):                                  # the per-start values are held to the same figures
                for i in np.nonzero(a["ends"][d] >= 0)[0]:
                    worst[group] = max(worst[group], R.gap(b["errors"][d, i, k], a["errors"][d, i, k], group))
    print("\nmeasured:", {k: float(f"{v:.4g}") for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= R.TOL[k], (k, v, R.TOL[k])


def test_every_end_point_decision_is_clear():
    """A condition on the inputs: where the index is computed (a cumulative sum: "m", "rad", "deg") the two sides' indices differ in their
    last bits, so every decision of every case must have a margin above 1e-9 of the index range (reach: |u_j - u_i - delta| at j and j - 1;
    closest: the gap between the best and the second best).  "f" and "s" compare numbers that both sides hold exactly (k, the stamps): they
    decide exactly, ties included, and their ties stay in the cases on purpose (closest at half a frame: n = 4, delta 1.5)."""
    ties = 0
    for n, unit, end, along, pose_dtype, stamp_kind in R.cases():
        est, est_t, gt, gt_t, max_diff = R.case(n, pose_dtype, stamp_kind)
        o = R.relative(est, est_t, gt, gt_t, R.FRACTIONS, unit=unit, relative=True, along=along, end=end, max_diff=max_diff)
        assert o["n"] == n
        if unit in ("m", "rad", "deg"):
            assert o["margins"].min() > R.MARGIN * (o["u"][-1] - o["u"][0]), (n, unit, end, along, pose_dtype, stamp_kind, o["margins"].min())
        else:
            ties += int((o["margins"] == 0).sum())
    assert ties > 0


def test_ties_take_the_lowest_index():
    # equal stamps: the estimate (short) has the stamps 0 1 1 2 3 of which both 1s match; "s", closest, delta 1: from 0 the nearest is 1, twice: the lower
    gt, gt_t = T.spiral(8), np.arange(8, dtype=np.int64) * 10
    est, est_t = T.image_of(gt, 0.01, seed=3)[[0, 1, 1, 2, 3]], np.array([0, 10, 10, 20, 30], np.int64)
    o = R.relative(est, est_t, gt, gt_t, [10], unit="s", end="closest", scale=1.0, max_diff=0)
    assert o["n"] == 5 and o["ends"][0].tolist() == [1, 3, 3, -1, -1]        # (from 1 and 2: 20 -> match 3; from 3 and 4: the last match, dropped)
    o = R.relative(est, est_t, gt, gt_t, [10], unit="s", end="reach", scale=1.0, max_diff=0)
    assert o["ends"][0].tolist() == [1, 3, 3, 4, -1]
    # a stationary stretch: the ground truth stands at matches 2 .. 4; "m" along it, u = 0 1 2 2 2 3 4 exactly (unit steps along x)
    pos = np.array([0.0, 1.0, 2.0, 2.0, 2.0, 3.0, 4.0])
    gt = np.zeros((7, 7))
    gt[:, 0], gt[:, 6] = pos, 1.0
    t = np.arange(7, dtype=np.int64)
    o = R.relative(gt, t, gt, t, [2.0], unit="m", end="closest", scale=1.0, max_diff=0)
    assert o["u"].tolist() == [0, 1, 2, 2, 2, 3, 4] and o["ends"][0].tolist() == [2, 5, -1, -1, -1, -1, -1]   # (from 0: 2, three times: the lowest)
    o = R.relative(gt, t, gt, t, [1.0], unit="m", end="closest", scale=1.0, max_diff=0)
    assert o["ends"][0].tolist() == [1, 2, 5, 5, 5, -1, -1]
    o = R.relative(gt, t, gt, t, [2.0], unit="m", end="reach", scale=1.0, max_diff=0)
    assert o["ends"][0].tolist() == [2, 5, 6, 6, 6, -1, -1] and np.all(o["errors"][0, :5] == 0)
    assert o["stats"][0, 0] == 5 and o["stats"][0, 14] == 2.0


def test_exact_reach_and_the_last_match_rule():
    est, est_t, gt, gt_t, max_diff = R.case(64)
    o = R.relative(est, est_t, gt, gt_t, [5], unit="f", end="reach", max_diff=max_diff)
    assert o["ends"][0, :59].tolist() == list(range(5, 64)) and (o["ends"][0, 59:] == -1).all() and o["stats"][0, 0] == 59 and o["stats"][0, 14] == 5
    o = R.relative(est, est_t, gt, gt_t, [5], unit="f", end="closest", max_diff=max_diff)
    assert o["ends"][0, :58].tolist() == list(range(5, 63)) and (o["ends"][0, 58:] == -1).all()       # (j = 63 = n - 1 is dropped)
    o = R.relative(est, est_t, gt, gt_t, [64], unit="f", end="reach", max_diff=max_diff)
    assert o["status"].tolist() == [R.NO_PAIR] and o["stats"][0, 0] == 0 and np.isnan(o["stats"][0, 1:]).all()


def test_flags_follow_the_evaluation():
    gt, t = T.spiral(16), T.stamps(16, "int64")
    est = T.image_of(gt, 0.01, seed=1)
    line = gt.copy()
    line[:, :3] = np.outer(np.arange(16), [1.0, 2.0, 3.0])
    assert R.relative(line, t, line, t, [2], unit="f", max_diff=0)["status"].tolist() == [T.DEGENERATE]
    assert R.relative(line, t, line, t, [2], unit="f", max_diff=0, scale=1.0)["status"].tolist() == [0]           # a given scale: no alignment
    assert R.relative(est, t + 10_000_000, gt, t, [2, 3], unit="f", max_diff=10)["status"].tolist() == [T.NO_MATCH] * 2
    assert R.relative(est[:3], t[:2].tolist() + [t[15]], gt, t, [1], unit="f", max_diff=0, scale=2.0)["status"].tolist() == [0]
    assert R.relative(est[:2], t[:2], gt, t, [1], unit="f", max_diff=0)["status"].tolist() == [T.TOO_FEW]          # "sim3" keeps the rule of three
    assert R.relative(est[:2], t[:2], gt, t, [1], unit="f", max_diff=0, scale=2.0)["status"].tolist() == [0]       # two suffice for a given scale
    assert R.relative(est[:1], t[:1], gt, t, [1], unit="f", max_diff=0, scale=2.0)["status"].tolist() == [T.TOO_FEW]
    back = np.array([t[0], t[2], t[1], t[3]])
    assert R.relative(est[:4], back, gt, t, [1], unit="s", max_diff=0, scale=1.0)["status"].tolist() == [T.UNSORTED]


# ------------------------------------------------------------------------------------------------ the layers
def test_the_entry_points_are_declared_everywhere():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bdevo_traj_rel_eval\s*\(", txt) and re.search(r"\bdevo_traj_rel_workspace_bytes\s*\(", txt)
    assert re.search(r"#define\s+DEVO_ABI_VERSION\s+9\b", txt)
    assert re.search(r"#define\s+DEVO_TRAJ_REL_COLS\s+16\b", txt) and re.search(r"#define\s+DEVO_TRAJ_REL_MAX_DELTAS\s+16\b", txt)
    assert re.search(r"DEVO_TRAJ_REL_NO_PAIR\s*=\s*128\b", txt)
    from devo_amd import _lib, build
    assert {"devo_traj_rel_eval", "devo_traj_rel_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "traj_rel.hip" in build.SOURCES and "traj_eval.hip" in build.SOURCES
    build.build_lib(verbose=False)
    lib = _lib.lib()
    assert lib.devo_abi_version() == 9
    one, five = lib.devo_traj_rel_workspace_bytes(1000, 0, 2, 1), lib.devo_traj_rel_workspace_bytes(1000, 0, 2, 5)
    assert one >= lib.devo_traj_eval_workspace_bytes(1000, 0) + 1000 * 8 + 1000 * 20 and five >= one + 4 * 1000 * 20
    assert lib.devo_traj_rel_workspace_bytes(1000, 1, 2, 1) >= one + 1000 * 56
    build.build_binding(verbose=False)
    from devo_amd import _C
    from devo_amd import evaluation as E
    assert callable(_C.evaluation.traj_rel_eval) and _C.evaluation.rel_workspace_bytes(1000, 0, 2, 5) == five
    assert _C.evaluation.REL_COLS == len(E.REL_COLUMNS) == len(R.COLUMNS) == 16 and E.REL_COLUMNS == R.COLUMNS
    assert hasattr(torch.ops.devo_hip, "traj_rel_eval")
    assert E.NO_PAIR == R.NO_PAIR and E.MAX_DELTAS == 16 and tuple(E.UNITS) == R.UNITS


def test_cpu_tensors_are_refused_and_arguments_checked():
    from devo_amd import evaluation as E
    p, t = torch.from_numpy(T.spiral(8)), torch.arange(8)
    kw = dict(deltas=[1.0], max_diff=0)
    with pytest.raises(RuntimeError, match="GPU"):
        E.relative_errors(p, t, p, t, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        E.relative_errors([p, p], [t, t], [p, p], [t, t], scale=2.0, **kw)
    for name, bad in (("unit", "km"), ("end", "nearest"), ("along", "both"), ("association", "spline"), ("scale", "se3")):
        with pytest.raises(ValueError, match=name):
            E.relative_errors(p, t, p, t, **dict(kw, **{name: bad}))
    for deltas in ([], [1.0] * 17, [0.0], [1.0, -2.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="deltas"):
            E.relative_errors(p, t, p, t, deltas=deltas, max_diff=0)
    with pytest.raises(ValueError, match="scale"):
        E.relative_errors(p, t, p, t, scale=torch.ones(2, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="scale"):
        E.relative_errors([p, p], [t, t], [p, p], [t, t], scale=torch.ones(3, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match="scale"):
        E.relative_errors(p, t, p, t, scale=0.0, **kw)
    with pytest.raises(ValueError, match="max_diff"):
        E.relative_errors(p, t, p, t, deltas=[1.0], max_diff=-1)
    r = E.RelativeResult(torch.zeros(1, 2, 16, dtype=torch.float64), torch.zeros(1, 2, dtype=torch.int32), None, None, [0, 8], "s")
    assert r.trans_mean.shape == (1, 2) and len(r) == 1
    with pytest.raises(ValueError, match="metres"):
        r.percent()
    with pytest.raises(ValueError, match="return_errors"):
        r.errors_of(0, 1)
