"""devo_amd.evaluation (csrc/traj_eval.hip): association, Umeyama alignment and the ATE statistics of a batch of trajectory pairs in one
launch, against tests/traj_eval_ref.py (the numpy fp64 restatement, itself checked in test_traj_eval_cpu.py).  Integer outputs (n, the
matched indices, the status) must be exact; every other figure must agree within GPU_FACTOR = 16 times the disagreement of the two CPU
formulations recorded in traj_eval_ref.py (REL per column, relative; ABS over the ground truth's RMS extent where the errors are ~ 0).
Every case is a few launches on at most 1025 poses."""
import functools
import os

import numpy as np
import pytest
import torch

import traj_eval_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = T.GPU_FACTOR


def E():
    from devo_amd import evaluation
    return evaluation


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


ROT_ABS_DEG = 1e-12     # where both sides' rotation angles are pure rounding (identical rotations): a product of three or four unit quaternions carries at
                        # most ~8 eps of absolute error per component, so each side's angle is below 2 sqrt(3) 8 eps rad = 3.5e-13 degrees


def _check(res, b, ref, what, near_zero_extent=None, rot_near_zero=None):
    """pair b of a Result against the restatement's dict.  near_zero_extent: the errors are ~ 0 (exact recovery): the error columns are held
    to ABS times this extent instead of REL; rot_near_zero (default: the same cases): the rotation-angle columns to ROT_ABS_DEG"""
    rot_near_zero = (near_zero_extent is not None) if rot_near_zero is None else rot_near_zero
    stats, tf = res.stats[b].cpu().numpy(), res.transform[b].cpu().numpy()
    assert int(res.status[b]) == ref["status"], (what, "status", int(res.status[b]), ref["status"])
    assert stats[0] == ref["stats"][0], (what, "n", stats[0], ref["stats"][0])
    assert res.short_is_est[b] == ref["short_is_est"], (what, "short")
    if res.matched is not None:
        assert np.array_equal(res.matched_of(b).cpu().numpy(), ref["matched"]), (what, "matched")
    if ref["status"]:
        assert np.isnan(stats[1:]).all() and np.isnan(tf).all(), (what, "a flagged row must be NaN")
        if res.errors is not None:
            assert np.isnan(res.errors_of(b).cpu().numpy()).all(), (what, "errors of a flagged pair")
        return
    assert stats[15] == ref["stats"][15], (what, "rpe_terms")
    error_like = ("rmse", "mean", "median", "std", "min", "max", "sse", "mpe", "rpe_trans_rmse")
    for k, name in enumerate(T.COLUMNS):
        if name not in T.REL:
            continue
        want, got = ref["stats"][k], stats[k]
        if np.isnan(want):
            assert np.isnan(got), (what, name, got)
            continue
        if rot_near_zero and name in ("rot_rmse_deg", "rot_mean_deg", "rpe_rot_rmse_deg"):   # (identical rotations: identical relative rotations too)
            bound = ROT_ABS_DEG
        elif near_zero_extent is not None and name in error_like:
            scale = near_zero_extent ** 2 if name == "sse" else near_zero_extent * (100.0 / ref["stats"][10] if name == "mpe" else 1.0)
            bound = (F * T.ABS) ** (2 if name == "sse" else 1) * scale
        else:
            bound = F * T.REL[name] * abs(want)
        assert abs(got - want) <= bound, (what, name, got, want, abs(got - want), bound)
    qa, qb = ref["transform"][4:], tf[4:]
    if np.dot(qa, qb) < 0:
        qb = -qb
    ta = ref["transform"]
    worst = max(abs(ta[0] - tf[0]) / abs(ta[0]), np.abs(ta[1:4] - tf[1:4]).max() / max(np.abs(ta[1:4]).max(), 1.0), np.abs(qa - qb).max())
    assert worst <= F * T.REL["transform"], (what, "transform", worst)
    assert tf[7] >= 0 and abs(np.linalg.norm(tf[4:]) - 1) < 1e-14, (what, "the rotation's quaternion")
    if res.errors is not None:
        got, want = res.errors_of(b).cpu().numpy(), ref["errors"]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "unmatched errors")
        m = ~np.isnan(want)
        if near_zero_extent is not None:
            assert np.abs(got[m] - want[m]).max() <= F * T.ABS * near_zero_extent, (what, "errors")
        else:                                                        # (the min column's figure is the largest per-element disagreement measured)
            assert (np.abs(got[m] - want[m]) <= F * T.REL["min"] * want[m]).all(), (what, "errors")


def _run(est, est_t, gt, gt_t, **kw):
    kw.setdefault("check", False)
    kw.setdefault("return_errors", True)
    kw.setdefault("return_matches", True)
    return E().evaluate(est, est_t, gt, gt_t, **kw)


# ------------------------------------------------------------------------------------------------ 1. every column and the transform
@functools.lru_cache(maxsize=None)
def _ref_case(n, align, pose_dtype, stamp_kind):
    est, est_t, gt, gt_t, max_diff = T.case(n, pose_dtype, stamp_kind)
    return T.evaluate(est, est_t, gt, gt_t, max_diff=max_diff, align=align, rpe_delta=1)


@pytest.mark.parametrize("align", ["none", "se3", "sim3"])
@pytest.mark.parametrize("n", T.SIZES)
def test_every_column_equals_the_restatement(n, align):
    for pose_dtype in ("float32", "float64"):
        for stamp_kind in ("int64", "float64"):
            est, est_t, gt, gt_t, max_diff = T.case(n, pose_dtype, stamp_kind)
            res = _run(est, est_t, gt, gt_t, max_diff=max_diff, align=align, rpe_delta=1)
            ref = _ref_case(n, align, pose_dtype, stamp_kind)
            assert ref["status"] == 0 and ref["stats"][0] == n
            _check(res, 0, ref, (n, align, pose_dtype, stamp_kind))


@pytest.mark.parametrize("n", [4, 257])
def test_exact_recovery(n):
    gt = T.spiral(n)
    est = T.image_of(gt, 0.0, seed=n)
    t = T.stamps(n, "int64")
    res = _run(est, t, gt, t, max_diff=0, rpe_delta=1)
    ref = T.evaluate(est, t, gt, t, rpe_delta=1)
    _check(res, 0, ref, ("exact", n), near_zero_extent=T.extent(gt))
    tf = res.transform[0].cpu().numpy()
    assert abs(tf[0] - T.SIM3[0]) <= F * T.REL["scale"] * T.SIM3[0] and abs(abs(np.dot(tf[4:], T.SIM3[1])) - 1) < 1e-14


# ------------------------------------------------------------------------------------------------ 2. ragged batch
LENGTHS = (3, 64, 257, 1, 700)


@pytest.fixture(scope="module")
def ragged():
    pairs = [T.case(n, "float32", "int64") for n in LENGTHS]
    dev = [[torch.from_numpy(a).to(DEV) for a in p[:4]] for p in pairs]
    refs = [T.evaluate(*p[:4], max_diff=10_000, rpe_delta=2) for p in pairs]
    return pairs, dev, refs


def _batch(dev, **kw):
    return _run([d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], [d[3] for d in dev], max_diff=10_000, rpe_delta=2, **kw)


def test_ragged_batch(ragged):
    pairs, dev, refs = ragged
    res = _batch(dev)
    assert len(res) == 5 and res.status.tolist() == [0, 0, 0, T.TOO_FEW, 0]
    for b, ref in enumerate(refs):
        _check(res, b, ref, ("ragged", b))
    with pytest.raises(RuntimeError, match="pair 3 .*fewer than three"):
        _batch(dev, check=True)
    # row b of the batch is the single-pair call on pair b, bit for bit
    for b, d in enumerate(dev):
        one = _run(*d, max_diff=10_000, rpe_delta=2)
        assert torch.equal(_bits(one.stats[0]), _bits(res.stats[b])) and torch.equal(_bits(one.transform[0]), _bits(res.transform[b])), b
        assert torch.equal(_bits(one.errors_of(0)), _bits(res.errors_of(b))) and torch.equal(one.matched_of(0), res.matched_of(b)), b
    # packed tensors with offsets are the same call
    eo, go = np.cumsum([0] + list(LENGTHS)), np.cumsum([0] + list(LENGTHS))
    packed = _run(torch.cat([d[0] for d in dev]), torch.cat([d[1] for d in dev]), torch.cat([d[2] for d in dev]), torch.cat([d[3] for d in dev]), max_diff=10_000,
                  rpe_delta=2, offsets=(eo, go))
    assert torch.equal(_bits(packed.stats), _bits(res.stats)) and torch.equal(packed.status, res.status)


def test_two_calls_and_another_stream_give_the_same_bits(ragged):
    _, dev, _ = ragged
    a, b = _batch(dev), _batch(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = _batch(dev)
    s.synchronize()
    for other in (b, c):
        for name in ("stats", "transform", "errors", "matched", "status"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(other, name))), name


# ------------------------------------------------------------------------------------------------ 3. association
def _noisy(n, seed):
    gt = T.spiral(n)
    return T.image_of(gt, 0.01, seed=seed), gt


@pytest.mark.parametrize("ne,ng", [(40, 100), (100, 40), (64, 64)])
def test_the_roles_swap_with_the_lengths(ne, ng):
    n = max(ne, ng)
    est, gt = _noisy(n, seed=ne)
    t = T.stamps(n, "int64")
    pick_e, pick_g = np.sort(np.random.default_rng(1).choice(n, ne, replace=False)), np.sort(np.random.default_rng(2).choice(n, ng, replace=False))
    est, est_t, gt, gt_t = est[pick_e], t[pick_e] + 1500, gt[pick_g], t[pick_g]
    ref = T.evaluate(est, est_t, gt, gt_t, max_diff=60_000, rpe_delta=3)
    assert ref["status"] == 0 and ref["short_is_est"] == (ne < ng) and 3 <= ref["stats"][0] <= min(ne, ng)
    _check(_run(est, est_t, gt, gt_t, max_diff=60_000, rpe_delta=3), 0, ref, ("roles", ne, ng))


@pytest.mark.parametrize("origin", [0, (1 << 31) + 12345, 1_700_000_000_000_000])
def test_ties_duplicates_and_the_max_diff_edge(origin):
    """stamps halfway between two ground-truth stamps take the lower index, duplicates the leftmost; a distance equal to max_diff matches,
    one unit more does not; above 2^31 and at epoch microseconds"""
    gt_t = origin + np.array([0, 10, 10, 20, 30, 40, 40, 40, 60, 70, 80, 90], np.int64)
    est_t = origin + np.array([5, 10, 26, 33, 40, 50, 66, 85], np.int64)    # (all below 2^53: the same stamps go in as fp64 as well)
    est, gt = _noisy(12, seed=5)
    est = est[:8]
    for max_diff, want in ((4, [-1, 1, 4, 4, 5, -1, 9, -1]), (5, [0, 1, 4, 4, 5, -1, 9, 10]), (10, [0, 1, 4, 4, 5, 5, 9, 10])):
        ref = T.evaluate(est, est_t, gt, gt_t, max_diff=max_diff)
        assert ref["matched"].tolist() == want
        _check(_run(est, est_t, gt, gt_t, max_diff=max_diff), 0, ref, ("ties", origin, max_diff))
        _check(_run(est, est_t.astype(np.float64), gt, gt_t.astype(np.float64), max_diff=max_diff), 0, ref, ("ties fp64", origin, max_diff))


def test_no_match_and_unsorted_stamps_are_flagged():
    est, gt = _noisy(12, seed=6)
    t = T.stamps(12, "int64")
    far = _run(est[:8], t[:8] + 10_000_000, gt, t, max_diff=1000)
    _check(far, 0, T.evaluate(est[:8], t[:8] + 10_000_000, gt, t, max_diff=1000), "no match")
    assert int(far.status[0]) == T.NO_MATCH
    with pytest.raises(RuntimeError, match="pair 0 .*within max_diff"):
        _run(est[:8], t[:8] + 10_000_000, gt, t, max_diff=1000, check=True)
    bad = t.copy()
    bad[[4, 5]] = bad[[5, 4]]
    res = _run(est[:8], t[:8], gt, bad, max_diff=1000)
    _check(res, 0, T.evaluate(est[:8], t[:8], gt, bad, max_diff=1000), "unsorted")
    assert int(res.status[0]) == T.UNSORTED
    assert int(_run(est[:8], bad[:8], gt, t, max_diff=1000).status[0]) == 0          # the SHORT stamps may come in any order
    huge = torch.from_numpy(t).to(DEV) + (1 << 53)                   # device stamps cannot be checked on the host: the pair is flagged
    assert int(_run(torch.from_numpy(est).to(DEV), huge, torch.from_numpy(gt).to(DEV), huge, max_diff=0).status[0]) == 32


# ------------------------------------------------------------------------------------------------ 4. rotation edge cases
@pytest.mark.parametrize("n", [4, 65])
def test_a_mirrored_estimate_gets_a_proper_rotation(n):
    gt = T.spiral(n)
    est = T.image_of(gt, 0.0, seed=n)
    est[:, 2] *= -1                                                  # non-planar, mirrored: U V^T alone would be a reflection with error ~ 0
    t = T.stamps(n, "int64")
    ref = T.evaluate(est, t, gt, t)
    assert ref["status"] == 0 and ref["stats"][1] > 0.05 * T.extent(gt) and abs(np.linalg.det(ref["R"]) - 1) < 1e-12
    res = _run(est, t, gt, t, max_diff=0)
    _check(res, 0, ref, ("mirrored", n))
    assert abs(np.linalg.det(T.quat_to_matrix(res.transform[0, 4:].cpu().numpy())) - 1) < 1e-14


@pytest.mark.parametrize("n", [3, 65, 257])
def test_a_planar_trajectory_is_valid(n):
    gt = T.spiral(n, planar=True)
    est = T.image_of(gt, 0.0, seed=n)                                # planar in its own frame: sigma_3 = 0 up to rounding
    t = T.stamps(n, "int64")
    ref = T.evaluate(est, t, gt, t)
    assert ref["status"] == 0
    _check(_run(est, t, gt, t, max_diff=0), 0, ref, ("planar", n), near_zero_extent=T.extent(gt))
    moved = np.concatenate([gt[:, :2] + 0.01 * np.random.default_rng(n).standard_normal((n, 2)), gt[:, 2:]], 1)      # noise inside the plane
    est2 = T.image_of(moved, 0.0, seed=n)
    for k, dv in enumerate(0.02 * np.random.default_rng(n + 1).standard_normal((n, 3))):      # and on the orientations: no column is near zero
        est2[k, 3:] = T.qmul(est2[k, 3:], np.concatenate([dv, [1.0]]) / np.sqrt(1.0 + dv @ dv))
    ref = T.evaluate(est2, t, gt, t)
    assert ref["status"] == 0 and ref["stats"][1] > 1e-3
    _check(_run(est2, t, gt, t, max_diff=0), 0, ref, ("planar noisy", n))


def test_collinear_points_are_degenerate():
    gt = T.spiral(65)
    gt[:, :3] = np.arange(65)[:, None] * np.array([1.0, 2.0, -1.0])  # small integers: Sigma is exact, sigma_2 = 0
    t = T.stamps(65, "int64")
    res = _run(gt, t, gt, t, max_diff=0)
    _check(res, 0, T.evaluate(gt, t, gt, t), "collinear")
    assert int(res.status[0]) == T.DEGENERATE
    assert int(_run(gt, t, gt, t, max_diff=0, align="none").status[0]) == 0       # nothing to align: valid
    with pytest.raises(RuntimeError, match="degenerate"):
        _run(gt, t, gt, t, max_diff=0, check=True)


# ------------------------------------------------------------------------------------------------ 5. median
@pytest.mark.parametrize("n", [5, 6, 255, 256])
def test_the_median_of_odd_and_even_counts(n):
    est, gt = _noisy(n, seed=n)
    t = T.stamps(n, "int64")
    res = _run(est, t, gt, t, max_diff=0)
    ref = T.evaluate(est, t, gt, t)
    _check(res, 0, ref, ("median", n))
    e = np.sort(res.errors_of(0).cpu().numpy())                      # exactly numpy's median of the kernel's own errors
    assert float(res.median[0]) == 0.5 * (e[(n - 1) // 2] + e[n // 2])


def test_the_median_of_equal_errors():
    gt = T.spiral(64)
    gt[:, :3] = np.round(gt[:, :3] * 1024) / 1024                    # multiples of 2^-10: the offset adds and subtracts exactly
    est = gt.copy()
    est[:, :3] += np.array([3.0, -4.0, 12.0])                        # every error is exactly 13
    t = T.stamps(64, "int64")
    res = _run(est, t, gt, t, max_diff=0, align="none")
    _check(res, 0, T.evaluate(est, t, gt, t, align="none"), "equal errors", rot_near_zero=True)
    assert (res.errors_of(0) == 13.0).all() and float(res.median[0]) == 13.0 and float(res.std[0]) == 0.0


# ------------------------------------------------------------------------------------------------ 6. interpolation
def test_interpolation():
    gt = T.spiral(12)
    gt[5, 3:] *= -1                                                  # a neighbour of opposite sign
    gt[8] = gt[7]                                                    # identical neighbours
    gt_t = (np.arange(12) * 500_000).astype(np.int64)
    est_t = np.array([-100_000, 0, 200_000, 2_250_000, 2_500_000, 2_800_000, 3_700_000, 5_500_000, 5_600_000, 6_000_000], np.int64)   # before, on, between, after
    est = T.image_of(T.spiral(10), 0.01, seed=9)
    for align in ("se3", "sim3"):
        ref = T.evaluate(est, est_t, gt, gt_t, association="interpolate", align=align, rpe_delta=2)
        assert ref["status"] == 0 and ref["matched"].tolist() == [-1, 0, 0, 4, 5, 5, 7, 11, -1, -1]
        _check(_run(est, est_t, gt, gt_t, max_diff=0, association="interpolate", align=align, rpe_delta=2), 0, ref, ("interpolate", align))
        ref = T.evaluate(est, est_t * 1e-6, gt, gt_t * 1e-6, association="interpolate", align=align)
        _check(_run(est, est_t * 1e-6, gt, gt_t * 1e-6, max_diff=0, association="interpolate", align=align), 0, ref, ("interpolate fp64", align))
    # more estimated poses than ground-truth ones: the estimate stays the short one
    est_t = np.linspace(-1e5, 5.6e6, 40).astype(np.int64)
    est = T.image_of(T.spiral(40), 0.01, seed=10)
    ref = T.evaluate(est, est_t, gt, gt_t, association="interpolate")
    assert ref["short_is_est"] and ref["status"] == 0
    _check(_run(est, est_t, gt, gt_t, max_diff=0, association="interpolate"), 0, ref, "interpolate long")


# ------------------------------------------------------------------------------------------------ 7. relative pose error
def test_rpe_deltas():
    n = 65
    est, gt = _noisy(n, seed=11)
    t = T.stamps(n, "int64")
    for delta, terms in ((1, n - 1), (n - 1, 1), (n, 0), (n + 5, 0), (0, 0)):
        ref = T.evaluate(est, t, gt, t, rpe_delta=delta)
        assert ref["stats"][15] == terms and np.isnan(ref["stats"][13]) == (terms == 0)
        _check(_run(est, t, gt, t, max_diff=0, rpe_delta=delta), 0, ref, ("rpe", delta))


# ------------------------------------------------------------------------------------------------ 8. bindings and refusals
def test_both_bindings_return_the_same_tensors(ragged, monkeypatch):
    from devo_amd import backends
    nat = backends.native()
    assert (nat is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
    assert nat is None or (nat.evaluation.COLS == len(E().COLUMNS) and nat.evaluation.MAX_MATCHES == E().MAX_MATCHES)
    _, dev, _ = ragged
    compiled = {a: _batch(dev, association=a) for a in ("nearest", "interpolate")}
    if nat is not None:                                              # the registered operator is the same function
        d = dev[2]
        off = torch.tensor([0, 257], device=DEV)
        op = torch.ops.devo_hip.traj_eval(d[0], d[1], off, d[2], d[3], off, 0, 2, 10_000.0, 2, True, True)
        one = _run(*d, max_diff=10_000, rpe_delta=2)
        for got, name in zip(op, ("stats", "transform", "status", "errors", "matched")):
            assert torch.equal(_bits(got), _bits(getattr(one, name))), name
    monkeypatch.setattr(backends, "_native", None)
    for a, want in compiled.items():
        got = _batch(dev, association=a)
        for name in ("stats", "transform", "status", "errors", "matched"):
            assert torch.equal(_bits(getattr(got, name)), _bits(getattr(want, name))), (a, name)


def test_refusals_and_non_contiguous_inputs(ragged):
    pairs, dev, refs = ragged
    est, est_t, gt, gt_t = dev[2]
    with pytest.raises(RuntimeError, match="GPU"):
        E().evaluate(est.cpu(), est_t.cpu(), gt.cpu(), gt_t.cpu(), max_diff=0)
    with pytest.raises(RuntimeError, match="GPU"):
        E().evaluate(est, est_t, gt.cpu(), gt_t, max_diff=0)
    with pytest.raises(ValueError):
        E().evaluate(est[:, :6], est_t, gt, gt_t, max_diff=0)
    with pytest.raises(ValueError):
        E().evaluate(est, est_t[:-1], gt, gt_t, max_diff=0)
    with pytest.raises(ValueError, match="offsets"):
        E().evaluate(est, est_t, gt, gt_t, max_diff=0, offsets=([0, 300], [0, 257]))
    # non-contiguous views are handled (copied): every second column of a wider buffer, every second stamp
    wide = torch.zeros(257, 14, dtype=est.dtype, device=DEV)
    wide[:, ::2] = est
    stamps2 = torch.zeros(514, dtype=torch.int64, device=DEV)
    stamps2[::2] = est_t
    assert not wide[:, ::2].is_contiguous() and not stamps2[::2].is_contiguous()
    a = _run(wide[:, ::2], stamps2[::2], gt, gt_t, max_diff=10_000, rpe_delta=2)
    b = _run(est, est_t, gt, gt_t, max_diff=10_000, rpe_delta=2)
    assert torch.equal(_bits(a.stats), _bits(b.stats))
    _check(a, 0, refs[2], "non-contiguous")


def test_the_reference_entry_points():
    """ate / ate_real with the reference's argument order: metres / centimetres, Trajectory.complete's types (fp32 poses, int64 stamps)"""
    n = 100
    est, gt = _noisy(n, seed=12)
    t = T.stamps(n, "int64")
    ref = T.evaluate(est, t, gt, t)
    assert abs(E().ate(gt, est, t) - ref["stats"][1]) <= F * T.REL["rmse"] * ref["stats"][1]
    cm, m_ref, m_est = E().ate_real(gt, t, est, t)
    assert abs(cm - 100 * ref["stats"][1]) <= F * T.REL["rmse"] * cm and m_ref.shape == m_est.shape == (n, 7)
    pick = np.sort(np.random.default_rng(3).choice(n, 40, replace=False))
    est32, t_est = torch.from_numpy(est[pick].astype(np.float32)).to(DEV), torch.from_numpy(t[pick] + 700).to(DEV)
    ref = T.evaluate(est[pick].astype(np.float32), t[pick] + 700, gt, t, max_diff=1e6)
    cm, m_ref, m_est = E().ate_real(gt, t, est32, t_est)
    assert abs(cm - 100 * ref["stats"][1]) <= F * T.REL["rmse"] * cm
    assert torch.equal(m_est, est32) and np.array_equal(m_ref.cpu().numpy(), gt[pick])
