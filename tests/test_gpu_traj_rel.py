"""devo_amd.evaluation.relative_errors (csrc/traj_rel.hip): the relative pose error of a batch of trajectory pairs over sub-trajectories of
given lengths, against tests/traj_rel_ref.py (the numpy fp64 restatement, itself checked in test_traj_rel_cpu.py against the reference's
script for the units "s" and "f"; for "m", "rad" and "deg" that script does not run and the restatement is the only oracle).  Integer
outputs (n, the ends, the status) must be exact; every other figure must agree within GPU_FACTOR = 8 times the gap between the restatement
in fp64 and in long double recorded in traj_rel_ref.py (TOL per column group, relative).  Every case is a few launches on at most 1000 poses."""
import functools
import os

import numpy as np
import pytest
import torch

import traj_eval_ref as T
import traj_rel_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = R.GPU_FACTOR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
# Where the estimate is an exact similarity image of the ground truth the errors are pure rounding.  |t_E|: each relative translation is a
# difference of positions of magnitude <= M rotated once and scaled (~10 operations, each rounding <= eps M), E adds one difference and one
# rotation: both sides stay below 64 eps M.  The angle: traj_rel_ref.FLOOR.
ZERO_TRANS = 64 * EPS


def E():
    from devo_amd import evaluation
    return evaluation


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _run(est, est_t, gt, gt_t, **kw):
    kw.setdefault("check", False)
    kw.setdefault("return_errors", True)
    return E().relative_errors(est, est_t, gt, gt_t, **kw)


def _check(res, b, ref, what, zero_extent=None, sim3=False):
    """pair b of a RelativeResult against the restatement's dict.  zero_extent: the errors are ~ 0 (exact recovery): the translation columns
    are held to ZERO_TRANS times this extent, the rotation columns to the floor"""
    stats, status = res.stats[b].cpu().numpy(), res.status[b].cpu().numpy()
    assert np.array_equal(status, ref["status"]), (what, "status", status, ref["status"])
    assert np.array_equal(stats[:, 0], ref["stats"][:, 0]), (what, "n", stats[:, 0], ref["stats"][:, 0])
    for d in range(len(status)):
        want, got = ref["stats"][d], stats[d]
        ends, errs = res.ends_of(b, d).cpu().numpy(), res.errors_of(b, d).cpu().numpy()
        assert np.array_equal(ends, ref["ends"][d]), (what, d, "ends")
        if status[d]:
            assert np.isnan(got[1:]).all() and got[0] == 0 and np.isnan(errs).all(), (what, d, "a flagged row must be NaN")
            continue
        assert np.array_equal(np.isnan(errs), np.isnan(ref["errors"][d])), (what, d, "rows without a pair")
        for group, cols in R.GROUPS.items():
            for col in cols:
                if zero_extent is not None and group != "index":
                    bound = ZERO_TRANS * zero_extent if group == "trans" else R.FLOOR["rot"]
                    assert abs(got[col]) <= bound and abs(want[col]) <= bound, (what, d, R.COLUMNS[col], got[col], want[col], bound)
                else:
                    assert R.gap(want[col], got[col], group) <= F * R.TOL[group], (what, d, R.COLUMNS[col], got[col], want[col])
        if sim3:                                                     # (the same figure as `evaluate`'s: test_sim3_scale_is_evaluates; here against numpy's SVD)
            assert abs(got[15] - want[15]) <= T.GPU_FACTOR * T.REL["scale"] * abs(want[15]), (what, d, "scale")
        else:
            assert got[15] == want[15], (what, d, "scale")
        for k, group in enumerate(("trans", "rot")):
            for i in np.nonzero(ends >= 0)[0]:
                if zero_extent is not None:
                    assert abs(errs[i, k]) <= (ZERO_TRANS * zero_extent if group == "trans" else R.FLOOR["rot"]), (what, d, i, group, errs[i, k])
                else:
                    assert R.gap(ref["errors"][d, i, k], errs[i, k], group) <= F * R.TOL[group], (what, d, i, group, errs[i, k], ref["errors"][d, i, k])


def _clear(ref, unit, what):
    """the condition on the inputs of test_traj_rel_cpu.py, for the scenes of this file"""
    if unit in ("m", "rad", "deg") and ref["u"] is not None:
        assert ref["margins"].min() > R.MARGIN * (ref["u"][-1] - ref["u"][0]), (what, "an end-point decision too close to call")


# ------------------------------------------------------------------------------------------------ 1. every column, size, unit, rule
@functools.lru_cache(maxsize=None)
def _ref_case(n, unit, end, along, pose_dtype, stamp_kind, relative=True, deltas=R.FRACTIONS, scale="sim3"):
    est, est_t, gt, gt_t, max_diff = R.case(n, pose_dtype, stamp_kind)
    return R.relative(est, est_t, gt, gt_t, deltas, unit=unit, relative=relative, along=along, end=end, max_diff=max_diff, scale=scale)


@pytest.mark.parametrize("unit", R.UNITS)
@pytest.mark.parametrize("n", R.SIZES)
def test_every_column_equals_the_restatement(n, unit):
    seen = 0
    for n_, unit_, end, along, pose_dtype, stamp_kind in R.cases():
        if (n_, unit_) != (n, unit):
            continue
        est, est_t, gt, gt_t, max_diff = R.case(n, pose_dtype, stamp_kind)
        res = _run(est, est_t, gt, gt_t, deltas=R.FRACTIONS, unit=unit, relative=True, along=along, end=end, max_diff=max_diff)
        ref = _ref_case(n, unit, end, along, pose_dtype, stamp_kind)
        assert ref["n"] == n
        _check(res, 0, ref, (n, unit, end, along, pose_dtype, stamp_kind), sim3=True)
        seen += 1
    assert seen == 8


@pytest.mark.parametrize("unit,delta", [("f", 7.0), ("s", 400_000.0), ("m", 0.8), ("rad", 0.3), ("deg", 20.0)])
def test_one_absolute_delta(unit, delta):
    for n in (65, 257):
        est, est_t, gt, gt_t, max_diff = R.case(n, "float64", "int64")
        for end in ("reach", "closest"):
            ref = R.relative(est, est_t, gt, gt_t, [delta], unit=unit, end=end, max_diff=max_diff, scale=1.7)
            _clear(ref, unit, (n, unit, end))
            assert ref["status"].tolist() == [0] and ref["stats"][0, 13] == delta
            res = _run(est, est_t, gt, gt_t, deltas=delta, unit=unit, end=end, max_diff=max_diff, scale=1.7)
            assert res.stats.shape == (1, 1, 16) and float(res.delta[0, 0]) == delta
            _check(res, 0, ref, (n, unit, end, "absolute"))


def test_exact_reach_and_the_last_match_rule():
    est, est_t, gt, gt_t, max_diff = R.case(64)
    for end, count in (("reach", 59), ("closest", 58)):              # u_j - u_i = 5 exactly is reached; closest drops j = 63
        res = _run(est, est_t, gt, gt_t, deltas=[5], unit="f", end=end, max_diff=max_diff)
        ends = res.ends_of(0, 0).cpu().numpy()
        assert ends[:count].tolist() == list(range(5, 5 + count)) and (ends[count:] == -1).all() and float(res.n[0, 0]) == count
        assert float(res.span_mean[0, 0]) == 5.0
        _check(res, 0, R.relative(est, est_t, gt, gt_t, [5], unit="f", end=end, max_diff=max_diff), ("exact reach", end), sim3=True)


def test_ties_take_the_lowest_index():
    gt, gt_t = T.spiral(8), np.arange(8, dtype=np.int64) * 10       # equal stamps in the (short) estimate: see test_traj_rel_cpu.py
    est, est_t = T.image_of(gt, 0.01, seed=3)[[0, 1, 1, 2, 3]], np.array([0, 10, 10, 20, 30], np.int64)
    for end, want in (("closest", [1, 3, 3, -1, -1]), ("reach", [1, 3, 3, 4, -1])):
        res = _run(est, est_t, gt, gt_t, deltas=[10], unit="s", end=end, scale=1.0, max_diff=0)
        assert res.ends_of(0, 0).tolist() == want
        _check(res, 0, R.relative(est, est_t, gt, gt_t, [10], unit="s", end=end, scale=1.0, max_diff=0), ("equal stamps", end))
    gt = np.zeros((7, 7))                                            # a stationary stretch: u = 0 1 2 2 2 3 4 exactly
    gt[:, 0], gt[:, 6] = [0.0, 1.0, 2.0, 2.0, 2.0, 3.0, 4.0], 1.0
    t = np.arange(7, dtype=np.int64)
    for end, delta, want in (("closest", 2.0, [2, 5, -1, -1, -1, -1, -1]), ("closest", 1.0, [1, 2, 5, 5, 5, -1, -1]), ("reach", 2.0, [2, 5, 6, 6, 6, -1, -1])):
        res = _run(gt, t, gt, t, deltas=[delta], unit="m", end=end, scale=1.0, max_diff=0)
        assert res.ends_of(0, 0).tolist() == want, (end, delta)
        assert float(res.trans_max[0, 0]) == 0.0 and float(res.rot_max_deg[0, 0]) == 0.0 and float(res.delta[0, 0]) == delta


# ------------------------------------------------------------------------------------------------ 2. the scale
def test_sim3_scale_is_evaluates():
    est, est_t, gt, gt_t, max_diff = R.case(257, "float32", "int64")
    res = _run(est, est_t, gt, gt_t, deltas=[0.2, 0.4], unit="m", relative=True, max_diff=max_diff)
    ev = E().evaluate(est, est_t, gt, gt_t, max_diff=max_diff, align="sim3")
    assert torch.equal(_bits(res.scale), _bits(ev.scale[:, None].expand(1, 2)))


def test_given_scales():
    pairs = [R.case(65), R.sparse_case(300, 3, seed=5)]
    lists = [[torch.from_numpy(p[k]).to(DEV) for p in pairs] for k in range(4)]
    c = torch.tensor([1.7, 0.6], dtype=torch.float64, device=DEV)
    res = _run(*lists, deltas=[0.5, 1.5], unit="m", along="est", max_diff=10_000, scale=c)
    for b, p in enumerate(pairs):
        ref = R.relative(*p[:4], [0.5, 1.5], unit="m", along="est", max_diff=10_000, scale=float(c[b]))
        _clear(ref, "m", ("per-pair scale", b))
        _check(res, b, ref, ("per-pair scale", b))
        one = _run(*p[:4], deltas=[0.5, 1.5], unit="m", along="est", max_diff=10_000, scale=float(c[b]))
        assert torch.equal(_bits(one.stats[0]), _bits(res.stats[b])), "a float scale and a tensor scale must give the same bits"
    with pytest.raises(ValueError, match="scale"):
        _run(*lists, deltas=[0.5], max_diff=10_000, scale=c[:1])
    line = T.spiral(16)                                              # collinear matches: degenerate for "sim3", valid for a given scale; two matches suffice
    line[:, :3] = np.outer(np.arange(16), [1.0, 2.0, 3.0])
    t = T.stamps(16, "int64")
    assert _run(line, t, line, t, deltas=[2], unit="f", max_diff=0).status.tolist() == [[T.DEGENERATE]]
    assert _run(line, t, line, t, deltas=[2], unit="f", max_diff=0, scale=1.0).status.tolist() == [[0]]
    assert _run(line[:2], t[:2], line, t, deltas=[1], unit="f", max_diff=0, scale=2.0).status.tolist() == [[0]]
    assert _run(line[:2], t[:2], T.spiral(16), t, deltas=[1], unit="f", max_diff=0).status.tolist() == [[T.TOO_FEW]]
    assert _run(line[:1], t[:1], line, t, deltas=[1], unit="f", max_diff=0, scale=2.0).status.tolist() == [[T.TOO_FEW]]


@pytest.mark.parametrize("n", [4, 257])
def test_exact_recovery(n):
    """est = a similarity image of gt: zero errors with the Umeyama scale, the scale's share of every step without it"""
    gt = T.spiral(n)
    est = T.image_of(gt, 0.0, seed=n)
    t = T.stamps(n, "int64")
    M = max(R.extent(gt), R.extent(est))
    for unit in ("f", "m"):
        kw = dict(deltas=[0.25, 0.5], unit=unit, relative=True, max_diff=0)
        _check(_run(est, t, gt, t, **kw), 0, R.relative(est, t, gt, t, kw["deltas"], unit=unit, relative=True), ("exact", n, unit), zero_extent=M, sim3=True)
        res, ref = _run(est, t, gt, t, scale=1.0, **kw), R.relative(est, t, gt, t, kw["deltas"], unit=unit, relative=True, scale=1.0)
        _check(res, 0, ref, ("exact, unscaled", n, unit))
        # Y_i^-1 Y_j = c . (X_i^-1 X_j) here, so without the scale |t_E| = (1 - 1 / c) |y_j - y_i|: far from zero
        assert float(res.trans_min[0].min()) > 0.1 * (1 - 1 / T.SIM3[0]) * np.linalg.norm(gt[-1, :3] - gt[0, :3]) * 0.25


# ------------------------------------------------------------------------------------------------ 3. a ragged batch
DELTAS_M = (0.5, 2.0, 6.0)


@pytest.fixture(scope="module")
def ragged():
    short = T.spiral(40, span=3.0)                                   # its path is 3.3 m long: no pair for the largest delta
    pairs = [R.case(257, "float32", "int64"), R.sparse_case(300, 3, seed=5, pose_dtype="float32"),
             (T.image_of(short, 0.01, seed=8).astype(np.float32), T.stamps(40, "int64"), short.astype(np.float32), T.stamps(40, "int64"), 10_000),
             (T.image_of(T.spiral(30), 0.01, seed=9).astype(np.float32), T.stamps(30, "int64") + 10_000_000, T.spiral(30).astype(np.float32), T.stamps(30, "int64"), 10_000)]
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in p[:4]] for p in pairs]
    refs = [R.relative(*p[:4], DELTAS_M, unit="m", max_diff=10_000) for p in pairs]
    for b, ref in enumerate(refs):
        _clear(ref, "m", ("ragged", b))
    assert refs[2]["status"].tolist() == [0, 0, R.NO_PAIR] and refs[3]["status"].tolist() == [T.NO_MATCH] * 3
    return pairs, dev, refs


def _batch(dev, **kw):
    kw.setdefault("deltas", DELTAS_M)
    kw.setdefault("unit", "m")
    return _run([d[0] for d in dev], [d[1] for d in dev], [d[2] for d in dev], [d[3] for d in dev], max_diff=10_000, **kw)


def test_ragged_batch_equals_every_pair_alone(ragged):
    pairs, dev, refs = ragged
    res = _batch(dev)
    assert res.stats.shape == (4, 3, 16) and res.status.shape == (4, 3) and res.errors.shape == (3, 257 + 100 + 40 + 30, 2)
    for b in range(4):
        _check(res, b, refs[b], ("ragged", b), sim3=True)
        one = _run(*dev[b], deltas=DELTAS_M, unit="m", max_diff=10_000)
        assert torch.equal(one.status[0], res.status[b]), b
        assert torch.equal(_bits(one.stats[0]), _bits(res.stats[b])), ("a pair's rows must not depend on the batch", b)
        for d in range(3):
            assert torch.equal(_bits(one.errors_of(0, d)), _bits(res.errors_of(b, d))) and torch.equal(one.ends_of(0, d), res.ends_of(b, d))
    assert res.status[3].tolist() == [T.NO_MATCH] * 3 and torch.isnan(res.stats[3, :, 1:]).all() and (res.stats[3, :, 0] == 0).all()
    fewer = _batch(dev, deltas=DELTAS_M[:2])                         # ... nor on the other deltas
    assert torch.equal(_bits(fewer.stats), _bits(res.stats[:, :2]))
    again = _batch(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _batch(dev)
    side.synchronize()
    for got in (again, other):
        for name in ("stats", "status", "errors", "ends"):
            assert torch.equal(_bits(getattr(got, name)), _bits(getattr(res, name))), name
    packed = _run(torch.cat([d[0] for d in dev]), torch.cat([d[1] for d in dev]), torch.cat([d[2] for d in dev]), torch.cat([d[3] for d in dev]),
                  offsets=([0, 257, 357, 397, 427], [0, 257, 557, 597, 627]), deltas=DELTAS_M, unit="m", max_diff=10_000)
    assert torch.equal(_bits(packed.stats), _bits(res.stats)) and torch.equal(_bits(packed.errors), _bits(res.errors))
    pct, deg_per_m = res.percent()
    assert torch.equal(_bits(pct), _bits(100.0 * res.trans_mean / res.delta)) and torch.equal(_bits(deg_per_m), _bits(res.rot_mean_deg / res.delta))


def test_check_raises_naming_pair_and_delta(ragged):
    pairs, dev, refs = ragged
    with pytest.raises(RuntimeError, match=r"pair 2 .*delta 2 \(6 m\).*no sub-trajectory"):
        _batch(dev[:3], check=True)
    with pytest.raises(RuntimeError, match=r"pair 1 .*delta 0 .*max_diff"):
        _batch(dev[:1] + dev[3:], check=True)
    ok = _batch(dev[:2], check=True)
    assert int(ok.status.abs().sum()) == 0


def test_interpolated_association(ragged):
    pairs, dev, refs = ragged
    for b in (0, 1):
        for unit, deltas in (("m", [0.5, 2.0]), ("s", [500_000, 2_000_000])):
            ref = R.relative(*pairs[b][:4], deltas, unit=unit, association="interpolate")
            _clear(ref, unit, ("interpolate", b))
            assert ref["status"].tolist() == [0, 0]
            _check(_run(*dev[b], deltas=deltas, unit=unit, association="interpolate", max_diff=0), 0, ref, ("interpolate", b, unit), sim3=True)


# ------------------------------------------------------------------------------------------------ 4. the medians
def test_medians_of_odd_even_and_equal_counts():
    est, est_t, gt, gt_t, max_diff = R.case(64)
    for delta, count in ((5, 59), (4, 60), (63, 1), (62, 2)):
        res = _run(est, est_t, gt, gt_t, deltas=[delta], unit="f", max_diff=max_diff)
        errs = res.errors_of(0, 0).cpu().numpy()[:count]
        assert float(res.n[0, 0]) == count
        assert float(res.trans_median[0, 0]) == np.median(errs[:, 0]) and float(res.rot_median_deg[0, 0]) == np.median(errs[:, 1]), (delta, "the median is exact")
    # all errors equal: uniform motion along x without rotation, the estimate's steps doubled by c = 2: |t_E| = the step, every time
    gt = np.zeros((50, 7))
    gt[:, 0], gt[:, 6] = 0.5 * np.arange(50), 1.0
    t = T.stamps(50, "int64")
    res = _run(gt, t, gt, t, deltas=[3], unit="f", scale=2.0, max_diff=0)
    row = res.stats[0, 0].tolist()
    assert row[0] == 47 and row[1:7] == [1.5, 1.5, 1.5, 0.0, 1.5, 1.5] and row[7:13] == [0.0] * 6 and row[13:] == [3.0, 3.0, 2.0]


# ------------------------------------------------------------------------------------------------ 5. bindings and refusals
def test_both_bindings_return_the_same_tensors(ragged, monkeypatch):
    from devo_amd import backends
    nat = backends.native()
    assert (nat is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
    assert nat is None or nat.evaluation.REL_COLS == len(E().REL_COLUMNS)
    _, dev, _ = ragged
    c = torch.tensor([1.7, 0.6, 1.0, 2.0], dtype=torch.float64, device=DEV)
    variants = [dict(), dict(association="interpolate", unit="rad", deltas=[0.1, 0.4], end="closest", along="est"), dict(scale=c, unit="deg", deltas=[10.0], relative=False),
                dict(scale=1.3, unit="s", deltas=[0.3], relative=True)]
    compiled = [_batch(dev, **v) for v in variants]
    if nat is not None:                                              # the registered operator is the same function
        d = dev[0]
        off = torch.tensor([0, 257], device=DEV)
        op = torch.ops.devo_hip.traj_rel_eval(d[0], d[1], off, d[2], d[3], off, 0, 10_000.0, list(DELTAS_M), 2, False, 0, 0, 0, 1.0, None, True)
        one = _run(*d, deltas=DELTAS_M, unit="m", max_diff=10_000)
        for got, name in zip(op, ("stats", "status", "errors", "ends")):
            assert torch.equal(_bits(got), _bits(getattr(one, name))), name
        assert nat.evaluation.rel_workspace_bytes(627, 0, 4, 3) >= nat.evaluation.workspace_bytes(627, 0)
    monkeypatch.setattr(backends, "_native", None)
    for v, want in zip(variants, compiled):
        got = _batch(dev, **v)
        for name in ("stats", "status", "errors", "ends"):
            assert torch.equal(_bits(getattr(got, name)), _bits(getattr(want, name))), (v, name)


def test_refusals_and_without_errors(ragged):
    pairs, dev, refs = ragged
    est, est_t, gt, gt_t = dev[1]
    with pytest.raises(RuntimeError, match="GPU"):
        E().relative_errors(est.cpu(), est_t.cpu(), gt.cpu(), gt_t.cpu(), deltas=[1.0], max_diff=0)
    with pytest.raises(RuntimeError, match="GPU"):
        E().relative_errors(est, est_t, gt, gt_t, deltas=[1.0], max_diff=0, scale=torch.ones(1, dtype=torch.float64))
    res = E().relative_errors(est, est_t, gt, gt_t, deltas=DELTAS_M, max_diff=10_000)
    assert res.errors is None and res.ends is None
    assert torch.equal(_bits(res.stats[0]), _bits(_batch(dev).stats[1]))
    with pytest.raises(ValueError, match="return_errors"):
        res.ends_of(0, 0)
    back = est_t[[0, 2, 1, 3]]                                       # the estimate's matched stamps go back: the index "s" would decrease
    assert _run(est[:4], back, gt, gt_t, deltas=[1.0], unit="s", scale=1.0, max_diff=10_000).status.tolist() == [[T.UNSORTED]]
    assert _run(est[:4], back, gt, gt_t, deltas=[1.0], unit="f", scale=1.0, max_diff=10_000).status.tolist() == [[0]]


# ------------------------------------------------------------------------------------------------ 6. the golden scene
def test_the_golden_scene():
    """the reference's scripts/evaluate_rpe.py on tests/golden/rpe_scene.npz: the pairs it evaluates, exactly; its rotation errors (arccos of a
    trace at angles >= 1e-2 rad: 1e-12 rad, see test_traj_rel_cpu.py); the translation errors against the restatement, which
    test_traj_rel_cpu.py ties to the script's (the script measures the motion from the end pose back to the start)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rpe_scene.npz"))
    est, est_t, gt, gt_t = g["est"], g["est_t"], g["gt"], g["gt_t"]
    max_diff = 2.0 * float(np.median(np.diff(gt_t)))
    for unit in ("s", "f"):
        ks = [k for k, u in enumerate(g["units"]) if str(u) == unit]
        deltas = [float(g["deltas"][k]) for k in ks]
        res = _run(est, est_t, gt, gt_t, deltas=deltas, unit=unit, along="est", end="closest", scale=1.0, max_diff=max_diff)
        _check(res, 0, R.relative(est, est_t, gt, gt_t, deltas, unit=unit, along="est", end="closest", scale=1.0, max_diff=max_diff), ("golden", unit))
        for d, k in enumerate(ks):
            rows = g[f"rows_{k}"]
            ends, errs = res.ends_of(0, d).cpu().numpy(), res.errors_of(0, d).cpu().numpy()
            i = np.nonzero(ends >= 0)[0]
            assert len(i) == len(rows) == float(res.n[0, d]), (unit, deltas[d])
            assert np.array_equal(est_t[i], rows[:, 0]) and np.array_equal(est_t[ends[i]], rows[:, 1]), (unit, deltas[d], "pair selection")
            assert np.abs(np.radians(errs[i, 1]) - rows[:, 5]).max() <= 1e-12, (unit, deltas[d], "rotation")
