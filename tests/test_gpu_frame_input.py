"""frames.frame_input (devo/devo.py:406-467 in two launches) against the numpy fp64 restatement tests/frame_input_ref.py: counts and gate
records exact, "none" bit-equal, "rescale" bit-equal to the fp32 division by the restated extrema, "std" within
8 * 2^-24 * (|x| + |mean|) / sigma of the fp64 restatement (a few fp32 roundings of a difference and a quotient whose statistics are
exact to fp64), the degenerate grids as events.std returns them, and two calls on one input bit-equal."""
import numpy as np
import pytest
import torch

import frame_input_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grid(shape, density, seed, sign=0, dtype=np.float32):
    g = np.random.default_rng(seed)
    v = g.standard_normal(shape).astype(np.float32) * 1.5
    if sign:
        v = np.abs(v) * sign
    v[g.random(shape) >= density] = 0.0
    return v.astype(dtype)


def _exactly(shape, count, seed):
    """`count` non-zero voxels at random places."""
    g = np.random.default_rng(seed)
    v = np.zeros(shape, np.float32).reshape(-1)
    v[g.permutation(v.size)[:count]] = g.standard_normal(count).astype(np.float32) + np.float32(3.0) * g.choice([-1, 1], count).astype(np.float32)
    return v.reshape(shape)


CASES = {
    "density_0.02": lambda: _exactly((5, 16, 25), 40, 1),
    "odd_extents": lambda: _grid((5, 37, 53), 0.3, 2),
    "crop_346": lambda: _grid((5, 20, 346), 0.3, 3),
    "all_zero": lambda: np.zeros((5, 16, 25), np.float32),
    "positives_only": lambda: _grid((5, 37, 53), 0.3, 4, sign=1),
    "negatives_only": lambda: _grid((5, 37, 53), 0.3, 5, sign=-1),
    "fp16": lambda: _grid((5, 37, 53), 0.3, 6, dtype=np.float16),
    "many_blocks": lambda: _grid((5, 120, 346), 0.3, 7),             # more voxels than one workgroup of the statistics pass takes
}


def _run(x, norm, **kw):
    from devo_amd import frames
    out, rec = frames.frame_input(torch.from_numpy(x).to(DEV), norm, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rec.clone().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_input_against_the_restatement(case):
    x = CASES[case]()
    s = R.stats(x)
    bins, H, W = x.shape
    Wout = W - 2 if W == 346 else W
    for norm in ("none", "rescale", "std"):
        got, rec = _run(x, norm, gate=True)
        assert got.shape == (1, 1, bins, H, Wout) and got.dtype == np.float32
        assert rec[0] == s["nnz"] and rec[1] == s["numel"], (case, norm)                  # exact: the statistics include the dropped columns
        again, _ = _run(x, norm)
        assert np.array_equal(_bits(got), _bits(again)), (case, norm)                     # bit-reproducible from run to run
        want = R.frame_input(x, norm)
        if norm == "none":
            assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))
            assert rec[2] == 0.0 and rec[3] == 0.0
        elif norm == "rescale":
            assert np.array_equal(_bits(got), _bits(R.rescale_f32(x))), case
            assert rec[2] == s["pmax"] and rec[3] == s["nmax"]                            # the extrema are exact
        elif s["nnz"] == 0:
            assert np.array_equal(_bits(got), _bits(want.astype(np.float32)))             # returned as it is
        else:
            err, bound = np.abs(got.astype(np.float64) - want), R.std_bound(x)
            print(f"{case}: std worst error / bound = {float((err / bound).max()):.3f}, mean {s['mean']:.4f}, sigma {s['sigma']:.4f}")
            assert (err <= bound).all(), (case, float((err / bound).max()))
            assert abs(rec[2] - s["mean"]) <= 2.0 ** -23 * abs(s["mean"]) and abs(rec[3] - s["sigma"]) <= 2.0 ** -23 * s["sigma"]
            assert not got[want == 0.0].any()                                             # 0 elsewhere


def test_the_gate_is_exact_at_the_threshold():
    x = _exactly((5, 16, 25), 40, 11)
    _, rec = _run(x, "std", gate=True)
    assert (int(rec[0]), int(rec[1])) == (40, 2000) and not (int(rec[0]) / int(rec[1]) < 2e-2) and not R.skipped(x)      # exactly 0.02: kept
    y = x.copy().reshape(-1)
    y[np.flatnonzero(y)[0]] = 0.0
    y = y.reshape(x.shape)
    _, rec = _run(y, "std", gate=True)
    assert (int(rec[0]), int(rec[1])) == (39, 2000) and int(rec[0]) / int(rec[1]) < 2e-2 and R.skipped(y)                # 39: skipped


@pytest.mark.parametrize("value", [1.0, 1.1, -0.7, 3.3, 1e-3, 257.25])
def test_degenerate_grids_are_what_events_std_returns(value):
    """One non-zero voxel, and all non-zero voxels equal: sigma = 0, the quotient is 0 / 0 or 0 / (a rounding error) — whatever events.std
    makes of the grid is the package's answer, here too (NaN patterns included: compared as bits)."""
    from devo_amd import events, frames
    for count in (1, 37):
        x = np.zeros((5, 16, 25), np.float32).reshape(-1)
        x[np.random.default_rng(count).permutation(x.size)[:count]] = np.float32(value)
        v = torch.from_numpy(x.reshape(5, 16, 25)).to(DEV)
        want = events.std(v[None, None], sequence=False)
        got, _ = frames.frame_input(v, "std")
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (value, count)


def test_out_and_record_are_used_in_place_and_bad_arguments_raise():
    from devo_amd import frames
    x = torch.from_numpy(_grid((5, 20, 346), 0.3, 9)).to(DEV)
    out = torch.empty(1, 1, 5, 20, 344, device=DEV)
    rec = frames.pinned_record()
    got, r = frames.frame_input(x, "rescale", out=out, record=rec)
    assert got.data_ptr() == out.data_ptr() and r is rec
    torch.cuda.synchronize()
    assert rec[0] > 0 and rec[1] == x.numel()
    with pytest.raises(ValueError):
        frames.frame_input(x, "std", out=torch.empty(1, 1, 5, 20, 346, device=DEV))
    with pytest.raises(NotImplementedError):
        frames.frame_input(x, "minmax")
    with pytest.raises(ValueError):
        frames.frame_input(x[None], "std")
