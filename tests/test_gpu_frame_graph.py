"""devo_amd.frame_graph on the GPU against the fp64 oracle of tests/frame_graph_ref.py, on the scenes of tests/golden/frame_graph.npz.

Allowance: 4 x the deviation of the REFERENCE's own fp32 matrix from the oracle, measured per scene by the generator (`ref_dev`, as
max |a - b| / max(|b|, 1) over non-fragile finite entries) — the factor covers fused multiply-adds, another summation order and another
square root / division than torch's.  Entries whose decisions a rounding error can flip (the oracle's fragile mask: a point within 1e-4 of
the validity threshold, or the entry within 1e-4 * 256 of max_flow) are left out, at most 2 % per scene."""
import os
import numpy as np
import pytest
import torch

import frame_graph_ref as R
from devo_amd import frame_graph as FG

pytestmark = pytest.mark.gpu
SCENES = ("A", "B", "C", "E")
KEYS = ("poses", "depths", "intr", "disps", "matrix", "rowptr", "cols", "dists", "ref_dev", "disp_dev")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_graph.npz"))


@pytest.fixture(scope="module")
def scenes(golden):
    """Per scene: the golden arrays, the oracle (scaled matrix, fragile, tie, CSR) and the kernel's results, computed once."""
    f, max_flow = int(golden["f"]), float(golden["max_flow"])
    out = {}
    for name in SCENES:
        s = {k: golden[f"{name}/{k}"] for k in KEYS}
        s["f"], s["max_flow"] = f, max_flow
        s["oracle"], s["fragile"], s["tie"] = R.distance_oracle(s["poses"], s["disps"], s["intr"] / f, scale=float(f), max_flow=max_flow)
        s["lists"] = R.lists_oracle(s["oracle"], max_flow)
        s["matrix_gpu"] = FG.distance_matrix(s["poses"], s["disps"], s["intr"] / f).cpu()
        s["graph"] = FG.build_frame_graph(s["poses"], s["depths"], s["intr"], f=f, max_flow=max_flow)
        out[name] = s
    return out


def reference_dict(s):
    return {i: (s["cols"][a:b], s["dists"][a:b]) for i, (a, b) in enumerate(zip(s["rowptr"][:-1], s["rowptr"][1:]))}


@pytest.mark.parametrize("name", SCENES)
def test_matrix_against_oracle(scenes, name):
    s = scenes[name]
    got, oracle, fragile = s["matrix_gpu"], s["oracle"] / s["f"], s["fragile"]
    assert not bool(torch.isnan(got).any())
    solid = ~fragile
    assert float(fragile.double().mean()) <= 0.02
    assert bool((torch.isinf(got) == torch.isinf(oracle))[solid].all())
    finite = solid & torch.isfinite(oracle)
    dev = R.rel_dev(got[finite], oracle[finite])
    print(f"scene {name}: kernel vs oracle {dev:.3e}, allowance 4 x {float(s['ref_dev']):.3e}")
    assert dev <= 4 * float(s["ref_dev"])
    assert bool(torch.isfinite(got[s["tie"] & solid]).all())
    if name == "A":
        assert int(s["tie"].sum()) > 0 and bool(torch.isfinite(got[s["tie"]]).all())             # every tie entry is finite


@pytest.mark.parametrize("name", SCENES)
def test_lists_against_oracle(scenes, name):
    s = scenes[name]
    g, f = s["graph"], s["f"]
    assert g.rowptr.is_cuda and g.cols.is_cuda and g.dists.is_cuda and g.n == len(s["poses"])
    rowptr, cols, dists = (t.cpu() for t in (g.rowptr, g.cols, g.dists))
    o_rowptr, o_cols, o_dists = s["lists"]
    clean = ~s["fragile"].any(1)                                                                  # rows without a fragile entry
    worst = 0.0
    for i in range(g.n):
        a, b = int(rowptr[i]), int(rowptr[i + 1])
        c, d = cols[a:b], dists[a:b]
        assert bool((c[1:] > c[:-1]).all()) and int((c == i).sum()) == 1                          # strictly ascending, holds its own index
        keep = ~s["fragile"][i][c]                                                                # outside the fragile mask: the oracle's row
        oa, ob = int(o_rowptr[i]), int(o_rowptr[i + 1])
        oc, od = o_cols[oa:ob], o_dists[oa:ob]
        okeep = ~s["fragile"][i][oc]
        assert torch.equal(c[keep], oc[okeep])
        worst = max(worst, R.rel_dev(d[keep] / f, od[okeep] / f))
        if bool(clean[i]):
            assert b - a == ob - oa
    if bool(clean.all()):
        assert torch.equal(rowptr, o_rowptr) and torch.equal(cols, o_cols)
    print(f"scene {name}: dists vs oracle {worst:.3e}, allowance 4 x {float(s['ref_dev']):.3e}")
    assert worst <= 4 * float(s["ref_dev"])
    got_full = (FG.distance_matrix(s["poses"], FG.prepare_disps(s["depths"]), s["intr"] / f) * f).cpu()
    assert torch.equal(dists, got_full[got_full < s["max_flow"]])                                  # the lists are the matrix's entries, row-major


@pytest.mark.parametrize("name", SCENES)
def test_symmetric_and_reproducible(scenes, name):
    s = scenes[name]
    m = s["matrix_gpu"]
    assert torch.equal(m.view(torch.int32), m.t().contiguous().view(torch.int32))
    again = FG.distance_matrix(s["poses"], s["disps"], s["intr"] / s["f"]).cpu()
    assert torch.equal(m.view(torch.int32), again.view(torch.int32))
    g2 = FG.build_frame_graph(s["poses"], s["depths"], s["intr"], f=s["f"], max_flow=s["max_flow"])
    for a, b in zip((s["graph"].rowptr, s["graph"].cols, s["graph"].dists.view(torch.int32)), (g2.rowptr, g2.cols, g2.dists.view(torch.int32))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", (1, 2))
def test_tiny_scenes(scenes, n):
    s = scenes["B"]
    f = s["f"]
    poses, disps, intr = s["poses"][:n], s["disps"][:n], s["intr"][:n] / f
    got = FG.distance_matrix(poses, disps, intr).cpu()
    oracle, fragile, _ = R.distance_oracle(poses, disps, intr, scale=1.0, max_flow=s["max_flow"] / f)
    assert got.shape == (n, n) and not bool(fragile.any()) and bool(torch.isfinite(got).all())
    assert R.rel_dev(got, oracle) <= 4 * float(s["ref_dev"])
    assert float(got[0, 0]) > 0                                                                   # the fixed pose of a frame against itself
    g = FG.build_frame_graph(s["poses"][:n], s["depths"][:n], s["intr"][:n], f=f, max_flow=s["max_flow"])
    assert g.n == n and int(g.rowptr[-1]) == int((got * f < s["max_flow"]).sum())
    assert 0 in g.neighbours(0)[0]


def test_no_valid_point_is_inf_not_nan():
    """Two frames back to back: no point of either lies in front of the other."""
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1, 0, 1, 0, 0]], np.float32)                   # the second turned by pi about y
    disps = np.full((2, 5, 8), 0.5, np.float32)
    intr = np.tile(np.array([20.0, 20.0, 4.0, 2.5], np.float32), (2, 1))
    V = R.directed_sums(poses, disps, intr)[1]
    assert int(V[0, 1]) == 0 and int(V[1, 0]) == 0
    got = FG.distance_matrix(poses, disps, intr).cpu()
    assert not bool(torch.isnan(got).any())
    assert bool(torch.isinf(got[0, 1])) and bool(torch.isinf(got[1, 0])) and float(got[0, 1]) > 0 and bool(torch.isfinite(got.diagonal()).all())


@pytest.mark.parametrize("name", ("A", "B"))
def test_disparity_preparation(scenes, name):
    s = scenes[name]
    got = FG.prepare_disps(s["depths"]).cpu().numpy()
    oracle, low = R.disps_oracle(s["depths"])
    low = low.numpy()
    assert low.sum() >= 3
    assert got[~low].tobytes() == (np.float32(1) / s["depths"])[~low].tobytes()
    dev = R.rel_dev(got[low], oracle.numpy()[low])
    print(f"scene {name}: replaced disparities vs oracle {dev:.3e}, allowance 4 x {float(s['disp_dev']):.3e}")
    assert dev <= 4 * float(s["disp_dev"])


def test_reference_dict_and_clips(scenes, golden):
    s = scenes["A"]
    got, ref, fragile = s["graph"].to_reference(), reference_dict(s), s["fragile"]
    assert list(got) == list(ref)
    for i in ref:
        c, d = got[i]
        assert c.dtype == np.int64 and d.dtype == np.float32
        keep, rkeep = ~fragile[i][c].numpy(), ~fragile[i][ref[i][0]].numpy()
        assert np.array_equal(c[keep], ref[i][0][rkeep])
        assert R.rel_dev(d[keep] / s["f"], ref[i][1][rkeep] / s["f"]) <= 4 * float(s["ref_dev"])
    n_frames, fmin, fmax = int(golden["clips/n_frames"]), float(golden["clips/fmin"]), float(golden["clips/fmax"])
    for k in range(int(golden["clips/n"])):
        start, seed, sample, inds = (golden[f"clips/{k}/{key}"] for key in ("start", "seed", "sample", "inds"))
        assert not bool(fragile[inds[:-1]].any())                                                 # the rows the walk reads hold no fragile entry
        np.random.seed(int(seed))
        assert np.array_equal(s["graph"].sample_clip(int(start), n_frames, fmin, fmax, s["graph"].n, sample=bool(sample)), inds), k


def test_chunked_composition_agrees(scenes):
    """The reference's composition restated in torch, on the GPU, against the kernel: scene B, under the same rule."""
    s = scenes["B"]
    dev = torch.device("cuda")
    ref = torch.from_numpy(R.chunked_distance_matrix(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (s["poses"], s["disps"], s["intr"] / s["f"]))))
    got, solid = s["matrix_gpu"], ~s["fragile"]
    assert bool((torch.isinf(got) == torch.isinf(ref))[solid].all())
    finite = solid & torch.isfinite(ref)
    dev_ = R.rel_dev(got[finite], ref[finite])
    print(f"scene B: kernel vs chunked torch composition {dev_:.3e}, allowance 4 x {float(s['ref_dev']):.3e}")
    assert dev_ <= 4 * float(s["ref_dev"])
    assert bool(((got * s["f"] < s["max_flow"]) == (ref * s["f"] < s["max_flow"]))[solid].all())


def test_argument_errors(scenes):
    s = scenes["C"]
    f = s["f"]
    with pytest.raises(RuntimeError, match="2 h w"):
        FG.distance_matrix(s["poses"][:1], torch.ones(1, 1024, 512, device="cuda"), s["intr"][:1] / f)      # 2 h w = 2^20
    with pytest.raises(RuntimeError, match="2 h w"):
        FG.prepare_disps(torch.ones(1, 1024, 512, device="cuda"))
    with pytest.raises((ValueError, RuntimeError)):
        FG.distance_matrix(s["poses"][:3], s["disps"], s["intr"] / f)
    with pytest.raises((ValueError, RuntimeError)):
        FG.build_frame_graph(s["poses"], s["depths"], s["intr"][:4], f=f)
    with pytest.raises(RuntimeError, match="GPU"):
        FG.distance_matrix(torch.from_numpy(s["poses"]), torch.from_numpy(s["disps"]), torch.from_numpy(s["intr"] / f))
    with pytest.raises(RuntimeError, match="GPU"):
        FG.build_frame_graph(torch.from_numpy(s["poses"]), torch.from_numpy(s["depths"]), torch.from_numpy(s["intr"]))
