"""The frame graph without a GPU: the fp64 oracle (tests/frame_graph_ref.py) against the reference's own results in
tests/golden/frame_graph.npz (tools/gen_golden_frame_graph.py), the conditions the scenes were chosen under, and the host side of
devo_amd.frame_graph.FrameGraph: the dict round trip, the dataset index and the clip sampler against EVSDDataset.__getitem__'s indices."""
import os
import numpy as np
import pytest
import torch

import frame_graph_ref as R
from devo_amd.frame_graph import FrameGraph

SCENES = ("A", "B", "C", "E")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_graph.npz"))


def scene(golden, name):
    return {k: golden[f"{name}/{k}"] for k in ("poses", "depths", "intr", "disps", "matrix", "rowptr", "cols", "dists", "ref_dev", "disp_dev")}


def reference_dict(s):
    return {i: (s["cols"][a:b], s["dists"][a:b]) for i, (a, b) in enumerate(zip(s["rowptr"][:-1], s["rowptr"][1:]))}


def oracle_of(golden, s):
    f = float(golden["f"])
    matrix, fragile, tie = R.distance_oracle(s["poses"], s["disps"], s["intr"] / f, scale=f, max_flow=float(golden["max_flow"]))
    return matrix, fragile, tie


@pytest.mark.parametrize("name", SCENES)
def test_oracle_matches_the_reference(golden, name):
    s = scene(golden, name)
    f, max_flow = float(golden["f"]), float(golden["max_flow"])
    matrix, fragile, tie = oracle_of(golden, s)
    ref = torch.from_numpy(s["matrix"])
    solid = ~fragile
    assert bool((torch.isinf(ref) == torch.isinf(matrix))[solid].all())
    finite = solid & torch.isfinite(matrix)
    dev = R.rel_dev(ref[finite], matrix[finite] / f)
    print(f"scene {name}: oracle vs reference {dev:.3e}, stored ref_dev {float(s['ref_dev']):.3e}")
    assert dev <= 4 * float(s["ref_dev"])
    assert bool(((f * ref < max_flow) == (matrix < max_flow))[solid].all())                    # list membership
    assert not bool(torch.isinf(ref[tie & solid]).any())                                       # the reference keeps the tie finite
    # the lists of the oracle are the reference's dict wherever no fragile entry is involved
    rowptr, cols, dists = R.lists_oracle(matrix, max_flow)
    for i, (c, d) in reference_dict(s).items():
        if bool(fragile[i].any()):
            continue
        a, b = int(rowptr[i]), int(rowptr[i + 1])
        assert np.array_equal(cols[a:b].numpy(), c)
        assert R.rel_dev(d / f, dists[a:b] / f) <= 4 * float(s["ref_dev"])
    # the disparity preparation
    d_oracle, low = R.disps_oracle(s["depths"])
    assert np.array_equal(s["disps"][~low.numpy()], (np.float32(1) / s["depths"])[~low.numpy()])
    assert R.rel_dev(s["disps"][low.numpy()], d_oracle[low]) <= max(float(s["disp_dev"]), 0.0)


@pytest.mark.parametrize("name", ("A", "B"))
def test_scene_conditions(golden, name):
    s = scene(golden, name)
    f, max_flow = float(golden["f"]), float(golden["max_flow"])
    matrix, fragile, tie = oracle_of(golden, s)
    ref = f * s["matrix"]
    n = ref.size
    for count in (np.isinf(ref).sum(), (np.isfinite(ref) & (ref >= max_flow)).sum(), (ref < max_flow).sum()):
        assert count >= 8 and count >= 0.01 * n
    assert float(fragile.double().mean()) <= 0.02
    if name == "A":
        assert s["depths"].shape == (33, 5, 8) and bool((tie & ~fragile).any())
    else:
        assert s["depths"].shape == (40, 6, 8)
    intr = s["intr"]
    assert len(np.unique(intr[:, 0])) == len(intr) and bool((intr[:, 0] != intr[:, 1]).all()) and int((s["depths"] < 0.01).sum()) >= 3


def test_clamp_scene(golden):
    s = scene(golden, "E")
    f = float(golden["f"])
    matrix, fragile, _ = oracle_of(golden, s)
    peak = R.directed_sums(s["poses"], s["disps"], s["intr"] / f)[3]
    assert float(peak[0, 1]) > 100.0 and bool(torch.isfinite(matrix[0, 1])) and not bool(fragile[0, 1])


@pytest.mark.parametrize("name", SCENES)
def test_reference_round_trip(golden, name):
    s = scene(golden, name)
    ref = reference_dict(s)
    g = FrameGraph.from_reference(ref)
    assert g.n == len(ref) and not g.rowptr.is_cuda
    assert np.array_equal(g.rowptr.numpy(), s["rowptr"]) and g.cols.dtype == torch.int64 and g.dists.dtype == torch.float32
    back = g.to_reference()
    assert list(back) == list(ref)
    for i in ref:
        assert back[i][0].dtype == np.int64 and back[i][1].dtype == np.float32
        assert np.array_equal(back[i][0], ref[i][0]) and back[i][1].tobytes() == ref[i][1].tobytes()
        c, d = g.neighbours(i)
        assert np.array_equal(c, ref[i][0]) and np.array_equal(d, ref[i][1])
    with pytest.raises(ValueError):
        FrameGraph.from_reference({1: ref[0]})


def test_dataset_index(golden):
    ref = reference_dict(scene(golden, "A"))
    g = FrameGraph.from_reference(ref)
    for n_frames in (0, 6, 15, 40):
        assert g.dataset_index(n_frames) == [i for i in ref if len(ref[i][0]) > n_frames]
    assert g.dataset_index(40) == [] and len(g.dataset_index(0)) == g.n                       # every frame is its own neighbour


def test_sample_clip_reproduces_the_reference(golden):
    g = FrameGraph.from_reference(reference_dict(scene(golden, "A")))
    n_frames, fmin, fmax = int(golden["clips/n_frames"]), float(golden["clips/fmin"]), float(golden["clips/fmax"])
    modes, backward = set(), set()
    for k in range(int(golden["clips/n"])):
        start, seed, sample, inds = (golden[f"clips/{k}/{key}"] for key in ("start", "seed", "sample", "inds"))
        np.random.seed(int(seed))
        got = g.sample_clip(int(start), n_frames, fmin, fmax, g.n, sample=bool(sample))
        assert got.dtype == np.int64 and np.array_equal(got, inds), (k, got, inds)
        modes.add(bool(sample))
        if (np.diff(inds) < 0).any():
            backward.add(bool(sample))
    assert modes == {True, False} and backward == {True, False}
