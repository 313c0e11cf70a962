"""Host-side checks of devo_amd/data.py (the training sample's tail): the draws against the reference's (tests/golden/train_sample.npz,
tools/gen_golden_train_sample.py), the crop geometry, and that CPU tensors and crops larger than the image are refused."""
import os
import numpy as np
import pytest
import torch

from devo_amd import data

CROP = (8, 120)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "train_sample.npz"))


def _seeds(gold, prefix):
    return sorted({int(k.split("/")[1]) for k in gold.files if k.startswith(prefix)})


def test_draw_reproduces_reference_scales(gold):
    aug = data.EVSDAugmentor(list(CROP))
    seeds = _seeds(gold, "aug/")
    assert len(seeds) >= 5
    branches = set()
    for s in seeds:
        np.random.seed(s)
        p = aug.draw(11, 141)
        branch = int(gold[f"aug/{s}/branch"])
        branches.add(branch)
        assert p["scale"] == float(gold[f"aug/{s}/scale"]), s
        assert (p["scale"] != 1) == bool(branch)
        assert isinstance(p["seed"], int)
    assert branches == {0, 1}                                   # both the zoom and the scale-1 branch are covered


def test_draw_fix_scale(gold):
    aug = data.EVSDAugmentor(list(CROP))
    for f in (0.9, 1.25):
        for s in (0, 1):
            np.random.seed(s)
            assert aug.draw(11, 141, fix_scale=f)["scale"] == float(gold[f"fix/{f}/{s}/scale"])
    np.random.seed(0)
    assert aug.draw(11, 141, fix_scale=1.25)["scale"] == 1.25    # log2(1.25) >= max_scale: no draw


def test_draw_order_matches_numpy_stream():
    """draw() consumes np.random exactly as the reference does: rand, then uniform only when rand < 0.8."""
    aug = data.EVSDAugmentor([10, 10])
    for s in range(20):
        np.random.seed(s)
        aug.draw(20, 20)
        after = np.random.rand()
        np.random.seed(s)
        r = np.random.rand()
        if r < 0.8:
            np.random.uniform(0, 1)
        assert after == np.random.rand()


def test_crop_geometry_matches_golden_shapes(gold):
    aug = data.EVSDAugmentor(list(CROP))
    for s in _seeds(gold, "aug/"):
        Hs, Ws, y0, x0 = aug.crop(11, 141, {"scale": float(gold[f"aug/{s}/scale"]), "seed": 0})
        assert gold[f"aug/{s}/v"].shape[-2:] == CROP
        assert y0 >= 0 and x0 >= 0 and y0 + CROP[0] <= Hs and x0 + CROP[1] <= Ws


def test_crop_larger_than_image_raises():
    aug = data.EVSDAugmentor([20, 200])
    with pytest.raises(ValueError, match="smaller than the crop"):
        aug.crop(11, 141, {"scale": 1.0, "seed": 0})
    with pytest.raises(ValueError, match="smaller than the crop"):
        data.EVSDAugmentor([8, 120]).crop(11, 141, {"scale": 0.7, "seed": 0})


def test_cpu_tensors_refused():
    v = torch.zeros(1, 2, 2, 11, 141)
    d = torch.ones(1, 2, 11, 141)
    p = torch.zeros(1, 2, 7)
    k = torch.ones(1, 2, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        data.prepare_batch(v, p, d, k, CROP)
    with pytest.raises(RuntimeError, match="GPU"):
        data.normalise_depth(d, p)
    with pytest.raises(RuntimeError, match="GPU"):
        data.voxel_color_jitter(v[0])
    with pytest.raises(RuntimeError, match="GPU"):
        data.transform_rescale(0.5, v[0], d[0])
    with pytest.raises(RuntimeError, match="GPU"):
        data.EVSDAugmentor(list(CROP)).apply(v[0], p[0], d[0], k[0], {"scale": 1.0, "seed": 0})


def test_jitter_amplitude_is_fixed():
    with pytest.raises(ValueError):
        data.voxel_color_jitter(torch.zeros(1, 1, 2, 2), EPS=1e-3)
