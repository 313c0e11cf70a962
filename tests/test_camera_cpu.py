"""CPU checks of the camera module: tests/camera_ref.py (the numpy restatement test_gpu_camera.py compares the kernels with) against
itself — round trips, a closed-form known answer, its two inverse formulations — and the host side of devo_amd.camera: `new_camera_matrix`
against the restatement and the prototype figures of the rule text, the coverage properties of alpha = 0 / alpha = 1, `Camera` validation,
and the C ABI's names."""
import os
import re

import numpy as np
import pytest
import torch

import camera_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def C():
    from devo_amd import camera
    return camera


def _cam(name):
    return C().Camera(*T.FIXTURES[name])


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("name", sorted(T.MILD))
def test_oracle_round_trip_and_two_formulations(name):
    """distort(undistort(p)) = p on every pixel, every pixel valid, and the fixed-point / bisection inverse agrees with the Newton one
    within the figure the header records (in pixels of K_new, over the rotations)"""
    fx = T.MILD[name]
    grid = T.pixel_grid(*fx[3])
    K_new = T.new_camera_matrix(fx)
    (a, ok_a, _), (b, ok_b, _) = T.grid_normalised(name, "independent"), T.grid_normalised(name, "newton")
    assert ok_a.all() and ok_b.all()
    for R in T.ROTATIONS.values():
        pa, pb = T.project(a, K_new, R), T.project(b, K_new, R)
        assert np.abs(pa - pb).max() <= 2 * T.MEASURED_DISAGREEMENT_PX          # (another libm may move the last bits)
        back = T.distort(fx, pa, K_new, R)
        assert np.abs(back - grid).max() < 1e-9, (name, np.abs(back - grid).max())


def test_measured_disagreement_is_what_the_header_records():
    worst = max(T.measure_disagreement().values())
    assert 0.25 * T.MEASURED_DISAGREEMENT_PX <= worst <= 2 * T.MEASURED_DISAGREEMENT_PX, worst     # the recorded figure is a measurement, not a guess
    assert T.PX_TOL == 16 * T.MEASURED_DISAGREEMENT_PX


def test_oracle_pure_radial_known_answer():
    """k1 only: x_d = x (1 + k1 r^2) in closed form; both inverses recover x"""
    k1 = -0.2
    x = np.array([0.3, -0.5, 0.0, 0.45])
    y = np.array([0.4, 0.1, -0.6, 0.45])
    s = 1.0 + k1 * (x * x + y * y)
    xd, yd = x * s, y * s
    K, dist = (100.0, 110.0, 50.0, 40.0), (k1, 0.0, 0.0, 0.0)
    px = np.stack([K[0] * xd + K[2], K[1] * yd + K[3]], 1)
    for method in ("independent", "newton"):
        got, ok, _ = T.undistort_normalised("radtan", K, dist, px, method)
        assert ok.all() and np.abs(got - np.stack([x, y], 1)).max() < 1e-14
    # equidistant with no coefficients: theta_d = theta, r = tan(theta)
    theta = np.array([0.2, 0.9, 1.4])
    px = np.stack([K[0] * theta + K[2], np.full(3, K[3])], 1)
    for method in ("independent", "newton"):
        got, ok, _ = T.undistort_normalised("equidistant", K, (0.0, 0.0, 0.0, 0.0), px, method)
        assert ok.all() and np.abs(got[:, 0] - np.tan(theta)).max() < 1e-13 and np.abs(got[:, 1]).max() == 0.0


def test_oracle_folding_fixtures_have_the_stated_shape():
    _, ok, margin = T.grid_normalised("fold_radtan", "newton")
    assert abs(ok.mean() - 0.335) < 0.001 and int((ok & (margin <= 0.05)).sum()) == 88
    _, ok, _ = T.grid_normalised("fold_equi", "independent")
    assert 0 < (~ok).sum() < ok.size
    theta = np.arctan(np.hypot(*T.grid_normalised("equi346")[0].T))
    assert abs(np.degrees(theta.max()) - 81.6) < 0.05


def test_oracle_remap():
    img = np.arange(2 * 3 * 4 * 1, dtype=np.float64).reshape(2, 3, 4, 1)
    coords = np.array([[[0.0, 0.0], [2.5, 1.0], [-0.5, 0.0], [3.5, 2.0], [np.nan, 1.0], [4.0, 0.0]]], dtype=np.float32)
    out = T.remap(img, coords)[:, 0, :, 0]
    assert np.array_equal(out[0], [0.0, 6.5, 0.0, 5.5, 0.0, 0.0]) and np.array_equal(out[1], [12.0, 18.5, 6.0, 11.5, 0.0, 0.0])
    assert np.array_equal(T.to_uint8(np.array([0.5, 1.5, 2.5, -3.0, 300.0])), [0, 2, 2, 0, 255])


# ------------------------------------------------------------------------------------------------ new_camera_matrix
PROTOTYPE = [("davis240", dict(alpha=0.0), (169.375, 179.559, 136.270, 114.282)), ("davis240", dict(alpha=1.0), (155.303, 155.505, 132.803, 111.481)),
             ("equi1280", dict(balance=0.0), (996.958, 996.673, 633.326, 254.217)), ("equi1280", dict(balance=0.5), (948.385, 948.114, 633.651, 259.371))]


@pytest.mark.parametrize("name,kw,want", PROTOTYPE)
def test_new_camera_matrix_prototype_rows(name, kw, want):
    got = C().new_camera_matrix(_cam(name), **kw)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-3, got


@pytest.mark.parametrize("name", sorted(T.MILD) + ["fold_equi"])
def test_new_camera_matrix_against_the_restatement(name):
    cam, fx = _cam(name), T.FIXTURES[name]
    cases = [dict(balance=b) for b in (0.0, 0.3, 1.0)] if fx[0] == "equidistant" else [dict(alpha=a) for a in (0.0, 0.4, 1.0)]
    for kw in cases:
        for new_size in (None, (fx[3][0] // 2 + 1, fx[3][1] * 2)):
            got, want = np.array(C().new_camera_matrix(cam, new_size=new_size, **kw)), np.array(T.new_camera_matrix(fx, new_size=new_size, **kw))
            assert (np.abs(got - want) <= 1e-9 * np.abs(want)).all(), (name, kw, new_size, got, want)


def test_new_camera_matrix_of_a_pinhole_is_its_own_matrix():
    cam = C().Camera("pinhole", (300.0, 310.0, 160.5, 119.25), (), (320, 240))
    for alpha in (0.0, 1.0):
        assert np.allclose(C().new_camera_matrix(cam, alpha=alpha), cam.K, rtol=1e-12)
    assert np.allclose(C().new_camera_matrix(cam, new_size=(640, 240)), (300.0 * 639 / 319, 310.0, 160.5 * 639 / 319, 119.25), rtol=1e-12)


def test_new_camera_matrix_refusals():
    with pytest.raises(ValueError, match="fold"):
        C().new_camera_matrix(_cam("fold_radtan"))
    with pytest.raises(ValueError, match="balance"):
        C().new_camera_matrix(_cam("davis240"), balance=0.5)
    with pytest.raises(ValueError, match="alpha"):
        C().new_camera_matrix(_cam("davis240"), alpha=1.5)
    with pytest.raises(ValueError, match="balance"):
        C().new_camera_matrix(_cam("equi346"), balance=-0.1)


@pytest.mark.parametrize("name", ["davis240", "radtan640", "pincushion"])
def test_alpha_zero_sources_lie_inside_and_alpha_one_keeps_every_corner(name):
    """alpha = 0: at least 99.8 % of the undistorted image's pixels have their source inside the raw image (the 9 x 9 sample leaves a sliver);
    alpha = 1: every raw corner lands inside [-0.5, W - 0.5] x [-0.5, H - 0.5] of the new image"""
    cam, fx = _cam(name), T.MILD[name]
    W, H = fx[3]
    K0 = C().new_camera_matrix(cam, alpha=0.0)
    src = T.distort(fx, T.pixel_grid(W, H), K0)
    inside = (src[:, 0] >= 0) & (src[:, 0] <= W - 1) & (src[:, 1] >= 0) & (src[:, 1] <= H - 1)
    assert inside.mean() >= 0.998, inside.mean()
    K1 = C().new_camera_matrix(cam, alpha=1.0)
    corners = np.array([[0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0]])
    p, ok, _ = T.undistort(fx, corners, K1)
    assert ok.all() and (p[:, 0] >= -0.5).all() and (p[:, 0] <= W - 0.5).all() and (p[:, 1] >= -0.5).all() and (p[:, 1] <= H - 0.5).all(), p


# ------------------------------------------------------------------------------------------------ Camera, the ABI, no fallback
def test_camera_validation():
    Cam = C().Camera
    cam = Cam("radtan", [1.0, 2.0, 3.0, 4.0], np.zeros(4), size=[10, 8])
    assert cam.K == (1.0, 2.0, 3.0, 4.0) and cam.dist == (0.0,) * 4 and cam.size == (10, 8) and hash(cam) == hash(Cam("radtan", (1, 2, 3, 4), (0, 0, 0, 0), (10, 8)))
    with pytest.raises(Exception):
        cam.model = "pinhole"                                          # frozen
    for model in ("fisheye", "", "RADTAN"):
        with pytest.raises(ValueError, match="model"):
            Cam(model, (1, 1, 0, 0), (), (4, 4))
    for model, n in (("pinhole", 1), ("pinhole", 4), ("radtan", 0), ("radtan", 3), ("radtan", 6), ("radtan", 8), ("equidistant", 0), ("equidistant", 3), ("equidistant", 5)):
        with pytest.raises(ValueError, match="entries"):
            Cam(model, (1, 1, 0, 0), (0.0,) * n, (4, 4))
    for K in ((1, 1, 0), (1, 1, 0, 0, 0)):
        with pytest.raises(ValueError, match="entries"):
            Cam("pinhole", K, (), (4, 4))
    for K in ((float("nan"), 1, 0, 0), (1, float("inf"), 0, 0), (1, 1, float("nan"), 0)):
        with pytest.raises(ValueError, match="non-finite"):
            Cam("pinhole", K, (), (4, 4))
    with pytest.raises(ValueError, match="non-finite"):
        Cam("radtan", (1, 1, 0, 0), (0, float("nan"), 0, 0), (4, 4))
    for K in ((0, 1, 0, 0), (1, -1, 0, 0)):
        with pytest.raises(ValueError, match="positive"):
            Cam("pinhole", K, (), (4, 4))
    for size in ((0, 4), (4,), (4.5, 4), (4, -1)):
        with pytest.raises(ValueError, match="size"):
            Cam("pinhole", (1, 1, 0, 0), (), size)


def test_header_lists_the_camera_entry_points_and_the_version_stays():
    txt = open(os.path.join(ROOT, "include", "devo_hip.h")).read()
    assert re.search(r"#define\s+DEVO_ABI_VERSION\s+9\b", txt)
    version_comment = txt[txt.index("#define DEVO_ABI_VERSION"):txt.index("int devo_abi_version(void)")]
    from devo_amd import _lib
    for name in ("devo_camera_undistort_points", "devo_camera_distort_points", "devo_image_remap"):
        assert name in version_comment and re.search(r"\bint " + name + r"\(", txt) and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 9
    assert "camera.hip" in __import__("devo_amd.build", fromlist=["SOURCES"]).SOURCES
    import devo_amd
    assert devo_amd.camera is C()


def test_cpu_tensors_raise():
    cam = _cam("davis240")
    with pytest.raises(RuntimeError, match="GPU"):
        C().undistort_points(torch.zeros(4, 2), cam)
    with pytest.raises(RuntimeError, match="GPU"):
        C().distort_points(torch.zeros(4, 2), cam, cam.K)
    with pytest.raises(RuntimeError, match="GPU"):
        C().remap(torch.zeros(1, 4, 4, 1), torch.zeros(2, 2, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        C().undistort_images(torch.zeros(1, 180, 240, 3, dtype=torch.uint8), cam)
    with pytest.raises(RuntimeError, match="GPU"):
        C().rectify_map(cam, device="cpu")
