"""devo_amd.camera (csrc/camera.hip) against tests/camera_ref.py (the numpy fp64 restatement, itself checked in test_camera_cpu.py).
Point outputs: fp32 maps within one fp32 ulp of the restatement's value, fp64 outputs within camera_ref.PX_TOL = 16 x the disagreement of
the restatement's two inverse formulations.  Validity is stated so that no borderline pixel decides.  The remap is held to
16 * 2^-24 * max|image| of the real bilinear value on the same fp32 map.  The restatement's grids are computed once per fixture and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import camera_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def C():
    from devo_amd import camera
    return camera


@functools.lru_cache(maxsize=None)
def _cam(name):
    return C().Camera(*T.FIXTURES[name])


@functools.lru_cache(maxsize=None)
def _K_new(name):
    if name == "fold_radtan":                                          # (its 9 x 9 sample crosses the fold: new_camera_matrix refuses it)
        return T.FIXTURES[name][1]
    return C().new_camera_matrix(_cam(name))


@functools.lru_cache(maxsize=None)
def _grid(name, dtype=torch.float64):
    return torch.from_numpy(T.pixel_grid(*T.FIXTURES[name][3])).to(DEV, dtype)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _R(key):
    return T.ROTATIONS[key]


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """the grids kept on the device for this module and the module's map cache go when its last test has run, and the allocator's cached
    blocks with them: later test modules find the device as they would without this one"""
    yield
    _grid.cache_clear()
    C().clear_cache()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ point outputs
def _K_off(name):
    """the default matrix with its principal point moved by a fraction of a pixel.  alpha = 0 puts the outermost sample of the left column
    and of the top row at coordinate 0 EXACTLY, and where that sample is a pixel (a corner, for the pincushion fixture) the map's entry is
    the residue of a cancellation, ~1e-14: one fp32 ulp of such a value is far below the fp64 rounding of the projection itself, in the
    restatement as much as in the kernel, and the ulp criterion says nothing there.  No entry is such a residue with this matrix."""
    fx, fy, cx, cy = _K_new(name)
    return (fx, fy, cx + 0.37, cy + 0.21)


@pytest.mark.parametrize("name", sorted(T.MILD))
def test_rectify_map_is_the_oracle_rounded_to_fp32(name):
    """every entry within one fp32 ulp of the restatement's fp64 value; no NaN, invalid count 0; [H, W, 2] as events.voxel_grids takes it"""
    W, H = T.MILD[name][3]
    m, invalid = C().rectify_map(_cam(name), _K_off(name), return_invalid=True)
    assert m.shape == (H, W, 2) and m.dtype == torch.float32 and m.is_cuda and m.is_contiguous()
    assert invalid.dtype == torch.int32 and int(invalid) == 0
    got = m.cpu().numpy().reshape(-1, 2).astype(np.float64)
    want = T.project(T.grid_normalised(name)[0], _K_off(name))
    assert np.isfinite(got).all()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = (np.abs(got - want) / ulp).max()
    print(name, "worst |map - oracle| in fp32 ulps:", worst, " smallest |oracle value|:", np.abs(want).min())
    assert worst <= 1.0, worst
    d = C().rectify_map(_cam(name))                                     # K_new=None is new_camera_matrix(cam): the same map, moved
    assert torch.equal(_bits(d), _bits(C().rectify_map(_cam(name), _K_new(name))))
    assert float((d - m + torch.tensor([0.37, 0.21], device=DEV)).abs().max()) <= 3 * np.spacing(np.float32(float(d.abs().max()) + 1.0))   # three fp32 roundings


@pytest.mark.parametrize("rot", sorted(T.ROTATIONS))
@pytest.mark.parametrize("name", sorted(T.MILD))
def test_undistort_points_fp64_and_the_way_back(name, rot):
    """fp64 in, fp64 out, with and without a 5 degree rectifying rotation: within PX_TOL of the restatement, and distort_points brings every
    point back to its pixel within the same tolerance"""
    cam, K_new, R = _cam(name), _K_new(name), _R(rot)
    got = C().undistort_points(_grid(name), cam, K_new, R)
    assert got.dtype == torch.float64 and got.shape == _grid(name).shape
    want = T.project(T.grid_normalised(name)[0], K_new, R)
    err = np.abs(got.cpu().numpy() - want).max()
    back = C().distort_points(got, cam, K_new, R)
    err_back = float((back - _grid(name)).abs().max())
    print(name, rot, "max |gpu - oracle| px:", err, " round trip px:", err_back, " tolerance:", T.PX_TOL)
    assert err <= T.PX_TOL and err_back <= T.PX_TOL
    if rot != "none":
        assert np.abs(want - T.project(T.grid_normalised(name)[0], K_new)).max() > 1.0     # (the rotation is not a no-op)


@pytest.mark.parametrize("name", sorted(T.FIXTURES))
def test_given_points_equal_the_in_kernel_grid_bit_for_bit(name):
    cam, K_new = _cam(name), _K_new(name)
    W, H = cam.size
    m = C().rectify_map(cam, K_new)
    for dt in (torch.float32, torch.float64):                           # (the grid's integers are exact in both)
        p = C().undistort_points(_grid(name, dt).view(H, W, 2), cam, K_new)
        assert p.dtype == dt and p.shape == (H, W, 2)
        assert torch.equal(_bits(p.float()), _bits(m)), dt
    s = C().undistort_map(cam, K_new)
    d = C().distort_points(_grid(name, torch.float32), cam, K_new)
    assert torch.equal(_bits(d.view(H, W, 2)), _bits(s))


def test_normalised_output_pinhole_and_distort_against_the_oracle():
    """K_new=None gives normalised coordinates; a pinhole camera's map is the grid; distort_points / undistort_map against the restatement,
    with a rotation, and NaN behind the camera"""
    name = "pincushion"
    cam, fx = _cam(name), T.MILD[name]
    got = C().undistort_points(_grid(name), cam).cpu().numpy()
    assert np.abs(got - T.grid_normalised(name)[0]).max() <= T.PX_TOL / min(_K_new(name)[:2])
    pin = C().Camera("pinhole", (250.0, 251.0, 170.2, 130.7), (), (346, 260))
    m = C().rectify_map(pin, pin.K).cpu().numpy().reshape(-1, 2)
    grid = T.pixel_grid(346, 260)
    assert (np.abs(m - grid) <= np.spacing(grid.astype(np.float32)) + 1e-12).all()      # (K K^-1 in fp64 leaves ~1e-14 px where the pixel is 0)
    for rot in ("none", "ry"):
        K_new, R = _K_new(name), _R(rot)
        ideal = torch.from_numpy(T.pixel_grid(50, 40) * 7.0 - 20.0).to(DEV)
        want = T.distort(fx, ideal.cpu().numpy(), K_new, R)
        got = C().distort_points(ideal, cam, K_new, R).cpu().numpy()
        assert np.isfinite(want).all() and np.abs(got - want).max() <= T.PX_TOL
    Rb = T.rotation(1, 100.0)                                           # most of the image looks backwards
    ideal = torch.from_numpy(T.pixel_grid(30, 20) * 10.0).to(DEV)
    want = T.distort(fx, ideal.cpu().numpy(), _K_new(name), Rb)
    got = C().distort_points(ideal, cam, _K_new(name), Rb).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and 0 < np.isnan(want[:, 0]).sum() < len(want)
    ok = ~np.isnan(want[:, 0])
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.maximum(1.0, np.abs(want[ok]))).all()
    k = C().new_camera_matrix(cam, new_size=(173, 130))
    assert torch.equal(C().undistort_map(cam, out_size=(173, 130)), C().undistort_map(cam, k, out_size=(173, 130)))
    k = (k[0], k[1], k[2] + 0.37, k[3] + 0.21)                          # (_K_off: the default matrix sends a corner to source coordinate 0 up to rounding)
    m = C().undistort_map(cam, k, out_size=(173, 130)).cpu().numpy().reshape(-1, 2).astype(np.float64)
    want = T.distort(fx, T.pixel_grid(173, 130), k)
    assert m.shape == want.shape and (np.abs(m - want) <= np.spacing(np.abs(want).astype(np.float32))).all()


# ------------------------------------------------------------------------------------------------ validity
@pytest.mark.parametrize("name", sorted(T.FOLDING))
def test_validity_on_the_folding_fixtures(name):
    """every pixel the kernel calls valid round-trips through the restatement's forward model to 1e-6 px; every pixel the restatement calls
    valid with margin (min det J > 0.05; theta_d < (1 - 1e-6) theta_d,max) is valid in the kernel; the count equals the NaN rows"""
    cam, fx, K_new = _cam(name), T.FOLDING[name], _K_new(name)
    got = C().undistort_points(_grid(name), cam, K_new).cpu().numpy()
    nan = np.isnan(got[:, 0])
    assert np.array_equal(nan, np.isnan(got[:, 1])) and 0 < nan.sum() < len(nan)
    grid = T.pixel_grid(*fx[3])
    back = T.distort(fx, got[~nan], K_new)
    assert np.abs(back - grid[~nan]).max() <= 1e-6, np.abs(back - grid[~nan]).max()
    _, ok, margin = T.grid_normalised(name, "newton")
    sure = ok & (margin > (0.05 if fx[0] == "radtan" else 1e-6))
    print(name, "valid in the kernel:", (~nan).sum(), " in the oracle:", ok.sum(), " with margin:", sure.sum())
    assert sure.sum() > 0.3 * len(sure) and not nan[sure].any()
    m, count = C().rectify_map(cam, K_new, return_invalid=True)          # the fp32 map: the same pixels
    assert int(count) == int(nan.sum()) and np.array_equal(np.isnan(m.cpu().numpy().reshape(-1, 2)[:, 0]), nan)


# ------------------------------------------------------------------------------------------------ remap
H_IN, W_IN, H_OUT, W_OUT = 23, 37, 19, 41


def _images(B, C_, dtype, seed):
    g = np.random.default_rng(seed)
    if dtype == torch.uint8:
        return torch.from_numpy(g.integers(0, 256, (B, H_IN, W_IN, C_), dtype=np.uint8))
    return torch.from_numpy((g.standard_normal((B, H_IN, W_IN, C_)) * 100.0 + 100.0).astype(np.float32))


def _maps():
    oy, ox = np.meshgrid(np.arange(H_OUT), np.arange(W_OUT), indexing="ij")
    integer = np.stack([(ox * 3) % W_IN, (oy * 5) % H_IN], -1).astype(np.float32)
    ex = np.array([-1.0, -0.5, 0.0, W_IN - 1, W_IN - 0.5, W_IN, np.nan], dtype=np.float32)
    ey = np.array([-1.0, -0.5, 0.0, H_IN - 1, H_IN - 0.5, H_IN, np.nan], dtype=np.float32)
    edges = np.stack(np.meshgrid(ex, ey), -1)
    g = np.random.default_rng(11)
    rand = np.stack([g.uniform(-2.0, W_IN + 1.0, (H_OUT, W_OUT)), g.uniform(-2.0, H_IN + 1.0, (H_OUT, W_OUT))], -1).astype(np.float32)
    return {"integer": integer, "edges": edges, "random": rand}


def _check_remap(img, coords, out, what):
    real = T.remap(img.numpy(), coords)
    bound = 16 * 2.0 ** -24 * float(np.abs(img.numpy().astype(np.float64)).max())
    got = out.cpu().numpy()
    assert got.shape == real.shape, (what, got.shape)
    if out.dtype == torch.float32:
        err = np.abs(got - real).max()
        assert err <= bound, (what, err, bound)
        return
    assert out.dtype == torch.uint8
    want = T.to_uint8(real)
    near_tie = np.abs(real - np.floor(real) - 0.5) <= bound
    wrong = got != want
    assert not (wrong & ~near_tie).any(), (what, int((wrong & ~near_tie).sum()))
    assert (np.abs(got.astype(np.int64) - want.astype(np.int64))[wrong] <= 1).all(), what
    assert wrong.mean() <= 0.01, (what, wrong.mean())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_remap(C_, B, dtype):
    img = _images(B, C_, dtype, seed=C_ * 10 + B)
    dev = img.to(DEV)
    for key, coords in _maps().items():
        m = torch.from_numpy(coords).to(DEV)
        out = C().remap(dev, m)
        assert out.dtype == dtype and out.shape == (B,) + coords.shape[:2] + (C_,)
        _check_remap(img, coords, out, (key, C_, B, dtype))
        if key == "integer":                                            # output equals input exactly
            assert torch.equal(out.cpu(), img[:, coords[..., 1].astype(np.int64), coords[..., 0].astype(np.int64), :])
        if key == "random" and dtype == torch.uint8:                    # the fixture's own near-ties stay below the allowance
            real = T.remap(img.numpy(), coords)
            assert (np.abs(real - np.floor(real) - 0.5) <= 16 * 2.0 ** -24 * 255).mean() < 0.01
        if key == "edges":
            o = out.cpu().numpy().astype(np.float64)
            assert not o[:, [0, 5, 6], :, :].any() and not o[:, :, [0, 5, 6], :].any()        # -1, W and NaN: nothing
            assert np.array_equal(o[:, 2, 2], img[:, 0, 0].numpy()) and np.array_equal(o[:, 3, 3], img[:, -1, -1].numpy())
    other = torch.float32 if dtype == torch.uint8 else torch.uint8
    coords = _maps()["random"]
    m = torch.from_numpy(coords).to(DEV)
    _check_remap(img, coords, C().remap(dev, m, dtype=other), ("cross", C_, B, dtype))
    out = torch.empty((B, H_OUT, W_OUT, C_), dtype=dtype, device=DEV)
    assert C().remap(dev, m, out=out) is out and torch.equal(out, C().remap(dev, m))
    if B == 1:
        assert torch.equal(C().remap(dev[0], m), out[0])               # [H, W, C] in, [Ho, Wo, C] out


def test_remap_to_uint8_saturates_and_rounds_to_even():
    img = torch.tensor([-40.0, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 3.5]).view(1, 1, 8, 1).to(DEV)
    m = torch.stack([torch.arange(8.0), torch.zeros(8)], -1).view(1, 8, 2).to(DEV)
    assert C().remap(img, m, dtype=torch.uint8).flatten().tolist() == [0, 0, 2, 2, 254, 255, 255, 4]


def test_undistort_images_is_remap_of_the_map_and_keeps_the_map():
    """bit for bit remap(undistort_map(...)); the second call is ONE launch (the map is kept per camera, K_new, R, size, device)"""
    from torch.profiler import profile, ProfilerActivity
    cam = _cam("davis240")
    W, H = cam.size
    g = np.random.default_rng(5)
    frames = torch.from_numpy(g.integers(0, 256, (2, H, W, 3), dtype=np.uint8)).to(DEV)
    C().clear_cache()
    for kw in (dict(), dict(out_size=(120, 90)), dict(K_new=cam.K, R=T.rotation(2, 5.0))):
        out = C().undistort_images(frames, cam, **kw)
        want = C().remap(frames, C().undistort_map(cam, **kw))
        assert out.dtype == torch.uint8 and torch.equal(out, want) and out.shape == (2,) + tuple(reversed(kw.get("out_size", (W, H)))) + (3,)
    assert len(C()._maps) == 3
    real = T.remap(frames.cpu().numpy(), C().undistort_map(cam).cpu().numpy())
    inside = C().undistort_images(frames, cam).cpu().numpy()
    assert (np.abs(inside.astype(np.float64) - real) <= 0.5 + 1e-3).all() and inside.any()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        again = C().undistort_images(frames, cam)
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if "cuda" in str(getattr(ev, "device_type", "")).lower() and ("k_remap" in ev.name or "k_cam" in ev.name)]
    assert len(names) == 1 and "k_remap" in names[0], names
    assert torch.equal(again, C().remap(frames, C().undistort_map(cam))) and len(C()._maps) == 3
    with pytest.raises(ValueError, match="W, H"):
        C().undistort_images(frames[:, :-1], cam)


# ------------------------------------------------------------------------------------------------ acceptance: the map feeds the event front end
def _events(W, H, n, seed):
    g = torch.Generator().manual_seed(seed)
    xs, ys = torch.randint(0, W, (n,), generator=g), torch.randint(0, H, (n,), generator=g)
    xs[0], ys[0], xs[-1], ys[-1] = W // 2, H // 2, W // 2, H // 2        # (the window's first and last event, which fix its time axis, stay)
    ts = torch.sort(torch.randint(0, 50_000, (n,), generator=g)).values
    ts[0], ts[-1] = 0, 49_999
    ps = torch.randint(0, 2, (n,), generator=g)
    return xs.to(DEV), ys.to(DEV), ts.to(DEV), ps.to(DEV)


def test_the_map_goes_into_voxel_grids_and_invalid_pixels_drop_their_events():
    from devo_amd import events
    cam = _cam("davis240")
    W, H = cam.size
    xs, ys, ts, ps = _events(W, H, 20_000, 1)
    grids, counts = events.voxel_grids(xs, ys, ts, ps, [0.0], [50_000.0], H, W, bins=5, rectify_map=C().rectify_map(cam))
    assert grids.shape == (1, 5, H, W) and bool(torch.isfinite(grids).all()) and float(grids.abs().sum()) > 0 and int(counts[0]) == 20_000
    cam = _cam("fold_radtan")
    W, H = cam.size
    m = C().rectify_map(cam, cam.K)
    xs, ys, ts, ps = _events(W, H, 20_000, 2)
    keep = ~torch.isnan(m[ys, xs, 0])
    assert 0.2 < float(keep.float().mean()) < 0.5 and bool(keep[0]) and bool(keep[-1])
    a, _ = events.voxel_grids(xs, ys, ts, ps, [0.0], [50_000.0], H, W, bins=5, rectify_map=m)
    b, _ = events.voxel_grids(xs[keep], ys[keep], ts[keep], ps[keep], [0.0], [50_000.0], H, W, bins=5, rectify_map=m)
    assert bool(torch.isfinite(a).all()) and float(a.abs().sum()) > 0
    assert torch.allclose(a, b, rtol=0.0, atol=1e-4 * float(a.abs().max()))       # (atomic float sums: the order of the votes differs between the two streams)


# ------------------------------------------------------------------------------------------------ interface
_LEG = r"""
import sys, os, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import camera_ref as T
from devo_amd import camera as C
import devo_amd.backends as B
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
out = {}
for name in ("small37", "davis240", "equi346", "fold_radtan", "fold_equi"):
    cam = C.Camera(*T.FIXTURES[name])
    K_new = cam.K if name == "fold_radtan" else None
    fx, fy, cx, cy = K_new or C.new_camera_matrix(cam)
    m, n = C.rectify_map(cam, (fx, fy, cx + 0.37, cy + 0.21), return_invalid=True)
    out[name + "/map"], out[name + "/invalid"] = m, n
    out[name + "/source"] = C.undistort_map(cam, K_new, R=T.rotation(0, 5.0), out_size=(41, 19))
    p = torch.from_numpy(T.pixel_grid(*cam.size)).cuda()
    out[name + "/points"] = C.undistort_points(p, cam, R=T.rotation(1, 5.0))
    out[name + "/back"] = C.distort_points(p, cam, cam.K)
g = np.random.default_rng(3)
for C_ in (1, 3, 4):
    for dt in (np.uint8, np.float32):
        img = torch.from_numpy((g.uniform(0, 255, (2, 23, 37, C_))).astype(dt)).cuda()
        for o in (torch.uint8, torch.float32):
            out[f"remap/{C_}/{np.dtype(dt).name}/{o}"] = C.remap(img, out["small37/source"], dtype=o)
cam = C.Camera(*T.FIXTURES["small37"])
out["undistorted"] = C.undistort_images(torch.from_numpy(g.integers(0, 256, (3, 23, 37, 3), dtype=np.uint8)).cuda(), cam)
torch.cuda.synchronize()
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_both_bindings_return_the_same_bits(tmp_path):
    """the map and remap cases under DEVO_BINDING=ctypes and under the compiled binding: the same bits, and the restatement's values"""
    res = []
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res.append(torch.load(path))
    a, b = res
    assert a.keys() == b.keys() and len(a) == 5 * 5 + 12 + 1
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(_bits(a[k]) if a[k].is_floating_point() else a[k], _bits(b[k]) if b[k].is_floating_point() else b[k]), f"{k}: the two bindings disagree"
    for name in ("small37", "davis240", "equi346"):                     # either leg against the restatement (the other has the same bits)
        want = T.project(T.grid_normalised(name)[0], _K_off(name))
        got = b[name + "/map"].numpy().reshape(-1, 2).astype(np.float64)
        assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32))).all() and int(b[name + "/invalid"]) == 0
    assert int(b["fold_radtan/invalid"]) > 0 and int(b["fold_equi/invalid"]) > 0 and bool(b["undistorted"].any())


def test_cpu_tensors_raise():
    cam = _cam("davis240")
    for call in (lambda: C().undistort_points(torch.zeros(4, 2), cam), lambda: C().distort_points(torch.zeros(4, 2), cam, cam.K),
                 lambda: C().remap(torch.zeros(1, 4, 4, 1), torch.zeros(2, 2, 2, device=DEV)), lambda: C().remap(torch.zeros(1, 4, 4, 1, device=DEV), torch.zeros(2, 2, 2)),
                 lambda: C().undistort_images(torch.zeros(1, 180, 240, 3, dtype=torch.uint8), cam), lambda: C().rectify_map(cam, device="cpu")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(ValueError):
        C().remap(torch.zeros(1, 4, 4, 5, device=DEV), torch.zeros(2, 2, 2, device=DEV))       # five channels
    with pytest.raises(ValueError):
        C().remap(torch.zeros(1, 4, 4, 3, device=DEV, dtype=torch.float64), torch.zeros(2, 2, 2, device=DEV))
    with pytest.raises(ValueError):
        C().undistort_points(torch.zeros(4, 3, device=DEV), cam)
