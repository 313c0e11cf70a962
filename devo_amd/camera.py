"""Camera models on the GPU over csrc/camera.hip: what the reference obtains from OpenCV before anything reaches the network — the
rectification map of an event sensor (utils/load_utils.py `compute_rmap_ecd`, `compute_rmap_vector`; scripts/pp_*.py), the undistortion of
points, and the undistortion of RGB frames (devo/stream.py, evals/eval_rgb/eval_tum.py, scripts/e2v/undist_*.py).

Lens models: "pinhole" (no coefficients), "radtan" (OpenCV's k1 k2 p1 p2 [k3]) and "equidistant" (Kannala-Brandt / OpenCV fisheye, k1..k4).

  * `rectify_map(cam)` is the [H, W, 2] fp32 tensor `events.voxel_grids` / `events.real_data_voxels` take: for every raw sensor pixel its
    position in the ideal camera `K_new`.  The pixel grid is generated in the kernel; all arithmetic is fp64 (it runs once per scene and
    decides where every event votes).  A pixel whose inverse does not exist on the principal branch (beyond the fold of a strongly
    distorted radtan model; beyond the monotone range of an equidistant one) is NaN: its events vote nowhere.
  * `undistort_images(frames, cam)` is `cv2.undistort`: the source map is built once per (camera, K_new, R, size, device) and kept; each
    call after the first is ONE launch for all B frames (bilinear, constant zero border).
  * `new_camera_matrix(cam, alpha | balance)` restates `cv2.getOptimalNewCameraMatrix` / `cv2.fisheye.estimateNewCameraMatrixForUndistortRectify`
    on the host in fp64 (81 or 4 points): `K_new=None` means this matrix for `rectify_map`, `undistort_map` and `undistort_images`, which
    is what the reference's loaders do.

Intrinsics are (fx, fy, cx, cy).  R is a 3 x 3 rectifying rotation (ideal = R · raw ray).  No CPU fallback: CPU tensors raise.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from . import backends

MODELS = {"pinhole": 0, "radtan": 1, "equidistant": 2}             # DEVO_CAM_*
_COUNTS = {"pinhole": (0,), "radtan": (4, 5), "equidistant": (4,)}


def _floats(v, n, what):
    try:
        out = tuple(float(x) for x in (v.tolist() if hasattr(v, "tolist") else v))
    except TypeError:
        raise TypeError(f"{what} must be a sequence of numbers")
    if n is not None and len(out) not in n:
        raise ValueError(f"{what} must have {' or '.join(str(c) for c in n)} entries, got {len(out)}")
    if not all(math.isfinite(x) for x in out):
        raise ValueError(f"{what} has a non-finite entry")
    return out


@dataclass(frozen=True)
class Camera:
    """model "pinhole" | "radtan" | "equidistant"; K = (fx, fy, cx, cy); dist = the model's coefficients; size = (W, H) of the sensor."""
    model: str
    K: tuple
    dist: tuple = ()
    size: tuple = (0, 0)

    def __post_init__(self):
        if self.model not in MODELS:
            raise ValueError(f"Camera: model {self.model!r} (have: {', '.join(MODELS)})")
        object.__setattr__(self, "K", _floats(self.K, (4,), "Camera: K"))
        object.__setattr__(self, "dist", _floats(self.dist, _COUNTS[self.model], f"Camera: dist of a {self.model} model"))
        if not (self.K[0] > 0.0 and self.K[1] > 0.0):
            raise ValueError("Camera: focal lengths must be positive")
        size = tuple(self.size)
        if len(size) != 2 or any(int(s) != s or s < 1 or s >= 1 << 24 for s in size):
            raise ValueError(f"Camera: size must be (W, H) in pixels, got {self.size!r}")
        object.__setattr__(self, "size", (int(size[0]), int(size[1])))


# ------------------------------------------------------------------------------------------------ host arithmetic (new_camera_matrix)
def _equidistant_limit(k):
    """(theta_lim, theta_d,max): the smallest positive root of d theta_d / d theta in (0, pi / 2], or pi / 2, and theta_d there"""
    k1, k2, k3, k4 = k
    roots = np.roots([9.0 * k4, 7.0 * k3, 5.0 * k2, 3.0 * k1, 1.0])    # in u = theta^2
    u = [r.real for r in np.atleast_1d(roots) if abs(r.imag) <= 1e-12 * max(1.0, abs(r)) and 0.0 < r.real <= (math.pi / 2) ** 2]
    t = math.sqrt(min(u)) if u else math.pi / 2
    t2 = t * t
    return t, t * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))


def _undistort_normalised_host(cam, px):
    """raw pixels [n, 2] -> normalised ideal coordinates [n, 2], fp64, by the kernel's rules; NaN where invalid"""
    px = np.asarray(px, dtype=np.float64)
    fx, fy, cx, cy = cam.K
    xd, yd = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    if cam.model == "pinhole":
        return np.stack([xd, yd], 1)
    if cam.model == "radtan":
        k1, k2, p1, p2 = cam.dist[:4]
        k3 = cam.dist[4] if len(cam.dist) == 5 else 0.0
        x, y = xd.copy(), yd.copy()
        ok, done = np.ones(len(x), bool), np.zeros(len(x), bool)
        for _ in range(30):
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            D = k1 + r2 * (2.0 * k2 + r2 * 3.0 * k3)
            ex = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - xd
            ey = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - yd
            a = rad + 2.0 * x * x * D + 2.0 * p1 * y + 6.0 * p2 * x
            b = 2.0 * x * y * D + 2.0 * p1 * x + 2.0 * p2 * y
            d = rad + 2.0 * y * y * D + 6.0 * p1 * y + 2.0 * p2 * x
            det = a * d - b * b
            ok &= done | (det > 0.0)
            live = ok & ~done
            safe = np.where(det > 0.0, det, 1.0)
            dx, dy = (d * ex - b * ey) / safe, (a * ey - b * ex) / safe
            x, y = np.where(live, x - dx, x), np.where(live, y - dy, y)
            done |= live & (np.abs(dx) + np.abs(dy) < 1e-12)
            if not (ok & ~done).any():
                break
        ok &= done
        return np.stack([np.where(ok, x, np.nan), np.where(ok, y, np.nan)], 1)
    k1, k2, k3, k4 = cam.dist
    t_lim, td_max = _equidistant_limit(cam.dist)
    td = np.hypot(xd, yd)
    lo, hi = np.zeros_like(td), np.full_like(td, t_lim)
    for _ in range(64):                                                # (four points: bisection is enough here)
        mid = 0.5 * (lo + hi)
        m2 = mid * mid
        below = mid * (1.0 + m2 * (k1 + m2 * (k2 + m2 * (k3 + m2 * k4)))) < td
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    theta = 0.5 * (lo + hi)
    s = np.where(td > 0.0, np.tan(theta) / np.where(td > 0.0, td, 1.0), 1.0)
    s = np.where(td < td_max, s, np.nan)
    return np.stack([xd * s, yd * s], 1)


def new_camera_matrix(cam, alpha=0.0, balance=None, new_size=None):
    """-> (fx, fy, cx, cy) of the ideal camera; host arithmetic in fp64, no GPU.
    radtan / pinhole (cv2.getOptimalNewCameraMatrix): a 9 x 9 grid of raw pixels is undistorted; alpha = 0 fits the inner rectangle (every
    output pixel has a source), alpha = 1 the bounding box of all of them (every raw pixel is kept), values between blend the two matrices.
    equidistant (cv2.fisheye.estimateNewCameraMatrixForUndistortRectify): the four edge midpoints are undistorted; balance = 0 (the default)
    takes the largest of the four focal lengths they allow, balance = 1 the smallest.  new_size = (W', H') of the output, default the sensor's."""
    W, H = cam.size
    Wn, Hn = (W, H) if new_size is None else (int(new_size[0]), int(new_size[1]))
    if Wn < 1 or Hn < 1:
        raise ValueError(f"new_camera_matrix: new_size {new_size!r}")
    if cam.model == "equidistant":
        balance = 0.0 if balance is None else float(balance)
        if not 0.0 <= balance <= 1.0:
            raise ValueError("new_camera_matrix: balance must lie in [0, 1]")
        p = _undistort_normalised_host(cam, [(W / 2, 0.0), (W, H / 2), (W / 2, H), (0.0, H / 2)])
        if not np.isfinite(p).all():
            raise ValueError("new_camera_matrix: an edge midpoint of the sensor lies beyond the model's monotone range")
        a = cam.K[0] / cam.K[1]
        p[:, 1] *= a
        c = p.mean(0)
        f1, f2 = (W / 2) / (c[0] - p[:, 0].min()), (W / 2) / (p[:, 0].max() - c[0])
        f3, f4 = (H / 2) * a / (c[1] - p[:, 1].min()), (H / 2) * a / (p[:, 1].max() - c[1])
        f = balance * min(f1, f2, f3, f4) + (1.0 - balance) * max(f1, f2, f3, f4)
        cx, cy = -c[0] * f + W / 2, -c[1] * f + H * a / 2
        fx, fy, cy = f, f / a, cy / a
        sx, sy = Wn / W, Hn / H
        return (float(fx * sx), float(fy * sy), float(cx * sx), float(cy * sy))
    if balance is not None:
        raise ValueError("new_camera_matrix: balance belongs to the equidistant model; radtan and pinhole take alpha")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("new_camera_matrix: alpha must lie in [0, 1]")
    j, i = np.meshgrid(np.arange(9), np.arange(9))
    p = _undistort_normalised_host(cam, np.stack([j.ravel() * (W - 1) / 8, i.ravel() * (H - 1) / 8], 1)).reshape(9, 9, 2)
    if not np.isfinite(p).all():
        raise ValueError("new_camera_matrix: a pixel of the 9 x 9 sample lies beyond the fold of the distortion model")

    def fit(x0, x1, y0, y1):
        fx, fy = (Wn - 1) / (x1 - x0), (Hn - 1) / (y1 - y0)
        return np.array([fx, fy, -fx * x0, -fy * y0])
    inner = fit(p[:, 0, 0].max(), p[:, 8, 0].min(), p[0, :, 1].max(), p[8, :, 1].min())
    outer = fit(p[..., 0].min(), p[..., 0].max(), p[..., 1].min(), p[..., 1].max())
    return tuple(float(v) for v in (1.0 - alpha) * inner + alpha * outer)


# ------------------------------------------------------------------------------------------------ the three entry points
def _arr(v):
    return (ctypes.c_double * len(v))(*v) if v else None


def _rotation(R):
    if R is None:
        return ()
    R = _floats(np.asarray(R.detach().cpu() if torch.is_tensor(R) else R, dtype=np.float64).reshape(-1), (9,), "R")
    return R


def _points_call(points, n, H, W, device, cam, K_new, R, distort, out_f64, count):
    """one launch of devo_camera_undistort_points / devo_camera_distort_points -> (out, invalid i32 [1] or None)"""
    if not isinstance(cam, Camera):
        raise TypeError("a devo_amd.camera.Camera is expected")
    K_new = () if K_new is None else _floats(K_new, (4,), "K_new")
    R = _rotation(R)
    nat = backends.native()
    if nat is not None:
        out, invalid = nat.camera.points(points, H, W, device.index if device.index is not None else torch.cuda.current_device(), MODELS[cam.model], list(cam.K),
                                         list(cam.dist), list(R), list(K_new), bool(distort), bool(out_f64), bool(count))
        return out, (invalid if count else None)
    with torch.cuda.device(device):
        dt = torch.float64 if out_f64 else torch.float32
        out = torch.empty((H, W, 2) if points is None else (n, 2), dtype=dt, device=device)
        invalid = torch.zeros(1, dtype=torch.int32, device=device) if count else None
        fn = L.lib().devo_camera_distort_points if distort else L.lib().devo_camera_undistort_points
        rc = fn(L.ptr(points), n, H, W, L.DEVO_F64 if points is None else L.dtype_code(points), MODELS[cam.model], _arr(cam.K), _arr(cam.dist), len(cam.dist), _arr(R),
                _arr(K_new), L.ptr(out), L.DEVO_F64 if out_f64 else L.DEVO_F32, L.ptr(invalid), L.stream())
        L.check(rc, "camera.distort_points" if distort else "camera.undistort_points")
    return out, invalid


def _device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _given_points(points, cam, K_new, R, distort, what):
    if not torch.is_tensor(points):
        raise TypeError(f"{what}: points must be a tensor")
    L.require_gpu(points)
    if points.dim() < 1 or points.shape[-1] != 2 or points.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: points must be float32 or float64 [..., 2]")
    flat = points.reshape(-1, 2).contiguous()
    out, _ = _points_call(flat, flat.shape[0], 0, 0, points.device, cam, K_new, R, distort, points.dtype == torch.float64, False)
    return out.view(points.shape)


def rectify_map(cam, K_new=None, R=None, device="cuda", return_invalid=False):
    """[H, W, 2] fp32: map[y, x] = the ideal pixel (in K_new, default new_camera_matrix(cam)) of raw pixel (x, y); NaN where the pixel has
    no inverse.  One launch, nothing uploaded.  return_invalid=True -> (map, int32 [1] on the device: the number of NaN pixels)."""
    W, H = cam.size
    K_new = new_camera_matrix(cam) if K_new is None else K_new
    out, invalid = _points_call(None, H * W, H, W, _device(device), cam, K_new, R, False, False, return_invalid)
    return (out, invalid) if return_invalid else out


def undistort_points(points, cam, K_new=None, R=None):
    """raw pixels [..., 2] (fp32 or fp64 on the GPU; dtype kept, arithmetic fp64) -> ideal pixels in K_new, or normalised coordinates when
    K_new is None (cv2.undistortPoints).  Invalid points are NaN."""
    return _given_points(points, cam, K_new, R, False, "undistort_points")


def distort_points(points, cam, K_new, R=None):
    """ideal pixels [..., 2] in K_new -> raw pixels (the closed-form forward model).  NaN behind the camera and beyond an equidistant
    model's monotone range."""
    if K_new is None:
        raise ValueError("distort_points: K_new is required (the camera the points are pixels of)")
    return _given_points(points, cam, K_new, R, True, "distort_points")


def _out_size(cam, out_size):
    if out_size is None:
        return cam.size
    Wo, Ho = int(out_size[0]), int(out_size[1])
    if Wo < 1 or Ho < 1:
        raise ValueError(f"out_size must be (W, H), got {out_size!r}")
    return Wo, Ho


def undistort_map(cam, K_new=None, R=None, out_size=None, device="cuda"):
    """[Ho, Wo, 2] fp32: for every pixel of the undistorted image (camera K_new, size out_size = (Wo, Ho), default the sensor's) the raw
    image's source coordinates (cv2.initUndistortRectifyMap).  K_new=None: new_camera_matrix(cam, new_size=out_size)."""
    Wo, Ho = _out_size(cam, out_size)
    K_new = new_camera_matrix(cam, new_size=(Wo, Ho)) if K_new is None else K_new
    return _points_call(None, Ho * Wo, Ho, Wo, _device(device), cam, K_new, R, True, False, False)[0]


_TORCH_IMG = {torch.uint8: L.DEVO_U8, torch.float32: L.DEVO_F32}


def remap(images, map, out=None, dtype=None):
    """images [B, H, W, C] or [H, W, C] channels-last (uint8 or float32, C in 1..4), map float32 [Ho, Wo, 2] of source coordinates (x, y)
    -> [B, Ho, Wo, C] (or [Ho, Wo, C]) of `dtype` (default: the images').  Bilinear; outside the image is 0 (cv2.remap with
    BORDER_CONSTANT); uint8 output rounds to nearest even and saturates.  One launch."""
    if not torch.is_tensor(images) or not torch.is_tensor(map):
        raise TypeError("remap: images and map must be tensors")
    L.require_gpu(images, map, out)
    single = images.dim() == 3
    if single:
        images = images.unsqueeze(0)
    if images.dim() != 4 or not 1 <= images.shape[3] <= 4 or images.dtype not in _TORCH_IMG or images.numel() == 0:
        raise ValueError("remap: images must be uint8 or float32 [B, H, W, C] (or [H, W, C]) with 1 to 4 channels")
    if map.dim() != 3 or map.shape[2] != 2 or map.dtype != torch.float32 or map.numel() == 0 or map.device != images.device:
        raise ValueError("remap: map must be float32 [Ho, Wo, 2] on the images' GPU")
    dtype = (out.dtype if out is not None else images.dtype) if dtype is None else dtype
    if dtype not in _TORCH_IMG:
        raise ValueError(f"remap: output dtype {dtype} (have: uint8, float32)")
    B, H, W, C = images.shape
    Ho, Wo = map.shape[:2]
    images, map = images.contiguous(), map.contiguous()
    if out is not None:
        full = out.unsqueeze(0) if (single and out.dim() == 3) else out
        if tuple(full.shape) != (B, Ho, Wo, C) or out.dtype != dtype or out.device != images.device or not out.is_contiguous():
            raise ValueError(f"remap: out must be a contiguous {dtype} tensor of shape {(B, Ho, Wo, C)} on the images' GPU")
    else:
        full = None
    nat = backends.native()
    if nat is not None:
        full = nat.camera.remap(images, map, full, dtype == torch.uint8)
    else:
        with torch.cuda.device(images.device):
            if full is None:
                full = torch.empty((B, Ho, Wo, C), dtype=dtype, device=images.device)
            rc = L.lib().devo_image_remap(L.ptr(images), B, H, W, C, _TORCH_IMG[images.dtype], L.ptr(map), Ho, Wo, L.ptr(full), _TORCH_IMG[dtype], L.stream())
            L.check(rc, "camera.remap")
    if out is not None:
        return out
    return full[0] if single else full


_maps = {}                                                            # (cam, K_new, R, out_size, device) -> source map


def undistort_images(images, cam, K_new=None, R=None, out_size=None):
    """cv2.undistort on the GPU: images [B, H, W, C] or [H, W, C] taken with `cam` -> the same frames in the ideal camera K_new (default
    new_camera_matrix(cam, new_size=out_size)).  The source map is built on the first call per (cam, K_new, R, out_size, device) and kept:
    every later call is one launch."""
    if not torch.is_tensor(images):
        raise TypeError("undistort_images: images must be a tensor")
    L.require_gpu(images)
    if images.dim() not in (3, 4) or (images.shape[-2], images.shape[-3]) != cam.size:
        raise ValueError(f"undistort_images: images must be [B, H, W, C] or [H, W, C] with (W, H) = {cam.size}, got {tuple(images.shape)}")
    key = (cam, None if K_new is None else _floats(K_new, (4,), "K_new"), _rotation(R), _out_size(cam, out_size), images.device)
    m = _maps.get(key)
    if m is None:
        m = _maps[key] = undistort_map(cam, key[1], R, key[3], images.device)
    return remap(images, m)


def clear_cache():
    """drop the source maps undistort_images keeps"""
    _maps.clear()
