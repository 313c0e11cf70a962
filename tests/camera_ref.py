"""numpy fp64 restatement of devo_amd.camera (csrc/camera.hip): the lens models (pinhole, radtan, equidistant) forward and inverse, the two
new-camera-matrix rules and a bilinear remap.  Checked by itself in test_camera_cpu.py; test_gpu_camera.py holds the kernels to it.

Every inverse exists in TWO formulations:
  * `method="independent"` (what the GPU tests compare with): radtan by OpenCV's fixed-point iteration x <- (x_d - tangential(x)) / radial(x)
    run to convergence; equidistant by plain bisection on [0, theta_lim].
  * `method="newton"`: the kernel's rule restated — radtan by Newton on the two-dimensional forward model with its analytic Jacobian from
    x = x_d (at most 30 iterations, |dx| + |dy| < 1e-12, valid iff converged with det J > 0 at every iterate; min det J is returned);
    equidistant by Newton inside a bisection bracket.

PX_TOL, the GPU tolerance for fp64 point outputs, is GPU_FACTOR = 16 times the largest disagreement of the two formulations in pixels of
K_new = new_camera_matrix(cam), over every pixel of the MILD fixtures and the rotations the GPU test uses (none, 5 degrees about x, y, z):
`python tests/camera_ref.py` prints the figures.  Measured when this file was written:
    davis240 1.1e-13  radtan640 3.4e-13  pincushion 1.7e-13  equi1280 9.1e-13  equi346 5.9e-12   (px, the largest over the four rotations)
The last fixture reaches theta = 81.6 degrees (86.6 after a rotation), where d tan / d theta = 1 / cos^2 theta amplifies the last bit of theta by
285: its figure is the largest and is the one that counts.
"""
import functools

import numpy as np

GPU_FACTOR = 16
MEASURED_DISAGREEMENT_PX = 5.9e-12
PX_TOL = GPU_FACTOR * MEASURED_DISAGREEMENT_PX

# name -> (model, K, dist, (W, H))
MILD = {
    "small37": ("radtan", (30.0, 29.0, 18.3, 11.2), (-0.3684, 0.1510, -0.0003, -0.0002), (37, 23)),     # a partial workgroup, an odd row length, four coefficients
    "davis240": ("radtan", (199.09, 198.83, 132.19, 110.71), (-0.3684, 0.1510, -0.0003, -0.0002, 0.0), (240, 180)),
    "radtan640": ("radtan", (327.3, 327.5, 304.6, 230.0), (-0.031, 0.024, -0.0003, 0.0007, -0.010), (640, 480)),
    "pincushion": ("radtan", (250.0, 250.0, 170.0, 130.0), (0.12, -0.05, 0.001, -0.001, 0.01), (346, 260)),
    "equi1280": ("equidistant", (1049.6, 1049.3, 634.6, 263.5), (-0.0231, -0.0058, 0.0030, -0.0009), (1280, 720)),
    "equi346": ("equidistant", (172.98, 172.98, 163.33, 134.99), (-0.0275, -0.0065, 0.0008, -0.0003), (346, 260)),
}
FOLDING = {
    "fold_radtan": ("radtan", (180.0, 180.0, 173.0, 130.0), (-0.5, 0.0, 0.0, 0.0, 0.0), (346, 260)),
    "fold_equi": ("equidistant", (120.0, 121.0, 170.0, 128.0), (0.05, -0.02, 0.01, -0.004), (346, 260)),
}
FIXTURES = {**MILD, **FOLDING}


def rotation(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


ROTATIONS = {"none": None, "rx": rotation(0, 5.0), "ry": rotation(1, 5.0), "rz": rotation(2, 5.0)}


def pixel_grid(W, H):
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([x.ravel(), y.ravel()], 1)


# ------------------------------------------------------------------------------------------------ forward models (normalised coordinates)
def _radtan_terms(dist, x, y):
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    tx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    ty = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return radial, tx, ty


def equi_theta_d(k, theta):
    t2 = theta * theta
    return theta * (1.0 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4)


def equi_dtheta_d(k, theta):
    t2 = theta * theta
    return 1.0 + 3.0 * k[0] * t2 + 5.0 * k[1] * t2 ** 2 + 7.0 * k[2] * t2 ** 3 + 9.0 * k[3] * t2 ** 4


def equidistant_limit(k):
    """(theta_lim, theta_d,max): the first sign change of the derivative on a scan of (0, pi / 2], refined by bisection; pi / 2 if none"""
    ts = np.linspace(0.0, np.pi / 2, 20001)[1:]
    neg = np.nonzero(equi_dtheta_d(k, ts) <= 0.0)[0]
    if len(neg) == 0:
        t = np.pi / 2
    else:
        hi = ts[neg[0]]
        lo = ts[neg[0] - 1] if neg[0] > 0 else 0.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if equi_dtheta_d(k, mid) > 0.0:
                lo = mid
            else:
                hi = mid
        t = lo
    return t, equi_theta_d(k, t)


def distort_normalised(model, dist, x, y):
    """ideal normalised -> distorted normalised; for equidistant the third value is theta"""
    if model == "pinhole":
        return x, y, None
    if model == "radtan":
        radial, tx, ty = _radtan_terms(dist, x, y)
        return x * radial + tx, y * radial + ty, None
    r = np.hypot(x, y)
    theta = np.arctan(r)
    s = np.where(r > 0.0, equi_theta_d(dist, theta) / np.where(r > 0.0, r, 1.0), 1.0)
    return x * s, y * s, theta


# ------------------------------------------------------------------------------------------------ inverses
def radtan_newton(dist, xd, yd):
    """the kernel's rule -> (x, y, valid, min det J over the iterates)"""
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    x, y = xd.copy(), yd.copy()
    ok, done = np.ones(x.shape, bool), np.zeros(x.shape, bool)
    min_det = np.full(x.shape, np.inf)
    for _ in range(30):
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        D = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r2 ** 2
        fx = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - xd
        fy = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - yd
        a = radial + 2.0 * x * x * D + 2.0 * p1 * y + 6.0 * p2 * x
        b = 2.0 * x * y * D + 2.0 * p1 * x + 2.0 * p2 * y
        d = radial + 2.0 * y * y * D + 6.0 * p1 * y + 2.0 * p2 * x
        det = a * d - b * b
        live = ok & ~done
        min_det = np.where(live, np.minimum(min_det, det), min_det)
        ok &= ~live | (det > 0.0)
        live &= ok
        sdet = np.where(det > 0.0, det, 1.0)
        dx, dy = (d * fx - b * fy) / sdet, (a * fy - b * fx) / sdet
        x, y = np.where(live, x - dx, x), np.where(live, y - dy, y)
        done |= live & (np.abs(dx) + np.abs(dy) < 1e-12)
        if not (ok & ~done).any():
            break
    ok &= done
    return x, y, ok, min_det


def radtan_fixed_point(dist, xd, yd, iterations=500):
    """OpenCV's undistortPoints iteration, run until no point moves by more than rounding (or the count ends) -> (x, y, converged)"""
    x, y = xd.copy(), yd.copy()
    moved = np.full(x.shape, np.inf)
    for _ in range(iterations):
        radial, tx, ty = _radtan_terms(dist, x, y)
        xn, yn = (xd - tx) / radial, (yd - ty) / radial
        moved = np.abs(xn - x) + np.abs(yn - y)
        x, y = xn, yn
        if not (moved > 1e-15).any():
            break
    return x, y, moved < 1e-13


def equi_bisect(k, theta_d, theta_lim):
    lo, hi = np.zeros_like(theta_d), np.full_like(theta_d, theta_lim)
    for _ in range(120):
        mid = 0.5 * (lo + hi)
        below = equi_theta_d(k, mid) < theta_d
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def equi_newton(k, theta_d, theta_lim):
    lo, hi = np.zeros_like(theta_d), np.full_like(theta_d, theta_lim)
    t = np.minimum(theta_d, theta_lim)
    for _ in range(64):
        f = equi_theta_d(k, t) - theta_d
        hi, lo = np.where(f > 0.0, t, hi), np.where(f > 0.0, lo, t)
        tn = t - f / equi_dtheta_d(k, t)
        tn = np.where((tn > lo) & (tn < hi), tn, 0.5 * (lo + hi))
        tn = np.where(f == 0.0, t, tn)
        if not (np.abs(tn - t) > 2.3e-16 * np.abs(tn)).any():
            t = tn
            break
        t = tn
    return t


def undistort_normalised(model, K, dist, px, method="independent"):
    """raw pixels [n, 2] -> (normalised ideal [n, 2] with NaN rows where invalid, valid [n], margin [n]); margin is min det J (radtan) or
    1 - theta_d / theta_d,max (equidistant), +inf for pinhole"""
    px = np.asarray(px, dtype=np.float64)
    fx, fy, cx, cy = K
    xd, yd = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    if model == "pinhole":
        x, y, ok, margin = xd, yd, np.ones(len(xd), bool), np.full(len(xd), np.inf)
    elif model == "radtan":
        x, y, ok, margin = radtan_newton(dist, xd, yd)
        if method == "independent":
            x, y, conv = radtan_fixed_point(dist, xd, yd)
            ok = ok & conv
    else:
        t_lim, td_max = equidistant_limit(dist)
        td = np.hypot(xd, yd)
        ok = td < td_max
        tdc = np.where(ok, td, 0.0)
        theta = equi_bisect(dist, tdc, t_lim) if method == "independent" else equi_newton(dist, tdc, t_lim)
        s = np.where(td > 0.0, np.tan(theta) / np.where(td > 0.0, td, 1.0), 1.0)
        x, y, margin = xd * s, yd * s, 1.0 - td / td_max
    out = np.stack([np.where(ok, x, np.nan), np.where(ok, y, np.nan)], 1)
    return out, ok, margin


def project(p, K_new=None, R=None):
    """normalised ideal coordinates -> rotated, in pixels of K_new (or still normalised)"""
    if R is not None:
        v = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(R, dtype=np.float64).T
        p = v[:, :2] / v[:, 2:]
    if K_new is not None:
        p = p * np.array(K_new[:2]) + np.array(K_new[2:])
    return p


def undistort(fixture, px, K_new=None, R=None, method="independent"):
    """raw pixels -> (ideal pixels in K_new, or normalised coordinates; valid; margin)"""
    model, K, dist, _ = fixture
    p, ok, margin = undistort_normalised(model, K, dist, px, method)
    return project(p, K_new, R), ok, margin


@functools.lru_cache(maxsize=None)
def grid_normalised(name, method="independent"):
    """undistort_normalised on every pixel of a fixture, computed once (treat the arrays as read-only)"""
    model, K, dist, size = FIXTURES[name]
    out = undistort_normalised(model, K, dist, pixel_grid(*size), method)
    for a in out:
        a.setflags(write=False)
    return out


def distort(fixture, px, K_new, R=None):
    """ideal pixels in K_new -> raw pixels; NaN behind the camera and beyond the equidistant limit"""
    model, K, dist, _ = fixture
    px = np.asarray(px, dtype=np.float64)
    v = np.stack([(px[:, 0] - K_new[2]) / K_new[0], (px[:, 1] - K_new[3]) / K_new[1], np.ones(len(px))], 1)
    if R is not None:
        v = v @ np.asarray(R, dtype=np.float64)                       # rows times R = R^T v
    ok = v[:, 2] > 0.0
    z = np.where(ok, v[:, 2], 1.0)
    xd, yd, theta = distort_normalised(model, dist, v[:, 0] / z, v[:, 1] / z)
    if model == "equidistant":
        ok = ok & (theta <= equidistant_limit(dist)[0])
    return np.stack([np.where(ok, K[0] * xd + K[2], np.nan), np.where(ok, K[1] * yd + K[3], np.nan)], 1)


# ------------------------------------------------------------------------------------------------ the two matrix rules
def new_camera_matrix(fixture, alpha=0.0, balance=0.0, new_size=None):
    model, K, dist, (W, H) = fixture
    Wn, Hn = (W, H) if new_size is None else new_size
    if model == "equidistant":
        mid = np.array([[W / 2, 0.0], [W, H / 2], [W / 2, H], [0.0, H / 2]])
        p = undistort_normalised(model, K, dist, mid)[0]
        a = K[0] / K[1]
        p = p * np.array([1.0, a])
        c = p.mean(0)
        fs = [(W / 2) / (c[0] - p[:, 0].min()), (W / 2) / (p[:, 0].max() - c[0]), (H / 2) * a / (c[1] - p[:, 1].min()), (H / 2) * a / (p[:, 1].max() - c[1])]
        f = balance * min(fs) + (1.0 - balance) * max(fs)
        centre = -c * f + np.array([W, H * a]) / 2
        return (f * Wn / W, f / a * Hn / H, centre[0] * Wn / W, centre[1] / a * Hn / H)
    grid = np.array([[j * (W - 1) / 8, i * (H - 1) / 8] for i in range(9) for j in range(9)])
    p = undistort_normalised(model, K, dist, grid)[0].reshape(9, 9, 2)            # [row i, column j]

    def matrix(x0, x1, y0, y1):
        fx, fy = (Wn - 1) / (x1 - x0), (Hn - 1) / (y1 - y0)
        return np.array([fx, fy, -fx * x0, -fy * y0])
    inner = matrix(p[:, 0, 0].max(), p[:, -1, 0].min(), p[0, :, 1].max(), p[-1, :, 1].min())
    outer = matrix(p[:, :, 0].min(), p[:, :, 0].max(), p[:, :, 1].min(), p[:, :, 1].max())
    return tuple((1.0 - alpha) * inner + alpha * outer)


# ------------------------------------------------------------------------------------------------ remap
def remap(images, coords):
    """images [B, H, W, C] (any real dtype), coords fp32 [Ho, Wo, 2] -> the real bilinear value fp64 [B, Ho, Wo, C]: weights from the fp32
    coordinates (x - floor x is exact in fp32), a tap outside the image contributes 0, a non-finite coordinate gives 0"""
    img = np.asarray(images, dtype=np.float64)
    B, H, W, C = img.shape
    c = np.asarray(coords)
    assert c.dtype == np.float32
    x, y = c[..., 0].astype(np.float64), c[..., 1].astype(np.float64)
    fin = np.isfinite(x) & np.isfinite(y)
    x, y = np.where(fin, x, -5.0), np.where(fin, y, -5.0)
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = x - x0, y - y0
    out = np.zeros((B,) + x.shape + (C,))
    for dy, dx, w in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H) & fin
        tap = img[:, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1), :]
        out += np.where(ok, w, 0.0)[None, ..., None] * tap
    return out


def to_uint8(real):
    return np.clip(np.rint(real), 0, 255).astype(np.uint8)           # rint: to nearest even


def measure_disagreement():
    """name -> the largest |independent - newton| in pixels of K_new over every pixel and the four rotations"""
    out = {}
    for name, fx in MILD.items():
        K_new = new_camera_matrix(fx)
        (a, ok_a, _), (b, ok_b, _) = grid_normalised(name, "independent"), grid_normalised(name, "newton")
        assert ok_a.all() and ok_b.all(), name
        worst = 0.0
        for R in ROTATIONS.values():
            worst = max(worst, float(np.abs(project(a, K_new, R) - project(b, K_new, R)).max()))
        out[name] = worst
    return out


if __name__ == "__main__":
    for k, v in measure_disagreement().items():
        print(f"{k:12s} {v:.3e} px")
