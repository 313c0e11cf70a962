"""Branch-free fp64 reference for SE(3) exp / log and their left Jacobians (test infrastructure, CPU, plain torch).

oracle/se3.py restates the reference's closed forms, thresholds included, so it cancels where the kernels cancel.  This file has no
threshold and no closed-form coefficient: the 6x6 left Jacobian is the power series  J_l(a) = sum_{k>=0} ad(a)^k / (k+1)!  (60 terms:
for |phi| <= pi and |tau| of a few units the terms fall below 1e-30 long before that), its inverse is a numerical inverse, and the only
transcendental calls are sinc / cos / atan2, none of which cancels.  Layouts and the gradient convention are those of oracle/se3.py:
X = (t, qx, qy, qz, qw), a = (tau, phi), the gradient of a group element is a left-perturbation tangent in six of seven slots.
Every function takes [n, dim] tensors and computes in float64."""
import math
import torch

TERMS = 60

# devo_amd/csrc/se3_dev.h: Consts<T>::eps (so3_exp / so3_log) and Consts<T>::series_max (series below, closed forms above) per type.
# tests/test_se3_series_ref_cpu.py checks this list against the header; the sweep brackets every entry.
SWITCH_POINTS = {"eps": {"float": 1e-6, "double": 1e-6}, "series_max": {"float": 1.0, "double": 0.3}}
# 9e-7 / 1.1e-6 bracket eps and 0.99 / 1.01 the float series switch; 0.97x and 1.03x of each series switch are added explicitly
SWEEP_THETAS = [1e-7, 9e-7, 1.1e-6, 3e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-2, 0.1, 0.97 * 0.3, 0.3, 1.03 * 0.3, 0.5, 0.97 * 1.0, 0.99, 1.01, 1.03 * 1.0,
                2.0, 3.1, math.pi - 1e-3]


def _hat(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).view(*v.shape[:-1], 3, 3)


def ad(a):
    """[[hat(phi), hat(tau)], [0, hat(phi)]], tangent order (tau, phi)."""
    a = a.double()
    Tau, Phi = _hat(a[..., :3]), _hat(a[..., 3:])
    Z = torch.zeros_like(Phi)
    return torch.cat([torch.cat([Phi, Tau], -1), torch.cat([Z, Phi], -1)], -2)


def left_jacobian(a):
    A = ad(a)
    term = torch.eye(6, dtype=torch.float64).expand_as(A).clone()      # ad^k / (k+1)!
    J = term.clone()
    for k in range(1, TERMS):
        term = term @ A / (k + 1)
        J = J + term
    return J


def left_jacobian_inverse(a):
    return torch.linalg.inv(left_jacobian(a))


def _rot_only(phi):
    return torch.cat([torch.zeros_like(phi), phi], -1)


def exp_ref(a):
    a = a.double()
    tau, phi = a[..., :3], a[..., 3:]
    theta = phi.norm(dim=-1, keepdim=True)
    imag = 0.5 * torch.sinc(theta / (2 * math.pi))                      # sin(t/2)/t = sinc(t / 2pi) / 2, torch.sinc(x) = sin(pi x)/(pi x)
    q = torch.cat([imag * phi, torch.cos(0.5 * theta)], -1)
    t = (left_jacobian(a)[..., :3, :3] @ tau[..., None])[..., 0]
    return torch.cat([t, q], -1)


def _so3_log(q):
    q = q / q.norm(dim=-1, keepdim=True)
    q = torch.where(q[..., 3:] < 0, -q, q)
    v, w = q[..., :3], q[..., 3:]
    n = v.norm(dim=-1, keepdim=True)
    zero = n == 0
    ns = torch.where(zero, torch.ones_like(n), n)
    return torch.where(zero, 2 * v / w, 2 * torch.atan2(n, w) / ns * v)


def log_ref(X):
    X = X.double()
    phi = _so3_log(X[..., 3:7])
    V = left_jacobian(_rot_only(phi))[..., :3, :3]
    tau = torch.linalg.solve(V, X[..., :3, None])[..., 0]
    return torch.cat([tau, phi], -1)


def sweep_inputs(theta, dt, n=256, seed=0):
    """One rotation magnitude of the small-angle sweep: n random unit directions scaled to |phi| = theta, tau, g7, b ~ N(0,1); rounded to dt
    first, X = exp_ref of the rounded a, rounded to dt.  Every fourth quaternion negated (w < 0), every fifth scaled by 1.7."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    a = torch.cat([torch.randn(n, 3, generator=g, dtype=torch.float64), theta * u / u.norm(dim=-1, keepdim=True)], -1).to(dt)
    g7 = torch.randn(n, 7, generator=g, dtype=torch.float64).to(dt)
    b = torch.randn(n, 6, generator=g, dtype=torch.float64).to(dt)
    X = exp_ref(a)
    X[::4, 3:] *= -1.0
    X[::5, 3:] *= 1.7
    return a, X.to(dt), g7, b


def sweep_batch(thetas, dt, n=256):
    """sweep_inputs of every magnitude (seed = its index) in one batch: rows [i n, (i + 1) n) belong to thetas[i]."""
    parts = [sweep_inputs(th, dt, n, seed=i) for i, th in enumerate(thetas)]
    return [torch.cat(p) for p in zip(*parts)]


def _pad7(g6):
    return torch.cat([g6, torch.zeros_like(g6[..., :1])], -1)


def _rowmat(g, M):
    return (g[..., None, :] @ M)[..., 0, :]


def expm_backward(g7, a):
    return _rowmat(g7.double()[..., :6], left_jacobian(a))


def logm_backward(b, X):
    return _pad7(_rowmat(b.double()[..., :6], left_jacobian_inverse(log_ref(X))))


def jinv(X, b):
    return (left_jacobian_inverse(log_ref(X)) @ b.double()[..., None])[..., 0]
