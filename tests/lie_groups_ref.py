"""Branch-free fp64 reference for the four lietorch groups (test infrastructure, CPU, plain torch).

    group  id  element (N)           tangent (K)
    SO3    1   q_xyzw           (4)  phi              (3)
    RxSO3  2   q_xyzw, s        (5)  phi, sigma       (4)
    SE3    3   t, q_xyzw        (7)  tau, phi         (6)
    Sim3   4   t, q_xyzw, s     (8)  tau, phi, sigma  (7)

Nothing here restates a closed form of devo_amd/csrc/lie_dev.h.  Every group is handled as a sub-group of Sim3 through its 4x4 matrix
[[s R, t], [0, 1]] and the definitions:  hat / vee of the 4x4 algebra,  exp = sum hat^k / k!,  W = sum (Phi + sigma I)^k / (k+1)!,
ad(a) b = vee([hat a, hat b]),  J_l = sum ad^k / (k+1)!  (90 terms: no branch, and no cancellation for theta <= pi, |sigma| <= 1,
|tau| <= 3, where 60 and 120 terms give the same bits),  J_l^-1 = numpy-style inverse of that,  Adj(X) a = vee(X hat(a) X^-1), the
actions as matrix-vector products, the projector as d(embedded coordinates) / d(left perturbation), and the backward ops as the
vector-Jacobian products of those.  The only transcendental calls are sinc / cos / atan2 / exp / log, none of which cancels.
tests/test_lie_groups_ref_cpu.py checks the pieces against torch.linalg.matrix_exp, conjugation and finite differences.
Every function takes [n, dim] tensors and computes in float64; gradients of group elements are K-vectors in the first K of N slots."""
import math
import torch

TERMS = 90
NAMES = {1: "SO3", 2: "RxSO3", 3: "SE3", 4: "Sim3"}
# where a group's tangent / element coordinates sit among Sim3's (tau 0-2, phi 3-5, sigma 6 / t 0-2, q 3-6, s 7)
TAN_IDX = {1: [3, 4, 5], 2: [3, 4, 5, 6], 3: [0, 1, 2, 3, 4, 5], 4: [0, 1, 2, 3, 4, 5, 6]}
ELEM_IDX = {1: [3, 4, 5, 6], 2: [3, 4, 5, 6, 7], 3: [0, 1, 2, 3, 4, 5, 6], 4: [0, 1, 2, 3, 4, 5, 6, 7]}
# devo_amd/csrc/lie_dev.h LieConsts<T>::w_series_max (tests/test_lie_groups_ref_cpu.py compares it with the header)
W_SERIES_MAX = {"float": 1.0, "double": 0.3}
SWEEP_SMALL = [0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.3, 1.0]
SWEEP_THETAS = SWEEP_SMALL + [math.pi - 0.05]
SWEEP_SIGMAS = SWEEP_SMALL + [-s for s in SWEEP_SMALL[1:]]


def dims(gid):
    return len(ELEM_IDX[gid]), len(TAN_IDX[gid])


def tan7(gid, a):
    """[n, K] -> Sim3 tangent [n, 7] (missing parts zero)."""
    out = torch.zeros(a.shape[0], 7, dtype=torch.float64)
    out[:, TAN_IDX[gid]] = a.double()
    return out


def elem8(gid, X):
    """[n, N] -> Sim3 element [n, 8] (missing t = 0, s = 1), quaternion normalised as the kernels do on load."""
    out = torch.zeros(X.shape[0], 8, dtype=torch.float64)
    out[:, 7] = 1.0
    out[:, ELEM_IDX[gid]] = X.double()
    out[:, 3:7] = out[:, 3:7] / out[:, 3:7].norm(dim=-1, keepdim=True)
    return out


def _tan(gid, a7):
    return a7[:, TAN_IDX[gid]]


def _elem(gid, X8):
    return X8[:, ELEM_IDX[gid]]


def pad(gid, g):
    """tangent-shaped gradient -> element-shaped (last slot zero)."""
    return torch.cat([g, torch.zeros_like(g[:, :1])], -1)


def hat3(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).view(*v.shape[:-1], 3, 3)


def hat4(a7):
    """Sim3 algebra element [[Phi + sigma I, tau], [0, 0]]."""
    H = torch.zeros(a7.shape[0], 4, 4, dtype=torch.float64)
    H[:, :3, :3] = hat3(a7[:, 3:6]) + a7[:, 6, None, None] * torch.eye(3, dtype=torch.float64)
    H[:, :3, 3] = a7[:, :3]
    return H


def vee4(H):
    phi = 0.5 * torch.stack([H[:, 2, 1] - H[:, 1, 2], H[:, 0, 2] - H[:, 2, 0], H[:, 1, 0] - H[:, 0, 1]], -1)
    sigma = (H[:, 0, 0] + H[:, 1, 1] + H[:, 2, 2]) / 3.0
    return torch.cat([H[:, :3, 3], phi, sigma[:, None]], -1)


def series_exp(M, terms=TERMS):
    term = torch.eye(M.shape[-1], dtype=torch.float64).expand_as(M).clone()
    out = term.clone()
    for k in range(1, terms):
        term = term @ M / k
        out = out + term
    return out


def series_int(M, terms=TERMS):
    """sum_k M^k / (k+1)!"""
    term = torch.eye(M.shape[-1], dtype=torch.float64).expand_as(M).clone()
    out = term.clone()
    for k in range(1, terms):
        term = term @ M / (k + 1)
        out = out + term
    return out


def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qmat(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def matrix8(X8):
    T = torch.zeros(X8.shape[0], 4, 4, dtype=torch.float64)
    T[:, :3, :3] = X8[:, 7, None, None] * qmat(X8[:, 3:7])
    T[:, :3, 3] = X8[:, :3]
    T[:, 3, 3] = 1.0
    return T


def as_matrix(gid, X):
    return matrix8(elem8(gid, X))


def W(a7):
    return series_int(hat4(a7)[:, :3, :3])


def _exp8(a7):
    phi = a7[:, 3:6]
    theta = phi.norm(dim=-1, keepdim=True)
    q = torch.cat([0.5 * torch.sinc(theta / (2 * math.pi)) * phi, torch.cos(0.5 * theta)], -1)     # sin(t/2)/t = sinc(t / 2pi) / 2
    t = (W(a7) @ a7[:, :3, None])[..., 0]
    return torch.cat([t, q, torch.exp(a7[:, 6:7])], -1)


def expm(gid, a):
    return _elem(gid, _exp8(tan7(gid, a)))


def _log8(X8):
    q = X8[:, 3:7]
    q = torch.where(q[:, 3:] < 0, -q, q)
    v, w = q[:, :3], q[:, 3:]
    n = v.norm(dim=-1, keepdim=True)
    zero = n == 0
    phi = torch.where(zero, 2 * v / w, 2 * torch.atan2(n, w) / torch.where(zero, torch.ones_like(n), n) * v)
    a7 = torch.cat([torch.zeros_like(phi), phi, torch.log(X8[:, 7:8])], -1)
    tau = torch.linalg.solve(W(a7), X8[:, :3, None])[..., 0]
    return torch.cat([tau, a7[:, 3:]], -1)


def logm(gid, X):
    return _tan(gid, _log8(elem8(gid, X)))


def _inv8(X8):
    q = X8[:, 3:7] * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=torch.float64)
    s = 1.0 / X8[:, 7:8]
    t = -s * (qmat(q) @ X8[:, :3, None])[..., 0]
    return torch.cat([t, q, s], -1)


def inv(gid, X):
    return _elem(gid, _inv8(elem8(gid, X)))


def mul(gid, X, Y):
    A, B = elem8(gid, X), elem8(gid, Y)
    q = qmul(A[:, 3:7], B[:, 3:7])
    q = q / q.norm(dim=-1, keepdim=True)
    t = A[:, :3] + A[:, 7:8] * (qmat(A[:, 3:7]) @ B[:, :3, None])[..., 0]
    return _elem(gid, torch.cat([t, q, A[:, 7:8] * B[:, 7:8]], -1))


def _basis(n, j):
    e = torch.zeros(n, 7, dtype=torch.float64)
    e[:, j] = 1.0
    return e


def Adj_matrix(gid, X):
    """K x K, column j = vee(T hat(e_j) T^-1)."""
    T = as_matrix(gid, X)
    Ti = torch.linalg.inv(T)
    cols = [vee4(T @ hat4(_basis(T.shape[0], j)) @ Ti) for j in range(7)]
    A = torch.stack(cols, -1)
    return A[:, TAN_IDX[gid]][:, :, TAN_IDX[gid]]


def ad_matrix(gid, a):
    """K x K, column j = vee([hat a, hat e_j])."""
    Ha = hat4(tan7(gid, a))
    cols = []
    for j in range(7):
        He = hat4(_basis(Ha.shape[0], j))
        cols.append(vee4(Ha @ He - He @ Ha))
    A = torch.stack(cols, -1)
    return A[:, TAN_IDX[gid]][:, :, TAN_IDX[gid]]


def left_jacobian(gid, a):
    return series_int(ad_matrix(gid, a))


def left_jacobian_inverse(gid, a):
    return torch.linalg.inv(left_jacobian(gid, a))


def _mv(M, v):
    return (M @ v.double()[..., None])[..., 0]


def _vm(g, M):
    return (g.double()[..., None, :] @ M)[..., 0, :]


def adj(gid, X, a):
    return _mv(Adj_matrix(gid, X), a)


def adjT(gid, X, a):
    return _mv(Adj_matrix(gid, X).transpose(-1, -2), a)


def act(gid, X, p):
    T = as_matrix(gid, X)
    return _mv(T[:, :3, :3], p) + T[:, :3, 3]


def act4(gid, X, p):
    return _mv(as_matrix(gid, X), p)


def jinv(gid, X, a):
    return _mv(left_jacobian_inverse(gid, logm(gid, X)), a)


def projector(gid, X):
    """[n, N, N]: column j < K is d/d eps of the embedded coordinates of exp(eps e_j) X at eps = 0; the last column is zero."""
    X8 = elem8(gid, X)
    n = X8.shape[0]
    T = matrix8(X8)
    P = torch.zeros(n, 8, 8, dtype=torch.float64)
    for j in range(7):
        e = _basis(n, j)
        P[:, :3, j] = (hat4(e) @ T)[:, :3, 3]
        P[:, 3:7, j] = 0.5 * qmul(torch.cat([e[:, 3:6], torch.zeros(n, 1, dtype=torch.float64)], -1), X8[:, 3:7])
        P[:, 7, j] = e[:, 6] * X8[:, 7]
    N, K = dims(gid)
    out = torch.zeros(n, N, N, dtype=torch.float64)
    out[:, :, :K] = P[:, ELEM_IDX[gid]][:, :, TAN_IDX[gid]]
    return out


# ---- backward ops: vector-Jacobian products (lietorch_gpu.cu:32-256) --------------------------------------------------------------
def expm_backward(gid, g, a):
    K = dims(gid)[1]
    return _vm(g[:, :K], left_jacobian(gid, a))


def logm_backward(gid, g, X):
    return pad(gid, _vm(g, left_jacobian_inverse(gid, logm(gid, X))))


def inv_backward(gid, g, X):
    K = dims(gid)[1]
    return pad(gid, -_vm(g[:, :K], Adj_matrix(gid, inv(gid, X))))


def mul_backward(gid, g, X, Y):
    K = dims(gid)[1]
    return pad(gid, g[:, :K].double()), pad(gid, _vm(g[:, :K], Adj_matrix(gid, X)))


def adj_backward(gid, g, X, a):
    A = Adj_matrix(gid, X)
    return pad(gid, -_vm(g, ad_matrix(gid, _mv(A, a)))), _vm(g, A)


def adjT_backward(gid, g, X, a):
    Ag = _mv(Adj_matrix(gid, X), g)
    return pad(gid, -_vm(a, ad_matrix(gid, Ag))), Ag


def _act_jacobian(gid, q4):
    """[n, 4, K]: column j = hat(e_j) q4, the derivative of exp(eps e_j) acting on the homogeneous point q4."""
    n = q4.shape[0]
    J = torch.stack([_mv(hat4(_basis(n, j)), q4) for j in range(7)], -1)
    return J[:, :, TAN_IDX[gid]]


def act_backward(gid, g, X, p):
    T = as_matrix(gid, X)
    q = act(gid, X, p)
    q4 = torch.cat([q, torch.ones_like(q[:, :1])], -1)
    return pad(gid, _vm(g, _act_jacobian(gid, q4)[:, :3])), _vm(g, T[:, :3, :3])


def act4_backward(gid, g, X, p):
    T = as_matrix(gid, X)
    return pad(gid, _vm(g, _act_jacobian(gid, act4(gid, X, p)))), _vm(g, T)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _unit(n, g):
    u = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def tangent(gid, theta, sigma, tau_norm, n, g):
    """n Sim3-ordered tangents with |phi| = theta, sigma, |tau| = tau_norm (tensors [n] or floats), random directions, cut to the group."""
    as_col = lambda v: (v if torch.is_tensor(v) else torch.full((n,), float(v), dtype=torch.float64)).view(n, 1)
    a7 = torch.cat([as_col(tau_norm) * _unit(n, g), as_col(theta) * _unit(n, g), as_col(sigma)], -1)
    return _tan(gid, a7)


def random_batch(gid, n, seed, dt):
    """Random operands in the domain theta <= pi - 0.05, |sigma| <= 1, |tau| <= 3, rounded to dt; elements are exp of such tangents (rounded to dt),
    every fourth quaternion negated (w < 0), every fifth scaled by 1.7 (renormalised on load)."""
    N, K = dims(gid)
    g = torch.Generator().manual_seed(seed)
    U = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    a = tangent(gid, U(0, math.pi - 0.05), U(-1, 1), U(0, 3), n, g).to(dt)
    X = expm(gid, tangent(gid, U(0, math.pi - 0.05), U(-1, 1), U(0, 3), n, g))
    qo = ELEM_IDX[gid].index(3)
    X[::4, qo:qo + 4] *= -1.0
    X[::5, qo:qo + 4] *= 1.7
    Y = expm(gid, tangent(gid, U(0, math.pi - 0.05), U(-1, 1), U(0, 3), n, g))
    R = lambda d: torch.randn(n, d, generator=g, dtype=torch.float64).to(dt)
    return {"a": a, "X": X.to(dt), "Y": Y.to(dt), "b": R(K), "p4": R(4), "gN": R(N), "gK": R(K), "g4": R(4)}


def sweep_batch(gid, dt, per=4):
    """theta x sigma over SWEEP_THETAS x SWEEP_SIGMAS (RxSO3, Sim3) with |tau| = 1, `per` random directions each, rounded to dt; X = exp of the
    rounded tangent, rounded to dt.  Returns the operands and the list of (theta, sigma, first row, last row + 1)."""
    N, K = dims(gid)
    g = torch.Generator().manual_seed(100 + gid)
    bands, th, sg = [], [], []
    for theta in SWEEP_THETAS:
        for sigma in SWEEP_SIGMAS:
            bands.append((theta, sigma, len(th), len(th) + per))
            th += [theta] * per
            sg += [sigma] * per
    n = len(th)
    a = tangent(gid, torch.tensor(th, dtype=torch.float64), torch.tensor(sg, dtype=torch.float64), 1.0, n, g).to(dt)
    X = expm(gid, a).to(dt)
    gN = torch.randn(n, N, generator=g, dtype=torch.float64).to(dt)
    b = torch.randn(n, K, generator=g, dtype=torch.float64).to(dt)
    return {"a": a, "X": X, "gN": gN, "b": b}, bands
