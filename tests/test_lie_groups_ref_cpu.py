"""The fp64 reference of the four lietorch groups (tests/lie_groups_ref.py) against definitions it does not use itself:
torch.linalg.matrix_exp, conjugation of the 4x4 matrices, matrix products / inverses, and central finite differences.  All fp64, 1e-9.
No GPU: this is where the reference that tests/test_gpu_lie_groups.py compares the kernels with earns its name."""
import math
import os
import re
import pytest
import torch

import lie_groups_ref as R

GROUPS = [1, 2, 3, 4]
TOL = 1e-9


def _batch(gid, n=40, seed=0):
    return R.random_batch(gid, n, seed, torch.float64)


@pytest.mark.parametrize("gid", GROUPS)
def test_exp_is_the_matrix_exponential(gid):
    B = _batch(gid)
    H = R.hat4(R.tan7(gid, B["a"]))
    T = R.as_matrix(gid, R.expm(gid, B["a"]))
    assert (T - torch.linalg.matrix_exp(H)).abs().max() < TOL
    assert (T - R.series_exp(H)).abs().max() < TOL
    assert (R.series_exp(H) - torch.linalg.matrix_exp(H)).abs().max() < 1e-13


@pytest.mark.parametrize("gid", GROUPS)
def test_log_inverts_exp_and_exp_inverts_log(gid):
    B = _batch(gid, seed=1)
    assert (R.logm(gid, R.expm(gid, B["a"])) - B["a"]).abs().max() < TOL
    T = R.as_matrix(gid, B["X"])
    assert (R.as_matrix(gid, R.expm(gid, R.logm(gid, B["X"]))) - T).abs().max() < TOL


@pytest.mark.parametrize("gid", GROUPS)
def test_inv_and_mul_are_the_matrix_ones(gid):
    B = _batch(gid, seed=2)
    TX, TY = R.as_matrix(gid, B["X"]), R.as_matrix(gid, B["Y"])
    assert (R.as_matrix(gid, R.inv(gid, B["X"])) - torch.linalg.inv(TX)).abs().max() < TOL
    assert (R.as_matrix(gid, R.mul(gid, B["X"], B["Y"])) - TX @ TY).abs().max() < TOL


@pytest.mark.parametrize("gid", GROUPS)
def test_adj_is_conjugation(gid):
    """Adj(X) a = vee(X hat(a) X^-1), checked through the group: exp(Adj(X) a) = X exp(a) X^-1."""
    B = _batch(gid, seed=3)
    b = 0.3 * B["b"]
    T = R.as_matrix(gid, B["X"])
    lhs = torch.linalg.matrix_exp(R.hat4(R.tan7(gid, R.adj(gid, B["X"], b))))
    rhs = T @ torch.linalg.matrix_exp(R.hat4(R.tan7(gid, b))) @ torch.linalg.inv(T)
    assert (lhs - rhs).abs().max() < TOL
    c = B["gK"]
    assert ((R.adjT(gid, B["X"], c) * b).sum(-1) - (c * R.adj(gid, B["X"], b)).sum(-1)).abs().max() < TOL


def _fd_columns(f, K, n, h=1e-6):
    """central differences of f(delta) over the K tangent directions: [n, dim, K]"""
    cols = []
    for j in range(K):
        d = torch.zeros(n, K, dtype=torch.float64)
        d[:, j] = h
        cols.append((f(d) - f(-d)) / (2 * h))
    return torch.stack(cols, -1)


@pytest.mark.parametrize("gid", GROUPS)
@pytest.mark.parametrize("sigma", [0.2, 1.0])
def test_left_jacobian_matches_finite_differences(gid, sigma):
    """J_l(a) = d/d delta of log(exp(a + delta) exp(a)^-1) at 0, and its inverse d/d delta of log(exp(delta) exp(a)) at 0."""
    N, K = R.dims(gid)
    g = torch.Generator().manual_seed(4)
    n = 12
    a = sigma * torch.randn(n, K, generator=g, dtype=torch.float64)
    po = R.TAN_IDX[gid].index(3)
    theta = a[:, po:po + 3].norm(dim=-1, keepdim=True)
    a[:, po:po + 3] *= torch.clamp(theta, max=math.pi - 0.05) / theta                  # log is the principal branch: stay inside it
    Xi =R.inv(gid, R.expm(gid, a))
    J = _fd_columns(lambda d: R.logm(gid, R.mul(gid, R.expm(gid, a + d), Xi)), K, n)
    assert (R.left_jacobian(gid, a) - J).abs().max() < TOL * max(1.0, J.abs().max().item())
    X = R.expm(gid, a)
    Ji = _fd_columns(lambda d: R.logm(gid, R.mul(gid, R.expm(gid, d), X)), K, n)
    assert (R.left_jacobian_inverse(gid, a) - Ji).abs().max() < TOL * max(1.0, Ji.abs().max().item())


@pytest.mark.parametrize("gid", GROUPS)
def test_projector_and_point_jacobians_match_finite_differences(gid):
    N, K = R.dims(gid)
    B = _batch(gid, n=12, seed=5)
    X, n = B["X"].clone(), 12
    qo = R.ELEM_IDX[gid].index(3)
    X[:, qo:qo + 4] /= X[:, qo:qo + 4].norm(dim=-1, keepdim=True)          # the embedded coordinates of a proper element
    P = R.projector(gid, X)
    assert P[:, :, K:].abs().max() == 0
    fd = _fd_columns(lambda d: R.mul(gid, R.expm(gid, d), X), K, n)
    assert (P[:, :, :K] - fd).abs().max() < TOL
    # act / act4 backward: the gradient for X is g * d(exp(delta) X p)/d delta, for p it is g * d(X p)/dp
    p4 = B["p4"]
    dX, dp = R.act4_backward(gid, B["g4"], X, p4)
    fdX = _fd_columns(lambda d: R.act4(gid, R.mul(gid, R.expm(gid, d), X), p4), K, n)
    assert (dX[:, :K] - (B["g4"][:, None, :] @ fdX)[:, 0]).abs().max() < 1e-8 and dX[:, K:].abs().max() == 0
    fdp = torch.stack([(R.act4(gid, X, p4 + 1e-6 * torch.eye(4, dtype=torch.float64)[j]) - R.act4(gid, X, p4 - 1e-6 * torch.eye(4, dtype=torch.float64)[j])) / 2e-6
                       for j in range(4)], -1)
    assert (dp - (B["g4"][:, None, :] @ fdp)[:, 0]).abs().max() < 1e-8
    p3 = p4[:, :3].contiguous()
    dX3, dp3 = R.act_backward(gid, B["g4"][:, :3], X, p3)
    fdX3 = _fd_columns(lambda d: R.act(gid, R.mul(gid, R.expm(gid, d), X), p3), K, n)
    assert (dX3[:, :K] - (B["g4"][:, None, :3] @ fdX3)[:, 0]).abs().max() < 1e-8


@pytest.mark.parametrize("gid", GROUPS)
def test_backward_ops_are_the_vjps_of_the_forward_ops(gid):
    """Each backward op against central differences of <g, forward(exp(delta) X, ...)> in the left perturbation delta (the convention of
    lietorch_gpu.cu: the gradient of a group element is taken with respect to exp(delta) X) and in the Euclidean operand."""
    N, K = R.dims(gid)
    n = 10
    B = _batch(gid, n=n, seed=6)
    X, Y, a, b, gK, gN = B["X"], B["Y"], B["a"], B["b"], B["gK"], B["gN"]
    left = lambda d, Z: R.mul(gid, R.expm(gid, d), Z)
    tol = 2e-8

    def close(got, fd, g):
        want = (g[:, None, :].double() @ fd)[:, 0]
        return (got - want).abs().max() < tol * max(1.0, want.abs().max().item())

    # exp: gN is a tangent cotangent of exp(a) in K of N slots: d/d delta of log(exp(a + delta) exp(a)^-1)
    Xi = R.inv(gid, R.expm(gid, a))
    assert close(R.expm_backward(gid, gN, a), _fd_columns(lambda d: R.logm(gid, R.mul(gid, R.expm(gid, a + d), Xi)), K, n), gN[:, :K])
    assert close(R.logm_backward(gid, gK, X)[:, :K], _fd_columns(lambda d: R.logm(gid, left(d, X)), K, n), gK)
    # an output element's perturbation: log(out(delta) out(0)^-1)
    out_pert = lambda f, f0: (lambda d: R.logm(gid, R.mul(gid, f(d), R.inv(gid, f0))))
    assert close(R.inv_backward(gid, gN, X)[:, :K], _fd_columns(out_pert(lambda d: R.inv(gid, left(d, X)), R.inv(gid, X)), K, n), gN[:, :K])
    Z = R.mul(gid, X, Y)
    dX, dY = R.mul_backward(gid, gN, X, Y)
    assert close(dX[:, :K], _fd_columns(out_pert(lambda d: R.mul(gid, left(d, X), Y), Z), K, n), gN[:, :K])
    assert close(dY[:, :K], _fd_columns(out_pert(lambda d: R.mul(gid, X, left(d, Y)), Z), K, n), gN[:, :K])
    dX, da = R.adj_backward(gid, gK, X, b)
    assert close(dX[:, :K], _fd_columns(lambda d: R.adj(gid, left(d, X), b), K, n), gK)
    assert close(da, _fd_columns(lambda d: R.adj(gid, X, b + d), K, n), gK)
    dX, da = R.adjT_backward(gid, gK, X, b)
    assert close(dX[:, :K], _fd_columns(lambda d: R.adjT(gid, left(d, X), b), K, n), gK)
    assert close(da, _fd_columns(lambda d: R.adjT(gid, X, b + d), K, n), gK)
    assert (R.jinv(gid, X, b) - (R.left_jacobian_inverse(gid, R.logm(gid, X)) @ b[..., None])[..., 0]).abs().max() == 0


def test_series_terms_are_enough():
    """60, 90 and 120 terms of W and of Sim3's J_l agree at theta = 3.14, sigma = 1, |tau| = 3 (no branch, no cancellation in the domain)."""
    g = torch.Generator().manual_seed(7)
    a = R.tangent(4, 3.14, 1.0, 3.0, 8, g)
    A, M = R.ad_matrix(4, a), R.hat4(R.tan7(4, a))[:, :3, :3]
    for X in (A, M):
        s60, s90, s120 = R.series_int(X, 60), R.series_int(X, 90), R.series_int(X, 120)
        assert torch.equal(s60, s120) and torch.equal(s90, s120)


def test_switch_point_matches_the_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "devo_amd", "csrc", "lie_dev.h")).read()
    for ctype, want in R.W_SERIES_MAX.items():
        m = re.search(r"struct LieConsts<%s>\s*\{[^}]*w_series_max = ([0-9.e+-]+)f?;" % ctype, src)
        assert m and float(m.group(1)) == want, ctype


def test_sweep_covers_the_issue_grid():
    S, bands = R.sweep_batch(4, torch.float64)
    assert len(bands) == 11 * 19 and S["a"].shape == (11 * 19 * 4, 7)
    assert math.isclose(max(t for t, _, _, _ in bands), math.pi - 0.05) and min(s for _, s, _, _ in bands) == -1.0
    assert (S["a"][:, :3].norm(dim=-1) - 1).abs().max() < 1e-12
