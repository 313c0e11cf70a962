"""GPU parity of the SE3 kernels (lietorch_backends.*) against the CPU oracle (oracle/se3.py), forward and
backward, fp64 (tight) and fp32; plus the reference's own algebraic identities (run_tests.py:16-52) through
the devo_amd.lietorch.SE3 type, and autograd through the HIP ops."""
import pytest
import torch
from oracle import se3 as K

import se3_series_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rand(n, seed=0, dt=torch.float64):
    g = torch.Generator().manual_seed(seed)
    a = 0.5 * torch.randn(n, 6, generator=g, dtype=torch.float64)
    a[: n // 8, 3:] *= 1e-9                                  # exercise the small-angle branches
    X = K.expm(a)
    X[n // 2:, 3:] *= 1.7                                    # un-normalised quaternions must be renormalised on load
    Y = K.expm(0.5 * torch.randn(n, 6, generator=g, dtype=torch.float64))
    b = torch.randn(n, 6, generator=g, dtype=torch.float64)
    p4 = torch.randn(n, 4, generator=g, dtype=torch.float64)
    g7 = torch.randn(n, 7, generator=g, dtype=torch.float64)
    return [t.to(dt) for t in (a, X, Y, b, p4, g7)]


@pytest.mark.parametrize("dt,tol", [(torch.float64, 1e-11), (torch.float32, 2e-5)])
def test_forward_backward_vs_oracle(dt, tol):
    from devo_amd.backends import lietorch_backends as B
    a, X, Y, b, p4, g7 = _rand(1000, 1, dt)
    d = lambda t: t.to(DEV).contiguous()
    o = lambda t: t.double()
    cases = [
        ("expm", B.expm(3, d(a)), K.expm(o(a))),
        ("logm", B.logm(3, d(X)), K.logm(o(X))),
        ("inv", B.inv(3, d(X)), K.inv(o(X))),
        ("mul", B.mul(3, d(X), d(Y)), K.mul(o(X), o(Y))),
        ("adj", B.adj(3, d(X), d(b)), K.adj(o(X), o(b))),
        ("adjT", B.adjT(3, d(X), d(b)), K.adjT(o(X), o(b))),
        ("act", B.act(3, d(X), d(p4[:, :3].contiguous())), K.act(o(X), o(p4[:, :3]))),
        ("act4", B.act4(3, d(X), d(p4)), K.act4(o(X), o(p4))),
        ("as_matrix", B.as_matrix(3, d(X)), K.as_matrix(o(X))),
        ("Jinv", B.Jinv(3, d(X), d(b)), K.jinv(o(X), o(b))),
        ("expm_backward", B.expm_backward(3, d(g7), d(a))[0], K.expm_backward(o(g7), o(a))),
        ("logm_backward", B.logm_backward(3, d(b), d(X))[0], K.logm_backward(o(b), o(X))),
        ("inv_backward", B.inv_backward(3, d(g7), d(X))[0], K.inv_backward(o(g7), o(X))),
    ]
    for name, got, ref in cases:
        err = (got.double().cpu() - ref).abs().max().item()
        assert err <= tol * max(1.0, ref.abs().max().item()), f"{name}: {err}"
    pairs = [
        ("mul_backward", B.mul_backward(3, d(g7), d(X), d(Y)), K.mul_backward(o(g7), o(X), o(Y))),
        ("adj_backward", B.adj_backward(3, d(b), d(X), d(a)), K.adj_backward(o(b), o(X), o(a))),
        ("adjT_backward", B.adjT_backward(3, d(b), d(X), d(a)), K.adjT_backward(o(b), o(X), o(a))),
        ("act_backward", B.act_backward(3, d(p4[:, :3].contiguous()), d(X), d(g7[:, :3].contiguous())),
         K.act_backward(o(p4[:, :3]), o(X), o(g7[:, :3]))),
        ("act4_backward", B.act4_backward(3, d(p4), d(X), d(g7[:, :4].contiguous())),
         K.act4_backward(o(p4), o(X), o(g7[:, :4]))),
    ]
    for name, got, ref in pairs:
        for gt, rf in zip(got, ref):
            err = (gt.double().cpu() - rf).abs().max().item()
            assert err <= tol * max(1.0, rf.abs().max().item()), f"{name}: {err}"


# ------------------------------------------------------------------------------------------------- the small-angle sweep
_SWEEP_REF = {}


def _sweep(dt):
    """Inputs rounded to dt and the series reference (tests/se3_series_ref.py, fp64, no thresholds) of the rounded values; built once per dtype."""
    if dt not in _SWEEP_REF:
        a, X, g7, b = S.sweep_batch(S.SWEEP_THETAS, dt)
        ref = {"expm": S.exp_ref(a), "logm": S.log_ref(X), "expm_backward": S.expm_backward(g7, a), "logm_backward": S.logm_backward(b, X),
               "Jinv": S.jinv(X, b)}
        _SWEEP_REF[dt] = ((a, X, g7, b), ref)
    return _SWEEP_REF[dt]


@pytest.mark.parametrize("dt,tol", [(torch.float64, 1e-11), (torch.float32, 2e-5)])
def test_small_angle_sweep_vs_series_reference(dt, tol):
    """Exp, Log, their backward kernels and Jinv at fixed rotation magnitudes from 1e-7 rad to pi - 1e-3, 256 random directions each, with
    tau, g7, b ~ N(0,1): below and above eps = 1e-6, through the band where the closed-form coefficients (1 - cos t)/t^2, (t - sin t)/t^3, ...
    cancel, and 0.97x / 1.03x either side of every series switch of csrc/se3_dev.h (S.SWITCH_POINTS: 0.3 for double, 1.0 for float).  Every
    fourth quaternion is negated (w < 0), every fifth scaled by 1.7 (renormalised on load).  The reference is the branch-free series of
    tests/se3_series_ref.py, not oracle/se3.py, which restates the closed forms and cancels with them.  The bound is
    test_forward_backward_vs_oracle's, err <= tol * max(1, |ref|_max), taken per magnitude so that large-angle rows do not set the scale."""
    from devo_amd.backends import lietorch_backends as B
    (a, X, g7, b), ref = _sweep(dt)
    d = lambda t: t.to(DEV).contiguous()
    got = {"expm": B.expm(3, d(a)), "logm": B.logm(3, d(X)), "expm_backward": B.expm_backward(3, d(g7), d(a))[0],
           "logm_backward": B.logm_backward(3, d(b), d(X))[0], "Jinv": B.Jinv(3, d(X), d(b))}
    n, bad = len(a) // len(S.SWEEP_THETAS), []
    for name, out in got.items():
        out = out.double().cpu()
        assert out.shape == ref[name].shape, name
        for i, theta in enumerate(S.SWEEP_THETAS):
            r = ref[name][i * n:(i + 1) * n]
            err = (out[i * n:(i + 1) * n] - r).abs().max().item()
            bound = tol * max(1.0, r.abs().max().item())
            ok = err <= bound                                            # (a NaN fails)
            print(f"{name:14s} {str(dt)[6:]:8s} |phi| = {theta:<12.6g} max err {err:9.3e}  bound {bound:9.3e}  {'ok' if ok else 'FAIL'}")
            if not ok:
                bad.append(f"{name} at |phi| = {theta:g}: {err:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


def test_small_angle_gradients_through_the_SE3_type():
    """fp32, |phi| = 1e-3, through devo_amd.lietorch.SE3 autograd.  Same reference and tolerance as the sweep: the Python layer reaches the same
    kernels.  Three legs: (1) d/da of <Log(Exp a), b> = b J_l^-1(a) J_l(a).  That product is the identity, so this leg sees only the uncorrelated
    rounding of the two Jacobians and is the weakest of the three (with closed-form coefficients it measured 7.4e-5 against a bound of about 8e-5).
    (2) X.retr(a) = Exp(a) X sends a cotangent g to g J_l(a) for a and g Adj(Exp a) for X: J_l alone.  (3) <Log(Exp(a) X), b>: J_l^-1 is taken at
    Log(Exp(a) X), not at a, so the two Jacobians do not cancel; its gradient is b J_l^-1(Log Y) J_l(a) for a and b J_l^-1(Log Y) Adj(Exp a) for X."""
    from devo_amd.lietorch import SE3
    tol = 2e-5
    a, X, g7, b = S.sweep_inputs(1e-3, torch.float32, n=256, seed=11)
    Xe = S.exp_ref(a)
    scale = lambda r: tol * max(1.0, r.abs().max().item())
    a1 = a.to(DEV).requires_grad_(True)
    (SE3.exp(a1).log() * b.to(DEV)).sum().backward()
    want = S.expm_backward(S.logm_backward(b, Xe), a)
    err = (a1.grad.double().cpu() - want).abs().max().item()
    print(f"exp().log() grad: max err {err:.3e}")
    assert err <= scale(want), f"exp().log(): {err:.3e}"
    a2, X2 = a.to(DEV).requires_grad_(True), X.to(DEV).requires_grad_(True)
    (SE3(X2).retr(a2).data * g7.to(DEV)).sum().backward()
    want_a = S.expm_backward(g7, a)
    want_X = K.mul_backward(g7.double(), Xe, X.double())[1]
    err_a = (a2.grad.double().cpu() - want_a).abs().max().item()
    err_X = (X2.grad.double().cpu() - want_X).abs().max().item()
    print(f"retr grad: a max err {err_a:.3e}, X max err {err_X:.3e}")
    assert err_a <= scale(want_a), f"retr, a: {err_a:.3e}"
    assert err_X <= scale(want_X), f"retr, X: {err_X:.3e}"
    a3, X3 = a.to(DEV).requires_grad_(True), X.to(DEV).requires_grad_(True)
    ((SE3.exp(a3) * SE3(X3)).log() * b.to(DEV)).sum().backward()
    gY = S.logm_backward(b, K.mul(Xe, X.double()))
    want_a = S.expm_backward(gY, a)
    want_X = K.mul_backward(gY, Xe, X.double())[1]
    err_a = (a3.grad.double().cpu() - want_a).abs().max().item()
    err_X = (X3.grad.double().cpu() - want_X).abs().max().item()
    print(f"(exp() * X).log() grad: a max err {err_a:.3e}, X max err {err_X:.3e}")
    assert err_a <= scale(want_a), f"(exp() * X).log(), a: {err_a:.3e}"
    assert err_X <= scale(want_X), f"(exp() * X).log(), X: {err_X:.3e}"


def test_reference_identities_fp64():
    """devo/lietorch/run_tests.py:16-52 on the GPU, float64, atol 1e-8."""
    from devo_amd.lietorch import SE3
    torch.manual_seed(0)
    a = 0.2 * torch.randn(2, 3, 4, 5, 6, device=DEV, dtype=torch.float64)
    assert torch.allclose(SE3.exp(a).log(), a, atol=1e-8)
    X = SE3.exp(0.1 * torch.randn(2, 3, 4, 5, 6, device=DEV, dtype=torch.float64))
    assert torch.allclose((X * X.inv()).log(), torch.zeros_like(a[..., :6]), atol=1e-8)
    X = SE3.exp(torch.randn(2, 3, 4, 5, 6, device=DEV, dtype=torch.float64))
    b = torch.randn(2, 3, 4, 5, 6, device=DEV, dtype=torch.float64)
    Y1, Y2 = X * SE3.exp(b), SE3.exp(X.adj(b)) * X
    assert torch.allclose((Y1 * Y2.inv()).log(), torch.zeros_like(b), atol=1e-8)
    X = SE3.exp(torch.randn(1, 6, device=DEV, dtype=torch.float64))
    p = torch.randn(1, 3, device=DEV, dtype=torch.float64)
    ph = torch.cat([p, torch.ones_like(p[..., :1])], -1)
    assert torch.allclose(X.act(p), (X.matrix() @ ph[..., None])[..., 0][..., :3], atol=1e-8)


def test_groups_golden_on_gpu(golden_dir):
    import os
    import numpy as np
    from devo_amd.lietorch import SE3
    z = np.load(os.path.join(golden_dir, "groups_f64.npz"))
    g = {k: torch.from_numpy(z[k]).to(DEV) for k in z.files}
    X = SE3(g["poses"])
    assert torch.allclose(SE3(g["poses"][:, :, None]) * g["pts"], g["act"], atol=1e-11)
    assert torch.allclose(X.retr(g["a"]).data, g["retr"], atol=1e-11)
    assert torch.allclose(X.matrix(), g["matrix"], atol=1e-11)
    assert torch.allclose(X.translation(), g["translation"], atol=1e-11)
    assert torch.allclose(X.inv().data, g["inv"], atol=1e-11)
    assert torch.allclose(X.log(), g["log"], atol=1e-11)
    assert torch.allclose((X * X.inv()[:, [0]]).data, g["mul"], atol=1e-11)
    assert torch.allclose(X.scale(torch.full((1, X.shape[1]), 2.0, device=DEV, dtype=torch.float64)).data, g["scale"], atol=1e-12)


def test_autograd_matches_finite_differences():
    """End-to-end real-valued function through Exp, Mul, Inv, Act4, AdjT, Log on the GPU (fp64)."""
    from devo_amd.lietorch import SE3
    torch.manual_seed(3)
    a = (0.3 * torch.randn(7, 6, device=DEV, dtype=torch.float64)).requires_grad_(True)
    Y = SE3.exp(0.4 * torch.randn(7, 6, device=DEV, dtype=torch.float64))
    p = torch.randn(7, 4, device=DEV, dtype=torch.float64)
    b = torch.randn(7, 6, device=DEV, dtype=torch.float64)

    def f(a_):
        X = SE3.exp(a_)
        G = (Y * X.inv()) * X.retr(0.1 * a_)
        return (G.act(p) ** 2).sum() + (G.adjT(b) * b).sum() + (G.log() ** 2).sum()

    f(a).backward()
    num = torch.zeros_like(a)
    h = 1e-6
    with torch.no_grad():
        for i in range(7):
            for k in range(6):
                d = torch.zeros_like(a)
                d[i, k] = h
                num[i, k] = (f(a + d) - f(a - d)) / (2 * h)
    assert torch.allclose(a.grad, num, rtol=1e-5, atol=1e-6)
