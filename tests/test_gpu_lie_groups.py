"""SO3, RxSO3, SE3 and Sim3 on the GPU (csrc/lie.hip, csrc/lie_dev.h) through the module interface `lietorch_backends` and the classes of
devo_amd.lietorch, against the branch-free fp64 reference tests/lie_groups_ref.py (checked on the CPU by tests/test_lie_groups_ref_cpu.py).
Tolerances are those of tests/test_gpu_lietorch.py: 1e-11 (fp64) and 2e-5 (fp32) relative to max(1, |reference|)."""
import math
import os
import subprocess
import sys
import pytest
import torch

import lie_groups_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOLS = [(torch.float64, 1e-11), (torch.float32, 2e-5)]
NMAX = 1031                                                      # several workgroups of 256 plus a tail; 65 is one past a wave, 1 a single lane
_REF = {}


def _dev(t):
    return t.to(DEV).contiguous()


def _classes():
    from devo_amd.lietorch import SO3, RxSO3, SE3, Sim3
    return {1: SO3, 2: RxSO3, 3: SE3, 4: Sim3}


def _reference(gid, dt):
    """The operands (rounded to dt) and the reference of all 19 functions on them, built once per (group, dtype) at n = NMAX and never changed:
    the smaller batches are its leading rows."""
    if (gid, dt) not in _REF:
        B = R.random_batch(gid, NMAX, 10 * gid + (dt == torch.float32), dt)
        a, X, Y, b, p4, gN, gK, g4 = (B[k] for k in ("a", "X", "Y", "b", "p4", "gN", "gK", "g4"))
        p3, g3 = p4[:, :3].contiguous(), g4[:, :3].contiguous()
        ref = {"expm": R.expm(gid, a), "logm": R.logm(gid, X), "inv": R.inv(gid, X), "mul": R.mul(gid, X, Y), "adj": R.adj(gid, X, b), "adjT": R.adjT(gid, X, b),
               "act": R.act(gid, X, p3), "act4": R.act4(gid, X, p4), "Jinv": R.jinv(gid, X, b), "as_matrix": R.as_matrix(gid, X), "projector": R.projector(gid, X),
               "expm_backward": (R.expm_backward(gid, gN, a),), "logm_backward": (R.logm_backward(gid, gK, X),), "inv_backward": (R.inv_backward(gid, gN, X),),
               "mul_backward": R.mul_backward(gid, gN, X, Y), "adj_backward": R.adj_backward(gid, gK, X, b), "adjT_backward": R.adjT_backward(gid, gK, X, b),
               "act_backward": R.act_backward(gid, g3, X, p3), "act4_backward": R.act4_backward(gid, g4, X, p4)}
        _REF[(gid, dt)] = (dict(B, p3=p3, g3=g3), ref)
    return _REF[(gid, dt)]


def _call_all(Bk, gid, ops, n):
    """Every function of the module once on the first n rows -> {name: tuple of outputs}."""
    d = lambda k: _dev(ops[k][:n])
    a, X, Y, b, p3, p4, gN, gK, g3, g4 = (d(k) for k in ("a", "X", "Y", "b", "p3", "p4", "gN", "gK", "g3", "g4"))
    one = lambda t: (t,)
    return {"expm": one(Bk.expm(gid, a)), "logm": one(Bk.logm(gid, X)), "inv": one(Bk.inv(gid, X)), "mul": one(Bk.mul(gid, X, Y)), "adj": one(Bk.adj(gid, X, b)),
            "adjT": one(Bk.adjT(gid, X, b)), "act": one(Bk.act(gid, X, p3)), "act4": one(Bk.act4(gid, X, p4)), "Jinv": one(Bk.Jinv(gid, X, b)),
            "as_matrix": one(Bk.as_matrix(gid, X)), "projector": one(Bk.projector(gid, X)),
            "expm_backward": tuple(Bk.expm_backward(gid, gN, a)), "logm_backward": tuple(Bk.logm_backward(gid, gK, X)), "inv_backward": tuple(Bk.inv_backward(gid, gN, X)),
            "mul_backward": tuple(Bk.mul_backward(gid, gN, X, Y)), "adj_backward": tuple(Bk.adj_backward(gid, gK, X, b)),
            "adjT_backward": tuple(Bk.adjT_backward(gid, gK, X, b)), "act_backward": tuple(Bk.act_backward(gid, g3, X, p3)),
            "act4_backward": tuple(Bk.act4_backward(gid, g4, X, p4))}


@pytest.mark.parametrize("n", [1, 65, NMAX])
@pytest.mark.parametrize("dt,tol", TOLS)
@pytest.mark.parametrize("gid", [1, 2, 3, 4])
def test_all_19_functions_vs_reference(gid, dt, tol, n):
    """Random operands in the domain theta <= pi - 0.05, |sigma| <= 1, |tau| <= 3 (a quarter of the quaternions negated, a fifth un-normalised)."""
    from devo_amd.backends import lietorch_backends as Bk
    ops, ref = _reference(gid, dt)
    got = _call_all(Bk, gid, ops, n)
    assert len(got) == 19
    bad = []
    for name, outs in got.items():
        refs = ref[name] if isinstance(ref[name], tuple) else (ref[name],)
        assert len(outs) == len(refs), name
        for k, (o, r) in enumerate(zip(outs, refs)):
            r = r[:n]
            assert o.dtype == dt and tuple(o.shape) == tuple(r.shape), f"{name}[{k}]: {tuple(o.shape)} vs {tuple(r.shape)}"
            err = (o.double().cpu() - r).abs().max().item()
            bound = tol * max(1.0, r.abs().max().item())
            print(f"{R.NAMES[gid]:6s} {str(dt)[6:]:8s} n = {n:<5d} {name}[{k}]  max err {err:9.3e}  bound {bound:9.3e}")
            if not err <= bound:
                bad.append(f"{name}[{k}]: {err:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


_SWEEP = {}


def _sweep(gid, dt):
    if (gid, dt) not in _SWEEP:
        S, bands = R.sweep_batch(gid, dt)
        ref = {"expm": R.expm(gid, S["a"]), "logm": R.logm(gid, S["X"]), "Jinv": R.jinv(gid, S["X"], S["b"]),
               "expm_backward": R.expm_backward(gid, S["gN"], S["a"]), "logm_backward": R.logm_backward(gid, S["b"], S["X"])}
        _SWEEP[(gid, dt)] = (S, bands, ref)
    return _SWEEP[(gid, dt)]


@pytest.mark.parametrize("dt,tol", TOLS)
@pytest.mark.parametrize("gid", [2, 4])
def test_small_argument_sweep(gid, dt, tol):
    """theta and |sigma| independently over {0, 1e-7, ..., 1e-2, 0.1, 0.3, 1}, theta also pi - 0.05, both signs of sigma, |tau| = 1: exp, log,
    Jinv and the backward kernels of exp and log of RxSO3 and Sim3, each (theta, sigma) band against its own bound tol * max(1, |ref|).  The
    grid brackets the W switch of csrc/lie_dev.h (0.3 double, 1.0 float: both values are on it, the series side at 0.1 / 0.3).  fp32 log near
    theta = pi - 0.05 needs no wider bound: it measured below 3e-7 there (bound 5e-5: |phi| sets the scale)."""
    from devo_amd.backends import lietorch_backends as Bk
    S, bands, ref = _sweep(gid, dt)
    a, X, gN, b = (_dev(S[k]) for k in ("a", "X", "gN", "b"))
    got = {"expm": Bk.expm(gid, a), "logm": Bk.logm(gid, X), "Jinv": Bk.Jinv(gid, X, b), "expm_backward": Bk.expm_backward(gid, gN, a)[0],
           "logm_backward": Bk.logm_backward(gid, b, X)[0]}
    bad = []
    for name, out in got.items():
        out = out.double().cpu()
        assert out.shape == ref[name].shape, name
        for theta, sigma, i0, i1 in bands:
            r = ref[name][i0:i1]
            err = (out[i0:i1] - r).abs().max().item()
            bound = tol * max(1.0, r.abs().max().item())
            ok = err <= bound                                              # (a NaN fails)
            print(f"{R.NAMES[gid]:6s} {name:14s} {str(dt)[6:]:8s} theta = {theta:<8.3g} sigma = {sigma:<8.3g} max err {err:9.3e}  bound {bound:9.3e}  {'ok' if ok else 'FAIL'}")
            if not ok:
                bad.append(f"{name} at theta = {theta:g}, sigma = {sigma:g}: {err:.3e} > {bound:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("gid", [1, 2, 4])
def test_exp_holds_up_to_theta_6(gid):
    from devo_amd.backends import lietorch_backends as Bk
    g = torch.Generator().manual_seed(3)
    n = 65
    for dt, tol in TOLS:
        a = R.tangent(gid, torch.linspace(3.0, 6.0, n, dtype=torch.float64), 2 * torch.rand(n, generator=g, dtype=torch.float64) - 1, 3.0, n, g).to(dt)
        ref = R.expm(gid, a)
        err = (Bk.expm(gid, _dev(a)).double().cpu() - ref).abs().max().item()
        assert err <= tol * max(1.0, ref.abs().max().item()), f"{dt}: {err:.3e}"


@pytest.mark.parametrize("gid", [1, 2, 3, 4])
def test_reference_identities_fp64(gid):
    """devo/lietorch/run_tests.py:16-52 on the GPU, float64, atol 1e-8, plus matrix() against as_matrix and act against act4."""
    from devo_amd.backends import lietorch_backends as Bk
    G = _classes()[gid]
    K = G.manifold_dim
    torch.manual_seed(gid)
    rn = lambda *s: torch.randn(*s, device=DEV, dtype=torch.float64)
    a = 0.2 * rn(2, 3, 4, 5, K)
    assert torch.allclose(G.exp(a).log(), a, atol=1e-8)
    X = G.exp(0.1 * rn(2, 3, 4, 5, K))
    assert torch.allclose((X * X.inv()).log(), torch.zeros_like(a), atol=1e-8)
    X, b = G.exp(rn(2, 3, 4, 5, K)), rn(2, 3, 4, 5, K)
    Y1, Y2 = X * G.exp(b), G.exp(X.adj(b)) * X
    assert torch.allclose((Y1 * Y2.inv()).log(), torch.zeros_like(b), atol=1e-8)
    X, p = G.exp(rn(6, K)), rn(6, 3)
    ph = torch.cat([p, torch.ones_like(p[..., :1])], -1)
    assert torch.allclose(X.act(p), (X.matrix() @ ph[..., None])[..., 0][..., :3], atol=1e-8)
    assert torch.allclose(X.act(ph)[..., :3], X.act(p), atol=1e-8) and torch.equal(X.act(ph)[..., 3], ph[..., 3])
    assert torch.allclose(X.matrix(), Bk.as_matrix(gid, X.data.contiguous()), atol=1e-8)


def _tangents(G, std, n, seed):
    """std * N(0, 1) tangents with the rotation part clipped to pi - 0.05 (log is the principal branch)."""
    g = torch.Generator().manual_seed(seed)
    a = std * torch.randn(n, G.manifold_dim, generator=g, dtype=torch.float64)
    po = R.TAN_IDX[G.group_id].index(3)
    theta = a[:, po:po + 3].norm(dim=-1, keepdim=True)
    a[:, po:po + 3] *= torch.clamp(theta, max=math.pi - 0.05) / theta
    return a.to(DEV)


def _grad_vs_fd(fn, args, seed):
    """fn(*args) -> [n, ...]; a fixed random weight makes it one real number per row.  Autograd against central differences (h = 1e-6) in every
    coordinate of every argument, at the tolerances of tests/test_gpu_lietorch.py::test_autograd_matches_finite_differences."""
    g = torch.Generator().manual_seed(seed)
    args = [x.clone().requires_grad_(True) for x in args]
    out = fn(*args)
    w = torch.randn(out.shape, generator=g, dtype=torch.float64).to(DEV)
    rows = lambda o: (o * w).reshape(o.shape[0], -1).sum(-1)
    rows(out).sum().backward()
    h = 1e-6
    with torch.no_grad():
        for i, x in enumerate(args):
            num = torch.zeros_like(x)
            flat = num.view(x.shape[0], -1)
            for k in range(flat.shape[1]):
                d = torch.zeros_like(flat)
                d[:, k] = h
                d = d.view_as(x)
                plus = [y + d if j == i else y for j, y in enumerate(args)]
                minus = [y - d if j == i else y for j, y in enumerate(args)]
                flat[:, k] = (rows(fn(*plus)) - rows(fn(*minus))) / (2 * h)
            assert torch.allclose(x.grad, num, rtol=1e-5, atol=1e-6), f"argument {i}: max |autograd - fd| = {(x.grad - num).abs().max().item():.3e}"


@pytest.mark.parametrize("std", [0.2, 1.0])
@pytest.mark.parametrize("gid", [1, 2, 3, 4])
def test_autograd_matches_finite_differences(gid, std):
    """The compositions of devo/lietorch/run_tests.py:56-226 through the classes, fp64, at tangents of standard deviation `std` (the reference
    takes them at a = 0 and lowers its tolerance to 1e-3 for Sim3, whose Jacobians it truncates; here Sim3 holds SE3's tolerance)."""
    G = _classes()[gid]
    K, N, n = G.manifold_dim, G.embedded_dim, 5
    X = G.exp(_tangents(G, std, n, 1))
    a = _tangents(G, std, n, 2)
    rn = lambda d, s: torch.randn(n, d, generator=torch.Generator().manual_seed(s), dtype=torch.float64).to(DEV)
    # exp o log: the Jacobian is the identity
    a1 = a.clone().requires_grad_(True)
    out = G.exp(a1).log()
    for k in range(K):
        (gk,) = torch.autograd.grad(out[:, k].sum(), a1, retain_graph=True)
        e = torch.zeros(K, dtype=torch.float64, device=DEV)
        e[k] = 1.0
        assert torch.allclose(gk, e.expand(n, K), atol=1e-6), f"exp o log, row {k}: {(gk - e).abs().max().item():.3e}"
    _grad_vs_fd(lambda a_: (G.exp(a_) * X).inv().log(), [0.3 * a], 3)
    _grad_vs_fd(lambda a_, b_: (G.exp(a_) * X).adj(b_), [a, rn(K, 4)], 4)
    _grad_vs_fd(lambda a_, b_: (G.exp(a_) * X).adjT(b_), [a, rn(K, 5)], 5)
    _grad_vs_fd(lambda a_, p_: (X * G.exp(a_)).act(p_), [a, rn(3, 6)], 6)
    _grad_vs_fd(lambda a_, p_: (X * G.exp(a_)).act(p_), [a, rn(4, 7)], 7)
    _grad_vs_fd(lambda a_: (G.exp(a_) * X).matrix(), [a], 8)
    _grad_vs_fd(lambda a_: (G.exp(a_) * X).translation(), [a], 9)
    _grad_vs_fd(lambda a_: (G.exp(a_) * X).vec(), [a], 10)
    _grad_vs_fd(lambda a_: (G.exp(a_) * X).retr(0.5 * a_).log(), [0.3 * a], 11)

    def from_vec(v):                                                          # run_tests.py:197-218
        parts = {1: [4], 2: [4, 1], 3: [3, 4], 4: [3, 4, 1]}[gid]
        cols = list(v.split(parts, dim=-1))
        qi = 0 if gid in (1, 2) else 1
        cols[qi] = cols[qi] / cols[qi].norm(dim=-1, keepdim=True)
        if gid in (2, 4):
            cols[-1] = cols[-1].exp()
        return G.InitFromVec(torch.cat(cols, -1)).vec()

    _grad_vs_fd(from_vec, [rn(N, 12)], 12)


@pytest.mark.parametrize("gid", [1, 2, 3, 4])
def test_interface_refuses_what_it_cannot_take(gid):
    from devo_amd.backends import lietorch_backends as Bk
    N, K = R.dims(gid)
    X = _classes()[gid].Identity(4, device=DEV, dtype=torch.float32).data.contiguous()
    a = torch.zeros(4, K, device=DEV)
    p3, p4 = torch.zeros(4, 3, device=DEV), torch.zeros(4, 4, device=DEV)
    assert tuple(Bk.projector(gid, X).shape) == (4, N, N)
    import devo_amd.backends as backends
    if backends.native() is not None:                                       # the op names under torch.ops.devo_hip take the group id as well
        assert torch.equal(torch.ops.devo_hip.se3_projector(gid, X), Bk.projector(gid, X)) and torch.equal(torch.ops.devo_hip.se3_inv(gid, X), Bk.inv(gid, X))
        with pytest.raises(RuntimeError):
            torch.ops.devo_hip.se3_exp(0, a)
    for bad_id in (0, 5):
        for call in (lambda: Bk.expm(bad_id, a), lambda: Bk.inv(bad_id, X), lambda: Bk.projector(bad_id, X), lambda: Bk.act(bad_id, X, p3),
                     lambda: Bk.mul_backward(bad_id, X, X, X)):
            with pytest.raises(RuntimeError):
                call()
    wide = lambda t: torch.zeros(t.shape[0], t.shape[1] + 1, device=DEV)
    for call in (lambda: Bk.expm(gid, wide(a)), lambda: Bk.logm(gid, wide(X)), lambda: Bk.inv(gid, a), lambda: Bk.mul(gid, X, wide(X)), lambda: Bk.adj(gid, X, wide(a)),
                 lambda: Bk.adjT(gid, X, X), lambda: Bk.act(gid, X, p4), lambda: Bk.act4(gid, X, p3), lambda: Bk.Jinv(gid, X, wide(a)), lambda: Bk.as_matrix(gid, a),
                 lambda: Bk.projector(gid, wide(X)), lambda: Bk.expm_backward(gid, a, a), lambda: Bk.logm_backward(gid, X, X), lambda: Bk.inv_backward(gid, a, X),
                 lambda: Bk.mul_backward(gid, X, X, a), lambda: Bk.adj_backward(gid, X, X, a), lambda: Bk.adjT_backward(gid, a, X, X),
                 lambda: Bk.act_backward(gid, p4, X, p3), lambda: Bk.act4_backward(gid, p4, X, p3), lambda: Bk.mul(gid, X, X[:2].contiguous())):
        with pytest.raises(RuntimeError):
            call()
    for call in (lambda: Bk.inv(gid, X.cpu()), lambda: Bk.projector(gid, X.cpu()), lambda: Bk.adj(gid, X, a.cpu())):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    for call in (lambda: Bk.mul(gid, X, X.double()), lambda: Bk.adj(gid, X.double(), a), lambda: Bk.inv(gid, X.half()), lambda: Bk.expm_backward(gid, X.double(), a)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        Bk.inv(gid, torch.zeros(4, 2 * N, device=DEV)[:, :N])               # not contiguous


_LEG = r"""
import sys, os, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import devo_amd.backends as B
from devo_amd.backends import lietorch_backends as lie
import lie_groups_ref as R
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
out = {}
for gid in (1, 2, 3, 4):
    ops = R.random_batch(gid, 65, 7, torch.float32)
    ops = {k: v.cuda().contiguous() for k, v in ops.items()}
    a, X, Y, b, p4, gN, gK, g4 = (ops[k] for k in ("a", "X", "Y", "b", "p4", "gN", "gK", "g4"))
    p3, g3 = p4[:, :3].contiguous(), g4[:, :3].contiguous()
    res = {"expm": [lie.expm(gid, a)], "logm": [lie.logm(gid, X)], "inv": [lie.inv(gid, X)], "mul": [lie.mul(gid, X, Y)], "adj": [lie.adj(gid, X, b)],
           "adjT": [lie.adjT(gid, X, b)], "act": [lie.act(gid, X, p3)], "act4": [lie.act4(gid, X, p4)], "Jinv": [lie.Jinv(gid, X, b)],
           "as_matrix": [lie.as_matrix(gid, X)], "projector": [lie.projector(gid, X)], "expm_backward": lie.expm_backward(gid, gN, a),
           "logm_backward": lie.logm_backward(gid, gK, X), "inv_backward": lie.inv_backward(gid, gN, X), "mul_backward": lie.mul_backward(gid, gN, X, Y),
           "adj_backward": lie.adj_backward(gid, gK, X, b), "adjT_backward": lie.adjT_backward(gid, gK, X, b), "act_backward": lie.act_backward(gid, g3, X, p3),
           "act4_backward": lie.act4_backward(gid, g4, X, p4)}
    for name, ts in res.items():
        for k, t in enumerate(ts):
            out[f"{gid}.{name}.{k}"] = t
torch.cuda.synchronize()
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_both_bindings_return_the_same_bits(tmp_path):
    """One call of each of the 19 functions per group through devo_amd._C and through ctypes (the switch is read at import: child processes)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, root, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res.append(torch.load(path))
    a, b = res
    assert a.keys() == b.keys() and len(a) == 4 * (19 + 5)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]), f"{k}: the two bindings disagree"


def test_conversions_cat_stack_and_broadcasting():
    from devo_amd import lietorch
    from devo_amd.lietorch import SO3, RxSO3, SE3, Sim3
    torch.manual_seed(5)
    kw = dict(device=DEV, dtype=torch.float64)
    T = SE3.exp(torch.randn(3, 6, **kw))
    S = Sim3.exp(0.5 * torch.randn(3, 7, **kw))
    Rq = SO3(T)
    assert isinstance(Rq, SO3) and torch.equal(Rq.data, T.data[..., 3:7])
    assert torch.equal(SO3(SE3(Rq)).data, Rq.data) and torch.equal(SE3(Rq).data[..., :3], torch.zeros(3, 3, **kw))
    assert torch.equal(RxSO3(S).data, S.data[..., 3:8]) and torch.equal(Sim3(S).data, S.data) and torch.equal(SE3(T).data, T.data)
    assert torch.equal(Sim3(T).data, torch.cat([T.data, torch.ones(3, 1, **kw)], -1))
    assert torch.equal(Sim3(Rq).data, torch.cat([torch.zeros(3, 3, **kw), Rq.data, torch.ones(3, 1, **kw)], -1))
    p = torch.randn(3, 3, **kw)
    assert torch.allclose(Sim3(T).act(p), T.act(p), atol=1e-12) and torch.allclose(Sim3(Rq).act(p), Rq.act(p), atol=1e-12)
    assert torch.allclose(SE3(Rq).act(p), Rq.act(p), atol=1e-12) and torch.allclose(RxSO3(S).act(p), S.act(p) - S.translation()[..., :3], atol=1e-12)
    for G, X in ((SO3, Rq), (RxSO3, RxSO3(S)), (SE3, T), (Sim3, S)):
        assert (G.group_id, G.manifold_dim, G.embedded_dim) == (X.group_id, X.data.shape[-1] - 1, X.data.shape[-1]) and G.group_name == G.__name__
        C, St = lietorch.cat([X, X], 0), lietorch.stack([X, X], 0)
        assert type(C) is G and type(St) is G and tuple(C.shape) == (6,) and tuple(St.shape) == (2, 3)
        assert type(X.inv()) is G and type(X * X) is G and type(X[1:]) is G and type(X.detach()) is G and type(X.view((3, 1))) is G
        I = G.Identity(2, 3, **kw)
        assert tuple(I.shape) == (2, 3) and torch.equal(I.data, G.id_elem.to(**kw).expand(2, 3, G.embedded_dim))
        assert torch.allclose(G.IdentityLike(X).log(), torch.zeros(3, G.manifold_dim, **kw), atol=1e-15)
        assert tuple(G.Random(4, 2, **kw).shape) == (4, 2) and tuple(X.tangent_shape) == (3, G.manifold_dim)
        # broadcasting over leading dimensions, as for SE3
        pts = torch.randn(5, 3, 3, **kw)
        out = G(X.data[None]).act(pts)
        assert tuple(out.shape) == (5, 3, 3) and torch.allclose(out[2], X.act(pts[2]), atol=1e-12)
        Z = G(X.data[:, None]) * G(X.data[None, :])
        assert tuple(Z.shape) == (3, 3) and torch.allclose(Z.data[1, 2], (X[1:2] * X[2:3]).data[0], atol=1e-12)
        with pytest.raises(AssertionError):
            G(X.data[:2]).act(pts)


def test_result_sim3_applies_the_alignment():
    """One synthetic pair: 40 poses, the estimate is the ground truth under a known similarity plus noise.  Result.sim3() is the alignment as a group
    element: S.act(estimated positions) gives the errors whose rmse the result reports; a flagged pair stays NaN."""
    from devo_amd import evaluation as E
    from devo_amd.lietorch import Sim3
    g = torch.Generator().manual_seed(11)
    n = 40
    gt = torch.zeros(n, 7, dtype=torch.float64)
    gt[:, :3] = torch.cumsum(0.3 * torch.randn(n, 3, generator=g, dtype=torch.float64), 0)
    gt[:, 6] = 1.0
    known = torch.tensor([[0.4, -1.0, 2.0, 0.3, -0.5, 0.1, 0.8, 2.5]], dtype=torch.float64)
    known[:, 3:7] /= known[:, 3:7].norm()
    est = gt.clone()
    est[:, :3] = R.act(4, R.inv(4, known).expand(n, 8), gt[:, :3]) + 0.01 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    stamps = torch.arange(n, dtype=torch.int64) * 1000
    res = E.evaluate(est.to(DEV), stamps.to(DEV), gt.to(DEV), stamps.to(DEV), max_diff=10, align="sim3")
    S = res.sim3()
    assert isinstance(S, Sim3) and tuple(S.shape) == (1,) and S.dtype == torch.float64
    assert torch.equal(S.data[:, :7], res.transform[:, 1:8]) and torch.equal(S.data[:, 7], res.transform[:, 0])
    aligned = S.act(est[:, :3].contiguous().to(DEV))                                        # [n, 3]: the one element broadcasts over the poses
    rmse = ((aligned - gt[:, :3].to(DEV)) ** 2).sum(-1).mean().sqrt()
    assert abs(rmse.item() - res.rmse[0].item()) < 1e-9, (rmse.item(), res.rmse[0].item())
    assert abs(S.data[0, 7].item() - 2.5) < 0.05
    flagged = E.evaluate(est[:8].to(DEV), (stamps[:8] + 10_000_000).to(DEV), gt.to(DEV), stamps.to(DEV), max_diff=10, align="sim3", check=False)
    assert int(flagged.status[0]) != 0 and bool(torch.isnan(flagged.sim3().data).all())
