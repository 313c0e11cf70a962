"""Plain references for the three kernel pairs of the differentiable bundle adjustment (devo_amd/ba.py: devo_ba_edge_terms,
devo_ba_solve_terms, devo_ba_apply_step and their adjoints): test infrastructure, everything here runs on the CPU in the dtype of
its inputs (fp64 as the yardstick, fp32 for the envelope of the reference's own arithmetic).  Every function is written with
ordinary differentiable torch operations, so torch.autograd.grad gives the reference adjoint.

  edge_terms_ref   devo/ba.py:95-106   residual, gates, the 30 numbers per edge  r(2) | w(2) | Jz(2) | -Ji(12) | Jj(12)
  solve_from_terms devo/ba.py:108-170  dense normal equations, Schur complement, damped Cholesky solve
  apply_step_ref   devo/ba.py:172-182  depth update + clamp, retraction of the optimised poses (oracle/se3.py's group operations)

tests/test_ba_terms_ref_cpu.py pins their composition to oracle/pops.py:BA, which the goldens pin to the reference."""
import functools
import torch
from oracle import lie
from oracle.pops import CholeskySolver
from util import rel_err

GROUPS = (("r", slice(0, 2)), ("w", slice(2, 4)), ("Jz", slice(4, 6)), ("Ji", slice(6, 18)), ("Jj", slice(18, 30)))    # columns of the terms


def edge_terms_ref(coords, valid, Ji, Jj, Jz, target, weight, bounds):
    """coords [1,E,P,P,2], valid [1,E], Ji / Jj [1,E,2,6], Jz [1,E,2,1], target / weight [1,E,2] -> (terms [E,30], gate [E]).
    The gate is piecewise constant: it carries no gradient.  Every operation is a subtraction, a negation or a product with 0 / 1 (the
    norm only decides the gate), so an fp32 evaluation is exact up to the one rounding of the subtraction."""
    E = coords.shape[1]
    c = coords.shape[3] // 2
    ctr = coords[0, :, c, c, :]
    r = target[0] - ctr
    rx, ry = r.detach().unbind(-1)
    cx, cy = ctr.detach().unbind(-1)
    gate = valid[0].detach() * (torch.sqrt(rx * rx + ry * ry) < 250).to(r.dtype)
    gate = gate * ((cx > bounds[0]) & (cy > bounds[1]) & (cx < bounds[2]) & (cy < bounds[3])).to(r.dtype)
    terms = torch.cat([gate[:, None] * r, gate[:, None] * weight[0], Jz[0, :, :, 0], (-Ji[0]).reshape(E, 12), Jj[0].reshape(E, 12)], dim=1)
    return terms, gate


def solve_from_terms(terms, lmbda, ii, jj, kk, Np, t0, N, ep):
    """terms [E,30] -> (dX [6N], dZ [Np]).  Frames outside [t0, t0 + N) are dropped from the pose system; S' = S + (ep + 1e-4 diag S),
    Q = 1 / (C + lambda); patch slots without an edge get dZ = 0; a Cholesky breakdown gives dX = 0 and no gradient through the solve."""
    dt = terms.dtype
    E, n6 = terms.shape[0], 6 * N
    r, w, Jz = terms[:, 0:2], terms[:, 2:4], terms[:, 4:6]
    Ji, Jj = -terms[:, 6:18].reshape(E, 2, 6), terms[:, 18:30].reshape(E, 2, 6)
    C = torch.zeros(Np, dtype=dt).index_add(0, kk, (w * Jz * Jz).sum(-1))
    u = torch.zeros(Np, dtype=dt).index_add(0, kk, (w * Jz * r).sum(-1))
    seen = torch.bincount(kk, minlength=Np) > 0
    Q = torch.where(seen, 1.0 / torch.where(seen, C + lmbda, torch.ones_like(C)), torch.zeros_like(C))
    if N == 0:
        return torch.zeros(0, dtype=dt), Q * u
    # A[e, d, :]: row d of the edge's Jacobian with respect to all 6N pose parameters (ii == jj: both blocks land in one)
    a, b = ii - t0, jj - t0
    ina, inb = ((a >= 0) & (a < N)).to(dt), ((b >= 0) & (b < N)).to(dt)
    oh = lambda ix, m: torch.nn.functional.one_hot(ix.clamp(0, N - 1), N).to(dt) * m[:, None]                  # [E, N]
    A = (oh(a, ina)[:, None, :, None] * Ji[:, :, None, :] + oh(b, inb)[:, None, :, None] * Jj[:, :, None, :]).reshape(E, 2, n6)
    wA = w[:, :, None] * A
    B = torch.einsum('edp,edq->pq', wA, A)
    v = (wA * r[:, :, None]).sum((0, 1))
    Ec = torch.zeros(Np, n6, dtype=dt).index_add(0, kk, (wA * Jz[:, :, None]).sum(1))                           # [Np, 6N]
    EQ = Ec.t() * Q[None]
    S = B - EQ @ Ec
    y = v - EQ @ u
    S = S + (ep + 1e-4 * S) * torch.eye(n6, dtype=dt)
    dX = CholeskySolver.apply(S[None], y[None, :, None])[0, :, 0]
    return dX, Q * (u - Ec @ dX)


def apply_step_ref(poses, patches, dX, dZ, fixedp, n_opt, dmin, dmax):
    """poses [1,n,7], patches [1,Np,3,P,P] -> (Exp(dX_i) * pose_i on [fixedp, fixedp + n_opt) and Exp(0) * pose_i elsewhere, as
    devo/ba.py:179-180 does; inverse depths d + dZ_k clamped to [dmin, dmax]).  Quaternions are renormalised on load (so3.h:31-37);
    pose gradients follow lietorch's convention (a tangent in the first six of seven slots).  oracle.lie.Exp / Mul are nothing but
    torch.autograd.Function shells around oracle/se3.py: forward = expm / mul, backward = expm_backward / mul_backward."""
    n = poses.shape[1]
    disp = (patches[:, :, 2] + dZ.view(1, -1, 1, 1)).clamp(min=dmin, max=dmax)
    patches = torch.stack([patches[:, :, 0], patches[:, :, 1], disp], dim=2)
    upd = torch.zeros(n, 6, dtype=poses.dtype)
    if n_opt > 0:
        upd = upd.index_add(0, fixedp + torch.arange(n_opt), dX.view(n_opt, 6))
    return lie.Mul.apply(lie.Exp.apply(upd), poses[0].contiguous())[None], patches


def whole_step(transform, poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, bounds, ep, fixedp, structure_only=False):
    """one Gauss-Newton step as the fused path composes it: transform(jacobian) -> edge terms -> solve -> apply.  poses: a [1,n,7] tensor."""
    n = max(int(ii.max()), int(jj.max())) + 1 - fixedp
    coords, ok, (Ji, Jj, Jz) = transform(lie.SE3(poses), patches, intrinsics, ii, jj, kk, jacobian=True)
    terms, _ = edge_terms_ref(coords, ok, Ji, Jj, Jz, target, weight, bounds)
    n_opt = 0 if structure_only else max(n, 0)
    dX, dZ = solve_from_terms(terms, lmbda, ii, jj, kk, patches.shape[1], fixedp, n_opt, ep)
    return apply_step_ref(poses, patches, dX, dZ, fixedp, n_opt, 1e-3, 10.0)


# ------------------------------------------------------------------------------------------------- random terms for the solve
TERMS_N = (0, 1, 8, 9, 11, 12, 14, 15, 16, 17, 21, 22, 32)      # both sides of every switch: accumulate <8> | <11> | <14> | <16> | general, solver chain | k_ba_solve
TERMS_NP = 61                                                   # patch slots: no multiple of the accumulate kernels' 8 / 6 / 4 / 16 waves ...
TERMS_SEEN = 53                                                 # ... nor is the number of slots with an edge


def terms_t0(N):
    return (0, 1, 3)[TERMS_N.index(N) % 3] if N in TERMS_N else 1


@functools.lru_cache(maxsize=None)
def terms_case(N, t0=None, ep=None, zero_weight=False, seed=0):
    """Random edge terms around the pose window [t0, t0 + N): independent columns (not derived from geometry, so a swapped or mis-signed
    column shows) with the magnitudes of real ones — Jacobians O(100), Jz O(10), r O(1 px), w in (0, 1).  Frames reach two below t0 (where
    there are any) and two above the window; every case has edges with ii == jj inside the window (N > 0), edges with both ends outside, patch
    slots without an edge, and E no multiple of 64.  The edge list is patch-major; `shuffle` is a permutation of it.  zero_weight: every edge
    of one patch carries w = 0 (C = 0, Q = 1 / lambda).  -> dict; nobody may write into it."""
    t0 = terms_t0(N) if t0 is None else t0
    ep = (10.0, 100.0)[(N + t0) % 2] if ep is None else ep
    g = torch.Generator().manual_seed(9000 + 37 * N + t0 + seed)
    lo, hi = max(0, t0 - 2), t0 + N + 2
    F = hi - lo
    slots = torch.randperm(TERMS_NP, generator=g)[:TERMS_SEEN].sort().values
    src = lo + torch.randint(0, F, (TERMS_SEEN,), generator=g)
    if N > 0:
        src[:8] = t0 + torch.randint(0, N, (8,), generator=g)                       # these patches live inside the window ...
    src[8:12] = t0 + N + torch.randint(0, 2, (4,), generator=g)                     # ... and these above it
    see = torch.rand(TERMS_SEEN, F, generator=g) < min(0.9, 44.0 / F)
    see[torch.arange(12), src[:12] - lo] = True                                     # ii == jj inside the window / both ends outside
    see[8:12, F - 2:] = True
    p, f = torch.nonzero(see, as_tuple=True)                                        # patch-major
    if len(p) % 64 == 0:
        p, f = p[:-1], f[:-1]
    ii, jj, kk = src[p].contiguous(), (lo + f).contiguous(), slots[p].contiguous()
    E = len(ii)
    scale = torch.cat([torch.full((2,), 1.0), torch.full((2,), 1.0), torch.full((2,), 10.0), torch.full((24,), 100.0)])
    terms = torch.randn(E, 30, generator=g) * scale
    terms[:, 2:4] = 0.02 + 0.96 * torch.rand(E, 2, generator=g)
    zero_slot = int(slots[20])
    if zero_weight:
        terms[kk == zero_slot, 2:4] = 0.0
    inside = lambda x: (x >= t0) & (x < t0 + N)
    assert E % 64 != 0 and 60 <= E <= 3000 and bool((torch.bincount(kk, minlength=TERMS_NP) == 0).any())
    assert bool((~inside(ii) & ~inside(jj)).any()) and (N == 0 or bool(((ii == jj) & inside(ii)).any()))
    assert N == 0 or (bool((~inside(ii) & inside(jj)).any()) and bool((inside(ii) & ~inside(jj)).any()))
    assert t0 == 0 or bool(((ii < t0) | (jj < t0)).any())
    return dict(N=N, t0=t0, ep=ep, lmbda=1e-4, Np=TERMS_NP, E=E, terms=terms, ii=ii, jj=jj, kk=kk, shuffle=torch.randperm(E, generator=g),
                g_dX=torch.randn(6 * N, generator=g), g_dZ=torch.randn(TERMS_NP, generator=g), zero_rows=(kk == zero_slot) if zero_weight else None)


def solve_with_gradient(c, dt):
    """solve_from_terms and its adjoint for the case's cotangents, on the CPU in `dt` -> (dX, dZ, g_terms)"""
    t = c["terms"].detach().to(dt, copy=True).requires_grad_(True)
    dX, dZ = solve_from_terms(t, c["lmbda"], c["ii"], c["jj"], c["kk"], c["Np"], c["t0"], c["N"], c["ep"])
    g, = torch.autograd.grad((dX * c["g_dX"].to(dt)).sum() + (dZ * c["g_dZ"].to(dt)).sum(), t)
    return dX.detach(), dZ.detach(), g


@functools.lru_cache(maxsize=None)
def terms_reference(N, t0=None, ep=None, zero_weight=False):
    """{fp64: (dX, dZ, g_terms), fp32: ...} of the case, cached"""
    c = terms_case(N, t0, ep, zero_weight)
    n = torch.get_num_threads()
    torch.set_num_threads(1)                                    # fp32 sums depend on torch's split among threads: the envelope must not
    try:
        return {dt: solve_with_gradient(c, dt) for dt in (torch.float64, torch.float32)}
    finally:
        torch.set_num_threads(n)


def terms_errors(got, ref, perm=None):
    """(dX, dZ, g_terms) against the reference's -> relative error of dX, dZ and of every column group of g_terms on its own scale (the groups'
    scales differ by orders of magnitude).  perm: `got` belongs to the edge list in this order."""
    g = got[2].detach().cpu().double()
    if perm is not None:
        g = torch.empty_like(g).index_copy_(0, perm, g)
    e = {"dX": rel_err(got[0], ref[0]) if ref[0].numel() else 0.0, "dZ": rel_err(got[1], ref[1])}
    e.update({"g_" + name: rel_err(g[:, sl], ref[2][:, sl]) if float(ref[2][:, sl].abs().max()) > 0 else float(g[:, sl].abs().max()) for name, sl in GROUPS})
    return e
