"""The fused reprojection (csrc/transform.hip: k_transform, its adjoint k_transform_vjp, k_reproject) against the fp64 oracle
(oracle/pops.py over oracle/lie.py; gradients by its autograd) on the scenes of tests/transform_scenes.py: per-frame intrinsics with
fx != fy, frames on both sides of the adjoint's 128-frame LDS table, P = 1, 3, 5, pixels in every regime of the Z clamp and of the
Jacobians' gate, the grid-stride loops, one edge, one edge past a workgroup, no edge.

Tolerances are the project's (tests/test_gpu_fastba.py, tests/test_gpu_training.py): 1e-5 coordinates, 1e-4 Jacobians and flow magnitude,
2e-4 gradients, validity bit-equal; per row (tests/util.py:row_rel_err).  On the edge scenes a row's bound is the larger of the tolerance
and twice the error of the oracle itself in fp32 on the same inputs (tests/test_gpu_fastba.py:check).  Every comparison prints its
worst error over its bound."""
import pytest
import torch
import transform_scenes as T
from oracle import fastba as F
from oracle import pops as opops
from oracle.lie import SE3 as OSE3

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("interior", "edge")
PS = (1, 3, 5)
F64, F32 = torch.float64, torch.float32
E_FWD = 4096 * 64 + 77            # one more pass than the forward's largest grid (devo_transform: 4096 workgroups of 64)
E_VJP = 8192 * 128 + 77           # and than the adjoint's (devo_transform_vjp: 8192 workgroups of 128)


def dev(s):
    return tuple(t.to(DEV) for t in s)


def envelope(kind, ref, key):
    return ref[F32][key] if kind == "edge" else None


def used_masks():
    used = torch.zeros(T.NBUF, dtype=torch.bool)
    used[list(T.SLOTS)] = True
    lo = used & (torch.arange(T.NBUF) < 128)
    return used, lo, used & ~lo


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("kind", KINDS)
def test_coordinates_and_validity_match_the_oracle(kind, P):
    from devo_amd.backends import cuda_ba
    s, ref = T.scene(kind, P), T.reference(kind, P)
    d = dev(s)
    far = (T.oracle_z(s) > 0.3).reshape(-1)                              # the pixels whose coordinates stay at image scale
    short = cuda_ba.transform(*d)                                        # coordinates only: the compiled binding's short form
    short2 = cuda_ba.transform(*d, layout="2pp")
    c, v = cuda_ba.transform(*d, valid=True)                             # the C ABI
    c2, v2 = cuda_ba.transform(*d, valid=True, layout="2pp")
    assert short.shape == (1, 384, P, P, 2) and short2.shape == (1, 384, 2, P, P) and v.shape == (1, 384)
    assert torch.equal(short2, short.permute(0, 1, 4, 2, 3).contiguous())            # devo.py:223
    assert torch.equal(c2, c.permute(0, 1, 4, 2, 3).contiguous())
    assert torch.equal(c, short) and torch.equal(v2, v)
    assert torch.equal(v.cpu().double(), ref[F64]["valid"])
    got = dict(coords=c, depth=cuda_ba.transform(*d, depth=True), tonly=cuda_ba.transform(*d, tonly=True))
    assert torch.equal(got["depth"][..., :2], c)
    for key, x in got.items():
        w = x.shape[-1]
        env = envelope(kind, ref, key)
        T.compare(f"{kind} P={P} {key}", x.reshape(-1, w), ref[F64][key].reshape(-1, w), 1e-5, None if env is None else env.reshape(-1, w))
        if kind == "edge" and key != "tonly":
            T.compare(f"{kind} P={P} {key}, Z > 0.3", x.reshape(-1, w), ref[F64][key].reshape(-1, w), 1e-5, env.reshape(-1, w), rows=far)


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("kind", KINDS)
def test_jacobians_match_the_oracle_per_edge(kind, P):
    from devo_amd.backends import cuda_ba
    s, ref = T.scene(kind, P), T.reference(kind, P)
    Zc = T.oracle_z(s)[:, P // 2, P // 2]
    gated, behind, far = Zc.abs() <= 0.2, Zc < -0.2, Zc > 0.3
    if kind == "edge":
        assert int(gated.sum()) >= 6 and int(behind.sum()) >= 20
    c, v, J = cuda_ba.transform(*dev(s), jacobian=True)
    assert torch.equal(c, cuda_ba.transform(*dev(s))) and torch.equal(v.cpu().double(), ref[F64]["valid"])
    assert float(v.cpu()[0, behind].abs().max() if bool(behind.any()) else 0.0) == 0.0
    for key, x in zip(("Ji", "Jj", "Jz"), J):
        x, r64 = x.cpu().reshape(384, -1), ref[F64][key].reshape(384, -1)
        env = envelope(kind, ref, key)
        env = None if env is None else env.reshape(384, -1)
        T.compare(f"{kind} P={P} {key}", x, r64, 1e-4, env)
        if kind == "edge":
            T.compare(f"{kind} P={P} {key}, Z > 0.3", x, r64, 1e-4, env, rows=far)
        assert bool((r64[gated] == 0).all()) and bool((x[gated] == 0).all()), f"{key}: not zero where |Z| <= 0.2"
        assert bool((x[behind].abs().amax(dim=1) > 0).all()), f"{key}: zero behind the camera (Z < -0.2)"


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("kind", KINDS)
def test_public_transform_and_flow_mag(kind, P):
    from devo_amd import projective_ops as pops
    from devo_amd.lietorch import SE3
    s, ref = T.scene(kind, P), T.reference(kind, P)
    d = dev(s)
    args = (SE3(d[0]), *d[1:])
    with torch.no_grad():
        c0 = pops.transform(*args)                                       # the [1,E,P,P,2] view of the 2 x P x P layout
        c, v, J = pops.transform(*args, jacobian=True)
        cd, vd = pops.transform(*args, depth=True, valid=True)
        fm = pops.flow_mag(*args, beta=0.3)
    assert c0.shape == c.shape and torch.equal(c0.contiguous(), c) and torch.equal(cd[..., :2], c)
    assert torch.equal(v.cpu().double(), ref[F64]["valid"]) and torch.equal(vd, v)
    for key, x, tol in (("coords", c0, 1e-5), ("depth", cd, 1e-5), ("Ji", J[0], 1e-4), ("Jj", J[1], 1e-4), ("Jz", J[2], 1e-4)):
        w = x.shape[-1] if key in ("coords", "depth") else x[0, 0].numel()
        env = envelope(kind, ref, key)
        T.compare(f"{kind} P={P} projective_ops {key}", x.reshape(-1, w), ref[F64][key].reshape(-1, w), tol, None if env is None else env.reshape(-1, w))
    o = lambda dt: opops.flow_mag(OSE3(s[0].to(dt)), s[1].to(dt), s[2].to(dt), *s[3:], beta=0.3).reshape(-1)
    T.compare(f"{kind} P={P} flow_mag", fm.reshape(-1), o(F64), 1e-4, o(F32) if kind == "edge" else None)


@pytest.mark.parametrize("P", PS)
def test_reproject_reads_the_first_intrinsics_row(P):
    """cuda_ba.reproject (ba_cuda.cu:368-418) takes one intrinsics row for all frames, and no Z clamp: the oracle says so, the kernel must
    do the same on a scene whose other rows differ, and must not look at them."""
    from devo_amd.backends import cuda_ba
    s = T.interior_scene(P)
    d = dev(s)
    r = cuda_ba.reproject(*d)
    rows = lambda t: t.permute(0, 1, 3, 4, 2).reshape(-1, 2)
    assert r.shape == (1, 384, 2, P, P)
    T.compare(f"P={P} reproject", rows(r), rows(F.reproject(*s, dtype=F64)), 1e-5)
    other = d[2].clone()
    other[0, 1:] = torch.tensor([7.0, 9.0, 11.0, 13.0], device=DEV)
    assert torch.equal(cuda_ba.reproject(d[0], d[1], other, *d[3:]), r)
    e = torch.zeros(0, dtype=torch.long, device=DEV)
    assert cuda_ba.reproject(*d[:3], e, e, e).shape == (1, 0, 2, P, P)


def _poison(nbytes):
    """fill the caching allocator's free blocks: what a kernel leaves unwritten in a fresh output is then NaN, not an old result"""
    junk = [torch.full((nbytes // 4,), float("nan"), device=DEV) for _ in range(2)]
    del junk


def test_forward_grid_stride_repeats_the_small_call_bit_for_bit():
    from devo_amd.backends import cuda_ba
    poses, patches, intr, ii, jj, kk = dev(T.edge_scene(3))
    small, sv = cuda_ba.transform(poses, patches, intr, ii, jj, kk, valid=True)
    idx = torch.arange(E_FWD, device=DEV) % 384
    n, rem = divmod(E_FWD, 384)
    for abi in ("binding", "C"):
        _poison(E_FWD * 18 * 4)
        if abi == "binding":
            big, bv = cuda_ba.transform(poses, patches, intr, ii[idx], jj[idx], kk[idx]), None
        else:
            big, bv = cuda_ba.transform(poses, patches, intr, ii[idx], jj[idx], kk[idx], valid=True)
        assert big.shape == (1, E_FWD, 3, 3, 2)
        assert bool((big[0, :n * 384].view(n, 384, 3, 3, 2) == small).all()), abi
        assert torch.equal(big[0, n * 384:], small[0, :rem]), abi
        if bv is not None:
            assert bool((bv[0, :n * 384].view(n, 384) == sv).all()) and torch.equal(bv[0, n * 384:], sv[0, :rem])


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("E", [0, 1, 65])
def test_small_and_empty_edge_lists(E, P):
    from devo_amd.backends import cuda_ba
    poses, patches, intr, ii, jj, kk = dev(T.edge_scene(P))
    full_c, full_v, full_J = cuda_ba.transform(poses, patches, intr, ii, jj, kk, jacobian=True)
    full_d = cuda_ba.transform(poses, patches, intr, ii, jj, kk, depth=True)
    a = (poses, patches, intr, ii[:E], jj[:E], kk[:E])
    c, v, J = cuda_ba.transform(*a, jacobian=True)
    assert c.shape == (1, E, P, P, 2) and v.shape == (1, E) and J[0].shape == (1, E, 2, 6) and J[1].shape == (1, E, 2, 6) and J[2].shape == (1, E, 2, 1)
    assert torch.equal(c, full_c[:, :E]) and torch.equal(v, full_v[:, :E]) and all(torch.equal(x, y[:, :E]) for x, y in zip(J, full_J))
    assert torch.equal(cuda_ba.transform(*a), full_c[:, :E])
    assert torch.equal(cuda_ba.transform(*a, layout="2pp"), full_c[:, :E].permute(0, 1, 4, 2, 3).contiguous())
    assert torch.equal(cuda_ba.transform(*a, depth=True), full_d[:, :E])
    cv, vv = cuda_ba.transform(*a, valid=True, layout="2pp")
    assert cv.shape == (1, E, 2, P, P) and torch.equal(vv, full_v[:, :E])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- adjoint
def check_gradients(kind, what, gp, gq, ref, scale=None):
    """(d/d poses [1,Nbuf,7], d/d patches) against the oracle's {dtype: (d/d poses, d/d patches)}: exact zeros where nothing is connected,
    both sides of the 128-frame table non-zero, translation and rotation parts per frame and x / y / inverse depth per pixel within 2e-4."""
    used, lo, hi = used_masks()
    gp, gq = gp.detach().cpu(), gq.detach().cpu()
    p64, q64 = ref[F64]
    p32, q32 = ref[F32] if kind == "edge" else (None, None)
    assert gp.shape == (1, T.NBUF, 7) and gq.shape == q64.shape
    assert float(gp[..., 6].abs().max()) == 0.0                          # the 7th slot of a group gradient stays empty
    assert float(gp[0, ~used].abs().max()) == 0.0                        # identity poses that no edge names
    assert float(gq[0, -T.N_EDGELESS:].abs().max()) == 0.0               # patches that no edge names
    assert bool((gp[0, lo, :6].abs().amax(dim=1) > 0).all()), "no gradient for a frame < 128"
    assert bool((gp[0, hi, :6].abs().amax(dim=1) > 0).all()), "no gradient for a frame >= 128"
    for part, sl in (("translation", slice(0, 3)), ("rotation", slice(3, 6))):
        for side, rows in (("frames < 128", lo), ("frames >= 128", hi)):
            T.compare(f"{what} d/d {part}, {side}", gp[0, :, sl], p64[0, :, sl], 2e-4, None if p32 is None else p32[0, :, sl], rows=rows)
    for c, name in enumerate(("x", "y", "inverse depth")):
        T.compare(f"{what} d/d patch {name}", gq[0, :, c].reshape(-1), q64[0, :, c].reshape(-1), 2e-4, None if q32 is None else q32[0, :, c].reshape(-1))


def _to_dev(cot):
    return tuple(None if t is None else t.to(DEV) for t in cot)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_matches_the_oracles_autograd(kind, P, mode):
    from devo_amd.backends import cuda_ba
    from devo_amd import projective_ops as pops
    from devo_amd.lietorch import SE3
    s, ref = T.scene(kind, P), T.gradients(kind, P, mode)
    d = dev(s)
    gc, gi, gj, gz = _to_dev(T.cotangents(384, P, mode))
    depth, jac = mode == "depth", gj is not None
    gp, gq = cuda_ba.transform_vjp(*d, gc, (gi, gj, gz) if jac else None, depth=depth)
    check_gradients(kind, f"{kind} P={P} {mode}: transform_vjp", gp, gq, ref)
    pos, pat = d[0].clone().requires_grad_(True), d[1].clone().requires_grad_(True)
    out = pops.transform(SE3(pos), pat, *d[2:], depth=depth, jacobian=jac)
    outs = (out[0], *out[2]) if jac else (out,)
    assert "FusedTransform" in type(outs[0].grad_fn).__name__
    sum((o * w).sum() for o, w in zip(outs, (gc, gi, gj, gz)) if w is not None).backward()
    check_gradients(kind, f"{kind} P={P} {mode}: projective_ops.transform", pos.grad, pat.grad, ref)


def test_adjoint_clamped_pixel_has_no_gradient_through_z():
    """One edge, every pixel at 0.02 < Z < 0.08: Z.clamp(min=0.1) (projective_ops.py:43) cuts the derivative through Z, so the coordinates
    move with X and Y only.  Here Gij is a pure translation along z: neither its z component nor the inverse depth reaches X or Y."""
    from devo_amd.backends import cuda_ba
    P = 3
    poses = torch.tensor([[[0, 0, 0, 0, 0, 0, 1.0], [0, 0, -0.95, 0, 0, 0, 1.0]]])
    intr = torch.tensor([[[40.0, 37.0, 41.0, 29.0], [42.0, 35.0, 39.0, 31.0]]])
    off = torch.arange(P, dtype=torch.float32) - 1
    x, y = torch.broadcast_tensors(30.0 + off[None, :], 20.0 + off[:, None])
    w = 1.0 + 0.03 * torch.linspace(-1, 1, P * P).view(P, P)
    patches = torch.stack([x, y, w])[None, None].contiguous()
    ii, jj, kk = torch.tensor([0]), torch.tensor([1]), torch.tensor([0])
    s = (poses, patches, intr, ii, jj, kk)
    Z = T.oracle_z(s)
    assert float(Z.min()) > 0.01 and float(Z.max()) < 0.09
    cot = T.cotangents(1, P, "coords")
    p64, q64 = T.oracle_gradients(s, cot, F64)
    gp, gq = cuda_ba.transform_vjp(*dev(s), cot[0].to(DEV), None)
    gp, gq = gp.cpu(), gq.cpu()
    assert float(p64[0, :, 2].abs().max()) == 0.0 and float(q64[0, 0, 2].abs().max()) == 0.0
    assert float(gp[0, :, 2].abs().max()) == 0.0, "a gradient through Z below the clamp (pose translation z)"
    assert float(gq[0, 0, 2].abs().max()) == 0.0, "a gradient through Z below the clamp (inverse depth)"
    want = cot[0][0, 0] * (intr[0, 1, :2] / intr[0, 0, :2]) * 10.0      # u = fx_j (x - cx_i) / (0.1 fx_i) + cx_j
    assert float((gq[0, 0, :2].permute(1, 2, 0) - want).abs().max()) <= 2e-4 * float(want.abs().max())
    T.compare("clamped edge d/d poses", gp[0, :, :6], p64[0, :, :6], 2e-4)
    T.compare("clamped edge d/d patch x, y", gq[0, 0, :2].reshape(-1), q64[0, 0, :2].reshape(-1), 2e-4)


def test_adjoint_grid_stride_is_linear_in_the_edge_list():
    """The 384 edges and their cotangents tiled past the adjoint's largest grid: the gradient is the tile count times the 384-edge oracle
    gradient plus that of the remainder's edges.  Float atomics: the order of summation varies, so this is held to the gradient tolerance,
    not to bits — 2e-4 per row, or twice the error of the reference's own sum in fp32 where that is larger: every used frame collects 262 000
    terms in one float here and every patch pixel 21 800, the same 96 (8) over and over, and the oracle's per-edge terms added up in fp32 in
    the list's order are themselves 0.7e-4 ... 2.3e-4 of a row away from their fp64 sum."""
    from devo_amd.backends import cuda_ba
    P = 1
    s = T.interior_scene(P)
    cot = T.cotangents(384, P, "all")
    n, rem = divmod(E_VJP, 384)
    assert n == 2730 and rem == 333
    whole, part = T.gradients("interior", P, "all")[F64], T.oracle_gradients(s, cot, F64, edges=slice(0, rem))
    ti, tj, tq = T.oracle_edge_terms(s, cot)
    both = torch.zeros(1, T.NBUF, 7, dtype=F64)
    both[0, :, :6].index_add_(0, s[3], ti).index_add_(0, s[4], tj)
    assert float((both - whole[0]).abs().max()) <= 1e-9 * float(whole[0].abs().max())          # the terms are the oracle's gradient, edge by edge
    order = torch.arange(E_VJP) % 384
    p32, q32 = torch.zeros(1, T.NBUF, 7), torch.zeros(s[1].shape)
    p32[0, :, :6].index_add_(0, torch.stack([s[4][order], s[3][order]], 1).reshape(-1), torch.stack([tj.float()[order], ti.float()[order]], 1).reshape(-1, 6))
    q32[0].index_add_(0, s[5][order], tq.float()[order])
    ref = {F64: (n * whole[0] + part[0], n * whole[1] + part[1]), F32: (p32, q32)}
    idx = order.to(DEV)
    poses, patches, intr, ii, jj, kk = dev(s)
    gc, gi, gj, gz = (t[:, idx].contiguous() for t in _to_dev(cot))
    gp, gq = cuda_ba.transform_vjp(poses, patches, intr, ii[idx], jj[idx], kk[idx], gc, (gi, gj, gz))
    check_gradients("edge", f"P=1, {E_VJP} edges: transform_vjp", gp, gq, ref)


def test_seven_by_seven_patches_take_the_composition():
    """P * P > 25 is more than the adjoint kernel holds per thread: projective_ops.transform with gradients then runs the composition over the
    SE3 ops; values and gradients are the oracle's all the same."""
    from devo_amd import projective_ops as pops
    from devo_amd.lietorch import SE3
    P = 7
    s = T.interior_scene(P)
    d = dev(s)
    cot = T.cotangents(384, P, "all")
    ref = {F64: T.oracle_gradients(s, cot, F64)}
    r64 = opops.transform(OSE3(s[0].double()), s[1].double(), s[2].double(), *s[3:], jacobian=True)
    pos, pat = d[0].clone().requires_grad_(True), d[1].clone().requires_grad_(True)
    c, v, J = pops.transform(SE3(pos), pat, *d[2:], jacobian=True)
    assert "FusedTransform" not in type(c.grad_fn).__name__
    T.compare("P=7 coords", c.reshape(-1, 2), r64[0].reshape(-1, 2), 1e-5)
    assert torch.equal(v.detach().cpu().double(), r64[1])
    for name, x, r in zip(("Ji", "Jj", "Jz"), J, r64[2]):
        T.compare(f"P=7 {name}", x.reshape(384, -1), r.reshape(384, -1), 1e-4)
    sum((o * w.to(DEV)).sum() for o, w in zip((c, *J), cot)).backward()
    check_gradients("interior", "P=7 composition", pos.grad, pat.grad, ref)


@pytest.mark.parametrize("P", PS)
def test_adjoint_without_edges_is_zero(P):
    from devo_amd.backends import cuda_ba
    from devo_amd import projective_ops as pops
    from devo_amd.lietorch import SE3
    poses, patches, intr, ii, jj, kk = dev(T.edge_scene(P))
    e = ii[:0]
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    for g_c, g_J in ((z(1, 0, P, P, 2), None), (None, (None, z(1, 0, 2, 6), None)), (z(1, 0, P, P, 2), (z(1, 0, 2, 6), z(1, 0, 2, 6), z(1, 0, 2, 1)))):
        gp, gq = cuda_ba.transform_vjp(poses, patches, intr, e, e, e, g_c, g_J)
        assert gp.shape == poses.shape and gq.shape == patches.shape
        assert float(gp.abs().max()) == 0.0 and float(gq.abs().max()) == 0.0
    pos, pat = poses.clone().requires_grad_(True), patches.clone().requires_grad_(True)
    c, v, J = pops.transform(SE3(pos), pat, intr, e, e, e, jacobian=True)
    assert c.shape == (1, 0, P, P, 2) and v.shape == (1, 0) and J[2].shape == (1, 0, 2, 1)
    (c.sum() + J[0].sum() + J[1].sum() + J[2].sum()).backward()
    assert pos.grad.shape == poses.shape and pat.grad.shape == patches.shape
    assert float(pos.grad.abs().max()) == 0.0 and float(pat.grad.abs().max()) == 0.0
