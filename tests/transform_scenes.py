"""Scenes and fp64 references for the fused reprojection (csrc/transform.hip: k_transform, k_transform_vjp, k_reproject), the
yardstick of tests/test_gpu_transform.py: test infrastructure, everything here runs on the CPU.

edge_scene(P, seed) puts pixels in every regime of devo/projective_ops.py:32-105 at once (the Z < 0.1 clamp of proj, the |Z| > 0.2 gate of
the Jacobians, centres behind the camera) and frames on both sides of the adjoint's 128-frame LDS table; interior_scene(P, seed) has the
same frames, intrinsics and graph with every Z > 0.3, so that per-row errors mean something.  Every frame has its own intrinsics with
fx != fy and cx != cy.  The conditions are asserted here on the fp64 oracle's Z (regimes()), for every scene that is built.

reference(kind, P) and gradients(kind, P, mode) run oracle/pops.py once per scene in fp64 and once in fp32 (the envelope of an
ill-conditioned row: tests/test_gpu_fastba.py:check) and are cached; nobody may write into what they return."""
import functools
import torch
from oracle import pops
from oracle.lie import SE3 as OSE3
from devo_amd import synth
from util import row_rel_err

NBUF = 140                                        # pose / intrinsics slots
SLOTS = (0, 1, 2, 3, 127, 128, 129, 139)          # the eight used frames: both sides of the adjoint's LDS table (128 frames)
M = 6                                             # patches per frame: 48 patches with edges, 8 * 8 * 6 = 384 edges
N_EDGELESS = 3                                    # patches behind them that no edge names
H, W = 60, 80
BASE_K = (40.0, 37.0, 41.0, 29.0)
SEED = 12                                         # the seed of every GPU test (tests/test_transform_scenes_cpu.py checks the conditions for it)
MODES = ("coords", "depth", "Jj", "all")          # cotangents of the adjoint tests


def _scene(P, seed, push):
    n = len(SLOTS)
    slots = torch.tensor(SLOTS)
    g = torch.Generator().manual_seed(1000 + int(seed))
    p8 = synth.make_poses(n, seed)[0]
    if push:
        p8[2, 2] -= 3.0                                                   # one camera 3 units back: its points come close to / behind the others
    p8[1::2, 3:] *= 1.7                                                   # the kernels renormalise on load, as lietorch does (so3.h:31-37)
    poses = torch.zeros(1, NBUF, 7)
    poses[..., 6] = 1.0
    poses[0, slots] = p8
    k = torch.arange(n, dtype=torch.float32)[:, None] - 3.5               # per frame a few per cent, another sign and size per component
    K8 = torch.tensor(BASE_K) * (1.0 + 0.01 * k * torch.tensor([1.0, -0.8, -1.3, 0.6]))
    intrinsics = torch.tensor(BASE_K).expand(1, NBUF, 4).contiguous()
    intrinsics[0, slots] = K8
    patches, _ = synth.make_patches(n, M, H, W, P=P, seed=seed)
    extra = patches[:, :N_EDGELESS].clone()
    extra[:, :, :2] += 2.0
    patches = torch.cat([patches, extra], 1)
    if push:
        patches[0, ::5, 2] = 40.0                                         # every fifth patch 1/40 in front of its camera
    patches[0, :, 2] *= 1.0 + 0.03 * (2.0 * torch.rand(patches.shape[1], P, P, generator=g) - 1.0)      # inverse depth differs per pixel
    i8, j8, kk = synth.full_graph(n, M)
    return poses, patches.contiguous(), intrinsics, slots[i8], slots[j8], kk


def oracle_z(scene):
    """Z of every pixel after the transform, fp64 (projective_ops.py:57-66) -> [E, P, P]"""
    poses, patches, intrinsics, ii, jj, kk = scene
    G = OSE3(poses.double())
    Gij = G[:, jj] * G[:, ii].inv()
    X1 = Gij[:, :, None, None] * pops.iproj(patches.double()[:, kk], intrinsics.double()[:, ii])
    return X1[0, ..., 2]


def regimes(scene):
    """how many pixels / centres of the scene lie in each regime of the kernels, and how close any comes to a threshold"""
    Z = oracle_z(scene)
    c = Z.shape[-1] // 2
    Zc = Z[:, c, c]
    return dict(pixels_clamped=int((Z < 0.1).sum()), centres_01_02=int(((Zc > 0.1) & (Zc < 0.2)).sum()),
                centres_m02_01=int(((Zc > -0.2) & (Zc < 0.1)).sum()), centres_behind=int((Zc < -0.2).sum()),
                centres_far=int((Zc > 0.3).sum()), z_min=float(Z.min()),
                clamp_margin=float((Z - 0.1).abs().min()), gate_margin=float((Zc.abs() - 0.2).abs().min()))


def assert_edge_conditions(r):
    assert r["pixels_clamped"] >= 20 and r["centres_01_02"] >= 3 and r["centres_m02_01"] >= 3, r
    assert r["centres_behind"] >= 20 and r["centres_far"] >= 100, r
    assert r["clamp_margin"] >= 1e-3 and r["gate_margin"] >= 1e-3, r      # fp32 moves Z by 1e-6 of itself: the kernel takes the oracle's side


def assert_graph_conditions(scene):
    poses, patches, intrinsics, ii, jj, kk = scene
    K = intrinsics[0, list(SLOTS)]
    assert poses.shape == (1, NBUF, 7) and intrinsics.shape == (1, NBUF, 4) and len(ii) == len(SLOTS) ** 2 * M
    assert bool((K[:, 0] != K[:, 1]).all()) and bool((K[:, 2] != K[:, 3]).all()) and len(torch.unique(K, dim=0)) == len(SLOTS)
    assert bool((ii == jj).any()) and int(torch.bincount(kk).max()) >= len(SLOTS) and int(kk.max()) + N_EDGELESS == patches.shape[1] - 1
    lo, hi = ii < 128, jj < 128
    assert bool((lo & hi).any()) and bool((~lo & ~hi).any()) and bool((lo & ~hi).any()) and bool((~lo & hi).any())
    q = poses[0, list(SLOTS), 3:].norm(dim=-1)
    assert int((q > 1.5).sum()) == len(SLOTS) // 2
    d = patches[0, :, 2].reshape(patches.shape[1], -1)
    assert patches.shape[-1] == 1 or bool((d.std(dim=1) > 0).all())


@functools.lru_cache(maxsize=None)
def edge_scene(P, seed=SEED):
    s = _scene(P, seed, True)
    assert_graph_conditions(s)
    assert_edge_conditions(regimes(s))
    return s


@functools.lru_cache(maxsize=None)
def interior_scene(P, seed=SEED):
    s = _scene(P, seed, False)
    assert_graph_conditions(s)
    assert regimes(s)["z_min"] > 0.3
    return s


def scene(kind, P, seed=SEED):
    return {"edge": edge_scene, "interior": interior_scene}[kind](P, seed)


def _oracle(s, dtype, **kw):
    poses, patches, intrinsics, ii, jj, kk = s
    return pops.transform(OSE3(poses.to(dtype)), patches.to(dtype), intrinsics.to(dtype), ii, jj, kk, **kw)


@functools.lru_cache(maxsize=None)
def reference(kind, P, seed=SEED):
    """the oracle's outputs for the scene -> {dtype: dict(coords, valid, Ji, Jj, Jz, depth, tonly)}"""
    s = scene(kind, P, seed)
    out = {}
    with torch.no_grad():
        for dtype in (torch.float64, torch.float32):
            c, v, (Ji, Jj, Jz) = _oracle(s, dtype, jacobian=True)
            out[dtype] = dict(coords=c, valid=v, Ji=Ji, Jj=Jj, Jz=Jz, depth=_oracle(s, dtype, depth=True), tonly=_oracle(s, dtype, tonly=True))
    return out


def cotangents(E, P, mode, seed=5):
    """fixed seeded cotangents (coords [1,E,P,P,2|3], Ji, Jj, Jz; None where the mode has none), fp32"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    gc, gi, gj, gz = r(1, E, P, P, 3), r(1, E, 2, 6), r(1, E, 2, 6), r(1, E, 2, 1)
    if mode == "coords":
        return gc[..., :2].contiguous(), None, None, None
    if mode == "depth":
        return gc, None, None, None
    if mode == "Jj":
        return None, None, gj, None
    assert mode == "all"
    return gc[..., :2].contiguous(), gi, gj, gz


def oracle_gradients(s, cot, dtype, depth=False, edges=None):
    """d <cotangent, outputs> / d (poses, patches) by the oracle's autograd (lietorch's 6-of-7 convention for the poses)"""
    poses, patches, intrinsics, ii, jj, kk = s
    e = slice(None) if edges is None else edges
    pos = poses.detach().to(dtype, copy=True).requires_grad_(True)
    pat = patches.detach().to(dtype, copy=True).requires_grad_(True)
    gc, gi, gj, gz = cot
    jac = gj is not None
    out = pops.transform(OSE3(pos), pat, intrinsics.to(dtype), ii[e], jj[e], kk[e], depth=depth, jacobian=jac)
    outs = (out[0], *out[2]) if jac else (out,)
    loss = sum((o * w[:, e].to(dtype)).sum() for o, w in zip(outs, (gc, gi, gj, gz)) if w is not None)
    loss.backward()
    return pos.grad.detach(), pat.grad.detach()


def oracle_edge_terms(s, cot, dtype=torch.float64):
    """what every edge adds to the pose gradient, by the oracle's autograd -> (to poses[ii] [E,6], to poses[jj] [E,6], to patches[kk] like
    patches[kk]): Gij of edge e stands alone in slot E + e of a pose buffer whose slot e is the identity, so the gradient of slot E + e is
    the edge's term for frame j and that of slot e (through Mul and Inv, lietorch_gpu.cu:85-125) its term for frame i."""
    poses, patches, intrinsics, ii, jj, kk = s
    E = len(ii)
    G = OSE3(poses.to(dtype))
    Gij = (G[:, jj] * G[:, ii].inv()).data[0]
    eye = torch.zeros(E, 7, dtype=dtype)
    eye[:, 6] = 1.0
    buf = torch.cat([eye, Gij])[None].clone().requires_grad_(True)
    pat = patches.to(dtype)[:, kk].clone().requires_grad_(True)
    K = torch.cat([intrinsics[0, ii], intrinsics[0, jj]])[None].to(dtype)
    a = torch.arange(E)
    gc, gi, gj, gz = cot
    jac = gj is not None
    out = pops.transform(OSE3(buf), pat, K, a, a + E, a, jacobian=jac)
    outs = (out[0], *out[2]) if jac else (out,)
    sum((o * w.to(dtype)).sum() for o, w in zip(outs, (gc, gi, gj, gz)) if w is not None).backward()
    return buf.grad[0, :E, :6].detach(), buf.grad[0, E:, :6].detach(), pat.grad[0].detach()


@functools.lru_cache(maxsize=None)
def gradients(kind, P, mode, seed=SEED):
    s = scene(kind, P, seed)
    cot = cotangents(len(s[3]), P, mode)
    return {dtype: oracle_gradients(s, cot, dtype, depth=(mode == "depth")) for dtype in (torch.float64, torch.float32)}


def compare(what, got, ref64, tol, ref32=None, rows=None):
    """tests/util.py:row_rel_err per row against `tol`; with ref32 (the oracle in fp32 on the same inputs) a row's bound is the larger of
    tol and twice the oracle's own fp32 error, the rule of tests/test_gpu_fastba.py:check.  `rows`: compare these rows of the [rows, width]
    view among themselves (boolean mask).  Prints and returns the worst error over its bound."""
    got, ref64 = got.detach().double().cpu(), ref64.double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    err = row_rel_err(pick(got), pick(ref64))
    bound = torch.full_like(err, tol)
    if ref32 is not None:
        bound = torch.maximum(bound, 2.0 * row_rel_err(pick(ref32.double()), pick(ref64)))
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"{what}: worst per-row relative error {float(err.max()) if err.numel() else 0.0:.3e}, worst error / bound {worst:.3f} (tol {tol:.0e})")
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.2f} (tol {tol:.1e}, per-row relative error {float(err.max()):.3e})"
    return worst
