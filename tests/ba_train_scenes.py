"""Scenes for the whole differentiable Gauss-Newton step (tests/test_gpu_ba_train_kernels.py, part D) and the conditions they have to
meet: test infrastructure, everything here runs on the CPU.  scene(n_opt, fixedp) is a devo_amd.synth trajectory of n_opt + fixedp frames
with a randomly thinned and shuffled full graph; a few patches and edges are placed so that every gate of devo/ba.py:98-106 and both ends
of the depth clamp (:175-176) are exercised.  conditions() measures that on the fp64 oracle and assert_conditions() asserts it, with the
margins that keep an fp32 evaluation on the oracle's side of every threshold.  Results are cached; nobody may write into them."""
import contextlib
import functools
import torch
from devo_amd import synth
from oracle import pops
from oracle.lie import SE3 as OSE3
import ba_terms_ref as R
from util import rel_err, row_rel_err

H, W = 120, 160
BOUNDS = (2.5, 2.5, W + 31.5, H + 31.5)           # patch centres are integers in [1, W - 2] x [1, H - 2]: one is placed outside
EP, LMBDA = 10.0, 1e-4
N_OPT = (1, 8, 9, 16, 17, 22, 32)                 # both sides of every kernel switch: <8> | <11>, <16> | general, chain | k_ba_solve, the limit
FIXEDP = (1, 3)
STRUCTURE_ONLY = (9, 1)                           # (n_opt, fixedp) of the structure-only step
CHAINED = (17, 22)                                # two chained steps at these sizes
SEED = 31
SEEDS = {(8, 1): 36, (9, 3): 32, (16, 1): 35, (17, 1): 35, (22, 1): 39, (32, 1): 32}      # where SEED's scene is not admitted (assert_conditions, assert_margin)
MIN_C = 1.0                                       # every patch with an ungated edge has at least this curvature (lambda = 1e-4)


def motion(n):
    """(trans_step, rot_step) of synth.make_poses per trajectory length: the defaults drift out of frame on long trajectories"""
    return min(0.05, 0.3 / n), min(0.01, 0.06 / n)


@functools.lru_cache(maxsize=None)
def scene(n_opt, fixedp, seed=None):
    n = n_opt + fixedp
    seed = SEEDS.get((n_opt, fixedp), SEED) if seed is None else seed
    M = 6 if n <= 12 else 4 if n <= 24 else 3
    dt = torch.float64
    g = torch.Generator().manual_seed(7000 + 100 * n + seed)
    poses = synth.make_poses(n, seed + n, *motion(n))
    back, d0 = (0.4, 4.0) if n > 2 else (0.05, 20.0)                         # (two frames: every placed patch sees the last camera, so it stays close)
    poses[0, n - 1, 0] += 0.05 if n == 2 else 0.0                           # (... and gets a baseline)
    poses[0, n - 1, 2] = -back                                             # the last camera stands back: the nearest point falls behind it
    patches, _ = synth.make_patches(n, M, H, W, seed=seed + n)
    intr = synth.make_intrinsics(n, H, W)
    # placed patches: ids 0 .. 3 (frame 0) and the first two of frame n - 1
    last = (n - 1) * M
    patches[0, 0, 2] = d0                                                  # close in front of frame 0: invalid in the last frame
    patches[0, 1, 0] = torch.tensor([0.0, 1.0, 2.0]).expand(3, 3)          # centre (1, 1): outside the bounds in its own frame
    patches[0, 1, 1] = torch.tensor([0.0, 1.0, 2.0])[:, None].expand(3, 3)
    low, high = torch.tensor([2, last]), torch.tensor([3, last + 1])
    patches[0, low, 2] = 0.002                                             # far points whose targets ask for a step of -0.5: clamp at 1e-3
    patches[0, high, 2] = 9.9                                              # near points whose targets ask for a step of +2: clamp at 10
    placed = torch.zeros(n * M, dtype=torch.bool)
    placed[torch.cat([torch.arange(4), low, high])] = True
    ii, jj, kk = synth.full_graph(n, M)
    keep = (torch.rand(len(ii), generator=g) < (0.9 if n <= 4 else 0.6)) | placed[kk]
    near = (kk == 0) | (kk == 3) | (kk == last + 1)                        # the near ones only see the frames around their own: bounded parallax
    keep &= ~near | ((ii - jj).abs() <= max(1, n // 8))
    keep[(ii == 0) & (jj == n - 1) | (ii == n - 1) & (jj == 0)] = True     # the graph keeps its first and last frame (and patch 0 the last camera)
    order = torch.nonzero(keep)[:, 0]
    order = order[torch.randperm(len(order), generator=g)]
    ii, jj, kk = ii[order], jj[order], kk[order]
    E = len(ii)
    with torch.no_grad():
        c0, ok, (_, _, Jz) = pops.transform(OSE3(poses.to(dt)), patches.to(dt), intr.to(dt), ii, jj, kk, jacobian=True)
    ask = torch.zeros(n * M, dtype=dt)
    ask[low], ask[high] = -0.5, 2.0
    target = c0[0, :, 1, 1] + Jz[0, :, :, 0] * ask[kk][:, None] + torch.randn(E, 2, generator=g, dtype=dt)
    plain = ~placed[kk] & (ii != jj) & (ok[0] > 0)
    far = torch.nonzero(plain)[:2, 0] if n > 2 else torch.nonzero(~placed[kk] & (ii == jj))[:1, 0]     # (two frames: an edge that carries no depth information)
    target[far] += torch.tensor([260.0, 150.0], dtype=dt)                  # the residual gate: 300 px
    weight = torch.rand(1, E, 2, generator=g)
    lw = torch.randn(1, E, 3, 3, 2, generator=g)                           # the loss weights of tests/test_gpu_training.py's loss
    target = target.float()[None].contiguous()
    # Edges within 0.05 px of a gate threshold go (an fp32 evaluation may decide them differently; conditions() asserts the margin afterwards).
    # So do the edges of a patch that only its own frame, or frames almost without parallax, observe; it becomes a slot without an edge.  Its
    # C = sum w Jz^2 is rounding noise against lambda = 1e-4, and its depth step Q (u - E^T dX), Q = 1 / (C + lambda) ~ 1e4, is noise in ANY fp32
    # evaluation.  Measured on the 17-frame scene before the filter: a patch left with its own frame's edge alone has C = 6.8e-31 in fp64 (Jz = 0 up
    # to rounding) and 1e-14 in fp32; oracle.pops.BA in fp32 then misses that patch's depth by 1.1e-2 and d loss / d weight by 6.7e-2 of the
    # tensor's scale, against 2.0e-5 and 1.6e-4 without it — no fp32 bound could hold.  The regime Q = 1 / lambda itself is covered exactly
    # where it is well defined: a patch whose edges all carry w = 0 (C = 0), per row, in the solve_terms tests.
    e = _margins(c0[0, :, 1, 1], target[0].to(dt)) >= 0.05
    C = _curvature(poses, patches, intr, target[:, e], weight[:, e], ii[e], jj[e], kk[e])
    e &= ~((C > 0) & (C < MIN_C))[kk]
    if int(e.sum()) % 64 == 0:
        e[int(torch.nonzero(e & plain)[-1])] = False
    ii, jj, kk, target, weight, lw = ii[e].contiguous(), jj[e].contiguous(), kk[e].contiguous(), target[:, e].contiguous(), weight[:, e].contiguous(), lw[:, e].contiguous()
    return dict(poses=poses, patches=patches.contiguous(), intr=intr, target=target, weight=weight, ii=ii, jj=jj, kk=kk,
                bounds=BOUNDS, fixedp=fixedp, n_opt=n_opt, n=n, lw=lw)


def _margins(ctr, target):
    """distance of every edge from the nearest gate threshold, in pixels -> [E]"""
    b = BOUNDS
    edge = torch.stack([ctr[:, 0] - b[0], ctr[:, 1] - b[1], b[2] - ctr[:, 0], b[3] - ctr[:, 1]], -1).abs().amin(-1)
    return torch.minimum(((target - ctr).norm(dim=-1) - 250).abs(), edge)


def _curvature(poses, patches, intr, target, weight, ii, jj, kk):
    """C = sum over a patch's edges of w Jz^2 (devo/ba.py:147) on the fp64 oracle -> [Np]"""
    dt = torch.float64
    with torch.no_grad():
        coords, ok, (Ji, Jj, Jz) = pops.transform(OSE3(poses.to(dt)), patches.to(dt), intr.to(dt), ii, jj, kk, jacobian=True)
        t, _ = R.edge_terms_ref(coords, ok, Ji, Jj, Jz, target.to(dt), weight.to(dt), BOUNDS)
    return torch.zeros(patches.shape[1], dtype=dt).index_add(0, kk, (t[:, 2:4] * t[:, 4:6] ** 2).sum(-1))


def conditions(s, poses=None, patches=None, structure_only=False):
    """the gates and the clamp of one step on the fp64 oracle's numbers (optionally from other poses / patches: the second chained step)"""
    dt = torch.float64
    poses = s["poses"].to(dt) if poses is None else poses.to(dt)
    patches = s["patches"].to(dt) if patches is None else patches.to(dt)
    ii, jj, kk = s["ii"], s["jj"], s["kk"]
    with torch.no_grad():
        G = OSE3(poses)
        X1 = (G[:, jj] * G[:, ii].inv())[:, :, None, None] * pops.iproj(patches[:, kk], s["intr"].to(dt)[:, ii])
        Z = X1[0, :, 1, 1, 2]
        coords, ok, (Ji, Jj, Jz) = pops.transform(G, patches, s["intr"].to(dt), ii, jj, kk, jacobian=True)
        ctr = coords[0, :, 1, 1]
        res = (s["target"].to(dt)[0] - ctr).norm(dim=-1)
        b = s["bounds"]
        edge = torch.stack([ctr[:, 0] - b[0], ctr[:, 1] - b[1], b[2] - ctr[:, 0], b[3] - ctr[:, 1]], -1)
        invalid, big, out = Z <= 0.2, res >= 250, (edge <= 0).any(-1)
        terms, gate = R.edge_terms_ref(coords, ok, Ji, Jj, Jz, s["target"].to(dt), s["weight"].to(dt), b)
        dX, dZ = R.solve_from_terms(terms, LMBDA, ii, jj, kk, patches.shape[1], s["fixedp"], 0 if structure_only else s["n_opt"], EP)
        d = patches[0, :, 2, 1, 1] + dZ
        C = torch.zeros(patches.shape[1], dtype=dt).index_add(0, kk, (terms[:, 2:4] * terms[:, 4:6] ** 2).sum(-1))
    return dict(E=len(ii), invalid=int(invalid.sum()), residual=int((big & ~invalid).sum()), outside=int((out & ~invalid).sum()),
                removed=int((gate == 0).sum()), gate_margin=float(torch.minimum((res - 250).abs().min(), edge.abs().min())),
                z_margin=float((Z - 0.2).abs().min()), clamp_low=int((d < 1e-3).sum()), clamp_high=int((d > 10).sum()),
                clamp_margin=float(torch.minimum((d - 1e-3).abs().min(), (d - 10).abs().min())), max_frame=int(max(ii.max(), jj.max())),
                min_curvature=float(C[C > 0].min()), edgeless=int((torch.bincount(kk, minlength=patches.shape[1]) == 0).sum()))


def assert_conditions(c, n, first=True):
    if first:                                     # what the scene was built to contain
        assert c["invalid"] >= 1 and c["residual"] >= 1 and c["outside"] >= 1, c
        assert c["clamp_low"] >= 1 and c["clamp_high"] >= 1, c
        assert c["max_frame"] == n - 1 and c["E"] % 64 != 0, c
        assert c["min_curvature"] >= MIN_C, c
    assert 4 * c["removed"] <= c["E"], c
    assert c["gate_margin"] >= 1e-2 and c["z_margin"] >= 1e-3 and c["clamp_margin"] >= 1e-4, c


def loss_of(transform, G, P, s, dt):
    """the loss of test_fused_solve_matches_the_torch_composition_in_value_and_gradient; G: an SE3 of the transform's own kind"""
    dev = P.device
    cf = transform(G, P, s["intr"].to(dev, dt), s["ii"].to(dev), s["jj"].to(dev), s["kk"].to(dev))
    return (cf * s["lw"].to(dev, dt)).sum() + (G.log() ** 2).sum() + (P[:, :, 2] ** 2).sum()


@contextlib.contextmanager
def one_thread():
    """fp32 sums on the CPU depend on how torch splits them among its threads: every reference evaluation runs on one, so that the envelope
    (and with it the pass / fail line) does not depend on the machine's core count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def composed_step(G, P, intr, tgt, wgt, lm, ii, jj, kk, bounds, ep, fixedp, structure_only):
    """oracle.pops.BA's step as tests/ba_terms_ref.py composes it (dense, another summation order)"""
    p, q = R.whole_step(pops.transform, G.data, P, intr, tgt, wgt, lm, ii, jj, kk, bounds, ep, fixedp, structure_only)
    return OSE3(p), q


def oracle_step(s, dt, steps=1, structure_only=False, step=pops.BA):
    """`steps` chained steps of oracle.pops.BA (or another step function of its signature) on the CPU in `dt` ->
    dict(poses, patches, g_target, g_weight, g_poses, g_patches, stages): stages = the (poses, patches) entering every step"""
    tgt = s["target"].detach().to(dt, copy=True).requires_grad_(True)
    wgt = s["weight"].detach().to(dt, copy=True).requires_grad_(True)
    pos = s["poses"].detach().to(dt, copy=True).requires_grad_(True)
    pat = s["patches"].detach().to(dt, copy=True).requires_grad_(True)
    G, P, stages = OSE3(pos), pat, []
    for _ in range(steps):
        stages.append((G.data.detach(), P.detach()))
        G, P = step(G, P, s["intr"].to(dt), tgt, wgt, LMBDA, s["ii"], s["jj"], s["kk"], s["bounds"], ep=EP, fixedp=s["fixedp"],
                    structure_only=structure_only)
    loss_of(pops.transform, G, P, s, dt).backward()
    return dict(poses=G.data.detach(), patches=P.detach(), g_target=tgt.grad, g_weight=wgt.grad, g_poses=pos.grad, g_patches=pat.grad, stages=stages)


@functools.lru_cache(maxsize=None)
def reference(n_opt, fixedp, steps=1, structure_only=False):
    """{fp64: ..., fp32: ...} of oracle_step for scene(n_opt, fixedp), cached"""
    s = scene(n_opt, fixedp)
    with one_thread():
        return {dt: oracle_step(s, dt, steps, structure_only) for dt in (torch.float64, torch.float32)}


@functools.lru_cache(maxsize=None)
def second_opinion(n_opt, fixedp, steps=1, structure_only=False):
    """the fp32 error of the SAME step with another summation order (composed_step, one thread): a second sample of the rounding noise"""
    with one_thread():
        return errors(oracle_step(scene(n_opt, fixedp), torch.float32, steps, structure_only, step=composed_step), reference(n_opt, fixedp, steps, structure_only)[torch.float64])


VALUES, GRADIENTS = ("translation", "quaternion", "inverse depth"), ("g_target", "g_weight", "g_poses", "g_patches")
FLOOR = dict.fromkeys(VALUES, 1e-4) | dict.fromkeys(GRADIENTS, 2e-3)      # the project's figures (tests/test_gpu_training.py)
LIMIT = dict.fromkeys(VALUES, 5e-5) | dict.fromkeys(GRADIENTS, 1e-2)      # what the reference's own fp32 evaluation may be off by


def errors(got, ref):
    """got, ref: dicts of oracle_step's kind -> per tensor: the worst per-row relative error of the translations, the quaternions and the inverse
    depths (util.row_rel_err), the relative error of every gradient (util.rel_err)"""
    P = got["patches"].shape[-1] // 2
    e = dict(zip(VALUES, (float(row_rel_err(got["poses"][0, :, :3], ref["poses"][0, :, :3]).max()),
                          float(row_rel_err(got["poses"][0, :, 3:], ref["poses"][0, :, 3:]).max()),
                          float(row_rel_err(got["patches"][0, :, 2, P, P], ref["patches"][0, :, 2, P, P]).max()))))
    e.update({k: rel_err(got[k], ref[k]) for k in GRADIENTS})
    return e


def envelope(ref):
    """the reference's own fp32 error: reference()'s fp32 result against its fp64 result"""
    return errors(ref[torch.float32], ref[torch.float64])


def assert_envelope(e):
    for k, v in e.items():
        assert v <= LIMIT[k], f"{k}: oracle.pops.BA in fp32 is {v:.1e} from fp64 (> {LIMIT[k]:.0e}): the scene is too ill-conditioned"


def assert_margin(*samples):
    """Admission of a scene, decided on the CPU from the reference alone: every fp32 evaluation of the reference (oracle.pops.BA and the dense
    composition) is within HALF the floor of fp64.  The bound max(floor, 2 x e_ref32) is then the floor itself and leaves a factor 2 over the
    rounding noise that the algorithm shows in fp32 in ANY summation order; a scene that is noisier sits on its bound and is replaced (SEEDS)."""
    for e in samples:
        for k, v in e.items():
            assert v <= 0.5 * FLOOR[k], f"{k}: an fp32 evaluation of the reference is {v:.1e} from fp64 (> {0.5 * FLOOR[k]:.0e}): no margin, replace the scene"


def bounds_of(e):
    """per tensor: max(floor, 2 x the reference's own fp32 error)"""
    return {k: max(FLOOR[k], 2.0 * v) for k, v in e.items()}
