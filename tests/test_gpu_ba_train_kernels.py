"""The three kernel pairs of the differentiable bundle adjustment (devo_amd/ba.py) against plain fp64 references, at the pose counts where
the kernels switch paths:

  A  devo_ba_solve_terms / _backward   against tests/ba_terms_ref.py:solve_from_terms on random terms, N in ba_terms_ref.TERMS_N
  B  devo_ba_edge_terms / _backward    against edge_terms_ref: bit-equal terms, the strict gate thresholds
  C  devo_ba_apply_step / _backward    against apply_step_ref: the window, un-normalised quaternions, the inclusive clamp mask
  D  devo_amd.ba.BA (fused fp32 path)  against oracle/pops.py:BA (fp64, CPU) on the scenes of tests/ba_train_scenes.py

Which case runs which kernel (terms mode, forward and backward; the adjoint's second solve uses the same solver as the forward):
  k_ba_accumulate_reg<8>   A: N = 1, 8        D: n_opt = 1, 8        k_ba_accumulate_reg<11>  A: N = 9, 11       D: n_opt = 9
  k_ba_accumulate_reg<14>  A: N = 12, 14                             k_ba_accumulate_reg<16>  A: N = 15, 16      D: n_opt = 16
  k_ba_accumulate + ba_deferred_schur   A: N = 17, 21, 22, 32   D: n_opt = 17, 22, 32
  k_ba_solve_chain  A: N = 1 .. 21   D: n_opt = 1 .. 17        k_ba_solve  A: N = 22, 32   D: n_opt = 22, 32
  no solver (structure only)  A: N = 0   D: structure_only at n_opt = 9

Bounds of A and D, per compared tensor: max(floor, 2 x e_ref32), floor = 1e-4 for values and 2e-3 for gradients (tests/test_gpu_training.py),
e_ref32 = the error of the REFERENCE evaluated in fp32 on the CPU against its own fp64 result (the factor 2: test_gpu_fullsize's envelope);
e_ref32 itself must stay below 5e-5 / 1e-2, else the scene is too ill-conditioned to test anything (tests/test_ba_terms_ref_cpu.py).

Measured on an MI355X (worst e_hip / bound per tensor over the cases; e_hip and e_ref32 are the errors against fp64):
A, solve_terms, both edge orders (e_hip / e_ref32, each the largest of its group; values = dX, dZ; gradients = g_r, g_w, g_Jz, g_Ji, g_Jj):
  N =  0   values 8.2e-08 / 8.2e-08   gradients 2.3e-07 / 3.0e-07   worst e_hip / bound 0.00
  N =  1   values 2.5e-07 / 2.9e-07   gradients 3.7e-07 / 4.7e-07   worst e_hip / bound 0.00
  N =  8   values 3.5e-07 / 4.0e-07   gradients 4.3e-07 / 4.3e-07   worst e_hip / bound 0.00
  N =  9   values 3.5e-07 / 2.7e-07   gradients 4.2e-07 / 3.5e-07   worst e_hip / bound 0.00
  N = 11   values 3.9e-07 / 4.4e-07   gradients 3.1e-07 / 4.5e-07   worst e_hip / bound 0.00
  N = 12   values 4.9e-07 / 2.5e-07   gradients 5.2e-07 / 3.0e-07   worst e_hip / bound 0.00
  N = 14   values 2.5e-07 / 4.6e-07   gradients 3.5e-07 / 2.8e-07   worst e_hip / bound 0.00
  N = 15   values 3.2e-07 / 1.7e-07   gradients 5.3e-07 / 2.6e-07   worst e_hip / bound 0.00
  N = 16   values 5.3e-07 / 4.2e-07   gradients 8.3e-07 / 3.7e-07   worst e_hip / bound 0.01
  N = 17   values 4.0e-07 / 3.5e-07   gradients 4.3e-07 / 4.5e-07   worst e_hip / bound 0.00
  N = 21   values 4.8e-07 / 4.4e-07   gradients 4.8e-07 / 4.0e-07   worst e_hip / bound 0.00
  N = 22   values 4.8e-07 / 3.6e-07   gradients 5.5e-07 / 3.2e-07   worst e_hip / bound 0.00
  N = 32   values 5.8e-07 / 4.8e-07   gradients 6.2e-07 / 4.2e-07   worst e_hip / bound 0.01
D, devo_amd.ba.BA (e_hip / e_ref32): translation | inverse depth | g_target | g_weight | g_poses | g_patches   (quaternion rows: at most 1.2e-07 / 9.8e-08)
  n_opt = 1 fixedp = 1 E = 21 steps = 1:   1.8e-06 / 8.1e-06 | 2.5e-06 / 9.3e-06 | 5.3e-05 / 1.0e-04 | 9.6e-05 / 1.1e-04 | 1.0e-04 / 1.3e-04 | 1.2e-04 / 5.8e-04   worst e_hip / bound 0.06
  n_opt = 1 fixedp = 3 E = 81 steps = 1:   1.9e-07 / 1.6e-07 | 1.2e-06 / 9.2e-07 | 3.9e-06 / 4.3e-06 | 5.0e-06 / 3.4e-06 | 3.1e-06 / 3.4e-06 | 5.7e-06 / 4.6e-06   worst e_hip / bound 0.01
  n_opt = 8 fixedp = 1 E = 305 steps = 1:   1.9e-05 / 2.0e-05 | 1.6e-05 / 1.9e-05 | 1.0e-04 / 2.0e-04 | 1.1e-04 / 2.2e-04 | 1.5e-04 / 3.0e-04 | 7.7e-04 / 4.9e-04   worst e_hip / bound 0.39
  n_opt = 8 fixedp = 3 E = 440 steps = 1:   2.2e-06 / 1.9e-06 | 2.4e-06 / 2.2e-06 | 6.5e-06 / 1.4e-05 | 2.4e-05 / 4.4e-05 | 6.2e-06 / 1.6e-05 | 1.9e-05 / 3.0e-05   worst e_hip / bound 0.02
  n_opt = 9 fixedp = 1 E = 374 steps = 1:   7.3e-06 / 6.7e-06 | 1.2e-05 / 8.2e-06 | 8.2e-06 / 8.1e-06 | 1.4e-05 / 1.0e-05 | 1.5e-05 / 9.5e-06 | 8.8e-06 / 1.2e-05   worst e_hip / bound 0.12
  n_opt = 9 fixedp = 3 E = 545 steps = 1:   9.4e-07 / 1.2e-06 | 1.5e-06 / 1.5e-06 | 1.3e-06 / 1.8e-06 | 6.4e-06 / 6.6e-06 | 6.6e-06 / 1.1e-05 | 1.2e-05 / 2.2e-05   worst e_hip / bound 0.01
  n_opt = 16 fixedp = 1 E = 682 steps = 1:   1.3e-05 / 1.4e-05 | 1.9e-05 / 2.1e-05 | 1.4e-05 / 1.7e-05 | 1.0e-05 / 9.5e-06 | 1.2e-05 / 1.1e-05 | 2.5e-05 / 2.6e-05   worst e_hip / bound 0.19
  n_opt = 16 fixedp = 3 E = 849 steps = 1:   3.1e-06 / 2.0e-06 | 2.7e-06 / 3.1e-06 | 6.4e-06 / 1.1e-05 | 1.0e-05 / 9.0e-06 | 4.5e-05 / 3.1e-05 | 5.9e-06 / 4.7e-06   worst e_hip / bound 0.03
  n_opt = 17 fixedp = 1 E = 771 steps = 2:   1.5e-05 / 8.9e-06 | 2.0e-05 / 7.4e-06 | 1.0e-05 / 1.7e-05 | 9.0e-06 / 4.3e-06 | 5.2e-04 / 5.9e-04 | 6.1e-05 / 9.1e-05   worst e_hip / bound 0.26
  n_opt = 17 fixedp = 3 E = 939 steps = 2:   3.1e-06 / 5.4e-06 | 3.2e-06 / 5.6e-06 | 4.5e-05 / 3.6e-05 | 3.3e-05 / 3.2e-05 | 5.8e-05 / 4.9e-05 | 2.3e-05 / 1.9e-05   worst e_hip / bound 0.03
  n_opt = 22 fixedp = 1 E = 1268 steps = 2:   2.5e-05 / 8.4e-06 | 2.4e-05 / 8.6e-06 | 4.8e-05 / 3.5e-05 | 3.3e-04 / 4.8e-05 | 5.1e-04 / 4.1e-04 | 2.4e-04 / 4.1e-04   worst e_hip / bound 0.26
  n_opt = 22 fixedp = 3 E = 1129 steps = 2:   4.6e-06 / 2.6e-06 | 5.0e-06 / 1.6e-06 | 1.4e-05 / 3.0e-05 | 3.2e-05 / 6.0e-05 | 3.4e-05 / 7.6e-05 | 6.4e-06 / 2.5e-05   worst e_hip / bound 0.05
  n_opt = 32 fixedp = 1 E = 1947 steps = 1:   1.9e-05 / 7.5e-06 | 2.2e-05 / 7.3e-06 | 1.0e-04 / 5.0e-05 | 3.5e-05 / 2.5e-05 | 1.3e-03 / 3.6e-04 | 3.3e-05 / 4.6e-05   worst e_hip / bound 0.65
  n_opt = 32 fixedp = 3 E = 2214 steps = 1:   2.0e-06 / 1.7e-06 | 1.7e-06 / 9.7e-07 | 1.9e-04 / 1.9e-05 | 1.2e-04 / 1.4e-05 | 1.2e-04 / 1.2e-05 | 3.1e-05 / 1.8e-05   worst e_hip / bound 0.10
  structure only, 9 + 1 frames:   0.0e+00 / 0.0e+00 | 1.9e-06 / 2.3e-06 | 2.1e-07 / 2.3e-07 | 2.6e-06 / 2.7e-06 | 2.5e-07 / 3.1e-07 | 7.0e-07 / 7.0e-07   worst e_hip / bound 0.02
  n_opt = 33 (torch composition):   2.9e-05 / 9.1e-06 | 2.7e-05 / 6.1e-06 | 4.6e-05 / 2.1e-05 | 1.4e-04 / 5.9e-05 | 2.3e-04 / 1.7e-04 | 7.0e-05 / 1.3e-04   worst e_hip / bound 0.29
B and C pass as written (bit-equal terms and gates; apply_step within 2e-5).  All figures are from one run of the scenes as committed.

Rounding noise.  The pose system is reduced with float atomics (k_ba_schur, k_bt_rhs), so e_hip moves from run to run: on a 17 + 1 frame scene
that is NOT admitted (ba_train_scenes.assert_margin: oracle.pops.BA in fp32 1.3e-3 from fp64 in d loss / d poses, the dense composition 1.5e-3
to 2.4e-3) two runs of the fused path gave 3.1e-3 and 1.5e-3 and the torch composition (DEVO_BA_TORCH=1, fp32, same GPU) 3.4e-3: with one
fixed pose the scale of the scene is held by the damping alone, and every fp32 evaluation of the algorithm carries that noise, the fused
kernels no more than the others.  Scenes are therefore admitted on the CPU, from the reference alone, only if its fp32 error is at most half
the floor in both summation orders; the bound is then the floor and the worst ratio above is 0.65.

Sensitivity (a scratch build, never committed).  `same` treated as false in k_bt_edge: test_whole_step_against_the_fp64_oracle fails in 11 of 14
cases, [1-1] [8-1] [9-1] [9-3] [16-1] [16-3] [17-3] [22-1] [22-3] [32-1] [32-3], each on d loss / d weight (8.7e-1 at worst against 2e-3: an
ii == jj edge has Ji = -Jj, its true damping term is zero).  A strict clamp mask in k_ba_apply_step_bwd: all four cases of
test_apply_step_and_adjoint_against_the_reference fail on g_patches (the entries that land exactly on 0.25 and 8).
"""
import ctypes
import pytest
import torch
import ba_terms_ref as R
import ba_train_scenes as S
from util import rel_err, row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def _report(what, e_hip, e_ref, bound):
    worst = {k: e_hip[k] / bound[k] for k in e_hip}
    print(f"{what}: " + "  ".join(f"{k} hip {e_hip[k]:.1e} ref32 {e_ref[k]:.1e} ratio {worst[k]:.2f}" for k in e_hip))
    return worst


# ------------------------------------------------------------------------------------------------- A: solve_terms
def _hip_solve(c, order=None, poison=False):
    from devo_amd.backends import cuda_ba
    sel = slice(None) if order is None else order
    d = lambda t: t[sel].to(DEV).contiguous()
    terms, ii, jj, kk = d(c["terms"]), d(c["ii"]), d(c["jj"]), d(c["kk"])
    lm = torch.tensor([c["lmbda"]], device=DEV)
    if poison:                                                          # the caching allocator's free blocks: a fresh workspace is then garbage
        junk = [torch.full((1 << 18,), float("nan"), device=DEV) for _ in range(8)]
        del junk
    dX, dZ, ws = cuda_ba.solve_terms(terms, lm, ii, jj, kk, c["Np"], c["t0"], c["N"], c["ep"])
    g = cuda_ba.solve_terms_backward(terms, ii, jj, kk, c["Np"], c["t0"], c["N"], ws, c["g_dX"].to(DEV), c["g_dZ"].to(DEV))
    torch.cuda.synchronize()
    return dX.cpu(), dZ.cpu(), g.cpu()


def _terms_bounds(ref):
    e_ref = R.terms_errors(ref[F32], ref[F64])
    for k, v in e_ref.items():
        assert v <= (5e-5 if k in ("dX", "dZ") else 1e-2), f"{k}: the reference in fp32 is {v:.1e} from fp64: the case is too ill-conditioned"
    return e_ref, {k: max(1e-4 if k in ("dX", "dZ") else 2e-3, 2.0 * v) for k, v in e_ref.items()}


@pytest.mark.parametrize("N", R.TERMS_N)
def test_solve_terms_and_adjoint_against_the_dense_reference(N):
    """dX, dZ and g_terms (per column group r | w | Jz | Ji | Jj) for a patch-major edge list and for the same list shuffled (k_bt_inv): both
    within the bound of the fp64 reference, and of each other.  t0 in {0, 1, 3}; frames below and above the window (I = -1, J = -1, both),
    ii == jj inside the window, patch slots without an edge, 53 of 61 slots seen, E no multiple of 64.  N = 0: structure only."""
    c, ref = R.terms_case(N), R.terms_reference(N)
    e_ref, bound = _terms_bounds(ref)
    a = _hip_solve(c)
    b = _hip_solve(c, c["shuffle"])
    assert a[0].shape == (6 * N,) and a[1].shape == (c["Np"],) and a[2].shape == (c["E"], 30)
    assert all(bool(torch.isfinite(t).all()) for t in a + b)
    ea, eb = R.terms_errors(a, ref[F64]), R.terms_errors(b, ref[F64], c["shuffle"])
    b_back = (b[0], b[1], torch.empty_like(b[2]).index_copy_(0, c["shuffle"], b[2]))
    eab = R.terms_errors(a, tuple(t.double() for t in b_back))
    wa = _report(f"solve_terms N={N} t0={c['t0']} ep={c['ep']:g} E={c['E']} patch-major", ea, e_ref, bound)
    wb = _report(f"solve_terms N={N} shuffled", eb, e_ref, bound)
    for k in bound:
        assert wa[k] <= 1.0 and wb[k] <= 1.0, f"N={N} {k}: patch-major {ea[k]:.2e}, shuffled {eb[k]:.2e} > {bound[k]:.1e}"
        assert eab[k] <= bound[k], f"N={N} {k}: the two edge orders differ by {eab[k]:.2e} > {bound[k]:.1e}"
    unseen = torch.bincount(c["kk"], minlength=c["Np"]) == 0
    assert float(a[1][unseen].abs().max()) == 0.0 and float(b[1][unseen].abs().max()) == 0.0        # slots without an edge do not move
    out = ~((c["ii"] >= c["t0"]) & (c["ii"] < c["t0"] + N)), ~((c["jj"] >= c["t0"]) & (c["jj"] < c["t0"] + N))
    assert float(a[2][out[0], 6:18].abs().max()) == 0.0 and float(a[2][out[1], 18:30].abs().max()) == 0.0   # no gradient into a block outside the window


def test_solve_terms_with_a_patch_of_zero_weight():
    """every edge of one patch carries w = 0: C = 0, Q = 1 / lambda = 1e4.  Finite; its rows of g_terms are 1e6 times the others', so the rows are
    compared each on its own scale (row_rel_err, floored at 1e-2 of the largest ORDINARY row)."""
    N = 9
    c, ref = R.terms_case(N, zero_weight=True), R.terms_reference(N, zero_weight=True)
    e_ref, bound = _terms_bounds(R.terms_reference(N))
    z = c["zero_rows"]
    assert int(z.sum()) >= 3 and float(ref[F64][2][z].abs().max()) > 1e3 * float(ref[F64][2][~z].abs().max())
    for order in (None, c["shuffle"]):
        dX, dZ, g = _hip_solve(c, order)
        if order is not None:
            g = torch.empty_like(g).index_copy_(0, order, g)
        assert bool(torch.isfinite(dX).all() and torch.isfinite(dZ).all() and torch.isfinite(g).all())
        assert rel_err(dX, ref[F64][0]) <= bound["dX"] and rel_err(dZ, ref[F64][1]) <= bound["dZ"]
        assert float(dZ[c["kk"][z][0]]) == 0.0
        for name, sl in R.GROUPS:
            r64, r32 = ref[F64][2][:, sl], ref[F32][2][:, sl]
            frac = 1e-2 * float(r64[~z].abs().max()) / float(r64.abs().max())
            e_hip, e_32 = row_rel_err(g[:, sl], r64, frac), row_rel_err(r32, r64, frac)
            assert float(e_32.max()) <= 1e-2, name
            ratio = float((e_hip / torch.clamp(2.0 * e_32, min=2e-3)).max())
            print(f"zero-weight patch, g_{name}: worst per-row error {float(e_hip.max()):.1e} (reference in fp32 {float(e_32.max()):.1e}), worst ratio {ratio:.2f}")
            assert ratio <= 1.0, name


@pytest.mark.parametrize("N", [17, 22])
def test_solve_terms_breakdown_on_both_solvers(N):
    """ep = -1e9: the factorisation breaks down (devo/ba.py:16-20).  dX == 0 although the workspace starts as garbage, dZ = Q u, and g_terms is
    the reference's, which has no gradient through the solve — on k_ba_solve_chain (N = 17, behind the deferred Schur product) and k_ba_solve."""
    c, ref = R.terms_case(N, ep=-1e9), R.terms_reference(N, ep=-1e9)
    assert float(ref[F64][0].abs().max()) == 0.0 and float(ref[F64][2][:, 6:].abs().max()) == 0.0
    e_ref, bound = _terms_bounds(ref)
    got = _hip_solve(c, poison=True)
    assert got[0].shape == (6 * N,) and float(got[0].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in got)
    e = R.terms_errors(got, ref[F64])
    _report(f"breakdown N={N}", e, e_ref, bound)
    for k in bound:
        assert e[k] <= bound[k], (k, e[k])
    assert float(got[2][:, 6:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- B: edge_terms
BOUNDS_B = (2.0, 3.0, 150.0, 110.0)


def _edge_inputs(E, P):
    g = torch.Generator().manual_seed(40 + E + P)
    c = P // 2
    coords = torch.rand(1, E, P, P, 2, generator=g) * 90.0 + 10.0
    target = coords[:, :, c, c] + 5.0 * torch.randn(1, E, 2, generator=g)
    valid = (torch.rand(1, E, generator=g) < 0.8).float()
    expect = {}
    if E >= 10:
        b = torch.tensor(BOUNDS_B)
        inf = torch.tensor([1e9, 1e9, -1e9, -1e9])
        valid[0, :10] = 1.0
        coords[0, :10, c, c] = torch.tensor([10.5, 20.25])
        target[0, :10] = torch.tensor([11.5, 19.25])
        target[0, 0] = torch.tensor([160.5, 220.25])                       # residual exactly (150, 200): |r| = 250, not < 250
        target[0, 1] = torch.tensor([160.5, 20.25]) + torch.tensor([0.0, 199.99])
        for k in range(4):                                              # centre exactly on a bound / one ulp inside it
            coords[0, 2 + k, c, c, k % 2] = b[k]
            coords[0, 6 + k, c, c, k % 2] = torch.nextafter(b[k], inf[k])
            target[0, 2 + k] = coords[0, 2 + k, c, c] + 1.0
            target[0, 6 + k] = coords[0, 6 + k, c, c] + 1.0
        expect = {0: 0.0, 1: 1.0, 2: 0.0, 3: 0.0, 4: 0.0, 5: 0.0, 6: 1.0, 7: 1.0, 8: 1.0, 9: 1.0}
        r = target[0, :2] - coords[0, :2, c, c]
        assert r[0].tolist() == [150.0, 200.0] and r[1, 0] == 150.0 and 199.98 < float(r[1, 1]) < 200.0
        assert float(torch.sqrt((r[0] * r[0]).sum())) == 250.0
    rn = lambda *s: torch.randn(*s, generator=g)
    return coords, valid, 100.0 * rn(1, E, 2, 6), 100.0 * rn(1, E, 2, 6), 10.0 * rn(1, E, 2, 1), target, torch.rand(1, E, 2, generator=g), expect


@pytest.mark.parametrize("E,P", [(257, 3), (257, 1), (1, 3), (1, 1)])
def test_edge_terms_are_bit_equal_and_the_gates_are_strict(E, P):
    """terms and gate against the same formula in fp32 on the CPU: bit-equal (every operation is a subtraction, a negation or a product with 0 / 1),
    and the gate equal to the fp64 reference's.  |r| = 250 exactly and a centre exactly on any of the four bounds close the gate; (150, 199.99) and a
    centre one ulp inside leave it open.  The adjoint: exact products again."""
    from devo_amd.backends import cuda_ba
    coords, valid, Ji, Jj, Jz, target, weight, expect = _edge_inputs(E, P)
    ins = (coords, valid, Ji, Jj, Jz, target, weight)
    t32, g32 = R.edge_terms_ref(*ins, BOUNDS_B)
    _, g64 = R.edge_terms_ref(*(t.double() for t in ins), BOUNDS_B)
    terms, gate = cuda_ba.edge_terms(*(t.to(DEV) for t in ins), BOUNDS_B)
    terms, gate = terms.cpu(), gate.cpu()
    assert torch.equal(gate, g32) and torch.equal(gate.double(), g64)
    for e, want in expect.items():
        assert float(gate[e]) == want, (e, float(gate[e]))
    if E > 1:
        assert 0 < int((valid[0] == 0).sum()) and 0 < int(gate.sum()) < E
    assert torch.equal(terms, t32)
    # the adjoint
    g = torch.randn(E, 30, generator=torch.Generator().manual_seed(3))
    gc, gt, gw, gi, gj, gz = (t.cpu() for t in cuda_ba.edge_terms_backward(g.to(DEV), gate.to(DEV), P))
    c = P // 2
    centre = gc[0, :, c, c].clone()
    gc[0, :, c, c] = 0.0
    assert float(gc.abs().max()) == 0.0                                  # only the centre pixel
    assert torch.equal(gt[0], gate[:, None] * g[:, 0:2]) and torch.equal(centre, -gt[0])
    assert torch.equal(gw[0], gate[:, None] * g[:, 2:4])
    assert torch.equal(gz[0, :, :, 0], g[:, 4:6]) and torch.equal(gi[0].reshape(E, 12), -g[:, 6:18]) and torch.equal(gj[0].reshape(E, 12), g[:, 18:30])
    assert float(gt[0][gate == 0].abs().sum()) == 0.0 and float(gw[0][gate == 0].abs().sum()) == 0.0
    leaves = [t.clone().requires_grad_(True) for t in (coords, Ji, Jj, Jz, target, weight)]      # ... and the reference's autograd says the same
    tr, _ = R.edge_terms_ref(leaves[0], valid, leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], BOUNDS_B)
    ref = torch.autograd.grad((tr * g).sum(), leaves)
    gc[0, :, c, c] = centre
    for got, want in zip((gc, gi, gj, gz, gt, gw), ref):
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------- C: apply_step
DMIN, DMAX = 0.25, 8.0


def _apply_inputs(N, fixedp, n_opt, Np=300, P=3):
    g = torch.Generator().manual_seed(70 + 10 * N + n_opt)
    q = torch.randn(N, 4, generator=g)
    q = q / q.norm(dim=-1, keepdim=True)
    q[1::2] *= 1.7                                                      # the kernel renormalises on load, as lietorch does
    poses = torch.cat([torch.randn(N, 3, generator=g), q], -1)[None].contiguous()
    patches = torch.cat([100.0 * torch.rand(1, Np, 2, P, P, generator=g), 0.1 + 8.9 * torch.rand(1, Np, 1, P, P, generator=g)], 2).contiguous()
    dZ = 0.5 * torch.randn(Np, generator=g)
    one = torch.tensor(1.0)
    # patch 0, dz = 0.125: p + dz == 0.25 exactly | one ulp below | far inside | far outside;  patch 1, dz = 4: == 8 | one ulp above | inside | outside
    dZ[0], dZ[1] = 0.125, 4.0
    lo_out = torch.nextafter(torch.tensor(DMIN), -one) - 0.125
    hi_out = torch.nextafter(torch.tensor(DMAX), 100 * one) - 4.0
    patches[0, 0, 2].view(-1)[:4] = torch.stack([torch.tensor(0.125), lo_out, torch.tensor(1.0), torch.tensor(0.01)])
    patches[0, 1, 2].view(-1)[:4] = torch.stack([torch.tensor(4.0), hi_out, torch.tensor(1.0), torch.tensor(20.0)])
    rest = torch.ones(Np, P, P, dtype=torch.bool)
    rest[0].view(-1)[:2] = False
    rest[1].view(-1)[:2] = False
    near = lambda: torch.minimum((patches[0, :, 2] + dZ.view(-1, 1, 1) - DMIN).abs(), (patches[0, :, 2] + dZ.view(-1, 1, 1) - DMAX).abs())
    patches[0, :, 2] += 0.01 * ((near() < 1e-3) & rest)                  # the random depths keep clear of the bounds
    d = patches[0, :, 2] + dZ.view(-1, 1, 1)                              # fp32, as the kernel forms it
    assert d[0].view(-1)[:2].tolist() == [DMIN, float(torch.nextafter(torch.tensor(DMIN), -one))]
    assert d[1].view(-1)[:2].tolist() == [DMAX, float(torch.nextafter(torch.tensor(DMAX), 100 * one))]
    assert float(near()[rest].min()) > 1e-4 and bool((d[rest] < DMIN).any()) and bool((d[rest] > DMAX).any())
    dX = torch.zeros(n_opt, 6)
    if n_opt:
        dX[:, :3] = 0.1 * torch.randn(n_opt, 3, generator=g)
        phi = torch.randn(n_opt, 3, generator=g)
        dX[:, 3:] = phi / phi.norm(dim=-1, keepdim=True) * (0.05 + 0.45 * torch.rand(n_opt, 1, generator=g))
        # |phi| cycles through exactly zero, the band where the closed-form Jacobian coefficients cancel (3e-6 ... 1e-2), and the random 0.05 .. 0.5
        # (None: the random magnitude stays).  In-band rows get translations of order one: the coefficients' error enters g_dX times |tau|
        band = [0.0, None, 1e-3, 3e-6, 1e-4, 1e-2, None, None, None]
        for i in range(n_opt):
            if band[i % len(band)] is not None:
                dX[i, 3:] *= band[i % len(band)] / dX[i, 3:].norm()
                dX[i, :3] *= 10.0
    g_poses = torch.cat([torch.randn(1, N, 6, generator=g), torch.zeros(1, N, 1)], -1).contiguous()      # lietorch: a tangent in six of seven slots
    g_patches = torch.randn(1, Np, 3, P, P, generator=g)
    return poses, patches, dX.reshape(-1), dZ, g_poses, g_patches


def _apply_ref(poses, patches, dX, dZ, fixedp, n_opt, g_poses, g_patches):
    leaves = [t.double().clone().requires_grad_(True) for t in (poses, patches, dX, dZ)]
    po, qo = R.apply_step_ref(*leaves, fixedp, n_opt, DMIN, DMAX)
    loss = 0.0 * po.sum() + 0.0 * sum(t.sum() for t in leaves)
    loss = loss + ((po * g_poses.double()).sum() if g_poses is not None else 0.0) + ((qo * g_patches.double()).sum() if g_patches is not None else 0.0)
    return po.detach(), qo.detach(), torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("N,fixedp,n_opt", [(5, 1, 4), (5, 2, 2), (6, 0, 6), (4, 1, 0), (10, 1, 9)])
def test_apply_step_and_adjoint_against_the_reference(N, fixedp, n_opt):
    """devo_ba_apply_step / _backward through the C interface (n_opt = 0: dX = NULL).  300 patches: N + Np crosses a workgroup.  Quaternions partly
    un-normalised.  The clamp [0.25, 8]: a depth that lands exactly on a bound passes its gradient (ATen's inclusive mask), one ulp outside does not.
    A missing cotangent (NULL) contributes zero; the seventh slot of every pose gradient is 0.  Rotations of dX are exactly zero, in the band
    3e-6 .. 1e-2 where the closed form of (1 - cos t) / t^2 cancels in fp32 (nine optimised poses reach every magnitude), or between 0.05 and 0.5.
    Tolerance: 2e-5 of each tensor's scale, the figure tests/test_gpu_lietorch.py uses for the same group operations."""
    from devo_amd import _lib as L
    poses, patches, dX, dZ, g_poses, g_patches = _apply_inputs(N, fixedp, n_opt)
    Np, P = patches.shape[1], patches.shape[-1]
    d = [t.to(DEV) for t in (poses, patches, dX, dZ)]
    pX = L.ptr(d[2]) if n_opt > 0 else None
    po, qo = torch.full_like(d[0], float("nan")), torch.full_like(d[1], float("nan"))
    L.check(L.lib().devo_ba_apply_step(L.ptr(d[0]), L.ptr(d[1]), pX, L.ptr(d[3]), N, Np, P, fixedp, n_opt, DMIN, DMAX, L.ptr(po), L.ptr(qo), L.stream()), "apply_step")
    r_po, r_qo, _ = _apply_ref(poses, patches, dX, dZ, fixedp, n_opt, g_poses, g_patches)
    assert rel_err(po, r_po) <= 2e-5 and rel_err(qo, r_qo) <= 2e-5
    assert float((po.cpu()[0, :, 3:].norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(qo.cpu()[:, :, :2], patches[:, :, :2])
    assert qo.cpu()[0, 0, 2].view(-1)[:2].tolist() == [DMIN, DMIN] and qo.cpu()[0, 1, 2].view(-1)[:2].tolist() == [DMAX, DMAX]
    for gp, gq in ((g_poses, g_patches), (None, g_patches), (g_poses, None)):
        nan = lambda t: torch.full_like(t, float("nan"))
        o_p, o_q, o_X, o_Z = nan(d[0]), nan(d[1]), nan(d[2]), nan(d[3])
        dgp, dgq = (None if gp is None else gp.to(DEV)), (None if gq is None else gq.to(DEV))
        L.check(L.lib().devo_ba_apply_step_backward(L.ptr(d[0]), L.ptr(d[1]), pX, L.ptr(d[3]), L.ptr(dgp), L.ptr(dgq), N, Np, P, fixedp, n_opt, DMIN, DMAX,
                                                    L.ptr(o_p), L.ptr(o_q), L.ptr(o_X) if n_opt > 0 else None, L.ptr(o_Z), L.stream()), "apply_step_backward")
        _, _, (r_p, r_q, r_X, r_Z) = _apply_ref(poses, patches, dX, dZ, fixedp, n_opt, gp, gq)
        tag = f"(g_poses {'given' if gp is not None else 'NULL'}, g_patches {'given' if gq is not None else 'NULL'})"
        for name, got, want in (("g_poses", o_p, r_p), ("g_patches", o_q, r_q), ("g_dX", o_X, r_X), ("g_dZ", o_Z, r_Z)):
            got = got.cpu()
            if got.numel() == 0:                                         # (g_dX without optimised poses)
                continue
            assert bool(torch.isfinite(got).all()), name + tag
            if float(want.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0, name + tag
            else:
                assert rel_err(got, want) <= 2e-5, f"{name} {tag}: {rel_err(got, want):.2e}"
        assert float(o_p.cpu()[..., 6].abs().max()) == 0.0
        if gq is not None:                                               # the clamp mask, entry by entry
            m = o_q.cpu()[0, :2, 2].reshape(2, -1)[:, :4] != 0
            assert m.tolist() == [[True, False, True, False], [True, False, True, False]], m.tolist()
            assert torch.equal(o_q.cpu()[0, :2, 2].reshape(2, -1)[:, [0, 2]], gq[0, :2, 2].reshape(2, -1)[:, [0, 2]])


# ------------------------------------------------------------------------------------------------- D: the whole step
def _hip_step(s, steps=1, structure_only=False):
    from devo_amd.ba import BA
    from devo_amd import projective_ops as pops
    from devo_amd.lietorch import SE3
    leaf = lambda t: t.detach().to(DEV, copy=True).requires_grad_(True)
    tgt, wgt, pos, pat = leaf(s["target"]), leaf(s["weight"]), leaf(s["poses"]), leaf(s["patches"])
    intr, ii, jj, kk = (s[k].to(DEV) for k in ("intr", "ii", "jj", "kk"))
    G, P = SE3(pos), pat
    for _ in range(steps):
        G, P = BA(G, P, intr, tgt, wgt, S.LMBDA, ii, jj, kk, list(s["bounds"]), ep=S.EP, fixedp=s["fixedp"], structure_only=structure_only)
    S.loss_of(pops.transform, G, P, s, F32).backward()
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu()
    return dict(poses=c(G.data), patches=c(P), g_target=c(tgt.grad), g_weight=c(wgt.grad), g_poses=c(pos.grad), g_patches=c(pat.grad))


def _check_step(s, ref, got, what):
    e_ref = S.envelope(ref)
    S.assert_envelope(e_ref)
    bound = S.bounds_of(e_ref)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    e_hip = S.errors(got, ref[F64])
    worst = _report(what, e_hip, e_ref, bound)
    for k in bound:
        assert worst[k] <= 1.0, f"{what}, {k}: HIP {e_hip[k]:.2e} > bound {bound[k]:.1e} (reference in fp32: {e_ref[k]:.1e})"
    assert float(got["g_poses"][..., 6].abs().max()) == 0.0


@pytest.fixture
def solves(monkeypatch):
    """the n_opt of every devo_ba_solve_terms call"""
    from devo_amd.backends import cuda_ba
    calls, real = [], cuda_ba.solve_terms

    def spy(terms, lm, ii, jj, kk, n_slots, t0, n_opt, ep, status=None):
        calls.append(int(n_opt))
        return real(terms, lm, ii, jj, kk, n_slots, t0, n_opt, ep, status)
    monkeypatch.setattr(cuda_ba, "solve_terms", spy)
    return calls


@pytest.mark.parametrize("fixedp", S.FIXEDP)
@pytest.mark.parametrize("n_opt", S.N_OPT)
def test_whole_step_against_the_fp64_oracle(n_opt, fixedp, solves):
    """devo_amd.ba.BA (fused) against oracle.pops.BA: new poses (translation rows, quaternion rows), new inverse depths, and the gradients of
    test_gpu_training's loss with respect to target, weight, poses and patches; two chained steps at n_opt = 17 and 22.  The scene's conditions
    (every gate cause, both clamps, nothing within reach of a threshold) are asserted, not assumed."""
    s = S.scene(n_opt, fixedp)
    steps = 2 if n_opt in S.CHAINED else 1
    ref = S.reference(n_opt, fixedp, steps)
    S.assert_conditions(S.conditions(s), s["n"])
    if steps == 2:
        S.assert_conditions(S.conditions(s, *ref[F64]["stages"][1]), s["n"], first=False)
    got = _hip_step(s, steps)
    assert solves == [n_opt] * steps                                    # the fused path, with this many poses
    _check_step(s, ref, got, f"BA n_opt={n_opt} fixedp={fixedp} E={len(s['ii'])} steps={steps}")


def test_whole_structure_only_step_against_the_fp64_oracle(solves):
    n_opt, fixedp = S.STRUCTURE_ONLY
    s, ref = S.scene(n_opt, fixedp), S.reference(n_opt, fixedp, 1, True)
    S.assert_conditions(S.conditions(s, structure_only=True), s["n"])
    got = _hip_step(s, 1, True)
    assert solves == [0]
    assert torch.equal(got["poses"][0, :, :3], s["poses"][0, :, :3])
    _check_step(s, ref, got, f"BA structure only, {n_opt} + {fixedp} frames")


def test_33_poses_take_the_torch_composition(solves):
    """beyond the 32 poses whose system fits the LDS, devo_amd.ba.BA runs the torch composition (same result, against the same oracle) and the C
    entry points refuse without launching anything."""
    from devo_amd import _lib as L
    from devo_amd.backends import cuda_ba
    s, ref = S.scene(33, 1), S.reference(33, 1)
    S.assert_conditions(S.conditions(s), s["n"])
    got = _hip_step(s)
    assert solves == []
    _check_step(s, ref, got, "BA n_opt=33 (torch composition)")
    c = R.terms_case(32)
    terms, ii, jj, kk = (c[k].to(DEV) for k in ("terms", "ii", "jj", "kk"))
    ws = cuda_ba.workspace(c["E"], c["Np"], 33, DEV)
    out = torch.full((6 * 33 + c["Np"],), 7.0, device=DEV)
    g = torch.full((c["E"], 30), 7.0, device=DEV)
    lm = torch.tensor([1e-4], device=DEV)
    rc = L.lib().devo_ba_solve_terms(L.ptr(terms), L.ptr(lm), L.ptr(ii), L.ptr(jj), L.ptr(kk), c["E"], c["Np"], 0, 33, ctypes.c_float(10.0), L.ptr(ws), ws.numel(),
                                     L.ptr(out), L.ptr(out[6 * 33:]), None, L.stream())
    rb = L.lib().devo_ba_solve_terms_backward(L.ptr(terms), L.ptr(ii), L.ptr(jj), L.ptr(kk), c["E"], c["Np"], 0, 33, L.ptr(ws), ws.numel(), L.ptr(out), L.ptr(out[6 * 33:]),
                                              L.ptr(g), L.stream())
    torch.cuda.synchronize()
    assert rc == 3 and rb == 3                                          # DEVO_ERR_UNSUPPORTED
    assert bool((out == 7.0).all()) and bool((g == 7.0).all())           # nothing was written
