"""The yardsticks of tests/test_gpu_ba_train_kernels.py, checked on the CPU: tests/ba_terms_ref.py (edge terms -> dense solve -> retraction, fp64)
composes to oracle/pops.py:BA, which the goldens pin to the reference, in value and in all four input gradients; and the scenes of
tests/ba_train_scenes.py meet the conditions the GPU comparison relies on (every gate and both clamps occur, nothing sits on a threshold, the
reference's own fp32 evaluation stays close enough to fp64 for an envelope to mean something)."""
import os
import numpy as np
import pytest
import torch
import ba_terms_ref as R
import ba_train_scenes as S
from util import rel_err

KEYS = ("poses", "patches", "g_target", "g_weight", "g_poses", "g_patches")


def _golden_scene(golden_dir):
    z = np.load(os.path.join(golden_dir, "ba_train_f64.npz"))
    t = lambda k: torch.from_numpy(z[k])
    return dict(poses=t("poses"), patches=t("patches"), intr=t("intrinsics"), target=t("target"), weight=t("weight"), ii=t("ii"), jj=t("jj"), kk=t("kk"),
                bounds=tuple(z["bounds"].tolist()), fixedp=1, n_opt=4, n=5, lw=t("loss_weights"))


@pytest.mark.parametrize("which", ["golden", "synthetic"])
@pytest.mark.parametrize("structure_only", [False, True])
def test_the_composed_reference_reproduces_the_oracle_step(golden_dir, which, structure_only):
    """transform(jacobian) -> edge_terms_ref -> solve_from_terms -> apply_step_ref against oracle.pops.BA in fp64: new poses, new patches and the
    gradients of test_gpu_training's loss with respect to target, weight, poses and patches, two chained steps, to 1e-10 of each tensor's scale.
    Scenes: the golden's inputs (5 frames, fixedp = 1) and a synthetic one with 17 optimised poses behind 2 fixed ones."""
    s = _golden_scene(golden_dir) if which == "golden" else dict(S.scene(17, 2))
    q = s["poses"].double()                                           # unit quaternions in fp64: a structure-only step of devo/ba.py returns its poses as
    s["poses"] = torch.cat([q[..., :3], q[..., 3:] / q[..., 3:].norm(dim=-1, keepdim=True)], -1)      # they came, apply_step_ref renormalises them (as the kernel does)
    a = S.oracle_step(s, torch.float64, steps=2, structure_only=structure_only)
    b = S.oracle_step(s, torch.float64, steps=2, structure_only=structure_only, step=S.composed_step)
    for k in KEYS:
        assert float(a[k].abs().max()) > 0, k
        assert rel_err(b[k], a[k]) <= 1e-10, (k, rel_err(b[k], a[k]))
    assert float(a["g_poses"][..., 6].abs().max()) == 0.0 and float(b["g_poses"][..., 6].abs().max()) == 0.0


def test_solve_from_terms_breaks_down_like_the_oracle():
    """ep = -1e9: the factorisation fails, dX = 0, the depth step is Q u and no gradient passes through the solve (devo/ba.py:16-20)"""
    c = R.terms_case(17, ep=-1e9)
    dX, dZ, g = R.solve_with_gradient(c, torch.float64)
    assert float(dX.abs().max()) == 0.0 and float(dZ.abs().max()) > 0 and bool(torch.isfinite(g).all())
    assert float(g[:, 6:].abs().max()) == 0.0 and float(g[:, :6].abs().max()) > 0


CASES = [(n, f) for n in S.N_OPT for f in S.FIXEDP] + [(33, 1)]


@pytest.mark.parametrize("n_opt,fixedp", CASES)
def test_scene_conditions(n_opt, fixedp):
    """every scene of the GPU test: each gate cause removes an edge and all together at most a quarter; no edge within 1e-2 px of a gate threshold
    (1e-3 of the depth gate), no depth within 1e-4 of a clamp bound; both clamps occur; and oracle.pops.BA in fp32 stays within 5e-5 (values) and
    1e-2 (gradients) of its own fp64 result, so that the envelope max(floor, 2 x that) cannot hide a wrong kernel.  Admission (assert_margin): in
    both summation orders the fp32 reference stays within half the floor, so no case sits on its bound by rounding noise alone."""
    s = S.scene(n_opt, fixedp)
    S.assert_conditions(S.conditions(s), s["n"])
    steps = 2 if n_opt in S.CHAINED else 1
    ref = S.reference(n_opt, fixedp, steps)
    if steps == 2:
        S.assert_conditions(S.conditions(s, *ref[torch.float64]["stages"][1]), s["n"], first=False)
    e, e2 = S.envelope(ref), S.second_opinion(n_opt, fixedp, steps)
    print(n_opt, fixedp, {k: f"{v:.1e} {e2[k]:.1e}" for k, v in e.items()})
    S.assert_envelope(e)
    S.assert_margin(e, e2)


def test_structure_only_scene_conditions():
    s = S.scene(*S.STRUCTURE_ONLY)
    S.assert_conditions(S.conditions(s, structure_only=True), s["n"])
    e, e2 = S.envelope(S.reference(*S.STRUCTURE_ONLY, 1, True)), S.second_opinion(*S.STRUCTURE_ONLY, 1, True)
    S.assert_envelope(e)
    S.assert_margin(e, e2)


@pytest.mark.parametrize("N", R.TERMS_N)
def test_random_terms_are_well_conditioned(N):
    """the reference's own fp32 evaluation of every random-terms case: within 5e-5 (dX, dZ) and 1e-2 (each column group of g_terms) of fp64"""
    ref = R.terms_reference(N)
    for name, e in R.terms_errors(ref[torch.float32], ref[torch.float64]).items():
        assert e <= (5e-5 if name in ("dX", "dZ") else 1e-2), (N, name, e)
