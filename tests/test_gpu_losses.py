"""devo_amd.losses (csrc/loss.hip) against tests/golden/train_loss_f64.npz — the reference's loss, train.py:172-236, evaluated on CPU
in fp64 with the reference's SE3 and kabsch_umeyama (tools/gen_golden_loss.py; tests/test_losses_cpu.py pins the file to an
independent restatement).  Tolerances: values 1e-4 of the output scale; gradients 1e-6 (fp64) and 3e-4 (fp32) of the
gradient's largest magnitude (tests/test_gpu_train_iteration.py); the Sim(3) scale 1e-6 relative.

The case Gs = Ps comes twice.  `same`: pure translations on a lattice, where every operation of the chain is exact in any faithful
implementation (s = 1, zero pair errors, zero norms): the gradient is asserted to be exactly zero.  `same_rot`: with rotations the pair
errors are rounding noise of the order of 1e-16 and the reference's own gradient is a set of unit directions of that noise, not zero —
there the values are compared and the gradient is asserted to be finite."""
import os
import subprocess
import sys
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("flow", "pose", "tr", "ro", "px1", "r1", "r2", "t1", "t2", "scores", "scale")
FLOW_CASES = ("flow/mixed_1", "flow/mixed_65", "flow/mixed_513", "flow/all_65", "flow/none_65")
KINDS = ("general", "collinear", "planar", "identity", "twentieth", "same", "same_rot")
GRAD_TOL = {torch.float64: 1e-6, torch.float32: 3e-4}


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "train_loss_f64.npz"))
    return {k: z[k] for k in z.files}


def inputs(golden, name, dt, grad=True):
    k = "case/" + name + "/"
    d = lambda f: torch.from_numpy(golden[k + f]).to(dt).to(DEV)
    v, x, y, Gs, Ps = d("v"), d("x").requires_grad_(grad), d("y"), d("Gs").requires_grad_(grad), d("Ps")
    scorer = None
    if k + "scores" in golden:
        scorer = (d("scores").requires_grad_(grad), d("v_full"), d("x_full"), d("y_full"), d("ba_weights"), torch.from_numpy(golden[k + "kk"]).to(DEV))
    return v, x, y, Gs, Ps, scorer


def run(golden, name, dt=torch.float64, index=2, **kw):
    from devo_amd import losses
    v, x, y, Gs, Ps, scorer = inputs(golden, name, dt)
    loss, stats = losses.iteration_loss(v, x, y, Gs, Ps, index=index, scorer=scorer, **kw)
    assert loss.dim() == 0 and loss.dtype == dt and stats.data.dtype == torch.float32 and stats.data.shape == (11,)
    loss.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return loss.detach(), stats.data.clone(), zero(x), zero(Gs), (zero(scorer[0]) if scorer else None)


def check_values(golden, name, loss, stats, tol=1e-4):
    want = torch.from_numpy(golden["case/" + name + "/stats"])
    got = stats.double().cpu()
    nan = torch.isnan(want)
    assert torch.equal(nan, torch.isnan(got)), f"{name}: NaN pattern {got.tolist()} vs {want.tolist()}"
    for f, w, g in zip(FIELDS, want.tolist(), got.tolist()):
        if w == w:
            assert abs(g - w) <= tol * max(1.0, abs(w)), f"{name}: {f} = {g!r}, fixture {w!r}"
    wl = float(golden["case/" + name + "/loss"])
    if wl == wl:
        assert abs(float(loss) - wl) <= tol * max(1.0, abs(wl)), f"{name}: loss {float(loss)!r}, fixture {wl!r}"
    else:
        assert bool(torch.isnan(loss))


def check_grad(got, want, tol, what):
    want = torch.as_tensor(want).double().reshape(got.shape)
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all()), what
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= tol * scale if scale > 0 else err == 0.0, f"{what}: max |diff| {err:.3e}, gradient scale {scale:.3e}"


@pytest.mark.parametrize("name", FLOW_CASES)
def test_flow_term(golden, name):
    loss, stats, gx, gG, _ = run(golden, name)
    check_values(golden, name, loss, stats)
    check_grad(gx, golden["case/" + name + "/g_coords"], 1e-6, name + " d/d coords")
    check_grad(gG, golden["case/" + name + "/g_Gs"], 1e-6, name + " d/d Gs")
    if name == "flow/none_65":
        assert bool(torch.isnan(stats[0])) and not bool(gx.any())
    if name in ("flow/mixed_65", "flow/mixed_513"):                                    # the edge with v == 0.5 is out, the zero residual passes nothing
        assert not bool(gx[0, 3].any()) and not bool(gx[0, 5].any()) and bool(torch.isfinite(gx).all())
    again = run(golden, name)
    assert all(torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)) for a, b in zip((loss, stats, gx, gG), again[:4])), name + ": two runs differ"


def test_flow_term_fp32(golden):
    for name in ("flow/mixed_513", "flow/all_65"):
        loss, stats, gx, gG, _ = run(golden, name, torch.float32)
        check_values(golden, name, loss, stats)
        check_grad(gx, golden["case/" + name + "/g_coords"], 3e-4, name + " d/d coords (fp32)")
        check_grad(gG, golden["case/" + name + "/g_Gs"], 3e-4, name + " d/d Gs (fp32)")


def lietorch_pose_loss(Gs_data, Ps_data, s):
    """train.py:207-234 through devo_amd.lietorch on the GPU, with the scale of the kernel under test as the constant the reference detaches."""
    from devo_amd.lietorch import SE3
    n = Gs_data.shape[1]
    ii, jj = torch.meshgrid(torch.arange(n, device=DEV), torch.arange(n, device=DEV), indexing="ij")
    keep = ii != jj
    ii, jj = ii[keep], jj[keep]
    P1, P2 = SE3(Gs_data).inv(), SE3(Ps_data).inv()
    P1 = P1.scale(s.view(1, 1))
    dP = P1[:, ii].inv() * P1[:, jj]
    dG = P2[:, ii].inv() * P2[:, jj]
    e1 = (dP * dG.inv()).log()
    return e1[..., 0:3].norm(dim=-1).mean() + e1[..., 3:6].norm(dim=-1).mean()


@pytest.mark.parametrize("n", [2, 3, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_pose_term(golden, kind, n):
    name = f"pose/{kind}_{n}"
    loss, stats, gx, gG, _ = run(golden, name)
    check_values(golden, name, loss, stats)
    want_s = float(golden["case/" + name + "/stats"][10])
    assert abs(float(stats[10]) - want_s) <= 1e-6 * want_s, f"{name}: s = {float(stats[10])!r}, torch.svd gives {want_s!r}"
    assert bool(torch.isfinite(gG).all()) and not bool(gG[..., 6].any())
    if kind == "same":
        assert float(stats[10]) == 1.0 and float(stats[2]) == 0.0 and float(stats[3]) == 0.0 and not bool(gG.any())
    elif kind == "same_rot":
        assert float(stats[2]) <= 1e-4 and float(stats[3]) <= 1e-4
    else:
        check_grad(gG, golden["case/" + name + "/g_Gs"], 1e-6, name + " d/d Gs")
        v, x, y, Gs, Ps, _ = inputs(golden, name, torch.float64)
        w = golden["weights"]
        (float(w[1]) * lietorch_pose_loss(Gs, Ps, stats[10].double())).backward()
        check_grad(gG, Gs.grad.cpu(), 1e-6, name + " d/d Gs against devo_amd.lietorch")
    again = run(golden, name)
    assert torch.equal(loss, again[0]) and torch.equal(stats, again[1]) and torch.equal(gG, again[3]), name + ": two runs differ"


def test_pose_term_fp32(golden):
    for name in ("pose/general_15", "pose/planar_3", "pose/identity_15"):
        loss, stats, gx, gG, _ = run(golden, name, torch.float32)
        check_values(golden, name, loss, stats)
        check_grad(gG, golden["case/" + name + "/g_Gs"], 3e-4, name + " d/d Gs (fp32)")


@pytest.mark.parametrize("name", ["score/general", "score/none"])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_scorer_term_atomic_scatter(golden, name, dt):
    assert not torch.are_deterministic_algorithms_enabled()
    loss, stats, gx, gG, gs = run(golden, name, dt)
    check_values(golden, name, loss, stats)
    check_grad(gs, golden["case/" + name + "/g_scores"], GRAD_TOL[torch.float32], name + " d/d scores")        # atomics: the fp32 tolerance
    check_grad(gx, golden["case/" + name + "/g_coords"], GRAD_TOL[dt], name + " d/d coords")
    if name == "score/none":
        assert bool(torch.isnan(stats[9])) and bool(torch.isnan(loss))
    below = torch.from_numpy(golden["case/" + name + "/scores"]) < 1e-6
    assert int(below.sum()) == 3


@pytest.mark.parametrize("name", ["score/general", "score/none"])
def test_scorer_term_fixed_order_scatter(golden, name):
    torch.use_deterministic_algorithms(True)
    try:
        a = run(golden, name)
        b = run(golden, name)
    finally:
        torch.use_deterministic_algorithms(False)
    check_values(golden, name, a[0], a[1])
    check_grad(a[4], golden["case/" + name + "/g_scores"], 1e-6, name + " d/d scores (fixed order)")
    assert torch.equal(a[4], b[4]) and torch.equal(a[1].nan_to_num(7.0), b[1].nan_to_num(7.0)), name + ": two runs differ"


def test_the_two_masks_differ(golden):
    """v == 0.5: out of the flow term (>), in the scorer term (>=)."""
    from devo_amd import losses
    v, x, y, Gs, Ps, scorer = inputs(golden, "score/general", torch.float64, grad=False)
    half = torch.full_like(v, 0.5)
    _, st = losses.iteration_loss(half, x, y, Gs, Ps, index=0, scorer=(scorer[0], torch.full_like(scorer[1], 0.5), *scorer[2:]))
    assert bool(torch.isnan(st.flow)) and bool(torch.isfinite(st.scores))


def test_weighting_rules(golden):
    name = "score/general"
    w = [float(t) for t in golden["weights"]]
    st = dict(zip(FIELDS, golden["case/" + name + "/stats"].tolist()))
    cases = {"on": (dict(index=2), w[0] * st["flow"] + w[2] * st["scores"] + w[1] * st["pose"]),
             "index<2": (dict(index=1), w[0] * st["flow"] + w[2] * st["scores"]),
             "structure_only": (dict(index=5, structure_only=True), w[0] * st["flow"] + w[2] * st["scores"])}
    for tag, (kw, want) in cases.items():
        loss, stats, gx, gG, gs = run(golden, name, **kw)
        assert abs(float(loss) - want) <= 1e-4 * max(1.0, abs(want)), tag
        assert abs(float(stats[1]) - st["pose"]) <= 1e-4 * max(1.0, st["pose"]), tag + ": the pose term is reported either way"
        assert bool(gG.any()) == (tag == "on"), tag
    from devo_amd import losses
    v, x, y, Gs, Ps, scorer = inputs(golden, name, torch.float64)
    loss, stats = losses.iteration_loss(v, x, y, Gs, Ps, index=2, flow_weight=0.3, pose_weight=2.0)             # no scorer=: no scorer term
    want = 0.3 * st["flow"] + 2.0 * st["pose"]
    assert abs(float(loss) - want) <= 1e-4 * max(1.0, abs(want)) and float(stats.scores) == 0.0
    loss.backward()
    assert scorer[0].grad is None


@pytest.mark.parametrize("width", [13, 6])
def test_sequence_loss(golden, width):
    from devo_amd import losses
    from devo_amd.lietorch import SE3
    sc = inputs(golden, str(golden["seq/scorer"]), torch.float64)[5]
    traj, leaves = [], []
    for entry in golden["seq/entries"]:
        fl, po = str(entry).split()
        v, x, y, _, _, _ = inputs(golden, fl, torch.float64)
        _, _, _, Gs, Ps, _ = inputs(golden, po, torch.float64)
        leaves.append((x, Gs))
        head = (v, x, y, SE3(Gs), SE3(Ps), torch.as_tensor(0))
        traj.append(head + (*sc, torch.zeros(0, device=DEV)) if width == 13 else head)
    total, stats = losses.sequence_loss(traj)
    total.backward()
    if width == 13:
        want = float(golden["seq/loss"])
        assert abs(float(total) - want) <= 1e-4 * max(1.0, abs(want))
        want_stats = torch.from_numpy(golden["seq/stats"])
        assert float((stats.data.double().cpu() - want_stats).abs().max()) <= 1e-4 * max(1.0, float(want_stats.abs().max()))
        for i, (x, Gs) in enumerate(leaves):
            check_grad(x.grad, golden[f"seq/g_coords{i}"], 1e-6, f"sequence d/d coords {i}")
            check_grad(Gs.grad if Gs.grad is not None else torch.zeros_like(Gs), golden[f"seq/g_Gs{i}"], 1e-6, f"sequence d/d Gs {i}")
        check_grad(sc[0].grad, golden["seq/g_scores"], 3e-4, "sequence d/d scores")
    else:                                                                          # 6-tuples (enet.py:374): no scorer term, the rest as above
        for i, (x, Gs) in enumerate(leaves):
            check_grad(x.grad, golden[f"seq/g_coords{i}"], 1e-6, f"sequence d/d coords {i}")
        assert sc[0].grad is None and float(stats.scores) == 0.0
    m = losses.metrics(stats, total)
    assert list(m) == ["loss/train", "loss/pose_train", "loss/rotation_train", "loss/translation_train", "loss/flow_train", "loss/scores_train", "px1", "r1", "r2",
                       "t1", "t2"]
    assert all(isinstance(t, float) for t in m.values()) and abs(m["loss/train"] - float(total)) <= 1e-6 * abs(float(total))


_LEG = r"""
import sys, os, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import devo_amd.backends as B
from devo_amd import losses
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
z = np.load(os.path.join(sys.argv[1], "tests", "golden", "train_loss_f64.npz"))
out = {}
torch.use_deterministic_algorithms(True)                      # (the atomic scatter is the one piece that is not reproducible bit for bit)
for name in ("flow/mixed_513", "pose/general_15", "pose/collinear_3", "score/general"):
    for dt in (torch.float64, torch.float32):
        k = "case/" + name + "/"
        d = lambda f: torch.from_numpy(z[k + f]).to(dt).cuda()
        x, Gs = d("x").requires_grad_(True), d("Gs").requires_grad_(True)
        scorer = None
        if k + "scores" in z.files:
            scorer = (d("scores").requires_grad_(True), d("v_full"), d("x_full"), d("y_full"), d("ba_weights"), torch.from_numpy(z[k + "kk"]).cuda())
        loss, stats = losses.iteration_loss(d("v"), x, d("y"), Gs, d("Ps"), index=2, scorer=scorer)
        loss.backward()
        tag = name + str(dt)
        out[tag + "loss"], out[tag + "stats"], out[tag + "gx"], out[tag + "gG"] = loss.detach(), stats.data, x.grad, Gs.grad
        if scorer:
            out[tag + "gs"] = scorer[0].grad
torch.cuda.synchronize()
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_both_bindings_return_the_same_bits(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, root, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res.append(torch.load(path))
    a, b = res
    assert a.keys() == b.keys() and len(a) == 34
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{k}: the two bindings disagree"


def test_no_host_synchronisation(golden):
    from devo_amd import losses
    v, x, y, Gs, Ps, scorer = inputs(golden, "score/general", torch.float32)
    losses.iteration_loss(v, x, y, Gs, Ps, index=2, scorer=scorer)[0].backward()            # (first call: the library is loaded)
    x.grad = Gs.grad = scorer[0].grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, stats = losses.iteration_loss(v, x, y, Gs, Ps, index=2, scorer=scorer)
        loss.backward()
        flow = stats.flow
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert x.grad is not None and Gs.grad is not None and scorer[0].grad is not None and flow.is_cuda
    m = losses.metrics(stats, loss)                                                          # the one call that copies
    assert len(m) == 11 and m["loss/train"] == float(loss)


def test_trainnet_objectives():
    from devo_amd import training as T
    net, model, opt = T.build_trainer(DEV, 1)
    batch = T.make_batch("cfg1", 1234, DEV)
    torch.manual_seed(5)
    a = model(batch, iters=2)
    torch.manual_seed(5)
    b = model(batch, iters=2, objective="bench")
    assert torch.equal(a.detach(), b.detach())
    opt.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    loss = model(batch, iters=2, objective="reference")
    loss.backward()
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    missing = [n for n, q in net.update.named_parameters() if q.grad is None or not bool(torch.isfinite(q.grad).all())]
    assert not missing, missing
    assert any(float(q.grad.abs().max()) > 0 for q in net.update.parameters())
    scorer = [q for n, q in net.named_parameters() if n.startswith("patchify.scorer")]
    assert scorer and all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in scorer)      # (through the scorer term)
    with pytest.raises(ValueError):
        model(batch, iters=1, objective="other")
    assert bool(torch.isfinite(T.train_step(model, opt, batch, iters=2, objective="reference")))
