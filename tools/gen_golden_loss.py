#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference and oracle/).

tests/golden/train_loss_f64.npz: the reference's training loss (train.py:172-236) and logged statistics (:254-266) evaluated on CPU in
fp64 with the reference's own pieces — `SE3` from devo.lietorch over the oracle backend (the shims of tools/gen_golden_update.py) and
`kabsch_umeyama` compiled from the reference's train.py at generation time (the function's syntax tree is taken out of the file: the
module itself imports a data loader, OpenCV and a plotting stack at module scope).  The loop body around them is inline code of `train()`
and is restated below line by line.  The file holds data only: inputs (fp32-representable, stored as fp32), every statistic, the loss
and the gradients with respect to coords, Gs.data and scores.

Cases (tests/test_gpu_losses.py):
  flow/*    Ec = 1, 65, 513 (one lane, one more than a wave, two workgroups of 256 and one edge), every edge valid, no edge valid,
            a v of exactly 0.5, an edge whose minimising pixel has a zero residual.  No edge has two equal minima (asserted).
  pose/*    n = 2, 3, 15: general, collinear (rank-1 H), planar (rank-2 H), identity prediction (H = 0, s = inf -> 10), a prediction
            at a twentieth of the scale (s = 20 -> 10), Gs = Ps on a lattice of pure translations (every operation exact: s = 1,
            gradient exactly zero — asserted here) and Gs = Ps with rotations (`same_rot`: the pair errors are rounding noise, the
            reference's gradient is a set of unit directions of that noise; stored, compared for the values only).
  score/*   kk with repeats (at most 40 edges to a patch), scores below 1e-6 and none equal to it, a case without a valid edge.
  seq       a three-iteration trajectory of 13-tuples: the total and its gradients."""
import ast
import os
import sys
import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_update as GU                            # noqa: E402

DT = torch.float64
P = 3
FW, PW, SW = 0.1, 10.0, 0.05                               # the defaults of train.py's arguments


def reference_kabsch():
    tree = ast.parse(open(os.path.join(GU.REF, "train.py")).read())
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "kabsch_umeyama"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "train.py", "exec"), ns)
    return ns["kabsch_umeyama"]


def f32(t):
    """fp32-representable fp64 values: the fixture stores fp32, both sides compute from the same numbers."""
    return t.to(torch.float32).to(DT)


def reference_iteration(SE3, kabsch, data, i, last, so=False):
    """train.py:176-236 for one entry of traj -> (this iteration's contribution to loss, the statistics of :254-266 + s)."""
    v, x, y, P1, P2 = data[:5]
    valid = (v > 0.5).reshape(-1)
    e = (x - y).norm(dim=-1)
    ef = e.reshape(-1, P ** 2)[valid].min(dim=-1).values
    flow_loss = ef.mean()
    if len(data) == 13 and last:
        scores, v_full, x_full, y_full, ba_weights, kk = data[6:12]
        valid_full = (v_full >= 0.5).reshape(-1)
        kk = kk[valid_full]
        e_full = (x_full - y_full).norm(dim=-1)
        e_full = e_full.reshape(-1, P ** 2)[valid_full].min(dim=-1).values
        scores_loss = ((-0.5 * (ba_weights.view(-1, 2)[valid_full].mean(dim=-1)).log() + 1) * scores.view(-1)[kk] * e_full).mean()
        scores = torch.max(scores, torch.as_tensor(1e-6, dtype=DT))
        scores = -scores.log()
        scores_loss = scores_loss + scores.mean()
    else:
        scores_loss = torch.as_tensor(0.0, dtype=DT)
    N = P1.shape[1]
    ii, jj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    k = ii != jj
    ii, jj = ii[k], jj[k]
    P1 = P1.inv()
    P2 = P2.inv()
    t1 = P1.matrix()[..., :3, 3]
    t2 = P2.matrix()[..., :3, 3]
    raw = kabsch(t2[0], t1[0]).detach()
    s = raw.clamp(max=10.0)
    P1 = P1.scale(s.view(1, 1))
    dP = P1[:, ii].inv() * P1[:, jj]
    dG = P2[:, ii].inv() * P2[:, jj]
    e1 = (dP * dG.inv()).log()
    tr = e1[..., 0:3].norm(dim=-1)
    ro = e1[..., 3:6].norm(dim=-1)
    loss = FW * flow_loss + SW * scores_loss
    pose_loss = tr.mean() + ro.mean()
    if not so and i >= 2:
        loss = loss + PW * pose_loss
    stats = [flow_loss, pose_loss, tr.mean(), ro.mean(), (e < .25).double().mean(), (ro < .001).double().mean(), (ro < .01).double().mean(),
             (tr < .001).double().mean(), (tr < .01).double().mean(), scores_loss, s]
    return loss, torch.stack([t.detach().reshape(()) for t in stats]), float(raw)


def flow_inputs(g, Ec, mode):
    x = f32(torch.rand(1, Ec, P, P, 2, generator=g, dtype=DT) * 60)
    y = f32(x + torch.randn(1, Ec, P, P, 2, generator=g, dtype=DT) * 1.5)
    v = (torch.rand(1, Ec, generator=g, dtype=DT) > 0.3).to(DT)
    if mode == "all":
        v[:] = 1.0
    elif mode == "none":
        v[:] = 0.0
        v[0, ::3] = 0.5                                    # exactly 0.5 is NOT valid here (v > 0.5)
    elif Ec > 8:
        v[0, 3] = 0.5
        v[0, 5] = 1.0
        y[0, 5, 1, 2] = x[0, 5, 1, 2]                      # a valid edge whose minimising pixel has a zero residual
    else:
        v[:] = 1.0
    e = (x - y).norm(dim=-1).reshape(Ec, P * P)
    srt = e.sort(dim=-1).values
    assert bool((srt[:, 1] - srt[:, 0] > 1e-6).all()), "two equal minima"
    assert bool(((e - 0.25).abs() > 1e-6).all())
    return v, x, y


def pose_inputs(SE3, g, n, kind):
    """-> (Gs.data, Ps.data) [1, n, 7], world-to-camera like train.py:162."""
    r = lambda *s: torch.randn(*s, generator=g, dtype=DT)
    if kind in ("same",):                                  # pure translations on the x axis, spacing 2: every operation is exact
        d = torch.zeros(1, n, 7, dtype=DT)
        d[0, :, 0] = 2.0 * torch.arange(n, dtype=DT)
        d[0, :, 6] = 1.0
        return d.clone(), d
    cam = SE3.exp(r(1, n, 6) * torch.tensor([1.0, 1.0, 1.0, 0.3, 0.3, 0.3], dtype=DT))      # camera-to-world
    if kind in ("collinear", "planar"):
        lam = r(n, 1) * 2
        t = torch.tensor([[0.3, -0.2, 0.5]], dtype=DT) + lam * torch.tensor([[0.6, 0.3, -0.7]], dtype=DT)
        if kind == "planar":
            t = t + r(n, 1) * torch.tensor([[0.1, 0.9, 0.2]], dtype=DT)
        cam = SE3(torch.cat([t[None], cam.data[..., 3:]], dim=-1))
    Ps = SE3(f32(cam.inv().data))
    if kind == "identity":
        Gs = SE3.Identity(1, n, dtype=DT)
    elif kind == "twentieth":
        small = Ps.inv().scale(torch.full((1, 1), 0.05, dtype=DT))
        Gs = (SE3.exp(r(1, n, 6) * 0.002) * small).inv()
    elif kind == "same_rot":
        Gs = SE3(Ps.data.clone())
    else:
        Gs = SE3.exp(r(1, n, 6) * 0.05) * Ps
        Gs = (Gs.inv().scale(torch.full((1, 1), 0.7, dtype=DT))).inv()
    return f32(Gs.data).clone(), Ps.data


def score_inputs(g, n_patches, Ef, mode):
    kk = torch.randint(0, n_patches, (Ef,), generator=g)
    assert int(torch.bincount(kk, minlength=n_patches).max()) <= 40 and int(torch.bincount(kk).max()) > 1
    scores = f32(torch.rand(n_patches, generator=g, dtype=DT))
    scores[1], scores[4], scores[7] = 1e-8, 0.0, 5e-7      # below 1e-6: clamped, no gradient through the entropy term
    scores = f32(scores)
    assert bool((scores != 1e-6).all()) and int((scores < 1e-6).sum()) == 3
    v_full = (torch.rand(Ef, generator=g, dtype=DT) > 0.3).to(DT)
    v_full[2] = 0.5                                        # exactly 0.5 IS valid here (v_full >= 0.5)
    if mode == "none":
        v_full[:] = 0.0
    x = f32(torch.rand(Ef, P, P, 2, generator=g, dtype=DT) * 60)
    y = f32(x + torch.randn(Ef, P, P, 2, generator=g, dtype=DT) * 1.5)
    w = f32(torch.rand(Ef, 2, generator=g, dtype=DT) * 0.9 + 0.05)
    return scores, v_full, x, y, w, kk


def main():
    GU.install_shims()
    from devo.lietorch import SE3
    kabsch = reference_kabsch()
    g = torch.Generator().manual_seed(20240611)
    out, names = {}, []

    def run(name, flow, pose, score=None):
        v, x, y = flow
        x = x.clone().requires_grad_(True)
        Gd = pose[0].clone().requires_grad_(True)
        data = [v, x, y, SE3(Gd), SE3(pose[1]), torch.as_tensor(0)]
        sc = None
        if score is not None:
            sc = score[0].clone().requires_grad_(True)
            data += [sc, *score[1:], torch.zeros(0)]
        loss, stats, raw = reference_iteration(SE3, kabsch, data, 2, True)
        gx, gG = torch.autograd.grad(loss, [x, Gd], retain_graph=sc is not None, allow_unused=True)
        k = "case/" + name + "/"
        out[k + "v"], out[k + "x"], out[k + "y"] = v.numpy().astype(np.float32), x.detach().numpy().astype(np.float32), y.numpy().astype(np.float32)
        out[k + "Gs"], out[k + "Ps"] = pose[0].numpy().astype(np.float32), pose[1].numpy().astype(np.float32)
        out[k + "stats"], out[k + "loss"], out[k + "raw_scale"] = stats.numpy(), float(loss.detach()), raw
        out[k + "g_coords"] = gx.numpy() if gx is not None else np.zeros(tuple(x.shape))
        out[k + "g_Gs"] = gG.numpy()
        if sc is not None:
            out[k + "g_scores"] = torch.autograd.grad(loss, sc)[0].numpy()
            for nm, t in zip(("scores", "v_full", "x_full", "y_full", "ba_weights"), score[:5]):
                out[k + nm] = t.detach().numpy().astype(np.float32)
            out[k + "kk"] = score[5].numpy()
        names.append(name)
        return stats, raw, gG

    general3 = pose_inputs(SE3, g, 3, "general")
    tiny = flow_inputs(g, 1, "mixed")
    flows = {}
    for Ec, mode in ((1, "mixed"), (65, "mixed"), (513, "mixed"), (65, "all"), (65, "none")):
        flows[(Ec, mode)] = flow_inputs(g, Ec, mode)
        stats, _, _ = run(f"flow/{mode}_{Ec}", flows[(Ec, mode)], general3)
        assert bool(torch.isnan(stats[0])) == (mode == "none")
    poses = {}
    for n in (2, 3, 15):
        for kind in ("general", "collinear", "planar", "identity", "twentieth", "same", "same_rot"):
            poses[(kind, n)] = pose_inputs(SE3, g, n, kind)
            stats, raw, gG = run(f"pose/{kind}_{n}", tiny, poses[(kind, n)])
            s = float(stats[10])
            assert np.isfinite(s), (kind, n)
            if kind == "identity":
                assert raw == float("inf") and s == 10.0
            if kind == "twentieth":
                assert 19.0 < raw < 21.0 and s == 10.0
            if kind == "same":
                assert s == 1.0 and float(stats[1]) == 0.0 and float(gG.abs().max()) == 0.0, (n, s, float(stats[1]))
            if kind == "same_rot":
                assert abs(s - 1.0) < 1e-12 and float(stats[1]) < 1e-12
    scores = {m: score_inputs(g, 24, 300, m) for m in ("general", "none")}
    for m in scores:
        stats, _, _ = run(f"score/{m}", flows[(65, "mixed")], general3, scores[m])
        assert bool(torch.isnan(stats[9])) == (m == "none")

    # a three-iteration trajectory of 13-tuples (enet.py:369): the scorer term and the pose weight arrive in the last entry only
    entries = [(flows[(65, "all")], poses[("general", 15)]), (flows[(1, "mixed")], poses[("planar", 3)]), (flows[(513, "mixed")], poses[("collinear", 15)])]
    sc = scores["general"][0].clone().requires_grad_(True)
    leaves, total = [], 0.0
    for i, (fl, po) in enumerate(entries):
        x = fl[1].clone().requires_grad_(True)
        Gd = po[0].clone().requires_grad_(True)
        leaves += [x, Gd]
        data = [fl[0], x, fl[2], SE3(Gd), SE3(po[1]), torch.as_tensor(0), sc, *scores["general"][1:], torch.zeros(0)]
        loss, stats, _ = reference_iteration(SE3, kabsch, data, i, i == len(entries) - 1)
        total = total + loss
    grads = torch.autograd.grad(total, leaves + [sc], allow_unused=True)
    out["seq/entries"] = np.array(["flow/all_65 pose/general_15", "flow/mixed_1 pose/planar_3", "flow/mixed_513 pose/collinear_15"])
    out["seq/scorer"] = "score/general"
    out["seq/loss"], out["seq/stats"] = float(total.detach()), stats.numpy()
    for i in range(3):
        out[f"seq/g_coords{i}"] = grads[2 * i].numpy()
        out[f"seq/g_Gs{i}"] = grads[2 * i + 1].numpy() if grads[2 * i + 1] is not None else np.zeros(tuple(leaves[2 * i + 1].shape))
    out["seq/g_scores"] = grads[-1].numpy()
    out["names"] = np.array(names)
    out["weights"] = np.array([FW, PW, SW])
    path = os.path.join(ROOT, "tests", "golden", "train_loss_f64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "cases")


if __name__ == "__main__":
    main()
