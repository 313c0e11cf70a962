"""The reference's training loss (train.py:172-236) and its logged metrics (:254-266) over csrc/loss.hip.

Per update iteration the reference composes, in eager torch and lietorch: the flow term over the close edges (the smallest of the P x P
residual norms of every valid edge, averaged), the pose term (both pose sets inverted, the prediction rescaled by the Sim(3) scale of
`kabsch_umeyama` — a 3 x 3 `torch.svd` —, the pairwise error `log(dP dG^-1)` over all ordered frame pairs) and, in the last iteration,
the scorer term; then eleven `.item()` calls per step.  Here an iteration is two launches forward (four with the scorer term) and one
backward: the forward kernels keep the adjoints for a unit incoming gradient, backward scales them.  Nothing is read on the host:
`stats` stays on the device until `metrics()` copies it, once.  No CPU path.

Not a drop-in under a reference module name (the loss is inline code of train.py): INTEGRATION.md shows train.py:172-266 over
`sequence_loss` and `metrics`."""
import collections
import torch
from . import _lib as L
from . import backends

STATS = ("flow", "pose", "tr", "ro", "px1", "r1", "r2", "t1", "t2", "scores", "scale")
# the defaults of train.py's arguments (:363-365)
FLOW_WEIGHT, POSE_WEIGHT, SCORES_WEIGHT = 0.1, 10.0, 0.05


class Stats(collections.namedtuple("Stats", ("data",))):
    """One fp32 device tensor [11] with named 0-d views: flow, pose, tr, ro, px1, r1, r2, t1, t2, scores, scale."""
    __slots__ = ()

    def __getattr__(self, name):
        try:
            return self.data[STATS.index(name)]
        except ValueError:
            raise AttributeError(name) from None

    def _asdict(self):
        return {k: self.data[i] for i, k in enumerate(STATS)}


class _IterationLoss(torch.autograd.Function):
    """(coords, Gs.data, scores | None; the data tensors; the weights) -> (loss [1], stats).  Gradients reach coords, Gs.data and scores."""

    @staticmethod
    def forward(ctx, coords, Gs, scores, coords_gt, valid, Ps, full, weights, use_pose, deterministic):
        fw, pw, sw = weights
        v_full, x_full, y_full, ba_w, kk = full if scores is not None else (None,) * 5
        P, Ec, n = coords.shape[-2], valid.numel(), Gs.numel() // 7
        Ef, n_patches = (kk.numel(), scores.numel()) if scores is not None else (0, 0)
        nat = backends.native()
        with torch.cuda.device(coords.device):
            if nat is not None:
                loss, stats, state = nat.losses.forward(coords, coords_gt, valid, Gs, Ps, scores, v_full, x_full, y_full, ba_w, kk, deterministic, fw, pw, sw, use_pose)
            else:
                code = L.dtype_code(coords)
                nbytes = L.lib().devo_loss_state_bytes(Ec, n, Ef, n_patches, code)
                loss = torch.empty(1, dtype=coords.dtype, device=coords.device)
                stats = torch.empty(len(STATS), dtype=torch.float32, device=coords.device)
                state = torch.empty(nbytes, dtype=torch.uint8, device=coords.device)
                rc = L.lib().devo_loss_forward(L.ptr(coords), L.ptr(coords_gt), L.ptr(valid), Ec, P, L.ptr(Gs), L.ptr(Ps), n, L.ptr(scores), n_patches, L.ptr(v_full),
                                               L.ptr(x_full), L.ptr(y_full), L.ptr(ba_w), L.ptr(kk), Ef, int(deterministic), fw, pw, sw, int(use_pose), L.ptr(loss),
                                               L.ptr(stats), L.ptr(state), nbytes, code, L.stream())
                L.check(rc, "losses.iteration_loss")
        ctx.save_for_backward(state)
        ctx.sizes = (Ec, P, n, Ef, n_patches)
        ctx.weights = (fw, pw if use_pose else 0.0, sw)
        ctx.shapes = (coords.shape, Gs.shape, None if scores is None else scores.shape)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)                                  # (no zero-filled gradient for stats: a launch per iteration)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        if g is None:
            return (None,) * 10
        state, = ctx.saved_tensors
        Ec, P, n, Ef, n_patches = ctx.sizes
        fw, pw, sw = ctx.weights
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and n_patches > 0)
        g = g.contiguous()
        nat = backends.native()
        with torch.cuda.device(g.device):
            if nat is not None:
                gc, gG, gs = nat.losses.backward(g, state, Ec, P, n, Ef, n_patches, fw, pw, sw, *need)
            else:
                mk = lambda on, *shape: torch.empty(*shape, dtype=g.dtype, device=g.device) if on else None
                gc, gG, gs = mk(need[0], Ec, P, P, 2), mk(need[1], n, 7), mk(need[2], n_patches)
                rc = L.lib().devo_loss_backward(L.ptr(g), L.ptr(state), state.numel(), Ec, P, n, Ef, n_patches, fw, pw, sw, L.ptr(gc), L.ptr(gG), L.ptr(gs),
                                                L.dtype_code(g), L.stream())
                L.check(rc, "losses.iteration_loss backward")
        sc, sG, ss = ctx.shapes
        return (gc.view(sc) if need[0] else None, gG.view(sG) if need[1] else None, gs.view(ss) if need[2] else None, None, None, None, None, None, None, None)


def _data(G):
    return G if isinstance(G, torch.Tensor) else G.data                  # (SE3.data is the tensor on the tape; Tensor.data would leave it)


def iteration_loss(valid, coords, coords_gt, Gs, Ps, *, index, flow_weight=FLOW_WEIGHT, pose_weight=POSE_WEIGHT, scores_weight=SCORES_WEIGHT,
                   structure_only=False, scorer=None):
    """The body of train.py:176-236 for one entry of `traj`: valid [1, Ec], coords / coords_gt [1, Ec, P, P, 2], Gs / Ps SE3 (or their
    data) [1, n, 7], 2 <= n <= 128.  scorer: (scores, v_full, coords_full, coords_gt_full, ba_weights, kk) — entries 6 to 11 of a
    13-tuple — adds the scorer term (train.py:189-203; the caller passes it in the last iteration).  The pose term is weighted in
    when `not structure_only and index >= 2`; it is computed and reported either way.
    -> (loss, a 0-d tensor on the autograd tape: gradients to coords, Gs.data and scores; Stats)."""
    Gd, Pd = _data(Gs), _data(Ps)
    tensors = [valid, coords, coords_gt, Gd, Pd] + (list(scorer[:6]) if scorer is not None else [])
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"losses.iteration_loss: expected tensors, got {type(t).__name__}")
    if coords.dim() != 5 or coords.shape[0] != 1 or Gd.dim() != 3 or Gd.shape[0] != 1:
        raise ValueError(f"losses.iteration_loss: one sequence to a call (the reference takes t2[0]): coords {tuple(coords.shape)}, poses {tuple(Gd.shape)}")
    dt = coords.dtype
    if dt not in (torch.float32, torch.float64):
        raise ValueError(f"losses.iteration_loss: fp32 or fp64, got {dt}")
    if coords_gt.shape != coords.shape or Pd.shape != Gd.shape or Gd.shape[-1] != 7 or valid.numel() != coords.shape[1]:
        raise ValueError("losses.iteration_loss: shapes disagree")
    if not 2 <= Gd.shape[1] <= 128:
        raise ValueError(f"losses.iteration_loss: 2 <= n <= 128 poses, got {Gd.shape[1]}")
    L.require_gpu(*tensors)
    c = lambda t: t if (t.dtype == dt and t.is_contiguous()) else t.to(dt).contiguous()
    scores, full = None, None
    if scorer is not None:
        scores, v_full, x_full, y_full, ba_w, kk = scorer[:6]
        if not (v_full.numel() == kk.numel() and ba_w.numel() == 2 * kk.numel() and x_full.shape == y_full.shape and x_full.numel() == kk.numel() * coords[0, 0].numel()):
            raise ValueError("losses.iteration_loss: the scorer term's tensors disagree in size")
        full = (c(v_full.detach()), c(x_full.detach()), c(y_full.detach()), c(ba_w.detach()), kk if (kk.dtype == torch.int64 and kk.is_contiguous()) else kk.long().contiguous())
        scores = c(scores)
    use_pose = (not structure_only) and index >= 2
    loss, stats = _IterationLoss.apply(c(coords), c(Gd), scores, c(coords_gt.detach()), c(valid.detach()), c(Pd.detach()), full,
                                       (float(flow_weight), float(pose_weight), float(scores_weight)), bool(use_pose),
                                       torch.are_deterministic_algorithms_enabled())
    return loss.view(()), Stats(stats)


def sequence_loss(traj, *, flow_weight=FLOW_WEIGHT, pose_weight=POSE_WEIGHT, scores_weight=SCORES_WEIGHT, structure_only=False):
    """train.py:172-236 over what eVONet.forward returns: a list of (valid, coords, coords_gt, Gs, Ps, kl) (enet.py:374) or of the
    13-tuples of the scorer selector (:369), whose last entry carries the scorer term.  -> (the summed loss, the LAST iteration's Stats:
    what train.py:254-266 logs)."""
    if not traj:
        raise ValueError("losses.sequence_loss: an empty trajectory")
    total, stats = None, None
    for i, data in enumerate(traj):
        if len(data) not in (6, 13):
            raise ValueError(f"losses.sequence_loss: entries of 6 or 13 tensors (enet.py:369, :374), got {len(data)}")
        scorer = data[6:12] if (len(data) == 13 and i == len(traj) - 1) else None
        loss, stats = iteration_loss(data[0], data[1], data[2], data[3], data[4], index=i, flow_weight=flow_weight, pose_weight=pose_weight,
                                     scores_weight=scores_weight, structure_only=structure_only, scorer=scorer)
        total = loss if total is None else total + loss
    return total, stats


def metrics(stats, loss):
    """The dictionary of train.py:254-266, same keys, from ONE device -> host copy."""
    f = torch.cat([stats.data, loss.detach().reshape(1).to(torch.float32)]).tolist()
    s = dict(zip(STATS, f))
    return {"loss/train": f[-1], "loss/pose_train": s["pose"], "loss/rotation_train": s["ro"], "loss/translation_train": s["tr"], "loss/flow_train": s["flow"],
            "loss/scores_train": s["scores"], "px1": s["px1"], "r1": s["r1"], "r2": s["r2"], "t1": s["t1"], "t2": s["t2"]}
