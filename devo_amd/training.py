"""Training step of the update + bundle-adjustment path under data parallelism (BASELINE.json configurations 3 and 4).

What the reference trains (train.py:31-42, 90-107, 172-246; devo/enet.py:203-370): one process per GPU, `DDP(net)`, every
rank draws its own sequences (DistributedSampler), runs the recurrent update for STEPS iterations — reprojection, 2-level
correlation lookup (gradients through 20 % of the edges, correlation.py:20-25), Update operator, two differentiable
Gauss-Newton steps — accumulates flow + pose losses, and `loss.backward()` all-reduces ONE bucket of 3 397 061 fp32
gradients (13.59 MB: Update 3 004 804 + fnet 184 576 + inet 201 216 + scorer 6 465) over NCCL = RCCL.

Here the same step runs on this repo's path: devo_amd.patchifier (the two encoders + scorer through MIOpen, HIP gathers),
projective_ops / altcorr / update / ba (HIP kernels + autograd) on synthetic TartanAir-shaped inputs (random voxel
grids, the synthetic trajectory's poses and patch centres).  The module tree is the reference's (`update`, `patchify.fnet`,
`patchify.inet`, `patchify.scorer`): the gradient bucket DDP all-reduces is the reference's by construction.
"""
import numpy as np
import torch
import torch.nn as nn

from . import synth

N_FNET, N_INET, N_SCORER = 184_576, 201_216, 6_465          # parameter counts of the modules this path does not build
N_TOTAL = 3_397_061
FUSED_LOOKUP = __import__("os").environ.get("DEVO_TRAIN_FUSED_LOOKUP", "1") != "0"     # 0: two altcorr.corr calls + torch.stack, as enet.py:203-216 writes it


class TrainNet(nn.Module):
    """The parameters the reference's DDP wraps (eVONet, enet.py:218-233): `patchify` (fnet, inet, scorer — devo_amd.patchifier)
    and `update` (devo_amd.update.Update), same names.  `norm` and `randaug` are eVONet's (enet.py:218-233, train.py:381-382): how
    the voxel grids are normalised before the patchifier, and whether training steps augment them (normalise_images)."""

    NORMS = ("none", "rescale", "norm", "standard", "std", "standard2", "std2")

    def __init__(self, p=3, dim=384, norm="none", randaug=False):
        super().__init__()
        if norm not in self.NORMS:
            raise NotImplementedError(f"norm {norm!r} is not implemented: one of {self.NORMS}")
        from .update import Update
        from .patchifier import Patchifier
        self.patchify = Patchifier(patch_size=p, dim_inet=dim, dim_fnet=128, dim=32, patch_selector="scorer")
        self.update = Update(p, dim)
        self.P, self.dim = p, dim
        self.norm, self.randaug = norm, randaug

    def num_parameters(self):
        return sum(q.numel() for q in self.parameters())

    def normalise_images(self, images):
        """enet.py:245-266: images [b, n, bins, h, w] normalised by `norm` (none, rescale / norm, standard / std: frame-wise std,
        standard2 / std2: sequence-wise std); then, with `randaug` in training mode, on a third of the calls (np.random.rand() < 0.33)
        events.voxel_augment (a random op and factor from torch's CPU generator), which like the reference raises for a norm that is
        neither a rescale nor contains 'std'."""
        from . import events
        if self.norm == "none":
            pass
        elif self.norm in ("rescale", "norm"):
            images = events.rescale(images)
        elif self.norm in ("standard", "std"):
            images = events.std(images, sequence=False)
        elif self.norm in ("standard2", "std2"):
            images = events.std(images)
        else:
            raise NotImplementedError(f"norm {self.norm!r} is not implemented")
        if self.training and self.randaug:
            if np.random.rand() < 0.33:
                if self.norm in ("rescale", "norm"):
                    images = events.voxel_augment(images, rescaled=True)
                elif "std" in self.norm:
                    images = events.voxel_augment(images, rescaled=False)
                else:
                    raise NotImplementedError(f"randaug with norm {self.norm!r} is not implemented")
        return images

    OBJECTIVES = ("bench", "reference")

    SCHEDULES = ("full", "reference")

    def forward(self, batch, iters=18, corr_dropout=0.2, flow_weight=0.1, pose_weight=10.0, objective="bench", schedule="full", init_frames=None, warmup=8):
        """One sequence (batch 1) through `iters` update iterations on its patch graph -> scalar loss
        (enet.py:300-370 + train.py:172-236).  objective: "bench", the simplified composition below (what
        bench.py --mode train measures), or "reference", the reference's loss through devo_amd.losses (scale-aligned pose term, the
        scorer term in the last iteration, train.py's default scores weight).  schedule: "full", every iteration on the batch's fixed
        full graph, or "reference", the reference's growing graph (enet.py:297-339) driven by devo_amd.train_graph.TrainGraph: the
        batch's ii / jj / kk are ignored, the graph starts on init_frames (default min(8, n)) frames and grows by one frame per
        iteration from iteration `warmup` on."""
        if objective not in self.OBJECTIVES:
            raise ValueError(f"objective {objective!r}: one of {self.OBJECTIVES}")
        if schedule not in self.SCHEDULES:
            raise ValueError(f"schedule {schedule!r}: one of {self.SCHEDULES}")
        if schedule == "reference" and "wiring_check" not in batch:
            return self._forward_growing(batch, iters, corr_dropout, flow_weight, pose_weight, objective, init_frames, warmup)
        if "wiring_check" in batch:
            # not a training step: sum(parameters) * factor, so that a CPU / gloo run can check the DDP wiring of THIS module
            # (every parameter in the all-reduced bucket) without the HIP kernels — tests/test_distributed_gloo.py
            return sum((q * float(batch["wiring_check"])).sum() for q in self.parameters())
        from . import altcorr, projective_ops as pops
        from .ba import BA
        from .lietorch import SE3
        b = batch
        ii, jj, kk = b["ii"], b["jj"], b["kk"]
        E, n = ii.numel(), b["poses_gt"].shape[1]
        # enet.py:279-291: features, patch gathers and scores from the voxel grids; the patch centres are the synthetic
        # trajectory's (so that the ground-truth patches of the flow loss belong to them), the scorer is evaluated there
        fmap, gmap, imap, _, _, scores = self.patchify(self.normalise_images(b["images"]), b["M"], coords=b["centres"])
        pyramid = [altcorr.channels_last(fmap), altcorr.channels_last(torch.nn.functional.avg_pool2d(fmap[0], 4, 4)[None])]   # enet.py:207-210
        imap = imap.view(1, -1, self.dim)
        Ps = SE3(b["poses_gt"])
        Gs = SE3(b["poses0"].clone())
        patches = b["patches0"].clone()
        net = torch.zeros(1, E, self.dim, device=ii.device)
        inp = torch.index_select(imap, 1, kk)
        bounds = [-64, -64, b["W"] + 64, b["H"] + 64]
        dij = (ii - jj).abs()
        close = (dij > 0) & (dij <= 2)
        ci, cj, ck = ii[close], jj[close], kk[close]
        with torch.no_grad():
            coords_gt, valid_gt = pops.transform(Ps, b["patches_gt"], b["intr"], ci, cj, ck, valid=True)[:2]
        if objective == "reference":
            from . import losses
            far = ((dij > 0) & (dij <= 16)).nonzero().squeeze(1)         # enet.py:368: the edges of the scorer term
            fi16, fj16, fk16 = ii[far], jj[far], kk[far]
            with torch.no_grad():
                coords_gt_far, valid_far = pops.transform(Ps, b["patches_gt"], b["intr"], fi16, fj16, fk16, valid=True)[:2]
        fi, fj = torch.meshgrid(torch.arange(n, device=ii.device), torch.arange(n, device=ii.device), indexing="ij")
        fk = fi != fj
        fi, fj = fi[fk], fj[fk]
        loss = 0.0
        for it in range(iters):
            Gs = SE3(Gs.data.detach())
            patches = patches.detach()
            coords = pops.transform(Gs, patches, b["intr"], ii, jj, kk)
            coords1 = coords.permute(0, 1, 4, 2, 3).contiguous()
            if FUSED_LOOKUP:                                           # enet.py:203-216 as one launch (altcorr.CorrPyramidLayer)
                corr = altcorr.corr_pyramid(gmap, pyramid, coords1, kk, jj, b["R"], (1, 4), dropout=corr_dropout)
            else:
                corr = torch.stack([altcorr.corr(gmap, pyramid[0], coords1 / 1, kk, jj, b["R"], corr_dropout),
                                    altcorr.corr(gmap, pyramid[1], coords1 / 4, kk, jj, b["R"], corr_dropout)], -1).view(1, E, -1)
            net, (delta, weight, _) = self.update(net, inp, corr, None, ii, jj, kk)
            target = coords[..., self.P // 2, self.P // 2, :] + delta
            for _ in range(2):
                Gs, patches = BA(Gs, patches, b["intr"], target, weight, 1e-4, ii, jj, kk, bounds, ep=10.0, fixedp=1, n_frames=n)
            # flow loss over the close edges (train.py:177-181), pose loss over all frame pairs (:199-225, without the scale alignment)
            cf = pops.transform(Gs, patches, b["intr"], ci, cj, ck)
            if objective == "reference":                               # enet.py:362-369 + train.py:176-236
                scorer = None
                if it == iters - 1:
                    with torch.no_grad():
                        coords_far = pops.transform(Gs, patches, b["intr"], fi16, fj16, fk16)
                    scorer = (scores, valid_far[0], coords_far[0], coords_gt_far[0], torch.index_select(weight.detach()[0], 0, far), fk16)
                loss = loss + losses.iteration_loss(valid_gt, cf, coords_gt, Gs, Ps, index=it, flow_weight=flow_weight, pose_weight=pose_weight, scorer=scorer)[0]
                continue
            e = (cf - coords_gt).norm(dim=-1).reshape(-1, self.P * self.P)
            ok = valid_gt.reshape(-1) > 0.5
            flow_loss = (e.min(dim=-1).values * ok).sum() / ok.sum().clamp(min=1)
            P1, P2 = Gs.inv(), Ps.inv()
            take = lambda G, idx: SE3(torch.index_select(G.data, 1, idx))
            dP = take(P1, fi).inv() * take(P1, fj)
            dG = take(P2, fi).inv() * take(P2, fj)
            e1 = (dP * dG.inv()).log()
            pose_loss = e1[..., 0:3].norm(dim=-1).mean() + e1[..., 3:6].norm(dim=-1).mean()
            loss = loss + flow_weight * flow_loss
            if it >= 2:
                loss = loss + pose_weight * pose_loss
        if objective == "reference":
            return loss
        return loss + 1e-3 * scores.mean()                      # (the reference's scorer term, train.py:226-232, reduced to a mean)

    def _forward_growing(self, b, iters, corr_dropout, flow_weight, pose_weight, objective, init_frames, warmup):
        """forward() under schedule="reference": enet.py:297-370.  The graph is `g`'s in every iteration: a growth (g.step) prepends the
        new frame's edges, extends net with zero rows (gradient flows through), copies the previous pose and takes the depth median; the
        drop is drawn here, only inside a growth (the reference's draw order, enet.py:331).  The flow term runs on g.close, the pose term
        on the g.n frames of the graph, the scorer term (last iteration) on g.far.  The per-iteration body (lookup, operator, two BA
        steps, the two objectives) is forward()'s, written out a second time so that the "full" path keeps its exact sequence of calls:
        a change to one of the two loops belongs in the other as well."""
        from . import altcorr, projective_ops as pops
        from .ba import BA
        from .lietorch import SE3
        n, M = b["poses_gt"].shape[1], b["M"]
        dev = b["poses_gt"].device
        from . import train_graph
        g = train_graph.TrainGraph(n, M, P=self.P, dim=self.dim, init_frames=min(8, n) if init_frames is None else init_frames, warmup=warmup, device=dev)
        fmap, gmap, imap, _, _, scores = self.patchify(self.normalise_images(b["images"]), M, coords=b["centres"])
        pyramid = [altcorr.channels_last(fmap), altcorr.channels_last(torch.nn.functional.avg_pool2d(fmap[0], 4, 4)[None])]   # enet.py:207-210
        imap = imap.view(1, -1, self.dim)
        Ps = SE3(b["poses_gt"])
        poses = b["poses0"].clone()
        patches = b["patches0"].clone()
        net = torch.zeros(1, len(g), self.dim, device=dev)
        bounds = [-64, -64, b["W"] + 64, b["H"] + 64]
        if objective == "reference":
            from . import losses
        loss = 0.0
        for it in range(iters):
            poses, patches = poses.detach(), patches.detach()
            if g.grows(it):                                           # enet.py:319-339
                net, poses, patches = g.step(it, net, poses, patches, drop=np.random.rand() < 0.1)
            Gs = SE3(poses)
            ii, jj, kk, close = g.ii, g.jj, g.kk, g.close
            E, nf = ii.numel(), g.n
            coords = pops.transform(Gs, patches, b["intr"], ii, jj, kk)
            coords1 = coords.permute(0, 1, 4, 2, 3).contiguous()
            if FUSED_LOOKUP:
                corr = altcorr.corr_pyramid(gmap, pyramid, coords1, kk, jj, b["R"], (1, 4), dropout=corr_dropout)
            else:
                corr = torch.stack([altcorr.corr(gmap, pyramid[0], coords1 / 1, kk, jj, b["R"], corr_dropout),
                                    altcorr.corr(gmap, pyramid[1], coords1 / 4, kk, jj, b["R"], corr_dropout)], -1).view(1, E, -1)
            net, (delta, weight, _) = self.update(net, torch.index_select(imap, 1, kk), corr, None, ii, jj, kk)
            target = coords[..., self.P // 2, self.P // 2, :] + delta
            for _ in range(2):
                Gs, patches = BA(Gs, patches, b["intr"], target, weight, 1e-4, ii, jj, kk, bounds, ep=10.0, fixedp=1, n_frames=nf)
            poses = Gs.data
            with torch.no_grad():                                      # enet.py:366: the truth on the CURRENT close edges
                coords_gt, valid_gt = pops.transform(Ps, b["patches_gt"], b["intr"], close.ii, close.jj, close.kk, valid=True)[:2]
            cf = pops.transform(Gs, patches, b["intr"], close.ii, close.jj, close.kk)
            Gn, Pn = SE3(Gs.data[:, :nf]), SE3(Ps.data[:, :nf])        # enet.py:369: Gs[:, :n], Ps[:, :n]
            if objective == "reference":                               # enet.py:362-369 + train.py:176-236
                scorer = None
                if it == iters - 1:
                    far = g.far
                    with torch.no_grad():
                        coords_far = pops.transform(Gs, patches, b["intr"], far.ii, far.jj, far.kk)
                        coords_gt_far, valid_far = pops.transform(Ps, b["patches_gt"], b["intr"], far.ii, far.jj, far.kk, valid=True)[:2]
                    scorer = (scores, valid_far[0], coords_far[0], coords_gt_far[0], torch.index_select(weight.detach()[0], 0, far.pos), far.kk)
                loss = loss + losses.iteration_loss(valid_gt, cf, coords_gt, Gn, Pn, index=it, flow_weight=flow_weight, pose_weight=pose_weight, scorer=scorer)[0]
                continue
            e = (cf - coords_gt).norm(dim=-1).reshape(-1, self.P * self.P)
            ok = valid_gt.reshape(-1) > 0.5
            flow_loss = (e.min(dim=-1).values * ok).sum() / ok.sum().clamp(min=1)
            q = torch.arange(nf * (nf - 1), device=dev)               # the ordered frame pairs fi != fj in closed form (no mask gather)
            fi, r = q // (nf - 1), q % (nf - 1)
            fj = r + (r >= fi)
            P1, P2 = Gn.inv(), Pn.inv()
            take = lambda G, idx: SE3(torch.index_select(G.data, 1, idx))
            e1 = ((take(P1, fi).inv() * take(P1, fj)) * (take(P2, fi).inv() * take(P2, fj)).inv()).log()
            pose_loss = e1[..., 0:3].norm(dim=-1).mean() + e1[..., 3:6].norm(dim=-1).mean()
            loss = loss + flow_weight * flow_loss
            if it >= 2:
                loss = loss + pose_weight * pose_loss
        if objective == "reference":
            return loss
        return loss + 1e-3 * scores.mean()


def make_batch(workload="cfg2_m80", seed=1234, device="cuda"):
    """One synthetic training sequence: features, patches with perturbed depths, identity-initialised poses,
    ground-truth poses / patches, the full patch graph."""
    cfg = synth.workload(workload)
    n, M, H, W, C, R = cfg["n"], cfg["M"], cfg["H"], cfg["W"], cfg["C"], cfg["R"]
    dev = torch.device(device)
    from . import altcorr
    poses_gt = synth.make_poses(n, seed)
    patches_gt, centres = synth.make_patches(n, M, H, W, seed=seed)
    intr = synth.make_intrinsics(n, H, W)
    ii, jj, kk = synth.full_graph(n, M)
    g = torch.Generator().manual_seed(seed + 7)
    images = torch.randn(1, n, 5, 4 * H, 4 * W, generator=g)                                  # event voxel grids, 5 bins (std-normalised)
    patches0 = patches_gt.clone()
    patches0[:, :, 2] = torch.rand(1, n * M, 1, 1, generator=g).expand(1, n * M, 3, 3)       # enet.py:294-295: random initial depth
    poses0 = poses_gt.clone()
    poses0[:, 1:, :3] += 0.01 * torch.randn(1, n - 1, 3, generator=g)                         # start near, not at, the truth
    d = lambda t: t.to(dev)
    cx = patches_gt[0, :, 0, 1, 1].round().long().view(n, M).clamp(1, W - 2)                  # patch centres, feature-map pixels
    cy = patches_gt[0, :, 1, 1, 1].round().long().view(n, M).clamp(1, H - 2)
    return dict(images=d(images), centres=(d(cx), d(cy)),
                poses_gt=d(poses_gt), poses0=d(poses0), patches_gt=d(patches_gt), patches0=d(patches0), intr=d(intr),
                ii=d(ii), jj=d(jj), kk=d(kk), H=H, W=W, R=R, n=n, M=M, E=int(ii.numel()))


def build_trainer(device, world_size, lr=8e-5, seed=0, ddp=None, norm="none", randaug=False, optimizer="torch", total_steps=None, clip=10.0):
    """net (DDP-wrapped when world_size > 1, train.py:106-107; ddp=True: also at world size 1, given a process group), AdamW (train.py:109).
    norm, randaug: TrainNet's.  optimizer: "torch" (torch.optim.AdamW; train_step clips in front of it) or "fused" (devo_amd.optim.AdamW with
    max_norm = clip: clip and step in two launches).  total_steps: also build the reference's OneCycleLR (train.py:110-111) and return it as a
    fourth value."""
    if optimizer not in ("torch", "fused"):
        raise ValueError(f"build_trainer: optimizer {optimizer!r} (torch or fused)")
    torch.manual_seed(seed)                                   # identical initial weights on every rank (train.py:41)
    net = TrainNet(norm=norm, randaug=randaug).to(device).train()
    model = net
    if world_size > 1 or ddp:
        from torch.nn.parallel import DistributedDataParallel as DDP
        dev = torch.device(device)
        model = DDP(net, device_ids=[dev.index] if dev.type == "cuda" else None, find_unused_parameters=False)
    if optimizer == "fused":
        from . import optim
        named = list(model.named_parameters())
        opt = optim.AdamW([q for _, q in named], lr=lr, weight_decay=1e-6, max_norm=clip, names=[k for k, _ in named])
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-6)
    if total_steps is None:
        return net, model, opt
    from . import optim
    return net, model, opt, optim.one_cycle(opt, lr, total_steps)


def train_step(model, opt, batch, iters=18, clip=10.0, objective="bench", schedule="full", scheduler=None, **schedule_args):
    """optimizer.zero_grad -> forward -> backward (DDP: gradient all-reduce) -> clip -> step -> scheduler.step (train.py:166-250).  An
    optimiser that clips itself (devo_amd.optim.AdamW with max_norm) is not clipped for again.  objective, schedule (and init_frames / warmup
    through schedule_args): TrainNet.forward's."""
    opt.zero_grad(set_to_none=True)
    loss = model(batch, iters=iters, objective=objective, schedule=schedule, **schedule_args)
    loss.backward()
    if getattr(opt, "max_norm", None) is None:
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
    opt.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach()


def save_checkpoint(path, steps, model, opt, scheduler=None):
    """train.py:275-280: {'steps', 'model_state_dict' (of the bare module under DDP), 'optimizer_state_dict', 'scheduler_state_dict'}.  Either
    optimiser writes torch.optim.AdamW's format, so a checkpoint of one resumes in the other."""
    net = model.module if hasattr(model, "module") else model
    ckpt = {"steps": int(steps), "model_state_dict": net.state_dict(), "optimizer_state_dict": opt.state_dict()}
    if scheduler is not None:
        ckpt["scheduler_state_dict"] = scheduler.state_dict()
    torch.save(ckpt, path)


def load_checkpoint(path, model, opt=None, scheduler=None):
    """train.py:114-138 -> the checkpoint's step count (0 when it has none).  A checkpoint without 'model_state_dict' is the legacy form, a
    bare state dict: 'module.' is stripped from its keys and only entries whose name and shape match the model are taken (train.py:120-132)."""
    ckpt = torch.load(path)
    net = model.module if hasattr(model, "module") else model
    if "model_state_dict" in ckpt:
        net.load_state_dict(ckpt["model_state_dict"])
    else:
        have = net.state_dict()
        renamed = {k.replace("module.", ""): v for k, v in ckpt.items()}
        have.update({k: v for k, v in renamed.items() if k in have and have[k].shape == v.shape})
        net.load_state_dict(have, strict=False)
    if opt is not None and "optimizer_state_dict" in ckpt:
        opt.load_state_dict(ckpt["optimizer_state_dict"])
    if scheduler is not None and "scheduler_state_dict" in ckpt:
        scheduler.load_state_dict(ckpt["scheduler_state_dict"])
    return int(ckpt["steps"]) if "steps" in ckpt else 0
