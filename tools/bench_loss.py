#!/usr/bin/env python3
"""The training loss of one update iteration (train.py:176-236), forward + backward, at the training shape (n = 15 frames, M = 80
patches a frame, the full graph's close edges and its |dij| <= 16 edges): devo_amd.losses (csrc/loss.hip) against the SAME objective
composed in torch on the GPU — devo_amd.lietorch group ops + torch.linalg.svdvals, written here, not in the package.

Per variant and repeat: GPU time between two events around `iters` iterations and the host time to enqueue them (no wait inside);
the variants alternate repeat by repeat; medians and the spread (max - min over the repeats) are printed, then the training step under
objective="reference" against objective="bench" (--step).  python tools/bench_loss.py [--repeats 15] [--iters 20] [--step]"""
import argparse
import os
import statistics
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import losses, synth                        # noqa: E402
from devo_amd.lietorch import SE3                         # noqa: E402

DEV = "cuda"


def torch_loss(v, x, y, Gs, Ps, index, scorer, fw=0.1, pw=10.0, sw=0.05, P=3):
    valid = (v > 0.5).reshape(-1)
    e = (x - y).norm(dim=-1)
    flow = e.reshape(-1, P * P)[valid].min(dim=-1).values.mean()
    sc = 0.0
    if scorer is not None:
        scores, vf, xf, yf, w, kk = scorer
        ok = (vf >= 0.5).reshape(-1)
        ef = (xf - yf).norm(dim=-1).reshape(-1, P * P)[ok].min(dim=-1).values
        sc = ((-0.5 * w.view(-1, 2)[ok].mean(dim=-1).log() + 1) * scores.view(-1)[kk[ok]] * ef).mean() + (-torch.clamp(scores, min=1e-6).log()).mean()
    n = Gs.shape[1]
    ii, jj = torch.meshgrid(torch.arange(n, device=DEV), torch.arange(n, device=DEV), indexing="ij")
    keep = ii != jj
    ii, jj = ii[keep], jj[keep]
    P1, P2 = SE3(Gs).inv(), SE3(Ps).inv()
    t1, t2 = P1.data[0, :, :3].detach(), P2.data[0, :, :3]
    c1, c2 = t1 - t1.mean(0), t2 - t2.mean(0)
    s = ((c2.norm(dim=1) ** 2).mean() / torch.linalg.svdvals(c2.T @ c1 / n).sum()).clamp(max=10.0)
    P1 = P1.scale(s.view(1, 1))
    e1 = ((P1[:, ii].inv() * P1[:, jj]) * (P2[:, ii].inv() * P2[:, jj]).inv()).log()
    pose = e1[..., 0:3].norm(dim=-1).mean() + e1[..., 3:6].norm(dim=-1).mean()
    loss = fw * flow + sw * sc
    return loss + pw * pose if index >= 2 else loss


def make_inputs(n=15, M=80, seed=3):
    g = torch.Generator().manual_seed(seed)
    ii, jj, kk = synth.full_graph(n, M)
    dij = (ii - jj).abs()
    close, far = (dij > 0) & (dij <= 2), (dij > 0) & (dij <= 16)
    Ec, Ef = int(close.sum()), int(far.sum())
    d = lambda t: t.to(DEV)
    x = d(torch.rand(1, Ec, 3, 3, 2, generator=g) * 60)
    y = x + d(torch.randn(1, Ec, 3, 3, 2, generator=g))
    v = d((torch.rand(1, Ec, generator=g) > 0.2).float())
    Ps = d(synth.make_poses(n, seed))
    Gs = Ps.clone()
    Gs[:, 1:, :3] += 0.01 * d(torch.randn(1, n - 1, 3, generator=g))
    xf = d(torch.rand(Ef, 3, 3, 2, generator=g) * 60)
    scorer = (d(torch.rand(n * M, generator=g)), d((torch.rand(Ef, generator=g) > 0.2).float()), xf, xf + d(torch.randn(Ef, 3, 3, 2, generator=g)),
              d(torch.rand(Ef, 2, generator=g) * 0.9 + 0.05), d(kk[far]))
    return v, x, y, Gs, Ps, scorer, Ec, Ef


def one_iteration(kind, v, x, y, Gs, Ps, scorer):
    x = x.detach().requires_grad_(True)
    Gs = Gs.detach().requires_grad_(True)
    if scorer is not None:
        scorer = (scorer[0].detach().requires_grad_(True),) + scorer[1:]
    if kind == "hip":
        loss = losses.iteration_loss(v, x, y, Gs, Ps, index=2, scorer=scorer)[0]
    else:
        loss = torch_loss(v, x, y, Gs, Ps, 2, scorer)
    loss.backward()


def measure(kind, args, iters, scorer_on):
    v, x, y, Gs, Ps, scorer = args
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        one_iteration(kind, v, x, y, Gs, Ps, scorer if scorer_on else None)
    b.record()
    host = (time.perf_counter() - t0) / iters * 1e6
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3, host


def report(tag, rows):
    med = lambda k, i: statistics.median(r[i] for r in rows[k])
    spread = lambda k, i: max(r[i] for r in rows[k]) - min(r[i] for r in rows[k])
    for i, clock in enumerate(("GPU", "host")):
        h, t = med("hip", i), med("torch", i)
        print(f"{tag:28s} {clock:4s} us/iteration: hip {h:9.1f} (spread {spread('hip', i):7.1f})   torch {t:9.1f} (spread {spread('torch', i):7.1f})   "
              f"torch / hip = {t / h:6.2f}   gap {t - h:9.1f} vs spreads {spread('hip', i) + spread('torch', i):8.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also the training step, objective reference against bench")
    ap.add_argument("--step-iters", type=int, default=18)
    a = ap.parse_args()
    *args, Ec, Ef = make_inputs()
    print(f"n = 15, M = 80: {Ec} close edges, {Ef} edges with |dij| <= 16, {a.repeats} interleaved repeats of {a.iters} iterations")
    for scorer_on in (False, True):
        for kind in ("hip", "torch"):
            measure(kind, args, 3, scorer_on)              # warm-up
        rows = {"hip": [], "torch": []}
        for _ in range(a.repeats):
            for kind in ("hip", "torch"):
                rows[kind].append(measure(kind, args, a.iters, scorer_on))
        report("with the scorer term" if scorer_on else "flow + pose terms", rows)
    if a.step:
        from devo_amd import training as T
        net, model, opt = T.build_trainer(DEV, 1)
        batch = T.make_batch("cfg2_m80", 1234, DEV)
        rows = {"bench": [], "reference": []}
        for obj in rows:
            T.train_step(model, opt, batch, iters=a.step_iters, objective=obj)
        for _ in range(max(5, a.repeats // 2)):
            for obj in rows:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                T.train_step(model, opt, batch, iters=a.step_iters, objective=obj)
                torch.cuda.synchronize()
                rows[obj].append((time.perf_counter() - t0) * 1e3)
        for obj, r in rows.items():
            print(f"train_step objective={obj:9s} ms: median {statistics.median(r):8.2f}  min {min(r):8.2f}  max {max(r):8.2f}  ({len(r)} interleaved steps of {a.step_iters} iterations)")
        print(f"reference - bench = {statistics.median(rows['reference']) - statistics.median(rows['bench']):.2f} ms; spread of the bench step {max(rows['bench']) - min(rows['bench']):.2f} ms")


if __name__ == "__main__":
    main()
