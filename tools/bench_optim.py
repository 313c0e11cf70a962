#!/usr/bin/env python3
"""The tail of a training step on TrainNet's 102 parameter tensors (3 397 061 fp32 elements), three ways, interleaved:
  (i)   torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with torch's defaults + OneCycleLR.step()
  (ii)  the same with AdamW(fused=True)
  (iii) devo_amd.optim.AdamW(max_norm=10) + OneCycleLR.step()
Host time: a host clock around the enqueue of STEPS steps, no synchronise inside (what the training loop's thread pays).  Device time: device
events around STEPS steps enqueued BEHIND about 50 ms of matmuls, so the host is ahead and the steps run back to back on the device.
Medians over ROUNDS rounds, the variants alternating inside a round.  Launches per step: kernels torch's profiler sees in one step.
--train-step: also devo_amd.training.train_step at the benchmark's workload under optimizer="torch" and optimizer="fused", interleaved,
synchronised per step.  Results: profiles/optim.txt."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import optim, training as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--train-step", action="store_true")
ap.add_argument("--workload", default="cfg2_m80")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_optim needs a GPU"
DEV = "cuda:0"
LR, WD, CLIP, TOTAL = 8e-5, 1e-6, 10.0, 240000

net0 = T.build_trainer(DEV, 1)[0]
gen = torch.Generator(device=DEV).manual_seed(1)
grads = [torch.empty_like(q).copy_(0.05 * torch.randn(q.shape, device=DEV, generator=gen)) for q in net0.parameters()]


def variant(kind):
    ps = [torch.nn.Parameter(q.detach().clone(memory_format=torch.preserve_format)) for q in net0.parameters()]
    for q, g in zip(ps, grads):
        q.grad = g.clone(memory_format=torch.preserve_format)
    if kind == "fused-hip":
        opt = optim.AdamW(ps, lr=LR, weight_decay=WD, max_norm=CLIP)
    else:
        opt = torch.optim.AdamW(ps, lr=LR, weight_decay=WD, fused=True if kind == "torch-fused" else None)
    sched = optim.one_cycle(opt, LR, TOTAL)

    def step():
        if kind != "fused-hip":
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
        opt.step()
        sched.step()
    return step


KINDS = ("torch-default", "torch-fused", "fused-hip")
steps = {k: variant(k) for k in KINDS}
for k in KINDS:
    for _ in range(5):
        steps[k]()
torch.cuda.synchronize()
big = torch.randn(8192, 8192, device=DEV)
host, device = {k: [] for k in KINDS}, {k: [] for k in KINDS}
for r in range(args.rounds):
    order = KINDS if r % 2 == 0 else KINDS[::-1]
    for k in order:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            steps[k]()
        host[k].append((time.perf_counter() - t0) / args.steps * 1e6)
        torch.cuda.synchronize()
        for _ in range(6):
            big @ big
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            steps[k]()
        e1.record()
        torch.cuda.synchronize()
        device[k].append(e0.elapsed_time(e1) / args.steps * 1e3)

launches = {}
for k in KINDS:
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        launches[k] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()
                          and not e.name.startswith("Optimizer.step"))        # (the profiler's own annotation of Optimizer.step is no kernel)
    except Exception as exc:                                        # the profiler is not what is measured here
        launches[k] = f"not measured ({type(exc).__name__})"

n = sum(q.numel() for q in net0.parameters())
print(f"optimiser tail on TrainNet: {len(grads)} tensors, {n} fp32 elements, {args.rounds} rounds x {args.steps} steps, medians (min .. max)")
for k in KINDS:
    h, d = host[k], device[k]
    print(f"  {k:14s} host {statistics.median(h):8.1f} us ({min(h):.1f} .. {max(h):.1f})   device {statistics.median(d):8.1f} us ({min(d):.1f} .. {max(d):.1f})"
          f"   launches/step {launches[k]}")

if args.train_step:
    batch = T.make_batch(args.workload, 1234, DEV)
    runs = {}
    for kind in ("torch", "fused"):
        net, model, opt = T.build_trainer(DEV, 1, optimizer=kind)
        runs[kind] = (model, opt)
        for _ in range(3):
            T.train_step(model, opt, batch)
    torch.cuda.synchronize()
    times = {kind: [] for kind in runs}
    for r in range(8):
        for kind in (("torch", "fused") if r % 2 == 0 else ("fused", "torch")):
            model, opt = runs[kind]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T.train_step(model, opt, batch)
            torch.cuda.synchronize()
            times[kind].append((time.perf_counter() - t0) * 1e3)
    print(f"training.train_step at {args.workload} (18 iterations), synchronised per step, 8 interleaved rounds, medians (min .. max)")
    for kind, t in times.items():
        print(f"  optimizer={kind:6s} {statistics.median(t):8.2f} ms ({min(t):.2f} .. {max(t):.2f})")
