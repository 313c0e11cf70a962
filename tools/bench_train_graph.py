"""Cost of the training graph's schedule (devo/enet.py:297-339 + the edge selections of :359-369) at the training shape: N = 15 frames,
M = 80, dim 384, net in fp32, 18 iterations, the graph grows at iterations 8 .. 14 (the drop at 8 and 12).

    python tools/bench_train_graph.py                      # the table of profiles/train_graph.txt
    python tools/bench_train_graph.py --no-step            # without the training step

(a) reference: the reference's torch composition on the GPU — torch.where x 2, torch.cat x 4 (net among them), the mask gathers of a
    drop, ii.max() x 2, torch.median, and the close / far mask gathers of EVERY iteration;
(b) graph:     devo_amd.train_graph.TrainGraph.step (its lists are refreshed inside the growth; other iterations launch nothing).
An iteration's bookkeeping is timed from the host with a device synchronisation in front and behind; whole drives of the two
implementations alternate (a, b, a, b, ...), and the figures are medians over the repeats with the p90 - p10 spread beside them.
Kernel launches per iteration are counted with torch.profiler in one drive of each implementation, outside the timed repeats.
The training step: devo_amd.training.train_step on the cfg2_m80 workload, schedule="full" against schedule="reference", alternating."""
import argparse
import collections
import os
import sys
import time
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd.train_graph import TrainGraph                            # noqa: E402

DEV = "cuda"
N, M, P, DIM, INIT, WARMUP, STEPS, DROPS = 15, 80, 3, 384, 8, 8, 18, (8, 12)


def _pairs(rows, cols):
    r, c = torch.meshgrid(rows, cols, indexing="ij")
    return r.reshape(-1), c.reshape(-1)


class Reference:
    """The torch ops of enet.py:300-339, :359-369 — `where` + meshgrid index lists, `cat`, mask gathers, `max`, `median` — on GPU tensors:
    what a training loop without devo_amd.train_graph runs."""

    def __init__(self):
        self.frame_of = torch.arange(N, device=DEV).repeat_interleave(M)
        self.patch, self.target = _pairs(torch.where(self.frame_of < INIT)[0], torch.arange(INIT, device=DEV))
        self.source = self.frame_of[self.patch]

    def grow(self, f, net, poses, patches, drop):
        frame_of = self.frame_of
        p1, t1 = _pairs(torch.where(frame_of < f)[0], torch.arange(f, f + 1, device=DEV))
        p2, t2 = _pairs(torch.where(frame_of == f)[0], torch.arange(f + 1, device=DEV))
        source = torch.cat([frame_of[p1], frame_of[p2], self.source])
        target = torch.cat([t1, t2, self.target])
        patch = torch.cat([p1, p2, self.patch])
        net = torch.cat([net.new_zeros(1, len(p1) + len(p2), DIM), net], dim=1)
        if drop:
            stay = (source != f - 4) & (target != f - 4)
            source, target, patch, net = source[stay], target[stay], patch[stay], net[:, stay]
        poses[:, f] = poses[:, f - 1]
        patches[:, frame_of == f, 2] = torch.median(patches[:, (frame_of == f - 1) | (frame_of == f - 2), 2])
        self.source, self.target, self.patch = source, target, patch
        return net, source.max() + 1

    def iteration(self, t, net, poses, patches, drop):
        f = self.source.max() + 1                              # a device scalar: the comparisons below wait for it, as the reference's do
        if t >= WARMUP and f < N:
            net, f = self.grow(f, net, poses, patches, drop)
        gap = (self.source - self.target).abs()
        near = (gap > 0) & (gap <= 2)
        close = (self.source[near], self.target[near], self.patch[near])
        wide = (gap > 0) & (gap <= 16)
        far = (self.patch[wide], gap[wide])
        return net, poses, patches, (close, far)


class Graph:
    def __init__(self):
        self.g = TrainGraph(N, M, P=P, dim=DIM, init_frames=INIT, warmup=WARMUP, device=DEV)
        self.g.ii                                              # the initial graph: built here, like Reference.__init__

    def iteration(self, t, net, poses, patches, drop):
        net, poses, patches = self.g.step(t, net, poses, patches, drop=drop)
        return net, poses, patches, (self.g.close, self.g.far)


def kind(t):
    return "no growth" if not (WARMUP <= t < WARMUP + N - INIT) else ("growth + drop" if t in DROPS else "growth")


def drive(impl, poses0, patches0, timed=True):
    s = impl()
    net = torch.zeros(1, INIT * INIT * M, DIM, device=DEV)
    poses, patches = poses0.clone(), patches0.clone()
    times = []
    for t in range(STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net, poses, patches, _ = s.iteration(t, net, poses, patches, t in DROPS)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
        net = net + 1.0                                        # (the operator returns a new tensor every iteration)
    return times


def launches(impl, poses0, patches0):
    from torch.profiler import profile, ProfilerActivity
    from torch.autograd import DeviceType
    kernels = lambda prof: sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.key and "Memset" not in e.key)      # device kernels, not the runtime's API calls
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        s = impl()
        torch.cuda.synchronize()
    net = torch.zeros(1, INIT * INIT * M, DIM, device=DEV)
    poses, patches = poses0.clone(), patches0.clone()
    out = collections.defaultdict(list)
    out["initial graph"].append(kernels(prof))
    for t in range(STEPS):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            net, poses, patches, _ = s.iteration(t, net, poses, patches, t in DROPS)
            torch.cuda.synchronize()
        out[kind(t)].append(kernels(prof))
    return {k: float(np.median(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-repeats", type=int, default=6)
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(1)
    poses0, patches0 = torch.randn(1, N, 7, generator=gen).to(DEV), torch.rand(1, N * M, 3, P, P, generator=gen).to(DEV)
    impls = {"reference": Reference, "graph": Graph}
    times = {k: collections.defaultdict(list) for k in impls}
    totals = {k: [] for k in impls}
    for r in range(a.warmup + a.repeats):
        for name, impl in impls.items():
            ts = drive(impl, poses0, patches0)
            if r >= a.warmup:
                for t, us in enumerate(ts):
                    times[name][kind(t)].append(us)
                totals[name].append(sum(ts))
    try:
        counts = {name: launches(impl, poses0, patches0) for name, impl in impls.items()}
    except Exception as e:                                     # the profiler is optional: the timings stand without it
        print(f"# torch.profiler did not run ({type(e).__name__}: {e}): kernels per iteration not counted")
        counts = {name: {} for name in impls}
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    print(f"# python tools/bench_train_graph.py  ({torch.cuda.get_device_name(0)}; N = {N}, M = {M}, dim {DIM}, fp32, {STEPS} iterations, growths at {WARMUP} .. {WARMUP + N - INIT - 1}, "
          f"the drop at {DROPS}; {a.repeats} alternating drives after {a.warmup} warm-up drives; us per iteration of bookkeeping, host wall time between two device synchronisations)")
    print(f"{'iteration':>14} {'impl':>10} {'kernels':>8} {'min':>9} {'median':>9} {'p90-p10':>9}")
    for k in ("growth", "growth + drop", "no growth"):
        for name in impls:
            v = times[name][k]
            c = counts[name].get(k)
            print(f"{k:>14} {name:>10} {('%.0f' % c) if c is not None else 'n/a':>8} {min(v):>9.1f} {q(v, 0.5):>9.1f} {q(v, 0.9) - q(v, 0.1):>9.1f}", flush=True)
        ref, g = times["reference"][k], times["graph"][k]
        print(f"{'':>14} {'ratio':>10} {'':>8} {min(ref) / min(g):>8.2f}x {q(ref, 0.5) / q(g, 0.5):>8.2f}x")
    for name in impls:
        c = counts[name].get("initial graph")
        print(f"{'initial graph':>14} {name:>10} {('%.0f' % c) if c is not None else 'n/a':>8}")
    for name in impls:
        v = totals[name]
        print(f"{'whole drive':>14} {name:>10} {'':>8} {min(v):>9.1f} {q(v, 0.5):>9.1f} {q(v, 0.9) - q(v, 0.1):>9.1f}")
    print(f"{'':>14} {'ratio':>10} {'':>8} {min(totals['reference']) / min(totals['graph']):>8.2f}x {q(totals['reference'], 0.5) / q(totals['graph'], 0.5):>8.2f}x")
    if a.no_step:
        return
    from devo_amd import training as T
    net, model, opt = T.build_trainer(DEV, 1)
    batch = T.make_batch("cfg2_m80", 1234, DEV)
    step = {"full": [], "reference": []}
    np.random.seed(0)
    for r in range(2 + a.step_repeats):
        for sched in step:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            T.train_step(model, opt, batch, iters=STEPS, schedule=sched)
            torch.cuda.synchronize()
            if r >= 2:
                step[sched].append((time.perf_counter() - t0) * 1e3)
    print(f"# devo_amd.training.train_step, workload cfg2_m80 (n = {batch['n']}, M = {batch['M']}), {STEPS} iterations, objective bench; ms per step, {a.step_repeats} alternating steps after 2 warm-up steps;")
    print("# schedule=\"reference\" starts on 8 frames (5 120 edges) and reaches the full graph (18 000 edges) at iteration 14; the drop is drawn with probability 0.1 per growth")
    for sched, v in step.items():
        print(f"{'train step':>14} {sched:>10} {'':>8} {min(v):>9.1f} {q(v, 0.5):>9.1f} {q(v, 0.9) - q(v, 0.1):>9.1f}")


if __name__ == "__main__":
    main()
