"""Patch selection and its tail (score gather, xy, patches, index) per call: devo_amd.select (one launch, csrc/select.hip) against the torch
composition it replaces in Patchifier.forward (devo_amd.patchifier.select + the lines behind it; what DEVO_PATCHIFIER_SELECT=0 runs).

    python tools/bench_select.py                            # the table of profiles/patch_select.txt
    python tools/bench_select.py --out profiles/patch_select.txt

Shapes: the scorer's map of a 480 x 640 input, 118 x 158, one frame, M = 96 for 'multi', 'topk', 'nms' on the 2 x 2 grid (evaluation, one
frame per call); 15 frames, M = 80 for '3xrandom' (a training clip).  A batch of --calls calls is timed on the host clock: `host` until the
last call has returned (what the call costs the Python thread), `wall` until the device has finished as well.  Batches of the two paths
alternate (kernel, composition, kernel, ...) after a warm-up batch each; medians over the batches with the p90 - p10 spread beside them.
Launches per call: GPU activities (kernels and copies) the profiler records over 5 calls.  Both paths return the same tensors for 'topk' and
'nms' (checked here); 'multi' and '3xrandom' draw from different random streams."""
import argparse
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from devo_amd import patchifier as PF                                  # noqa: E402
from devo_amd import select as S                                       # noqa: E402

P = 3


def composition(smap, M, mode):
    """Patchifier.forward's scorer branch behind the score map, as the torch composition (patchifier.py: the selection, the score gather, the
    closed-form patches, index)."""
    _, n, h, w = smap.shape
    dev = smap.device
    if mode == "3xrandom":
        x, y, scores = PF.select_three_x_random(smap, M)
    else:
        x, y = PF.select(smap, M, mode, True)
        scores = smap[0][torch.arange(n, device=dev)[:, None], y, x]
        x, y = x + 1, y + 1
    xy = torch.stack([x, y], dim=-1).float()
    r = P // 2
    off = torch.arange(-r, r + 1, device=dev, dtype=torch.float32)
    px = (xy[..., 0, None, None] + off[None, None, None, :]).expand(n, M, P, P)
    py = (xy[..., 1, None, None] + off[None, None, :, None]).expand(n, M, P, P)
    pd = torch.ones(n, M, P, P, device=dev)
    patches = torch.stack([px, py, pd], dim=2).view(n * M, 3, P, P)
    index = torch.arange(n, device=dev).view(n, 1).repeat(1, M).reshape(-1)
    return x, y, xy, scores, patches, index


def kernel(smap, M, mode):
    if mode == "3xrandom":
        return S.select(smap, M, mode, pad=False, P=P)
    return S.select(smap, M, mode, True, offset=1, P=P)


def batch(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return host / calls * 1e6, (time.perf_counter() - t0) / calls * 1e6


def launches(fn, calls=5):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if "cuda" in str(getattr(ev, "device_type", "")).lower()) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="calls per timed batch")
    ap.add_argument("--repeats", type=int, default=9, help="alternating batches per path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    lines = [f"# python tools/bench_select.py  ({torch.cuda.get_device_name(0)}; 118 x 158 score map; us per call over batches of {a.calls} calls, batches of the two paths "
             f"alternating after one warm-up batch each; median (p90 - p10) of {a.repeats} batches)",
             f"{'mode':>9} {'n':>3} {'M':>3} {'path':>12} {'launches':>9} {'host us':>16} {'wall us':>16}"]
    g = torch.Generator().manual_seed(0)
    for mode, n, M in (("multi", 1, 96), ("topk", 1, 96), ("nms", 1, 96), ("3xrandom", 15, 80)):
        smap = torch.sigmoid(torch.randn(1, n, 118, 158, generator=g)).to(dev)
        paths = {"kernel": lambda: kernel(smap, M, mode), "composition": lambda: composition(smap, M, mode)}
        if mode in ("topk", "nms"):
            for u, v in zip(paths["kernel"](), paths["composition"]()):
                assert torch.equal(u.reshape(v.shape), v), mode
        times = {k: ([], []) for k in paths}
        for r in range(1 + a.repeats):
            for name, fn in paths.items():
                host, wall = batch(fn, a.calls)
                if r >= 1:
                    times[name][0].append(host)
                    times[name][1].append(wall)
        for name, fn in paths.items():
            h, w = times[name]
            lines.append(f"{mode:>9} {n:>3} {M:>3} {name:>12} {launches(fn):>9.1f} {q(h, 0.5):>8.1f} ({q(h, 0.9) - q(h, 0.1):>5.1f}) {q(w, 0.5):>8.1f} ({q(w, 0.9) - q(w, 0.1):>5.1f})")
        lines.append(f"{mode:>9} {'':>3} {'':>3} {'ratio':>12} {'':>9} {q(times['composition'][0], 0.5) / q(times['kernel'][0], 0.5):>15.1f}x "
                     f"{q(times['composition'][1], 0.5) / q(times['kernel'][1], 0.5):>15.1f}x")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
