#!/usr/bin/env python3
"""Time the tail of a training sample (devo_amd.data.prepare_batch: jitter, zoom, centre crop, depth normalisation) at the training
size [1, 15, 5, 480, 640] against two compositions of the reference's ops (devo/data_readers/augmentation.py:79-174, base.py:366-369):
in torch on the GPU, and in torch on the host's CPU as the reference's DataLoader workers run them (one thread per worker; one worker,
and four concurrent workers as train.py uses).  Both zoom branches are timed: scale 1 (the draw with probability 0.2) and scale 1.1.
The GPU composition's output is checked against the HIP call first.  Device events after warm-up; prints one block of text
(profiles/train_sample.txt).

    python tools/bench_train_sample.py [--reps 20] [--cpu-reps 3] [--no-cpu]"""
import argparse
import multiprocessing as mp
import os
import sys
import time
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (1, 15, 5, 480, 640)
CROP = (480, 640)


def reference_tail(vox, poses, disps, intr, scale):
    """EVSDAugmentor.__call__ + the depth normalisation for one sample [n, ...], with the draw `scale`, in torch (any device)."""
    vox = vox + (torch.rand_like(vox) - 0.5) * 2 * 1e-4
    intr = scale * intr
    d = disps.unsqueeze(1)
    vox = F.interpolate(vox, scale_factor=scale, mode="bilinear", align_corners=False, recompute_scale_factor=True)
    d = F.interpolate(d, scale_factor=scale, recompute_scale_factor=True)
    y0 = (vox.shape[2] - CROP[0]) // 2
    x0 = (vox.shape[3] - CROP[1]) // 2
    intr = intr - torch.tensor([0.0, 0.0, x0, y0], device=intr.device)
    vox = vox[:, :, y0:y0 + CROP[0], x0:x0 + CROP[1]]
    d = d[:, :, y0:y0 + CROP[0], x0:x0 + CROP[1]].squeeze(1)
    s = .7 * torch.quantile(d, .98)
    d = d / s
    poses = poses.clone()
    poses[..., :3] *= s
    return vox, poses, d, intr


def inputs(device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    B, n, bins, H, W = SHAPE
    vox = torch.randn(B, n, bins, H, W, device=device, generator=g)
    disps = 1.0 / (torch.rand(B, n, H, W, device=device, generator=g) * 20 + 0.5)
    poses = torch.randn(B, n, 7, device=device, generator=g)
    intr = torch.tensor([320.0, 320.0, 320.0, 240.0], device=device).repeat(B, n, 1)
    return vox, poses, disps, intr


def gpu_time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def _cpu_worker(args):
    scale, reps = args
    torch.set_num_threads(1)
    vox, poses, disps, intr = inputs("cpu")
    reference_tail(vox[0], poses[0], disps[0], intr[0], scale)
    t0 = time.perf_counter()
    for _ in range(reps):
        reference_tail(vox[0], poses[0], disps[0], intr[0], scale)
    return time.perf_counter() - t0


def cpu_time(scale, reps, workers):
    """Seconds per sample with `workers` one-thread processes working at once (wall time / samples)."""
    ctx = mp.get_context("spawn")
    with ctx.Pool(workers) as pool:
        t0 = time.perf_counter()
        pool.map(_cpu_worker, [(scale, reps)] * workers)
        wall = time.perf_counter() - t0
    return wall / (workers * reps), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from devo_amd import data
    dev = torch.device("cuda", 0)
    vox, poses, disps, intr = inputs(dev)
    mb = vox.numel() * 4 / 1e6
    print(f"training sample tail {list(SHAPE)} fp32 ({mb:.0f} MB voxels, {disps.numel() * 4 / 1e6:.0f} MB disparities), crop {CROP[0]}x{CROP[1]}, "
          f"reps {a.reps}; {torch.cuda.get_device_name(0)}")
    print(f"{'scale':>6} {'HIP prepare_batch':>18} {'torch GPU':>12} {'x':>6} {'host 1 worker':>14} {'host 4 workers':>15}")
    for scale in (1.0, 1.1):
        p = [{"scale": scale, "seed": 1}]
        noise = torch.rand_like(vox)
        hv, hp, hd, hk = data.prepare_batch(vox, poses, disps, intr, CROP, params=p, noise=noise)
        rv, rp, rd, rk = reference_tail(vox[0], poses[0], disps[0], intr[0], scale)          # shapes and the exact parts
        assert rv.shape == hv[0].shape and torch.equal(rk, hk[0])
        ref_d = F.interpolate(disps[0].unsqueeze(1), scale_factor=scale, recompute_scale_factor=True).squeeze(1)
        y0, x0 = (ref_d.shape[1] - CROP[0]) // 2, (ref_d.shape[2] - CROP[1]) // 2
        ref_d = ref_d[:, y0:y0 + CROP[0], x0:x0 + CROP[1]]
        assert torch.equal(hd[0], ref_d / (.7 * torch.quantile(ref_d, .98)))
        t_hip = gpu_time(lambda: data.prepare_batch(vox, poses, disps, intr, CROP, params=p), a.reps)
        t_tg = gpu_time(lambda: reference_tail(vox[0], poses[0], disps[0], intr[0], scale), a.reps)
        c1 = c4 = float("nan")
        if not a.no_cpu:
            c1, _ = cpu_time(scale, a.cpu_reps, 1)
            c4, _ = cpu_time(scale, a.cpu_reps, 4)
        print(f"{scale:>6} {t_hip[0]:>12.1f} us   {t_tg[0]:>9.1f} us {t_tg[0] / t_hip[0]:>5.1f}x {c1 * 1e3:>11.0f} ms {c4 * 1e3:>12.0f} ms")
    print("HIP: prepare_batch with in-kernel jitter (one resample launch per tensor, one normalisation call: 7 kernels, a few host-side "
          "intrinsics ops).  torch GPU: the reference's ops on the device (torch.rand_like, F.interpolate, slicing, torch.quantile's sort).  "
          "host: the same ops on this machine's CPU, one torch thread per worker process, seconds per sample (wall / samples).")


if __name__ == "__main__":
    main()
