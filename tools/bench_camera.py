"""Camera models per call: devo_amd.camera (csrc/camera.hip) against the same arithmetic composed in torch on the GPU and the numpy
restatement (tests/camera_ref.py) on the host.

    python tools/bench_camera.py                              # the table of profiles/camera.txt
    python tools/bench_camera.py --out profiles/camera.txt

Rows: `rectify_map` of a 1280 x 720 equidistant sensor and of a 640 x 480 radtan sensor (one launch, fp64, the pixel grid generated in the
kernel); `undistort_images` of 1 and of 15 frames 480 x 640 x 3 uint8 with the source map already kept (one launch).  The torch composition
is Newton as tensor operations in fp64 on a grid kept on the device (12 iterations, no validity bookkeeping) and, for the frames,
uint8 -> float NCHW, `grid_sample` on a kept normalised grid (bilinear, zeros, align_corners) and the way back to uint8 channels-last.
A batch of --calls calls is timed on the host clock until the device has finished; batches of the paths alternate after a warm-up batch
each; medians over the batches with the p90 - p10 spread.  Launches per call: GPU activities the profiler records over 3 calls.  GB/s of the
remap: (B frames read + B frames written + the map read once) / time."""
import argparse
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from devo_amd import camera as C                                       # noqa: E402
import camera_ref as T                                                 # noqa: E402


def torch_rectify(fx, K_new, grid, iters=12):
    model, K, dist, _ = fx
    xd, yd = (grid[:, 0] - K[2]) / K[0], (grid[:, 1] - K[3]) / K[1]
    if model == "equidistant":
        k1, k2, k3, k4 = dist
        td = torch.hypot(xd, yd)
        t = td.clone()
        for _ in range(iters):
            t2 = t * t
            f = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
            t = t - f / (1 + t2 * (3 * k1 + t2 * (5 * k2 + t2 * (7 * k3 + t2 * 9 * k4))))
        s = torch.where(td > 0, torch.tan(t) / td.clamp_min(1e-300), torch.ones_like(td))
        x, y = xd * s, yd * s
    else:
        k1, k2, p1, p2, k3 = dist
        x, y = xd.clone(), yd.clone()
        for _ in range(iters):
            r2 = x * x + y * y
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            D = k1 + r2 * (2 * k2 + r2 * 3 * k3)
            ex = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) - xd
            ey = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y - yd
            a = rad + 2 * x * x * D + 2 * p1 * y + 6 * p2 * x
            b = 2 * x * y * D + 2 * p1 * x + 2 * p2 * y
            d = rad + 2 * y * y * D + 6 * p1 * y + 2 * p2 * x
            det = a * d - b * b
            x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
    return torch.stack([K_new[0] * x + K_new[2], K_new[1] * y + K_new[3]], 1).float()


def torch_undistort(frames, norm_grid):
    x = frames.permute(0, 3, 1, 2).float()
    y = torch.nn.functional.grid_sample(x, norm_grid.expand(x.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)
    return y.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def batch(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def launches(fn, calls=3):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if "cuda" in str(getattr(ev, "device_type", "")).lower()) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timed batch (the host path: 1)")
    ap.add_argument("--repeats", type=int, default=7, help="alternating batches per path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    lines = [f"# python tools/bench_camera.py  ({torch.cuda.get_device_name(0)}; ms per call over batches of {a.calls} calls (numpy: 1), batches of the paths alternating after "
             f"one warm-up batch each; median (p90 - p10) of {a.repeats} batches)",
             f"{'case':>34} {'path':>15} {'launches':>9} {'ms per call':>18} {'GB/s':>7}"]

    def measure(case, paths, nbytes=None):
        times = {k: [] for k in paths}
        for r in range(1 + a.repeats):
            for name, fn in paths.items():
                ms = batch(fn, 1 if name == "numpy on host" else a.calls)
                if r >= 1:
                    times[name].append(ms)
        for name, fn in paths.items():
            n_l = launches(fn) if name != "numpy on host" else 0.0
            v = times[name]
            rate = f"{nbytes / (q(v, 0.5) * 1e-3) / 1e9:>7.0f}" if nbytes and name != "numpy on host" else f"{'':>7}"
            lines.append(f"{case:>34} {name:>15} {n_l:>9.1f} {q(v, 0.5):>9.3f} ({q(v, 0.9) - q(v, 0.1):>6.3f}) {rate}")

    for name in ("equi1280", "radtan640"):
        fx = T.MILD[name]
        cam = C.Camera(*fx)
        K_new = C.new_camera_matrix(cam)
        grid = torch.from_numpy(T.pixel_grid(*fx[3])).to(dev)
        paths = {"kernel": lambda: C.rectify_map(cam, K_new), "torch on GPU": lambda: torch_rectify(fx, K_new, grid),
                 "numpy on host": lambda: T.undistort(fx, T.pixel_grid(*fx[3]), K_new)[0]}
        want = paths["numpy on host"]()
        for k in ("kernel", "torch on GPU"):
            assert np.abs(paths[k]().cpu().numpy().reshape(-1, 2) - want).max() <= 2 * np.spacing(np.float32(np.abs(want).max())), k
        measure(f"rectify_map {fx[0]} {fx[3][0]} x {fx[3][1]}", paths)

    fx = T.MILD["radtan640"]
    cam = C.Camera(*fx)
    W, H = cam.size
    src = C.undistort_map(cam)
    norm = (src / torch.tensor([(W - 1) / 2, (H - 1) / 2], device=dev) - 1.0).unsqueeze(0)
    g = np.random.default_rng(0)
    for B in (1, 15):
        host = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        frames = torch.from_numpy(host).to(dev)
        paths = {"kernel": lambda: C.undistort_images(frames, cam), "torch on GPU": lambda: torch_undistort(frames, norm),
                 "numpy on host": lambda: T.to_uint8(T.remap(host, src_host))}
        src_host = src.cpu().numpy()
        want = paths["numpy on host"]().astype(np.int64)
        for k in ("kernel", "torch on GPU"):
            assert np.abs(paths[k]().cpu().numpy().astype(np.int64) - want).max() <= 1, k
        measure(f"undistort_images {B} x 480 x 640 x 3 u8", paths, nbytes=2 * host.size + src.numel() * 4)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
