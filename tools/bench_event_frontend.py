#!/usr/bin/env python3
"""Time the event front end (devo_amd.events.voxel_grids: window bounds + rectified voxelisation + hot-pixel filter for every
window of a recording in one call) against a Python loop over the windows of today's per-window pieces (torch slicing and
rectify_map[y, x], events.to_voxel_grid, torch hot-pixel ops), at the loaders' sensor sizes: 720 x 1280 x 5 (TUM-VIE, k = 6)
and 480 x 640 x 5 (EDS, k = 10), 100 windows of about 1 M events each.  Each size is measured on a uniform stream and on one
where a single pixel carries 10 % of the events.  Prints one block of text (profiles/event_frontend.txt holds a run).

    python tools/bench_event_frontend.py [--windows 100] [--events-per-window 1000000] [--reps 5]"""
import argparse
import os
import sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import events


def stream(n_win, per_win, H, W, dT_us, hot_frac, gen, dev):
    N = n_win * per_win
    ts = torch.arange(N, device=dev, dtype=torch.int64) * (n_win * dT_us) // N + 1_600_000_000_000     # ascending us, uniform rate
    x = torch.randint(0, W, (N,), device=dev, dtype=torch.int32, generator=gen)
    y = torch.randint(0, H, (N,), device=dev, dtype=torch.int32, generator=gen)
    p = torch.randint(0, 2, (N,), device=dev, dtype=torch.int8, generator=gen)
    if hot_frac > 0:
        h = torch.rand(N, device=dev, generator=gen) < hot_frac
        x[h], y[h] = W // 3, H // 2
    gy, gx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    rmap = torch.stack([gx * 0.995 + 3.2 + 1.5 * torch.sin(gy / 97), gy * 1.004 - 2.1 + 1.2 * torch.cos(gx / 131)], -1).contiguous()
    t0 = ts[0].double() + torch.arange(n_win, device=dev, dtype=torch.float64) * dT_us
    return x, y, ts, p, rmap, t0, t0 + dT_us


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                                    # us per call


def loop(x, y, ts, p, rmap, lo, hi, H, W, k):
    """The per-window path available before voxel_grids: host-known bounds, one window at a time."""
    out = []
    for a, b in zip(lo, hi):
        if b <= a:
            continue
        r = rmap[y[a:b].long(), x[a:b].long()]
        v = events.to_voxel_grid(r[:, 0], r[:, 1], ts[a:b], p[a:b], H, W, 5)
        if k is not None:
            thr = v.mean() + k * v.std()
            v[v.abs() > thr] = 0
        out.append(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=100)
    ap.add_argument("--events-per-window", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    S, per = a.windows, a.events_per_window
    print(f"event front end: {S} windows x {per} events, rectified, 5 bins; {torch.cuda.get_device_name(dev)}")
    print(f"{'sensor':>10} {'stream':>8} {'path':>28} {'us/window':>10} {'Gev/s':>7}")
    for name, H, W, k in (("TUM-VIE", 720, 1280, 6.0), ("EDS", 480, 640, 10.0)):
        per_event = {}
        for label, frac in (("uniform", 0.0), ("hot 10%", 0.10)):
            x, y, ts, p, rmap, t0, t1 = stream(S, per, H, W, 50_000, frac, gen, dev)
            out = torch.empty(S, 5, H, W, device=dev)
            lo = torch.searchsorted(ts.double(), t0).tolist()
            hi = torch.searchsorted(ts.double(), t1).tolist()
            nev = sum(b - a for a, b in zip(lo, hi))
            rows = (("voxel_grids", lambda: events.voxel_grids(x, y, ts, p, t0, t1, H, W, rectify_map=rmap, out=out), a.reps),
                    (f"voxel_grids + hot k={k:g}", lambda: events.voxel_grids(x, y, ts, p, t0, t1, H, W, rectify_map=rmap, hot_pixel_stds=k, out=out), a.reps),
                    (f"per-window loop + hot k={k:g}", lambda: loop(x, y, ts, p, rmap, lo, hi, H, W, k), 1))
            for path, fn, reps in rows:
                us = timed(fn, reps)
                print(f"{name:>10} {label:>8} {path:>28} {us / S:10.1f} {nev / us / 1e3:7.2f}")
                if path == "voxel_grids":
                    per_event[label] = us / nev
            del x, y, ts, p, out
            torch.cuda.empty_cache()
        print(f"{name:>10} hot-pixel stream / uniform stream, voxelisation time per event: {per_event['hot 10%'] / per_event['uniform']:.2f}x")


if __name__ == "__main__":
    main()
