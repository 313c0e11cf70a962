#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Writes tests/golden/train_graph.npz: the reference's growing training graph (devo/enet.py:297-339) and its close / far edge selections
(:359-369) on the CPU, with the REFERENCE's own `devo.utils.flatmeshgrid` and `set_depth`; enet.py itself needs a GPU and the compiled
extensions, so the schedule is run here through those two functions, with the reference's order of edges.  Schedule: N = 11, M = 2, P = 3, 14 iterations,
the drop forced at iterations 9 and 12.  Recorded per iteration: ii, jj, kk, n, the close / far positions, the new frame's pose row and
every patch's depth.  Data only: inputs and recorded results."""
import importlib.util
import os
import sys
import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden import REF                          # noqa: E402

N, M, P, STEPS, DROPS = 11, 2, 3, 14, (9, 12)


def main():
    spec = importlib.util.spec_from_file_location("devo_utils", os.path.join(REF, "devo", "utils.py"))       # (devo/__init__ pulls in the extensions)
    U = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(U)
    gen = torch.Generator().manual_seed(31)
    poses = torch.randn(1, N, 7, generator=gen)
    patches = U.set_depth(torch.rand(1, N * M, 3, P, P, generator=gen), torch.rand(1, N * M, generator=gen))
    out = dict(N=N, M=M, P=P, steps=STEPS, drops=np.array(DROPS), poses0=poses.numpy().copy(), patches0=patches.numpy().copy())
    frame_of = torch.arange(N).repeat_interleave(M)             # the Patchifier's ix in training
    frames = lambda lo, hi: torch.arange(lo, hi)
    pairs = lambda which, targets: tuple(U.flatmeshgrid(torch.where(which)[0], targets, indexing="ij"))     # (patch, target frame) per edge
    patch, target = pairs(frame_of < 8, frames(0, 8))
    source = frame_of[patch]
    for t in range(STEPS):
        f = int(source.max()) + 1                               # the frame that would arrive
        if t >= 8 and f < N:
            arrivals = [pairs(frame_of < f, frames(f, f + 1)), pairs(frame_of == f, frames(0, f + 1))]
            patch = torch.cat([arrivals[0][0], arrivals[1][0], patch])
            target = torch.cat([arrivals[0][1], arrivals[1][1], target])
            source = frame_of[patch]
            if t in DROPS:
                stay = (source != f - 4) & (target != f - 4)
                source, target, patch = source[stay], target[stay], patch[stay]
            poses[:, f] = poses[:, f - 1]
            last_two = (frame_of == f - 1) | (frame_of == f - 2)
            patches[:, frame_of == f, 2] = torch.median(patches[:, last_two, 2])
        n = int(source.max()) + 1
        gap = (source - target).abs()
        out[f"ii{t}"], out[f"jj{t}"], out[f"kk{t}"], out[f"n{t}"] = source.numpy().copy(), target.numpy().copy(), patch.numpy().copy(), n
        out[f"close{t}"] = torch.where((gap > 0) & (gap <= 2))[0].numpy()
        out[f"far{t}"] = torch.where((gap > 0) & (gap <= 16))[0].numpy()
        out[f"pose{t}"] = poses[0, n - 1].numpy().copy()
        out[f"depths{t}"] = patches[0, :, 2, 0, 0].numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", "train_graph.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
