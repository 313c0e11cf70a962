#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Writes tests/golden/frame_graph.npz by running the REAL reference on the CPU: EVSDDataset.build_frame_graph (devo/data_readers/base.py)
with its own compute_distance_matrix_flow / induced_flow (rgbd_utils.py, the data readers' projective_ops.py) over tools/gen_golden.py's
install_shims() (the oracle's SE3 backend), and EVSDDataset.__getitem__ itself for the sampled frame indices, on an in-memory scene_info
as tools/gen_golden_train_sample.py does.  The reference moves its tensors with `.cuda()` and writes one `device="cuda"` literal: both are
neutralised here (Tensor.cuda returns the tensor, torch.as_tensor drops the device).  The file holds data only.

Scenes (tests/test_frame_graph_cpu.py asserts the same conditions again):
  A  N = 33, 5 x 8 maps   fewer pixels than a wave; 2 h w = 80, so the 0.7 tie at 56 valid points exists
  B  N = 40, 6 x 8
  C  N = 5, 30 x 40       the workload's map
  E  N = 3, 6 x 8         hand-made: valid points whose flow exceeds 100 px before the clamp, in an entry that stays finite
A, B: own intrinsics per frame, fx != fy, a few depths below 0.01; each class of entries (+inf, finite >= 256, < 256) holds at least 1 %
and 8 entries; A has an entry exactly at the tie; at most 2 % of the entries are fragile (tests/frame_graph_ref.py).

Per scene <s>: <s>/poses [N, 7], <s>/depths [N, h, w] (subsampled), <s>/intr [N, 4] (full resolution), <s>/disps (the reference's),
<s>/matrix (the reference's, unscaled), <s>/rowptr, <s>/cols, <s>/dists (its dict, rows concatenated), <s>/ref_dev and <s>/disp_dev (the
largest deviation max |a - b| / max(|b|, 1) of the reference's fp32 matrix — non-fragile finite entries — and replaced disparities from
the fp64 oracle).  clips/<k>/{start, seed, sample, inds}: __getitem__'s frame indices on scene A's graph (n_frames, fmin, fmax: clips/...)."""
import os
import sys
import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from gen_golden import install_shims                                  # noqa: E402
from gen_golden_train_sample import _StubFinder, _torchvision           # noqa: E402
import frame_graph_ref as R                                           # noqa: E402

F, MAX_FLOW = 16, 256.0
CLIP_FRAMES, FMIN, FMAX = 6, 16.0, 160.0


def walk_scene(rng, N, h, w, own_intrinsics, holes):
    """A forward-biased random walk of cameras over random depths."""
    from scipy.spatial.transform import Rotation
    rot, pos, poses = Rotation.identity(), np.zeros(3), []
    for _ in range(N):
        poses.append(np.concatenate([pos, rot.as_quat()]))
        axis = rng.standard_normal(3)
        rot = rot * Rotation.from_rotvec(axis / np.linalg.norm(axis) * rng.uniform(0.10, 0.15))
        pos = pos + rot.apply(np.array([0.0, 0.0, 1.0])) * rng.uniform(0.12, 0.2) + rng.standard_normal(3) * 0.02
    depths = rng.uniform(0.4, 4.0, size=(N, h, w)).astype(np.float32)
    for _ in range(holes):
        depths[rng.integers(N), rng.integers(h), rng.integers(w)] = np.float32(rng.uniform(0.0, 0.009))
    intr = np.tile(np.array([20.0, 20.0, w / 2, h / 2]), (N, 1))
    if own_intrinsics:
        intr[:, 0] += rng.uniform(-1, 1, N)
        intr[:, 1] += 1.5 + rng.uniform(-1, 1, N)
        intr[:, 2:] += rng.uniform(-0.3, 0.3, (N, 2))
    return np.array(poses, dtype=np.float32), depths, (intr * F).astype(np.float32)


def clamp_scene():
    h, w = 6, 8
    poses = np.zeros((3, 7), np.float32)
    poses[:, 6] = 1.0
    poses[1, :3] = (-3.0, 0.0, 0.39)                              # frame 0 seen from frame 1: 3 units sideways, 0.39 closer
    poses[2, :3] = (0.1, 0.0, 0.0)
    depths = np.full((3, h, w), 20.0, np.float32)
    depths[0, 2, 3:6] = 0.5                                       # disparity 2: Z = 1 - 0.39 * 2 = 0.22
    intr = np.tile(np.array([20.0, 20.0, w / 2, h / 2], np.float32) * F, (3, 1))
    return poses, depths, intr


def classes(matrix):
    m = np.asarray(matrix)
    return np.isinf(m).sum(), (np.isfinite(m) & (m >= MAX_FLOW)).sum(), (m < MAX_FLOW).sum()


def main():
    torch.set_num_threads(1)
    sys.meta_path.insert(0, _StubFinder())
    _torchvision()
    install_shims()
    torch.Tensor.cuda = lambda self, *a, **k: self
    as_tensor = torch.as_tensor
    torch.as_tensor = lambda data, *a, device=None, **k: as_tensor(data, *a, **k)
    from devo.data_readers import base
    from devo.data_readers.base import EVSDDataset

    recorded = {}
    flow = base.compute_distance_matrix_flow

    def recording(poses, disps, intrinsics):
        recorded["disps"] = np.array(disps, dtype=np.float32)
        recorded["matrix"] = flow(poses, disps, intrinsics)
        return recorded["matrix"]
    base.compute_distance_matrix_flow = recording

    def reference_graph(poses, depths, intr):
        class Mem(EVSDDataset):
            @staticmethod
            def depth_read(i):
                return np.repeat(np.repeat(depths[i], F, 0), F, 1)      # a full-size map whose [F//2::F, F//2::F] is depths[i]
        ds = Mem.__new__(Mem)
        graph = ds.build_frame_graph(list(poses), list(range(len(poses))), list(intr), f=F, max_flow=MAX_FLOW)
        return graph, recorded["disps"].copy(), recorded["matrix"].copy()

    def measure(poses, depths, intr):
        graph, disps, matrix = reference_graph(poses, depths, intr)
        oracle, fragile, tie = R.distance_oracle(poses, disps, intr / F, scale=float(F), max_flow=MAX_FLOW)
        return graph, disps, matrix, (oracle / F).numpy(), fragile.numpy(), tie.numpy()

    # ---- EVSDDataset.__getitem__'s frame indices on a graph: clips whose walk reads only rows without a fragile entry
    visited = []

    class Clip(EVSDDataset):
        @staticmethod
        def voxel_read(i):
            visited.append(int(i))
            return np.zeros((2, 4, 4), np.float32)

        @staticmethod
        def depth_read(i):
            return np.ones((4, 4), np.float32)

    def clips_of(graph, fragile):
        """[(start, seed, sample, inds)]: per mode up to 4 clips that walk backwards somewhere and 4 that do not; None if a mode lacks
        either kind or has fewer than 6."""
        N = len(graph)
        ds = Clip.__new__(Clip)
        ds.n_frames, ds.fmin, ds.fmax, ds.scale, ds.return_fname, ds.aug = CLIP_FRAMES, FMIN, FMAX, 1.0, False, None
        ds.scene_info = {"s": {"graph": graph, "voxels": list(range(N)), "depths": list(range(N)), "poses": [np.zeros(7, np.float32)] * N,
                               "intrinsics": [np.ones(4, np.float32)] * N}}
        clean = ~fragile.any(1)                                      # rows without a fragile entry
        chosen = []
        for sample in (True, False):
            ds.sample = sample
            found = {True: [], False: []}
            for start in range(N):
                for seed in (0, 1, 2):
                    ds.dataset_index = [("s", start)]
                    del visited[:]
                    np.random.seed(seed)
                    ds[0]
                    inds = np.array(visited, dtype=np.int64)
                    if clean[inds[:-1]].all():                      # the rows the walk read
                        found[bool((np.diff(inds) < 0).any())].append((start, seed, sample, inds))
            if not found[True] or len(found[True][:4] + found[False][:4]) < 6:
                return None
            chosen += found[True][:4] + found[False][:4]
        return chosen

    out = {"f": F, "max_flow": MAX_FLOW}
    kept = {}
    for name, (N, h, w, own, holes) in {"A": (33, 5, 8, True, 6), "B": (40, 6, 8, True, 6), "C": (5, 30, 40, False, 0), "E": (3, 6, 8, False, 0)}.items():
        for seed in range(200):
            rng = np.random.default_rng(20261018 + 1000 * ord(name) + seed)
            poses, depths, intr = clamp_scene() if name == "E" else walk_scene(rng, N, h, w, own, holes)
            graph, disps, matrix, oracle, fragile, tie = measure(poses, depths, intr)
            n_inf, n_far, n_near = classes(F * matrix)
            if fragile.mean() <= 0.02 and (name not in "AB" or min(n_inf, n_far, n_near) >= max(8, 0.01 * N * N)) and (name != "A" or (tie & ~fragile).any()):
                if name == "A":
                    kept_clips = clips_of(graph, fragile)
                    if kept_clips is None:
                        continue
                break
        else:
            raise AssertionError(f"scene {name}: no seed meets the conditions")
        solid = ~fragile
        assert (np.isinf(matrix) == np.isinf(oracle))[solid].all(), name
        assert ((F * matrix < MAX_FLOW) == (F * oracle < MAX_FLOW))[solid].all(), name
        assert not np.isinf(matrix[tie & solid]).any()
        finite = solid & np.isfinite(oracle)
        ref_dev = R.rel_dev(matrix[finite], oracle[finite])
        d_oracle, low = R.disps_oracle(depths)
        assert (int(low.sum()) > 0) == (name in "AB")
        assert (disps[~low.numpy()] == (np.float32(1) / depths)[~low.numpy()]).all()
        disp_dev = R.rel_dev(disps[low.numpy()], d_oracle.numpy()[low.numpy()])
        if name == "E":
            _, _, _, peak = R.directed_sums(poses, disps, intr / F)
            assert float(peak[0, 1]) > 100.0 and np.isfinite(oracle[0, 1]) and not fragile[0, 1], "scene E does not reach the clamp"
        rowptr = np.concatenate([[0], np.cumsum([len(graph[i][0]) for i in range(N)])]).astype(np.int64)
        out.update({f"{name}/poses": poses, f"{name}/depths": depths, f"{name}/intr": intr, f"{name}/disps": disps, f"{name}/matrix": matrix,
                    f"{name}/rowptr": rowptr, f"{name}/cols": np.concatenate([graph[i][0] for i in range(N)]).astype(np.int64),
                    f"{name}/dists": np.concatenate([graph[i][1] for i in range(N)]).astype(np.float32),
                    f"{name}/ref_dev": np.float64(ref_dev), f"{name}/disp_dev": np.float64(disp_dev)})
        kept[name] = (graph, fragile)
        print(f"scene {name}: seed {seed}, classes (inf, >= max, < max) {classes(F * matrix)}, ties {int(tie.sum())}, fragile {fragile.mean():.4f}, "
              f"ref_dev {ref_dev:.3e}, disp_dev {disp_dev:.3e}, replaced {int(low.sum())}")

    for k, (start, seed, sample, inds) in enumerate(kept_clips):
        out.update({f"clips/{k}/start": start, f"clips/{k}/seed": seed, f"clips/{k}/sample": sample, f"clips/{k}/inds": inds})
    k = len(kept_clips)
    out.update({"clips/n": k, "clips/n_frames": CLIP_FRAMES, "clips/fmin": FMIN, "clips/fmax": FMAX})
    print(k, "clips")

    path = os.path.join(ROOT, "tests", "golden", "frame_graph.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
