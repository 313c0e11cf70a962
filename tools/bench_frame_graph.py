"""Build time of a scene's training frame graph (devo/data_readers/base.py:263-286) at N = 500 and N = 2000 frames with the reference's
30 x 40 subsampled maps (f = 16, max_flow = 256).

    python tools/bench_frame_graph.py                      # the table of profiles/frame_graph.txt
    python tools/bench_frame_graph.py --out profiles/frame_graph.txt

(a) reference: the reference's composition restated in fp32 torch on the GPU (tests/frame_graph_ref.chunked_distance_matrix: all N^2
    ordered pairs in chunks of 2048, both directions per chunk, a copy to the host per chunk), then its host loop over the rows
    (np.where per row) — what rgbd_utils.compute_distance_matrix_flow + build_frame_graph run;
(b) graph:     devo_amd.frame_graph.build_frame_graph from device tensors to the CSR lists on the device (7 launches, one read-back).
Whole builds alternate (a, b, a, b, ...); a build is timed on the host clock between two device synchronisations; medians over the
repeats with the p90 - p10 spread beside them.  The distances call of (b) alone (3 launches, the pair kernel among them) is timed with
device events, and turned into a rate: N^2 h w reprojections (each directed pair once) of 30 flops (9 + 9 + 3 for the action and the
projection's multiplies, the rest for the flow, its norm and the sums; the division and the square root counted as one each) over that
time, against the 157.3 TFLOP/s fp32 vector peak.  The two matrices are compared at every size (inf pattern, list membership,
deviation); the pairs that disagree most are checked one by one against the fp64 oracle of tests/frame_graph_ref.py on their two frames:
two fp32 computations differ visibly only where a point sits on the validity threshold (one point of 2 400 changing sides moves the mean
by up to 100 / 2 400 px), which is what the oracle's fragile mask marks."""
import argparse
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from devo_amd import frame_graph as FG                                 # noqa: E402
import frame_graph_ref as R                                            # noqa: E402

H, W, F, MAX_FLOW = 30, 40, 16, 256.0
FLOPS_PER_POINT, PEAK = 30, 157.3e12
WORST = 48


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _rotate(q, v):
    u, w = q[:3], q[3]
    c = np.cross(u, v)
    return v + 2 * w * c + 2 * np.cross(u, c)


def scene(N, seed=0):
    """A forward-biased random walk (steps of 0.12 - 0.2, 0.10 - 0.15 rad per frame) over depths uniform in [0.4, 4]."""
    rng = np.random.default_rng(seed)
    q, pos, poses = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), []
    for _ in range(N):
        poses.append(np.concatenate([pos, q]))
        axis = rng.standard_normal(3)
        half = rng.uniform(0.10, 0.15) / 2
        q = _quat_mul(q, np.concatenate([axis / np.linalg.norm(axis) * np.sin(half), [np.cos(half)]]))
        q /= np.linalg.norm(q)
        pos = pos + _rotate(q, np.array([0.0, 0.0, 1.0])) * rng.uniform(0.12, 0.2) + rng.standard_normal(3) * 0.02
    depths = rng.uniform(0.4, 4.0, size=(N, H, W)).astype(np.float32)
    intr = np.tile(np.array([20.0 * F, 20.0 * F, W / 2 * F, H / 2 * F], np.float32), (N, 1))
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (np.array(poses), depths, intr))


def reference_build(poses, depths, intr):
    depths = depths.clone()
    mean = depths.mean(dim=(1, 2), keepdim=True).expand_as(depths)
    low = depths < 0.01
    depths[low] = mean[low]
    d = F * R.chunked_distance_matrix(poses, 1.0 / depths, intr / F)
    graph = {}
    for i in range(d.shape[0]):
        j, = np.where(d[i] < MAX_FLOW)
        graph[i] = (j, d[i, j])
    return d, graph


def compare(lines, d_ref, ours, poses, disps, intr, n_lists, n_lists_ref):
    """Appends the agreement of the two scaled matrices (numpy [N, N]) to `lines`."""
    N = len(ours)
    both = np.isfinite(d_ref) & np.isfinite(ours)
    dev = np.zeros_like(ours, dtype=np.float64)
    dev[both] = np.abs(ours[both].astype(np.float64) - d_ref[both]) / np.maximum(np.abs(d_ref[both]), 1)
    differ = (np.isinf(d_ref) != np.isinf(ours)) | ((d_ref < MAX_FLOW) != (ours < MAX_FLOW))
    lines.append(f"{'':>6} {'agreement':>10}   inf pattern differs in {int((np.isinf(d_ref) != np.isinf(ours)).sum())} of {N * N} entries, list membership in "
                 f"{int(((d_ref < MAX_FLOW) != (ours < MAX_FLOW)).sum())}; deviation of the finite entries relative to max(|d|, 1): median {np.median(dev[both]):.2e}, "
                 f"above 1e-5 in {int((dev > 1e-5).sum())}, largest {dev.max():.2e}; {n_lists} list entries (reference {n_lists_ref})")
    # the entries that disagree most, one by one against the fp64 oracle on their two frames
    score = np.where(differ, np.inf, dev)
    worst = np.argsort(score, axis=None)[::-1][:WORST]
    worst = [(int(e // N), int(e % N)) for e in worst if score.flat[e] > 1e-5 and e // N < e % N] + [(int(i), int(j)) for i, j in zip(*np.nonzero(differ)) if i < j][:4 * WORST]
    P, D, K = poses.cpu().numpy(), disps.cpu().numpy(), (intr / F).cpu().numpy()
    n_fragile, ours_dev, ref_dev = 0, 0.0, 0.0
    for i, j in dict.fromkeys(worst):
        o, fragile, _ = R.distance_oracle(P[[i, j]], D[[i, j]], K[[i, j]], scale=float(F), max_flow=MAX_FLOW)
        if bool(fragile[0, 1]):
            n_fragile += 1
        elif np.isfinite(float(o[0, 1])):
            ours_dev = max(ours_dev, abs(ours[i, j] - float(o[0, 1])) / max(abs(float(o[0, 1])), 1))
            ref_dev = max(ref_dev, abs(d_ref[i, j] - float(o[0, 1])) / max(abs(float(o[0, 1])), 1))
    n_worst = len(dict.fromkeys(worst))
    lines.append(f"{'':>6} {'':>10}   of the {n_worst} unordered pairs that disagree most (membership or deviation above 1e-5), {n_fragile} are fragile by the fp64 oracle "
                 f"(a point within 1e-4 of the validity threshold, or the entry within 0.0256 of max_flow); the other {n_worst - n_fragile}: graph vs oracle {ours_dev:.2e}, "
                 f"reference vs oracle {ref_dev:.2e}")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--repeats", type=int, nargs="+", default=[7, 3], help="alternating builds per size")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_graph needs a GPU: nothing is measured without one")
    lines = [f"# python tools/bench_frame_graph.py  ({torch.cuda.get_device_name(0)}; {H} x {W} maps, f = {F}, max_flow = {MAX_FLOW:g}; ms per build, host wall time between two "
             "device synchronisations, whole builds alternating after one warm-up build each; median, p90 - p10)",
             f"{'N':>6} {'impl':>10} {'repeats':>8} {'min':>10} {'median':>10} {'p90-p10':>10}"]
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    for N, repeats in zip(a.sizes, a.repeats):
        poses, depths, intr = scene(N)
        impls = {"reference": lambda: reference_build(poses, depths, intr), "graph": lambda: FG.build_frame_graph(poses, depths, intr, f=F, max_flow=MAX_FLOW)}
        times = {k: [] for k in impls}
        results = {}
        for r in range(1 + repeats):
            for name, fn in impls.items():
                ms, results[name] = timed(fn)
                if r >= 1:
                    times[name].append(ms)
        for name, v in times.items():
            lines.append(f"{N:>6} {name:>10} {len(v):>8} {min(v):>10.2f} {q(v, 0.5):>10.2f} {q(v, 0.9) - q(v, 0.1):>10.2f}")
        lines.append(f"{'':>6} {'ratio':>10} {'':>8} {min(times['reference']) / min(times['graph']):>9.1f}x {q(times['reference'], 0.5) / q(times['graph'], 0.5):>9.1f}x")
        # the distances call alone, device events
        disps = FG.prepare_disps(depths)
        ev = []
        for r in range(2 + 9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            matrix = FG.distance_matrix(poses, disps, intr / F)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ev.append(e0.elapsed_time(e1))
        points = N * N * H * W
        med = q(ev, 0.5)
        rate = points / (med * 1e-3)
        lines.append(f"{N:>6} {'distances':>10} {len(ev):>8} {min(ev):>10.3f} {med:>10.3f} {q(ev, 0.9) - q(ev, 0.1):>10.3f}   device events; {points:.3e} reprojections, "
                     f"{rate:.3e} /s, x {FLOPS_PER_POINT} flops = {rate * FLOPS_PER_POINT / 1e12:.1f} TFLOP/s = {100 * rate * FLOPS_PER_POINT / PEAK:.1f} % of the fp32 vector peak")
        # the two results
        d_ref, g_ref = results["reference"]
        ours = (matrix * F).cpu().numpy()
        compare(lines, d_ref, ours, poses, disps, intr, int(results["graph"].rowptr[-1]), sum(len(v[0]) for v in g_ref.values()))
        print("\n".join(lines[-6:] if N != a.sizes[0] else lines), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
