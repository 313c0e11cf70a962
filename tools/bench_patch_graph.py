"""Per-frame cost of the patch-graph bookkeeping (devo/devo.py:541-552: append forward edges, append backward edges, keyframe) at the
config/default.yaml steady state: 45 312 edges, M = 96, dim 384, net in fp16 and in fp32.

    python tools/bench_patch_graph.py                      # both implementations, both dtypes, both branches -> the table of profiles/patch_graph.txt
    python tools/bench_patch_graph.py --impl graph --net fp16 --branch remove --frames 20      # one cell (what a kernel trace is taken of)

(a) reference: the reference's composition — torch.cat, boolean-mask gathers, pops.flow_mag + .item(), the Python frame shift — on
    the GPU over this package's projective_ops: what a user of the state machine runs without devo_amd.graph;
(b) graph:     devo_amd.graph.PatchGraph + shift_frames.
A frame is timed from the host with a device synchronisation in front and behind (the wall time the frame's bookkeeping adds);
warm-up frames first, then min / median / spread (p90 - p10) over the timed frames.  `remove`: a threshold every frame passes (the
keyframe goes, the graph is renumbered, the frame buffers shift), `keep`: one no frame passes (only the removal window acts)."""
import argparse
import json
import os
import sys
import time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import synth, graph                                       # noqa: E402
from devo_amd import projective_ops as pops                             # noqa: E402
from devo_amd.lietorch import SE3                                       # noqa: E402

DEV = "cuda"
M, DIM, LIFE, WINDOW, KI, N0, H, W = 96, 384, 13, 22, 4, 40, 120, 160


class Reference:
    """devo.py:225-239, :258-306 as the reference writes them, on GPU tensors."""

    def __init__(self, ix, ii, jj, kk, dtype):
        self.ix, self.ii, self.jj, self.kk = ix, ii.clone(), jj.clone(), kk.clone()
        self.net = torch.zeros(1, len(ii), DIM, dtype=dtype, device=DEV)

    def __len__(self):
        return len(self.ii)

    def append(self, ii, jj, ix):
        self.jj = torch.cat([self.jj, jj])
        self.kk = torch.cat([self.kk, ii])
        self.ii = torch.cat([self.ii, self.ix[ii]])
        net = torch.zeros(1, len(ii), DIM, dtype=self.net.dtype, device=DEV)
        self.net = torch.cat([self.net, net], dim=1)

    def remove_factors(self, m):
        self.ii = self.ii[~m]
        self.jj = self.jj[~m]
        self.kk = self.kk[~m]
        self.net = self.net[:, ~m]

    def motionmag(self, st, i, j):
        k = (self.ii == i) & (self.jj == j)
        flow = pops.flow_mag(SE3(st["poses"]), st["patches"], st["intrinsics"], self.ii[k], self.jj[k], self.kk[k], beta=0.5)
        return flow.mean().item()

    def keyframe(self, st, n, thresh):
        i, j = n - KI - 1, n - KI + 1
        m = self.motionmag(st, i, j) + self.motionmag(st, j, i)
        removed = m / 2 < thresh
        if removed:
            k = n - KI
            self.remove_factors((self.ii == k) | (self.jj == k))
            self.kk[self.ii > k] -= M
            self.ii[self.ii > k] -= 1
            self.jj[self.jj > k] -= 1
            for r in range(k, n - 1):
                for t in st["frames"]:
                    t[r] = t[r + 1]
            n -= 1
        self.remove_factors(self.ix[self.kk] < n - WINDOW)
        return removed


class Graph:
    def __init__(self, ix, ii, jj, kk, dtype):
        self.g = graph.PatchGraph(M, dim=DIM, device=DEV, dtype=dtype)
        self.g.append(kk, jj, ix)

    def __len__(self):
        return len(self.g)

    def append(self, ii, jj, ix):
        self.g.append(ii, jj, ix)

    def keyframe(self, st, n, thresh):
        r = self.g.keyframe(st["poses"], st["patches"], st["intrinsics"], st["ix"], n, keyframe_index=KI, thresh=thresh, removal_window=WINDOW)
        if r.removed:
            graph.shift_frames(st["frames"], r.k, n)
        return r.removed


def run(impl, dtype, branch, frames, warmup):
    nbuf = N0 + frames + warmup + 4
    poses = synth.make_poses(nbuf, 11, trans_step=0.01, rot_step=0.002).to(DEV)
    patches = synth.make_patches(nbuf, M, H, W, seed=11)[0].to(DEV)
    intr = synth.make_intrinsics(nbuf, H, W).to(DEV)
    ix = (torch.arange(nbuf * M) // M).to(DEV)
    tstamps = torch.arange(nbuf, dtype=torch.float64, device=DEV)
    colors = torch.zeros(nbuf, M, 3, dtype=torch.uint8, device=DEV)
    patches_gt = patches[0].clone()
    st = {"poses": poses, "patches": patches, "intrinsics": intr, "ix": ix,
          "frames": [tstamps, colors, poses[0], patches[0], patches_gt, intr[0]]}                 # devo.py:290-295
    ii, jj, kk = [t.to(DEV) for t in synth.sliding_window_graph(N0, M, LIFE, WINDOW)]
    s = (Reference if impl == "reference" else Graph)(ix, ii, jj, kk, dtype)
    thresh = 1e9 if branch == "remove" else -1.0
    n, times, sizes = N0, [], []
    for f in range(warmup + frames):
        n += 1
        fk = torch.arange(M * max(n - LIFE, 0), M * (n - 1), device=DEV)                         # (the index lists of devo.py:366-380 are not bookkeeping:
        fj = torch.full_like(fk, n - 1)                                                           #  made outside the timed region)
        bj = torch.arange(max(n - LIFE, 0), n, device=DEV)
        bk = torch.arange(M * (n - 1), M * n, device=DEV).repeat_interleave(len(bj))
        bj = bj.repeat(M)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.append(fk, fj, ix)
        s.append(bk, bj, ix)
        if s.keyframe(st, n, thresh):
            n -= 1
        torch.cuda.synchronize()
        if f >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
            sizes.append(len(s))
    t = torch.tensor(times, dtype=torch.float64)
    q = lambda p: float(torch.quantile(t, p))
    return {"impl": impl, "net": str(dtype).replace("torch.", ""), "branch": branch, "frames": frames, "edges": sizes[-1], "min_us": float(t.min()),
            "median_us": q(0.5), "spread_us": q(0.9) - q(0.1), "max_us": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["reference", "graph", "both"], default="both")
    ap.add_argument("--net", choices=["fp16", "fp32", "both"], default="both")
    ap.add_argument("--branch", choices=["remove", "keep", "both"], default="both")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    pick = lambda v, all_: all_ if v == "both" else [v]
    rows = []
    print(f"# python tools/bench_patch_graph.py  ({torch.cuda.get_device_name(0)}; {a.frames} frames after {a.warmup} warm-up frames; us per frame: "
          f"2 appends + keyframe, host wall time between two device synchronisations)")
    print(f"{'net':>5} {'branch':>7} {'impl':>10} {'edges':>6} {'min':>9} {'median':>9} {'p90-p10':>9} {'max':>9}")
    for net in pick(a.net, ["fp16", "fp32"]):
        for branch in pick(a.branch, ["remove", "keep"]):
            cell = {}
            for impl in pick(a.impl, ["reference", "graph"]):
                r = run(impl, torch.float16 if net == "fp16" else torch.float32, branch, a.frames, a.warmup)
                rows.append(r)
                cell[impl] = r
                print(f"{net:>5} {branch:>7} {impl:>10} {r['edges']:>6} {r['min_us']:>9.1f} {r['median_us']:>9.1f} {r['spread_us']:>9.1f} {r['max_us']:>9.1f}", flush=True)
            if len(cell) == 2:
                ref, g = cell["reference"], cell["graph"]
                print(f"{'':>5} {'':>7} {'ratio':>10} {'':>6} {ref['min_us'] / g['min_us']:>8.2f}x {ref['median_us'] / g['median_us']:>8.2f}x   "
                      f"(median gain {ref['median_us'] - g['median_us']:.1f} us against a reference spread of {ref['spread_us']:.1f} us)")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
