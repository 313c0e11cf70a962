"""A torch restatement of the reference's growing training graph (devo/enet.py:300-339) and of its close / far edge selections
(:359-369), written anew in closed form (aranges instead of meshgrids over `where`), device-agnostic: the oracle of tests/test_train_graph_cpu.py and tests/test_gpu_train_graph.py, pinned by
tests/golden/train_graph.npz (tools/gen_golden_train_graph.py runs the schedule with the reference's own flatmeshgrid / set_depth).
It has the interface of devo_amd.train_graph.TrainGraph (n, len, ii / jj / kk, close, far, grows, step), so it can drive
TrainNet.forward(schedule="reference") in TrainGraph's place as the baseline of the end-to-end test."""
import collections
import torch

EdgeList = collections.namedtuple("EdgeList", "pos ii jj kk")


class RefTrainGraph:
    """State: `edges`, an int64 [3, E] tensor of (source frame, target frame, patch) per edge — the reference's ii, jj, kk.  Patch p
    belongs to frame p // M, so every index list is arithmetic on aranges; nothing is looked up in a frame-of-patch table."""

    def __init__(self, n_frames, M, init_frames=8, warmup=8, device="cpu"):
        self.n_frames, self.M, self.warmup, self.device = n_frames, M, warmup, torch.device(device)
        patch = torch.arange(init_frames * M, device=device).repeat_interleave(init_frames)     # every patch of the first frames, into each of them
        target = torch.arange(init_frames, device=device).repeat(init_frames * M)
        self.edges = torch.stack([patch // M, target, patch])
        self.n = init_frames
        self.keep = None                                      # the last growth's mask over [new edges | old edges], or None

    ii = property(lambda self: self.edges[0])
    jj = property(lambda self: self.edges[1])
    kk = property(lambda self: self.edges[2])

    def __len__(self):
        return self.edges.shape[1]

    def grows(self, t):
        return t >= self.warmup and self.n < self.n_frames

    def _arrivals(self, f):
        """The edges frame f brings: every older patch into frame f, then every patch of frame f into frames 0 .. f."""
        M, dev = self.M, self.device
        older = torch.arange(f * M, device=dev)
        own = torch.arange(f * M, (f + 1) * M, device=dev).repeat_interleave(f + 1)
        patch = torch.cat([older, own])
        target = torch.cat([torch.full_like(older, f), torch.arange(f + 1, device=dev).repeat(M)])
        return torch.stack([patch // M, target, patch])

    def step(self, t, net, poses, patches, drop=False):
        """One iteration on copies of poses [1, N, 7] and patches [1, N M, 3, P, P]; net [1, E, dim] through torch.cat / a mask."""
        if not self.grows(t):
            return net, poses, patches
        f, M = self.n, self.M
        arrivals = self._arrivals(f)
        edges = torch.cat([arrivals, self.edges], dim=1)
        net = torch.cat([net.new_zeros(1, arrivals.shape[1], net.shape[2]), net], dim=1)
        self.keep = None
        if drop:
            stay = (edges[:2] != f - 4).all(dim=0)              # neither end of the edge is frame f - 4
            edges, net, self.keep = edges[:, stay], net[:, stay], stay
        poses, patches = poses.clone(), patches.clone()
        poses[0, f] = poses[0, f - 1]
        patches[0, f * M:(f + 1) * M, 2] = patches[0, max(f - 2, 0) * M:f * M, 2].median()      # the lower median of the last two frames' depths
        self.edges = edges
        self.n = int(edges[0].max()) + 1
        assert self.n == f + 1
        return net, poses, patches

    def _select(self, reach):
        gap = (self.edges[0] - self.edges[1]).abs()
        pos = ((gap > 0) & (gap <= reach)).nonzero().squeeze(1)
        return EdgeList(pos, *self.edges[:, pos])

    close = property(lambda self: self._select(2))
    far = property(lambda self: self._select(16))


def drive(n_frames, M, init_frames, warmup, steps, drops, P=3, seed=0, device="cpu", poses=None, patches=None):
    """The whole schedule on the given (or random) poses / patches: a list with one record per iteration (after its growth, if any)."""
    gen = torch.Generator().manual_seed(seed)
    poses = torch.randn(1, n_frames, 7, generator=gen).to(device) if poses is None else poses.to(device)
    patches = torch.rand(1, n_frames * M, 3, P, P, generator=gen).to(device) if patches is None else patches.to(device)
    g = RefTrainGraph(n_frames, M, init_frames, warmup, device)
    net = torch.zeros(1, len(g), 8, device=device)
    out = []
    for t in range(steps):
        net, poses, patches = g.step(t, net, poses, patches, drop=t in drops)
        c, f = g.close, g.far
        out.append(dict(ii=g.ii, jj=g.jj, kk=g.kk, n=g.n, close=c.pos, far=f.pos, pose=poses[0, g.n - 1].clone(), depths=patches[0, :, 2, 0, 0].clone()))
    return out, (poses, patches)
