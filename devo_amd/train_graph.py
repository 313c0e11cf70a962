"""The growing patch graph of DEVO's training loop on the GPU (devo/enet.py:297-339, the edge selections of :359-369) over
csrc/train_graph.hip.  The reference starts on the first 8 frames and, from the 8th update iteration on, adds one frame per iteration:
it prepends the new frame's edges (`torch.where` x 2, `torch.cat` x 4, all of `net` among them), copies the previous pose, initialises
the new depths with a `torch.median`, with probability 0.1 drops every edge of frame n - 4 (four boolean-mask gathers), reads `ii.max()`
twice, and selects the close and the scorer edges with more mask gathers in EVERY iteration — a `nonzero` and a host wait each.  Here a
growth is three launches (the initial graph two, an iteration that does not grow none) and nothing waits for the device: every size is
host arithmetic over a presence matrix of frame pairs (`GraphSizes`).  No CPU fallback.

Buffers: a training step keeps every iteration's index tensors alive until its backward (pops.transform, the lookup and the BA save
them), so a growth never writes a buffer an earlier iteration handed out: growth number g of a drive owns segment g (three rows of
(init_frames + g)^2 M int64 and the two lists), written once per drive.  `reset()` starts the next drive on the same segments; the Update
operator's graph tables, the BA's prepared tables and the lookup plan are keyed on (data_ptr, _version, numel) of the index tensors, and
two drives can reach one segment with equal sizes and different edges, so every call that writes a segment bumps its version counters
the way graph.py does."""
import collections
import numpy as np
import torch
from . import _lib as L
from . import backends
from .graph import _bump

MAX_FRAMES = 64               # DEVO_TRAIN_GRAPH_MAX_FRAMES
MEDIAN_MAX = 32768            # DEVO_FRAME_MEDIAN_MAX: depth values the median selects from (2 M P P)

EdgeList = collections.namedtuple("EdgeList", "pos ii jj kk")


class GraphSizes:
    """The host's model of the schedule: A[source frame][target frame], every present pair holds exactly M edges.  Pure host
    arithmetic (no torch, no device): E, |close|, |far| and n of every iteration without asking the device."""

    def __init__(self, n_frames, M, init_frames=8, warmup=8):
        self.n_frames, self.M, self.init_frames, self.warmup = int(n_frames), int(M), int(init_frames), int(warmup)
        i = np.arange(self.n_frames)
        d = np.abs(i[:, None] - i[None, :])
        self._close, self._far = (d > 0) & (d <= 2), (d > 0) & (d <= 16)
        self.reset()

    def reset(self):
        self.A = np.zeros((self.n_frames, self.n_frames), dtype=bool)
        self.A[:self.init_frames, :self.init_frames] = True
        self.n = self.init_frames

    def grows(self, t):
        return int(t) >= self.warmup and self.n < self.n_frames

    @staticmethod
    def after_growth(A, n, drop):
        """The presence matrix after the growth to frame n (enet.py:321-336); A is not modified."""
        A = A.copy()
        A[:n, n] = True
        A[n, :n + 1] = True
        if drop and n - 4 >= 0:
            A[n - 4, :] = False
            A[:, n - 4] = False
        return A

    def grow(self, drop=False):
        self.A = self.after_growth(self.A, self.n, drop)
        self.n += 1

    def counts(self, A=None):
        """(E, |close|, |far|)"""
        A = self.A if A is None else A
        return self.M * int(A.sum()), self.M * int((A & self._close).sum()), self.M * int((A & self._far).sum())

    def capacities(self, n):
        """(E, |close|, |far|) of the full graph on n frames: what growth number n - init_frames can hold at most (a drop only removes)."""
        return self.M * n * n, self.M * int(self._close[:n, :n].sum()), self.M * int(self._far[:n, :n].sum())

    E = property(lambda self: self.counts()[0])
    n_close = property(lambda self: self.counts()[1])
    n_far = property(lambda self: self.counts()[2])


class _Segment:
    def __init__(self, caps, device):
        # (not filled: the kernels write every element of every view that is handed out)
        self.idx = torch.empty(3, max(caps[0], 1), dtype=torch.int64, device=device)
        self.close = torch.empty(4, max(caps[1], 1), dtype=torch.int64, device=device)
        self.far = torch.empty(4, max(caps[2], 1), dtype=torch.int64, device=device)

    def written(self):
        for t in (self.idx, self.close, self.far):
            _bump(t)


class _Grow(torch.autograd.Function):
    """net -> net' of one growth (zero rows in front, the old rows behind them, compacted under a drop); poses' and patches' ride along
    without gradient (the reference detaches both at the top of every iteration)."""

    @staticmethod
    def forward(ctx, net, graph, poses, patches, drop):
        net_new, poses_new, patches_new, row_map, n_new = graph._launch_growth(net, poses, patches, drop)
        ctx.sizes = (net.shape[1], net_new.shape[1], n_new, net.shape[2])
        ctx.save_for_backward(row_map)
        ctx.mark_non_differentiable(poses_new, patches_new)
        return net_new, poses_new, patches_new

    @staticmethod
    def backward(ctx, g_net, _g_poses, _g_patches):
        E_old, E_new, n_new, dim = ctx.sizes
        row_map, = ctx.saved_tensors
        if row_map is None:                                   # no drop: the old rows lie behind the new ones, in order
            return g_net[:, n_new:], None, None, None, None
        g_net = g_net.contiguous()
        g_old = torch.empty(1, E_old, dim, dtype=g_net.dtype, device=g_net.device)
        nat = backends.native()
        with torch.cuda.device(g_net.device):
            if nat is not None:
                nat.train_graph.net_backward(g_net[0], row_map, g_old[0], E_new)
            else:
                rc = L.lib().devo_train_graph_net_backward(L.ptr(g_net), L.ptr(row_map), L.ptr(g_old), E_old, E_new, dim, L.dtype_code(g_net), L.stream())
                L.check(rc, "TrainGraph.step (backward)")
        return g_old, None, None, None, None


class TrainGraph:
    """The training graph of one sequence whose patches are frame-major with M per frame (ix = arange(n_frames).repeat_interleave(M): what
    the Patchifier returns in training).  ii, jj, kk: int64 [E] views of device buffers (what Update / BA / altcorr / pops.transform take);
    close / far: EdgeList(pos, ii, jj, kk) of the edges with 0 < |ii - jj| <= 2 / <= 16, in edge order; n: frames in the graph and
    len(g) = E, host ints.  One stream per graph: the methods enqueue on the current stream and share one workspace.  Nothing is built on
    the device before the first access, and no method waits for it or copies from it."""

    def __init__(self, n_frames, M, P=3, dim=384, init_frames=8, warmup=8, device="cuda"):
        n_frames, M, P, dim, init_frames, warmup = int(n_frames), int(M), int(P), int(dim), int(init_frames), int(warmup)
        if n_frames < 1 or n_frames > MAX_FRAMES:
            raise ValueError(f"TrainGraph: 1 <= n_frames <= {MAX_FRAMES}, got {n_frames}")
        if init_frames < 1 or init_frames > n_frames:
            raise ValueError(f"TrainGraph: 1 <= init_frames <= n_frames = {n_frames}, got {init_frames}")
        if M < 1 or P < 1 or warmup < 0:
            raise ValueError("TrainGraph: M and P must be positive, warmup not negative")
        if 2 * M * P * P > MEDIAN_MAX:
            raise ValueError(f"TrainGraph: the depth median selects from 2 M P P = {2 * M * P * P} values, at most {MEDIAN_MAX}")
        if dim <= 0 or dim % 8:
            raise ValueError(f"TrainGraph: dim must be a positive multiple of 8 (rows of net move as 16-byte words), got {dim}")
        self.n_frames, self.M, self.P, self.dim = n_frames, M, P, dim
        self.capacity = n_frames * n_frames * M
        self.device = torch.device(device)
        self.sizes = GraphSizes(n_frames, M, init_frames, warmup)
        self._segments = {}
        self._g = 0                                            # growths of this drive = the segment that holds the graph
        self._built = False
        self._ws = None
        self._views = None

    # ------------------------------------------------------------------------------------------ state
    n = property(lambda self: self.sizes.n)

    def __len__(self):
        return self.sizes.E

    def grows(self, t):
        """Does iteration t grow the graph?  Host arithmetic: t >= warmup and n < n_frames."""
        return self.sizes.grows(t)

    def _segment(self, g):
        seg = self._segments.get(g)
        if seg is None:
            seg = self._segments[g] = _Segment(self.sizes.capacities(self.sizes.init_frames + g), self.device)
        return seg

    def _ready(self, what, *tensors):
        """Everything that can be refused is refused before any launch: the graph is unchanged by an error."""
        if self.device.type != "cuda":
            raise RuntimeError("devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
        L.require_gpu(*tensors)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"TrainGraph.{what} cannot be captured into a graph: the sizes of its results are host data")
        for t in tensors:
            if t.device != self._device():
                raise RuntimeError(f"TrainGraph.{what}: the graph lives on {self._device()}, got a tensor on {t.device}")
        if self._ws is None:
            with torch.cuda.device(self._device()):
                self._ws = torch.empty(L.lib().devo_train_graph_workspace_bytes(self.capacity), dtype=torch.uint8, device=self._device())

    def _device(self):
        if self.device.index is None and self.device.type == "cuda":
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _build(self):
        """The initial graph (enet.py:300-301) into segment 0: two launches."""
        if self._built:
            return
        self._ready("init")
        seg = self._segment(0)
        nat = backends.native()
        with torch.cuda.device(self.device):
            if nat is not None:
                nat.train_graph.init(seg.idx, self.M, self.sizes.init_frames, seg.close, seg.far, self._ws)
            else:
                rc = L.lib().devo_train_graph_init(L.ptr(seg.idx), seg.idx.shape[1], self.M, self.sizes.init_frames, L.ptr(seg.close), seg.close.shape[1], L.ptr(seg.far),
                                                   seg.far.shape[1], L.ptr(self._ws), self._ws.numel(), L.stream())
                L.check(rc, "TrainGraph (initial graph)")
        seg.written()
        self._built = True
        self._views = None

    def reset(self):
        """Back to the initial graph, on the same buffers: the next sequence.  Every tensor a finished drive handed out is dead after this."""
        self._ready("reset")
        self.sizes.reset()
        self._g = 0
        self._built = False
        self._views = None
        self._build()

    def _lists(self):
        if self._views is None:
            self._build()
            seg = self._segments[self._g]
            E, nc, nf = self.sizes.counts()
            self._views = (tuple(seg.idx[r, :E] for r in range(3)), EdgeList(*(seg.close[r, :nc] for r in range(4))), EdgeList(*(seg.far[r, :nf] for r in range(4))))
        return self._views

    ii = property(lambda self: self._lists()[0][0])
    jj = property(lambda self: self._lists()[0][1])
    kk = property(lambda self: self._lists()[0][2])
    close = property(lambda self: self._lists()[1])
    far = property(lambda self: self._lists()[2])

    # ------------------------------------------------------------------------------------------ enet.py:314-339
    def step(self, t, net, poses, patches, drop=False):
        """Iteration t of the loop.  Shapes and dtypes are checked in every iteration; then it grows when t >= warmup and n < n_frames
        (host arithmetic), else returns its inputs unchanged and launches nothing.  A growth returns (net', poses', patches') — new tensors, the inputs are not written — and refreshes ii, jj, kk,
        close and far.  net: [1, E, dim] fp16 or fp32 (gradient flows through it); poses: [1, n_frames, 7] and patches:
        [1, n_frames M, 3, P, P], fp32.  drop: the caller's draw (np.random.rand() < 0.1, only inside a growth)."""
        E = self.sizes.E
        if not isinstance(net, torch.Tensor) or tuple(net.shape) != (1, E, self.dim):
            raise ValueError(f"TrainGraph.step: expected net of shape (1, {E}, {self.dim}), got {tuple(getattr(net, 'shape', ()))}")
        if net.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"TrainGraph.step: net is fp16 or fp32, got {net.dtype}")
        if poses.numel() != self.n_frames * 7 or patches.numel() != self.n_frames * self.M * 3 * self.P * self.P or patches.shape[-1] != self.P:
            raise ValueError(f"TrainGraph.step: expected poses of {self.n_frames} rows and patches of {self.n_frames * self.M} x 3 x {self.P} x {self.P}")
        if poses.dtype != torch.float32 or patches.dtype != torch.float32:
            raise ValueError("TrainGraph.step: poses and patches are fp32")
        if not self.sizes.grows(t):
            return net, poses, patches
        self._ready("step", net, poses, patches)
        self._build()
        return _Grow.apply(net, self, poses, patches, bool(drop))

    def _launch_growth(self, net, poses, patches, drop):
        sz, n = self.sizes, self.sizes.n
        drop = bool(drop) and n - 4 >= 0                       # (n - 4 < 0: the reference's mask keeps everything)
        E_old = sz.E
        A = sz.after_growth(sz.A, n, drop)
        E_new = sz.counts(A)[0]
        n_new = self.M * (2 * n + 1)
        net, poses, patches = net.contiguous(), poses.contiguous(), patches.contiguous()
        dev = self.device
        src, dst = self._segments[self._g], self._segment(self._g + 1)
        net_new = torch.empty(1, E_new, self.dim, dtype=net.dtype, device=dev)
        poses_new, patches_new = torch.empty_like(poses), torch.empty_like(patches)
        row_map = torch.empty(E_old, dtype=torch.int32, device=dev) if drop else None
        nat = backends.native()
        with torch.cuda.device(dev):
            if nat is not None:
                nat.train_graph.grow(src.idx, E_old, dst.idx, E_new, self.M, n, drop, net[0], net_new[0], row_map, poses, poses_new, patches, patches_new, dst.close, dst.far,
                                     self._ws)
            else:
                rc = L.lib().devo_train_graph_grow(L.ptr(src.idx), src.idx.shape[1], E_old, L.ptr(dst.idx), dst.idx.shape[1], E_new, self.M, n, int(drop), L.ptr(net),
                                                   L.ptr(net_new), self.dim, L.dtype_code(net), L.ptr(row_map), L.ptr(poses), L.ptr(poses_new), self.n_frames, L.ptr(patches),
                                                   L.ptr(patches_new), self.P, L.ptr(dst.close), dst.close.shape[1], L.ptr(dst.far), dst.far.shape[1], L.ptr(self._ws),
                                                   self._ws.numel(), L.stream())
                L.check(rc, "TrainGraph.step")
        dst.written()
        sz.A, sz.n = A, n + 1
        self._g += 1
        self._views = None
        return net_new, poses_new, patches_new, row_map, n_new
