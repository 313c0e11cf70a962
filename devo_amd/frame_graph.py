"""The training frame graph of one scene on the GPU (devo/data_readers/base.py:263-286 over rgbd_utils.py:104-141) over
csrc/frame_graph.hip, and the clip sampler that walks it (base.py:244-250, :302-341).

The reference builds the graph once per scene and pickles it: for all N^2 ordered pairs of frames it reprojects every pixel of the
f-times subsampled depth maps in both directions (each unordered pair four times over), in chunks of 2048 pairs of about sixty eager ops
with a copy to the host per chunk, and assembles a dict of neighbour lists on the host.  Here a build is seven launches and one read-back
of the total list length: the disparity preparation (1), the all-pairs flow distance with each directed pair computed once (3) and the
CSR lists (2 + 1).  Results are bit-reproducible (no atomics).  No CPU fallback: the build needs the GPU; what reads a finished graph
(`from_reference`, `to_reference`, `dataset_index`, `sample_clip`) is host code.
"""
import numpy as np
import torch
from . import _lib as L
from . import backends

MAX_FRAMES = 32768            # DEVO_FRAME_GRAPH_MAX_FRAMES
MAX_POINTS = 1 << 20          # DEVO_FRAME_GRAPH_MAX_POINTS: 2 h w stays below it


def _upload(x, what):
    """A float32 contiguous device tensor of a device tensor or a numpy array (uploaded); a CPU tensor raises as everywhere else."""
    if isinstance(x, torch.Tensor):
        L.require_gpu(x)
        return x.float().contiguous()
    if not torch.cuda.is_available():
        raise RuntimeError(f"devo_amd: {what} must go to the GPU (the HIP path has no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).cuda()


def _shapes(poses, maps, intrinsics, what):
    if maps.dim() != 3 or poses.dim() != 2 or intrinsics.dim() != 2 or poses.shape[1] != 7 or intrinsics.shape[1] != 4:
        raise ValueError(f"{what}: expected poses [N, 7], maps [N, h, w] and intrinsics [N, 4]")
    N = maps.shape[0]
    if poses.shape[0] != N or intrinsics.shape[0] != N:
        raise ValueError(f"{what}: {poses.shape[0]} poses, {N} maps and {intrinsics.shape[0]} intrinsics: one N expected")
    if N < 1 or N > MAX_FRAMES:
        raise ValueError(f"{what}: 1 <= N <= {MAX_FRAMES}, got {N}")
    if poses.device != maps.device or intrinsics.device != maps.device:
        raise RuntimeError(f"{what}: the tensors live on different devices")


def _workspace(N, h, w, device):
    return torch.empty(L.lib().devo_frame_graph_workspace_bytes(N, h, w), dtype=torch.uint8, device=device)


def prepare_disps(depths_sub):
    """depths [N, h, w] (already subsampled) -> 1 / depth with every depth below 0.01 replaced by its frame's mean (base.py:265-268)."""
    depths = _upload(depths_sub, "the depth maps")
    if depths.dim() != 3 or depths.shape[0] < 1:
        raise ValueError("frame_graph.prepare_disps: expected depths [N, h, w]")
    nat = backends.native()
    with torch.cuda.device(depths.device):
        if nat is not None:
            return nat.frame_graph.disps(depths)
        out = torch.empty_like(depths)
        N, h, w = depths.shape
        L.check(L.lib().devo_frame_graph_disps(L.ptr(depths), L.ptr(out), N, h, w, L.stream()), "frame_graph.prepare_disps")
    return out


def _distances(poses, disps, intrinsics, scale):
    _shapes(poses, disps, intrinsics, "frame_graph.distance_matrix")
    nat = backends.native()
    with torch.cuda.device(disps.device):
        if nat is not None:
            return nat.frame_graph.distances(poses, disps, intrinsics, float(scale))
        N, h, w = disps.shape
        ws = _workspace(N, h, w, disps.device)
        matrix = torch.empty(N, N, dtype=torch.float32, device=disps.device)
        rc = L.lib().devo_frame_graph_distances(L.ptr(poses), L.ptr(disps), L.ptr(intrinsics), N, h, w, float(scale), L.ptr(matrix), L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, "frame_graph.distance_matrix")
    return matrix


def distance_matrix(poses, disps, intrinsics):
    """The unscaled matrix of rgbd_utils.compute_distance_matrix_flow: poses [N, 7] camera-to-world (t, q), disps [N, h, w], intrinsics
    [N, 4] at the maps' resolution -> float32 [N, N] on the device, +inf where fewer than 70 % of a pair's points are valid."""
    return _distances(_upload(poses, "the poses"), _upload(disps, "the disparities"), _upload(intrinsics, "the intrinsics"), 1.0)


def _lists(matrix, max_flow):
    nat = backends.native()
    with torch.cuda.device(matrix.device):
        if nat is not None:
            return nat.frame_graph.lists(matrix, float(max_flow))
        N = matrix.shape[0]
        ws = _workspace(N, 1, 1, matrix.device)
        rowptr = torch.empty(N + 1, dtype=torch.int64, device=matrix.device)
        args = (L.ptr(matrix), N, float(max_flow), L.ptr(rowptr))
        L.check(L.lib().devo_frame_graph_lists(*args, None, None, 0, L.ptr(ws), ws.numel(), L.stream()), "frame_graph.build_frame_graph (degrees)")
        total = int(rowptr[N])                                 # the one read-back
        cols = torch.empty(total, dtype=torch.int64, device=matrix.device)
        dists = torch.empty(total, dtype=torch.float32, device=matrix.device)
        if total:
            L.check(L.lib().devo_frame_graph_lists(*args, L.ptr(cols), L.ptr(dists), total, L.ptr(ws), ws.numel(), L.stream()), "frame_graph.build_frame_graph (lists)")
    return rowptr, cols, dists


class FrameGraph:
    """Neighbour lists in CSR form: row i holds the frames j with distance < max_flow in ascending j (`cols` int64) and their distances
    (`dists` float32); `rowptr` int64 [n + 1].  The tensors stay where they were built (the device for build_frame_graph, the host for
    from_reference); the host-side readers work on one cached host copy."""

    def __init__(self, rowptr, cols, dists):
        self.rowptr, self.cols, self.dists = rowptr, cols, dists
        self.n = int(rowptr.numel()) - 1
        self._host_arrays = None

    def _host(self):
        if self._host_arrays is None:
            self._host_arrays = tuple(t.cpu().numpy() for t in (self.rowptr, self.cols, self.dists))
        return self._host_arrays

    def neighbours(self, i):
        """(frames int64, distances float32) of row i, as host arrays (views of the host copy)."""
        rowptr, cols, dists = self._host()
        if not 0 <= int(i) < self.n:
            raise IndexError(f"FrameGraph: frame {i} of {self.n}")
        a, b = int(rowptr[int(i)]), int(rowptr[int(i) + 1])
        return cols[a:b], dists[a:b]

    def to_reference(self):
        """The reference's {i: (int64 array, float32 array)} dict (what it pickles as scene_info[scene]['graph'])."""
        return {i: tuple(x.copy() for x in self.neighbours(i)) for i in range(self.n)}

    @classmethod
    def from_reference(cls, graph):
        """The CSR of such a dict (an existing pickle's graph); host tensors, no GPU needed."""
        n = len(graph)
        if sorted(graph) != list(range(n)):
            raise ValueError("FrameGraph.from_reference: the keys must be the frames 0 .. n - 1")
        degree = np.array([len(graph[i][0]) for i in range(n)], dtype=np.int64)
        rowptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(degree)])
        cols = np.concatenate([np.asarray(graph[i][0], dtype=np.int64).reshape(-1) for i in range(n)]) if n else np.zeros(0, np.int64)
        dists = np.concatenate([np.asarray(graph[i][1], dtype=np.float32).reshape(-1) for i in range(n)]) if n else np.zeros(0, np.float32)
        if len(cols) != len(dists) or len(cols) != rowptr[-1]:
            raise ValueError("FrameGraph.from_reference: every row needs as many distances as frames")
        return cls(torch.from_numpy(rowptr), torch.from_numpy(cols), torch.from_numpy(dists))

    def dataset_index(self, n_frames):
        """The frames a clip of n_frames may start at: the rows with more than n_frames neighbours (base.py:244-250)."""
        rowptr = self._host()[0]
        return [int(i) for i in np.nonzero(np.diff(rowptr) > n_frames)[0]]

    def sample_clip(self, ix, n_frames, fmin, fmax, n_total, sample=True):
        """The frame indices of one training clip that starts at frame ix (EVSDDataset.__getitem__, base.py:302-341), int64 [n_frames].
        n_total: frames in the scene.  Consumes np.random in the reference's order — uniform(fmin, fmax), choice([1, 2, 3]), then one
        choice per sampled step — so after np.random.seed(s) it returns the reference's indices.
        sample=True: a random neighbour ahead of the current frame whose distance lies strictly inside (fmin, fmax); without one the next
        frame; at the scene's end a random such neighbour, if there is one.  sample=False: the most distant neighbour within the drawn
        distance in the walking direction, else a step of the drawn stride, turning round at either end of the scene."""
        reach = np.random.uniform(fmin, fmax)
        stride = np.random.choice([1, 2, 3])
        ix = int(ix)
        clip = [ix]
        while len(clip) < n_frames:
            frames, dist = self.neighbours(ix)
            if sample:
                inside = frames[(dist > fmin) & (dist < fmax)]
                ahead = inside[inside > ix]
                if ahead.size:
                    ix = int(np.random.choice(ahead))
                elif ix + 1 < n_total:
                    ix += 1
                elif np.count_nonzero(inside):                 # (the reference counts non-zero frame NUMBERS: frame 0 alone does not count)
                    ix = int(np.random.choice(inside))
            else:
                onward = frames > ix if stride > 0 else frames < ix
                score = np.where(onward & (dist <= reach), dist, np.float32(-1))
                if score.size and score.max() > 0:
                    ix = int(frames[np.argmax(score)])
                else:
                    if ix + stride >= n_total or ix + stride < 0:
                        stride = -stride
                    ix += int(stride)
            clip.append(ix)
        return np.asarray(clip, dtype=np.int64)


def build_frame_graph(poses, depths_sub, intrinsics, f=16, max_flow=256.0):
    """EVSDDataset.build_frame_graph on the GPU.  poses [N, 7] camera-to-world (t, q); depths_sub [N, h, w]: the depth maps as the caller
    sliced them while reading, depth[f//2::f, f//2::f] (full-size maps never go to the device); intrinsics [N, 4] at FULL resolution
    (divided by f here, base.py:271).  Device tensors, or numpy arrays that are uploaded.  -> FrameGraph on the device, distances in pixels
    of the full-size frame (f x the matrix)."""
    if isinstance(intrinsics, torch.Tensor):
        L.require_gpu(intrinsics)
        intr = (intrinsics / f).float().contiguous()
    else:
        intr = _upload(np.asarray(intrinsics) / f, "the intrinsics")
    poses = _upload(poses, "the poses")
    depths = _upload(depths_sub, "the depth maps")
    _shapes(poses, depths, intr, "frame_graph.build_frame_graph")
    matrix = _distances(poses, prepare_disps(depths), intr, float(f))
    return FrameGraph(*_lists(matrix, max_flow))
