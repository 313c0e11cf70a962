"""The patch graph of DEVO's inference on the GPU: the bookkeeping that closes every frame (devo/devo.py:225-239 `append_factors` /
`remove_factors`, :258-265 `motionmag`, :267-306 `keyframe`) over csrc/graph.hip.  The reference runs it in eager torch: boolean-mask
gathers (a `nonzero` and a host synchronisation each), `torch.cat` of the index lists and of the whole recurrent state `net`, `.item()`.
Here the edge lists live in capacity-sized device buffers, the keyframe decision is taken on the device, and a call waits at most once,
for one pinned host record.  This is NOT a drop-in under a reference module name (the reference has no extension here): INTEGRATION.md
shows the four `DEVO` methods rewritten over `PatchGraph`.  No CPU fallback.

Cache soundness: the Update operator's graph tables, the BA's prepared tables and the lookup plan are keyed on (data_ptr, _version,
numel) of the index tensors.  The kernels write through raw pointers and the two halves of the index buffers alternate, so every method
that writes a half bumps its version counter (shared by the `[:E]` views handed out) — without a launch."""
import collections
import ctypes
import torch
from . import _lib as L
from . import backends

KeyframeResult = collections.namedtuple("KeyframeResult", "removed k motion n_edges")
SHIFT_MAX = 8                 # DEVO_GRAPH_SHIFT_MAX: tensors to one launch of shift_frames

_increment_version = getattr(torch.autograd.graph, "increment_version", None)


def _bump(t):
    """Count a kernel's raw-pointer write as an in-place edit of `t` (and of every view of its storage)."""
    if _increment_version is not None:
        _increment_version(t)
    else:
        n = backends.native()
        if n is None:
            raise RuntimeError("devo_amd.graph: this torch has no torch.autograd.graph.increment_version and the compiled binding is not built")
        n.bump_version(t)


def _no_capture(what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"PatchGraph.{what} cannot be captured into a graph: the sizes of its results are host data")


class PatchGraph:
    """ii, jj, kk: int64 [E] views of capacity-sized device buffers (what Update / fastba.BA / altcorr take); net: [1, E, dim] fp16 or
    fp32, assignable (the operator returns a new tensor every iteration: adopted by reference, never copied); len(g) = E, a host int.
    One stream per graph: the methods enqueue on the current stream and share one workspace."""

    def __init__(self, M, dim=384, capacity=1 << 17, device="cuda", dtype=torch.float32):
        if int(dim) <= 0 or int(dim) % 8:
            raise ValueError(f"PatchGraph: dim must be a positive multiple of 8 (rows of net move as 16-byte words), got {dim}")
        if dtype not in (torch.float16, torch.float32):
            raise ValueError(f"PatchGraph: net is fp16 or fp32, got {dtype}")
        if int(capacity) <= 0 or int(M) <= 0:
            raise ValueError("PatchGraph: M and capacity must be positive")
        self.M, self.dim, self.capacity = int(M), int(dim), int(capacity)
        self.device = torch.device(device)
        self._buf = [torch.zeros(3, self.capacity, dtype=torch.int64, device=self.device) for _ in range(2)]     # the ping-pong pair: rows ii, jj, kk
        self._cur = 0
        self._E = 0
        self._net = torch.zeros(1, 0, self.dim, dtype=dtype, device=self.device)
        self._ws = self._record = self._record_f = self._event = None
        self._views = None

    # ------------------------------------------------------------------------------------------ state
    def __len__(self):
        return self._E

    def _idx(self):
        if self._views is None:
            b = self._buf[self._cur]
            self._views = (b[0, :self._E], b[1, :self._E], b[2, :self._E])
        return self._views

    ii = property(lambda self: self._idx()[0])
    jj = property(lambda self: self._idx()[1])
    kk = property(lambda self: self._idx()[2])

    @property
    def net(self):
        return self._net

    @net.setter
    def net(self, value):
        if not isinstance(value, torch.Tensor) or tuple(value.shape) != (1, self._E, self.dim):
            raise ValueError(f"PatchGraph.net: expected a tensor of shape (1, {self._E}, {self.dim}), got {tuple(getattr(value, 'shape', ()))}")
        if value.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"PatchGraph.net: fp16 or fp32, got {value.dtype}")
        if value.device != self._net.device:
            raise RuntimeError(f"PatchGraph.net: the graph lives on {self._net.device}, got a tensor on {value.device}")
        self._net = value

    def _ready(self, what, *tensors):
        """Everything that can be refused is refused here, before any launch: the graph is unchanged by an error."""
        L.require_gpu(self._buf[0], *tensors)
        _no_capture(what)
        dev = self._buf[0].device
        for t in tensors:
            if t is not None and t.device != dev:
                raise RuntimeError(f"PatchGraph.{what}: the graph lives on {dev}, got a tensor on {t.device}")
        net = self._net
        if not net.is_contiguous() or (net.numel() and net.stride(-1) != 1):
            raise RuntimeError(f"PatchGraph.{what}: net must be contiguous (its rows move as 16-byte words)")
        if net.numel() and net.data_ptr() % 16:
            raise RuntimeError(f"PatchGraph.{what}: net must be 16-byte aligned")
        if self._ws is None:
            with torch.cuda.device(dev):
                self._ws = torch.empty(L.lib().devo_graph_workspace_bytes(self.capacity), dtype=torch.uint8, device=dev)
                self._record = torch.zeros(4, dtype=torch.int32).pin_memory()          # {removed, n_edges, mean_ij, mean_ji}: this graph's own
                self._record_f = self._record.view(torch.float32)
                self._event = torch.cuda.Event()

    def _wait(self):
        """The one wait of a call: for the record its last kernel wrote, not for the stream."""
        self._event.record()
        self._event.synchronize()
        removed, n_edges = self._record[:2].tolist()
        mean_ij, mean_ji = self._record_f[2:].tolist()
        return bool(removed), int(n_edges), mean_ij, mean_ji

    @staticmethod
    def _geometry(poses, patches, intrinsics):
        poses = getattr(poses, "data", poses)
        L.require_gpu(poses, patches, intrinsics)
        f = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        poses, patches, intrinsics = f(poses), f(patches), f(intrinsics)
        P = patches.shape[-1]
        return poses, patches, intrinsics, poses.numel() // 7, patches.numel() // (3 * P * P), P

    def _adopt(self, n_edges, net_out):
        """The other half of the index pair now holds the graph."""
        self._cur ^= 1
        _bump(self._buf[self._cur])
        self._E = n_edges
        self._net = net_out[:, :n_edges]
        self._views = None

    # ------------------------------------------------------------------------------------------ devo.py:225-233
    def append(self, patch_ids, frame_ids, ix):
        """append_factors(ii = patch_ids, jj = frame_ids): kk += patch_ids, jj += frame_ids, ii += ix[patch_ids], net += zero rows.
        One launch, no wait."""
        self._ready("append", patch_ids, frame_ids, ix)
        n_new = patch_ids.numel()
        if frame_ids.numel() != n_new:
            raise ValueError("PatchGraph.append: patch_ids and frame_ids must have the same length")
        E = self._E
        if E + n_new > self.capacity:
            raise RuntimeError(f"PatchGraph.append: {E} + {n_new} edges exceed the capacity {self.capacity}")
        i64 = lambda t: t.reshape(-1) if (t.dtype == torch.int64 and t.is_contiguous()) else t.reshape(-1).long().contiguous()
        patch_ids, frame_ids, ix = i64(patch_ids), i64(frame_ids), i64(ix)
        b = self._buf[self._cur]
        net_new = torch.empty(1, E + n_new, self.dim, dtype=self._net.dtype, device=b.device)
        n = backends.native()
        with torch.cuda.device(b.device):
            if n is not None:
                n.patch_graph.append(b[0], b[1], b[2], self._net, net_new, ix, patch_ids, frame_ids, E, n_new)
            else:
                rc = L.lib().devo_graph_append(L.ptr(b[0]), L.ptr(b[1]), L.ptr(b[2]), L.ptr(self._net), L.ptr(net_new), L.ptr(ix), ix.numel(), L.ptr(patch_ids),
                                               L.ptr(frame_ids), E, n_new, self.capacity, self.dim, L.dtype_code(net_new), L.stream())
                L.check(rc, "PatchGraph.append")
        _bump(b)
        self._E = E + n_new
        self._net = net_new
        self._views = None

    # ------------------------------------------------------------------------------------------ devo.py:366-380, :541-542
    def append_frame(self, n, lifetime, ix):
        """The window edges of a new frame, for a state of n frames (after the increment of devo.py:537): append_factors(*edges_forw)
        followed by append_factors(*edges_back) with r = lifetime — patches M max(n - r, 0) .. M (n - 1) - 1 -> frame n - 1, then patches
        M (n - 1) .. M n - 1 -> frames max(n - r, 0) .. n - 1 in flatmeshgrid's `ij` order.  The ids are computed in the kernel: one
        launch, no index lists, no wait; the graph is what two `append` calls with the torch-built lists leave."""
        self._ready("append_frame", ix)
        n, lifetime = int(n), int(lifetime)
        if n < 1 or lifetime < 1:
            raise ValueError(f"PatchGraph.append_frame: a state of n = {n} frames with a patch lifetime of {lifetime} has no window edges")
        nat = backends.native()
        n_new = int(nat.patch_graph.append_frame_edges(self.M, n, lifetime) if nat is not None else L.lib().devo_odom_append_frame_edges(self.M, n, lifetime))
        E = self._E
        if E + n_new > self.capacity:
            raise RuntimeError(f"PatchGraph.append_frame: {E} + {n_new} edges exceed the capacity {self.capacity}")
        if ix.dtype != torch.int64 or not ix.is_contiguous():
            ix = ix.reshape(-1).long().contiguous()
        b = self._buf[self._cur]
        net_new = torch.empty(1, E + n_new, self.dim, dtype=self._net.dtype, device=b.device)
        with torch.cuda.device(b.device):
            if nat is not None:
                nat.patch_graph.append_frame(b[0], b[1], b[2], self._net, net_new, ix, self.M, n, lifetime, E)
            else:
                rc = L.lib().devo_odom_append_frame(L.ptr(b[0]), L.ptr(b[1]), L.ptr(b[2]), L.ptr(self._net), L.ptr(net_new), L.ptr(ix), ix.numel(), self.M, n, lifetime, E,
                                                    self.capacity, self.dim, L.dtype_code(net_new), L.stream())
                L.check(rc, "PatchGraph.append_frame")
        _bump(b)
        self._E = E + n_new
        self._net = net_new
        self._views = None

    # ------------------------------------------------------------------------------------------ devo.py:235-239
    def remove(self, mask):
        """remove_factors(mask): ii, jj, kk = x[~mask], net = net[:, ~mask], order kept.  Waits once (for the new edge count)."""
        self._ready("remove", mask)
        E = self._E
        if mask.numel() != E or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"PatchGraph.remove: the mask must be a bool tensor of {E} entries")
        if E == 0:
            return                                                       # nothing to compact, nothing to launch
        mask = mask.reshape(-1).contiguous()
        src, dst = self._buf[self._cur], self._buf[self._cur ^ 1]
        net_out = torch.empty(1, E, self.dim, dtype=self._net.dtype, device=src.device)
        n = backends.native()
        with torch.cuda.device(src.device):
            if n is not None:
                n.patch_graph.remove(src[0], src[1], src[2], self._net, mask, dst[0], dst[1], dst[2], net_out, E, self._ws, self._record)
            else:
                rc = L.lib().devo_graph_remove(L.ptr(src[0]), L.ptr(src[1]), L.ptr(src[2]), L.ptr(self._net), L.ptr(mask), L.ptr(dst[0]), L.ptr(dst[1]), L.ptr(dst[2]),
                                               L.ptr(net_out), E, self.dim, L.dtype_code(net_out), L.ptr(self._ws), self._ws.numel(), L.ptr(self._record), L.stream())
                L.check(rc, "PatchGraph.remove")
            _, n_edges, _, _ = self._wait()
        self._adopt(n_edges, net_out)

    # ------------------------------------------------------------------------------------------ devo.py:258-265
    def motion(self, poses, patches, intrinsics, i, j, beta=0.5):
        """(motionmag(i, j), motionmag(j, i)) as Python floats: the mean of pops.flow_mag over the edges i -> j and j -> i, NaN where
        there is none.  One pass over all edges, one wait; reproducible from run to run."""
        poses, patches, intrinsics, n_poses, n_patches, P = self._geometry(poses, patches, intrinsics)
        self._ready("motion", poses, patches, intrinsics)
        b = self._buf[self._cur]
        n = backends.native()
        with torch.cuda.device(b.device):
            if n is not None:
                n.patch_graph.motion(poses, patches, intrinsics, b[0], b[1], b[2], self._E, int(i), int(j), float(beta), self._ws, self._record)
            else:
                rc = L.lib().devo_graph_motion(L.ptr(poses), L.ptr(patches), L.ptr(intrinsics), L.ptr(b[0]), L.ptr(b[1]), L.ptr(b[2]), self._E, n_poses, n_patches, P,
                                               int(i), int(j), float(beta), L.ptr(self._ws), self._ws.numel(), L.ptr(self._record), L.stream())
                L.check(rc, "PatchGraph.motion")
            _, _, mean_ij, mean_ji = self._wait()
        return mean_ij, mean_ji

    # ------------------------------------------------------------------------------------------ devo.py:267-287, :305-306
    def keyframe(self, poses, patches, intrinsics, ix, n, keyframe_index=4, thresh=12.5, removal_window=20, beta=0.5):
        """The graph half of DEVO.keyframe for a state of n frames: k = n - keyframe_index; if (motionmag(k - 1, k + 1) +
        motionmag(k + 1, k - 1)) / 2 < thresh — decided on the device — the edges of frame k go and the rest is renumbered (the caller
        then shifts its frame buffers, `shift_frames`, and decrements n); then the edges of patches older than n' - removal_window go.
        Returns KeyframeResult(removed, k, motion = that mean, n_edges).  Enqueues its launches, then waits once."""
        poses, patches, intrinsics, n_poses, n_patches, P = self._geometry(poses, patches, intrinsics)
        self._ready("keyframe", poses, patches, intrinsics, ix)
        if ix.dtype != torch.int64 or not ix.is_contiguous():
            ix = ix.long().contiguous()
        E, n = self._E, int(n)
        src, dst = self._buf[self._cur], self._buf[self._cur ^ 1]
        net_out = torch.empty(1, E, self.dim, dtype=self._net.dtype, device=src.device)
        nat = backends.native()
        with torch.cuda.device(src.device):
            if nat is not None:
                nat.patch_graph.keyframe(poses, patches, intrinsics, src[0], src[1], src[2], self._net, ix, dst[0], dst[1], dst[2], net_out, E, self.M, n,
                                         int(keyframe_index), float(thresh), int(removal_window), float(beta), self._ws, self._record)
            else:
                rc = L.lib().devo_graph_keyframe(L.ptr(poses), L.ptr(patches), L.ptr(intrinsics), L.ptr(src[0]), L.ptr(src[1]), L.ptr(src[2]), L.ptr(self._net), L.ptr(ix),
                                                 L.ptr(dst[0]), L.ptr(dst[1]), L.ptr(dst[2]), L.ptr(net_out), E, n_poses, n_patches, ix.numel(), P, self.dim,
                                                 L.dtype_code(net_out), self.M, n, int(keyframe_index), float(thresh), int(removal_window), float(beta),
                                                 L.ptr(self._ws), self._ws.numel(), L.ptr(self._record), L.stream())
                L.check(rc, "PatchGraph.keyframe")
            removed, n_edges, mean_ij, mean_ji = self._wait()
        self._adopt(n_edges, net_out)
        return KeyframeResult(removed, n - int(keyframe_index), (mean_ij + mean_ji) / 2, n_edges)


def shift_frames(tensors, k, n):
    """devo.py:289-295 for the per-frame state (poses, patches, intrinsics, timestamps, colours, ...): rows k + 1 .. n - 1 of each
    tensor move down by one, in place, one launch per 8 tensors of any dtype.  The feature rings (imap_, gmap_, fmap1_, fmap2_) are
    NOT for this call: they stay on Tensor.__setitem__, whose write records backends/ring.py keeps."""
    tensors = [t for t in tensors if t.numel()]
    k, n = int(k), int(n)
    L.require_gpu(*tensors)
    if k < 0:
        raise ValueError(f"shift_frames: k = {k}")
    for t in tensors:
        if t.dim() < 1 or not t.is_contiguous() or t.shape[0] < n:
            raise ValueError("shift_frames: every tensor must be contiguous and hold at least n rows")
        if t.device != tensors[0].device:
            raise RuntimeError("shift_frames: the tensors must live on one device")
    if not tensors or k >= n - 1:
        return
    nat = backends.native()
    with torch.cuda.device(tensors[0].device):
        for s in range(0, len(tensors), SHIFT_MAX):
            part = tensors[s:s + SHIFT_MAX]
            if nat is not None:
                nat.patch_graph.shift_frames(part, k, n)
            else:
                ptrs = (ctypes.c_void_p * len(part))(*[t.data_ptr() for t in part])
                rows = L.i64arr([t.numel() // t.shape[0] * t.element_size() for t in part])
                L.check(L.lib().devo_graph_shift_frames(ptrs, rows, len(part), k, n, L.stream()), "shift_frames")
    for t in tensors:
        _bump(t)
