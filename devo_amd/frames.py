"""The per-frame state of DEVO's inference on the GPU, over csrc/frames.hip: what devo/devo.py does per frame and per sequence BETWEEN
the update step, the Patchifier and the patch graph — the frame store with the motion model and the depth initialisation (:487-488,
:502-520), the point cloud behind every update (:342-344), the relative-pose log (:276-280, :534) and terminate() (:179-196).  The
reference runs these as small eager ops (five lietorch launches for one pose, a sort for one median, a P x P point cloud for its centre
pixel) with `.item()` round trips and a recursive Python walk per frame; here each is one launch (terminate(): 1 + ceil(log2(counter))),
and the only wait is `Trajectory.complete`'s, behind its last kernel.  This is NOT a drop-in under a reference module name (the reference
has no extension here): INTEGRATION.md shows the `DEVO` lines rewritten over these calls.  No CPU fallback.
`frame_input` (the density gate, the normalisation and the 346-column crop of devo.py:406-467, two launches) and `probe_median` (the
quantile of :256, one) over csrc/frame_input.hip are the pieces of `__call__` in front of the Patchifier and behind the motion probe;
odometry.DEVO strings all of them together.

The frame buffers are the caller's (devo.py:56-65): poses fp32 [N, 7], patches fp32 [N, M, 3, P, P], intrinsics fp32 [N, 4], tstamps int64
[N] — or their `[1, ...]` views; they are written through raw pointers, so they must be contiguous and of these dtypes (nothing is
converted behind the caller's back), and every write bumps the tensor's version counter (graph.py: the version-keyed caches)."""
import torch
from . import _lib as L
from . import backends
from .graph import _bump

MEDIAN_MAX = 32768            # DEVO_FRAME_MEDIAN_MAX: depth values the median selects from, 3 M P P
_MODELS = {"DAMPED_LINEAR": 1}                # DEVO_FRAME_DAMPED_LINEAR; any other string: DEVO_FRAME_COPY_LAST, as devo.py:510-512
_STATUS = {1: "a log entry names a frame outside the capacity, or a parent that is not an earlier frame",
           2: "a frame below `counter` is neither a keyframe nor tied to one by log entries",
           3: "tstamps[:n] is not strictly increasing"}


def _state(what, t, dtype, name):
    if not isinstance(t, torch.Tensor):
        t = t.data                                                       # an SE3 object: its tensor
    L.require_gpu(t)
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"frames.{what}: {name} must be a contiguous {dtype} tensor (it is used in place), got {t.dtype}, strides {t.stride()}")
    return t


def _same_device(what, first, *rest):
    for t in rest:
        if t is not None and t.device != first.device:
            raise RuntimeError(f"frames.{what}: the frame buffers live on {first.device}, got a tensor on {t.device}")


def begin_frame(poses, patches, intrinsics, tstamps, n, new_patches, new_intrinsics, counter, res, motion_model="DAMPED_LINEAR", damping=0.5, depth="median"):
    """Row n of the four frame buffers in one launch (devo.py:487-488, :502-520); no other row is written.
    poses[n]: n > 1 — Exp(damping Log(P[n-1] P[n-2]^-1)) P[n-1] under "DAMPED_LINEAR", a bit-exact copy of row n - 1 under any other model;
    n <= 1 — untouched.  patches[n]: channels 0, 1 of new_patches [1, M, 3, P, P]; channel 2 = depth[m] over patch m for a tensor `depth` [M]
    (the caller's torch.rand before initialisation), or for depth="median" the lower median of patches[n-3:n, :, 2] — exactly what
    torch.median returns (n >= 3, 3 M P P <= MEDIAN_MAX; beyond it the call raises and launches nothing).  intrinsics[n] = new_intrinsics / res
    (a true fp32 division), tstamps[n] = counter."""
    poses, patches, intrinsics = (_state("begin_frame", t, torch.float32, s) for t, s in ((poses, "poses"), (patches, "patches"), (intrinsics, "intrinsics")))
    tstamps = _state("begin_frame", tstamps, torch.int64, "tstamps")
    L.require_gpu(new_patches, new_intrinsics)
    _same_device("begin_frame", poses, patches, intrinsics, tstamps, new_patches, new_intrinsics)
    n = int(n)
    P = patches.shape[-1]
    N = poses.numel() // 7
    if new_patches.dim() < 3 or tuple(new_patches.shape[-3:]) != (3, P, P):
        raise ValueError(f"frames.begin_frame: new_patches must be [1, M, 3, {P}, {P}], got {tuple(new_patches.shape)}")
    M = new_patches.numel() // (3 * P * P)
    if M <= 0 or patches.numel() != N * M * 3 * P * P or intrinsics.numel() != N * 4 or tstamps.numel() != N or patches.shape[-2] != P:
        raise ValueError(f"frames.begin_frame: the buffers disagree: poses {tuple(poses.shape)}, patches {tuple(patches.shape)}, intrinsics "
                         f"{tuple(intrinsics.shape)}, tstamps {tuple(tstamps.shape)} for M = {M}")
    if not 0 <= n < N:
        raise ValueError(f"frames.begin_frame: row n = {n} lies outside the {N} rows of the buffers")
    if new_intrinsics.numel() != 4:
        raise ValueError("frames.begin_frame: new_intrinsics must be [4]")
    f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
    new_patches, new_intrinsics = f32(new_patches), f32(new_intrinsics)
    if isinstance(depth, str):
        if depth != "median":
            raise ValueError(f"frames.begin_frame: depth is \"median\" or a tensor [M], got {depth!r}")
        if n < 3:
            raise ValueError(f"frames.begin_frame: the median depth is taken over the last three frames, n = {n}")
        depth = None
    else:
        L.require_gpu(depth)
        _same_device("begin_frame", poses, depth)
        if depth.numel() != M:
            raise ValueError(f"frames.begin_frame: depth must hold one value per patch ({M}), got {tuple(depth.shape)}")
        depth = f32(depth)
    model = _MODELS.get(motion_model, 0)
    nat = backends.native()
    with torch.cuda.device(poses.device):
        if nat is not None:
            nat.frames.begin_frame(poses, patches, intrinsics, tstamps, M, n, new_patches, new_intrinsics, int(counter), float(res), model, float(damping), depth)
        else:
            rc = L.lib().devo_frame_begin(L.ptr(poses), L.ptr(patches), L.ptr(intrinsics), L.ptr(tstamps), N, M, P, n, L.ptr(new_patches), L.ptr(new_intrinsics),
                                          int(counter), float(res), model, float(damping), L.ptr(depth), L.stream())
            L.check(rc, "frames.begin_frame")
    for t in (poses,) if n > 1 else ():
        _bump(t)
    for t in (patches, intrinsics, tstamps):
        _bump(t)


def point_cloud(poses, patches, intrinsics, ix, m, out, start_frame=0):
    """devo.py:342-344 for the patches k in [start_frame * M, m), one launch: out[k] = (X[:3] / X[3]) of X = G[ix[k]]^-1 ((x - cx) / fx,
    (y - cy) / fy, 1, d) at the centre pixel of patch k, with the intrinsics of frame ix[k].  out: fp32 [>= m, 3], the other rows are not
    touched.  start_frame = 0 is the reference's call; a caller that knows the frames below n - REMOVAL_WINDOW no longer change passes
    that frame.  (projective_ops.point_cloud, the P x P autograd form of the training losses, is another function.)"""
    poses, patches, intrinsics = (_state("point_cloud", t, torch.float32, s) for t, s in ((poses, "poses"), (patches, "patches"), (intrinsics, "intrinsics")))
    ix = _state("point_cloud", ix, torch.int64, "ix")
    out = _state("point_cloud", out, torch.float32, "out")
    _same_device("point_cloud", poses, patches, intrinsics, ix, out)
    m, start_frame = int(m), int(start_frame)
    if patches.dim() < 4:
        raise ValueError(f"frames.point_cloud: patches must be [N, M, 3, P, P] or [1, N M, 3, P, P], got {tuple(patches.shape)}")
    P = patches.shape[-1]
    n_poses, n_patches = poses.numel() // 7, patches.numel() // (3 * P * P)
    if n_poses <= 0 or n_patches % n_poses or intrinsics.numel() != n_poses * 4:
        raise ValueError("frames.point_cloud: poses, patches and intrinsics disagree in their number of frames")
    M = n_patches // n_poses
    if not 0 <= m <= min(n_patches, ix.numel()) or start_frame < 0:
        raise ValueError(f"frames.point_cloud: m = {m} exceeds the {n_patches} patches or the {ix.numel()} entries of ix")
    if out.dim() != 2 or out.shape[1] != 3 or out.shape[0] < m:
        raise ValueError(f"frames.point_cloud: out must be [>= {m}, 3], got {tuple(out.shape)}")
    if start_frame * M >= m:
        return
    nat = backends.native()
    with torch.cuda.device(poses.device):
        if nat is not None:
            nat.frames.point_cloud(poses, patches, intrinsics, ix, M, m, start_frame, out)
        else:
            rc = L.lib().devo_frame_point_cloud(L.ptr(poses), L.ptr(patches), L.ptr(intrinsics), L.ptr(ix), n_poses, n_patches, ix.numel(), P, M, m, start_frame, L.ptr(out),
                                                L.stream())
            L.check(rc, "frames.point_cloud")
    _bump(out)


_NORMS = {"none": 0, "rescale": 1, "norm": 1, "standard": 2, "std": 2}      # DEVO_INPUT_*; the names of devo.py:420-438
CROP_WIDTH = 346              # DEVO_INPUT_CROP_WIDTH (devo.py:466-467)
PROBE_MEDIAN_MAX = 1024       # DEVO_PROBE_MEDIAN_MAX


def pinned_record():
    """A record for frame_input: 4 pinned doubles the kernels write through their host address."""
    return torch.zeros(4, dtype=torch.float64).pin_memory()


def _host_visible(what, t, dtype, n, name):
    if not isinstance(t, torch.Tensor) or not (t.is_cuda or t.is_pinned()) or t.dtype != dtype or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"frames.{what}: {name} must be a contiguous {dtype} tensor of at least {n} elements on the GPU or in pinned host memory")


def frame_input(voxel, norm="std", gate=False, out=None, record=None):
    """devo.py:406-467 for one voxel grid [bins, H, W] (fp32 or fp16) -> (out fp32 [1, 1, bins, H, W'], record): the normalisation `norm`
    ("none"; "rescale" / "norm": positives divided by the largest positive, negatives by minus the smallest negative, true fp32 divisions,
    an absent polarity changes nothing; "std" / "standard": (x - mean) / sigma on the non-zero voxels, 0 elsewhere, mean and sigma exact to
    fp64 and rounded once; a grid without a non-zero voxel is returned as it is) and the crop W' = W - 2 of a 346-column grid (columns
    1 .. 344; the statistics include the two dropped columns, as the reference normalises first).  Two launches, no wait.
    record: 4 pinned doubles {nnz = #(x != 0), numel, c0, c1} ((mean, sigma) under std, (largest positive, largest -negative) under
    rescale), written behind the second launch: a caller that wants them records an event on the stream and waits for it — with
    gate=True (the tracker's n == 0) it does, for the reference's test `nnz / numel < 2e-2` (devo.py:413); `gate` itself changes nothing
    in what is launched.  Where all non-zero voxels are equal (sigma = 0) the result is events.std's for that grid.
    The reference's "empty voxel" return (devo.py:432-435) cannot be reached — a maximum over positives and a minimum over negatives
    are never 0, and a missing polarity is replaced by 1 — and is not built."""
    L.require_gpu(voxel)
    code = _NORMS.get(str(norm).lower())
    if code is None:
        raise NotImplementedError(f"frames.frame_input: norm {norm!r} is not implemented: one of {sorted(_NORMS)}")
    if voxel.dim() != 3 or voxel.dtype not in (torch.float32, torch.float16) or voxel.numel() == 0:
        raise ValueError(f"frames.frame_input: the voxel grid must be a non-empty fp32 or fp16 [bins, H, W] tensor, got {voxel.dtype} {tuple(voxel.shape)}")
    voxel = voxel.contiguous()
    bins, H, W = voxel.shape
    Wout = W - 2 if W == CROP_WIDTH else W
    if out is None:
        out = torch.empty(1, 1, bins, H, Wout, dtype=torch.float32, device=voxel.device)
    else:
        L.require_gpu(out)
        _same_device("frame_input", voxel, out)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != bins * H * Wout:
            raise ValueError(f"frames.frame_input: out must be a contiguous float32 tensor of {bins} x {H} x {Wout} elements")
    if record is None:
        record = pinned_record()
    _host_visible("frame_input", record, torch.float64, 4, "record")
    nat = backends.native()
    with torch.cuda.device(voxel.device):
        ws = torch.empty(L.lib().devo_odom_input_workspace_bytes(voxel.numel()), dtype=torch.uint8, device=voxel.device)
        if nat is not None:
            nat.frames.frame_input(voxel, code, out, ws, record)
        else:
            rc = L.lib().devo_odom_input(L.ptr(voxel), L.dtype_code(voxel), bins, H, W, code, L.ptr(out), L.ptr(ws), ws.numel(), L.ptr(record), L.stream())
            L.check(rc, "frames.frame_input")
    _bump(out)
    return out.view(1, 1, bins, H, Wout), record


def probe_median(delta, out=None):
    """torch.quantile(delta.norm(dim=-1).float(), 0.5) of the motion probe (devo.py:256) for delta [1, M, 2], fp32 or fp16, one launch of
    one workgroup -> fp32 [1] (`out`: a GPU tensor, or a pinned host tensor for a caller that reads it behind an event).  The norms are
    formed in fp64 from the exactly converted input and rounded to fp32, the selection is exact, and for even M the mean of the two
    middle values is formed in fp64 and rounded once."""
    L.require_gpu(delta)
    if delta.dtype not in (torch.float32, torch.float16) or delta.numel() == 0 or delta.shape[-1] != 2:
        raise ValueError(f"frames.probe_median: delta must be a non-empty fp32 or fp16 [1, M, 2] tensor, got {delta.dtype} {tuple(delta.shape)}")
    delta = delta.contiguous()
    M = delta.numel() // 2
    if M > PROBE_MEDIAN_MAX:
        raise RuntimeError(f"frames.probe_median: the median over {M} values exceeds the supported {PROBE_MEDIAN_MAX}")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=delta.device)
    _host_visible("probe_median", out, torch.float32, 1, "out")
    nat = backends.native()
    with torch.cuda.device(delta.device):
        if nat is not None:
            nat.frames.probe_median(delta, out)
        else:
            L.check(L.lib().devo_odom_probe_median(L.ptr(delta), L.dtype_code(delta), M, L.ptr(out), L.stream()), "frames.probe_median")
    return out


class Trajectory:
    """The `delta` dict of the reference (devo.py:280, :534) and its terminate() (:179-196), resident on the device: parent int64
    [capacity] (-1: no entry), rel fp32 [capacity, 7]; frame t's pose is rel[t] pose(parent[t]) unless t is a keyframe.  `capacity` is at
    least the largest `counter`.  One stream per trajectory."""

    def __init__(self, capacity, device="cuda"):
        if int(capacity) <= 0:
            raise ValueError("Trajectory: capacity must be positive")
        self.capacity = int(capacity)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
        self.parent = torch.full((self.capacity,), -1, dtype=torch.int64, device=self.device)
        self.rel = torch.zeros(self.capacity, 7, dtype=torch.float32, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32).pin_memory()      # written by the kernels, read behind complete()'s last one
        self._event = None

    def record_removed(self, poses, tstamps, k):
        """devo.py:276-280, to be called BEFORE shift_frames: parent[tstamps[k]] = tstamps[k - 1], rel[tstamps[k]] = P[k] P[k-1]^-1, the
        timestamps read on the device.  One launch, no wait."""
        poses = _state("Trajectory.record_removed", poses, torch.float32, "poses")
        tstamps = _state("Trajectory.record_removed", tstamps, torch.int64, "tstamps")
        _same_device("Trajectory.record_removed", self.parent, poses, tstamps)
        k, rows = int(k), min(poses.numel() // 7, tstamps.numel())
        if not 1 <= k < rows:
            raise ValueError(f"Trajectory.record_removed: frame k = {k} needs a frame in front of it inside the {rows} rows of the buffers")
        nat = backends.native()
        with torch.cuda.device(self.device):
            if nat is not None:
                nat.frames.record_removed(poses, tstamps, k, self.parent, self.rel, self._status)
            else:
                rc = L.lib().devo_frame_record_removed(L.ptr(poses), L.ptr(tstamps), rows, k, L.ptr(self.parent), L.ptr(self.rel), self.capacity, L.ptr(self._status),
                                                       L.stream())
                L.check(rc, "Trajectory.record_removed")

    def record_skipped(self, t, t0):
        """devo.py:534 (the motion probe rejected frame t): parent[t] = t0, rel[t] = identity.  One launch, no wait."""
        t, t0 = int(t), int(t0)
        if not 0 <= t < self.capacity:
            raise RuntimeError(f"Trajectory.record_skipped: frame {t} lies outside the capacity {self.capacity}")
        if not 0 <= t0 < t:
            raise ValueError(f"Trajectory.record_skipped: the parent {t0} of frame {t} must be an earlier frame")
        nat = backends.native()
        with torch.cuda.device(self.device):
            if nat is not None:
                nat.frames.record_skipped(t, t0, self.parent, self.rel, self._status)
            else:
                rc = L.lib().devo_frame_record_skipped(t, t0, L.ptr(self.parent), L.ptr(self.rel), self.capacity, L.ptr(self._status), L.stream())
                L.check(rc, "Trajectory.record_skipped")

    @staticmethod
    def launches(counter):
        """Kernel launches of complete(): 1 + ceil(log2(counter))."""
        return int(L.lib().devo_frame_complete_launches(int(counter)))

    def complete(self, poses, tstamps, n, counter):
        """terminate() (devo.py:186-196) -> fp32 [counter, 7] on the device, the INVERSE of every frame's pose: pose(tstamps[i]) = poses[i]
        for the keyframes i < n (they win over a log entry), pose(t) = rel[t] pose(parent[t]) for every other t < counter.  Parallel
        pointer jumping: 1 + ceil(log2(counter)) launches whatever the depth of the chains; one wait behind the last, for the status
        word: a frame that is neither a keyframe nor tied to one raises."""
        poses = _state("Trajectory.complete", poses, torch.float32, "poses")
        tstamps = _state("Trajectory.complete", tstamps, torch.int64, "tstamps")
        _same_device("Trajectory.complete", self.parent, poses, tstamps)
        n, counter = int(n), int(counter)
        if not 0 <= n <= min(poses.numel() // 7, tstamps.numel()):
            raise ValueError(f"Trajectory.complete: n = {n} exceeds the frame buffers")
        if not 0 <= counter <= self.capacity:
            raise RuntimeError(f"Trajectory.complete: counter = {counter} exceeds the capacity {self.capacity}")
        out = torch.empty(counter, 7, dtype=torch.float32, device=self.device)
        if counter == 0:
            return out
        nat = backends.native()
        with torch.cuda.device(self.device):
            ws = torch.empty(L.lib().devo_frame_complete_workspace_bytes(counter), dtype=torch.uint8, device=self.device)
            if self._event is None:
                self._event = torch.cuda.Event()
            if nat is not None:
                nat.frames.complete(poses, tstamps, n, counter, self.parent, self.rel, out, ws, self._status)
            else:
                rc = L.lib().devo_frame_complete(L.ptr(poses), L.ptr(tstamps), n, counter, L.ptr(self.parent), L.ptr(self.rel), self.capacity, L.ptr(out), L.ptr(ws),
                                                 ws.numel(), L.ptr(self._status), L.stream())
                L.check(rc, "Trajectory.complete")
            self._event.record()
            self._event.synchronize()
        code = self._status.tolist()[0]
        if code:
            self._status.zero_()
            raise RuntimeError(f"Trajectory.complete: {_STATUS.get(code, 'unknown status')} (status {code})")
        return out
