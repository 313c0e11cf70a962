"""The online tracker: devo/devo.py's `DEVO` class over this package's GPU modules — hand it voxel grids, get a trajectory back.

    slam = odometry.DEVO(odometry.Config(), network, ht=480, wd=640)
    for voxel, intrinsics, tstamp in frames:
        slam(tstamp, voxel, intrinsics)
    poses, tstamps = slam.terminate()                       # or: poses, tstamps = slam.run(frames)

What the class owns is the ORDER of the calls (devo.py:382-555); every step is a module of this package: the input gate, normalisation and
crop (frames.frame_input), the Patchifier, the frame store (frames.begin_frame), the feature rings (altcorr.build_pyramid(..., slot=) and
indexed assignment, whose write records backends/ring.py keeps), the motion probe's median (frames.probe_median), the window edges
(PatchGraph.append_frame), reprojection, the fused lookup, the Update operator, fastba.BA, the point cloud, the keyframe test with its
removals (PatchGraph.keyframe, Trajectory.record_removed, graph.shift_frames) and terminate() (Trajectory.complete).  Event input only:
the reference's RGB branch needs a `net.py` it does not ship.  No CPU fallback.

Host waits of a frame (counted from the code below; DESIGN.md 3.19 has the launches): in the steady state — NORM "std", "rescale" or
"none", initialised — ONE, PatchGraph.keyframe's, for the edge count the next frame's allocations need.  The input gate waits only while
n == 0 (devo.py:406-415), the motion probe only until initialisation (:531-535); both read this tracker's own pinned record behind this
tracker's own event — not a slot of a ring shared with other readers, whose reuse could hand a value to the wrong owner.  A failed
adjustment is reported like the reference's (devo.py:336-340): a warning, and the state stays as the BA left it; fastba.BA raises it
without a wait, at a later call.

One deviation from the reference's text: update() runs the lookup and the operator under `torch.autocast(enabled=cfg.MIXED_PRECISION)`
where devo.py:311 hard-codes `enabled=True` — with MIXED_PRECISION off the rings and the recurrent state are fp32 and so is the step."""
import warnings
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import altcorr, fastba, frames
from . import projective_ops as pops
from .backends import ring
from .graph import PatchGraph, shift_frames
from .lietorch import SE3

RES = 4                       # the encoders' stride (eVONet.RES)
GATE_DENSITY = 2e-2           # devo.py:413


class Config:
    """The fields and defaults of devo/config.py as a plain class (any object with these attributes is accepted by DEVO)."""
    BUFFER_SIZE = 2048 * 2
    PATCH_SELECTOR = "scorer"
    SCORER_EVAL_MODE = "multi"
    SCORER_EVAL_USE_GRID = True
    NORM = "std"
    PATCHES_PER_FRAME = 80
    REMOVAL_WINDOW = 20
    OPTIMIZATION_WINDOW = 12
    PATCH_LIFETIME = 12
    KEYFRAME_INDEX = 4
    KEYFRAME_THRESH = 12.5
    MOTION_MODEL = "DAMPED_LINEAR"
    MOTION_DAMPING = 0.5
    MIXED_PRECISION = True

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise AttributeError(f"Config: unknown field {k!r}")
            setattr(self, k, v)


class DEVO:
    """devo.py:21-555.  `network`: a module with `patchify` (patchifier.Patchifier), `update` (update.Update) and `P` — training.TrainNet
    qualifies.  `mem`: frames the feature rings hold (devo.py:69); it must exceed REMOVAL_WINDOW + 1, the oldest frame an edge can name.
    One stream per tracker.  Constructing one switches on backends/ring.py's process-wide record of indexed writes
    (`ring.track_ring_writes(True)`, what `backends.install()` does too; idempotent, left on): the fp32 rings need it."""

    def __init__(self, cfg, network, ht=480, wd=640, mem=32):
        self.cfg = cfg
        self.network = network
        self.P = int(network.P)
        self.RES = RES
        self.dim_inet = int(getattr(network, "dim_inet", None) or network.patchify.dim_inet)
        self.dim_fnet = int(getattr(network, "dim_fnet", None) or network.patchify.dim_fnet)
        self.M, self.N, self.mem = int(cfg.PATCHES_PER_FRAME), int(cfg.BUFFER_SIZE), int(mem)
        if self.mem <= int(cfg.REMOVAL_WINDOW) + 1:
            raise ValueError(f"odometry.DEVO: mem = {self.mem} must exceed REMOVAL_WINDOW + 1 = {int(cfg.REMOVAL_WINDOW) + 1}: a live edge would name an overwritten ring slot")
        if str(cfg.NORM).lower() not in frames._NORMS:
            raise NotImplementedError(f"{cfg.NORM} not implemented")
        if not torch.cuda.is_available():
            raise RuntimeError("devo_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
        self.device = dev = torch.device("cuda", torch.cuda.current_device())
        self.network.to(dev).eval()
        ring.track_ring_writes(True)
        self.ht, self.wd = int(ht), int(wd)
        self.is_initialized = False
        self.n = self.m = self.counter = 0
        self.tlist = []
        M, N, P = self.M, self.N, self.P
        # devo.py:56-66
        self.tstamps_ = torch.zeros(N, dtype=torch.long, device=dev)
        self.poses_ = torch.zeros(N, 7, dtype=torch.float, device=dev)
        self.patches_ = torch.zeros(N, M, 3, P, P, dtype=torch.float, device=dev)
        self.patches_gt_ = torch.zeros(N, M, 3, P, P, dtype=torch.float, device=dev)
        self.intrinsics_ = torch.zeros(N, 4, dtype=torch.float, device=dev)
        self.points_ = torch.zeros(N * M, 3, dtype=torch.float, device=dev)
        self.colors_ = torch.zeros(N, M, 3, dtype=torch.uint8, device=dev)
        self.index_ = torch.zeros(N, M, dtype=torch.long, device=dev)
        self.index_map_ = torch.zeros(N, dtype=torch.long, device=dev)
        self.poses_[:, 6] = 1.0
        # devo.py:71-83.  fp16 rings are kept channel-blocked, the layout the lookup reads as it is (altcorr.build_pyramid writes a slot of
        # both levels in one launch); fp32 rings stay NCHW: the lookup keeps a split copy of them per version, maintained slot by slot from
        # the records of the indexed writes below
        self.dtype = dt = torch.half if cfg.MIXED_PRECISION else torch.float
        self.imap_ = torch.zeros(self.mem, M, self.dim_inet, dtype=dt, device=dev)
        self.gmap_ = torch.zeros(self.mem, M, self.dim_fnet, P, P, dtype=dt, device=dev)
        h, w = self.ht // RES, (self.wd - 2 if self.wd == frames.CROP_WIDTH else self.wd) // RES
        C = self.dim_fnet
        self.blocked = bool(cfg.MIXED_PRECISION)
        if self.blocked:
            self.fmap1_ = torch.zeros(1, self.mem, C // 8, h, w, 8, dtype=dt, device=dev)
            self.fmap2_ = torch.zeros(1, self.mem, C // 8, h // 4, w // 4, 8, dtype=dt, device=dev)
        else:
            self.fmap1_ = torch.zeros(1, self.mem, C, h, w, dtype=dt, device=dev)
            self.fmap2_ = torch.zeros(1, self.mem, C, h // 4, w // 4, dtype=dt, device=dev)
        self.pyramid = (self.fmap1_, self.fmap2_)
        self.graph = PatchGraph(M, self.dim_inet, device=dev, dtype=dt)
        self.trajectory = frames.Trajectory(N, dev)
        self.lmbda = torch.as_tensor([1e-4], device=dev)
        # what the host reads of a frame: {nnz, numel, c0, c1} of frame_input and the probe's median, this tracker's own
        self._record = torch.zeros(5, dtype=torch.float64).pin_memory()
        self._record_input = self._record[:4]
        self._record_probe = self._record[4:].view(torch.float32)
        self._event = torch.cuda.Event()
        self.skipped = []                  # the stamps of the calls that returned early (gate, probe)

    # ------------------------------------------------------------------------------------------ devo.py:151-177
    poses = property(lambda self: self.poses_.view(1, self.N, 7))
    patches = property(lambda self: self.patches_.view(1, self.N * self.M, 3, self.P, self.P))
    intrinsics = property(lambda self: self.intrinsics_.view(1, self.N, 4))
    ix = property(lambda self: self.index_.view(-1))
    imap = property(lambda self: self.imap_.view(1, self.mem * self.M, self.dim_inet))
    gmap = property(lambda self: self.gmap_.view(1, self.mem * self.M, self.dim_fnet, self.P, self.P))
    ii = property(lambda self: self.graph.ii)
    jj = property(lambda self: self.graph.jj)
    kk = property(lambda self: self.graph.kk)
    net = property(lambda self: self.graph.net)

    def _read(self):
        """The tracker's wait: for the record behind the kernels enqueued so far, not for the stream's later work."""
        self._event.record()
        self._event.synchronize()

    def _grow_log(self):
        """`counter` counts every frame, kept or not: the relative-pose log (the reference's unbounded dict) doubles when it is full."""
        old = self.trajectory
        self.trajectory = frames.Trajectory(2 * old.capacity, self.device)
        self.trajectory.parent[:old.capacity] = old.parent
        self.trajectory.rel[:old.capacity] = old.rel

    def _autocast(self):
        return torch.autocast("cuda", enabled=bool(self.cfg.MIXED_PRECISION), dtype=torch.float16)

    def _step(self, ii, jj, kk, net):
        """reproject + corr + the operator (devo.py:309-317, :248-254) -> coords [1, E, 2, P, P], net, delta, weight."""
        coords = pops.transform(SE3(self.poses), self.patches, self.intrinsics, ii, jj, kk).permute(0, 1, 4, 2, 3).contiguous()
        with self._autocast():
            kk1 = kk % (self.M * self.mem)
            corr = altcorr.corr_pyramid(self.gmap, self.pyramid, coords, kk1, jj % self.mem, 3)
            ctx = self.imap[:, kk1]
            net, (delta, weight, _) = self.network.update(net, ctx, corr, None, ii, jj, kk)
        return coords, net, delta, weight

    # ------------------------------------------------------------------------------------------ devo.py:241-256
    def motion_probe(self):
        """The median flow the operator predicts from the last frame's patches into the new frame, as a Python float (one wait)."""
        kk = torch.arange(self.m - self.M, self.m, device=self.device)
        jj = self.n * torch.ones_like(kk)
        ii = self.ix[kk]
        net = torch.zeros(1, self.M, self.dim_inet, dtype=self.dtype, device=self.device)
        _, _, delta, _ = self._step(ii, jj, kk, net)
        frames.probe_median(delta, out=self._record_probe)
        self._read()
        return float(self._record_probe[0])

    # ------------------------------------------------------------------------------------------ devo.py:308-344
    def update(self):
        g = self.graph
        coords, g.net, delta, weight = self._step(g.ii, g.jj, g.kk, g.net)
        target = coords[..., self.P // 2, self.P // 2] + delta.float()
        t0 = max(self.n - int(self.cfg.OPTIMIZATION_WINDOW), 1) if self.is_initialized else 1
        try:
            fastba.BA(self.poses, self.patches, self.intrinsics, target, weight.float(), self.lmbda, g.ii, g.jj, g.kk, t0, self.n, 2)
        except fastba.BAFailure as e:
            warnings.warn(f"Warning BA failed... ({e})")
        frames.point_cloud(self.poses_, self.patches_, self.intrinsics_, self.ix, self.m, self.points_)

    # ------------------------------------------------------------------------------------------ devo.py:267-306
    def keyframe(self):
        cfg = self.cfg
        r = self.graph.keyframe(self.poses_, self.patches_, self.intrinsics_, self.ix, self.n, keyframe_index=cfg.KEYFRAME_INDEX, thresh=cfg.KEYFRAME_THRESH,
                                removal_window=cfg.REMOVAL_WINDOW)
        if r.removed:
            k, mem = r.k, self.mem
            self.trajectory.record_removed(self.poses_, self.tstamps_, k)               # reads tstamps_ / poses_ BEFORE the shift
            shift_frames([self.tstamps_, self.colors_, self.poses_, self.patches_, self.patches_gt_, self.intrinsics_], k, self.n)
            for i in range(k, self.n - 1):                                              # devo.py:297-300: ring.py keeps the records of these writes
                self.imap_[i % mem] = self.imap_[(i + 1) % mem]
                self.gmap_[i % mem] = self.gmap_[(i + 1) % mem]
                self.fmap1_[0, i % mem] = self.fmap1_[0, (i + 1) % mem]
                self.fmap2_[0, i % mem] = self.fmap2_[0, (i + 1) % mem]
            self.n -= 1
            self.m -= self.M
        return r

    # ------------------------------------------------------------------------------------------ devo.py:382-555
    @torch.no_grad()
    def __call__(self, tstamp, voxel, intrinsics, scale=1.0):
        """Track a new voxel grid [bins, H, W] with intrinsics [4] (fx, fy, cx, cy at full resolution).  Returns None."""
        cfg, M = self.cfg, self.M
        if (self.n + 1) >= self.N:
            raise Exception(f'The buffer size is too small. You can increase it using "--buffer {self.N * 2}"')
        L.require_gpu(voxel, intrinsics)
        with torch.cuda.device(self.device):
            gate = self.n == 0
            image, _ = frames.frame_input(voxel, cfg.NORM, gate=gate, record=self._record_input)      # normalised and cropped (:406-467)
            if gate:
                self._read()
                nnz, numel = int(self._record_input[0]), int(self._record_input[1])
                if nnz / numel < GATE_DENSITY:
                    print(f"skip voxel at {tstamp} due to lack of events!")
                    self.skipped.append(tstamp)
                    return
            with self._autocast():
                fmap, gmap, imap, patches, _, clr = self.network.patchify(image, patches_per_image=M, return_color=True, scorer_eval_mode=cfg.SCORER_EVAL_MODE,
                                                                          scorer_eval_use_grid=cfg.SCORER_EVAL_USE_GRID)
            n = self.n
            self.patches_gt_[n] = patches[0]
            self.tlist.append(tstamp)
            self.colors_[n] = ((clr[0].float() + 0.5) * (255.0 / 2)).to(torch.uint8)                   # :495-496, the three channels alike
            self.index_[n + 1] = n + 1
            self.index_map_[n + 1] = self.m + M
            depth = "median" if self.is_initialized else torch.rand(M, device=self.device)              # :515-518
            frames.begin_frame(self.poses_, self.patches_, self.intrinsics_, self.tstamps_, n, patches, intrinsics, self.counter, self.RES,
                               motion_model=cfg.MOTION_MODEL, damping=cfg.MOTION_DAMPING, depth=depth)
            slot = n % self.mem                                                                         # :523-527
            self.imap_[slot] = imap.view(M, self.dim_inet)
            self.gmap_[slot] = gmap.view(M, self.dim_fnet, self.P, self.P)
            if self.blocked:
                altcorr.build_pyramid(fmap.to(self.dtype), out=self.pyramid, slot=slot)
            else:
                self.fmap1_[:, slot] = fmap[0]
                self.fmap2_[:, slot] = F.avg_pool2d(fmap[0].float(), 4, 4)
            self.counter += 1
            if self.counter > self.trajectory.capacity:
                self._grow_log()
            if self.n > 0 and not self.is_initialized:
                thres = 2.0 if scale == 1.0 else scale ** 2
                if self.motion_probe() < thres:
                    self.trajectory.record_skipped(self.counter - 1, self.counter - 2)
                    self.skipped.append(tstamp)
                    return
            self.n += 1
            self.m += M
            self.graph.append_frame(self.n, cfg.PATCH_LIFETIME, self.ix)                              # :541-542
            if self.n == 8 and not self.is_initialized:
                self.is_initialized = True
                for _ in range(12):
                    self.update()
            elif self.is_initialized:
                self.update()
                self.keyframe()

    # ------------------------------------------------------------------------------------------ devo.py:186-208
    def terminate(self):
        """-> (poses [counter, 7] numpy, the inverse of every frame's pose as devo.py:196; tstamps float64 [counter])."""
        if self.is_initialized:
            poses = self.trajectory.complete(self.poses_, self.tstamps_, self.n, self.counter).cpu().numpy()
        else:
            print("Warning: Model is not initialized. Using Identity.")
            poses = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] for _ in range(self.counter)]).reshape(self.counter, 7)
            poses[:, :3] = poses[:, :3] + np.random.randn(self.counter, 3) * 0.01
        return poses, np.array(self.tlist, dtype=np.float64)

    def run(self, sequence, scale=1.0, final_updates=12):
        """utils/eval_utils.py:110-139 without the plots: `sequence` yields (voxel, intrinsics, tstamp); every frame is tracked, the 12
        closing update() calls of :127-128 follow (once initialised: before that there is nothing to adjust) -> terminate()'s
        (poses, tstamps), which evaluation.ate_real takes as they are."""
        for voxel, intrinsics, tstamp in sequence:
            self(tstamp, voxel, intrinsics, scale=scale)
        if self.is_initialized:
            with torch.no_grad():
                for _ in range(int(final_updates)):
                    self.update()
        return self.terminate()
