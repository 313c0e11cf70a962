"""devo_amd — MI355X-native (gfx950) implementation of DEVO's recurrent update + bundle-adjustment hot path:
altcorr (patch correlation lookup), fastba (sparse Gauss-Newton BA) and the lietorch SE3 ops, as hand-written
HIP kernels behind a C ABI (include/devo_hip.h, devo_amd/lib/libdevo_hip.so) and the reference's own Python
extension-module interfaces (devo_amd.backends.{cuda_corr, cuda_ba, lietorch_backends}).

The training input path sits beside it: `data` (the sample's tail) and `frame_graph` (a scene's frame graph and the clip sampler
that walks it).

`select` is the per-frame patch selection (the reference's PatchSelector and the Patchifier's tail behind it) as one launch.

`evaluation` scores a finished trajectory: association with the ground truth, Sim(3) alignment and the ATE of a batch of pairs in one launch.

`camera` turns a lens calibration into the tensors the rest takes: the rectification map of `events.voxel_grids`, undistorted points and
undistorted frames (pinhole, radtan and equidistant models; what the reference obtains from OpenCV).

`simulate` makes the training data's events: contrast-threshold events from log-intensity frames (`ESIM`, the reference's esim_torch.ESIM),
`log_intensity` in front of it and `frames_to_voxels` behind it (the loop of the reference's scripts/convert_tartan.py).

`optim` is the tail of a training step: gradient-norm clip + AdamW in two launches (`AdamW`, a torch.optim.Optimizer that torch's own
OneCycleLR drives and whose checkpoints are torch.optim.AdamW's).

Importing this package does not load the HIP library; the first call into a backend does, and fails loudly
if it is missing.  There is no CPU fallback anywhere in the package.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name in ("camera", "simulate", "optim"):            # devo_amd.camera / .simulate / .optim without an import of their own; loaded on first use
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
