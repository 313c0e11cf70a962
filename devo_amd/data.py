"""The tail of a training sample on the GPU, mirroring devo/data_readers: utils/transform_utils.py:9-28 `transform_rescale`,
devo/data_readers/augmentation.py:79-174 `voxel_color_jitter` and `EVSDAugmentor`, and the depth normalisation of
devo/data_readers/base.py:366-369 (`normalise_depth`); `prepare_batch` is base.py:356-371 for a batch [B, n, ...] of samples.

The reference runs these steps per sample in its CPU DataLoader workers.  Here the workers only read and draw: `EVSDAugmentor.draw`
makes the reference's np.random draws (and one jitter seed from torch's default CPU generator), and `prepare_batch` applies them
after `.cuda()`: one resample launch per tensor and step for all B samples, one normalisation call, no host synchronisation.
Arithmetic is ATen's CPU arithmetic, so a given draw and given jitter noise reproduce the reference's sample.
Inputs are device tensors; no CPU fallback."""
import ctypes
import math
import numpy as np
import torch
from . import _lib as L

BILINEAR, NEAREST = 0, 1               # DEVO_RESAMPLE_BILINEAR / _NEAREST
JITTER_EPS = 1e-4                      # voxel_color_jitter's EPS, fixed in the kernel


def _resample(src, size, crops, mode, noise=None, seeds=None):
    """src [B, C, H, W] -> [B, C, Hc, Wc]: sample b resized to its own scaled size and cropped at its own offset.  crops: B tuples
    (Hs, Ws, y0, x0); size: (Hc, Wc).  noise (src's shape) or seeds (B ints) add the jitter to every source tap."""
    L.require_gpu(src, noise)
    if src.dim() != 4:
        raise ValueError(f"expected [B, C, H, W], got {tuple(src.shape)}")
    B, C, H, W = src.shape
    Hc, Wc = int(size[0]), int(size[1])
    if len(crops) != B:
        raise ValueError(f"{len(crops)} crop parameters for {B} samples")
    x = src.float().contiguous()
    nz = None
    if noise is not None:
        if tuple(noise.shape) != tuple(src.shape):
            raise ValueError(f"noise must have the source's shape {tuple(src.shape)}, got {tuple(noise.shape)}")
        nz = noise.float().contiguous()
    out = torch.empty(B, C, Hc, Wc, dtype=torch.float32, device=src.device)
    params = (ctypes.c_int * (4 * max(B, 1)))(*[int(v) for c in crops for v in c])
    sd = None if seeds is None else (ctypes.c_uint64 * max(B, 1))(*[int(s) & (2 ** 64 - 1) for s in seeds])
    rc = L.lib().devo_voxel_resample(L.ptr(x), L.ptr(out), B, C, H, W, Hc, Wc, params, int(mode), L.ptr(nz), sd, L.stream())
    L.check(rc, "data.resample")
    return out


def _draw_seed():
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def voxel_color_jitter(voxels, EPS=1e-4, noise=None, seed=None):
    """voxel_color_jitter (augmentation.py:79-89): voxels + (u - 0.5) * 2 * EPS, u uniform in [0, 1) per voxel.  u is `noise` (the
    shape of voxels; the reference's torch.rand_like draw, for parity) or hashed from `seed` (drawn from torch's default CPU
    generator when None).  Returns a new float32 tensor."""
    if EPS != JITTER_EPS:
        raise ValueError(f"the jitter amplitude is fixed at {JITTER_EPS}")
    L.require_gpu(voxels)
    shp = voxels.shape
    H, W = shp[-2], shp[-1]
    x = voxels.reshape(1, -1, H, W)
    if noise is not None:
        noise = noise.reshape(x.shape)
        seeds = None
    else:
        seeds = [_draw_seed() if seed is None else seed]
    return _resample(x, (H, W), [(H, W, 0, 0)], BILINEAR, noise=noise, seeds=seeds).view(shp)


def _rescale_sizes(scale, H, W):
    return math.floor(scale * H), math.floor(scale * W)


def transform_rescale(scale, voxels, disps=None, poses=None, intrinsics=None):
    """transform_rescale (utils/transform_utils.py:9-28) on [..., H, W] voxels and disparities: torchvision 0.13's Resize
    (bilinear, align_corners=False, no antialias) to floor(scale * H) x floor(scale * W); poses' translations and the intrinsics are
    multiplied by scale.  Returns (voxels, disps, poses, intrinsics), new tensors (None stays None)."""
    L.require_gpu(voxels, disps, poses, intrinsics)
    H, W = voxels.shape[-2:]
    nH, nW = _rescale_sizes(scale, H, W)
    if nH < 1 or nW < 1:
        raise ValueError(f"scale {scale} leaves an empty image")

    def resize(t):
        x = t.reshape(1, -1, H, W)
        return _resample(x, (nH, nW), [(nH, nW, 0, 0)], BILINEAR).view(*t.shape[:-2], nH, nW)

    voxels = resize(voxels)
    if disps is not None:
        disps = resize(disps)
    if poses is not None:
        poses = poses.clone()
        poses[..., :3] *= float(scale)                       # SE3.scale: t * torch.tensor(scale) (fp32)
    if intrinsics is not None:
        intrinsics = float(scale) * intrinsics
    return voxels, disps, poses, intrinsics


def normalise_depth(disps, poses=None, q=.98, factor=.7):
    """The depth normalisation of base.py:366-369 per sample: s = factor * torch.quantile(disps[b], q) (exactly, NaN in -> NaN
    out), disps[b] / s, poses[b][..., :3] * s.  disps [B, ...] with B samples (a single sample: add the batch dimension), poses
    [B, ..., 7] or None.  Works in place on float32 contiguous inputs (others are converted first) and returns (disps, poses, s[B])."""
    L.require_gpu(disps, poses)
    if disps.dim() < 1 or disps[0].numel() == 0:
        raise ValueError("normalise_depth needs a batch of non-empty disparity maps")
    if disps.dtype != torch.float32 or not disps.is_contiguous():
        disps = disps.float().contiguous()
    B = disps.shape[0]
    n = disps[0].numel()
    P = stride = 0
    if poses is not None:
        if poses.shape[0] != B or poses.shape[-1] < 3:
            raise ValueError(f"poses [B, ..., 7] for B = {B}, got {tuple(poses.shape)}")
        if poses.dtype != torch.float32 or not poses.is_contiguous():
            poses = poses.float().contiguous()
        stride = poses.shape[-1]
        P = poses.numel() // max(B * stride, 1)
    s = torch.empty(B, dtype=torch.float32, device=disps.device)
    lib = L.lib()
    ws = torch.empty(lib.devo_depth_normalise_workspace_bytes(B), dtype=torch.uint8, device=disps.device)
    rc = lib.devo_depth_normalise(L.ptr(disps), n, B, L.ptr(poses), P, stride, float(q), float(factor), L.ptr(s), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "data.normalise_depth")
    return disps, poses, s


class EVSDAugmentor:
    """EVSDAugmentor (augmentation.py:92-174) on device tensors: voxels [n, bins, H, W], poses [n, 7], depths (disparities, as
    base.py passes them) [n, H, W], intrinsics [n, 4].  draw() makes the host draws, apply() does the work on the GPU; __call__ is
    both.  Unlike the reference, a scaled image smaller than the crop raises ValueError (the reference returns a smaller tensor)."""

    def __init__(self, crop_size):
        self.crop_size = [int(crop_size[0]), int(crop_size[1])]
        self.max_scale = 0.25

    def draw(self, ht, wd, fix_scale=None):
        """voxel_spatial_transform's draws (augmentation.py:119-132) from np.random, in the reference's order, plus the jitter seed
        from torch's default CPU generator.  Returns {"scale": the zoom, "seed": the jitter seed}."""
        max_scale = self.max_scale
        if fix_scale is None:
            scale = 1
            min_scale = np.log2(np.maximum((self.crop_size[0] + 1) / float(ht), (self.crop_size[1] + 1) / float(wd)))
            if np.random.rand() < 0.8:
                scale = 2 ** np.random.uniform(min_scale, max_scale)
        else:
            scale = fix_scale
            min_scale = np.log2(fix_scale)
            if min_scale < max_scale:
                scale = 2 ** np.random.uniform(min_scale, max_scale)
        return {"scale": scale, "seed": _draw_seed()}

    def crop(self, ht, wd, params):
        """(Hs, Ws, y0, x0) of a draw for an ht x wd image: F.interpolate's output size int(size * scale), the centre crop offsets."""
        scale = params["scale"]
        Hs, Ws = int(ht * scale), int(wd * scale)
        if Hs < self.crop_size[0] or Ws < self.crop_size[1]:
            raise ValueError(f"the scaled image {Hs}x{Ws} (scale {scale}) is smaller than the crop {self.crop_size[0]}x{self.crop_size[1]}")
        return Hs, Ws, (Hs - self.crop_size[0]) // 2, (Ws - self.crop_size[1]) // 2

    def apply(self, voxels, poses, depths, intrinsics, params, noise=None):
        """voxel_color_jitter then voxel_spatial_transform with the draw `params`; noise: the jitter's uniforms (voxels' shape) in
        place of the seed.  Returns (voxels, poses, depths, intrinsics) as the reference does (poses unchanged)."""
        v, d, intr = _augment_batch(voxels[None], depths[None], intrinsics[None], self, [params], None if noise is None else noise[None])
        return v[0], poses, d[0], intr[0]

    def __call__(self, voxels, poses, depths, intrinsics):
        return self.apply(voxels, poses, depths, intrinsics, self.draw(*voxels.shape[-2:]))


def _augment_batch(voxels, disps, intrinsics, aug, params, noise):
    """[B, n, bins, H, W] voxels, [B, n, H, W] disparities, [B, n, 4] intrinsics -> jittered, zoomed and cropped, one launch each."""
    L.require_gpu(voxels, disps, intrinsics, noise)
    B, n, bins, H, W = voxels.shape
    crops = [aug.crop(H, W, p) for p in params]
    size = aug.crop_size
    vox = _resample(voxels.reshape(B, n * bins, H, W), size, crops, BILINEAR, noise=None if noise is None else noise.reshape(B, n * bins, H, W),
                    seeds=[p["seed"] for p in params]).view(B, n, bins, *size)
    d = _resample(disps.reshape(B, n, H, W), size, crops, NEAREST).view(B, n, *size)
    intr = torch.empty_like(intrinsics)
    for b, (p, c) in enumerate(zip(params, crops)):          # scale * intrinsics - [0, 0, x0, y0], as the reference forms it
        intr[b] = float(p["scale"]) * intrinsics[b]
        intr[b, ..., 2] -= c[3]
        intr[b, ..., 3] -= c[2]
    return vox, d, intr


def prepare_batch(voxels, poses, disps, intrinsics, crop_size, scale=1.0, aug=True, params=None, noise=None):
    """EVSDDataset.__getitem__'s tail (base.py:356-371) for B samples at once, after the dataset read them: voxels [B, n, bins, H, W],
    poses [B, n, 7], disps [B, n, H, W], intrinsics [B, n, 4], all on one GPU.  transform_rescale when scale != 1; with aug,
    EVSDAugmentor(crop_size) (crop_size scaled by `scale` as the dataset's constructor does) with the draws `params` (B dicts from
    EVSDAugmentor.draw; drawn here when None) and optional jitter `noise` [B, n, bins, H', W']; then normalise_depth.
    Returns (voxels, poses, disps, intrinsics), new tensors."""
    L.require_gpu(voxels, poses, disps, intrinsics, noise)
    if voxels.dim() != 5 or disps.dim() != 4 or poses.dim() != 3 or intrinsics.dim() != 3:
        raise ValueError("expected voxels [B, n, bins, H, W], poses [B, n, 7], disps [B, n, H, W], intrinsics [B, n, 4]")
    if scale != 1.0:
        voxels, disps, poses, intrinsics = transform_rescale(scale, voxels, disps, poses, intrinsics)
        crop_size = np.floor(scale * np.array(crop_size)).astype(int).tolist()
    else:
        poses = poses.float().contiguous().clone()
    if aug:
        a = EVSDAugmentor(crop_size)
        H, W = voxels.shape[-2:]
        if params is None:
            params = [a.draw(H, W) for _ in range(voxels.shape[0])]
        if len(params) != voxels.shape[0]:
            raise ValueError(f"{len(params)} draws for {voxels.shape[0]} samples")
        voxels, disps, intrinsics = _augment_batch(voxels, disps, intrinsics, a, params, noise)
    elif scale == 1.0:
        voxels, disps, intrinsics = voxels.float().clone(), disps.float().clone(), intrinsics.clone()
    disps, poses, _ = normalise_depth(disps, poses)
    return voxels, poses, disps, intrinsics
