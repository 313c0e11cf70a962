#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Generate tests/golden/voxel_augment.npz by running the REAL reference utils/voxel_utils.py (rescale, evs2rgb, _augment, rgb2evs, std,
_aug_factors, voxel_augment) from /root/reference on CPU over small seeded voxel grids.

The reference imports `torchvision.transforms.functional as f` at module level and torchvision is not installed here, so that module is
a stub whose seven ops (adjust_brightness, adjust_contrast, invert, posterize, adjust_saturation, adjust_sharpness, solarize) are
restated below from torchvision 0.13's tensor implementation (transforms/functional_tensor.py, the version environment.yml pins) — in
torch, independently of the HIP kernels, as tools/gen_golden_nms.py does for batched_nms.  The file holds data only.

Contents:
  aug/x [1, 2, 5, 20, 28]   a rescaled grid (values in [-1, 1]): ~70 % zeros, magnitudes over four decades, voxels on and one ulp
                            either side of the quantisation steps k / 255, exact +-1
  aug/x_odd [1, 1, 5, 13, 19], aug/x_tiny [1, 1, 5, 2, 2]   odd sizes; a 2 x 2 image (adjust_sharpness returns it unchanged)
  aug/<grid>/<op>_<fi>      _augment(grid, op, _aug_factors(10)[op][fi]) for fi in {0, 3, 6, 9} (invert: <op>_0 only)
  raw/x [1, 2, 5, 20, 28]   an unscaled grid (magnitudes over several decades, both signs)
  va/<r>/<seed>             voxel_augment(grid, rescaled=r, num_bins=10) after torch.manual_seed(seed); r = 1 on aug/x, r = 0 on raw/x
  va/<r>/<seed>/choice      the (op, factor index) the seed draws
  factors/<i>               _aug_factors(10)[i]
"""
import os
import sys
import types
import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
FACTOR_INDICES = (0, 3, 6, 9)
SEEDS = (0, 1, 2, 3, 4, 5, 7, 13, 14, 20)


# ---- torchvision 0.13, transforms/functional_tensor.py, uint8 tensors [N, 3, H, W]

def _blend(img1, img2, ratio):
    ratio = float(ratio)
    bound = 1.0 if img1.is_floating_point() else 255.0
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, bound).to(img1.dtype)


def rgb_to_grayscale(img):
    r, g, b = img.unbind(dim=-3)
    l_img = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype)
    return l_img.unsqueeze(dim=-3)


def adjust_brightness(img, brightness_factor):
    if brightness_factor < 0:
        raise ValueError("brightness_factor is not non-negative")
    return _blend(img, torch.zeros_like(img), brightness_factor)


def adjust_contrast(img, contrast_factor):
    if contrast_factor < 0:
        raise ValueError("contrast_factor is not non-negative")
    mean = torch.mean(rgb_to_grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
    return _blend(img, mean, contrast_factor)


def invert(img):
    return 255 - img


def posterize(img, bits):
    mask = -int(2 ** (8 - bits))
    return img & mask


def adjust_saturation(img, saturation_factor):
    if saturation_factor < 0:
        raise ValueError("saturation_factor is not non-negative")
    return _blend(img, rgb_to_grayscale(img), saturation_factor)


def _blurred_degenerate_image(img):
    kernel = torch.ones((3, 3), dtype=torch.float32)
    kernel[1, 1] = 5.0
    kernel /= kernel.sum()
    kernel = kernel.expand(img.shape[-3], 1, kernel.shape[0], kernel.shape[1])
    tmp = F.conv2d(img.to(torch.float32), kernel, groups=img.shape[-3])          # _cast_squeeze_in / _out: float32, then round
    tmp = torch.round(tmp).to(img.dtype)
    result = img.clone()
    result[..., 1:-1, 1:-1] = tmp
    return result


def adjust_sharpness(img, sharpness_factor):
    if sharpness_factor < 0:
        raise ValueError("sharpness_factor is not non-negative")
    if img.size(-1) <= 2 or img.size(-2) <= 2:
        return img
    return _blend(img, _blurred_degenerate_image(img), sharpness_factor)


def solarize(img, threshold):
    if threshold > 255:
        raise TypeError("Threshold should be less than bound of img.")
    return torch.where(img >= threshold, invert(img), img)


def _reference():
    m = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")
    for f in (adjust_brightness, adjust_contrast, invert, posterize, adjust_saturation, adjust_sharpness, solarize):
        setattr(fn, f.__name__, f)
    m.transforms, tr.functional = tr, fn
    sys.modules.update({"torchvision": m, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    sys.path.insert(0, REF)
    import utils  # noqa: F401
    from utils import voxel_utils
    return voxel_utils


# ---- inputs

def rescaled_grid(rng, shape):
    """Values in [-1, 1]: ~70 % zeros, log-uniform magnitudes over 1e-4..1, a share on the quantisation steps fl(k / 255) and one ulp
    either side of them, and the extremes +-1."""
    n = int(np.prod(shape))
    mag = 10.0 ** rng.uniform(-4, 0, n)
    k = rng.integers(1, 256, n).astype(np.float32) / np.float32(255)
    step = rng.random(n)
    mag = np.where(step < 0.3, k, mag).astype(np.float32)
    mag = np.where((step >= 0.3) & (step < 0.4), np.nextafter(k, np.float32(2)), mag)
    mag = np.where((step >= 0.4) & (step < 0.5), np.nextafter(k, np.float32(0)), mag)
    mag = np.minimum(mag, np.float32(1))
    v = np.where(rng.random(n) < 0.5, -mag, mag).astype(np.float32)
    v[rng.random(n) < 0.7] = 0.0
    v[0], v[1] = 1.0, -1.0
    return torch.from_numpy(v.reshape(shape))


def raw_grid(rng, shape):
    n = int(np.prod(shape))
    v = (10.0 ** rng.uniform(-3, 1, n) * np.where(rng.random(n) < 0.45, -1.0, 1.0)).astype(np.float32)
    v[rng.random(n) < 0.7] = 0.0
    return torch.from_numpy(v.reshape(shape))


def main():
    vu = _reference()
    ops, factors = vu._aug_ops(), vu._aug_factors(10)
    names = [f.__name__ for f in ops]
    rng = np.random.default_rng(20261016)
    out = {}
    for i, t in enumerate(factors):
        out[f"factors/{i}"] = t.numpy()
    grids = {"x": rescaled_grid(rng, (1, 2, 5, 20, 28)), "x_odd": rescaled_grid(rng, (1, 1, 5, 13, 19)),
             "x_tiny": rescaled_grid(rng, (1, 1, 5, 2, 2))}
    for g, x in grids.items():
        out[f"aug/{g}"] = x.numpy()
        for i, (name, op) in enumerate(zip(names, ops)):
            for fi in ((0,) if factors[i].ndim == 0 else FACTOR_INDICES):
                factor = None if factors[i].ndim == 0 else factors[i][fi]
                out[f"aug/{g}/{name}_{fi}"] = vu._augment(x.clone(), op=op, factor=factor).numpy()
    raw = raw_grid(rng, (1, 2, 5, 20, 28))
    out["raw/x"] = raw.numpy()
    seen = set()
    for r, x in ((1, grids["x"]), (0, raw)):
        for s in SEEDS:
            torch.manual_seed(s)
            op, fi = int(torch.randint(7, (1,)).item()), int(torch.randint(10, (1,)).item())
            torch.manual_seed(s)
            out[f"va/{r}/{s}"] = vu.voxel_augment(x.clone(), rescaled=bool(r), num_bins=10).numpy()
            out[f"va/{r}/{s}/choice"] = np.array([op, fi], dtype=np.int64)
            seen.add(op)
    assert seen == set(range(7)), f"the seeds draw only the ops {sorted(seen)}"
    path = os.path.join(ROOT, "tests", "golden", "voxel_augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
