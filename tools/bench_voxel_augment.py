#!/usr/bin/env python3
"""Time the voxel augmentation (devo_amd.events: devo_voxel_augment) at the training size [1, 15, 5, 480, 640] for each op, against a
torch composition that follows the reference's voxel_augment step by step (utils/voxel_utils.py:117-136: rescale with its host
`.item()`, evs2rgb with its clones, masked writes and host asserts, the 6-D stack, uint8 casts, the op, rgb2evs, std).  torchvision is
not installed, so the seven ops are written in torch below, after torchvision 0.13's tensor code.  Every composition's output is checked
against the HIP call before it is timed.  Device events after warm-up; prints one block of text (profiles/voxel_augment.txt).

    python tools/bench_voxel_augment.py [--reps 20]"""
import argparse
import os
import sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devo_amd import events

SHAPE = (1, 15, 5, 480, 640)


# ---- the reference's sequence in torch (voxel_utils.py) with torchvision 0.13's uint8 ops

def t_rescale(v):
    flat = v.view(v.shape[0], -1)
    pos, neg = flat > 0.0, flat < 0.0
    vmax = flat[pos].max(dim=-1)[0] if pos.sum().item() else None
    vmin = flat[neg].min(dim=-1)[0] if neg.sum().item() else None
    if vmax is not None:
        flat[pos] = flat[pos] / vmax
    if vmin is not None:
        flat[neg] = flat[neg] / -vmin
    return flat.view(v.shape)


def t_evs2rgb(v):
    pos, neg = v.clone(), v.clone()
    pos[v < 0.0] = 0.0
    neg[v > 0.0] = 0.0
    assert pos.min().item() >= 0.0 and pos.max().item() <= 1.0
    assert neg.max().item() <= 0.0 and neg.min().item() >= -1.0
    neg *= -1.0
    return torch.stack((neg, torch.zeros_like(pos), pos), dim=-3)


def t_blend(a, b, ratio):
    ratio = float(ratio)
    return (ratio * a + (1.0 - ratio) * b).clamp(0, 255).to(a.dtype)


def t_gray(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(-3)


def t_blur(img):
    k = torch.ones((3, 3), dtype=torch.float32, device=img.device)
    k[1, 1] = 5.0
    k /= k.sum()
    k = k.expand(img.shape[-3], 1, 3, 3)
    tmp = torch.round(F.conv2d(img.to(torch.float32), k, groups=img.shape[-3])).to(img.dtype)
    out = img.clone()
    out[..., 1:-1, 1:-1] = tmp
    return out


OPS = {
    "adjust_brightness": lambda img, f: t_blend(img, torch.zeros_like(img), f),
    "adjust_contrast": lambda img, f: t_blend(img, torch.mean(t_gray(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True), f),
    "invert": lambda img, f: 255 - img,
    "posterize": lambda img, f: img & -int(2 ** (8 - int(f))),
    "adjust_saturation": lambda img, f: t_blend(img, t_gray(img), f),
    "adjust_sharpness": lambda img, f: t_blend(img, t_blur(img), f),
    "solarize": lambda img, f: torch.where(img >= f, 255 - img, img),
}


def t_std(v):
    b, n, c, h, w = v.shape
    flat = v.view(b, -1)
    nz = flat != 0.0
    cnt = nz.sum(dim=-1)
    if torch.all(cnt > 0):
        mean = torch.sum(flat, dim=-1, dtype=torch.float32) / cnt
        sd = torch.sqrt(torch.sum(flat ** 2, dim=-1, dtype=torch.float32) / cnt - mean ** 2)
        flat = nz.type_as(flat) * (flat - mean[..., None]) / sd[..., None]
    return flat.view(b, n, c, h, w)


def torch_voxel_augment(v, name, factor, rescale=True, std=True):
    if rescale:
        v = t_rescale(v)
    rgb = (255 * t_evs2rgb(v)).to(torch.uint8)
    flat = OPS[name](rgb.flatten(0, 2), factor)
    rgb = flat.view(*rgb.shape).to(torch.float32) / 255
    out = rgb[..., 2, :, :] + (-rgb[..., 0, :, :])
    return t_std(out) if std else out


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    mag = torch.pow(10.0, torch.rand(SHAPE, generator=g, device=dev) * 4 - 3)
    sign = torch.where(torch.rand(SHAPE, generator=g, device=dev) < 0.5, -1.0, 1.0)
    raw = (mag * sign * (torch.rand(SHAPE, generator=g, device=dev) >= 0.7)).float().contiguous()
    x = events.rescale(raw)
    mb = raw.numel() * 4 / 1e6
    fi = 5
    print(f"voxel augmentation {list(SHAPE)} fp32 ({mb:.0f} MB), factor index {fi}, reps {args.reps}; {torch.cuda.get_device_name()}")
    print(f"{'op':>18} {'HIP aug only':>13} {'TB/s':>6} {'HIP full':>9} {'torch aug only':>15} {'torch full':>11} {'full x':>7}")
    for name in events.AUG_OPS:
        f = events.aug_factors(10)[events.AUG_OPS.index(name)]
        f = f if f.dim() == 0 else f[fi]
        # outputs first: the composition must compute what the HIP call computes
        a = events.augment(x, name, fi)
        b = torch_voxel_augment(x.clone(), name, f, rescale=False, std=False)
        lv = ((a.double() - b.double()).abs() * 255).round()
        assert float(lv.max()) <= (1 if name == "adjust_contrast" else 0), f"{name}: augment differs by {float(lv.max())} levels"
        a = events.voxel_augment(raw, op=name, factor_index=fi)
        b = torch_voxel_augment(raw.clone(), name, f)
        err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
        assert err <= 1e-5, f"{name}: voxel_augment differs by {err:.2e}"
        t_aug = timed(lambda: events.augment(x, name, fi), args.reps)
        t_full = timed(lambda: events.voxel_augment(raw, op=name, factor_index=fi), args.reps)
        t_taug = timed(lambda: torch_voxel_augment(x.clone(), name, f, rescale=False, std=False), args.reps)
        t_tfull = timed(lambda: torch_voxel_augment(raw.clone(), name, f), args.reps)
        print(f"{name:>18} {t_aug * 1e3:10.1f} us {2 * mb / t_aug / 1e3:6.2f} {t_full * 1e3:6.1f} us {t_taug * 1e3:12.1f} us "
              f"{t_tfull * 1e3:8.1f} us {t_tfull / t_full:6.1f}x")
    print("aug only: augment() on a rescaled grid (quantise, op, back to float; contrast adds the grayscale-sum pass); TB/s = 2 x "
          f"{mb:.0f} MB / time.  full: voxel_augment() = rescale + op + std (HIP), the reference's sequence (torch; its .item() and "
          "asserts synchronise with the host; its times include one clone of the input, which the reference's rescale writes into).")


if __name__ == "__main__":
    main()
