"""Event stream -> voxel grid and voxel standardisation on the GPU, with the reference's function
names and argument meaning: utils/event_utils.py:180-232 `to_voxel_grid`, utils/voxel_utils.py:6-28 `std`
(== the NORM='std' branch of devo/devo.py:438-452), utils/voxel_utils.py:31-51 `rescale`, utils/event_utils.py:235-262
`RemoveHotPixelsVoxel`, utils/voxel_utils.py:55-136 `evs2rgb`, `rgb2evs`, `voxel_augment` (the training-time augmentation); and the
loaders' front end (utils/load_utils.py:47-76) for a whole recording: `voxel_grids` (many
windows of one stream in one call, rectified, hot pixels removed) and `real_data_voxels` (get_real_data_list's output).
Inputs are device tensors; no CPU fallback."""
import math
import numpy as np
import torch
from . import _lib as L


def to_voxel_grid(xs, ys, ts, ps, H=480, W=640, nb_of_time_bins=5):
    """xs, ys: pixel coordinates [N] (any numeric dtype; rectified = fractional allowed), ts: timestamps [N] ascending,
    ps: polarity [N] (0 / 1 or -1 / 1) -> voxel grid [nb_of_time_bins, H, W] float32 on the same GPU."""
    L.require_gpu(xs, ys, ts, ps)
    N = xs.numel()
    x = xs.reshape(-1).float().contiguous()
    y = ys.reshape(-1).float().contiguous()
    t = ts.reshape(-1).double().contiguous()
    p = ps.reshape(-1).to(torch.int8).contiguous()
    grid = torch.empty(int(nb_of_time_bins), int(H), int(W), dtype=torch.float32, device=xs.device)
    rc = L.lib().devo_voxelize(L.ptr(x), L.ptr(y), L.ptr(t), L.ptr(p), N, int(H), int(W), int(nb_of_time_bins), L.ptr(grid), L.stream())
    L.check(rc, "events.to_voxel_grid")
    return grid


def std(voxs, sequence=True):
    """voxs [b, n, c, h, w] float32 -> standardised copy (non-zero voxels of every sequence, or of every frame)."""
    L.require_gpu(voxs)
    b, n, c, h, w = voxs.shape
    out = voxs.float().contiguous().clone()
    nseg = b if sequence else b * n
    ws = torch.empty(L.lib().devo_voxel_std_workspace_bytes(nseg), dtype=torch.uint8, device=voxs.device)
    rc = L.lib().devo_voxel_std(L.ptr(out), nseg, out.numel() // max(nseg, 1), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "events.std")
    return out.view(b, n, c, h, w)


def _window_inputs(xs, ys, ts, ps, rectify_map, H, W):
    """The stream as devo_voxelize_windows reads it: (x, y, t, ts_is_i64, p, map)."""
    L.require_gpu(xs, ys, ts, ps, rectify_map)
    if rectify_map is not None:
        if tuple(rectify_map.shape) != (int(H), int(W), 2):
            raise ValueError(f"rectify_map must be [H, W, 2] = [{H}, {W}, 2] (the sensor size), got {tuple(rectify_map.shape)}")
        if xs.is_floating_point() or ys.is_floating_point():
            raise TypeError("with a rectify_map, xs and ys are the raw integer sensor coordinates")
        x = xs.reshape(-1).to(torch.int32).contiguous()
        y = ys.reshape(-1).to(torch.int32).contiguous()
        m = rectify_map.float().contiguous()
    else:
        x = xs.reshape(-1).float().contiguous()
        y = ys.reshape(-1).float().contiguous()
        m = None
    if ts.dtype == torch.int64:
        t, i64 = ts.reshape(-1).contiguous(), 1                  # microseconds, converted inside the kernels
    else:
        t, i64 = ts.reshape(-1).double().contiguous(), 0
    p = ps.reshape(-1).to(torch.int8).contiguous()
    if not (x.numel() == y.numel() == t.numel() == p.numel()):
        raise ValueError("xs, ys, ts and ps must have the same number of events")
    return x, y, t, i64, p, m


def _as_window_times(t, device):
    if isinstance(t, torch.Tensor):
        L.require_gpu(t)
        return t.reshape(-1).to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.asarray(t, dtype=np.float64).reshape(-1), device=device)


def _voxel_grids(x, y, t, i64, p, m, t0, t1, H, W, bins, hot_pixel_stds, out):
    S = t0.numel()
    if t1.numel() != S:
        raise ValueError("t0 and t1 must hold the same number of windows")
    shape = (S, int(bins), int(H), int(W))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        L.require_gpu(out)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape}")
    counts = torch.empty(S, dtype=torch.int64, device=x.device)
    h = L.lib()
    ws = torch.empty(h.devo_voxelize_windows_workspace_bytes(S), dtype=torch.uint8, device=x.device)
    rc = h.devo_voxelize_windows(L.ptr(x), L.ptr(y), L.ptr(t), i64, L.ptr(p), x.numel(), L.ptr(t0), L.ptr(t1), S, L.ptr(m), int(H), int(W),
                                 int(bins), L.ptr(out), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "events.voxel_grids")
    if hot_pixel_stds is not None:
        _hot_pixels_(out, S, int(bins) * int(H) * int(W), hot_pixel_stds)
    return out, counts


def voxel_grids(xs, ys, ts, ps, t0, t1, H, W, bins=5, rectify_map=None, hot_pixel_stds=None, out=None):
    """Voxel grids of S windows [t0[s], t1[s]) of ONE event stream (EventSlicer.get_events + to_voxel_grid + RemoveHotPixelsVoxel
    of utils/load_utils.py:47-62, for every window at once).

    xs, ys: raw integer sensor coordinates when `rectify_map` [H, W, 2] is given (the event votes at rectify_map[y, x]), pixel
    coordinates (float) otherwise; ts [N] ascending, int64 microseconds or float; ps [N] 0 / 1 or -1 / 1; t0, t1: S window
    bounds (device tensors or host sequences).  Every window's time axis is normalised by its own first and last event.
    hot_pixel_stds: RemoveHotPixelsVoxel(num_stds) applied to every window (None: off).  out: optional [S, bins, H, W] float32.
    Returns (grids [S, bins, H, W] float32, counts [S] int64: events per window), both on the device; no host synchronisation."""
    x, y, t, i64, p, m = _window_inputs(xs, ys, ts, ps, rectify_map, H, W)
    return _voxel_grids(x, y, t, i64, p, m, _as_window_times(t0, x.device), _as_window_times(t1, x.device), H, W, bins, hot_pixel_stds, out)


def _hot_pixels_(v, nseg, length, num_stds):
    h = L.lib()
    ws = torch.empty(h.devo_voxel_hot_pixels_workspace_bytes(nseg), dtype=torch.uint8, device=v.device)
    rc = h.devo_voxel_hot_pixels(L.ptr(v), nseg, length, float(num_stds), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "events.remove_hot_pixels")


def remove_hot_pixels(vox, num_stds):
    """RemoveHotPixelsVoxel(num_stds) (utils/event_utils.py:235-262) on every grid of vox [..., bins, H, W]: a float32 copy in which
    every voxel with |v| > mean + num_stds * std (over the grid's bins * H * W voxels, zeros included; unbiased std) is zero."""
    L.require_gpu(vox)
    if vox.dim() < 3:
        raise ValueError("remove_hot_pixels expects [..., bins, H, W]")
    out = vox.float().contiguous().clone()
    length = out.shape[-3] * out.shape[-2] * out.shape[-1]
    _hot_pixels_(out, out.numel() // max(length, 1), length, num_stds)
    return out


class RemoveHotPixelsVoxel:
    """Drop-in for utils/event_utils.py:RemoveHotPixelsVoxel (a loader transform on one [bins, H, W] grid), num_stds mode only.
    Returns the filtered grid as a new tensor."""

    def __init__(self, num_stds=10, num_hot_pixels=None):
        if num_hot_pixels is not None:
            raise NotImplementedError("RemoveHotPixelsVoxel(num_hot_pixels=...) (the top-k mode) is not implemented: no loader uses it; "
                                      "use num_stds")
        self.num_stds = num_stds
        self.num_hot_pixels = None

    def __call__(self, x):
        return remove_hot_pixels(x, self.num_stds)


def rescale(voxs, sequence=True):
    """rescale (utils/voxel_utils.py:31-51) of voxs [b, n, c, h, w]: a float32 copy with the positive voxels divided by the largest
    positive voxel and the negative ones by minus the smallest negative voxel.  Both extremes are taken over the WHOLE tensor for
    either value of `sequence` (the reference's masked selection is 1-D, so its flag changes nothing); a sign without voxels is
    left unchanged."""
    L.require_gpu(voxs)
    b, n, c, h, w = voxs.shape
    src = voxs.float().contiguous()
    out = torch.empty_like(src)
    lib = L.lib()
    ws = torch.empty(lib.devo_voxel_rescale_workspace_bytes(), dtype=torch.uint8, device=voxs.device)
    rc = lib.devo_voxel_rescale(L.ptr(src), L.ptr(out), src.numel(), L.ptr(ws), ws.numel(), L.stream())
    L.check(rc, "events.rescale")
    return out


def real_data_voxels(xs, ys, ts, ps, tss_imgs_us, dT_ms, intrinsics, rectify_map, H, W, hot_pixel_stds, chunk=64, ms_index_len=None,
                     t_offset=0, out_hw=None):
    """What get_real_data_list (utils/load_utils.py:64-76) returns, in its order, computed on the GPU: for every image timestamp
    ts_img, the window [ts_img, ts_img + dT_ms * 1e3) of the stream, rectified through rectify_map [H, W, 2] (raw integer xs, ys),
    voxelised at sensor size and filtered with RemoveHotPixelsVoxel(hot_pixel_stds) (None: no filter).  Yields
    (voxel [5, H, W] float32 on the device, torch.as_tensor(intrinsics), (t0 + t1) / 2); windows without events are skipped.

    ts are in the same time base as tss_imgs_us (EventSlicer returns the recording's t plus t_offset).  ms_index_len: the length
    of the recording's ms_to_idx; when given, windows EventSlicer cannot serve (ceil((t1 - t_offset) / 1000) past its end) are
    skipped as well.  Windows are processed `chunk` at a time, with one host synchronisation per chunk (the event counts).
    out_hw: the loaders' Resize target; only the sensor size (H, W) is supported."""
    if out_hw is not None and tuple(out_hw) != (int(H), int(W)):
        raise NotImplementedError(f"real_data_voxels: resizing the voxels to {tuple(out_hw)} is not supported (sensor size {H}x{W} only)")
    x, y, t, i64, p, m = _window_inputs(xs, ys, ts, ps, rectify_map, H, W)
    t0s = np.asarray(tss_imgs_us, dtype=np.float64).reshape(-1)
    t1s = t0s + dT_ms * 1e3
    keep = np.ones(len(t0s), dtype=bool)
    if ms_index_len is not None:
        for i, (a, b) in enumerate(zip(t0s, t1s)):                  # EventSlicer.get_events: ms2idx(...) is None -> skipped
            start_ms = max(math.floor((a - t_offset) / 1000), 0)
            end_ms = math.ceil((b - t_offset) / 1000)
            keep[i] = start_ms < ms_index_len and end_ms < ms_index_len
    idx = np.nonzero(keep)[0]
    dev = x.device
    t0_d = torch.as_tensor(t0s[idx], device=dev)
    t1_d = torch.as_tensor(t1s[idx], device=dev)
    chunk = max(int(chunk), 1)
    for c0 in range(0, len(idx), chunk):
        grids, counts = _voxel_grids(x, y, t, i64, p, m, t0_d[c0:c0 + chunk], t1_d[c0:c0 + chunk], H, W, 5, hot_pixel_stds, None)
        counts = counts.cpu()
        for j in range(grids.shape[0]):
            if counts[j] == 0:
                continue
            i = idx[c0 + j]
            yield grids[j], torch.as_tensor(intrinsics).clone(), (t0s[i] + t1s[i]) / 2


# ---- voxel augmentation (utils/voxel_utils.py:55-136)

AUG_OPS = ("adjust_brightness", "adjust_contrast", "invert", "posterize", "adjust_saturation", "adjust_sharpness", "solarize")   # :99-101, in order


def evs2rgb(voxs):
    """evs2rgb (utils/voxel_utils.py:55-67) without its host asserts: [..., h, w] -> [..., 3, h, w] with R = the negative part (as a
    positive value), G = 0, B = the positive part."""
    pos = torch.where(voxs < 0.0, torch.zeros_like(voxs), voxs)
    neg = torch.where(voxs > 0.0, torch.zeros_like(voxs), voxs) * -1.0
    return torch.stack((neg, torch.zeros_like(pos), pos), dim=-3)


def rgb2evs(rgb):
    """rgb2evs (utils/voxel_utils.py:70-75): [..., 3, h, w] -> B + (-R), [..., h, w]."""
    return rgb[..., 2, :, :] + (-rgb[..., 0, :, :])


def aug_factors(num_bins=10):
    """_aug_factors (utils/voxel_utils.py:104-114): the factor table of every op in AUG_OPS order; `num_bins` is the number of factor
    steps (not voxel bins).  float32 linspaces for the blends, the posterize bits (int32), a 0-d placeholder for invert, the solarize
    thresholds (int32)."""
    return [
        torch.linspace(0.1, 0.2, num_bins),
        torch.linspace(0.05, 0.2, num_bins),
        torch.tensor(0.0),
        8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int(),
        torch.linspace(0.05, 0.2, num_bins),
        torch.linspace(0.9, 2.0, num_bins),
        torch.linspace(0, 30, num_bins).round().int(),
    ]


def draw_augmentation(num_bins=10):
    """voxel_augment's random choice (utils/voxel_utils.py:124-125): op = torch.randint(7, (1,)), then factor_index =
    torch.randint(num_bins, (1,)), both from torch's default CPU generator and always both (invert draws an unused index too), so a
    seeded run picks what the reference picks.  Host only.  Returns (op index into AUG_OPS, factor index)."""
    op = int(torch.randint(len(AUG_OPS), (1,)).item())
    factor_index = int(torch.randint(num_bins, (1,)).item())
    return op, factor_index


def _op_index(op):
    if isinstance(op, str):
        if op not in AUG_OPS:
            raise ValueError(f"unknown augmentation op {op!r}: one of {AUG_OPS}")
        return AUG_OPS.index(op)
    i = int(op)
    if not 0 <= i < len(AUG_OPS):
        raise ValueError(f"unknown augmentation op index {i}: 0..{len(AUG_OPS) - 1}")
    return i


def _op_factor(op, factor_index, num_bins):
    table = aug_factors(num_bins)[op]
    if table.dim() == 0:
        return 0.0                                                 # invert: no factor
    if factor_index is None:
        raise ValueError(f"{AUG_OPS[op]} needs a factor_index")
    return float(table[int(factor_index)])                         # _blend's float(ratio): the fp32 table value


def _augment_call(voxs, op, factor, rescale, standardise):
    L.require_gpu(voxs)
    if voxs.dim() != 5:
        raise ValueError(f"expected voxel grids [b, n, c, h, w], got {tuple(voxs.shape)}")
    b, n, c, h, w = voxs.shape
    src = voxs.float().contiguous()
    out = torch.empty_like(src)
    lib = L.lib()
    ws = torch.empty(lib.devo_voxel_augment_workspace_bytes(b, n * c), dtype=torch.uint8, device=voxs.device)
    rc = lib.devo_voxel_augment(L.ptr(src), L.ptr(out), b, n * c, h, w, int(rescale), op, float(factor), int(standardise), L.ptr(ws),
                                ws.numel(), L.stream())
    L.check(rc, "events.voxel_augment")
    return out


def augment(voxs, op, factor_index=None, num_bins=10):
    """_augment (utils/voxel_utils.py:78-96) with the op AUG_OPS[op] (an index or a name) at aug_factors(num_bins)[op][factor_index]
    on an already rescaled grid voxs [b, n, c, h, w] (values in [-1, 1]; the reference asserts this, values outside are clamped here):
    quantised to uint8 R / B images, the torchvision op applied per (b, n, c) image, back to float.  No standardisation.  Returns a new
    float32 tensor."""
    i = _op_index(op)
    return _augment_call(voxs, i, _op_factor(i, factor_index, num_bins), rescale=False, standardise=False)


def voxel_augment(voxs, rescaled=False, num_bins=10, op=None, factor_index=None):
    """voxel_augment (utils/voxel_utils.py:117-136) of voxs [b, n, c, h, w]: rescale (unless `rescaled`), _augment with one op, then
    std (sequence-wise), in one HIP call.  op=None draws op and factor index as the reference does (draw_augmentation: two draws from
    torch's default CPU generator, no device synchronisation); otherwise op (index or name) and factor_index choose them.  Returns a new
    float32 tensor and leaves voxs unchanged (the reference's rescale writes into its input)."""
    if op is None:
        if factor_index is not None:
            raise ValueError("factor_index without op")
        op, factor_index = draw_augmentation(num_bins)
    i = _op_index(op)
    return _augment_call(voxs, i, _op_factor(i, factor_index, num_bins), rescale=not rescaled, standardise=True)
