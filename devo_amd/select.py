"""Patch selection on the GPU in one launch (devo/selector.py:50-287, PatchSelector.__call__, and what devo/enet.py:100-200 derives from the
chosen centres) over csrc/select.hip.

`select` does for one mode what `devo_amd.patchifier.select` does as a torch composition — zero padding to whole cells, the 4 x 4 pooling,
the ranking, the choice of cells and pixels, the shift back into the map — and in the same launch the tail the Patchifier hangs behind it:
the score at each centre, `xy`, `index` and the closed-form `patches`.  One workgroup per frame; the result is bit-reproducible.

  * one total order everywhere: the higher key ranks first, on equal keys the lower flat cell index;
  * `multi` is sampling without replacement as an exponential race on noise the caller may supply: `noise` fp32 [n, C + 16 m] of Exp(1)
    draws (`cells(h, w, grid, k)` gives C).  noise[:, :C] ranks the cells — key (mean + 1e-7) / noise with the grid, mean / noise without —,
    noise[:, C + 16 s : C + 16 s + 16] picks the pixel of output slot s in the reference's window (one pixel up-left of the cell).  With
    `noise=None` it is drawn by ONE `torch.empty(...).exponential_()` from torch's generator: reproducible under `torch.manual_seed`,
    legal under stream capture.  The draws follow the reference's law, not torch.multinomial's random stream;
  * `nms` reads the n survivor counts back once and raises like `patchifier.select_nms` when a frame keeps fewer than m boxes.  Under stream
    capture nothing can be read: the check is skipped and the unfilled slots repeat the frame's last survivor;
  * `3xrandom` ranks 3 m candidates (x, y) per frame — drawn with `torch.randint` on the padded map when not given — and returns the m best
    as x + 1, y + 1 with their scores in ascending order, like the reference's `_3xrandom`; `pad=False` runs it on the map as it is (the
    scorer's training branch, enet.py:152-164).

No CPU fallback: CPU tensors raise.  No host synchronisation apart from the nms count, no allocation outside torch's caching allocator.
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import backends

MAX_CELLS = 4096              # DEVO_SELECT_MAX_CELLS: cells per frame, patches per frame, 3xrandom candidates per frame
MODES = {"topk": 0, "multi": 1, "nms": 2, "3xrandom": 3}   # DEVO_SELECT_*

Selection = namedtuple("Selection", ("x", "y", "xy", "scores", "patches", "index"))


def padding(h, w, grid=True, k=4):
    """(top, left, padded height, padded width) of PatchSelector.__call__'s centred zero padding (the odd pixel goes bottom / right)."""
    f = 2 * k if grid else k
    ph, pw = (f - h % f) % f, (f - w % f) % f
    return ph // 2, pw // 2, h + ph, w + pw


def cells(h, w, grid=True, k=4):
    """C: the number of k x k cells of the padded h x w map (the first C noise values of a frame rank them)."""
    _, _, hp, wp = padding(h, w, grid, k)
    return (hp // k) * (wp // k)


def select(scores, m, mode, grid=True, k=4, *, noise=None, candidates=None, offset=0, clamp=None, disps=None, P=3, pad=True):
    """scores fp32 [n, h, w] or [1, n, h, w] on the GPU (any strides) -> Selection(x, y int64 [n, m]; xy fp32 [n, m, 2]; scores fp32 [n, m]: the
    map at the centre before `offset` (3xrandom: the candidates' scores, ascending); patches fp32 [n m, 3, P, P]; index int64 [n m]).
    offset: added to x and y after the shift back into the map; clamp = ((x0, x1), (y0, y1)): the final range (None: none);
    disps fp32 [n, H, W] or [1, n, H, W]: the inverse depths for the patches' third plane (None: 1).  It must have the size of the frame the
    centres live in (the feature map): patch pixels outside H x W get depth 0 and zeroed coordinates, as in Patchifier.forward.
    pad=False (3xrandom only): no padding, no clamp into the map — the scorer's training branch."""
    mode = mode.lower()
    if mode not in MODES:
        raise NotImplementedError(f"patch selection mode {mode!r} (have: 3xrandom, topk, multi, nms)")
    L.require_gpu(scores, noise, disps)
    if scores.dim() == 4 and scores.shape[0] == 1:
        scores = scores[0]
    if scores.dim() != 3 or scores.dtype != torch.float32:
        raise ValueError("select: scores must be float32 [n, h, w] or [1, n, h, w]")
    n, h, w = scores.shape
    m, k, P = int(m), int(k), int(P)
    if k != 4:
        raise NotImplementedError(f"select: cells of {k} x {k} (the kernel is built for the reference's 4 x 4 cells)")
    if not pad and mode != "3xrandom":
        raise ValueError("select: only 3xrandom runs on the unpadded map")
    top, left, hp, wp = padding(h, w, grid, k) if pad else (0, 0, h, w)
    C = (hp // k) * (wp // k)
    if m < 1 or m > MAX_CELLS or (mode == "3xrandom" and 3 * m > MAX_CELLS):
        raise ValueError(f"select: {m} patches per frame: at most {MAX_CELLS} ({MAX_CELLS // 3} in 3xrandom, which ranks 3 m candidates)")
    if mode != "3xrandom":
        if C > MAX_CELLS:
            raise ValueError(f"select: a {h} x {w} score map has {C} cells of {k} x {k} per frame; the kernel takes at most {MAX_CELLS} "
                             "(DEVO_PATCHIFIER_SELECT=0: the Patchifier's torch composition has no limit)")
        if mode != "nms" and (m > C or (grid and m % 4)):
            raise ValueError(f"select: {m} patches from {C} cells" + (" in 4 quadrants (m must be a multiple of 4)" if grid else ""))
    dev = scores.device
    cx = cy = None
    with torch.cuda.device(dev):
        if mode == "multi":
            if noise is None:
                noise = torch.empty((n, C + 16 * m), dtype=torch.float32, device=dev).exponential_()
            elif noise.shape != (n, C + 16 * m) or noise.dtype != torch.float32 or not noise.is_contiguous() or noise.device != dev:
                raise ValueError(f"select: noise must be contiguous float32 [n, C + 16 m] = [{n}, {C + 16 * m}] on the scores' device")
        elif mode == "3xrandom":
            if candidates is None:                   # on the padded map, x then y, as patchifier.select draws them
                cx = torch.randint(0, wp, (n, 3 * m), device=dev)
                cy = torch.randint(0, hp, (n, 3 * m), device=dev)
            else:
                cx, cy = candidates
                L.require_gpu(cx, cy)
                for t in (cx, cy):
                    if t.shape != (n, 3 * m) or t.dtype != torch.int64 or not t.is_contiguous() or t.device != dev:
                        raise ValueError(f"select: candidates must be contiguous int64 [n, 3 m] = [{n}, {3 * m}] on the scores' device")
        if disps is not None:
            if disps.dim() == 4 and disps.shape[0] == 1:
                disps = disps[0]
            if disps.dim() != 3 or disps.shape[0] != n or disps.device != dev:
                raise ValueError("select: disps must be [n, H, W] or [1, n, H, W] on the scores' device")
            if disps.dtype != torch.float32:
                disps = disps.float()
        (x0, x1), (y0, y1) = clamp if clamp is not None else ((0, 0), (0, 0))
        nat = backends.native()
        if nat is not None:
            x, y, xy, sc, patches, index, counts = nat.select.patch_select(scores, m, MODES[mode], bool(grid), k, bool(pad), noise if mode == "multi" else None, cx, cy,
                                                                           int(offset), clamp is not None, int(x0), int(x1), int(y0), int(y1), disps, P)
        else:
            x = torch.empty((n, m), dtype=torch.int64, device=dev)
            y, index = torch.empty_like(x), torch.empty(n * m, dtype=torch.int64, device=dev)
            xy = torch.empty((n, m, 2), dtype=torch.float32, device=dev)
            sc = torch.empty((n, m), dtype=torch.float32, device=dev)
            patches = torch.empty((n * m, 3, P, P), dtype=torch.float32, device=dev)
            counts = torch.empty(n if mode == "nms" else 0, dtype=torch.int32, device=dev)
            ds = disps.stride() if disps is not None else (0, 0, 0)
            dH, dW = disps.shape[1:] if disps is not None else (0, 0)
            rc = L.lib().devo_patch_select(L.ptr(scores), *scores.stride(), n, h, w, m, MODES[mode], int(bool(grid)), k, int(bool(pad)),
                                           L.ptr(noise if mode == "multi" else None), L.ptr(cx), L.ptr(cy), int(offset), int(clamp is not None), int(x0), int(x1),
                                           int(y0), int(y1), L.ptr(disps), *ds, dH, dW, P, L.ptr(x), L.ptr(y), L.ptr(xy), L.ptr(sc), L.ptr(patches), L.ptr(index),
                                           L.ptr(counts) if mode == "nms" else None, L.stream())
            L.check(rc, "select")
        if mode == "nms" and not torch.cuda.is_current_stream_capturing():
            for f, kept in enumerate(counts.tolist()):                                # the one read-back
                if kept < m:
                    raise RuntimeError(f"patch selection 'nms': frame {f} keeps {kept} of the {m} patches asked for")
    return Selection(x, y, xy, sc, patches, index)
