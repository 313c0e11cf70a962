"""Plain torch-CPU restatement of devo_amd.select.select (the four modes of the reference's PatchSelector, devo/selector.py:50-287, and the tail of
devo/enet.py:100-200 behind them), written for clarity: it materialises the padding, unfolds every cell, ranks with a stable sort and runs the
non-maximum suppression one box at a time.  It takes the same `noise` / `candidates` as the kernel, forms the `multi` keys with the same fp32
operations (one add, one division) and ranks with the same rule: the higher key first, on equal keys the lower flat cell index."""
from collections import namedtuple

import torch
import torch.nn.functional as F

Selection = namedtuple("Selection", ("x", "y", "xy", "scores", "patches", "index"))
EPS = 1e-7
TINY = 1.17549435e-38            # FLT_MIN: what a noise value <= 0 counts as


def _first_argmax(v, dim):
    """index of the FIRST maximum along dim (torch.max leaves the choice among equal maxima open)"""
    best = v.max(dim=dim, keepdim=True).values
    shape = [1] * v.dim()
    shape[dim] = v.shape[dim]
    pos = torch.arange(v.shape[dim]).view(shape).expand_as(v)
    return torch.where(v == best, pos, torch.full_like(pos, v.shape[dim])).min(dim=dim).values


def _rank(keys):
    """[n, L] -> the indices in decreasing key, equal keys in increasing index"""
    return torch.sort(keys, dim=-1, descending=True, stable=True).indices


def _quadrants(t):
    """[n, h1, w1] -> [n, 4, h2 w2], quadrant-local row-major (selector.py:59-70)"""
    n, h1, w1 = t.shape
    h2, w2 = h1 // 2, w1 // 2
    return t.reshape(n, 2, h2, 2, w2).permute(0, 1, 3, 2, 4).reshape(n, 4, h2 * w2)


def _cells_of_quadrant_picks(idx, h1, w1):
    """idx [n, m/4, 4] quadrant-local -> cx, cy [n, m] in the reference's k-major, quadrant-minor order (_grid2_coords_up)"""
    h2, w2 = h1 // 2, w1 // 2
    q = torch.arange(4)
    cx = idx % w2 + (q % 2) * w2
    cy = idx // w2 + (q // 2) * h2
    return cx.flatten(1), cy.flatten(1)


def _pick_cells(keys, m, grid):
    """keys [n, h1, w1] -> cx, cy [n, m]"""
    n, h1, w1 = keys.shape
    if grid:
        idx = _rank(_quadrants(keys))[..., :m // 4].transpose(1, 2)
        return _cells_of_quadrant_picks(idx, h1, w1)
    idx = _rank(keys.reshape(n, -1))[:, :m]
    return idx % w1, idx // w1


def _nms_frame(best, px, py, h1, w1, grid):
    """greedy suppression of one frame, one box at a time -> the surviving cells in decreasing score"""
    x1 = (px.float() - 1.5).clamp(min=0.0)
    y1 = (py.float() - 1.5).clamp(min=0.0)
    cat = torch.zeros_like(px)
    if grid:
        cat = (~(x1 < w1 / 2)).long() + 2 * (~(y1 < h1 / 2)).long()     # pixels against half the POOLED size, as the reference writes it
    kept = []
    for c in _rank(best[None])[0].tolist():
        ok = True
        for q in kept:
            if int(cat[q]) != int(cat[c]):
                continue
            iw = max(min(float(x1[q]), float(x1[c])) + 3.0 - max(float(x1[q]), float(x1[c])), 0.0)
            ih = max(min(float(y1[q]), float(y1[c])) + 3.0 - max(float(y1[q]), float(y1[c])), 0.0)
            inter = iw * ih
            if inter / (18.0 - inter) > 0.4:
                ok = False
                break
        if ok:
            kept.append(c)
    return kept


def _pad(scores, grid, k, pad=True):
    h, w = scores.shape[-2:]
    f = 2 * k if grid else k
    ph, pw = ((f - h % f) % f, (f - w % f) % f) if pad else (0, 0)
    top, left = ph // 2, pw // 2
    return F.pad(scores, (left, pw - left, top, ph - top)), top, left          # (the odd pixel goes to the bottom / right)


def _nms(padded, grid, k):
    """-> the offset of every cell's maximum [n, C] and, per frame, the surviving cells in decreasing score"""
    n, hp, wp = padded.shape
    h1, w1 = hp // k, wp // k
    cells = F.unfold(padded[:, None], kernel_size=k, stride=k)
    best, off = cells.max(dim=1).values, _first_argmax(cells, 1)
    cell = torch.arange(h1 * w1)
    px, py = k * (cell % w1) + off % k, k * (cell // w1) + off // k
    return off, [_nms_frame(best[fr], px[fr], py[fr], h1, w1, grid) for fr in range(n)]


def nms_survivors(scores, grid=True, k=4):
    """how many boxes every frame keeps: the largest m that 'nms' can deliver for this map"""
    scores = scores.detach().cpu().float()
    return [len(kept) for kept in _nms(_pad(scores[0] if scores.dim() == 4 else scores, grid, k)[0], grid, k)[1]]


def select_ref(scores, m, mode, grid=True, k=4, *, noise=None, candidates=None, offset=0, clamp=None, disps=None, P=3, pad=True):
    scores = scores.detach().cpu().float()
    if scores.dim() == 4:
        scores = scores[0]
    n, h, w = scores.shape
    padded, top, left = _pad(scores, grid, k, pad)
    hp, wp = padded.shape[-2:]
    h1, w1 = hp // k, wp // k
    C = h1 * w1
    rows = torch.arange(n)[:, None]
    picked = None
    if mode == "3xrandom":
        cx, cy = (c.cpu() for c in candidates)
        s = padded[rows, cy, cx]
        order = torch.sort(s, dim=1, stable=True).indices[:, -m:]
        xp, yp = torch.gather(cx, 1, order) + 1, torch.gather(cy, 1, order) + 1
        picked = torch.gather(s, 1, order)
    else:
        cells = F.unfold(padded[:, None], kernel_size=k, stride=k)              # [n, k k, C], row-major inside a cell
        best = cells.max(dim=1).values
        off = _first_argmax(cells, 1)
        if mode == "topk":
            cx, cy = _pick_cells(best.reshape(n, h1, w1), m, grid)
            o = torch.gather(off, 1, cy * w1 + cx)
        elif mode == "multi":
            nz = noise.detach().cpu().float()
            nz = torch.where(nz > 0, nz, torch.full_like(nz, TINY))
            total = cells[:, 0]
            for j in range(1, k * k):
                total = total + cells[:, j]
            mean = total * (1.0 / (k * k))
            keys = ((mean + EPS) if grid else mean) / nz[:, :C]
            cx, cy = _pick_cells(keys.reshape(n, h1, w1), m, grid)
            win = F.unfold(padded[:, None], kernel_size=k, stride=k, padding=1).transpose(1, 2)    # [n, C, k k]: one pixel up-left of the cell
            pick = torch.gather(win, 1, (cy * w1 + cx)[..., None].expand(-1, -1, k * k))
            o = _first_argmax((pick + EPS) / nz[:, C:].reshape(n, m, k * k), 2)
        else:
            cx, cy, o = (torch.empty(n, m, dtype=torch.long) for _ in range(3))
            off, survivors = _nms(padded, grid, k)
            for fr, kept in enumerate(survivors):
                if len(kept) < m:
                    raise RuntimeError(f"patch selection 'nms': frame {fr} keeps {len(kept)} of the {m} patches asked for")
                kept = torch.tensor(kept[:m])
                cx[fr], cy[fr], o[fr] = kept % w1, kept // w1, off[fr, kept]
        xp, yp = k * cx + o % k, k * cy + o // k
    x, y = xp - left, yp - top
    if pad:
        x, y = x.clamp(min=0, max=w - 1), y.clamp(min=0, max=h - 1)
    if picked is None:
        picked = scores[rows, y, x]
    x, y = x + offset, y + offset
    if clamp is not None:
        x, y = x.clamp(*clamp[0]), y.clamp(*clamp[1])
    xy = torch.stack([x, y], dim=-1).float()
    r = P // 2
    d = torch.arange(-r, r + 1)
    X = (x[..., None, None] + d[None, None, None, :]).expand(n, m, P, P)
    Y = (y[..., None, None] + d[None, None, :, None]).expand(n, m, P, P)
    if disps is None:
        px, py, pd = X.float(), Y.float(), torch.ones(n, m, P, P)
    else:
        dm = disps.detach().cpu().float()
        dm = dm[0] if dm.dim() == 4 else dm
        H, W = dm.shape[-2:]
        inside = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
        pd = dm[torch.arange(n)[:, None, None, None], Y.clamp(0, H - 1), X.clamp(0, W - 1)] * inside
        px, py = X.float() * inside, Y.float() * inside
    patches = torch.stack([px, py, pd], dim=2).reshape(n * m, 3, P, P)
    index = torch.arange(n).view(n, 1).repeat(1, m).reshape(-1)
    return Selection(x, y, xy, picked, patches, index)
