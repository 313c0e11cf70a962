"""Seeded coordinate cases for the lookup family (correlation lookup, its backward, the locality plan, patchify): non-finite, huge and
frame-border coordinates.  Pure CPU, torch only; shared by tests/test_corr_coord_cases_cpu.py (which pins these inputs and the oracle on
them) and tests/test_gpu_corr_coords.py (which holds the HIP kernels to the oracle on them).

A patch pixel is BAD if its x or y is non-finite, FAR if it is finite and no tap of its (2R+2)^2 window can lie in the frame (every
|v| >= 1e6 is), NEAR otherwise.  An edge whose nine pixels are all near is CLEAN."""
import math
import torch
from oracle import altcorr as A

N_FRAMES, N_PATCHES, C, H, W = 3, 24, 128, 24, 32          # level 1 at scale 4: 6 x 8

NAN, INF = float("nan"), float("inf")
HOSTILE_VALUES = (NAN, INF, -INF, 3e9, -3e9, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 1e6 + 1, -(1e6 + 1), 1e6, -1e6, 999999.5, -999999.5, 16777217.0)
PLACEMENTS = ("x of one pixel", "y of one pixel", "centre pixel", "all nine pixels", "all pixels but one")
SANITISED = -1.0e5                                          # where a bad pixel is moved to: finite and far, so it contributes nothing


def features(seed=0, channels=C, batch=1, dtype=torch.float32):
    """fmap1 [B, Np, C, 3, 3], fmap2 [B, n, C, H, W]: randn / 4"""
    g = torch.Generator().manual_seed(1000 + seed)
    f1 = torch.randn(batch, N_PATCHES, channels, 3, 3, generator=g) / 4
    f2 = torch.randn(batch, N_FRAMES, channels, H, W, generator=g) / 4
    return f1.to(dtype), f2.to(dtype)


def level1(f2):
    """the quarter-resolution level (4 x 4 means), frame by frame"""
    return torch.stack([torch.nn.functional.avg_pool2d(f2[b], 4, 4) for b in range(f2.shape[0])])


def classify(coords, R, height, width):
    """(bad, far) boolean masks [..., 3, 3] of the pixels of coords [..., 2, 3, 3] for a lookup of radius R into a height x width frame"""
    x, y = coords[..., 0, :, :], coords[..., 1, :, :]
    bad = ~(torch.isfinite(x) & torch.isfinite(y))
    fx, fy = torch.floor(x.double()), torch.floor(y.double())
    out = (fx + R + 1 < 0) | (fx - R > width - 1) | (fy + R + 1 < 0) | (fy - R > height - 1)     # window = floor - R .. floor + R + 1
    return bad, out & ~bad


def structural_zero(coords, ii, jj, R, height, width):
    """where the oracle returns exactly 0 for all-ones features: outputs [B, E, 2R+1, 2R+1, 3, 3] all of whose weighted taps lie outside
    the frame (a tap with a blend weight of exactly 0 does not count)"""
    B = coords.shape[0]
    one1 = torch.ones(B, int(ii.max()) + 1, 1, 3, 3)
    one2 = torch.ones(B, int(jj.max()) + 1, 1, height, width)
    return A.corr_forward(one1, one2, coords, ii, jj, R) == 0


def _clean_edges(g, E):
    """in-frame centres, compact 3 x 3 offsets (0.6 - 1.5 px apart) plus jitter: [E, 2, 3, 3]"""
    base = torch.stack([0.5 + torch.rand(E, generator=g) * (W - 2.0), 0.5 + torch.rand(E, generator=g) * (H - 2.0)], 1)
    oy, ox = torch.meshgrid(torch.arange(3.) - 1, torch.arange(3.) - 1, indexing="ij")
    off = torch.stack([ox, oy], 0)
    scale = 0.6 + 0.9 * torch.rand(E, 1, 1, 1, generator=g)
    return base[:, :, None, None] + scale * off[None] + 0.2 * torch.randn(E, 2, 3, 3, generator=g)


def hostile(seed=0):
    """160 edges: 80 clean ones (one of them exactly integer) and, interleaved with them in a seeded order, every value of HOSTILE_VALUES
    written into a clean edge in every placement of PLACEMENTS.

    Returns a dict: coords [1, E, 2, 3, 3]; benign (every dirty edge restored to its clean original); sanitised (every bad pixel moved to
    -1e5); bad_pixel [E, 3, 3]; clean_edge [E]; ii (patches 0..11 are used by edges without a bad pixel only); jj (the last frame has no
    edge); value / placement (index into HOSTILE_VALUES / PLACEMENTS per edge, -1 for clean edges)."""
    g = torch.Generator().manual_seed(seed)
    nd = len(HOSTILE_VALUES) * len(PLACEMENTS)
    E = 2 * nd
    benign = _clean_edges(g, E)
    benign[0] = benign[0].round()                                   # dx = dy = 0
    coords = benign.clone()
    value = torch.full((E,), -1, dtype=torch.long)
    placement = torch.full((E,), -1, dtype=torch.long)
    others = (0, 1, 2, 3, 5, 6, 7, 8)                               # the non-centre pixels
    k = 0
    for vi, v in enumerate(HOSTILE_VALUES):
        for pl in range(len(PLACEMENTS)):
            e = nd + k
            c = coords[e].view(2, 9)
            p = others[k % 8]
            if pl == 0:
                c[0, p] = v
            elif pl == 1:
                c[1, p] = v
            elif pl == 2:
                c[:, 4] = v
            elif pl == 3:
                c[:, :] = v
            else:
                keep = c[:, p].clone()
                c[:, :] = v
                c[:, p] = keep
            value[e], placement[e] = vi, pl
            k += 1
    perm = torch.randperm(E, generator=g)
    perm = torch.cat([perm[perm == 0], perm[perm != 0]])            # (the integer edge stays edge 0)
    coords, benign, value, placement = coords[perm], benign[perm], value[perm], placement[perm]
    bad_pixel = ~(torch.isfinite(coords[:, 0]) & torch.isfinite(coords[:, 1]))
    clean_edge = value < 0
    has_bad = bad_pixel.flatten(1).any(1)
    half = N_PATCHES // 2
    ii = torch.where(has_bad, half + torch.randint(0, half, (E,), generator=g), torch.randint(0, N_PATCHES, (E,), generator=g))
    ii[:half] = torch.where(has_bad[:half], ii[:half], torch.arange(half))       # (every patch of the first half is in use)
    jj = torch.randint(0, N_FRAMES - 1, (E,), generator=g)
    sanitised = coords.clone()
    sanitised[bad_pixel[:, None].expand(E, 2, 3, 3)] = SANITISED
    return dict(coords=coords[None].contiguous(), benign=benign[None].contiguous(), sanitised=sanitised[None].contiguous(),
                bad_pixel=bad_pixel, clean_edge=clean_edge, ii=ii, jj=jj, value=value, placement=placement)


def tiled(case, times):
    """`case` (hostile's dict) repeated `times` times along the edge axis (the multi-workgroup plan ordering from 2048 edges on, the cached
    channels-last copy of the backward from 1024)"""
    out = {}
    for k, v in case.items():
        out[k] = torch.cat([v] * times, 1 if v.dim() == 5 else 0)
    return out


def _up(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(INF)))


def _down(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(-INF)))


TINY = float(torch.finfo(torch.float32).tiny)              # "epsilon" next to 0: the smallest normal (denormals may be flushed: not a border)


def sweep_values(R, size):
    """patch-centre coordinates along an axis of `size` positions: every value at which floor(v) - R, the window's end floor(v) + R + 1 or the
    blend fraction v - floor(v) changes class at the frame's two borders (fp32 neighbours: nextafter).  -1e-7 has the fp32 fraction
    0.99999988, the largest but one below 1; -1e-8 has the fp32 fraction EXACTLY 1.0 (1 - 1e-8 rounds up): all weight on the tap at +1"""
    s = float(size)
    return [-R - 2.0, -R - 1.0, _up(-R - 1.0), -float(R), _down(-1.0), -1.0, -1e-7, -1e-8, -0.0, 0.0, TINY,
            _down(s - 1), s - 1, _up(s - 1), s, s + R - 1, s + R, _up(s + R), s + R + 1]


def border(seed=0, R=3):
    """About 110 edges: an integer-offset 3 x 3 patch and the same patch shifted by 0.5, the centre swept along x (y mid-frame), along y (x
    mid-frame), and along the diagonal through each of the four corners.

    Returns a dict: coords [1, E, 2, 3, 3]; ii; jj; zero0 / zero1: the structural-zero masks of a radius-R lookup with coords into the
    H x W level and with coords / 4 into the H/4 x W/4 level; sweep_x / sweep_y: the values swept."""
    g = torch.Generator().manual_seed(100 + seed)
    sx, sy = sweep_values(R, W), sweep_values(R, H)
    centres = [(v, H // 2) for v in sx] + [(W // 2, v) for v in sy]
    lo = lambda: [-R - 1.0, -float(R), -1.0, -1e-8, 0.0]
    hi = lambda s: [s - 1.0, _up(s - 1.0), float(s), s + R - 1.0, float(s + R)]
    for xs, ys in ((lo(), lo()), (hi(W), lo()), (lo(), hi(H)), (hi(W), hi(H))):
        centres += list(zip(xs, ys))
    ctr = torch.tensor(centres, dtype=torch.float32)               # [K, 2]
    oy, ox = torch.meshgrid(torch.arange(3.) - 1, torch.arange(3.) - 1, indexing="ij")
    off = torch.stack([ox, oy], 0)
    whole = ctr[:, :, None, None] + off[None]
    coords = torch.cat([whole, whole + 0.5], 0)
    coords[:len(ctr), :, 1, 1] = ctr                                # (the centre pixel carries the swept value itself)
    E = coords.shape[0]
    ii = torch.randint(0, N_PATCHES, (E,), generator=g)
    jj = torch.randint(0, N_FRAMES - 1, (E,), generator=g)
    coords = coords[None].contiguous()
    return dict(coords=coords, ii=ii, jj=jj, zero0=structural_zero(coords, ii, jj, R, H, W),
                zero1=structural_zero(coords / 4, ii, jj, R, H // 4, W // 4), sweep_x=sx, sweep_y=sy)


def wide_dead(seed=0):
    """16 edges: 4 clean ones and 12 whose box misses the frame on one side while it is millions of positions wide along the other axis —
    eight pixels 50 positions above / below / left of / right of the frame, the ninth there too but with -1e6, 1e6 + 1 or NaN as its other
    coordinate: no tap of any pixel lies in the frame (every pixel far or bad), the box has no position in the frame and an enormous extent.

    Returns a dict: coords [1, E, 2, 3, 3]; ii; jj; clean_edge [E]."""
    g = torch.Generator().manual_seed(300 + seed)
    clean = _clean_edges(g, 4)
    dead = _clean_edges(g, 12)
    k = 0
    for v in (-1e6, 1e6 + 1, NAN):
        for axis, where in ((1, -50.0), (1, H + 50.0), (0, -50.0), (0, W + 50.0)):
            c = dead[k]
            c[axis] = where + (c[axis] - c[axis, 1, 1])            # the whole patch beyond the frame along `axis`
            c.view(2, 9)[1 - axis, (2 * k + 1) % 9] = v             # one pixel's other coordinate
            k += 1
    coords = torch.cat([clean[:2], dead[:6], clean[2:], dead[6:]])
    clean_edge = torch.zeros(16, dtype=torch.bool)
    clean_edge[[0, 1, 8, 9]] = True
    ii = torch.randint(0, N_PATCHES, (16,), generator=g)
    jj = torch.randint(0, N_FRAMES - 1, (16,), generator=g)
    return dict(coords=coords[None].contiguous(), ii=ii, jj=jj, clean_edge=clean_edge)


def patch_centres(seed=0, M=40, height=12, width=16, batch=2):
    """patchify centres [B, M, 2]: in-frame ones, border ones and every value of HOSTILE_VALUES as x, as y or as both"""
    g = torch.Generator().manual_seed(200 + seed)
    c = torch.stack([torch.rand(batch, M, generator=g) * (width + 6) - 3, torch.rand(batch, M, generator=g) * (height + 6) - 3], -1)
    c[:, :4] = c[:, :4].floor()
    for k, v in enumerate(HOSTILE_VALUES):
        c[0, 4 + k, k % 2] = v                                      # one coordinate
        c[1, 4 + k, :] = v                                          # both
    c[0, 20], c[0, 21], c[0, 22], c[0, 23] = torch.tensor([-1e-7, -1e-7]), torch.tensor([-1.0, height - 1.0]), torch.tensor([width - 1.0, 0.0]), torch.tensor([float(width), float(height)])
    return c


def is_nan_or_zero(t):
    return torch.isnan(t) | (t == 0)


assert math.isnan(HOSTILE_VALUES[0])
