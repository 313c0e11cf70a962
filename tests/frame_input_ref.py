"""numpy fp64 restatement of devo_amd.frames.frame_input (devo/devo.py:406-467: the event-density gate, the normalisation, the
346-column crop) and of frames.probe_median (:256), written from the behaviour the functions document: test infrastructure, the yardstick
of tests/test_gpu_frame_input.py and tests/test_gpu_odometry_kernels.py, itself checked against a torch composition in
tests/test_frame_input_cpu.py.  Statistics are exact fp64 sums of the exactly converted input (math.fsum: no dependence on an order)."""
import math
import numpy as np

CROP_WIDTH = 346
GATE_DENSITY = 2e-2


def stats(x):
    """x: array [bins, H, W] of fp32 or fp16 values -> dict(nnz, numel, mean, sigma, pmax, nmax) in Python ints / floats (fp64)."""
    v = np.asarray(x).astype(np.float64).reshape(-1)
    nz = v[v != 0.0]
    nnz = int(nz.size)
    out = dict(nnz=nnz, numel=int(v.size), mean=0.0, sigma=0.0, pmax=0.0, nmax=0.0)
    if nnz:
        mean = math.fsum(nz.tolist()) / nnz
        var = math.fsum((nz * nz).tolist()) / nnz - mean * mean          # (the products of two fp32 values are exact in fp64)
        out.update(mean=mean, sigma=math.sqrt(var) if var > 0.0 else 0.0)
        if (nz > 0).any():
            out["pmax"] = float(nz[nz > 0].max())
        if (nz < 0).any():
            out["nmax"] = float(-nz[nz < 0].min())
    return out


def skipped(x):
    """The gate of devo.py:406-415 (applied by the tracker while n == 0), the reference's own expression in Python floats."""
    s = stats(x)
    return s["nnz"] / s["numel"] < GATE_DENSITY


def crop(a):
    return a[..., 1:-1] if a.shape[-1] == CROP_WIDTH else a


def frame_input(x, norm):
    """-> fp64 [1, 1, bins, H, W'] : what frames.frame_input returns, unrounded.  Under "rescale" the fp32 result is the correctly rounded
    fp32 quotient of the fp32 extrema; use rescale_f32 for the bits."""
    x = np.asarray(x)
    v = x.astype(np.float64)
    s = stats(x)
    norm = norm.lower()
    if norm == "none":
        out = v
    elif norm in ("rescale", "norm"):
        out = v.copy()
        if s["pmax"] > 0:
            out[v > 0] = v[v > 0] / s["pmax"]
        if s["nmax"] > 0:
            out[v < 0] = v[v < 0] / s["nmax"]
    elif norm in ("std", "standard"):
        if s["nnz"] == 0:
            out = v
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                out = np.where(v != 0.0, (v - s["mean"]) / s["sigma"], 0.0)      # sigma = 0 (all non-zeros equal): see events.std, not this file
    else:
        raise NotImplementedError(norm)
    return crop(out)[None, None]


def rescale_f32(x):
    """The bits of "rescale": fp32 divisions of the (exactly converted) input by the fp32 extrema."""
    v = np.asarray(x).astype(np.float32)
    s = stats(x)
    out = v.copy()
    if s["pmax"] > 0:
        out[v > 0] = v[v > 0] / np.float32(s["pmax"])
    if s["nmax"] > 0:
        out[v < 0] = v[v < 0] / np.float32(s["nmax"])
    return crop(out)[None, None]


def std_bound(x):
    """The tolerance of "std" per output voxel: 8 * 2^-24 * (|x| + |mean|) / sigma — a few fp32 roundings of a difference and a quotient whose
    statistics are exact to fp64."""
    s = stats(x)
    v = crop(np.abs(np.asarray(x).astype(np.float64)))[None, None]
    return 8.0 * 2.0 ** -24 * (v + abs(s["mean"])) / s["sigma"]


def probe_median(delta):
    """delta [..., M, 2], fp32 or fp16 -> np.float32: torch.quantile(delta.norm(dim=-1).float(), 0.5).  The norms are formed in fp64 from
    the exactly converted input and rounded to fp32 — the values `.float()` holds —, the two middle values are averaged in fp64 (the
    linear interpolation of torch.quantile at 0.5) and the mean is rounded once."""
    d = np.asarray(delta).astype(np.float64).reshape(-1, 2)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32)
    if np.isnan(r).any():
        return np.float32(np.nan)
    r = np.sort(r).astype(np.float64)
    M = r.size
    return np.float32(0.5 * (r[(M - 1) // 2] + r[M // 2]))
