"""The input path of the online tracker without a GPU: tests/frame_input_ref.py (numpy) agrees with the reference's own lines
(devo/devo.py:406-467) composed in torch fp64 on CPU, the new symbols are declared in the header, the ctypes table and the binding with the
ABI version still 9, and the modules refuse what they cannot run.  The first three tests validate the yardstick itself (one helper against
an independent composition): they say nothing about the package and pass without it; the last two need the new symbols and modules.  The
package's own kernels are held to this yardstick in tests/test_gpu_frame_input.py and tests/test_gpu_odometry_kernels.py."""
import os
import re
import numpy as np
import pytest
import torch

import frame_input_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("devo_odom_input", "devo_odom_input_workspace_bytes", "devo_odom_probe_median", "devo_odom_append_frame", "devo_odom_append_frame_edges")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _grid(shape, density, seed, sign=0):
    g = np.random.default_rng(seed)
    v = g.standard_normal(shape).astype(np.float32) * 1.5
    if sign:
        v = np.abs(v) * sign
    v[g.random(shape) >= density] = 0.0
    return v


def _torch_composition(x, norm):
    """devo.py:417-467 as written there, on a float64 CPU tensor (so the comparison is not limited by fp32)."""
    image = torch.from_numpy(np.asarray(x)).double()[None, None].clone()
    b, n, v, h, w = image.shape
    flat = image.view(b, n, -1)
    if norm == "none":
        pass
    elif norm == "rescale":
        pos, neg = flat > 0.0, flat < 0.0
        vx_max = torch.tensor([1.0], dtype=torch.float64) if pos.sum().item() == 0 else flat[pos].max(dim=-1, keepdim=True)[0]
        vx_min = torch.tensor([1.0], dtype=torch.float64) if neg.sum().item() == 0 else flat[neg].min(dim=-1, keepdim=True)[0]
        assert vx_min.item() != 0.0 and vx_max.item() != 0.0             # the "empty voxel" return of :432-435 cannot be reached
        flat[pos] = flat[pos] / vx_max
        flat[neg] = flat[neg] / -vx_min
    else:
        nonzero = flat != 0.0
        num = nonzero.sum(dim=-1)
        if torch.all(num > 0):
            mean = torch.sum(flat, dim=-1) / num
            std = torch.sqrt(torch.sum(flat ** 2, dim=-1) / num - mean ** 2)
            flat = nonzero.type_as(flat) * (flat - mean[..., None]) / std[..., None]
    image = flat.view(b, n, v, h, w)
    if image.shape[-1] == 346:
        image = image[..., 1:-1]
    return image.numpy()


CASES = [((5, 16, 25), 0.3, 1, 0), ((5, 37, 53), 0.3, 2, 0), ((5, 20, 346), 0.25, 3, 0), ((5, 9, 11), 0.5, 4, 1), ((5, 9, 11), 0.5, 5, -1)]


@pytest.mark.parametrize("norm", ["none", "rescale", "std"])
def test_restatement_agrees_with_the_reference_lines_in_torch(norm):
    for shape, density, seed, sign in CASES:
        x = _grid(shape, density, seed, sign)
        got, want = R.frame_input(x, norm), _torch_composition(x, norm)
        assert got.shape == want.shape == (1, 1, shape[0], shape[1], shape[2] - 2 if shape[2] == 346 else shape[2])
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (shape, norm)


def test_restatement_of_the_gate_and_the_empty_grid():
    x = np.zeros((5, 16, 25), np.float32)
    x.reshape(-1)[:40] = 1.0                                              # 40 of 2000: exactly 0.02, not below it
    assert R.stats(x)["nnz"] == 40 and R.stats(x)["numel"] == 2000 and not R.skipped(x)
    x.reshape(-1)[39] = 0.0
    assert R.stats(x)["nnz"] == 39 and R.skipped(x)
    z = np.zeros((5, 4, 6), np.float32)
    for norm in ("none", "rescale", "std"):
        assert not R.frame_input(z, norm).any()                          # no non-zero voxel: returned as it is
    assert np.array_equal(R.rescale_f32(_grid((5, 8, 9), 0.5, 7, 1)), R.frame_input(_grid((5, 8, 9), 0.5, 7, 1), "rescale").astype(np.float32))


def test_restatement_of_the_probe_median_is_torch_quantile():
    g = torch.Generator().manual_seed(11)
    for M in (1, 2, 7, 16, 80):
        d = torch.randn(1, M, 2, generator=g)
        d[0, : M // 3] = d[0, 0]                                          # ties
        want = torch.quantile(d.double().norm(dim=-1).float(), 0.5)
        got = R.probe_median(d.numpy())
        assert abs(float(got) - float(want)) <= 2.0 ** -22 * float(want), M     # torch interpolates in fp32: hi - (hi - lo) / 2, two roundings
    assert np.isnan(R.probe_median(np.array([[1.0, 2.0], [np.nan, 0.0]], np.float32)))


def test_symbols_are_declared_in_header_ctypes_table_and_binding_with_abi_9():
    from devo_amd import _lib, build
    header, bind = _read("include", "devo_hip.h"), _read("devo_amd", "csrc", "bind.cpp")
    assert re.search(r"#define DEVO_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9
    version_comment = header.split("int devo_abi_version")[0]
    for s in SYMBOLS:
        assert s in version_comment, s
        assert re.search(r"\b" + s + r"\(", header.split("int devo_abi_version")[1]), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\(", bind), s
    assert "frame_input.hip" in build.SOURCES
    h = _lib.lib()
    assert h.devo_odom_append_frame_edges(8, 1, 4) == 8 and h.devo_odom_append_frame_edges(8, 2, 4) == 24 and h.devo_odom_append_frame_edges(8, 7, 4) == 56
    assert h.devo_odom_append_frame_edges(8, 0, 4) == 0 and h.devo_odom_input_workspace_bytes(5 * 480 * 640) > 0
    # refused on the host, before any launch
    assert h.devo_odom_input(None, 0, 5, 4, 4, 2, None, None, 0, None, None) == 1
    assert h.devo_odom_probe_median(None, 0, 4, None, None) == 1
    assert h.devo_odom_append_frame(None, None, None, None, None, None, 0, 8, 0, 4, 0, 100, 8, 0, None) == 1


def test_the_modules_refuse_cpu_tensors_and_bad_arguments():
    from devo_amd import frames, graph, odometry
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.frame_input(torch.zeros(5, 4, 4), "std")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.probe_median(torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        graph.PatchGraph(8, dim=8, capacity=64, device="cpu").append_frame(1, 4, torch.zeros(16, dtype=torch.long))
    cfg = odometry.Config()
    assert (cfg.BUFFER_SIZE, cfg.PATCH_SELECTOR, cfg.SCORER_EVAL_MODE, cfg.SCORER_EVAL_USE_GRID, cfg.NORM) == (4096, "scorer", "multi", True, "std")
    assert (cfg.PATCHES_PER_FRAME, cfg.REMOVAL_WINDOW, cfg.OPTIMIZATION_WINDOW, cfg.PATCH_LIFETIME) == (80, 20, 12, 12)
    assert (cfg.KEYFRAME_INDEX, cfg.KEYFRAME_THRESH, cfg.MOTION_MODEL, cfg.MOTION_DAMPING, cfg.MIXED_PRECISION) == (4, 12.5, "DAMPED_LINEAR", 0.5, True)
    assert odometry.Config(NORM="none", PATCHES_PER_FRAME=16).PATCHES_PER_FRAME == 16
    with pytest.raises(AttributeError):
        odometry.Config(PATCHES=3)
