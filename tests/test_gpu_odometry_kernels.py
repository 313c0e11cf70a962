"""The two small kernels of the online tracker: PatchGraph.append_frame (devo/devo.py:366-380 with both append_factors calls of :541-542
in one launch) against two PatchGraph.append calls fed the torch-built index lists, and frames.probe_median (:256) against
torch.quantile and the fp64 restatement of tests/frame_input_ref.py."""
import numpy as np
import pytest
import torch

import frame_input_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, LIFETIME, DIM = 8, 4, 16


def _flatmeshgrid(a, b):
    """devo/utils.py flatmeshgrid(..., indexing='ij')."""
    return tuple(t.reshape(-1) for t in torch.meshgrid(a, b, indexing="ij"))


def _edges_forw(n, r):
    t0, t1 = M * max(n - r, 0), M * max(n - 1, 0)
    return _flatmeshgrid(torch.arange(t0, t1, device=DEV), torch.arange(n - 1, n, device=DEV))


def _edges_back(n, r):
    t0, t1 = M * max(n - 1, 0), M * max(n, 0)
    return _flatmeshgrid(torch.arange(t0, t1, device=DEV), torch.arange(max(n - r, 0), n, device=DEV))


def _ix(frames=16):
    return torch.arange(frames, device=DEV).repeat_interleave(M)


def _prefilled(dtype):
    """A graph that already holds edges and a non-zero recurrent state."""
    from devo_amd.graph import PatchGraph
    g = PatchGraph(M, dim=DIM, capacity=4096, device=DEV, dtype=dtype)
    kk = torch.arange(0, 2 * M, device=DEV)
    g.append(kk, torch.ones_like(kk), _ix())
    gen = torch.Generator().manual_seed(3)
    g.net = torch.randn(1, len(g), DIM, generator=gen).to(DEV, dtype)
    return g


@pytest.mark.parametrize("n", [1, 2, LIFETIME, LIFETIME + 3])
@pytest.mark.parametrize("prefilled", [False, True])
def test_append_frame_equals_two_appends(n, prefilled):
    from devo_amd.graph import PatchGraph
    for dtype in (torch.float32, torch.float16):
        a, b = (_prefilled(dtype), _prefilled(dtype)) if prefilled else (PatchGraph(M, dim=DIM, capacity=4096, device=DEV, dtype=dtype) for _ in range(2))
        E0, v0 = len(a), a.ii._version
        a.append_frame(n, LIFETIME, _ix())
        b.append(*_edges_forw(n, LIFETIME), _ix())
        b.append(*_edges_back(n, LIFETIME), _ix())
        assert len(a) == len(b) == E0 + M * (n - 1 - max(n - LIFETIME, 0)) + M * (n - max(n - LIFETIME, 0))
        for name in ("ii", "jj", "kk"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, n)
        assert a.net.shape == b.net.shape == (1, len(a), DIM) and a.net.dtype == dtype and torch.equal(a.net, b.net)
        assert not a.net[:, E0:].any() and (E0 == 0 or a.net[:, :E0].any())
        assert a.ii._version > v0                                       # the version-keyed caches see the write


def test_append_frame_refuses_what_it_cannot_do():
    from devo_amd.graph import PatchGraph
    g = PatchGraph(M, dim=DIM, capacity=20, device=DEV)
    with pytest.raises(RuntimeError, match="capacity"):
        g.append_frame(2, LIFETIME, _ix())                              # 24 edges
    with pytest.raises(ValueError):
        g.append_frame(0, LIFETIME, _ix())
    assert len(g) == 0
    g.append_frame(1, LIFETIME, _ix())
    assert len(g) == M


def _delta(Mp, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(1, Mp, 2, generator=g) * 3.0
    d[0, : Mp // 3] = d[0, 0]                                            # ties
    if Mp >= 7:
        d[0, -2] = d[0, -1]
    return d.to(dtype)


@pytest.mark.parametrize("Mp", [1, 2, 7, 16, 80])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_probe_median(Mp, dtype):
    from devo_amd import frames
    d = _delta(Mp, 100 + Mp, dtype)
    got = frames.probe_median(d.to(DEV))
    assert got.shape == (1,) and got.dtype == torch.float32
    want = R.probe_median(d.float().numpy())                             # (fp16 -> fp32 is exact)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), np.array([want]).view(np.uint32)), (Mp, dtype, float(got), float(want))
    # torch's own answer on the exactly converted input: it interpolates in fp32 (two roundings) on norms it rounded itself (one more)
    q = torch.quantile(d.float().to(DEV).norm(dim=-1).float(), 0.5)
    assert abs(float(got) - float(q)) <= 3 * 2.0 ** -23 * abs(float(q)), (Mp, dtype)
    host = torch.zeros(2, dtype=torch.float32).pin_memory()              # the tracker's way: a pinned word read behind an event
    frames.probe_median(d.to(DEV), out=host)
    torch.cuda.synchronize()
    assert float(host[0]) == float(got) and float(host[1]) == 0.0


def test_probe_median_nan_and_bounds():
    from devo_amd import frames
    d = _delta(16, 5, torch.float32)
    d[0, 3, 1] = float("nan")
    assert torch.isnan(frames.probe_median(d.to(DEV))).all()             # torch.quantile: NaN if there is one
    with pytest.raises(RuntimeError, match="exceeds"):
        frames.probe_median(torch.zeros(1, frames.PROBE_MEDIAN_MAX + 1, 2, device=DEV))
    big = _delta(frames.PROBE_MEDIAN_MAX, 6, torch.float32)              # every key slot of the workgroup in use
    assert float(frames.probe_median(big.to(DEV))) == float(R.probe_median(big.numpy()))
