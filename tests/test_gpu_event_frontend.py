"""GPU parity of the event front end (devo_amd/events.py: voxel_grids, remove_hot_pixels / RemoveHotPixelsVoxel, rescale,
real_data_voxels; csrc/events.hip through the C ABI) against the reference-generated golden (tests/golden/event_frontend.npz:
EventSlicer + get_real_data_list + RemoveHotPixelsVoxel + rescale of the reference, tools/gen_golden_event_frontend.py) and an fp64
torch restatement of the loaders' per-window formulation.  Votes are added with fp32 atomics in another order than the
reference's index_add_ passes: grids agree to fp32 rounding (1e-5 of the scale); the SET of zeroed hot voxels must match exactly
(the generator keeps every voxel 1e-4 away from its threshold)."""
import os
import numpy as np
import pytest
import torch
from util import assert_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = ("tumvie", "eds")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "event_frontend.npz"))


def _case(z, tag):
    g = lambda k: z[f"{tag}/{k}"]
    H, W = g("rmap").shape[:2]
    ev = dict(x=torch.from_numpy(g("x").astype(np.int32)).to(DEV), y=torch.from_numpy(g("y").astype(np.int32)).to(DEV),
              ts=torch.from_numpy(g("t") + int(g("t_offset"))).to(DEV), p=torch.from_numpy(g("p")).to(DEV),
              xf=torch.from_numpy(g("xf")).to(DEV), yf=torch.from_numpy(g("yf")).to(DEV), rmap=torch.from_numpy(g("rmap")).to(DEV))
    tss, dT = g("tss"), float(g("dT_ms"))
    return g, H, W, ev, tss, tss + dT * 1e3


def _zeroed(hot, raw):
    """Indices of the voxels the filter zeroed (a raw sum that cancels to zero in one summation order only is not one of them)."""
    return torch.nonzero((hot == 0) & (raw.abs() > 1e-4 * raw.abs().max())).cpu()


def _with_hot_zeroed(raw, inds):
    out = raw.clone()
    i = torch.from_numpy(inds).long()
    out[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = 0
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_windows_match_reference_golden(gold, tag):
    """Per-window grids with the rectify map and without (fractional coordinates), with and without the hot-pixel filter
    (k = 6 / 10); timestamps as int64 microseconds and as float64."""
    from devo_amd import events
    g, H, W, ev, t0, t1 = _case(gold, tag)
    k = float(g("k"))
    idx = torch.from_numpy(g("list_idx")).long()
    for ts in (ev["ts"], ev["ts"].double()):
        raw, cnt = events.voxel_grids(ev["x"], ev["y"], ts, ev["p"], t0, t1, H, W, rectify_map=ev["rmap"])
        assert raw.shape == (len(t0), 5, H, W) and raw.dtype == torch.float32 and cnt.dtype == torch.int64 and raw.is_cuda and cnt.is_cuda
        ref = torch.from_numpy(g("list_raw"))
        assert_rel(raw[idx.to(DEV)], ref, 1e-5, f"{tag} rectified windows")
        cnt = cnt.cpu()
        assert bool((cnt[idx] > 0).all()) and int(cnt[7]) == 0 and float(raw[7].abs().sum()) == 0.0     # window 7 lies in the gap
        hot, _ = events.voxel_grids(ev["x"], ev["y"], ts, ev["p"], t0, t1, H, W, rectify_map=ev["rmap"], hot_pixel_stds=k)
        assert_rel(hot[idx.to(DEV)], _with_hot_zeroed(ref, g("list_hot")), 1e-5, f"{tag} rectified windows, hot pixels removed")
        assert torch.equal(_zeroed(hot[idx.to(DEV)], raw[idx.to(DEV)]), torch.from_numpy(g("list_hot")).long())
    nidx = torch.from_numpy(g("nomap_idx")).long().to(DEV)
    raw, _ = events.voxel_grids(ev["xf"], ev["yf"], ev["ts"], ev["p"], t0, t1, H, W)
    ref = torch.from_numpy(g("nomap_raw"))
    assert_rel(raw[nidx], ref, 1e-5, f"{tag} unrectified windows")
    hot, _ = events.voxel_grids(ev["xf"], ev["yf"], ev["ts"], ev["p"], t0, t1, H, W, hot_pixel_stds=k)
    assert_rel(hot[nidx], _with_hot_zeroed(ref, g("nomap_hot")), 1e-5, f"{tag} unrectified windows, hot pixels removed")
    assert torch.equal(_zeroed(hot[nidx], raw[nidx]), torch.from_numpy(g("nomap_hot")).long())
    # the filter on its own, and as the loaders' transform, on the reference's own raw grids
    assert torch.equal(_zeroed(events.remove_hot_pixels(ref.to(DEV), k), ref.to(DEV)), torch.from_numpy(g("nomap_hot")).long())
    one = events.RemoveHotPixelsVoxel(num_stds=k)(ref[0].to(DEV))
    assert one.shape == ref[0].shape and torch.equal(one.cpu(), _with_hot_zeroed(ref[:1], g("nomap_hot")[g("nomap_hot")[:, 0] == 0])[0])


@pytest.mark.parametrize("tag", TAGS)
def test_real_data_voxels_matches_get_real_data_list(gold, tag):
    from devo_amd import events
    g, H, W, ev, t0, _ = _case(gold, tag)
    intr = [float(v) for v in g("intrinsics")]
    ref = _with_hot_zeroed(torch.from_numpy(g("list_raw")), g("list_hot"))
    got = list(events.real_data_voxels(ev["x"], ev["y"], ev["ts"], ev["p"], list(t0), float(g("dT_ms")), intr, ev["rmap"], H, W,
                                       float(g("k")), chunk=4, ms_index_len=len(g("ms_to_idx")), t_offset=int(g("t_offset"))))
    assert len(got) == len(ref)
    assert [m for _, _, m in got] == list(g("list_mid"))                      # the same windows in the same order, timestamps exact
    for j, (vox, K, _) in enumerate(got):
        assert vox.shape == (5, H, W) and vox.is_cuda
        assert torch.equal(K, torch.as_tensor(intr))
        assert_rel(vox, ref[j], 1e-5, f"{tag} real_data_voxels window {j}")
    # without the ms index every window with events is served, the one past the recording's index included
    more = list(events.real_data_voxels(ev["x"], ev["y"], ev["ts"], ev["p"], t0, float(g("dT_ms")), intr, ev["rmap"], H, W, float(g("k"))))
    assert len(more) == len(ref) + 1 and [m for _, _, m in more[:-1]] == list(g("list_mid"))


@pytest.mark.parametrize("tag", TAGS)
def test_rescale_matches_reference(gold, tag):
    from devo_amd import events
    g = lambda k: gold[f"{tag}/{k}"]
    vox = _with_hot_zeroed(torch.from_numpy(g("list_raw")), g("list_hot"))[None, :3].contiguous().to(DEV)    # the golden's sequence
    ref = torch.from_numpy(g("rescale"))[None]
    for seq in (True, False):
        out = events.rescale(vox, sequence=seq)
        assert out.shape == vox.shape
        assert_rel(out, ref, 1e-6, f"{tag} rescale sequence={seq}")
    assert float(out.max()) == 1.0 and float(out.min()) == -1.0
    two = torch.stack([vox[0], 0.5 * vox[0]])                                  # b = 2: the extremes are still global
    assert torch.equal(events.rescale(two, True)[0].cpu(), events.rescale(vox, True)[0].cpu())


def _restate(x, y, t, p, t0, t1, H, W, bins=5, rmap=None):
    """fp64 restatement of the loaders' per-window voxelisation (EventSlicer window, rectify_map[y, x], to_voxel_grid)."""
    t0, t1 = torch.as_tensor(t0, dtype=torch.float64), torch.as_tensor(t1, dtype=torch.float64)
    tt = t.double()
    out = torch.zeros(len(t0), bins, H, W, dtype=torch.float64, device=t.device)
    lo = torch.searchsorted(tt, t0.to(t.device)).tolist()
    hi = torch.searchsorted(tt, t1.to(t.device)).tolist()
    for s, (a, b) in enumerate(zip(lo, hi)):
        if b <= a:
            continue
        xs, ys = x[a:b], y[a:b]
        if rmap is not None:
            r = rmap[ys.long(), xs.long()].double()
            xs, ys = r[:, 0], r[:, 1]
        xs, ys = xs.double(), ys.double()
        tn = (tt[a:b] - tt[a]) * (bins - 1) / (tt[b - 1] - tt[a])
        pol = torch.where(p[a:b] == 0, -1.0, p[a:b].double())
        flat = out[s].view(-1)
        for lx in (xs.floor(), xs.floor() + 1):
            for ly in (ys.floor(), ys.floor() + 1):
                for lt in (tn.floor(), tn.floor() + 1):
                    m = (lx >= 0) & (ly >= 0) & (lt >= 0) & (lx <= W - 1) & (ly <= H - 1) & (lt <= bins - 1)
                    w = pol * (1 - (lx - xs).abs()) * (1 - (ly - ys).abs()) * (1 - (lt - tn).abs())
                    flat.index_add_(0, (lx.long() + ly.long() * W + lt.long() * W * H)[m], w[m])
    return out


def _hot_restated(g, k):
    v = g.double().flatten(1)
    thr = v.mean(1) + k * v.std(1)
    return torch.where(v.abs() > thr[:, None], 0.0, v).view(g.shape)


def test_large_stream_against_fp64_restatement():
    from devo_amd import events
    gen = torch.Generator().manual_seed(11)
    N, S, H, W = 2_000_000, 200, 120, 160
    ts = torch.sort(torch.randint(0, 2_000_000, (N,), generator=gen)).values + 1_500_000_000_000
    x, y = torch.randint(0, W, (N,), generator=gen), torch.randint(0, H, (N,), generator=gen)
    p = torch.randint(0, 2, (N,), generator=gen).to(torch.uint8)
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rmap = torch.stack([gx * 0.97 + 2.1 + 0.6 * torch.sin(gy / 11), gy * 1.02 - 1.3 + 0.4 * torch.cos(gx / 5)], -1)
    t0 = (torch.rand(S, generator=gen, dtype=torch.float64) * 2.1e6 - 0.05e6 + 1.5e12).sort().values   # some start before / after the stream
    t1 = t0 + torch.rand(S, generator=gen, dtype=torch.float64) * 4e4 + 1.0                             # overlapping, of varied length
    d = lambda a: a.to(DEV)
    grids, cnt = events.voxel_grids(d(x), d(y), d(ts), d(p), d(t0), d(t1), H, W, rectify_map=d(rmap))
    ref = _restate(d(x), d(y), d(ts), d(p), t0, t1, H, W, rmap=d(rmap))
    assert_rel(grids, ref, 1e-5, "2 M events, 200 windows")
    for s in range(S):
        if float(ref[s].abs().max()) > 0:
            assert_rel(grids[s], ref[s], 1e-5, f"window {s}")
        else:
            assert float(grids[s].abs().max()) == 0.0
    lo, hi = torch.searchsorted(ts.double(), t0), torch.searchsorted(ts.double(), t1)
    assert torch.equal(cnt.cpu(), hi - lo) and int((cnt == 0).sum()) > 0
    hot = events.remove_hot_pixels(grids, 6)                                 # on these very grids: the same set as fp64 statistics give
    assert torch.equal(hot == 0, _hot_restated(grids, 6) == 0) and int(((hot == 0) & (grids != 0)).sum()) > 0
    assert torch.equal(hot, torch.where(hot == 0, 0.0, grids))


def test_edge_cases():
    from devo_amd import events
    e = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
    H, W = 6, 7
    # an empty stream: every window empty
    g, c = events.voxel_grids(e([], torch.float32), e([], torch.float32), e([], torch.int64), e([], torch.int8), [0.0, 5.0], [1.0, 9.0], H, W)
    assert g.shape == (2, 5, H, W) and float(g.abs().sum()) == 0.0 and c.tolist() == [0, 0]
    # windows: before the stream, empty between events, a single event, overlapping, touching, t1 < t0, after the stream, all
    x = e([1.5, 2.25, 3.0, 4.75, 0.5, 5.5, 2.0], torch.float32)
    y = e([1.0, 2.5, 3.25, 0.75, 4.0, 1.5, 2.0], torch.float32)
    ts = e([10, 20, 20, 30, 45, 60, 61], torch.int64)
    p = e([1, 0, 1, 1, 0, 0, 1], torch.int8)
    t0 = [0.0, 31.0, 45.0, 10.0, 20.0, 31.0, 50.0, 62.0, 10.0]
    t1 = [5.0, 44.0, 46.0, 31.0, 45.5, 61.0, 40.0, 90.0, 62.0]
    g, c = events.voxel_grids(x, y, ts, p, t0, t1, H, W)
    assert c.tolist() == [0, 0, 1, 4, 4, 2, 0, 0, 7]
    ref = _restate(x, y, ts, p, t0, t1, H, W)
    assert torch.allclose(g.double(), ref, atol=1e-6, rtol=0)
    assert float(g[2].abs().sum()) == 0.0                                      # one event: 0 / 0 time, no vote (as the reference)
    out = torch.full((len(t0), 5, H, W), 7.0, device=DEV)
    g2, _ = events.voxel_grids(x, y, ts, p, e(t0, torch.float64), e(t1, torch.float64), H, W, out=out)
    assert g2.data_ptr() == out.data_ptr() and torch.allclose(out.double(), ref, atol=1e-6, rtol=0)
    # raw coordinates outside the rectify map are dropped, not read
    rm = torch.rand(H, W, 2, device=DEV) * 4
    xi, yi = e([0, W, 3, -1, 2], torch.int32), e([0, 1, H, 2, 2], torch.int32)
    tsi, pi_ = e([1.0, 2.0, 3.0, 4.0, 5.0], torch.float64), e([1, 1, 1, 1, 0], torch.int8)
    g, c = events.voxel_grids(xi, yi, tsi, pi_, [0.0], [9.0], H, W, rectify_map=rm)
    keep = torch.tensor([0, 4], device=DEV)                                 # the window's first and last event are among them
    sub = _restate(xi[keep], yi[keep], tsi[keep], pi_[keep], [0.0], [9.0], H, W, rmap=rm)
    assert c.tolist() == [5] and torch.allclose(g.double(), sub, atol=1e-6, rtol=0)
    # rescale: one polarity only, none at all
    pos = torch.rand(1, 2, 5, H, W, device=DEV) * (torch.rand(1, 2, 5, H, W, device=DEV) > 0.5)
    assert torch.equal(events.rescale(pos), pos / pos.max())
    assert torch.equal(events.rescale(-pos), -pos / pos.max())
    z = torch.zeros(1, 1, 5, H, W, device=DEV)
    assert torch.equal(events.rescale(z), z)
    # hot pixels: leading dimensions, one voxel (NaN std: nothing removed), an all-zero grid
    v = torch.randn(2, 3, 5, H, W, device=DEV)
    v[1, 2, 3, 4, 5] = 40.0
    hv = events.remove_hot_pixels(v, 3)
    assert torch.equal(hv, _hot_restated(v.view(-1, 5, H, W), 3).float().view_as(v)) and float(hv[1, 2, 3, 4, 5]) == 0.0
    assert torch.equal(events.remove_hot_pixels(torch.ones(1, 1, 1, device=DEV), 1), torch.ones(1, 1, 1, device=DEV))
    assert torch.equal(events.remove_hot_pixels(torch.zeros(5, H, W, device=DEV), 6), torch.zeros(5, H, W, device=DEV))
    with pytest.raises(NotImplementedError):
        events.RemoveHotPixelsVoxel(num_hot_pixels=10)
    # real_data_voxels: a resize is out of scope; the map must have the sensor size
    xr, yr = e([1, 2], torch.int32), e([1, 2], torch.int32)
    with pytest.raises(NotImplementedError):
        next(events.real_data_voxels(xr, yr, ts[:2], p[:2], [0.0], 5.0, [1, 1, 1, 1], rm, H, W, 6, out_hw=(H // 2, W // 2)))
    with pytest.raises(ValueError):
        next(events.real_data_voxels(xr, yr, ts[:2], p[:2], [0.0], 5.0, [1, 1, 1, 1], rm[:-1], H, W, 6))
    with pytest.raises(TypeError):
        events.voxel_grids(x, y, ts, p, [0.0], [9.0], H, W, rectify_map=rm)        # a map wants raw integer coordinates


def test_voxel_grids_replays_in_a_graph():
    """voxel_grids (window bounds, voxelisation, hot-pixel filter) captured into one graph and replayed on NEW events equals an eager
    call: nothing in it waits for the host.  (The float atomics add in another order on every run, so the filter is checked on the
    replayed grids themselves.)"""
    from devo_amd import events
    gen = torch.Generator().manual_seed(3)
    N, S, H, W = 200_000, 24, 60, 80

    def stream():
        ts = torch.sort(torch.randint(0, 1_000_000, (N,), generator=gen)).values
        return [a.to(DEV) for a in (torch.randint(0, W, (N,), generator=gen).int(), torch.randint(0, H, (N,), generator=gen).int(), ts,
                                    torch.randint(0, 2, (N,), generator=gen).to(torch.int8))]

    rmap = (torch.rand(H, W, 2, generator=gen) * torch.tensor([W, H]) - 0.5).to(DEV)
    t0 = (torch.arange(S, dtype=torch.float64) * 40_000).to(DEV)
    t1 = t0 + 55_000
    static = stream()

    def call():
        raw, cnt = events.voxel_grids(*static, t0, t1, H, W, rectify_map=rmap)
        fused, _ = events.voxel_grids(*static, t0, t1, H, W, rectify_map=rmap, hot_pixel_stds=6)
        return raw, cnt, events.remove_hot_pixels(raw, 6), fused

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                                # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            raw, counts, hot, fused = call()
    torch.cuda.current_stream().wait_stream(s)
    fresh = stream()
    for a, b in zip(static, fresh):
        a.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    eager, ec = events.voxel_grids(*fresh, t0, t1, H, W, rectify_map=rmap)
    assert torch.equal(counts, ec)
    assert_rel(raw, eager, 1e-6, "graph replay")
    assert torch.equal(hot == 0, _hot_restated(raw, 6) == 0) and torch.equal(hot, torch.where(hot == 0, 0.0, raw))
    flips = (fused == 0) != (hot == 0)                                         # only a voxel within fp32 rounding of its threshold
    assert int(flips.sum()) <= 10
    assert_rel(torch.where(flips, 0.0, fused), torch.where(flips, 0.0, hot), 1e-6, "graph replay, hot pixels removed")
