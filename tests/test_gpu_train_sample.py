"""GPU checks of the training sample's tail (devo_amd/data.py over csrc/data.hip devo_voxel_resample / devo_depth_normalise).

Parity with the reference (tests/golden/train_sample.npz: the reference's EVSDAugmentor, transform_rescale and EVSDDataset.__getitem__
on CPU, tools/gen_golden_train_sample.py), given its draws and its torch.rand_like jitter (regenerated here from the seed): crops,
nearest disparities, s, poses and intrinsics bit for bit; voxels within 2 ulp (bit for bit is expected).  The quantile against
torch.quantile on CPU and GPU, bit for bit, and above 2^24 elements against a sort.  Batching, the in-kernel jitter, the full training
size against torch on the GPU, and graph replay."""
import math
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from devo_amd import data

pytestmark = pytest.mark.gpu
DEV = "cuda"
CROP = (8, 120)
GI_CROP = (16, 250)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "train_sample.npz"))


def _vox(q):
    return torch.from_numpy(q.astype(np.float32) / np.float32(8))


def _disp(dq):
    return torch.from_numpy(1.0 / (dq.astype(np.float32) / np.float32(64)))


def _ulps(a, b):
    """Elementwise distance in fp32 ulps (NaN must match NaN)."""
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    b = np.ascontiguousarray(np.asarray(b, np.float32))
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all(), "NaN pattern differs"

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    d = np.abs(ordered(a) - ordered(b))
    d[na] = 0
    return d


def _bits_equal(a, b):
    assert _ulps(a, b).max(initial=0) == 0


def _rand_like(shape, seed):
    torch.manual_seed(seed)
    return torch.rand(shape)                                   # == torch.rand_like(voxels) on CPU for a float32 tensor


def _cuda(*ts):
    return [t.to(DEV) for t in ts]


# ---- golden parity

def test_augmentor_golden(gold):
    vox, disp = _vox(gold["in/vox_q"]), _disp(gold["in/depth_q"])
    poses, intr = torch.from_numpy(gold["in/poses"]), torch.from_numpy(gold["in/intr"])
    aug = data.EVSDAugmentor(list(CROP))
    seeds = sorted({int(k.split("/")[1]) for k in gold.files if k.startswith("aug/")})
    for s in seeds:
        noise = _rand_like(vox.shape, s)
        p = {"scale": float(gold[f"aug/{s}/scale"]), "seed": 0}
        v, po, d, k = aug.apply(*_cuda(vox, poses, disp, intr), p, noise=noise.to(DEV))
        _bits_equal(d.cpu(), gold[f"aug/{s}/d"])
        _bits_equal(k.cpu(), gold[f"aug/{s}/intr"])
        _bits_equal(po.cpu(), gold["in/poses"])
        u = _ulps(v.cpu(), gold[f"aug/{s}/v"])
        assert u.max() <= 2, (s, u.max())
        if p["scale"] == 1:
            _bits_equal(v.cpu(), gold[f"aug/{s}/v"])


def test_getitem_golden(gold):
    for key in sorted({k.rsplit("/", 1)[0] for k in gold.files if k.startswith("gi/") and k.count("/") == 3}):
        _, sc, s = key.split("/")
        sc, s = float(sc), int(s)
        src_v, src_d = ("in/vox_q", "in/depth_q") if sc == 1.0 else ("gi/vox_q", "gi/depth_q")
        crop = CROP if sc == 1.0 else GI_CROP
        vox, disp = _vox(gold[src_v]), _disp(gold[src_d])
        poses, intr = torch.from_numpy(gold["in/poses"]), torch.from_numpy(gold["in/intr"])
        H, W = vox.shape[-2:]
        shape = (vox.shape[0], vox.shape[1], math.floor(sc * H), math.floor(sc * W))        # the jitter runs after the rescale
        noise = _rand_like(shape, s)
        p = [{"scale": float(gold[f"{key}/scale_drawn"]), "seed": 0}]
        v, po, d, k = data.prepare_batch(*_cuda(vox[None], poses[None], disp[None], intr[None]), crop, scale=sc, params=p, noise=noise[None].to(DEV))
        _bits_equal(k[0].cpu(), gold[f"{key}/intr"])
        assert _ulps(v[0].cpu(), gold[f"{key}/v"]).max() <= 2, key
        if sc == 1.0:
            _bits_equal(v[0].cpu(), gold[f"{key}/v"])
            _bits_equal(d[0].cpu(), gold[f"{key}/d"])
            _bits_equal(po[0].cpu(), gold[f"{key}/poses"])
        else:
            assert _ulps(d[0].cpu(), gold[f"{key}/d"]).max() <= 2, key
            assert _ulps(po[0].cpu(), gold[f"{key}/poses"]).max() <= 2, key


def test_transform_rescale_golden(gold):
    vox, disp = _vox(gold["tr/vox_q"]), _disp(gold["tr/depth_q"])
    poses, intr = torch.from_numpy(gold["in/poses"][:1]), torch.from_numpy(gold["in/intr"][:1])
    for sc in (0.5, 0.75):
        v, d, p, k = data.transform_rescale(sc, *_cuda(vox, disp, poses, intr))
        assert _ulps(v.cpu(), gold[f"tr/{sc}/v"]).max() <= 2
        assert _ulps(d.cpu(), gold[f"tr/{sc}/d"]).max() <= 2
        _bits_equal(p.cpu(), gold[f"tr/{sc}/poses"])
        _bits_equal(k.cpu(), gold[f"tr/{sc}/intr"])


def test_normalise_golden_inf_nan_ties(gold):
    poses = torch.from_numpy(gold["in/poses"])
    for case in ("plain", "inf_few", "inf_at_q", "nan", "ties", "equal"):
        x = torch.from_numpy(gold[f"q/{case}/x"])
        d, p, s = data.normalise_depth(x[None].to(DEV).clone(), poses[None].to(DEV).clone())
        _bits_equal(s.cpu().reshape(()), gold[f"q/{case}/s"])
        _bits_equal(d[0].cpu(), gold[f"q/{case}/d"])
        _bits_equal(p[0].cpu(), gold[f"q/{case}/poses"])
    assert np.isnan(gold["q/nan/s"]) and np.isnan(gold["q/inf_at_q/s"])   # the cases do reach NaN


# ---- quantile

def _quantile(x, q):
    _, _, s = data.normalise_depth(x.reshape(1, -1).to(DEV).clone(), None, q=q, factor=1.0)
    return s.cpu()[0]


def _check_quantile(x, q):
    got = _quantile(x, q)
    ref_cpu = torch.quantile(x.cpu(), q)
    ref_gpu = torch.quantile(x.to(DEV), q).cpu()
    _bits_equal(got, ref_cpu)
    _bits_equal(got, ref_gpu)


def test_quantile_matches_torch():
    g = torch.Generator().manual_seed(3)
    cases = [
        torch.full((1000,), 2.5),                                        # all equal
        torch.randint(0, 4, (5000,), generator=g).float(),               # heavy ties
        torch.tensor([0.5]), torch.tensor([0.5, -1.0]), torch.tensor([3.0, -1.0, 2.0]),   # n = 1, 2, 3
        torch.rand(101, generator=g), torch.rand(1001, generator=g),     # the fp32 rank is integral at q = .98
        torch.randn(1000, generator=g), torch.randn(777, generator=g),   # ... and is not
        torch.randn(100000, generator=g) * 1e-3,
        torch.cat([torch.rand(300, generator=g), torch.full((50,), float("inf"))]),
        torch.cat([-torch.rand(300, generator=g), torch.full((5,), float("-inf"))]),
    ]
    for x in cases:
        for q in (0.98, 0.5, 0.3, 0.0, 1.0, 0.123):
            _check_quantile(x, q)


def test_quantile_signed_zero():
    x = torch.tensor([0.0, -0.0, 1.0, -2.0, 0.0, -0.0, 3.0])
    for q in (0.98, 0.5, 0.1, 0.9):
        got = _quantile(x, q)
        assert got == torch.quantile(x, q) and got == torch.quantile(x.to(DEV), q).cpu()
    x = torch.tensor([-0.0, -0.0, 1.0, 2.0])
    _bits_equal(_quantile(x, 0.2), torch.quantile(x, 0.2))               # only -0 at the rank: -0


def test_quantile_above_2_24():
    n = (1 << 24) + 4099
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(n, device=DEV, generator=g) * 3 + 0.25
    x[:1000] = 1.7                                                       # ties
    for q in (0.98, 0.31):
        got = _quantile(x, q)
        srt = torch.sort(x).values.cpu().numpy()
        r = np.float32(q) * np.float32(n - 1)
        lo, hi = int(r), int(np.ceil(r))
        w = np.float32(r - np.float32(lo))
        a, b = srt[lo], srt[min(hi, n - 1)]
        dd = np.float32(b - a)
        L = np.longdouble
        ref = (L(w) * L(dd) + L(a)) if abs(w) < 0.5 else (L(-dd) * L(np.float32(1) - w) + L(b))   # ATen's lerp (fused)
        _bits_equal(got, np.float32(ref))


# ---- batching and the in-kernel jitter

def _sample(seed, n=2, bins=5, H=40, W=150):
    g = torch.Generator().manual_seed(seed)
    vox = torch.randn(n, bins, H, W, generator=g)
    disp = torch.rand(n, H, W, generator=g) + 0.1
    poses = torch.randn(n, 7, generator=g)
    intr = torch.tensor([[300.0, 301.0, 75.0, 20.0]]).repeat(n, 1)
    return vox, poses, disp, intr


def test_batch_equals_single_calls():
    crop = (32, 128)
    samples = [_sample(s) for s in range(3)]
    params = [{"scale": 1.0, "seed": 11}, {"scale": 1.13, "seed": 12}, {"scale": 0.93, "seed": 13}]
    cat = [torch.stack([s[i] for s in samples]).to(DEV) for i in range(4)]
    out = data.prepare_batch(*cat, crop, params=params)
    for b in range(3):
        one = data.prepare_batch(*[t[None].to(DEV) for t in samples[b]], crop, params=[params[b]])
        for x, y in zip(out, one):
            assert torch.equal(x[b:b + 1], y)


def test_jitter_in_kernel():
    vox = torch.rand(1, 15, 5, 48, 64, device=DEV) * 0.01                # small: the sum's rounding stays far below the jitter
    size = vox.shape[-2:]
    j = lambda seed: data.voxel_color_jitter(vox, seed=seed)
    a, b, c = j(5), j(5), j(6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    d = (a.double() - vox.double()) / 1e-4
    assert d.abs().max() <= 1.0 + 1e-3 and d.abs().max() > 0.99
    assert abs(d.mean().item()) < 0.01
    hist = torch.histc(d.float(), bins=10, min=-1, max=1) / d.numel()
    assert (hist - 0.1).abs().max() < 0.01                                # roughly uniform
    assert size == a.shape[-2:]


def test_zoom_noise_is_keyed_on_source_index():
    """A zoomed call equals torch's bilinear + crop of the scale-1 output with the same seed (so the noise belongs to the source
    tap, not to the output pixel)."""
    g = torch.Generator().manual_seed(1)
    vox = (torch.rand(1, 2, 3, 44, 150, generator=g) + 0.5).to(DEV)      # positive: ulps of the output are meaningful
    disp = (torch.rand(1, 2, 44, 150, generator=g) + 0.1).to(DEV)
    poses = torch.zeros(1, 2, 7, device=DEV)
    intr = torch.ones(1, 2, 4, device=DEV)
    crop = (36, 120)
    aug = data.EVSDAugmentor(list(crop))
    scale = 1.07
    flat = data._resample(vox.reshape(1, 6, 44, 150), (44, 150), [(44, 150, 0, 0)], data.BILINEAR, seeds=[99])   # jittered source
    Hs, Ws, y0, x0 = aug.crop(44, 150, {"scale": scale})
    ref = F.interpolate(flat.cpu(), size=(Hs, Ws), mode="bilinear", align_corners=False)[..., y0:y0 + crop[0], x0:x0 + crop[1]]
    v, _, _, _ = aug.apply(vox[0], poses[0], disp[0], intr[0], {"scale": scale, "seed": 99})
    assert _ulps(v.reshape(ref.shape).cpu(), ref).max() <= 2


# ---- full size against torch on the GPU

def test_full_size_against_torch():
    B, n, bins, H, W = 1, 15, 5, 480, 640
    g = torch.Generator(device=DEV).manual_seed(0)
    vox = torch.randn(B, n, bins, H, W, device=DEV, generator=g)
    disp = 1.0 / (torch.rand(B, n, H, W, device=DEV, generator=g) * 20 + 0.5)
    poses = torch.randn(B, n, 7, device=DEV, generator=g)
    intr = torch.tensor([320.0, 320.0, 320.0, 240.0], device=DEV).repeat(B, n, 1)
    noise = torch.rand(B, n, bins, H, W, device=DEV, generator=g)
    for scale in (1.0, 1.1):
        p = [{"scale": scale, "seed": 0}]
        v, po, d, k = data.prepare_batch(vox, poses, disp, intr, (480, 640), params=p, noise=noise)
        # the reference's ops composed in torch on the GPU
        vj = vox[0] + (noise[0] - 0.5) * 2 * 1e-4
        Hs, Ws = int(H * scale), int(W * scale)
        y0, x0 = (Hs - 480) // 2, (Ws - 640) // 2
        rv = F.interpolate(vj, size=(Hs, Ws), mode="bilinear", align_corners=False)[..., y0:y0 + 480, x0:x0 + 640]
        rd = F.interpolate(disp[0][:, None], size=(Hs, Ws))[:, 0, y0:y0 + 480, x0:x0 + 640]
        assert torch.allclose(v[0], rv, rtol=1e-5, atol=1e-6)
        s = .7 * torch.quantile(rd, .98)
        assert torch.equal(d[0], rd / s)
        rp = poses[0].clone()
        rp[..., :3] *= s
        assert torch.equal(po[0], rp)
        rk = float(scale) * intr[0]
        rk[..., 2] -= x0
        rk[..., 3] -= y0
        assert torch.equal(k[0], rk)


# ---- graph capture

def test_graph_replay_equals_eager():
    crop = (32, 128)
    samples = [_sample(s) for s in range(2)]
    params = [{"scale": 1.0, "seed": 3}, {"scale": 1.1, "seed": 4}]
    static = [torch.stack([s[i] for s in samples]).to(DEV) for i in range(4)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        data.prepare_batch(*static, crop, params=params)                   # warm up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = data.prepare_batch(*static, crop, params=params)
    fresh = [_sample(s) for s in (7, 8)]
    for i in range(4):
        static[i].copy_(torch.stack([s[i] for s in fresh]))
    graph.replay()
    torch.cuda.synchronize()
    eager = data.prepare_batch(*static, crop, params=params)
    for x, y in zip(out, eager):
        assert torch.equal(x, y)
