"""GPU checks of the voxel augmentation (devo_amd/events.py augment / voxel_augment over csrc/events.hip devo_voxel_augment) and of
TrainNet's input normalisation.

Parity with the reference (tests/golden/voxel_augment.npz: the reference's own voxel_utils.py with torchvision 0.13's ops restated,
tools/gen_golden_voxel_augment.py): _augment bit for bit for every op but adjust_contrast, whose per-image fp32 mean is a reduction
whose order torch does not fix (one quantisation level on at most 0.1 % of the voxels); voxel_augment end to end at the std tolerance of
tests/test_gpu_events.py (1e-5 of the scale).  At full size, against a test-local integer / float64 restatement on the GPU."""
import os
import numpy as np
import pytest
import torch
from util import assert_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
FULL = (1, 15, 5, 480, 640)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "voxel_augment.npz"))


# ---- restatement: integers where torchvision's values are integers, its fp32 blend formula, float64 statistics

def _div(a, d):
    """a / d as a true fp32 division (torch on the GPU turns a division by a Python scalar into a product with its reciprocal)."""
    return a / torch.full((), d, dtype=a.dtype, device=a.device)


def _quantise(x):
    R = (255.0 * torch.where(x < 0, -x, torch.zeros_like(x))).clamp(0, 255).to(torch.int32)
    B = (255.0 * torch.where(x > 0, x, torch.zeros_like(x))).clamp(0, 255).to(torch.int32)
    return R, B


def _blend(q, img2, ratio):
    r, omr = float(np.float32(ratio)), float(np.float32(1.0 - float(ratio)))
    return (r * q.float() + omr * img2.float()).clamp(0, 255).to(torch.int32)


def _gray(R, B):
    return ((0.2989 * R.float() + 0.0) + 0.114 * B.float()).to(torch.int32)


def _blur(q):
    """round(conv(q, [[1,1,1],[1,5,1],[1,1,1]] / 13)) on the interior, from the exact integer sum k (k / 13 is never a tie); the
    border keeps q."""
    h, w = q.shape[-2:]
    k = 4 * q[..., 1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            k = k + q[..., dy:h - 2 + dy, dx:w - 2 + dx]
    out = q.clone()
    out[..., 1:-1, 1:-1] = torch.round(k.double() / 13.0).to(torch.int32)
    return out


def _op(q, R, B, name, f):
    if name == "adjust_brightness":
        return _blend(q, torch.zeros_like(q), f)
    if name == "adjust_contrast":
        g = _gray(R, B)
        mean = g.sum(dim=(-2, -1), dtype=torch.int64, keepdim=True).float()
        mean = _div(mean, float(g.shape[-1] * g.shape[-2]))
        return _blend(q, mean, f)
    if name == "invert":
        return 255 - q
    if name == "posterize":
        return q & ((0xFF << (8 - int(f))) & 0xFF)
    if name == "adjust_saturation":
        return _blend(q, _gray(R, B), f)
    if name == "adjust_sharpness":
        if q.shape[-1] <= 2 or q.shape[-2] <= 2:
            return q
        return _blend(q, _blur(q), f)
    return torch.where(q >= int(f), 255 - q, q)


def ref_augment(x, name, f, rescale=False):
    """_augment (and rescale first) of x [b, n, c, h, w] on the GPU; returns (out f32, d = B' - R' int32)."""
    if rescale:
        pos, neg = x[x > 0], x[x < 0]
        pmax = pos.max() if pos.numel() else torch.ones((), device=x.device)
        nmax = -neg.min() if neg.numel() else torch.ones((), device=x.device)
        x = torch.where(x > 0, x / pmax, torch.where(x < 0, x / nmax, x))
    R, B = _quantise(x)
    R2, B2 = _op(R, R, B, name, f), _op(B, R, B, name, f)
    return _div(B2.float(), 255.0) + (-_div(R2.float(), 255.0)), B2 - R2


def ref_std(v):
    """std(v) sequence-wise with float64 statistics."""
    b = v.shape[0]
    flat = v.double().reshape(b, -1)
    nz = flat != 0
    cnt = nz.sum(-1)
    if not bool((cnt > 0).all()):
        return v.clone()
    mean = flat.sum(-1) / cnt
    sd = torch.sqrt((flat * flat).sum(-1) / cnt - mean * mean)
    return (nz * (flat - mean[:, None]) / sd[:, None]).reshape(v.shape)


def _factor(name, fi):
    from devo_amd import events
    t = events.aug_factors(10)[events.AUG_OPS.index(name)]
    return 0.0 if t.dim() == 0 else float(t[fi])


def _assert_contrast_close(got, ref, what, frac=1e-3):
    lv = ((got.double() - ref.double()).abs() * 255.0).round()
    assert float(lv.max()) <= 1.0 + 1e-9, f"{what}: off by {float(lv.max())} levels"
    assert float((lv > 0).double().mean()) <= frac, f"{what}: {float((lv > 0).double().mean()):.2e} of the voxels off by one level"


def _assert_aug_equal(got, ref, name, what):
    if name == "adjust_contrast":
        _assert_contrast_close(got, ref, what)
    else:
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} voxels differ, max {float((got - ref).abs().max()):.3e}"


def _events_grid(shape, seed, zeros=0.7, scale=3.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mag = torch.pow(10.0, torch.rand(shape, generator=g, device=DEV) * 4 - 3) * scale
    sign = torch.where(torch.rand(shape, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    keep = torch.rand(shape, generator=g, device=DEV) >= zeros
    return (mag * sign * keep).float()


# ---- golden parity

def test_augment_matches_reference_golden(gold):
    from devo_amd import events
    for grid in ("x", "x_odd", "x_tiny"):
        x = torch.from_numpy(gold[f"aug/{grid}"]).to(DEV)
        for name in events.AUG_OPS:
            for fi in ((0,) if name == "invert" else (0, 3, 6, 9)):
                ref = torch.from_numpy(gold[f"aug/{grid}/{name}_{fi}"]).to(DEV)
                got = events.augment(x, name, fi)
                _assert_aug_equal(got, ref, name, f"{grid} {name}[{fi}]")


def test_voxel_augment_matches_reference_golden(gold):
    from devo_amd import events
    seeds = sorted({int(k.split("/")[2]) for k in gold.files if k.startswith("va/1/") and k.endswith("/choice")})
    for r, key in ((1, "aug/x"), (0, "raw/x")):
        x = torch.from_numpy(gold[key]).to(DEV)
        for s in seeds:
            torch.manual_seed(s)
            got = events.voxel_augment(x, rescaled=bool(r))
            assert_rel(got, torch.from_numpy(gold[f"va/{r}/{s}"]), 1e-5, f"voxel_augment rescaled={r} seed {s}")
            torch.manual_seed(s)
            assert list(events.draw_augmentation(10)) == gold[f"va/{r}/{s}/choice"].tolist()


# ---- full size against the restatement

@pytest.mark.parametrize("name", ["adjust_brightness", "adjust_contrast", "invert", "posterize", "adjust_saturation", "adjust_sharpness",
                                  "solarize"])
def test_full_size_every_op(name):
    from devo_amd import events
    raw = _events_grid(FULL, 11)
    x = events.rescale(raw)
    for fi in (0, 9):
        f = _factor(name, fi)
        ref, _ = ref_augment(x, name, f)
        _assert_aug_equal(events.augment(x, name, fi), ref, name, f"full size {name}[{fi}]")
        got = events.voxel_augment(raw, op=name, factor_index=fi)
        assert_rel(got, ref_std(ref), 1e-5, f"full size voxel_augment {name}[{fi}]")


# ---- edge cases

@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_polarity_only(sign):
    from devo_amd import events
    x = _events_grid((1, 3, 5, 24, 32), 3).abs() * sign
    for name in events.AUG_OPS:
        fi = 6
        ref, _ = ref_augment(x, name, _factor(name, fi), rescale=True)
        assert_rel(events.voxel_augment(x, op=name, factor_index=fi), ref_std(ref), 1e-5, f"{name} sign {sign}")


def test_sequence_without_events_leaves_tensor_unstandardised():
    from devo_amd import events
    x = _events_grid((2, 2, 5, 16, 24), 4)
    x[1] = 0.0
    for name in ("adjust_brightness", "invert", "adjust_sharpness", "solarize"):
        got = events.voxel_augment(x, op=name, factor_index=3)
        assert torch.equal(got, events.augment(events.rescale(x), name, 3)), name
        assert int((got[1] != 0).sum()) == 0


@pytest.mark.parametrize("hw", [(2, 7), (6, 2), (2, 2), (3, 3)])
def test_small_images_sharpness(hw):
    from devo_amd import events
    x = events.rescale(_events_grid((1, 2, 5) + hw, 5, zeros=0.2))
    for fi in (0, 9):
        ref, _ = ref_augment(x, "adjust_sharpness", _factor("adjust_sharpness", fi))
        assert torch.equal(events.augment(x, "adjust_sharpness", fi), ref), f"{hw} [{fi}]"
    if min(hw) <= 2:                                              # returned unchanged: quantised and back
        R, B = _quantise(x)
        assert torch.equal(events.augment(x, "adjust_sharpness", 9), _div(B.float(), 255.0) + (-_div(R.float(), 255.0)))


def test_width_not_multiple_of_four_and_several_sequences():
    from devo_amd import events
    for shape in ((1, 2, 5, 9, 13), (3, 2, 5, 17, 30), (2, 1, 5, 31, 21)):
        raw = _events_grid(shape, 6)
        raw[0] *= 10.0                                            # sequences with different statistics
        x = events.rescale(raw)
        for name in events.AUG_OPS:
            fi = 9
            f = _factor(name, fi)
            ref, _ = ref_augment(x, name, f)
            _assert_aug_equal(events.augment(x, name, fi), ref, name, f"{shape} {name}")
            assert_rel(events.voxel_augment(raw, op=name, factor_index=fi), ref_std(ref), 1e-5, f"{shape} {name} voxel_augment")
            assert_rel(events.voxel_augment(x, rescaled=True, op=name, factor_index=fi), ref_std(ref), 1e-5, f"{shape} {name} rescaled")


# ---- reproducibility and capture

def test_bit_reproducible_and_input_unchanged():
    from devo_amd import events
    raw = _events_grid((1, 15, 5, 120, 160), 7)
    keep = raw.clone()
    for name in ("adjust_contrast", "adjust_sharpness", "adjust_saturation"):
        a = events.voxel_augment(raw, op=name, factor_index=5)
        b = events.voxel_augment(raw, op=name, factor_index=5)
        assert torch.equal(a, b), name
    assert torch.equal(raw, keep)


def test_graph_replay_matches_eager():
    """Captured once, replayed on new input data: the workspace (extremes, grayscale sums, statistics) is cleared by a kernel that
    replays with the graph."""
    from devo_amd import events
    shape = (2, 3, 5, 48, 64)
    static = _events_grid(shape, 8).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        events.voxel_augment(static, op="adjust_contrast", factor_index=4)             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = events.voxel_augment(static, op="adjust_contrast", factor_index=4)
    for seed in (9, 10):
        new = _events_grid(shape, seed) * (1.0 + seed)
        static.copy_(new)
        g.replay()
        torch.cuda.synchronize()
        eager = events.voxel_augment(new, op="adjust_contrast", factor_index=4)
        assert torch.equal(out, eager), f"replay {seed}"


# ---- training

@pytest.mark.parametrize("norm", ["none", "rescale", "norm", "standard", "std", "standard2", "std2"])
def test_normalise_images_matches_events(norm):
    from devo_amd import events
    from devo_amd.training import TrainNet
    net = TrainNet(norm=norm).to(DEV).train()
    x = _events_grid((1, 4, 5, 32, 40), 12)
    expect = {"none": lambda v: v, "rescale": events.rescale, "norm": events.rescale, "standard": lambda v: events.std(v, sequence=False),
              "std": lambda v: events.std(v, sequence=False), "standard2": events.std, "std2": events.std}[norm](x)
    assert torch.equal(net.normalise_images(x), expect)


def _augmenting_numpy_seed():
    for s in range(1000):
        np.random.seed(s)
        if np.random.rand() < 0.33:
            return s
    raise AssertionError("no seed")


@pytest.mark.parametrize("norm", ["rescale", "std2"])
def test_randaug_branch_matches_voxel_augment(norm):
    from devo_amd import events
    from devo_amd.training import TrainNet
    net = TrainNet(norm=norm, randaug=True).to(DEV).train()
    x = _events_grid((1, 4, 5, 32, 40), 13)
    np.random.seed(_augmenting_numpy_seed())
    torch.manual_seed(3)
    got = net.normalise_images(x)
    torch.manual_seed(3)
    if norm == "rescale":
        expect = events.voxel_augment(events.rescale(x), rescaled=True)
    else:
        expect = events.voxel_augment(events.std(x), rescaled=False)
    assert torch.equal(got, expect)
    net.eval()                                                    # evaluation never augments
    np.random.seed(_augmenting_numpy_seed())
    assert torch.equal(net.normalise_images(x), events.std(x) if norm == "std2" else events.rescale(x))
    none = TrainNet(norm="none", randaug=True).to(DEV).train()
    np.random.seed(_augmenting_numpy_seed())
    with pytest.raises(NotImplementedError):
        none.normalise_images(x)


def test_train_step_with_rescale_and_randaug():
    from devo_amd import training as T
    net, model, opt = T.build_trainer(DEV, 1, norm="rescale", randaug=True)
    batch = T.make_batch("cfg1", 1234, DEV)
    np.random.seed(_augmenting_numpy_seed())
    opt.zero_grad(set_to_none=True)
    loss = model(batch, iters=3)
    loss.backward()
    assert torch.isfinite(loss)
    bad = [n for n, q in net.named_parameters() if q.grad is None or not torch.isfinite(q.grad).all()]
    assert not bad, bad
    l2 = T.train_step(model, opt, batch, iters=3)
    assert torch.isfinite(l2)
