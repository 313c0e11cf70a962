"""The inputs of tests/test_gpu_corr_coords.py and the oracle on them, pinned without a GPU — so that the GPU test cannot pass vacuously:
the hostile case really has clean edges, bad pixels and far pixels in the stated proportions, the oracle (oracle/altcorr.py) gives NaN exactly
on bad pixels' outputs, exact zeros on far ones and is bit-independent of other edges; the border case really contains every swept value, its
structural-zero mask is neither empty nor everything, and the vectorised oracle agrees with its scalar twin there."""
import math
import pytest
import torch
import corr_coord_cases as K
from oracle import altcorr as A


@pytest.fixture(scope="module")
def host():
    return K.hostile(0)


def test_hostile_case_has_the_stated_composition(host):
    E = host["coords"].shape[1]
    assert E == 160 and host["coords"].shape == (1, E, 2, 3, 3)
    assert host["clean_edge"].float().mean() >= 0.4
    assert 0 < host["bad_pixel"].float().mean() <= 0.25
    # every value in every placement
    seen = {(int(v), int(p)) for v, p in zip(host["value"], host["placement"]) if v >= 0}
    assert seen == {(v, p) for v in range(len(K.HOSTILE_VALUES)) for p in range(len(K.PLACEMENTS))}
    for e in range(E):
        v, p = int(host["value"][e]), int(host["placement"][e])
        if v < 0:
            assert torch.equal(host["coords"][0, e], host["benign"][0, e])
            continue
        val = torch.tensor(K.HOSTILE_VALUES[v], dtype=torch.float32)
        diff = ~((host["coords"][0, e] == host["benign"][0, e]))
        assert int(diff.sum()) == (1, 1, 2, 18, 16)[p]
        got = host["coords"][0, e][diff]
        assert bool(torch.isnan(got).all()) if math.isnan(K.HOSTILE_VALUES[v]) else bool((got == val).all())
        if p == 2:
            assert bool(diff[:, 1, 1].all())                       # the centre pixel: the one the plan reads
    # clean edges: nine near pixels at both levels; an exactly-integer one among them
    for s, (h, w) in ((1, (K.H, K.W)), (4, (K.H // 4, K.W // 4))):
        bad, far = K.classify(host["coords"][0] / s, 3, h, w)
        assert not bool((bad | far)[host["clean_edge"]].any())
        assert torch.equal(bad, host["bad_pixel"])
        assert bool(far.any())
    assert bool(host["clean_edge"][0]) and torch.equal(host["coords"][0, 0], host["coords"][0, 0].round())
    # patches 0..11 belong to edges without a bad pixel; the last frame has no edge
    has_bad = host["bad_pixel"].flatten(1).any(1)
    assert int(host["ii"][has_bad].min()) >= K.N_PATCHES // 2 and set(host["ii"][~has_bad].tolist()) >= set(range(K.N_PATCHES // 2))
    assert int(host["jj"].max()) == K.N_FRAMES - 2
    # sanitised: finite everywhere, bad pixels at -1e5, every other value untouched
    san = host["sanitised"][0]
    m = host["bad_pixel"][:, None].expand_as(san)
    assert bool(torch.isfinite(san).all()) and bool((san[m] == K.SANITISED).all()) and torch.equal(san[~m], host["coords"][0][~m])
    # every hostile magnitude is a far pixel at radius 5 too
    assert not bool(K.classify(host["coords"][0], 5, K.H, K.W)[1][host["clean_edge"]].any())


@pytest.mark.parametrize("R", [3, 5])
def test_oracle_on_the_hostile_case(host, R):
    f1, f2 = K.features(0)
    ii, jj = host["ii"], host["jj"]
    out = A.corr_forward(f1, f2, host["coords"], ii, jj, R)
    bad, far = K.classify(host["coords"][0], R, K.H, K.W)
    badm = bad[None, :, None, None].expand_as(out)
    farm = far[None, :, None, None].expand_as(out)
    assert bool(torch.isnan(out[badm]).all()), "the oracle is NaN on every output of a bad pixel"
    assert bool(torch.isfinite(out[~badm]).all()), "... and finite everywhere else"
    assert int(torch.count_nonzero(out[farm])) == 0 and int(farm.sum()) > 0, "far pixels: exact zeros"
    zero = K.structural_zero(host["coords"], ii, jj, R, K.H, K.W)
    assert bool(zero[farm].all()) and not bool(zero[badm].any())
    assert int(torch.count_nonzero(out[zero])) == 0
    # independence: the clean edges' outputs do not depend on what the other edges hold, bit for bit
    ben = A.corr_forward(f1, f2, host["benign"], ii, jj, R)
    ce = host["clean_edge"]
    assert torch.equal(out[:, ce], ben[:, ce]) and bool(torch.isfinite(ben).all())
    # the sanitised coordinates: the same finite outputs, zeros where the bad pixels were
    san = A.corr_forward(f1, f2, host["sanitised"], ii, jj, R)
    assert torch.equal(san[~badm], out[~badm]) and int(torch.count_nonzero(san[badm])) == 0


def test_oracle_on_the_hostile_case_at_level_1(host):
    f1, f2 = K.features(0)
    l1 = K.level1(f2)
    c4 = host["coords"] / 4
    out = A.corr_forward(f1, l1, c4, host["ii"], host["jj"], 3)
    bad, far = K.classify(c4[0], 3, K.H // 4, K.W // 4)
    badm = bad[None, :, None, None].expand_as(out)
    farm = far[None, :, None, None].expand_as(out)
    assert bool(torch.isnan(out[badm]).all()) and bool(torch.isfinite(out[~badm]).all())
    assert int(torch.count_nonzero(out[farm])) == 0 and int(farm.sum()) > 0


@pytest.mark.parametrize("R", [0, 1, 3, 5])
def test_border_case_contains_every_swept_value_and_is_not_vacuous(R):
    b = K.border(0, R)
    c = b["coords"][0]
    assert 100 <= c.shape[0] <= 120
    n = c.shape[0] // 2
    for axis, vals, size in ((0, b["sweep_x"], K.W), (1, b["sweep_y"], K.H)):
        assert len(vals) == 19 and (R < 3 or len(set(vals)) == 18)    # (-0.0 == 0.0 as numbers; at small radii -R - 1, -R and -1 coincide)
        centre = c[:n, axis, 1, 1]
        for v in vals:
            hit = centre == torch.tensor(v, dtype=torch.float32)
            if v == 0.0:
                hit = hit & (torch.signbit(centre) == (math.copysign(1.0, v) < 0))
            assert bool(hit.any()), (axis, v)
        # the named ones are what they are meant to be
        frac = lambda v: float(torch.tensor(v) - torch.tensor(v).floor())
        assert -1e-7 in vals and -1e-8 in vals and frac(-1e-7) < 1.0 and frac(-1e-8) == 1.0     # -1e-8: fp32 fraction exactly 1.0
        assert {-R - 2.0, -R - 1.0, -float(R), -1.0, size - 1.0, float(size), size + R - 1.0, float(size + R), size + R + 1.0} <= set(vals)
        assert any(-R - 1.0 < v < -R - 1.0 + 1e-5 for v in vals) and any(-1.0 - 1e-6 < v < -1.0 for v in vals)
        assert any(size - 1 - 1e-5 < v < size - 1 for v in vals) and any(size - 1 < v < size - 1 + 1e-5 for v in vals)
        assert any(size + R < v < size + R + 1e-5 for v in vals) and any(0 < v < 1e-30 for v in vals)
    assert torch.equal(c[n:], c[:n] + 0.5) and bool(torch.isfinite(c).all())                       # the same patches shifted by 0.5
    rel = c[:n] - c[:n, :, 1:2, 1:2]
    assert float((rel - rel.round()).abs().max()) <= 1e-5 and float(rel.abs().max()) <= 1.0 + 1e-5     # integer offsets (up to fp32 rounding)
    for z in (b["zero0"], b["zero1"]):
        assert z.shape == (1, c.shape[0], 2 * R + 1, 2 * R + 1, 3, 3)
        assert 0.2 <= float(z.float().mean()) <= 0.8, float(z.float().mean())


@pytest.mark.parametrize("R", [0, 1, 3, 5])
def test_vectorised_oracle_equals_its_scalar_twin_on_the_border_case(R):
    """A.corr_forward against A.corr_forward_scalar (one thread of the reference's kernel at a time) at the frame border, both levels"""
    b = K.border(0, R)
    f1, f2 = K.features(1, channels=4)
    for coords, fm, zero in ((b["coords"], f2, b["zero0"]), (b["coords"] / 4, K.level1(f2), b["zero1"])):
        vec = A.corr_forward(f1, fm, coords, b["ii"], b["jj"], R)
        sca = A.corr_forward_scalar(f1, fm, coords, b["ii"], b["jj"], R)
        assert float((vec - sca).abs().max()) <= 1e-12
        assert int(torch.count_nonzero(vec[zero])) == 0 and int(torch.count_nonzero(sca[zero])) == 0
        assert float((vec[~zero] != 0).float().mean()) > 0.99      # (and the mask is not wider than it has to be)


def test_wide_dead_case_misses_the_frame_with_an_enormous_box():
    w = K.wide_dead(0)
    c, ce = w["coords"], w["clean_edge"]
    assert c.shape == (1, 16, 2, 3, 3) and int(ce.sum()) == 4
    f1, f2 = K.features(0, channels=8)
    for s, (h, wd) in ((1, (K.H, K.W)), (4, (K.H // 4, K.W // 4))):
        for R in (3, 5):
            bad, far = K.classify(c[0] / s, R, h, wd)
            assert bool((bad | far)[~ce].all()) and not bool((bad | far)[ce].any()) and int(bad.sum()) == 4
            out = A.corr_forward(f1, f2 if s == 1 else K.level1(f2), c / s, w["ii"], w["jj"], R)
            badm = bad[None, :, None, None].expand_as(out)
            assert bool(torch.isnan(out[badm]).all()) and int(torch.count_nonzero(out[:, ~ce][~badm[:, ~ce]])) == 0
            assert bool(torch.isfinite(out[:, ce]).all()) and float(out[:, ce].abs().max()) > 0.1
    x0 = torch.nan_to_num(c[0, ~ce, 0], nan=-1e6).flatten(1)
    y0 = torch.nan_to_num(c[0, ~ce, 1], nan=-1e6).flatten(1)
    extent = torch.maximum(x0.amax(1) - x0.amin(1), y0.amax(1) - y0.amin(1))
    assert float(extent.min()) > 9e5                                   # every dead edge's box is about a million positions wide


def test_backward_and_patchify_oracles_stay_finite(host):
    f1, f2 = K.features(0, channels=16)
    ii, jj = host["ii"], host["jj"]
    E = len(ii)
    grad = torch.randn(1, E, 7, 7, 3, 3, generator=torch.Generator().manual_seed(5))
    for coords in (host["sanitised"], host["coords"]):
        d1, d2 = A.corr_backward(f1, f2, coords, ii, jj, grad, 3)
        assert bool(torch.isfinite(d2).all()) and int(torch.count_nonzero(d2[:, K.N_FRAMES - 1])) == 0
        if coords is host["sanitised"]:
            assert bool(torch.isfinite(d1).all())
            s1, s2 = d1, d2
    # hostile coordinates: d_fmap2 is what the sanitised ones give; d_fmap1 too, except (NaN) at bad pixels' own entries
    assert torch.equal(d2, s2)
    own = torch.zeros(K.N_PATCHES, 3, 3, dtype=torch.bool)
    for e in range(E):
        own[ii[e]] |= host["bad_pixel"][e]
    keep = ~own[None, :, None].expand_as(d1)
    assert torch.equal(d1[keep], s1[keep]) and not bool(own[:K.N_PATCHES // 2].any())
    net = torch.randn(2, 8, 12, 16, generator=torch.Generator().manual_seed(6))
    pc = K.patch_centres(0)
    assert pc.shape == (2, 40, 2)
    for R in (0, 1, 3):
        p = A.patchify_forward(net, pc, R)
        assert bool(torch.isfinite(p).all())
        bad, far = K.classify(pc[..., None, None].expand(2, 40, 2, 1, 1), R, 12, 16)
        dead = (bad | far)[:, :, 0, 0]
        assert int(dead.sum()) >= 32 and int(torch.count_nonzero(p[dead])) == 0 and int(torch.count_nonzero(p[~dead])) > 0
        gb = A.patchify_backward(net, pc, torch.randn(p.shape, generator=torch.Generator().manual_seed(7)), R)
        assert bool(torch.isfinite(gb).all())
