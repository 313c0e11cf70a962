"""devo_amd.select (csrc/select.hip): the patch selection and its tail in one launch, against tests/select_ref.py (the CPU restatement,
itself checked in test_select_cpu.py), the fixtures of the reference's PatchSelector and devo_amd.patchifier.select, the torch composition.
Every case is a few launches on maps of at most 40 x 56."""
import os

import numpy as np
import pytest
import torch

from devo_amd import patchifier as PF
from select_ref import nms_survivors, select_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def S():
    from devo_amd import select
    return select


def _assert_equal(got, ref, what):
    for name in ("x", "y", "index", "scores", "patches", "xy"):
        assert torch.equal(getattr(got, name).cpu(), getattr(ref, name)), (what, name)


def _exact_map(n, h, w, g):
    """a random permutation of 1 .. h w times 2^-10 per frame: all values distinct, every sum of 16 exact in fp32 in any order"""
    return torch.stack([(torch.randperm(h * w, generator=g) + 1).float().reshape(h, w) for _ in range(n)]) * 2.0 ** -10


def _exp_noise(shape, g):
    return -torch.log1p(-torch.rand(shape, generator=g))         # Exp(1) draws from the host generator


# ------------------------------------------------------------------------------------------------ 1. exact against the restatement
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(13, 22), (24, 32)])             # odd padding in both axes (3 and 2) / no padding
@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("mode", ["topk", "multi", "nms", "3xrandom"])
def test_every_mode_equals_the_restatement_bit_for_bit(mode, grid, hw, n):
    h, w = hw
    g = torch.Generator().manual_seed(1000 * n + 10 * h + int(grid))
    sm = _exact_map(n, h, w, g)
    C = S().cells(h, w, grid)
    _, _, hp, wp = S().padding(h, w, grid)
    disps = torch.rand(n, h, w, generator=g) + 0.5                # the map's own size: with offset 1 patch pixels leave the frame
    for m in (4, min(nms_survivors(sm, grid)) if mode == "nms" else C):      # one per quadrant / every cell of every quadrant
        kw = {}
        if mode == "multi":
            kw["noise"] = _exp_noise((n, C + 16 * m), g)
        if mode == "3xrandom":
            kw["candidates"] = (torch.randint(0, wp, (n, 3 * m), generator=g), torch.randint(0, hp, (n, 3 * m), generator=g))
        dkw = {k: (tuple(c.to(DEV) for c in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in kw.items()}
        _assert_equal(S().select(sm.to(DEV), m, mode, grid, **dkw), select_ref(sm, m, mode, grid, **kw), (mode, grid, hw, n, m))
        _assert_equal(S().select(sm.to(DEV), m, mode, grid, offset=1, disps=disps.to(DEV), clamp=((1, w - 1), (2, h)), **dkw),
                      select_ref(sm, m, mode, grid, offset=1, disps=disps, clamp=((1, w - 1), (2, h)), **kw), (mode, grid, hw, n, m, "disps"))


def test_strided_score_maps_are_read_in_place():
    g = torch.Generator().manual_seed(5)
    big = _exact_map(2, 26, 44, g).to(DEV)
    sm = big[:, ::2, ::2]                                         # 13 x 22 with strides (1144, 88, 2)
    assert not sm.is_contiguous()
    _assert_equal(S().select(sm[None], 8, "topk", True), select_ref(sm.cpu(), 8, "topk", True), "strided")


def test_both_bindings_return_the_same_tensors(monkeypatch):
    """the compiled binding (devo_amd._C.select, torch.ops.devo_hip.patch_select) and the ctypes binding call one C entry point; the compiled one
    is in use unless DEVO_BINDING=ctypes asks for the other (a binding that failed to build or load fails here)"""
    from devo_amd import backends
    nat = backends.native()
    assert (nat is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
    assert nat is None or nat.select.MAX_CELLS == S().MAX_CELLS
    g = torch.Generator().manual_seed(6)
    n, h, w, m = 2, 13, 22, 8
    sm = _exact_map(n, h, w, g).to(DEV)
    disps = (torch.rand(1, n, h + 2, w + 2, generator=g) + 0.5).to(DEV)
    kws = {"topk": {}, "nms": {}, "multi": {"noise": _exp_noise((n, S().cells(h, w) + 16 * m), g).to(DEV)},
           "3xrandom": {"candidates": (torch.randint(0, 24, (n, 3 * m), generator=g).to(DEV), torch.randint(0, 16, (n, 3 * m), generator=g).to(DEV))}}
    compiled = {mode: S().select(sm, m, mode, True, offset=1, disps=disps, **kw) for mode, kw in kws.items()}
    if nat is not None:                                           # the registered operator is the same function
        op = torch.ops.devo_hip.patch_select(sm, m, S().MODES["topk"], True, 4, True, None, None, None, 1, False, 0, 0, 0, 0, disps[0], 3)
        for got, name in zip(op, compiled["topk"]._fields):
            assert torch.equal(got, getattr(compiled["topk"], name)), name
    monkeypatch.setattr(backends, "_native", None)
    for mode, kw in kws.items():
        got = S().select(sm, m, mode, True, offset=1, disps=disps, **kw)
        for name in got._fields:
            assert torch.equal(getattr(got, name), getattr(compiled[mode], name)), (mode, name)


# ------------------------------------------------------------------------------------------------ 2. topk and nms on realistic scores
@pytest.fixture(scope="module")
def realistic():
    g = torch.Generator().manual_seed(21)
    return torch.sigmoid(torch.randn(1, 2, 30, 38, generator=g))


@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("mode", ["topk", "nms"])
def test_topk_and_nms_equal_the_composition_on_sigmoid_maps(realistic, mode, grid):
    x, y = PF.select(realistic, 12, mode, grid)
    got = S().select(realistic.to(DEV), 12, mode, grid)
    assert torch.equal(got.x.cpu(), x) and torch.equal(got.y.cpu(), y)
    _assert_equal(got, select_ref(realistic, 12, mode, grid), (mode, grid))


def test_topk_and_nms_equal_the_reference_fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "patchifier_f64.npz"))
    sm = torch.from_numpy(z["topk/scores"]).float().to(DEV)
    for grid in (True, False):
        got = S().select(sm, 8, "topk", grid)
        assert torch.equal(got.x.cpu(), torch.from_numpy(z[f"topk/x_grid{int(grid)}"])) and torch.equal(got.y.cpu(), torch.from_numpy(z[f"topk/y_grid{int(grid)}"])), grid
    z = np.load(os.path.join(golden_dir, "nms_select.npz"))
    for tag in ("a", "b"):
        sm = torch.from_numpy(z[f"{tag}/scores"]).to(DEV)
        for grid in (True, False):
            got = S().select(sm, int(z[f"{tag}/m"]), "nms", grid)
            assert torch.equal(got.x.cpu(), torch.from_numpy(z[f"{tag}/x_grid{int(grid)}"])) and torch.equal(got.y.cpu(), torch.from_numpy(z[f"{tag}/y_grid{int(grid)}"])), (tag, grid)


def test_nms_boxes_clamped_at_the_top_and_left_border():
    """maxima in the first row / column: x1 = max(cx - 1.5, 0) shifts the box instead of shrinking it"""
    g = torch.Generator().manual_seed(22)
    sm = 0.5 * torch.sigmoid(torch.randn(1, 2, 32, 40, generator=g))
    sm[..., 0, :] += 0.5 * torch.rand(2, 40, generator=g)
    sm[..., :, 0] += 0.5 * torch.rand(2, 32, generator=g)
    for grid in (True, False):
        x, y = PF.select(sm, 16, "nms", grid)
        assert bool((x == 0).any()) and bool((y == 0).any())      # clamped boxes are among the chosen
        got = S().select(sm.to(DEV), 16, "nms", grid)
        assert torch.equal(got.x.cpu(), x) and torch.equal(got.y.cpu(), y), grid


def test_nms_quadrant_test_in_pixels_against_the_pooled_size():
    """The reference compares the box corner in PIXELS with half the POOLED size (selector.py:221-224).  On a 32 x 40 map (8 x 10 cells) 'left'
    is x1 < 5 pixels, so two maxima at x = 19 and x = 20 — the two sides of the geometric middle — share a category, overlap with IoU 0.5 and the
    weaker one is suppressed; quadrants taken geometrically would keep both."""
    g = torch.Generator().manual_seed(23)
    sm = 0.5 * torch.sigmoid(torch.randn(1, 1, 32, 40, generator=g))
    sm[0, 0, 9, 19], sm[0, 0, 9, 20] = 0.99, 0.98                 # cells (2, 4) and (2, 5): the two strongest of the map
    x1a, x1b, w1 = 19 - 1.5, 20 - 1.5, 40 // 4
    assert (x1a < w1 / 2) == (x1b < w1 / 2) and (19 < 40 / 2) != (20 < 40 / 2)          # one category for the reference, two geometric quadrants
    x, y = PF.select(sm, 8, "nms", True)
    got = S().select(sm.to(DEV), 8, "nms", True)
    assert torch.equal(got.x.cpu(), x) and torch.equal(got.y.cpu(), y)
    chosen = set(zip(got.x[0].tolist(), got.y[0].tolist()))
    assert (19, 9) in chosen and (20, 9) not in chosen
    assert float(got.scores.min()) < 0.98                        # ... although it outscores chosen boxes


# ------------------------------------------------------------------------------------------------ 3. the tie rule
@pytest.mark.parametrize("grid", [True, False])
def test_equal_keys_rank_by_cell_index(grid):
    n, h, w, m = 1, 16, 24, 4
    C = S().cells(h, w, grid)
    const = torch.full((n, h, w), 0.5)
    g = torch.Generator().manual_seed(31)
    pair = 0.25 * torch.rand(n, h, w, generator=g)
    for y0, x0 in ((0, 8), (4, 0)):                               # cells (0, 2) and (1, 0) of one quadrant: the same 16 values, so equal maxima and means
        pair[0, y0:y0 + 4, x0:x0 + 4] = 0.5
        pair[0, y0 + 1, x0 + 1] = 0.75
    ones = torch.ones(n, C + 16 * m)
    cand = (torch.randint(0, w, (n, 3 * m), generator=g), torch.randint(0, h, (n, 3 * m), generator=g))
    cand[0][0, :2], cand[1][0, :2] = torch.tensor([9, 1]), torch.tensor([1, 5])        # the first two candidates sit on the two equal maxima
    for name, sm in (("constant", const), ("pair", pair)):
        for mode in ("topk", "multi", "nms", "3xrandom"):
            kw = {"noise": ones} if mode == "multi" else {"candidates": cand} if mode == "3xrandom" else {}
            dkw = {k: (tuple(c.to(DEV) for c in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in kw.items()}
            got = S().select(sm.to(DEV), m, mode, grid, **dkw)
            _assert_equal(got, select_ref(sm, m, mode, grid, **kw), (name, mode, grid))
            if name == "constant" and mode in ("topk", "nms") and not grid:
                assert got.x[0].tolist() == [0, 4, 8, 12] and got.y[0].tolist() == [0, 0, 0, 0]      # cells 0, 1, 2, 3 at their first pixel
            if name == "constant" and mode == "3xrandom":
                assert torch.equal(got.x.cpu(), (cand[0][:, 2 * m:] + 1).clamp(max=w - 1))                            # a stable sort leaves the candidates in order
            if name == "pair" and mode in ("topk", "nms"):
                assert (int(got.x[0, 0]), int(got.y[0, 0])) == (9, 1)                                # the lower cell index first
            if name == "pair" and mode == "multi":
                assert (int(got.x[0, 0]) // 4, int(got.y[0, 0]) // 4) == (2, 0)
            if name == "pair" and mode == "3xrandom":
                assert got.x[0, -2:].tolist() == [10, 2]                                             # ascending and stable: candidate 0 before candidate 1


# ------------------------------------------------------------------------------------------------ 4. the law of multi
def test_multi_draws_cells_in_proportion_to_their_mean():
    n = 4096
    sm = torch.empty(8, 8)
    sm[:4, :4], sm[:4, 4:], sm[4:, :4], sm[4:, 4:] = 0.1, 0.2, 0.3, 0.4
    sm = sm.expand(n, 8, 8).contiguous().to(DEV)
    torch.manual_seed(41)
    a = S().select(sm, 1, "multi", False)
    torch.manual_seed(41)
    b = S().select(sm, 1, "multi", False)
    torch.manual_seed(42)
    c = S().select(sm, 1, "multi", False)
    cell = (2 * (a.y // 4) + a.x // 4).flatten()
    freq = torch.bincount(cell, minlength=4).float().cpu() / n
    print("frequencies", freq.tolist())
    assert float((freq - torch.tensor([0.1, 0.2, 0.3, 0.4])).abs().max()) <= 0.04               # 5 sigma of a binomial with N = 4096 (sigma <= 32 counts)
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y) and torch.equal(a.patches, b.patches)
    assert not (torch.equal(a.x, c.x) and torch.equal(a.y, c.y))


# ------------------------------------------------------------------------------------------------ 5. nms with too few survivors
def test_nms_with_too_few_survivors_raises(golden_dir):
    z = np.load(os.path.join(golden_dir, "nms_select.npz"))
    with pytest.raises(RuntimeError, match="keeps"):
        S().select(torch.from_numpy(z["a/scores"]).to(DEV), 400, "nms", False)


def test_refusals():
    with pytest.raises(RuntimeError):
        S().select(torch.zeros(1, 16, 16), 4, "topk")             # CPU tensors: no fallback
    with pytest.raises(ValueError, match=str(S().MAX_CELLS)):
        S().select(torch.zeros(1, 264, 256, device=DEV), 4, "topk")          # 66 x 64 = 4224 cells


# ------------------------------------------------------------------------------------------------ 6. stream capture
def test_multi_and_topk_replay_from_a_captured_graph():
    g = torch.Generator().manual_seed(61)
    n, h, w, m = 2, 13, 22, 8
    C = S().cells(h, w, True)
    sm = _exact_map(n, h, w, g).to(DEV)
    nz = _exp_noise((n, C + 16 * m), g).to(DEV)
    S().select(sm, m, "multi", True, noise=nz)                    # (the library is loaded outside the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            a = S().select(sm, m, "multi", True, noise=nz)
            b = S().select(sm, m, "topk", True, offset=1)
    torch.cuda.current_stream().wait_stream(side)
    sm.copy_(_exact_map(n, h, w, g))
    nz.copy_(_exp_noise((n, C + 16 * m), g))
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(a, select_ref(sm.cpu(), m, "multi", True, noise=nz.cpu()), "replayed multi")
    _assert_equal(b, select_ref(sm.cpu(), m, "topk", True, offset=1), "replayed topk")
    ea, eb = S().select(sm, m, "multi", True, noise=nz), S().select(sm, m, "topk", True, offset=1)
    for name in a._fields:
        assert torch.equal(getattr(a, name), getattr(ea, name)) and torch.equal(getattr(b, name), getattr(eb, name)), name


# ------------------------------------------------------------------------------------------------ 7. the Patchifier
def _patchifier(kind):
    torch.manual_seed(71)
    pf = PF.Patchifier(3, 24, 16, 8, kind).to(DEV).eval()
    return pf, torch.randn(1, 2, 5, 48, 64, device=DEV)


def _both(pf, images, **kw):
    assert PF._SELECT
    with torch.no_grad():
        on = pf(images, **kw)
        PF._SELECT = False
        try:
            off = pf(images, **kw)
        finally:
            PF._SELECT = True
    return on, off


@pytest.mark.parametrize("mode,M", [("topk", 8), ("nms", 4)])
def test_patchifier_returns_the_compositions_tensors(mode, M):
    pf, images = _patchifier("scorer")
    disps = torch.rand(1, 2, 12, 16, device=DEV) + 0.5
    for kw in ({}, {"disps": disps}):
        on, off = _both(pf, images, patches_per_image=M, scorer_eval_mode=mode, **kw)
        fmap, gmap, imap, patches, index = on
        assert torch.equal(patches, off[3]) and torch.equal(index, off[4]) and torch.equal(gmap, off[1]) and torch.equal(imap, off[2])


def test_patchifier_multi_is_seeded_and_stays_inside():
    pf, images = _patchifier("scorer")
    outs = []
    for _ in range(2):
        torch.manual_seed(72)
        with torch.no_grad():
            outs.append(pf(images, patches_per_image=8))          # the default: 'multi' on the 2 x 2 grid
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    cx, cy = outs[0][3][0, :, 0, 1, 1], outs[0][3][0, :, 1, 1, 1]
    assert float(cx.min()) >= 1 and float(cx.max()) <= 16 - 2 and float(cy.min()) >= 1 and float(cy.max()) <= 12 - 2


def test_patchifier_gradient_selector_returns_the_compositions_tensors():
    pf, images = _patchifier("gradient")
    on, off = _both(pf, images, patches_per_image=8, scorer_eval_mode="topk")
    for a, b in zip(on, off):
        assert torch.equal(a, b)
