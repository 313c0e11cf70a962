"""tests/select_ref.py — the CPU restatement the GPU selection kernel is tested against — checked itself: against the fixtures of the
reference's PatchSelector (patchifier_f64.npz: pooled top-k, nms_select.npz: pooled NMS) and against devo_amd.patchifier.select, the torch
composition, on random maps."""
import os
import re

import numpy as np
import pytest
import torch

from devo_amd import patchifier as PF
from select_ref import select_ref


def test_topk_restatement_is_the_reference_selection(golden_dir):
    z = np.load(os.path.join(golden_dir, "patchifier_f64.npz"))
    sm = torch.from_numpy(z["topk/scores"])
    for grid in (True, False):
        r = select_ref(sm, 8, "topk", grid)
        assert torch.equal(r.x, torch.from_numpy(z[f"topk/x_grid{int(grid)}"])) and torch.equal(r.y, torch.from_numpy(z[f"topk/y_grid{int(grid)}"])), grid


def test_nms_restatement_is_the_reference_selection(golden_dir):
    z = np.load(os.path.join(golden_dir, "nms_select.npz"))
    for tag in ("a", "b"):
        sm = torch.from_numpy(z[f"{tag}/scores"])
        for grid in (True, False):
            r = select_ref(sm, int(z[f"{tag}/m"]), "nms", grid)
            assert torch.equal(r.x, torch.from_numpy(z[f"{tag}/x_grid{int(grid)}"])) and torch.equal(r.y, torch.from_numpy(z[f"{tag}/y_grid{int(grid)}"])), (tag, grid)
    with pytest.raises(RuntimeError, match="keeps"):
        select_ref(torch.from_numpy(z["a/scores"]), 400, "nms", False)


@pytest.mark.parametrize("mode", ["topk", "nms"])
def test_restatement_equals_the_composition_on_random_maps(mode):
    g = torch.Generator().manual_seed(7)
    for (n, h, w), m in (((2, 13, 22), 8), ((1, 24, 32), 12), ((3, 30, 38), 8)):
        sm = torch.sigmoid(torch.randn(1, n, h, w, generator=g))
        for grid in (True, False):
            x, y = PF.select(sm, m, mode, grid)
            r = select_ref(sm, m, mode, grid)
            assert torch.equal(r.x, x) and torch.equal(r.y, y), (mode, h, w, grid)
            assert torch.equal(r.scores, sm[0][torch.arange(n)[:, None], y, x])
            assert torch.equal(r.index, torch.arange(n).repeat_interleave(m))


def test_three_x_random_restatement_equals_the_composition():
    g = torch.Generator().manual_seed(9)
    sm = torch.rand(1, 2, 13, 22, generator=g)
    cand = (torch.randint(0, 22, (2, 18), generator=g), torch.randint(0, 13, (2, 18), generator=g))
    x, y, s = PF.select_three_x_random(sm, 6, cand)
    r = select_ref(sm, 6, "3xrandom", candidates=cand, pad=False)
    assert torch.equal(r.x, x) and torch.equal(r.y, y) and torch.equal(r.scores, s)


def test_patches_of_the_restatement_are_the_patchifier_closed_form():
    """select_ref's patches against the lines of Patchifier.forward they restate (depth plane 1 without disps; with disps the gathered depth and
    zeros outside the frame)."""
    g = torch.Generator().manual_seed(11)
    sm = torch.rand(1, 2, 10, 14, generator=g)
    disps = torch.rand(1, 2, 12, 16, generator=g) + 0.5
    r0 = select_ref(sm, 4, "topk", True, offset=1)
    r1 = select_ref(sm, 4, "topk", True, offset=1, disps=disps)
    assert torch.equal(r0.patches[:, :2, 1, 1], r0.xy.reshape(-1, 2)) and bool((r0.patches[:, 2] == 1).all())
    assert torch.equal(r1.patches[:, 2, 1, 1], disps[0][r1.index, r1.y.reshape(-1), r1.x.reshape(-1)])
    far = select_ref(sm, 4, "topk", True, offset=-3, disps=disps)              # centres pushed towards the top-left: patch pixels leave the frame
    out = (far.x.reshape(-1) < 1) | (far.y.reshape(-1) < 1)
    assert bool(out.any()) and bool((far.patches[out][:, :, 0, 0] == 0).all())


def test_cell_limit_is_the_headers():
    """devo_amd.select.MAX_CELLS restates DEVO_SELECT_MAX_CELLS of include/devo_hip.h, and the mode numbers its enum"""
    from devo_amd import select
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "devo_hip.h")).read()
    assert int(re.search(r"#define\s+DEVO_SELECT_MAX_CELLS\s+(\d+)", txt).group(1)) == select.MAX_CELLS
    enum = dict(re.findall(r"DEVO_SELECT_(\w+) = (\d+)", txt))
    assert {k.lower(): int(v) for k, v in enum.items()} == select.MODES
