"""CPU checks around devo_amd.graph: the plain-torch restatement of the reference's patch-graph bookkeeping (tests/patch_graph_ref.py, the
yardstick of tests/test_gpu_patch_graph.py) against hand-written tiny cases, so that the yardstick is not circular; every method of the
GPU class refuses CPU tensors (no fallback); header, ctypes table and library agree on ABI 9 and the devo_graph_* entry points."""
import math
import os
import re
import pytest
import torch
from patch_graph_ref import RefGraph, shift_frames as ref_shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 2
IX = torch.arange(6 * M) // M                                          # patch -> frame, 6 frames of 2 patches


def _hand_graph():
    """7 edges (ii = IX[kk], jj, kk), written out by hand for n = 6, keyframe_index = 2 (k = 4, motion pair 3 <-> 5)."""
    g = RefGraph(M, 8, IX)
    kk = torch.tensor([6, 10, 8, 2, 11, 0, 3])
    jj = torch.tensor([5, 3, 5, 4, 5, 3, 2])
    g.append_factors(kk, jj)
    assert g.ii.tolist() == [3, 5, 4, 1, 5, 0, 1] and g.net.shape == (1, 7, 8) and not g.net.any()
    g.net = torch.arange(7.0)[None, :, None].repeat(1, 1, 8)           # row e holds e
    return g


def _still_scene():
    poses = torch.zeros(1, 6, 7)
    poses[..., 6] = 1                                                   # every camera at the origin: no flow at all
    patches = torch.zeros(1, 12, 3, 3, 3)
    patches[:, :, 0] = 40.0
    patches[:, :, 1] = 30.0
    patches[:, :, 2] = 0.5
    intr = torch.tensor([80.0, 80.0, 80.0, 60.0]).expand(1, 6, 4).contiguous()
    return poses, patches, intr


def test_append_and_remove_by_hand():
    g = _hand_graph()
    g.append_factors(torch.tensor([5, 9]), torch.tensor([0, 1]))
    assert g.kk.tolist() == [6, 10, 8, 2, 11, 0, 3, 5, 9] and g.jj.tolist() == [5, 3, 5, 4, 5, 3, 2, 0, 1] and g.ii.tolist() == [3, 5, 4, 1, 5, 0, 1, 2, 4]
    assert g.net[0, :, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 0, 0]
    g.remove_factors(torch.tensor([1, 0, 0, 1, 0, 0, 0, 1, 0], dtype=torch.bool))
    assert g.kk.tolist() == [10, 8, 11, 0, 3, 9] and g.ii.tolist() == [5, 4, 5, 0, 1, 4] and g.jj.tolist() == [3, 5, 5, 3, 2, 1]
    assert g.net[0, :, 3].tolist() == [1, 2, 4, 5, 6, 0]


def test_keyframe_removal_branch_by_hand():
    """No motion: m / 2 = 0 < thresh.  Frame 4 goes: edges 2 (ii == 4) and 3 (jj == 4) are dropped, frames above 4 are renumbered
    (edge 0: jj 5 -> 4; edge 1: ii 5 -> 4, kk 10 -> 8; edge 4: (5, 5, 11) -> (4, 4, 9)), then with n' = 5 and a window of 4 the
    patches of frames < 1 go: edge 5 (patch 0 of frame 0)."""
    g = _hand_graph()
    removed, k, m, n = g.keyframe(*_still_scene(), 6, keyframe_index=2, thresh=12.5, removal_window=4)
    assert removed and k == 4 and m == 0.0 and n == 5
    assert g.ii.tolist() == [3, 4, 4, 1] and g.jj.tolist() == [4, 3, 4, 2] and g.kk.tolist() == [6, 8, 9, 3]
    assert g.net[0, :, 0].tolist() == [0, 1, 4, 6]


def test_keyframe_keep_branch_by_hand():
    """thresh below the motion: nothing is renumbered, n stays 6, and the window of 4 drops the patches of frames < 2: edges 3, 5, 6."""
    g = _hand_graph()
    removed, k, m, n = g.keyframe(*_still_scene(), 6, keyframe_index=2, thresh=-1.0, removal_window=4)
    assert not removed and k == 4 and n == 6
    assert g.ii.tolist() == [3, 5, 4, 5] and g.jj.tolist() == [5, 3, 5, 5] and g.kk.tolist() == [6, 10, 8, 11]
    assert g.net[0, :, 7].tolist() == [0, 1, 2, 4]
    # a pair without edges: NaN, and NaN < thresh is False
    g2 = _hand_graph()
    removed, _, m, n = g2.keyframe(*_still_scene(), 6, keyframe_index=5, thresh=12.5, removal_window=100)
    assert math.isnan(m) and not removed and n == 6 and len(g2.ii) == 7


def test_motionmag_by_hand():
    """A camera that steps 0.125 along x in front of points at inverse depth 0.5, fx = 80: every pixel moves fx * w * tx = 5 px, in the
    full and in the translation-only reprojection alike, so flow_mag = 5 for any beta; the reverse direction moves as far."""
    g = _hand_graph()
    poses, patches, intr = _still_scene()
    poses[0, 5, 0] = 0.125
    assert g.motionmag(poses, patches, intr, 3, 5) == pytest.approx(5.0, rel=1e-12)
    assert g.motionmag(poses, patches, intr, 5, 3) == pytest.approx(5.0, rel=1e-12)
    assert math.isnan(g.motionmag(poses, patches, intr, 2, 0))
    removed, _, m, _ = g.keyframe(poses, patches, intr, 6, keyframe_index=2, thresh=5.5, removal_window=100)
    assert removed and m == pytest.approx(5.0, rel=1e-12)
    removed, _, m, _ = _hand_graph().keyframe(poses, patches, intr, 6, keyframe_index=2, thresh=4.5, removal_window=100)
    assert not removed


def test_shift_by_hand():
    a = torch.arange(6.0)[:, None].repeat(1, 3)
    b = torch.arange(6)
    ref_shift([a, b], 2, 5)
    assert a[:, 0].tolist() == [0, 1, 3, 4, 4, 5] and b.tolist() == [0, 1, 3, 4, 4, 5]
    ref_shift([a], 4, 5)                                                # k = n - 1: nothing moves
    assert a[:, 1].tolist() == [0, 1, 3, 4, 4, 5]


def test_every_method_refuses_cpu_tensors():
    from devo_amd import graph
    g = graph.PatchGraph(M, dim=8, capacity=64, device="cpu")
    poses, patches, intr = _still_scene()
    assert len(g) == 0 and g.ii.numel() == 0 and g.net.shape == (1, 0, 8)
    for call in (lambda: g.append(torch.tensor([1]), torch.tensor([0]), IX), lambda: g.remove(torch.zeros(0, dtype=torch.bool)),
                 lambda: g.motion(poses, patches, intr, 3, 5), lambda: g.keyframe(poses, patches, intr, IX, 6),
                 lambda: graph.shift_frames([poses[0], patches[0]], 2, 5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert len(g) == 0
    with pytest.raises(ValueError):
        graph.PatchGraph(M, dim=12)                                     # rows of net move as 16-byte words
    with pytest.raises(ValueError):
        g.net = torch.zeros(1, 3, 8)                                    # not the graph's shape


def test_header_table_and_library_agree_on_abi_9():
    import ctypes
    from devo_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "devo_hip.h")).read()
    assert int(re.search(r"#define\s+DEVO_ABI_VERSION\s+(\d+)", txt).group(1)) == 9 == _lib.ABI_VERSION
    names = {"devo_graph_workspace_bytes", "devo_graph_motion", "devo_graph_keyframe", "devo_graph_remove", "devo_graph_append", "devo_graph_shift_frames"}
    declared = set(re.findall(r"\b(devo_graph_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert declared == names and names <= set(_lib.EXPORTED_SYMBOLS)
    assert "graph.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build_lib(verbose=False))
    assert lib.devo_abi_version() == 9
    for n in names:
        assert hasattr(lib, n)
    h = _lib.lib()
    assert h.devo_graph_workspace_bytes(1 << 17) >= (1 << 17) // 256 * 20
    # refused on the host, before any launch: too many tensors to one shift, an append beyond the capacity, a net that cannot move as 16-byte words
    assert h.devo_graph_shift_frames(None, None, 9, 0, 4, None) == 1
    assert h.devo_graph_append(None, None, None, None, None, None, 0, None, None, 60, 5, 64, 8, _lib.DEVO_F32, None) == 1
    assert b"capacity" in h.devo_last_error()
    assert h.devo_graph_append(None, None, None, None, None, None, 0, None, None, 1, 1, 64, 12, _lib.DEVO_F32, None) == 1
