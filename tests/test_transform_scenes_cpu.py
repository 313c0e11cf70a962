"""The scenes of tests/test_gpu_transform.py put what they promise in front of the kernels: conditions on the fp64 oracle's Z, checked on
the CPU for every patch size and seed that the GPU tests use (tests/transform_scenes.py)."""
import pytest
import torch
import transform_scenes as T


@pytest.mark.parametrize("P", [1, 3, 5])
def test_edge_scene_reaches_every_regime(P):
    s = T.edge_scene(P, T.SEED)
    T.assert_graph_conditions(s)
    r = T.regimes(s)
    print(r)
    assert r["pixels_clamped"] >= 20                       # Z < 0.1: the clamp of proj
    assert r["centres_01_02"] >= 3                         # clamp not reached, Jacobians gated off
    assert r["centres_m02_01"] >= 3                        # clamped and gated off
    assert r["centres_behind"] >= 20                       # Z < -0.2: Jacobians on, valid off
    assert r["centres_far"] >= 100
    assert r["clamp_margin"] >= 1e-3 and r["gate_margin"] >= 1e-3
    poses, patches, intrinsics, ii, jj, kk = s
    assert all(t.dtype == torch.float32 for t in (poses, patches, intrinsics))
    assert patches.shape == (1, 8 * T.M + T.N_EDGELESS, 3, P, P) and len(ii) == 384
    used = torch.zeros(T.NBUF, dtype=torch.bool)
    used[list(T.SLOTS)] = True
    assert bool((poses[0, ~used] == torch.tensor([0, 0, 0, 0, 0, 0, 1.0])).all())
    assert set(ii.tolist()) == set(T.SLOTS) == set(jj.tolist())


@pytest.mark.parametrize("P", [1, 3, 5, 7])
def test_interior_scene_stays_in_front(P):
    s, e = T.interior_scene(P, T.SEED), T.edge_scene(P if P < 7 else 5, T.SEED)
    T.assert_graph_conditions(s)
    assert T.regimes(s)["z_min"] > 0.3
    assert torch.equal(s[2], e[2]) and all(torch.equal(a, b) for a, b in zip(s[3:], e[3:]))       # the same intrinsics and graph


def test_references_are_differentiable_and_quick():
    """the oracle's gradients for a scene: finite, empty where nothing is connected"""
    gp, gq = T.gradients("edge", 3, "all")[torch.float64]
    used = torch.zeros(T.NBUF, dtype=torch.bool)
    used[list(T.SLOTS)] = True
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gq).all())
    assert float(gp[0, ~used].abs().max()) == 0.0 and float(gp[..., 6].abs().max()) == 0.0
    assert float(gq[0, -T.N_EDGELESS:].abs().max()) == 0.0 and bool((gp[0, used, :6].abs().amax(dim=1) > 0).all())
