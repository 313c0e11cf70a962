"""devo_amd.frames without a GPU: the new symbols are declared in all three places, the ABI version did not move, the fp64 restatement
tests/frames_ref.py agrees with the fixture tests/golden/frame_state_f64.npz (tools/gen_golden_frames.py: the reference's own SE3 class
and point_cloud on CPU in fp64, get_pose recursively) to 1e-10, its lower-median rule is torch.median's, and the module refuses what it
cannot run."""
import os
import re
import numpy as np
import pytest
import torch

import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("devo_frame_begin", "devo_frame_point_cloud", "devo_frame_record_removed", "devo_frame_record_skipped", "devo_frame_complete",
           "devo_frame_complete_workspace_bytes", "devo_frame_complete_launches")
TOL = 1e-10                                                             # tests/test_oracle_golden.py


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "frame_state_f64.npz"))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_are_declared_in_header_ctypes_table_and_binding():
    from devo_amd import _lib, frames                                   # noqa: F401
    header, bind = _read("include", "devo_hip.h"), _read("devo_amd", "csrc", "bind.cpp")
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\(", bind), s
    assert 'def_submodule("frames"' in bind
    assert "frames.hip" in __import__("devo_amd.build", fromlist=["SOURCES"]).SOURCES
    declared = set(re.findall(r"\b(devo_frame_\w+)\(", header))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)            # nothing declared that the table does not bind


def test_abi_version_is_still_9():
    from devo_amd import _lib, frames                                   # noqa: F401
    assert _lib.ABI_VERSION == 9
    assert re.search(r"#define DEVO_ABI_VERSION 9\b", _read("include", "devo_hip.h"))
    assert "devo_frame_begin" in _read("include", "devo_hip.h").split("int devo_abi_version")[0]      # listed in the version comment


def _close(got, want, what):
    err = float((torch.as_tensor(got) - torch.as_tensor(want)).abs().max())
    assert err <= TOL * max(1.0, float(torch.as_tensor(want).abs().max())), f"{what}: {err:.3e}"


def test_motion_model_restatement_agrees_with_the_fixture(golden):
    from devo_amd import frames                                         # noqa: F401
    P1, P2 = torch.from_numpy(golden["mm_P1"]), torch.from_numpy(golden["mm_P2"])
    want = torch.from_numpy(golden["mm_pred"])
    assert P1.shape == (4, 7) and torch.equal(P1[1], P2[1])             # the pair of identical poses ...
    half = 2 * torch.atan2(P1[2, 3:6].norm(), P1[2, 6])
    assert abs(float(half) - 0.5) < 1e-12 and float(P2[2, 3:6].norm()) == 0.0      # ... and the 0.5 rad step
    got = R.motion_model(P1, P2, float(golden["mm_damping"]))
    _close(got, want, "motion model")
    _close(got[1], P1[1], "two identical poses predict the pose")
    for a, b in zip(P1, P2):                                            # one pair at a time, as begin_frame calls it
        _close(R.motion_model(a, b, float(golden["mm_damping"])), R.motion_model(a[None], b[None], float(golden["mm_damping"]))[0], "single pair")
    assert torch.equal(R.motion_model(P1[0], P2[0], 0.5, "CONSTANT"), P1[0])


def test_point_cloud_restatement_agrees_with_the_fixture(golden):
    from devo_amd import frames                                         # noqa: F401
    d = lambda k: torch.from_numpy(golden[k])
    want = d("pc_points")
    assert want.shape == (35, 3)
    got = R.point_cloud(d("pc_poses"), d("pc_patches"), d("pc_intrinsics"), d("pc_ix"), 35)
    _close(got, want, "point cloud")
    _close(R.point_cloud(d("pc_poses"), d("pc_patches"), d("pc_intrinsics"), d("pc_ix"), 20), want[:20], "the first m patches")


def test_trajectory_restatement_agrees_with_the_fixture(golden):
    from devo_amd import frames                                         # noqa: F401
    d = lambda k: torch.from_numpy(golden[k])
    counter = int(golden["tr_counter"])
    kf_t, kf_p = d("tr_kf_tstamps"), d("tr_kf_poses")
    tr = R.RefTrajectory()
    for t, p, rel in zip(golden["tr_log_t"], golden["tr_log_parent"], d("tr_log_rel")):
        tr.delta[int(t)] = (int(p), rel)
    assert counter == 12 and tr.delta[5][0] == 4 and tr.delta[4][0] == 3 and 3 in kf_t.tolist()       # two chained removals
    got = tr.complete(kf_p, kf_t, len(kf_t), counter)
    _close(got, d("tr_out"), "trajectory")
    # the same log recorded through the restatement's own record_* calls, driven as the state machine drives them
    full = d("tr_poses_all")
    tr2, alive = R.RefTrajectory(), list(range(counter))
    tr2.record_skipped(1, 0)
    alive.remove(1)
    for t1 in (5, 4, 9):
        k = alive.index(t1)
        tr2.record_removed(full[alive], torch.tensor(alive), k)
        alive.remove(t1)
    _close(tr2.complete(full[alive], torch.tensor(alive), len(alive), counter), d("tr_out"), "trajectory through record_*")
    tr2.delta[3] = (2, torch.tensor(R.IDENTITY, dtype=torch.float64))   # precedence: a keyframe with a log entry keeps its pose
    _close(tr2.complete(full[alive], torch.tensor(alive), len(alive), counter), d("tr_out"), "precedence")
    del tr2.delta[9]
    with pytest.raises(KeyError):
        tr2.complete(full[alive], torch.tensor(alive), len(alive), counter)


@pytest.mark.parametrize("count", [1, 2, 27, 188, 189, 2592])
def test_lower_median_is_torch_median(count):
    from devo_amd import frames                                         # noqa: F401
    g = torch.Generator().manual_seed(count)
    levels = torch.linspace(-1.0, 3.0, 17)
    for trial in range(4):
        x = levels[torch.randint(0, 17 if trial < 2 else 3, (count,), generator=g)]    # ties straddle the median
        assert torch.equal(R.lower_median(x), torch.median(x))
    x = torch.randn(count, generator=g)
    assert torch.equal(R.lower_median(x), torch.median(x))


def test_begin_frame_restatement_writes_row_n_only():
    from devo_amd import frames                                         # noqa: F401
    g = torch.Generator().manual_seed(2)
    N, M, P, n = 6, 5, 3, 4
    poses = torch.randn(N, 7, generator=g, dtype=torch.float64)
    patches = torch.rand(N, M, 3, P, P, generator=g, dtype=torch.float64)
    intr, ts = torch.rand(N, 4, generator=g, dtype=torch.float64), torch.arange(N)
    before = [t.clone() for t in (poses, patches, intr, ts)]
    new = torch.rand(1, M, 3, P, P, generator=g, dtype=torch.float64)
    R.begin_frame(poses, patches, intr, ts, n, new, torch.tensor([320.0, 320.0, 320.0, 240.0], dtype=torch.float64), 17, 4.0)
    for a, b in zip((poses, patches, intr, ts), before):
        keep = torch.arange(N) != n
        assert torch.equal(a[keep], b[keep])
    assert int(ts[n]) == 17 and torch.equal(intr[n], torch.tensor([80.0, 80.0, 80.0, 60.0], dtype=torch.float64))
    assert torch.equal(patches[n, :, :2], new[0, :, :2]) and bool((patches[n, :, 2] == torch.median(before[1][1:4, :, 2])).all())
    _close(poses[n], R.motion_model(before[0][3], before[0][2]), "pose row")


def test_frames_refuse_cpu_tensors():
    from devo_amd import frames
    N, M, P = 6, 5, 3
    poses, patches, intr, ts = torch.zeros(N, 7), torch.zeros(N, M, 3, P, P), torch.ones(N, 4), torch.zeros(N, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.begin_frame(poses, patches, intr, ts, 4, torch.zeros(1, M, 3, P, P), torch.ones(4), 4, 4.0)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.point_cloud(poses, patches, intr, torch.zeros(N * M, dtype=torch.int64), N * M, torch.zeros(N * M, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        frames.Trajectory(16, device="cpu")
    assert frames.MEDIAN_MAX == 32768 and re.search(r"#define DEVO_FRAME_MEDIAN_MAX 32768\b", _read("include", "devo_hip.h"))
