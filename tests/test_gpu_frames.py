"""devo_amd.frames (csrc/frames.hip) against the fp64 restatement tests/frames_ref.py (pinned to the reference by
tests/golden/frame_state_f64.npz, test_frames_cpu.py).  fp32 geometry against the fp64 restatement at 1e-4 relative, the project's
standing tolerance (test_gpu_patch_graph.py): translations relative to 1 + |t|, quaternions absolute after aligning the sign,
points relative to the point's norm.  Integers and copied or selected values BIT for bit.  Shapes are the smallest at which the kernels
take another path: median counts 27 / 189 / 2592 / 6939 (odd and even, below and above one wave, above 4096 = more than four keys per
thread), point clouds of 63 and 624 patches, trajectories of 1 .. 3000 frames (a chain of depth 2999: twelve rounds, twelve workgroups)."""
import math
import os
import subprocess
import sys
import pytest
import torch
from devo_amd import synth
import frames_ref as R
from patch_graph_ref import RefGraph, shift_frames as ref_shift

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, P = 120, 160, 3
TOL = 1e-4


def _d(*ts):
    return [t.to(DEV) for t in ts]


def _pose_err(got, want):
    """(translation error relative to 1 + |t|, absolute quaternion error after aligning the sign), the worst over the rows."""
    got, want = got.double().cpu().reshape(-1, 7), want.double().reshape(-1, 7)
    et = (got[:, :3] - want[:, :3]).norm(dim=-1) / (1 + want[:, :3].norm(dim=-1))
    s = torch.sign((got[:, 3:] * want[:, 3:]).sum(-1, keepdim=True))
    eq = (got[:, 3:] - s * want[:, 3:]).abs().amax(dim=-1)
    return float(et.max()), float(eq.max())


def _assert_pose(got, want, what):
    et, eq = _pose_err(got, want)
    print(f"{what}: translation {et:.3e}, quaternion {eq:.3e}")
    assert et <= TOL and eq <= TOL, what


# ------------------------------------------------------------------------------------------------ begin_frame
_LEVELS = torch.linspace(0.125, 2.125, 17)


def _buffers(N, M, seed, depth_levels=_LEVELS, poses=None):
    g = torch.Generator().manual_seed(seed)
    poses = synth.make_poses(N, seed, trans_step=0.05, rot_step=0.01)[0] if poses is None else poses
    patches = synth.make_patches(N, M, H, W, seed=seed)[0].view(N, M, 3, P, P).clone()
    patches[:, :, 2] = depth_levels[torch.randint(0, len(depth_levels), (N, M, P, P), generator=g)]
    intr = synth.make_intrinsics(N, H, W)[0].clone()
    ts = torch.arange(100, 100 + N)
    new = synth.make_patches(1, M, H, W, seed=seed + 7)[0]
    return poses.contiguous(), patches, intr, ts, new, g


def _begin(bufs, n, depth="median", model="DAMPED_LINEAR", res=4.0, counter=1234567890123, views=False):
    """Run frames.begin_frame and the restatement on the same values -> (device buffers, fp32 CPU buffers the restatement edited)."""
    from devo_amd import frames
    poses, patches, intr, ts, new, _ = bufs
    K = torch.tensor([321.5, 319.25, 317.0, 243.0])
    dev = _d(poses, patches, intr, ts)
    args = [t[None] for t in dev] if views else dev
    if views:
        args[1] = dev[1].view(1, -1, 3, P, P)
    frames.begin_frame(*args, n, new.to(DEV), K.to(DEV), counter, res, motion_model=model, damping=0.5, depth=depth if isinstance(depth, str) else depth.to(DEV))
    ref = [t.clone() for t in (poses, patches, intr, ts)]
    R.begin_frame(*ref, n, new, K, counter, res, model, 0.5, depth)      # fp32 on the CPU: the copied and selected values, torch.median, torch's division
    return dev, ref


@pytest.mark.parametrize("M", [1, 7, 96, 257])
def test_begin_frame_median_depth_and_store(M):
    N, n = 8, 5
    bufs = _buffers(N, M, 40 + M)
    dev, ref = _begin(bufs, n, views=(M == 7))
    got = [t.cpu() for t in dev]
    want_med = torch.median(bufs[1][n - 3:n, :, 2])                      # on the CPU, from the same values
    levels = bufs[1][n - 3:n, :, 2].reshape(-1)
    assert levels.numel() == 27 * M and (M == 1 or ((levels < want_med).any() and (levels > want_med).any() and (levels == want_med).sum() > 1))
    assert torch.equal(got[1][n, :, 2], want_med.expand(M, P, P)), f"median {float(got[1][n, 0, 2, 0, 0])} against torch.median {float(want_med)}"
    assert torch.equal(got[1][n, :, :2], bufs[4][0, :, :2])
    assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])      # whole tensors: every other row unchanged
    assert int(got[3][n]) == 1234567890123
    keep = torch.arange(N) != n
    assert torch.equal(got[0][keep], bufs[0][keep])
    _assert_pose(got[0][n], R.motion_model(bufs[0][n - 1].double(), bufs[0][n - 2].double()), f"pose row, M = {M}")


def test_begin_frame_median_with_negative_values_and_zeros():
    levels = torch.tensor([-2.5, -1.0, -0.25, 0.0, 0.0, 0.0, 0.5, 1.0, 3.0])
    for seed, M in ((3, 7), (4, 8), (5, 96)):
        bufs = _buffers(6, M, seed, depth_levels=levels)
        dev, ref = _begin(bufs, 3)
        assert torch.equal(dev[1].cpu(), ref[1]), (seed, M)
    bufs = _buffers(6, 7, 9, depth_levels=torch.tensor([-3.0, -2.0, -1.0]))       # all negative
    dev, ref = _begin(bufs, 4)
    assert torch.equal(dev[1].cpu(), ref[1])


def test_begin_frame_intrinsics_division_is_true_division():
    for res in (4.0, 3.0, 0.7):
        bufs = _buffers(5, 3, 6)
        dev, ref = _begin(bufs, 3, res=res)
        assert torch.equal(dev[2].cpu(), ref[2]), res


def test_begin_frame_depth_per_patch():
    M, N = 24, 5
    bufs = _buffers(N, M, 8)
    depth = torch.rand(M, generator=bufs[5])
    for n in (0, 1, 2, 4):                                               # before initialisation: no median, any n
        dev, ref = _begin(bufs, n, depth=depth)
        got = [t.cpu() for t in dev]
        assert torch.equal(got[1][n, :, 2], depth[:, None, None].expand(M, P, P))
        assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
        if n <= 1:
            assert torch.equal(got[0], bufs[0])                          # n = 1: the pose row is left untouched
        else:
            _assert_pose(got[0][n], R.motion_model(bufs[0][n - 1].double(), bufs[0][n - 2].double()), f"pose row n = {n}")


@pytest.mark.parametrize("n", [2, 9])
def test_motion_model_cases(n):
    from devo_amd import frames                                          # noqa: F401
    N, M = 12, 3
    base = synth.make_poses(N, 77, trans_step=0.05, rot_step=0.01)[0]
    half = torch.tensor([0.2, -0.1, 0.4, 0.0, math.sin(0.25), 0.0, math.cos(0.25)])
    cases = {"smooth": base, "identical": base.clone(), "half_rad": base.clone()}
    cases["identical"][n - 2] = cases["identical"][n - 1]
    cases["half_rad"][n - 2] = torch.tensor(R.IDENTITY)
    cases["half_rad"][n - 1] = half
    depth = torch.full((M,), 0.5)
    for name, poses in cases.items():
        bufs = _buffers(N, M, 1, poses=poses.clone())
        dev, _ = _begin(bufs, n, depth=depth)
        got = dev[0].cpu()
        want = R.motion_model(poses[n - 1].double(), poses[n - 2].double())
        _assert_pose(got[n], want, f"{name}, n = {n}")
        keep = torch.arange(N) != n
        assert torch.equal(got[keep], poses[keep])
        if name == "identical":
            _assert_pose(got[n], poses[n - 1].double(), "two identical poses predict the pose")
        dev, _ = _begin(bufs, n, depth=depth, model="CONSTANT")
        assert torch.equal(dev[0].cpu()[n], poses[n - 1]) and torch.equal(dev[0].cpu()[keep], poses[keep])       # bit for bit


def test_begin_frame_refuses_a_count_above_the_bound_and_bad_arguments():
    from devo_amd import frames
    M = frames.MEDIAN_MAX // 27 + 1                                      # 1214 patches: 32 778 depth values
    N, n = 5, 3
    poses, intr, ts = torch.randn(N, 7), torch.rand(N, 4) + 1, torch.arange(N)
    patches, new = torch.rand(N, M, 3, P, P), torch.rand(1, M, 3, P, P)
    dev = _d(poses, patches, intr, ts)
    with pytest.raises(RuntimeError, match="exceeds the supported"):
        frames.begin_frame(*dev, n, new.to(DEV), torch.ones(4, device=DEV), 7, 4.0)
    torch.cuda.synchronize()
    for a, b in zip(dev, (poses, patches, intr, ts)):
        assert torch.equal(a.cpu(), b)                                   # nothing was launched
    frames.begin_frame(*dev, n, new.to(DEV), torch.ones(4, device=DEV), 7, 4.0, depth=torch.rand(M, device=DEV))       # the [M] mode has no bound
    assert torch.equal(dev[1][n, :, :2].cpu(), new[0, :, :2])
    small = _d(*_buffers(5, 3, 2)[:4])
    newp = torch.rand(1, 3, 3, P, P, device=DEV)
    with pytest.raises(ValueError):
        frames.begin_frame(*small, 2, newp, torch.ones(4, device=DEV), 7, 4.0)                 # the median needs three frames
    with pytest.raises(ValueError):
        frames.begin_frame(*small, 5, newp, torch.ones(4, device=DEV), 7, 4.0)                 # row 5 of 5
    with pytest.raises(ValueError):
        frames.begin_frame(small[0].double(), *small[1:], 3, newp, torch.ones(4, device=DEV), 7, 4.0)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.begin_frame(*small, 3, newp.cpu(), torch.ones(4, device=DEV), 7, 4.0)


# ------------------------------------------------------------------------------------------------ point cloud
_scenes = {}


def _scene(n, M, seed=11):
    if (n, M) not in _scenes:
        nbuf = n + 2
        poses = synth.make_poses(nbuf, seed, trans_step=0.05, rot_step=0.02)
        patches, _ = synth.make_patches(nbuf, M, H, W, seed=seed)
        intr = synth.make_intrinsics(nbuf, H, W).clone()
        intr[0] *= 1 + 0.01 * torch.arange(nbuf)[:, None]               # every frame its own intrinsics
        ix = torch.arange(nbuf * M) // M
        want = R.point_cloud(poses.double(), patches.double(), intr.double(), ix, n * M)
        from oracle import pops
        full = pops.point_cloud(pops.SE3(poses.double()), patches.double()[:, :n * M], intr.double(), ix[:n * M])
        orc = (full[..., P // 2, P // 2, :3] / full[..., P // 2, P // 2, 3:]).reshape(-1, 3)
        assert float((want - orc).abs().max()) <= 1e-10 * float(orc.abs().max())
        _scenes[(n, M)] = (poses, patches, intr, ix, orc)
    return _scenes[(n, M)]


@pytest.mark.parametrize("n,M", [(9, 7), (26, 24)])
def test_point_cloud_matches_the_fp64_oracle(n, M):
    from devo_amd import frames
    poses, patches, intr, ix, want = _scene(n, M)
    m = n * M
    Pd, Qd, Kd, IX = _d(poses, patches, intr, ix)
    for start in (0, 3):
        out = torch.full(((n + 2) * M, 3), -12345.0, device=DEV)
        frames.point_cloud(Pd, Qd, Kd, IX, m, out, start_frame=start)
        got = out.cpu()
        assert bool((got[m:] == -12345.0).all()) and bool((got[:start * M] == -12345.0).all())
        rel = (got[start * M:m].double() - want[start * M:]).norm(dim=-1) / want[start * M:].norm(dim=-1)
        print(f"point cloud ({n}, {M}) start {start}: worst relative error {float(rel.max()):.3e}")
        assert float(rel.max()) <= TOL
    out2 = torch.full((m, 3), -12345.0, device=DEV)                     # the [N, M, 3, P, P] / [N, 7] forms of the same buffers; out of exactly m rows
    frames.point_cloud(Pd[0], Qd[0].view(n + 2, M, 3, P, P), Kd[0], IX, m, out2)
    frames.point_cloud(Pd, Qd, Kd, IX, m, out)
    assert torch.equal(out2, out[:m])
    frames.point_cloud(Pd, Qd, Kd, IX, m, out2, start_frame=n)          # nothing to do
    assert torch.equal(out2, out[:m])
    with pytest.raises(ValueError):
        frames.point_cloud(Pd, Qd, Kd, IX, m, out[:m - 1])


# ------------------------------------------------------------------------------------------------ trajectory
def _forest(counter, keyframes, parents, seed):
    """A log over `counter` frames: frame t not in `keyframes` has parent parents[t] < t and a random relative pose.
    -> (kf poses [n, 7], kf tstamps [n], {t: (parent, rel)}) in fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    ax = torch.randn(counter, 3, generator=g)
    ang = 0.05 * torch.randn(counter, 1, generator=g)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    rel = torch.cat([0.1 * torch.randn(counter, 3, generator=g), torch.sin(ang / 2) * ax, torch.cos(ang / 2)], -1)
    kf = sorted(keyframes)
    poses = synth.make_poses(len(kf), seed, trans_step=0.05, rot_step=0.01)[0]
    return poses, torch.tensor(kf, dtype=torch.int64), {t: (int(parents[t]), rel[t]) for t in range(counter) if t not in keyframes}


def _run_forest(counter, poses, tstamps, log, capacity=None, extra_rows=2):
    from devo_amd import frames
    n = len(tstamps)
    tr = frames.Trajectory(capacity or counter, DEV)
    parent = torch.full((tr.capacity,), -1, dtype=torch.int64)
    rel = torch.zeros(tr.capacity, 7)
    ref = R.RefTrajectory()
    for t, (p, x) in log.items():
        parent[t], rel[t] = p, x
        ref.delta[t] = (p, x.double())
    tr.parent.copy_(parent)
    tr.rel.copy_(rel)
    Pb = torch.cat([poses, torch.full((extra_rows, 7), float("nan"))])   # rows >= n are never read
    Tb = torch.cat([tstamps, torch.full((extra_rows,), -7, dtype=torch.int64)])
    got = tr.complete(Pb.to(DEV), Tb.to(DEV), n, counter)
    assert got.shape == (counter, 7) and got.dtype == torch.float32 and got.is_cuda
    return got, ref.complete(poses.double(), tstamps, n, counter), tr


def test_trajectory_small_cases():
    from devo_amd import frames
    for counter, removed in ((1, set()), (5, set()), (64, set(range(1, 64, 2))), (65, set(range(1, 65, 2)))):
        kf = set(range(counter)) - removed
        poses, ts, log = _forest(counter, kf, {t: t - 1 for t in removed}, counter)
        got, want, _ = _run_forest(counter, poses, ts, log, capacity=counter + 3)
        _assert_pose(got, want, f"counter {counter}, {len(removed)} logged")
        assert frames.Trajectory.launches(counter) == 1 + math.ceil(math.log2(counter)) <= 2 + math.ceil(math.log2(counter))


def test_trajectory_random_forest():
    counter = 1000
    g = torch.Generator().manual_seed(5)
    kf = {0} | {int(t) for t in torch.nonzero(torch.rand(counter, generator=g) < 0.3).flatten()}
    parents = {t: int(torch.randint(0, t, (1,), generator=g)) for t in range(1, counter)}
    poses, ts, log = _forest(counter, kf, parents, 6)
    got, want, _ = _run_forest(counter, poses, ts, log)
    _assert_pose(got, want, "random forest of 1000 frames")


def test_trajectory_chain_of_depth_2999():
    from devo_amd import frames
    counter = 3000
    poses, ts, log = _forest(counter, {0}, {t: t - 1 for t in range(1, counter)}, 7)
    got, want, _ = _run_forest(counter, poses, ts, log)
    assert frames.Trajectory.launches(counter) == 13                    # 12 rounds: more than 11
    _assert_pose(got, want, "a single chain of depth 2999")


def test_trajectory_precedence_and_missing_frames():
    from devo_amd import frames
    counter = 20
    removed = {3, 4, 9, 15}
    poses, ts, log = _forest(counter, set(range(counter)) - removed, {t: t - 1 for t in range(counter)}, 8)
    full_log = dict(log)
    for t in (5, 10):                                                    # keyframes that ALSO have a log entry: the keyframe pose wins
        full_log[t] = (t - 1, torch.tensor([0.3, 0.2, 0.1, 0.0, 0.0, 0.0, 1.0]))
    got, want, _ = _run_forest(counter, poses, ts, full_log)
    plain, _, _ = _run_forest(counter, poses, ts, log)
    _assert_pose(got, want, "precedence")
    assert torch.equal(got, plain)
    del full_log[9]                                                      # frame 9: neither a keyframe nor logged
    with pytest.raises(RuntimeError, match="neither a keyframe"):
        _run_forest(counter, poses, ts, full_log)
    tr = frames.Trajectory(8, DEV)
    with pytest.raises(RuntimeError, match="capacity"):
        tr.complete(poses.to(DEV), ts.to(DEV), 2, 9)
    with pytest.raises(RuntimeError, match="capacity"):
        tr.record_skipped(8, 7)
    tr.record_skipped(2, 1)                                              # frames 0, 1 keyframes, 2 skipped
    out = tr.complete(poses.to(DEV), torch.tensor([0, 1], device=DEV), 2, 3)
    assert torch.allclose(out[2], out[1], rtol=0, atol=1e-6)            # the identity: the parent's pose
    with pytest.raises(RuntimeError, match="strictly increasing"):
        tr.complete(poses.to(DEV), torch.tensor([1, 0], device=DEV), 2, 3)
    out2 = tr.complete(poses.to(DEV), torch.tensor([0, 1], device=DEV), 2, 3)      # the status word was cleared by the raise
    assert torch.equal(out2, out)


def test_record_removed_through_the_pipeline_without_host_reads(monkeypatch):
    """The "odd" / "small" scene of test_gpu_patch_graph.py (n 9, M 7, camera steps 0.01 / 0.002, restated here): PatchGraph.keyframe reports
    `removed`, then record_removed, shift_frames and complete run with Tensor.item forbidden, against the restatement driven the same way."""
    from devo_amd import frames, graph
    n, M, seed, nbuf = 9, 7, 11, 11
    poses = synth.make_poses(nbuf, seed, trans_step=0.01, rot_step=0.002)
    patches, _ = synth.make_patches(nbuf, M, H, W, seed=seed)
    intr = synth.make_intrinsics(nbuf, H, W)
    ii, jj, kk = synth.sliding_window_graph(n, M)
    ix = torch.arange(nbuf * M) // M
    counter = 14
    live = [0, 1, 3, 4, 6, 7, 8, 10, 12]                                 # the timestamps of the 9 live frames; 2, 5, 9, 11, 13 were skipped
    tstamps = torch.tensor(live + [0] * (nbuf - n), dtype=torch.int64)
    g = graph.PatchGraph(M, dim=8, capacity=1 << 12, device=DEV, dtype=torch.float16)
    g.append(kk.to(DEV), jj.to(DEV), ix.to(DEV))
    ref = RefGraph(M, 8, ix, torch.float16)
    ref.append_factors(kk, jj)
    tr, rt = frames.Trajectory(counter, DEV), R.RefTrajectory()
    for t in sorted(set(range(counter)) - set(live)):
        tr.record_skipped(t, t - 1)
        rt.record_skipped(t, t - 1)
    Pd, Qd, Kd, IX, Td = _d(poses, patches, intr, ix, tstamps)
    removed, k, _, _ = ref.keyframe(poses, patches, intr, n)
    r = g.keyframe(Pd, Qd, Kd, IX, n)
    assert r.removed and removed and r.k == k == 5

    def forbidden(self, *a, **kw):
        raise AssertionError("a host read between keyframe() and complete()")
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", forbidden)
        mp.setattr(torch.Tensor, "cpu", forbidden)
        tr.record_removed(Pd, Td, r.k)                                   # before the shift
        graph.shift_frames([Pd[0], Qd[0].view(nbuf, M, 3, P, P), Kd[0], Td], r.k, n)
        got = tr.complete(Pd, Td, n - 1, counter)
    p64, t_ref = poses[0].double().clone(), tstamps.clone()
    rt.record_removed(p64, t_ref, k)
    ref_shift([p64, t_ref], k, n)
    assert torch.equal(Td.cpu(), t_ref) and int(tr.parent[live[5]]) == live[4]
    want = rt.complete(p64, t_ref, n - 1, counter)
    _assert_pose(got, want, "record_removed, shift_frames, complete")


# ------------------------------------------------------------------------------------------------ both bindings
_LEG = r"""
import sys, os, torch
sys.path.insert(0, sys.argv[1])
from devo_amd import synth, frames
import devo_amd.backends as B
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
dev = "cuda"
out = {}
N, M, P, H, W = 12, 24, 3, 120, 160
poses = synth.make_poses(N, 3)[0].contiguous().to(dev)
patches = synth.make_patches(N, M, H, W, seed=3)[0].view(N, M, 3, P, P).contiguous().to(dev)
intr = synth.make_intrinsics(N, H, W)[0].contiguous().to(dev)
ts = torch.arange(0, 2 * N, 2, device=dev)
new = synth.make_patches(1, M, H, W, seed=4)[0].to(dev)
K = torch.tensor([320.0, 321.0, 322.0, 243.0], device=dev)
frames.begin_frame(poses, patches, intr, ts, 9, new, K, 18, 3.0)
frames.begin_frame(poses, patches, intr, ts, 10, new, K, 20, 4.0, motion_model="CONSTANT", depth=torch.linspace(0.1, 1, M, device=dev))
out.update(poses=poses, patches=patches, intr=intr, ts=ts)
ix = torch.arange(N * M, device=dev) // M
pts = torch.zeros(N * M, 3, device=dev)
frames.point_cloud(poses, patches, intr, ix, 11 * M, pts)
frames.point_cloud(poses, patches, intr, ix, 11 * M, pts, start_frame=9)
out["points"] = pts
tr = frames.Trajectory(32, dev)
for t in range(1, 22, 2):
    tr.record_skipped(t, t - 1)
tr.record_removed(poses, ts, 4)                 # frame 8 goes: parent 6
ts2, poses2 = torch.cat([ts[:4], ts[5:]]).contiguous(), torch.cat([poses[:4], poses[5:]]).contiguous()
out["trajectory"] = tr.complete(poses2, ts2, 10, 21)
out.update(parent=tr.parent, rel=tr.rel)
torch.cuda.synchronize()
torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
"""


def test_both_bindings_return_the_same_bits(tmp_path):
    from devo_amd import frames                                          # noqa: F401
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, root, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res.append(torch.load(path))
    a, b = res
    assert a.keys() == b.keys() and len(a) == 8
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(a[k], b[k]), f"{k}: the two bindings disagree"
    assert bool(torch.isfinite(a["trajectory"]).all()) and bool(torch.isfinite(a["points"][:11 * 24]).all())
    assert int(a["parent"][8]) == 6 and int(a["ts"][9]) == 18 and int(a["ts"][10]) == 20
