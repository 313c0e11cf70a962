"""odometry.DEVO against tests/odometry_ref.py's ReferenceTracker (devo/devo.py's control flow in eager torch over the package's drop-in
entry points): one network, the same frames, the same seeds, one tracker after the other.

Decisions are FORCED, so no outcome sits near a threshold: the per-call `scale` makes the motion probe reject the first three candidate
frames (1e3: threshold 1e6) and accept every later one (1e-3: threshold 1e-6); KEYFRAME_THRESH = 1e9 makes every keyframe test remove,
KEYFRAME_THRESH = 0 none — then n grows past `mem`, the rings wrap and the removal window bites.  The integer state (n, m, counter, stamps,
the edge lists, index_, the early returns) is compared exactly after every frame.  The float state (poses_[:n], the patch depths,
points_[:m], terminate()'s poses) may deviate by 8 D, D being the restatement's OWN sensitivity: its largest deviation in that quantity
between a run on the frames and a run on the frames multiplied by 1 + 2^-22 — under "std" that changes nothing but roundings.  The tracker
differs from the restatement in four places of rounding size (normalisation statistics, motion model, fused lookup call, point cloud)
against the yardstick's one; the remaining factor 2 covers the spread between the two configurations.  D is computed here, at run time,
from the restatement alone (the values seen on an MI355X are in DESIGN.md 3.19).

Conditioning.  points = X / d, and the adjustment clamps the inverse depth d at 1e-4 from below: a patch that ends a little above the clamp
turns a depth change of 1e-5 into a point change of 1e2, and the restatement run twice on IDENTICAL frames already differs by that much
(points 4.5e2 and 6.1e1 in the two configurations at sequence seed 5, with 18 and 9 depth values inside the decade above the clamp) — a
maximum over such a patch measures nothing.  So the sequence seed is one at which the restatement leaves no depth value in (1e-4, 1e-3) at
any frame of either configuration (seeds 0-13 were looked at with the restatement alone: 1, 7 and 12 qualify; 7 keeps every free depth
above 2e-2), and the fixture asserts that from the restatement's own state before anything is compared."""
import numpy as np
import pytest
import torch

from odometry_ref import ReferenceTracker

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, BINS, FRAMES, STEP = 128, 160, 5, 24, 3
FLOATS = ("poses", "depths", "points")


def _cfg(**kw):
    from devo_amd import odometry
    base = dict(BUFFER_SIZE=64, PATCHES_PER_FRAME=16, PATCH_LIFETIME=4, OPTIMIZATION_WINDOW=4, REMOVAL_WINDOW=6, MIXED_PRECISION=False)
    base.update(kw)
    return odometry.Config(**base)


@pytest.fixture(scope="module")
def network():
    from devo_amd.training import TrainNet
    torch.manual_seed(0)
    net = TrainNet(p=3, dim=384).to(DEV).eval()
    with torch.no_grad():
        for p in net.update.parameters():
            if p.dim() == 2 and p.shape[0] == 2:
                p.mul_(0.05)                                             # small flow updates: the adjustment stays in its basin
    return net


def _sequence(frames=FRAMES, density=0.3, seed=7):
    """A sparse texture sliding under the camera: STEP pixels per frame in x, one in y every other frame."""
    g = torch.Generator().manual_seed(seed)
    tex = torch.randn(BINS, H + frames, W + STEP * frames, generator=g)
    tex = tex * (torch.rand(tex.shape, generator=g) < density)
    K = torch.tensor([160.0, 160.0, W / 2, H / 2], device=DEV)
    return [(tex[:, i // 2:i // 2 + H, STEP * i:STEP * i + W].contiguous().to(DEV), K, 1e4 * i) for i in range(frames)]


def _scales(frames):
    return [1e3 if i in (1, 2, 3) else 1e-3 for i in range(frames)]     # frame 0 has no probe: frames 1-3 are the first three candidates


def _snapshot(t):
    g = getattr(t, "graph", t)
    n, m = t.n, t.m
    return dict(n=n, m=m, counter=t.counter, tlist=list(t.tlist), skipped=list(t.skipped), tstamps=t.tstamps_[:n].cpu(), ii=g.ii.cpu().clone(), jj=g.jj.cpu().clone(),
                kk=g.kk.cpu().clone(), index=t.index_.cpu().clone(), index_map=t.index_map_.cpu().clone(), net_rows=g.net.shape[1], colors=t.colors_[:n + 1].cpu().clone(),
                poses=t.poses_[:n].cpu().clone(), depths=t.patches_[:n, :, 2].cpu().clone(), points=t.points_[:m].cpu().clone())


def _drive(tracker, seq, scales, factor=None):
    snaps = []
    for i, (v, K, ts) in enumerate(seq):
        torch.manual_seed(i)
        tracker(ts, v if factor is None else v * factor, K, scale=scales[i])
        snaps.append(_snapshot(tracker))
    np.random.seed(0)
    poses, stamps = tracker.terminate()
    return snaps, np.asarray(poses, dtype=np.float64), stamps, getattr(tracker, "log", None)


def _same_integers(a, b, what):
    assert len(a) == len(b)
    for f, (x, y) in enumerate(zip(a, b)):
        for k in ("n", "m", "counter", "tlist", "skipped", "net_rows"):
            assert x[k] == y[k], (what, f, k, x[k], y[k])
        for k in ("tstamps", "ii", "jj", "kk", "index", "index_map", "colors"):
            assert torch.equal(x[k], y[k]), (what, f, k)


def _deviation(a, b):
    """The largest deviation per float quantity over all frames (NaN counts as infinite)."""
    d = {}
    for k in FLOATS:
        worst = 0.0
        for x, y in zip(a, b):
            if x[k].numel():
                e = float((x[k].double() - y[k].double()).abs().max())
                worst = float("inf") if e != e else max(worst, e)
        d[k] = worst
    return d


def _compare(network, cfg, seq, scales, what, mem=8):
    from devo_amd import odometry
    base = _drive(ReferenceTracker(cfg, network, ht=H, wd=W, mem=mem), seq, scales)
    moved = _drive(ReferenceTracker(cfg, network, ht=H, wd=W, mem=mem), seq, scales, factor=1.0 + 2.0 ** -22)
    got = _drive(odometry.DEVO(cfg, network, ht=H, wd=W, mem=mem), seq, scales)
    _same_integers(base[0], moved[0], what + ": the yardstick's two runs")
    _same_integers(got[0], base[0], what)
    D = _deviation(base[0], moved[0])
    D["terminate"] = float(np.abs(base[1] - moved[1]).max()) if base[1].size else 0.0
    dev = _deviation(got[0], base[0])
    dev["terminate"] = float(np.abs(got[1] - base[1]).max()) if base[1].size else 0.0
    assert got[1].shape == base[1].shape == (base[0][-1]["counter"], 7) and np.array_equal(got[2], base[2]) and got[2].dtype == np.float64
    for k in FLOATS + ("terminate",):
        print(f"{what}: {k}: tracker - restatement {dev[k]:.3e}, D {D[k]:.3e}, ratio {dev[k] / D[k] if D[k] > 0 else float('nan'):.2f}")
    return dev, D, base, got


def _near_clamp(snaps):
    """Patches whose inverse depth lies within a decade above the adjustment's lower clamp of 1e-4, at any frame: there points = X / d turns
    rounding noise of the depth into deviations of 1e2, in the restatement's own runs as much as in the tracker's (a depth AT the clamp is
    pinned and harmless)."""
    worst = 0
    for s in snaps:
        d = s["depths"].reshape(-1)
        worst = max(worst, int(((d > 1.001e-4) & (d < 1e-3)).sum()))
    return worst


@pytest.fixture(scope="module")
def runs(network):
    """Both configurations once: (deviation, D, the restatement's log) per keyframe threshold."""
    seq, scales, out = _sequence(), _scales(FRAMES), {}
    for name, thresh in (("remove", 1e9), ("keep", 0.0)):
        dev, D, base, got = _compare(network, _cfg(KEYFRAME_THRESH=thresh), seq, scales, name)
        assert _near_clamp(base[0]) == 0, name                         # the scene is well conditioned, by the restatement's own state
        out[name] = dict(dev=dev, D=D, log=base[3], base=base, got=got)
    return out


def test_the_forced_decisions_all_occurred(runs):
    logs = {k: v["log"] for k, v in runs.items()}
    kf = {k: [e for e in log if e[0] == "keyframe"] for k, log in logs.items()}
    # both keyframe outcomes.  Under 1e9 every test that HAS a motion removes: with a patch lifetime of 4 the frame pair (k - 1, k + 1) shares no
    # edge right after two removals in a row, its motion is a mean over nothing (NaN) and NaN < thresh keeps the frame, in the reference too
    assert any(e[4] for e in kf["remove"]) and all(e[4] for e in kf["remove"] if e[2] == e[2]) and not any(e[4] for e in kf["remove"] if e[2] != e[2])
    assert kf["keep"] and not any(e[4] for e in kf["keep"])
    for name, log in logs.items():
        probes = [e for e in log if e[0] == "probe"]
        assert [e[4] for e in probes[:3]] == [True] * 3 and not any(e[4] for e in probes[3:]), name      # three rejections, then none
        assert all(e[2] < 1e-3 * e[3] for e in probes[:3]) and all(e[2] > 1e3 * e[3] for e in probes[3:])  # nowhere near the threshold
        assert any(e[0] == "ring_wrap" for e in log), name
        assert not any(e[0] == "ba_failed" for e in log), name
    assert any(e[0] == "removal_window" and e[4] for e in logs["keep"])                           # the removal window cut edges
    last = runs["keep"]["base"][0][-1]
    assert last["n"] > 8 and last["n"] == FRAMES - 3 and runs["remove"]["base"][0][-1]["n"] < last["n"]      # n grew past mem / removals held it back
    assert runs["keep"]["base"][0][3]["n"] == 1 and runs["keep"]["base"][0][3]["counter"] == 4      # a frozen n while the probe rejects


@pytest.mark.parametrize("name", ["remove", "keep"])
@pytest.mark.parametrize("quantity", FLOATS + ("terminate",))
def test_float_state_is_within_eight_times_the_restatements_sensitivity(runs, name, quantity):
    """The integer state was compared exactly, frame by frame, when the fixture ran."""
    dev, D = runs[name]["dev"][quantity], runs[name]["D"][quantity]
    assert np.isfinite(D) and np.isfinite(dev)
    assert dev <= 8.0 * D, (name, quantity, dev, D)


def test_first_frame_below_the_density_gate_is_skipped_by_both(network):
    from devo_amd import odometry
    seq = _sequence(frames=2, density=0.01)
    assert float((seq[0][0] != 0).float().mean()) < 2e-2
    cfg = _cfg()
    for t in (ReferenceTracker(cfg, network, ht=H, wd=W, mem=8), odometry.DEVO(cfg, network, ht=H, wd=W, mem=8)):
        assert t(seq[0][2], seq[0][0], seq[0][1]) is None
        assert t.counter == 0 and t.n == 0 and t.tlist == [] and t.skipped == [seq[0][2]]
        np.random.seed(0)
        poses, stamps = t.terminate()
        assert poses.shape == (0, 7) and stamps.shape == (0,)


@pytest.mark.parametrize("norm", ["rescale", "none"])
def test_other_normalisations_for_eight_frames(network, norm):
    """Every probe accepted: the eighth frame initialises, so the twelve updates run on inputs of this normalisation."""
    seq = _sequence(frames=8)
    dev, D, base, _ = _compare(network, _cfg(NORM=norm), seq, [1e-3] * 8, norm)
    assert base[0][-1]["n"] == 8 and base[1].shape == (8, 7)
    for k in FLOATS + ("terminate",):
        assert np.isfinite(dev[k]) and dev[k] <= 8.0 * D[k], (norm, k, dev[k], D[k])


def test_mixed_precision_rings_and_a_growing_log(network):
    """The default precision: fp16 channel-blocked rings written by build_pyramid(..., slot=), the fp16 recurrent state, lookup and operator
    under autocast — against the restatement at the same setting (NCHW fp16 rings, avg_pool2d), past initialisation, across ring wraps and
    keyframe removals, with slot copies of blocked rings.  BUFFER_SIZE = 13 is below the 14 frames, so the relative-pose log doubles on
    the way and terminate() reads through the grown one."""
    seq = _sequence(frames=14)
    cfg = _cfg(MIXED_PRECISION=True, KEYFRAME_THRESH=1e9, BUFFER_SIZE=13)
    dev, D, base, got = _compare(network, cfg, seq, [1e-3] * 14, "fp16")
    log = base[3]
    assert any(e[0] == "ring_wrap" for e in log) and any(e[0] == "keyframe" and e[4] for e in log) and base[0][-1]["counter"] == 14 > cfg.BUFFER_SIZE
    assert base[1].shape == (14, 7)
    for k in FLOATS + ("terminate",):
        assert np.isfinite(dev[k]) and dev[k] <= 8.0 * D[k], ("fp16", k, dev[k], D[k])


def test_a_sequence_that_never_initialises(network):
    from devo_amd import odometry
    seq = _sequence(frames=5)
    outs = []
    for t in (ReferenceTracker(_cfg(), network, ht=H, wd=W, mem=8), odometry.DEVO(_cfg(), network, ht=H, wd=W, mem=8)):
        snaps, poses, stamps, _ = _drive(t, seq, [1e3] * 5)
        assert not t.is_initialized and t.n == 1 and t.counter == 5 and len(t.skipped) == 4
        assert poses.shape == (5, 7) and np.abs(poses[:, :3]).max() < 0.1 and np.array_equal(poses[:, 3:], np.tile([0.0, 0.0, 0.0, 1.0], (5, 1)))
        outs.append((poses, stamps))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])      # the same np.random draw (devo.py:201)


def test_cpu_tensors_raise(network):
    from devo_amd import odometry
    t = odometry.DEVO(_cfg(), network, ht=H, wd=W, mem=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(0.0, torch.zeros(BINS, H, W), torch.tensor([160.0, 160.0, 80.0, 64.0]))
    assert t.counter == 0 and t.n == 0
    with pytest.raises(ValueError, match="mem"):
        odometry.DEVO(_cfg(), network, ht=H, wd=W, mem=7)


def test_run_is_the_calls_followed_by_terminate_and_feeds_ate_real(network, runs):
    """run(): every frame, the twelve closing update() calls of utils/eval_utils.py:127-128, terminate()."""
    from devo_amd import evaluation, odometry
    seq, cfg = _sequence(frames=12), _cfg(KEYFRAME_THRESH=0.0)

    def seeded():
        for i, item in enumerate(seq):
            torch.manual_seed(i)
            yield item

    a = odometry.DEVO(cfg, network, ht=H, wd=W, mem=8)
    poses_a, stamps_a = a.run(seeded(), scale=1e-3)
    b = odometry.DEVO(cfg, network, ht=H, wd=W, mem=8)
    for i, (v, K, ts) in enumerate(seq):
        torch.manual_seed(i)
        b(ts, v, K, scale=1e-3)
    with torch.no_grad():
        for _ in range(12):
            b.update()
    poses_b, stamps_b = b.terminate()
    assert a.is_initialized and poses_a.shape == (12, 7) and np.array_equal(stamps_a, stamps_b) and np.array_equal(stamps_a, [s[2] for s in seq])
    # two runs of one program: equal up to kernels of libraries that are not reproducible from run to run — far inside the yardstick above
    assert np.abs(poses_a - poses_b).max() <= 8.0 * runs["keep"]["D"]["terminate"]
    ate, ref, est = evaluation.ate_real(poses_a, stamps_a, poses_a, stamps_a)
    assert ate <= 1e-3 and ref.shape == est.shape == (12, 7)             # against itself: 0 (cm) up to the alignment's rounding
