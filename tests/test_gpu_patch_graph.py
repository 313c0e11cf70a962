"""devo_amd.graph.PatchGraph (csrc/graph.hip) against the reference's patch-graph bookkeeping: the integer side and the rows of net BIT
for bit against the plain-torch restatement tests/patch_graph_ref.py (devo.py:225-239, :267-287, :305-306; itself checked against
hand-written cases in test_patch_graph_cpu.py), the motion magnitudes against the fp64 oracle (oracle.pops.flow_mag) to 1e-4 relative,
the tolerance test_gpu_fastba.py uses for flow_mag.  Graphs from synth.sliding_window_graph at the smallest shapes at which the kernels
can go wrong: (n 9, M 7) 567 edges, not a multiple of 64; (n 26, M 24) 10 464 edges, 41 workgroups and a real scan; (n 4, M 3) fewer
than 64 edges; no edge at all.  The keyframe branches are chosen by the inputs: small camera steps put the oracle's m / 2 at most at
half the threshold, large steps at least at twice — conditions on the inputs (asserted on the oracle), not tolerances."""
import math
import pytest
import torch
from devo_amd import synth
from patch_graph_ref import RefGraph, shift_frames as ref_shift

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, DIM, THRESH = 120, 160, 384, 12.5
SHAPES = {"odd": (9, 7), "many": (26, 24), "tiny": (4, 3)}
STEPS = {"small": {"odd": (0.01, 0.002), "many": (0.003, 0.0006), "tiny": (0.01, 0.002)}, "large": {"odd": (0.3, 0.03), "many": (0.3, 0.03), "tiny": (0.3, 0.03)}}
_cache = {}


def _scene(shape, steps, seed=11):
    """(poses, patches, intrinsics, ix, ii, jj, kk) on the CPU, computed once and never changed."""
    key = (shape, steps, seed)
    if key not in _cache:
        n, M = SHAPES[shape]
        nbuf = n + 2
        ts, rs = STEPS[steps][shape]
        poses = synth.make_poses(nbuf, seed, trans_step=ts, rot_step=rs)
        patches, _ = synth.make_patches(nbuf, M, H, W, seed=seed)
        intr = synth.make_intrinsics(nbuf, H, W)
        ii, jj, kk = synth.sliding_window_graph(n, M)
        ix = torch.arange(nbuf * M) // M
        assert torch.equal(ix[kk], ii)
        _cache[key] = (poses, patches, intr, ix, ii, jj, kk)
    return _cache[key]


def _pattern(E, dtype, dim=DIM):
    """Row e identifies itself: (e % 2048, e // 2048, then (7 e + c) % 2039) — integers fp16 holds exactly."""
    e = torch.arange(E)[:, None]
    c = torch.arange(dim)[None, :]
    net = ((7 * e + c) % 2039).float()
    net[:, 0] = (e[:, 0] % 2048).float()
    net[:, 1] = (e[:, 0] // 2048).float()
    return net[None].to(dtype)


def _load(ix, jj, kk, M, dtype, dim=DIM, capacity=1 << 14):
    """The same graph in the GPU class and in the restatement, net filled with the pattern."""
    from devo_amd import graph
    g = graph.PatchGraph(M, dim=dim, capacity=capacity, device=DEV, dtype=dtype)
    g.append(kk.to(DEV), jj.to(DEV), ix.to(DEV))
    ref = RefGraph(M, dim, ix, dtype)
    ref.append_factors(kk, jj)
    net = _pattern(len(kk), dtype, dim)
    g.net = net.to(DEV)
    ref.net = net.clone()
    return g, ref


def _same(g, ref, what=""):
    assert len(g) == len(ref.ii), f"{what}: {len(g)} edges, the restatement has {len(ref.ii)}"
    assert g.ii.dtype == torch.int64 and g.ii.shape == (len(g),) and g.net.shape == (1, len(g), ref.dim) and g.net.dtype == ref.net.dtype
    assert torch.equal(g.ii.cpu(), ref.ii) and torch.equal(g.jj.cpu(), ref.jj) and torch.equal(g.kk.cpu(), ref.kk), f"{what}: index lists differ"
    assert torch.equal(g.net.cpu(), ref.net), f"{what}: rows of net differ"


def _d(*ts):
    return [t.to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------------ motion
@pytest.mark.parametrize("shape,steps", [("odd", "small"), ("odd", "large"), ("many", "small"), ("tiny", "small")])
def test_motion_matches_the_fp64_oracle(shape, steps):
    poses, patches, intr, ix, ii, jj, kk = _scene(shape, steps)
    n, M = SHAPES[shape]
    g, ref = _load(ix, jj, kk, M, torch.float16, dim=8)
    P, Q, K = _d(poses, patches, intr)
    k = n - (4 if n > 5 else 2)
    for (i, j) in ((k - 1, k + 1), (n - 2, n - 1)):
        got = g.motion(P, Q, K, i, j)
        want = (ref.motionmag(poses, patches, intr, i, j), ref.motionmag(poses, patches, intr, j, i))
        print(f"motion {shape}/{steps} ({i},{j}): got {got}, oracle {want}, rel {[abs(a - b) / b for a, b in zip(got, want)]}")
        for a, b in zip(got, want):
            assert math.isfinite(b) and abs(a - b) <= 1e-4 * abs(b)
        assert g.motion(P, Q, K, i, j) == got                           # bit-equal from run to run
        assert g.motion(P, Q, K, j, i) == (got[1], got[0])
    a, b = g.motion(P, Q, K, 0, n + 1)                                  # no edge between these frames: 0 / 0
    assert math.isnan(a) and math.isnan(b)
    _same(g, ref, "motion must not touch the graph")


def test_motion_of_an_empty_graph_is_nan():
    from devo_amd import graph
    poses, patches, intr, ix, *_ = _scene("tiny", "small")
    g = graph.PatchGraph(3, dim=DIM, capacity=256, device=DEV)
    a, b = g.motion(*_d(poses, patches, intr), 0, 1)
    assert math.isnan(a) and math.isnan(b) and len(g) == 0
    r = g.keyframe(*_d(poses, patches, intr, ix), 4)
    assert not r.removed and r.n_edges == 0 and math.isnan(r.motion) and len(g) == 0 and g.net.shape == (1, 0, DIM)
    g.remove(torch.zeros(0, dtype=torch.bool, device=DEV))
    g.append(*_d(torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), ix))
    assert len(g) == 0 and g.ii.numel() == 0


# ------------------------------------------------------------------------------------------------ keyframe
def _keyframe_case(shape, steps, dtype, removal_window, expect_removed):
    poses, patches, intr, ix, ii, jj, kk = _scene(shape, steps)
    n, M = SHAPES[shape]
    ki = 4 if n > 5 else 2
    g, ref = _load(ix, jj, kk, M, dtype)
    E0 = len(g)
    removed, k, m, n_after = ref.keyframe(poses, patches, intr, n, keyframe_index=ki, thresh=THRESH, removal_window=removal_window)
    # the condition on the inputs: the oracle is far from the threshold, so fp32 rounding cannot change the branch
    assert removed == expect_removed and (m <= 0.5 * THRESH if expect_removed else m >= 2 * THRESH), f"oracle m / 2 = {m}"
    r = g.keyframe(*_d(poses, patches, intr, ix), n, keyframe_index=ki, thresh=THRESH, removal_window=removal_window)
    print(f"keyframe {shape}/{steps}/{dtype}: {E0} -> {r.n_edges} edges, removed {r.removed}, motion {r.motion} (oracle {m})")
    assert r.removed == removed and r.k == k and r.n_edges == len(ref.ii) == len(g)
    if expect_removed:
        assert abs(r.motion - m) <= 1e-4 * m
    _same(g, ref, "keyframe")
    return E0, r


@pytest.mark.parametrize("shape", ["odd", "many", "tiny"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_keyframe_removal_branch(shape, dtype):
    E0, r = _keyframe_case(shape, "small", dtype, 20, True)
    assert 0 < r.n_edges < E0


@pytest.mark.parametrize("shape", ["odd", "many", "tiny"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_keyframe_keep_branch(shape, dtype):
    E0, r = _keyframe_case(shape, "large", dtype, 20, False)
    assert (r.n_edges < E0) == (shape == "many")                       # only the window rule acts, and only the 26-frame graph is older than it


def test_keyframe_window_removes_nothing_or_everything():
    E0, r = _keyframe_case("many", "large", torch.float16, 100, False)
    assert r.n_edges == E0
    E0, r = _keyframe_case("many", "large", torch.float16, -100, False)
    assert r.n_edges == 0
    E0, r = _keyframe_case("odd", "small", torch.float32, -100, True)
    assert r.n_edges == 0


# ------------------------------------------------------------------------------------------------ append / remove
@pytest.mark.parametrize("shape", ["odd", "many", "tiny"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_append_then_remove_with_random_masks(shape, dtype):
    poses, patches, intr, ix, ii, jj, kk = _scene(shape, "small")
    n, M = SHAPES[shape]
    g, ref = _load(ix, jj, kk, M, dtype)
    _same(g, ref, "append")
    gen = torch.Generator().manual_seed(3)
    for step, frac in enumerate((0.3, 0.9, 0.02)):
        mask = torch.rand(len(ref.ii), generator=gen) < frac
        g.remove(mask.to(DEV))
        ref.remove_factors(mask)
        _same(g, ref, f"remove {step}")
        e = 1 + int(torch.randint(0, 2 * M, (1,), generator=gen))
        pk = torch.randint(0, len(ix), (e,), generator=gen)
        fj = torch.randint(0, n, (e,), generator=gen)
        g.append(pk.to(DEV), fj.to(DEV), ix.to(DEV))
        ref.append_factors(pk, fj)
        _same(g, ref, f"append {step}")                                 # old rows kept, new rows zero
        net = _pattern(len(g), dtype) + 1                               # the operator hands back a new tensor: adopted by reference
        dev_net = net.to(DEV)
        g.net = dev_net
        ref.net = net
        assert g.net is dev_net
    for mask in (torch.zeros(len(g), dtype=torch.bool), torch.ones(len(g), dtype=torch.bool)):
        g.remove(mask.to(DEV))
        ref.remove_factors(mask)
        _same(g, ref, "remove none / all")


def test_errors_are_raised_on_the_host_and_leave_the_graph_intact():
    from devo_amd import graph
    poses, patches, intr, ix, ii, jj, kk = _scene("odd", "small")
    g, ref = _load(ix, jj, kk, 7, torch.float32, capacity=600)
    ptrs = (g.ii.data_ptr(), g.ii._version)
    with pytest.raises(RuntimeError, match="capacity"):
        g.append(*_d(kk[:40], jj[:40], ix))                             # 567 + 40 > 600
    with pytest.raises(RuntimeError):
        g.append(kk[:4], jj[:4].to(DEV), ix.to(DEV))                    # indices on the wrong device
    with pytest.raises(ValueError):
        g.remove(torch.zeros(5, dtype=torch.bool, device=DEV))
    wide = torch.zeros(1, len(g), 2 * DIM, device=DEV)
    good = g.net
    g.net = wide[:, :, ::2]                                             # the graph's shape, but not contiguous
    for call in (lambda: g.remove(torch.zeros(len(g), dtype=torch.bool, device=DEV)), lambda: g.append(*_d(kk[:4], jj[:4], ix)),
                 lambda: g.keyframe(*_d(poses, patches, intr, ix), 9)):
        with pytest.raises(RuntimeError, match="contiguous"):
            call()
    g.net = good
    with pytest.raises(ValueError):
        graph.PatchGraph(7, dim=100, device=DEV)
    a4, b4, ixd, P, Q, K = _d(kk[:4], jj[:4], ix, poses, patches, intr)
    mask = torch.zeros(len(g), dtype=torch.bool, device=DEV)
    dummy = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(torch.cuda.CUDAGraph()):                      # under stream capture every method raises: the result sizes are host data
        dummy.add_(1)
        for call in (lambda: g.append(a4, b4, ixd), lambda: g.motion(P, Q, K, 4, 6), lambda: g.remove(mask), lambda: g.keyframe(P, Q, K, ixd, 9)):
            with pytest.raises(RuntimeError, match="captured"):
                call()
    assert (g.ii.data_ptr(), g.ii._version) == ptrs
    _same(g, ref, "after refused calls")


# ------------------------------------------------------------------------------------------------ frame shift
@pytest.mark.parametrize("k,n", [(9, 10), (8, 10), (5, 10), (3, 4), (0, 12)])
def test_shift_frames_against_the_python_loop(k, n):
    from devo_amd import graph
    gen = torch.Generator().manual_seed(k * 31 + n)
    N, M = 12, 5
    ts = [torch.randn(N, 7, generator=gen), torch.randn(N, generator=gen, dtype=torch.float64), torch.randint(0, 1 << 40, (N,), generator=gen),
          torch.randint(0, 255, (N, M, 3), generator=gen, dtype=torch.uint8), torch.randn(N, M, 3, 3, 3, generator=gen)]
    dev = _d(*ts)
    v0 = [t._version for t in dev]
    graph.shift_frames(dev, k, n)
    ref_shift(ts, k, n)
    for a, b in zip(dev, ts):
        assert torch.equal(a.cpu(), b)
    moved = k < n - 1
    assert all((t._version > v) == moved for t, v in zip(dev, v0))      # a raw-pointer write counts as an in-place edit
    with pytest.raises(ValueError):
        graph.shift_frames([dev[0].t()], 0, 3)


def test_shift_frames_more_than_eight_tensors_and_odd_rows():
    from devo_amd import graph
    gen = torch.Generator().manual_seed(1)
    ts = [torch.randint(0, 255, (9, 1 + 3 * s), generator=gen, dtype=torch.uint8) for s in range(11)]     # rows of 1, 4, 7, ... bytes: every chunk width
    dev = _d(*ts)
    graph.shift_frames(dev, 2, 9)
    ref_shift(ts, 2, 9)
    for a, b in zip(dev, ts):
        assert torch.equal(a.cpu(), b)


# ------------------------------------------------------------------------------------------------ caches keyed on (data_ptr, _version, numel)
def test_version_keyed_caches_follow_the_graph():
    """The Update operator's graph tables, the BA's prepared tables and the lookup plan are keyed on (data_ptr, _version, numel) of the index
    tensors.  Remove e edges and append e others, twice: the ping-pong pair is back at its first address with the same number of edges and
    other contents.  The three consumers must give what they give on fresh clones of the index tensors, bit for bit — they do not if
    PatchGraph leaves out the version bump behind its raw-pointer writes."""
    from devo_amd import altcorr, fastba
    from devo_amd.backends import cuda_ba
    from devo_amd.update import Update
    poses, patches, intr, ix, *_ = _scene("odd", "small")
    n, M, C, dim = 9, 7, 128, 64
    # every patch of frames 0 .. 7 into every frame, and whole patches leave and arrive: every patch keeps 9 edges, the shape on which the
    # BA sums in a fixed order (test_gpu_fastba.py::test_ba_is_bit_reproducible_on_regular_graphs; on ragged graphs it adds with float
    # atomics and no two runs agree in the last bits, whatever the tables)
    ii, jj, kk = synth.full_graph(8, M, n_frames=n)
    _, centres = synth.make_patches(n + 2, M, H, W, seed=11)
    fmap, gmap = synth.make_features(n + 2, M, C, H, W, centres, seed=11)
    g, _ = _load(ix, jj, kk, M, torch.float32, dim=dim)
    E = len(g)
    torch.manual_seed(5)
    upd = Update(3, dim=dim).to(DEV).eval()
    gen = torch.Generator().manual_seed(5)
    net, inp, corr = _d(torch.randn(1, E, dim, generator=gen), torch.randn(1, E, dim, generator=gen), torch.randn(1, E, 882, generator=gen))
    delta, weight = synth.make_update_outputs(E, 11, sigma=0.5)
    P, Q, K = _d(poses, patches, intr)
    pyr = [altcorr.channels_last(fmap.to(DEV)), altcorr.channels_last(synth.pyramid_l1(fmap).to(DEV))]
    gm = gmap.to(DEV)
    lm = torch.tensor([1e-4], device=DEV)

    def consumers(a, b, c):
        with torch.no_grad():
            n1, (d1, w1, _) = upd(net, inp, corr, None, a, b, c)
        coords = cuda_ba.transform(P, Q, K, a, b, c, layout="2pp")
        look = altcorr.corr_pyramid(gm, pyr, coords, c, b, radius=3, scales=(1, 4))
        p2, q2 = P.clone(), Q.clone()
        fastba.BA(p2, q2, K, coords[:, :, :, 1, 1] + delta.to(DEV), weight.to(DEV), lm, a, b, c, 1, n, 2, check="never")
        return [n1, d1, w1, look, p2, q2]

    first = consumers(g.ii, g.jj, g.kk)
    addr, before = g.ii.data_ptr(), (g.ii.clone(), g.jj.clone(), g.kk.clone())
    gone = torch.randperm(8 * M, generator=gen)[:12]
    for leave, arrive in ((gone[:6], torch.arange(8 * M, 8 * M + 6)), (gone[6:], torch.cat([torch.tensor([8 * M + 6]), gone[:5]]))):
        g.remove(torch.isin(g.kk, leave.to(DEV)))                       # 6 patches x 9 edges go ...
        g.append(*_d(arrive.repeat_interleave(n), torch.arange(n).repeat(6), ix))       # ... and 6 others arrive with 9 edges each
    assert g.ii.data_ptr() == addr and len(g) == E and not torch.equal(g.kk, before[2])
    got = consumers(g.ii, g.jj, g.kk)
    want = consumers(g.ii.clone(), g.jj.clone(), g.kk.clone())
    names = ("net", "delta", "weight", "lookup", "poses", "patches")
    for name, a, b, f in zip(names, got, want, first):
        print(f"{name}: max |mutated - fresh clones| = {float((a.double() - b.double()).abs().max()):.3e}, against the first graph {float((a.double() - f.double()).abs().max()):.3e}")
    for name, a, b in zip(names, got, want):
        assert torch.equal(a, b), f"{name} on the mutated graph differs from the result on fresh clones of its index tensors"


# ------------------------------------------------------------------------------------------------ ten frames
def test_ten_frame_drive():
    """Ten frames of the state machine's order (devo.py:541-552): n += 1, append the forward edges, append the backward edges, keyframe()
    — with the frame buffers shifted when a keyframe goes — against the restatement after every frame: state carried between calls."""
    from devo_amd import graph
    M, LIFE, WINDOW, N0, NBUF = 24, 13, 10, 8, 24
    src_poses = synth.make_poses(NBUF, 12, trans_step=0.003, rot_step=0.0006)
    # every third incoming frame jumps: the test pair of frames then straddles a jump or does not — both branches occur
    jump = torch.zeros(NBUF, 3)
    jump[:, 0] = torch.cumsum((torch.arange(NBUF) % 3 == 0).float() * 0.4, 0)
    src_poses[0, :, :3] += jump
    src_patches, _ = synth.make_patches(NBUF, M, H, W, seed=12)
    intr = synth.make_intrinsics(NBUF, H, W)
    ix = torch.arange(NBUF * M) // M
    poses, patches = src_poses.clone(), src_patches.clone()
    ii, jj, kk = synth.sliding_window_graph(N0, M, lifetime=LIFE, removal=WINDOW)
    g, ref = _load(ix, jj, kk, M, torch.float16)
    P, Q, K, IXD = _d(poses, patches, intr, ix)
    n, branches = N0, []
    for frame in range(10):
        s = N0 + frame                                                  # the incoming frame's pose and patches go into slot n
        poses[0, n], patches[0, n * M:(n + 1) * M] = src_poses[0, s], src_patches[0, s * M:(s + 1) * M]
        P[0, n], Q[0, n * M:(n + 1) * M] = P.new_tensor(src_poses[0, s].tolist()), src_patches[0, s * M:(s + 1) * M].to(DEV)
        n += 1
        fwd_k = torch.arange(M * max(n - LIFE, 0), M * (n - 1))        # devo.py:366-372
        fwd_j = torch.full_like(fwd_k, n - 1)
        bj = torch.arange(max(n - LIFE, 0), n)                          # devo.py:374-380
        bwd_k = torch.arange(M * (n - 1), M * n).repeat_interleave(len(bj))
        bwd_j = bj.repeat(M)
        for pk, fj in ((fwd_k, fwd_j), (bwd_k, bwd_j)):
            g.append(pk.to(DEV), fj.to(DEV), IXD)
            ref.append_factors(pk, fj)
        net = _pattern(len(g), torch.float16) + frame                   # what the update operator would hand back
        g.net, ref.net = net.to(DEV), net
        removed, k, m, n_ref = ref.keyframe(poses, patches, intr, n, thresh=THRESH, removal_window=WINDOW)
        assert abs(m - THRESH) > 0.2 * THRESH, f"frame {frame}: the oracle's m / 2 = {m} is too close to the threshold for a bit-exact comparison"
        r = g.keyframe(P, Q, K, IXD, n, thresh=THRESH, removal_window=WINDOW)
        assert (r.removed, r.k, r.n_edges) == (removed, k, len(ref.ii)), f"frame {frame}"
        if r.removed:
            graph.shift_frames([P[0], Q[0].view(NBUF, M, 3, 3, 3)], r.k, n)
            ref_shift([poses[0], patches[0].view(NBUF, M, 3, 3, 3)], k, n)
            n -= 1
        assert n == n_ref
        _same(g, ref, f"frame {frame}")
        assert torch.equal(P.cpu(), poses) and torch.equal(Q.cpu(), patches)
        branches.append(removed)
    print("ten-frame drive: removed =", branches, "edges at the end", len(g))
    assert any(branches) and not all(branches)
