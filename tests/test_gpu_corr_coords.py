"""The lookup family (correlation lookup, its backward, the locality plan, patchify) at non-finite, huge and frame-border coordinates,
against the fp64 oracle (oracle/altcorr.py) on the cases of tests/corr_coord_cases.py (pinned on the CPU by test_corr_coord_cases_cpu.py).

CONTRACT.  A patch pixel is BAD if its x or y is non-finite, FAR if it is finite and no tap of its window can lie in the frame (every
|v| >= 1e6 is), NEAR otherwise; an edge whose nine pixels are all near is CLEAN.
 1. Forward, near and far pixels: out[b, e, :, :, i0, j0] equals the fp64 oracle within 1e-4 of the output scale (fp32; 2e-3 with fp16
    storage, the oracle run on the fp16-rounded features; 1e-12 for the fp64 generic kernel: 32 fp64 products per tap, the bound
    test_dtype_coverage_of_the_reference_dispatch holds it to).  Every structurally zero output — where the
    oracle returns 0 for all-ones features and the same coordinates — is exactly 0.  Far pixels are never excluded from a comparison.
 2. Forward, bad pixels: each of the pixel's own outputs is NaN or exactly 0, never a finite non-zero value (the oracle gives NaN).
    Measured on MI355X: every forward kernel — dense-product, its group form, mfma4x4, staged, generic — gives NaN on all of a bad pixel's
    outputs when SOME pixel of the edge (at that level) has a tap inside the frame, because the blend multiplies the pixel's zero taps
    by its NaN fraction; the dense-product kernel (both forms) and mfma4x4 give exact zeros for an edge whose whole box misses the frame
    (they skip the blend: all nine pixels bad or far), the staged and generic kernels give NaN there too.
 3. Independence: a clean edge's outputs are bit-identical between a call and the same call with every other edge's coordinates replaced by
    benign in-frame ones (the plans of the two calls differ).
 4. Plan: for any coordinates the first B E ints are a permutation of range(B E), 0 <= #heavy, #heavy + #dead <= B E; every edge in the
    DEAD tail of a group plan is structurally zero at both levels (all-ones oracle at scale 1 and at scale 4; an edge's bad pixels, whose
    outputs contract 2 allows to be 0, are moved to -1e5 for this: they have no tap anywhere); cuda_ba.transform(..., plan_for=...) +
    plan_finish agrees with cuda_corr.plan on the emitted coordinates (the sense of test_plan_started_by_the_reprojection_kernel_equals_plan)
    also with a NaN pose and inverse depths of 0, -1 and 1e-30.
 5. Backward: d_fmap2 is finite everywhere and within 1e-4 of its scale of the oracle on SANITISED coordinates (every bad pixel moved to
    -1e5: it contributes nothing); d_fmap1 matches the same oracle everywhere except at entries [b, ii[e], :, i0, j0] of a bad pixel
    (e, i0, j0), which may match or be NaN (measured: all three backward paths give the sanitised value there — a bad pixel's window gradient
    is zeroed with its out-of-frame taps); frames and positions no edge touches stay exactly 0.
 6. Patchify: forward bit-exact with the oracle, bad and far patches all zeros, the same for NCHW and channels-last input and for fp32 and
    fp16; backward finite and within 1e-5 of the oracle.

WHY EVERY PATH STAYS INSIDE ITS BUFFERS with one pixel at -1000000 and the rest in frame (corr_floor_to_int, csrc/corr_tile.h, clamps
floor(v) to +-1e6 and maps NaN there too, so every origin is an int of magnitude <= 1e6 + 6 and every box extent <= 2e6 + 12):
 - dense-product (corr_mm.h make_geo): the box's position count is a long long; beyond the result area's capacity the edge goes window by
   window (9 windows of D x D taps, origins from LDS); every fetch is a raw-buffer load whose descriptor spans ONE frame and whose offset
   is OFF_NONE unless 0 <= gy < H2 and 0 <= gx < W2; result-area writes are indexed by tile and lane, never by a coordinate.
 - mfma4x4 (corr_mfma.h:150-260): the same long long count and window mode, the same per-position frame test in front of a raw-buffer
   load; the scatter into the result area tests (unsigned)(gy - oy[p]) < D and (unsigned)(gx - ox[p]) < D.  A level whose box misses the
   frame has no passes and its outputs are forced to 0; its epilogue used to form its (unused) result-area reads with the box's own width,
   up to 2e6 — addresses far outside the LDS area for the `wide_dead` case; it now reads D x D windows at the area's start (fixed here).
 - staged (corr.hip:215-330): whole box, pixel rows or single windows by tile_fits on long long counts; a piece is fetched only if
   `sok` (position listed and inside the frame); LDS offsets of a stage use only that stage's pixels.
 - generic (corr.hip:468-520): one tap per lane behind an explicit frame test, int64 addressing.
 - backward, atomic / segments (corr.hip:518-765): the box is clipped to the frame before anything is addressed (empty: no work); taps
   outside the frame have their window gradient set to 0, so the 16-bit origin packing of the tile kernel can only mis-place zeros.
 - backward, product form (corr_bwd_mfma.h:68-100): the box clipped to the frame — at most the whole frame — is walked position by
   position; an empty box returns before the edge is listed; the frame kernel tests every window against its tile with plain ints.
 - plan (corr_plan_bin): extents as long long, centre coordinates through fminf / fmaxf (NaN -> 0) before the conversion to int, frame,
   band, column and group indices clamped into their ranges: every bin lies in [-1, nbins).
 - patchify forward / backward: one tap per lane behind an explicit frame test on ints of magnitude <= 1e6 + 6.
"""
import functools
import os
import subprocess
import sys
import pytest
import torch
import corr_coord_cases as K
from oracle import altcorr as A
from util import channels_last5

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pytest_child(args, env, limit):
    """One child pytest of this file in a process group of its own -> (exit code, stdout, stderr).  Never raises: a child that is still
    running after `limit` seconds is killed with everything it started (the whole group) and reported as exit code None."""
    import signal
    here = os.path.abspath(__file__)
    try:
        p = subprocess.Popen([sys.executable, "-m", "pytest", here, "-m", "gpu", "-q", "-x", "-s", "-p", "no:cacheprovider"] + list(args), env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True,
                             cwd=os.path.dirname(os.path.dirname(here)))
    except Exception as exc:                                 # (nothing was started)
        return None, "", f"the child pytest could not be started: {exc!r}"
    try:
        out, err = p.communicate(timeout=limit)
        return p.returncode, out, err
    except BaseException as exc:                             # the time limit, or anything else while waiting: nothing of the child survives
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        try:
            out, err = p.communicate(timeout=30)
        except Exception:
            out, err = "", ""
        if not isinstance(exc, Exception):                   # (KeyboardInterrupt, SystemExit: the group is gone, pass it on)
            raise
        return None, out or "", (err or "") + f"\nkilled with its process group after {limit} s: {exc!r}"


TOL = {torch.float32: 1e-4, torch.float16: 2e-3, torch.float64: 1e-12}


# ------------------------------------------------------------------------------------------------------------------ cases and references
@functools.lru_cache(maxsize=None)
def _feat(C, B, half):
    f1, f2 = K.features(0, C, B)
    l1 = K.level1(f2)
    if half:
        f1, f2, l1 = (t.half().float() for t in (f1, f2, l1))
    return f1, f2, l1


@functools.lru_cache(maxsize=None)
def _coords(case, R, B):
    """coords [B, E, 2, 3, 3], benign coords or None, ii, jj, clean [B, E] or None"""
    if case == "border":
        b = K.border(0, R)
        return b["coords"], None, b["ii"], b["jj"], None
    if case == "wide_dead":
        w = K.wide_dead(0)
        return w["coords"], None, w["ii"], w["jj"], None
    h = K.hostile(0)
    c, ben, clean = h["coords"], h["benign"], h["clean_edge"][None]
    if B == 2:                                           # the second batch entry: the same edges in reversed order
        c, ben, clean = torch.cat([c, c.flip(1)]), torch.cat([ben, ben.flip(1)]), torch.cat([clean, clean.flip(1)])
    return c.contiguous(), ben.contiguous(), h["ii"], h["jj"], clean


@functools.lru_cache(maxsize=None)
def _expect(case, R, C, B, half, level):
    """oracle output, structural-zero mask and bad-pixel mask [B, E, 3, 3] of a lookup at `level` (0: coords into H x W, 1: coords / 4
    into H/4 x W/4)"""
    f1, f2, l1 = _feat(C, B, half)
    coords, _, ii, jj, _ = _coords(case, R, B)
    s, fm, h, w = ((1, f2, K.H, K.W), (4, l1, K.H // 4, K.W // 4))[level]
    cs = coords / s
    ref = A.corr_forward(f1.double(), fm.double(), cs, ii, jj, R)
    zero = K.structural_zero(cs, ii, jj, R, h, w)
    bad = ~(torch.isfinite(coords[:, :, 0]) & torch.isfinite(coords[:, :, 1]))
    return ref, zero, bad


def _same(a, b):
    """bit-for-bit in the sense that matters here: equal values, NaN in the same places"""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _check_forward(got, ref, zero, bad, tol, what):
    """contracts 1 and 2"""
    got = got.detach().cpu().double().reshape(ref.shape)
    badm = bad[:, :, None, None].expand_as(got)
    gb = got[badm]
    n_nan, n_zero = int(torch.isnan(gb).sum()), int((gb == 0).sum())
    ok = ~badm
    assert bool(torch.isfinite(got[ok]).all()), f"{what}: non-finite output of a pixel that is not bad"
    scale = float(ref[ok].abs().max())
    err = float((got[ok] - ref[ok]).abs().max()) / scale
    nz = int(torch.count_nonzero(got[zero & ok]))
    print(f"[corr-coords] {what}: rel err {err:.2e} (tol {tol:.0e}), structural zeros {int((zero & ok).sum())} ({nz} non-zero), "
          f"bad-pixel outputs {n_nan} NaN / {n_zero} zero / {gb.numel() - n_nan - n_zero} other")
    assert n_nan + n_zero == gb.numel(), f"{what}: a bad pixel's output is finite and non-zero"
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e}"
    assert nz == 0, f"{what}: {nz} structurally zero outputs are not exactly 0"


def _fast_path(groups=False):
    """the kernel a C = 128 fp32 / fp16 lookup in a fast layout takes (test_other_kernels_stay_covered_at_hostile_coordinates sets the switches)"""
    if os.environ.get("DEVO_CORR_MFMA", "1") == "0":
        return "staged"
    if os.environ.get("DEVO_CORR_MM", "1") == "0":
        return "mfma4x4"
    return "dense-product-groups" if groups else "dense-product"


def _layout(t, layout):
    from devo_amd import altcorr
    return channels_last5(t) if layout == "cl" else altcorr.channel_blocked(t, 8) if layout == "blk8" else t


# ------------------------------------------------------------------------------------------------------------------ per-level forward
CASES = [("hostile", 3), ("hostile", 5), ("border", 0), ("border", 1), ("border", 3), ("border", 5), ("wide_dead", 3), ("wide_dead", 5)]


def _forward_case(case, R, layout, dtype, C=128, B=1, mm=None):
    from devo_amd.backends import cuda_corr
    half = dtype == torch.float16
    f1, f2, _ = _feat(C, B, half)
    coords, benign, ii, jj, clean = _coords(case, R, B)
    ref, zero, bad = _expect(case, R, C, B, half, 0)
    d = lambda t: t.to(DEV)
    was = cuda_corr.MM_KERNEL
    try:
        if mm is not None:
            cuda_corr.MM_KERNEL = mm
        run = lambda c: cuda_corr.forward(d(f1).to(dtype), _layout(d(f2).to(dtype), layout), d(c), d(ii), d(jj), R)[0]
        got = run(coords)
        path = cuda_corr.last_forward_path()
        got_benign = run(benign) if benign is not None else None
    finally:
        cuda_corr.MM_KERNEL = was
    what = f"{case} R={R} {layout} {str(dtype)[6:]} C={C} B={B} [{path}]"
    _check_forward(got, ref, zero, bad, TOL[dtype], what)
    if got_benign is not None:                           # contract 3 (and the benign call itself: all finite, against its own oracle)
        assert bool(clean.any()) and torch.equal(got[clean.to(DEV)], got_benign[clean.to(DEV)]), f"{what}: a clean edge depends on other edges"
        assert bool(torch.isfinite(got_benign).all())
    return path


def _nchw_path():
    """a short edge list into a raw NCHW level: converted into the split-blocked format for the dense-product kernel, else read directly"""
    return "dense-product" if _fast_path() == "dense-product" else "generic"


@pytest.mark.parametrize("layout", ["cl", "nchw", "blk8"])
@pytest.mark.parametrize("case,R", CASES)
def test_forward_fp32(case, R, layout):
    assert _forward_case(case, R, layout, torch.float32) == (_nchw_path() if layout == "nchw" else _fast_path())


@pytest.mark.parametrize("case,R", CASES)
def test_forward_fp16_blocked(case, R):
    assert _forward_case(case, R, "blk8", torch.float16) == _fast_path()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case,R", CASES)
def test_forward_generic_kernel(case, R, dtype):
    """C = 32 from a raw NCHW level: fp64 always takes the generic kernel, fp32 when the dense-product kernel is switched off"""
    assert _forward_case(case, R, "nchw", dtype, C=32, mm=False) == "generic"


@pytest.mark.parametrize("layout,dtype", [("cl", torch.float32), ("blk8", torch.float16)])
def test_forward_batch_of_two(layout, dtype):
    assert _forward_case("hostile", 3, layout, dtype, B=2) == _fast_path()


# ------------------------------------------------------------------------------------------------------------------ fused two-level lookup
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("case", ["hostile", "border", "wide_dead"])
def test_pyramid_own_plan_foreign_plan_and_group_form(case, dtype):
    """forward_pyramid with scales (1, 4) on channel-blocked levels: the caller's own plan, a plan made for the benign coordinates, and the
    group form (a GROUP plan, as test_group_form_reads_level_1_from_lds_and_changes_nothing selects it) — contracts 1 to 3 at both levels,
    and the same bits from all three"""
    from devo_amd.backends import cuda_corr
    R, half = 3, dtype == torch.float16
    f1, f2, l1 = _feat(128, 1, half)
    coords, benign, ii, jj, clean = _coords(case, R, 1)
    exp = [_expect(case, R, 128, 1, half, lvl) for lvl in (0, 1)]
    d = lambda t: t.to(DEV)
    pyr = [_layout(d(f2).to(dtype), "blk8"), _layout(d(l1).to(dtype), "blk8")]
    E = coords.shape[1]
    look = lambda c, order: cuda_corr.forward_pyramid(d(f1).to(dtype), pyr, d(c), d(ii), d(jj), R, (1, 4), order=order)
    plan = lambda c, grp: cuda_corr.plan(d(c), d(jj), K.N_FRAMES, K.H, 1.0, R, width=K.W if grp else 0, l1=4 if grp else 0)
    own, grp = plan(coords, False), plan(coords, True)
    assert cuda_corr.plan_kind(own, E) == 0 and cuda_corr.plan_kind(grp, E) == 1
    outs = {}
    for name, order, groups in (("own plan", own, False), ("foreign plan", plan(benign if benign is not None else coords.flip(1), False), False),
                                ("group form", grp, True)):
        got = look(coords, order)
        assert cuda_corr.last_forward_path() == _fast_path(groups), name
        outs[name] = got
        both = got.view(1, E, 7, 7, 3, 3, 2)
        for lvl in (0, 1):
            _check_forward(both[..., lvl], *exp[lvl], TOL[dtype], f"pyramid {case} {str(dtype)[6:]} {name} level {lvl} [{cuda_corr.last_forward_path()}]")
    assert _same(outs["foreign plan"], outs["own plan"]) and _same(outs["group form"], outs["own plan"])
    if benign is not None:                               # contract 3, with the benign call's own plans
        for grp_ in (False, True):
            ben = look(benign, plan(benign, grp_))
            sel = clean[0].to(DEV)
            assert torch.equal(ben[:, sel], outs["own plan"][:, sel]) and bool(torch.isfinite(ben).all())


# ------------------------------------------------------------------------------------------------------------------ plan
def _check_plan(order, BE, dead_ok=None):
    """contract 4: permutation, class counts; dead_ok [BE] (group plans): edges that may sit in the DEAD tail"""
    o = order.cpu()
    assert sorted(o[:BE].tolist()) == list(range(BE))
    nh, nd = int(o[BE]), int(o[2 * BE + 1])
    assert nh >= 0 and nd >= 0 and nh + nd <= BE
    if dead_ok is not None:
        tail = o[BE - nd:BE].long()
        assert bool(dead_ok[tail].all()), "a live edge sits in the DEAD tail"
    return nh, nd


@functools.lru_cache(maxsize=None)
def _hostile_dead_ok():
    """edges that are structurally zero at both levels (bad pixels moved to -1e5: they have no tap anywhere)"""
    h = K.hostile(0)
    z0 = K.structural_zero(h["sanitised"], h["ii"], h["jj"], 3, K.H, K.W)
    z1 = K.structural_zero(h["sanitised"] / 4, h["ii"], h["jj"], 3, K.H // 4, K.W // 4)
    return (z0.flatten(2).all(2) & z1.flatten(2).all(2))[0]


@pytest.mark.parametrize("times", [1, 13])
def test_plan_of_hostile_coordinates(times):
    """E = 160, and 2080 edges (the ordering step by several workgroups, corr_plan.h); edge plans and group plans, radius 3 and 5"""
    from devo_amd.backends import cuda_corr
    h = K.tiled(K.hostile(0), times)
    coords, jj = h["coords"].to(DEV), h["jj"].to(DEV)
    E = coords.shape[1]
    dead_ok = _hostile_dead_ok().repeat(times)
    assert 0 < int(dead_ok.sum()) < E // 2
    for R in (3, 5):
        _check_plan(cuda_corr.plan(coords, jj, K.N_FRAMES, K.H, radius=R), E)
        _check_plan(cuda_corr.plan(coords, jj, K.N_FRAMES, K.H // 4, 4.0, R), E)
    grp = cuda_corr.plan(coords, jj, K.N_FRAMES, K.H, 1.0, 3, width=K.W, l1=4)
    assert cuda_corr.plan_kind(grp, E) == 1
    nh, nd = _check_plan(grp, E, dead_ok)
    print(f"[corr-coords] group plan of {E} hostile edges: {nh} heavy, {nd} dead of {int(dead_ok.sum())} structurally zero")
    assert nd > 0
    c2 = torch.cat([coords, coords.flip(1)])                      # B = 2
    _check_plan(cuda_corr.plan(c2, jj, K.N_FRAMES, K.H, radius=3), 2 * E)


@pytest.mark.parametrize("scene", ["as it is", "NaN pose", "inverse depths 0, -1, 1e-30"])
def test_plan_started_by_the_reprojection_kernel_on_degenerate_scenes(scene):
    """cuda_ba.transform(..., plan_for=...) + plan_finish == cuda_corr.plan on the emitted coordinates: the same heavy set in front and the
    same (frame, band) sequence behind it — also when a pose is NaN and when inverse depths are 0, negative or tiny"""
    from devo_amd import synth
    from devo_amd.backends import cuda_ba, cuda_corr
    n, M, H, W = 6, 40, 60, 80
    poses, (patches, _), intr = synth.make_poses(n, 9), synth.make_patches(n, M, H, W, seed=9), synth.make_intrinsics(n, H, W)
    if scene == "NaN pose":
        poses[0, 2] = float("nan")
    elif scene != "as it is":
        for k, v in enumerate((0.0, -1.0, 1e-30) * 8):
            patches[0, 7 * k + 3, 2] = v
    ii, jj, kk = (t.to(DEV) for t in synth.full_graph(n, M))
    args = (poses.to(DEV), patches.to(DEV), intr.to(DEV), ii, jj, kk)
    E = ii.numel()
    for pf, kw in (((n, H, 3), {}), ((n, H, 3, W, 4), dict(width=W, l1=4))):
        coords, buf = cuda_ba.transform(*args, layout="2pp", plan_for=pf)
        assert _same(coords, cuda_ba.transform(*args, layout="2pp"))
        cc = coords.cpu()
        if scene == "NaN pose":
            assert 0 < int(torch.isnan(cc).flatten(2).any(2).sum()) < E
        a = cuda_corr.plan_finish(buf, jj, n, H, 3, **kw).cpu()
        b = cuda_corr.plan(coords, jj, n, H, 1.0, 3, **kw).cpu()
        assert cuda_corr.plan_kind(a, E) == cuda_corr.plan_kind(b, E) == (1 if kw else 0)
        nh, nd = _check_plan(a, E)
        assert (nh, nd) == _check_plan(b, E)
        assert sorted(a[:nh].tolist()) == sorted(b[:nh].tolist())
        if kw:                                                    # group plan: the same bin starts, the same edges in every group
            nb = n * ((H // 4 + 5) // 6) * ((W // 4 + 5) // 6) + 1
            sa, sb = a[2 * E + 2: 2 * E + 3 + nb], b[2 * E + 2: 2 * E + 3 + nb]
            assert torch.equal(sa, sb)
            grp_of = lambda o: torch.bucketize(torch.argsort(o[:E].long()), sa[1:].long(), right=True)     # (slot of every edge -> its bin)
            assert torch.equal(grp_of(a)[a[nh:E].long()], grp_of(b)[a[nh:E].long()])
            san = torch.where(torch.isfinite(cc), cc, torch.full_like(cc, K.SANITISED))
            dead_ok = (K.structural_zero(san, kk.cpu(), jj.cpu(), 3, H, W).flatten(2).all(2) &
                       K.structural_zero(san / 4, kk.cpu(), jj.cpu(), 3, H // 4, W // 4).flatten(2).all(2))[0]
            assert bool(dead_ok[a[E - nd:E].long()].all())
        else:
            cy = torch.nan_to_num(cc[0, :, 1, 1, 1], nan=0.0, posinf=float(H), neginf=-1.0)        # (the kernel's fmaxf / fminf send NaN to 0)
            key = lambda o: torch.stack([jj.cpu()[o[nh:E].long()], (cy[o[nh:E].long()].clamp(0, H - 1) / 16).floor().long()], 1)
            assert torch.equal(key(a), key(b))


# ------------------------------------------------------------------------------------------------------------------ backward
def _product_path():
    """what a channels-last C % 128 == 0 backward takes (test_other_kernels_stay_covered_at_hostile_coordinates sets the switches)"""
    return "atomic" if os.environ.get("DEVO_CORR_BWD_ATOMIC") else "segments" if os.environ.get("DEVO_CORR_BWD_SEG") else "product"


@functools.lru_cache(maxsize=None)
def _backward_ref(C, R):
    """oracle gradients on the SANITISED hostile coordinates; `own` [Np, 3, 3]: d_fmap1 entries that belong to a bad pixel"""
    h = K.hostile(0)
    f1, f2, _ = _feat(C, 1, False)
    Dm = 2 * R + 1
    grad = torch.randn(1, len(h["ii"]), Dm, Dm, 3, 3, generator=torch.Generator().manual_seed(11))
    r1, r2 = A.corr_backward(f1.double(), f2.double(), h["sanitised"], h["ii"], h["jj"], grad, R)
    own = torch.zeros(K.N_PATCHES, 3, 3, dtype=torch.bool)
    for e in range(len(h["ii"])):
        own[h["ii"][e]] |= h["bad_pixel"][e]
    assert bool(own.any()) and not bool(own[:K.N_PATCHES // 2].any())
    return grad, r1, r2, own


def _check_backward(d1, d2, r1, r2, own, what):
    """contract 5"""
    d1, d2 = d1.detach().cpu().double(), d2.detach().cpu().double()
    assert d1.shape == r1.shape and d2.shape == r2.shape
    assert bool(torch.isfinite(d2).all()), f"{what}: d_fmap2 is not finite"
    e2 = float((d2 - r2).abs().max() / r2.abs().max())
    ownm = own[None, :, None].expand_as(d1)
    assert bool(torch.isfinite(d1[~ownm]).all()), f"{what}: d_fmap1 is not finite outside bad pixels' own entries"
    s1 = float(r1.abs().max())
    e1 = float((d1 - r1)[~ownm].abs().max()) / s1
    o = d1[ownm]
    o_nan, o_err = int(torch.isnan(o).sum()), float(torch.nan_to_num((o - r1[ownm]).abs(), nan=0.0).max()) / s1
    print(f"[corr-coords] {what}: d_fmap1 rel err {e1:.2e}, d_fmap2 rel err {e2:.2e} (tol 1e-04); bad pixels' own d_fmap1 entries: "
          f"{o_nan} NaN of {o.numel()}, the others within {o_err:.2e}")
    assert e2 <= 1e-4, f"{what}: d_fmap2 relative error {e2:.3e}"
    assert e1 <= 1e-4, f"{what}: d_fmap1 relative error {e1:.3e}"
    assert o_err <= 1e-4, f"{what}: a bad pixel's own d_fmap1 entry is neither NaN nor the oracle's value"
    assert int(torch.count_nonzero(d2[:, K.N_FRAMES - 1])) == 0, f"{what}: the frame without an edge"
    untouched = (r2.abs().amax(2, keepdim=True) == 0).expand_as(r2)
    assert int(torch.count_nonzero(d2[untouched])) == 0 and int(torch.count_nonzero(d1[(r1 == 0) & ~ownm])) == 0, f"{what}: untouched positions"


@pytest.mark.parametrize("R", [3, 1])
def test_backward_product_form(R):
    """C = 128, channels-last: corr_bwd_mfma.h (the box clipped to the frame, which one pixel at -1e6 makes the whole frame wide)"""
    from devo_amd.backends import cuda_corr
    h = K.hostile(0)
    f1, f2, _ = _feat(128, 1, False)
    grad, r1, r2, own = _backward_ref(128, R)
    d = lambda t: t.to(DEV)
    f2d = channels_last5(d(f2))
    d1, d2 = cuda_corr.backward(d(f1), f2d, d(h["coords"]), d(h["ii"]), d(h["jj"]), d(grad), R)
    assert cuda_corr.last_backward_path == _product_path() and d2.stride() == f2d.stride()
    _check_backward(d1, d2, r1, r2, own, f"backward R={R} C=128 channels-last [{cuda_corr.last_backward_path}]")


@pytest.mark.parametrize("layout", ["cl", "nchw"])
def test_backward_atomic(layout):
    """C = 64: never the product form (channels-last under DEVO_CORR_BWD_SEG=1: the tile kernel)"""
    from devo_amd.backends import cuda_corr
    h = K.hostile(0)
    f1, f2, _ = _feat(64, 1, False)
    grad, r1, r2, own = _backward_ref(64, 3)
    d = lambda t: t.to(DEV)
    d1, d2 = cuda_corr.backward(d(f1), _layout(d(f2), layout), d(h["coords"]), d(h["ii"]), d(h["jj"]), d(grad), 3)
    assert cuda_corr.last_backward_path == ("segments" if (os.environ.get("DEVO_CORR_BWD_SEG") and layout == "cl") else "atomic")
    _check_backward(d1, d2, r1, r2, own, f"backward C=64 {layout} [{cuda_corr.last_backward_path}]")


def test_backward_nchw_through_the_cached_copy():
    """a plain NCHW level, C = 128, 1120 edges (hostile seven times): the product form on a cached channels-last copy.  Seven copies of the
    same edges and gradients: the oracle's gradients are seven times those of one copy (to fp64 rounding)"""
    from devo_amd.backends import cuda_corr
    times = 7
    h = K.tiled(K.hostile(0), times)
    assert h["coords"].shape[1] >= cuda_corr.NCHW_CONVERT_MIN_EDGES
    f1, f2, _ = _feat(128, 1, False)
    grad, r1, r2, own = _backward_ref(128, 3)
    d = lambda t: t.to(DEV)
    d1, d2 = cuda_corr.backward(d(f1), d(f2), d(h["coords"]), d(h["ii"]), d(h["jj"]), d(torch.cat([grad] * times, 1)), 3)
    assert cuda_corr.last_backward_path == _product_path() and d2.shape == f2.shape
    assert d2.stride(2) == 1 or _product_path() == "atomic"            # (the atomic path reads the NCHW level as it is)
    _check_backward(d1, d2, times * r1, times * r2, own, f"backward C=128 NCHW {h['coords'].shape[1]} edges [{cuda_corr.last_backward_path}]")


def test_backward_through_autograd():
    """altcorr.corr(...).backward(): the forward's NaN outputs do not enter the gradients"""
    from devo_amd import altcorr
    from devo_amd.backends import cuda_corr
    h = K.hostile(0)
    f1, f2, _ = _feat(128, 1, False)
    grad, r1, r2, own = _backward_ref(128, 3)
    d = lambda t: t.to(DEV)
    a, b = d(f1).requires_grad_(True), channels_last5(d(f2)).requires_grad_(True)
    out = altcorr.corr(a, b, d(h["coords"]), d(h["ii"]), d(h["jj"]), 3)
    _check_forward(out, *_expect("hostile", 3, 128, 1, False, 0), 1e-4, "autograd forward")
    out.backward(d(grad))
    assert cuda_corr.last_backward_path == _product_path()
    _check_backward(a.grad, b.grad, r1, r2, own, f"backward through autograd [{cuda_corr.last_backward_path}]")


# ------------------------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("R", [0, 1, 3])
def test_patchify(R):
    """contract 6"""
    from devo_amd.backends import cuda_corr
    net = torch.randn(2, 8, 12, 16, generator=torch.Generator().manual_seed(6))
    pc = K.patch_centres(0)
    ref = A.patchify_forward(net, pc, R)
    bad, far = K.classify(pc[..., None, None], R, 12, 16)
    dead = (bad | far)[:, :, 0, 0]
    assert int(dead.sum()) >= 32 and int((~dead).sum()) >= 16 and int(torch.count_nonzero(ref[dead])) == 0
    d = lambda t: t.to(DEV)
    for dtype in (torch.float32, torch.float16):
        want = A.patchify_forward(net.to(dtype), pc, R)
        for fmt in (torch.contiguous_format, torch.channels_last):
            got, = cuda_corr.patchify_forward(d(net).to(dtype).contiguous(memory_format=fmt), d(pc), R)
            assert torch.equal(got.cpu(), want), (dtype, fmt)
            assert int(torch.count_nonzero(got.cpu()[dead])) == 0
    gr = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7))
    rb = A.patchify_backward(net, pc, gr, R)
    for fmt in (torch.contiguous_format, torch.channels_last):
        back, = cuda_corr.patchify_backward(d(net).contiguous(memory_format=fmt), d(pc), d(gr), R)
        assert bool(torch.isfinite(back).all())
        err = float((back.cpu().double() - rb.double()).abs().max() / rb.abs().max())
        print(f"[corr-coords] patchify backward R={R} {fmt}: rel err {err:.2e} (tol 1e-05)")
        assert err <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ the other kernels
def test_other_kernels_stay_covered_at_hostile_coordinates():
    """The forward / backward tests of this module once more under each switch that selects another kernel (read once per process, so each
    in a child pytest with its own time limit): DEVO_CORR_MFMA=0 the staged kernel, DEVO_CORR_MM=0 the 4x4 matrix-core kernel,
    DEVO_CORR_BWD_SEG=1 the tile kernel of the backward, DEVO_CORR_BWD_ATOMIC=1 the one-kernel atomic backward.  One sequential walk that
    ends at the first child that does not return 0: nothing else is started on the GPU after a failure.  Every child runs in a process
    group of its own; one that outlives its limit is killed with everything it started, and counts as a failure."""
    fwd, bwd = "test_forward_fp32 or test_forward_fp16 or test_forward_batch or test_pyramid", "test_backward"
    for switch, sel in (("DEVO_CORR_MFMA=0", fwd), ("DEVO_CORR_MM=0", fwd), ("DEVO_CORR_BWD_SEG=1", bwd), ("DEVO_CORR_BWD_ATOMIC=1", bwd)):
        env = dict(os.environ)
        name, value = switch.split("=")
        env[name] = value
        rc, out, err = _pytest_child(["-k", sel], env, 300)
        print("\n".join(line.lstrip(".").replace("[corr-coords]", f"[corr-coords] {switch}:") for line in out.splitlines() if "[corr-coords]" in line))
        assert rc == 0, f"{switch}: " + ("killed at its time limit" if rc is None else f"exit {rc}") + "\n" + out[-3000:] + err[-2000:]
