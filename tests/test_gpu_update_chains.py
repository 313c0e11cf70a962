"""The row-resident chain kernels of the fp16 update operator (devo_amd/csrc/gemm_rs.hip), each on its own against the staged fp64 oracle
of tests/update_chain_ref.py: called through devo_amd._lib as Update._forward_rs calls them, at row counts around the 16-row matrix
tiles, the 32-row rounds of the row-wise stages and the 96-row workgroup tile.  For every kernel and row count: rows behind the
last one stay untouched (canary rows), and the rows of an E-row call come out of an (E + 40)-row call bit for bit.
Bounds: update_chain_ref.LINEAR_BOUND / BOUNDS (where they come from is written there)."""
import pytest
import torch
import update_chain_ref as R
from util import assert_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY_ROWS, SENTINEL = 96, -1234.0


def _ua():
    from devo_amd import update as UA
    return UA


def _dev(t, dtype=torch.float16):
    return None if t is None else t.to(DEV).to(dtype).contiguous()


def _img(w):
    """the weight image of a [384 n, K] fp64 (fp16-exact) weight, as the operator builds it"""
    return _ua()._rs_image(_dev(w))


def _out(rows, width, dtype=torch.float16):
    return torch.full((rows + CANARY_ROWS, width), SENTINEL, dtype=dtype, device=DEV)


def _canary_ok(t, rows):
    return bool((t[rows:] == SENTINEL).all())


def _call(name, *args):
    UA = _ua()
    L = UA.L
    conv = [L.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    L.check(getattr(L.lib(), name)(*conv, L.stream()), name)


FIGURES = {}                                                          # the largest figure of every check of the running test, printed behind it


def _note(tag, err):
    FIGURES[tag] = max(FIGURES.get(tag, 0.0), err)


@pytest.fixture(autouse=True)
def _figures_and_faults():
    FIGURES.clear()
    yield
    for tag, err in FIGURES.items():
        print(f"\n[figure] {tag}: {err:.3e}", end="")
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                          # a faulted GPU: nothing more is launched on it
        pytest.exit(f"the GPU reported {e}", returncode=3)


def _assert_ln(got, exact, key, what):
    err = R.row_err(got.double(), exact.to(DEV))
    _note(f"{what.split(' E=')[0]} {key[1]} / rms, bound {R.BOUNDS[key]:.1e}", err.max().item())
    assert torch.isfinite(got).all() and err.max().item() <= R.BOUNDS[key], (what, key, err.max().item(), int(err.argmax()))


def _assert_lin(got, staged, mag, what, bound=R.LINEAR_BOUND):
    err = (got.double() - staged.to(DEV)).abs() / mag.to(DEV).clamp(min=1e-30)
    _note(f"{what.split(' E=')[0].split(' M=')[0]} / term magnitude, bound {bound:.1e}", err.max().item())
    assert torch.isfinite(got).all() and err.max().item() <= bound, (what, err.max().item(), int(err.amax(-1).argmax()))


def _for_row_counts(run, what):
    """run(E) -> outputs with CANARY_ROWS sentinel rows behind E; checks the canaries and prefix independence, yields (E, outputs)"""
    for E in R.ROW_COUNTS:
        outs, more = run(E), run(E + R.PREFIX_EXTRA)
        for o, m in zip(outs, more):
            assert _canary_ok(o, E) and _canary_ok(m, E + R.PREFIX_EXTRA), (what, E, "rows behind the last one were written")
            assert torch.equal(o[:E], m[:E]), (what, E, "the rows depend on how many follow them")
        yield E, [o[:E] for o in outs]


# ---------------------------------------------------------------------------------------------------------------- correlation chain
class _Corr:
    def __init__(self, kind, K0, ldc):
        self.case, sd, self.eps, self.exact, self.staged = R.corr_ref(kind, K0)
        self.K0, self.ldc = K0, ldc
        # a view into a wider buffer whose rows are only 4-byte aligned; what lies between the rows is not part of them
        self.buf = torch.full((R.BASE_ROWS * ldc + 2,), 1000.0, dtype=torch.float16, device=DEV)
        self.corr = self.buf[2:].view(R.BASE_ROWS, ldc)[:, :K0]
        self.corr.copy_(_dev(self.case["corr"]))
        self.net, self.inp = _dev(self.case["net"]), _dev(self.case["inp"])
        v = lambda k: _dev(sd[k])
        self.keep = [v("corr.0.bias"), v("corr.2.bias"), v("corr.3.weight"), v("corr.3.bias"), v("corr.5.bias"), v("norm.weight"), v("norm.bias")]
        self.img = [_img(sd["corr.0.weight"]), _img(sd["corr.2.weight"]), _img(sd["corr.5.weight"])]

    def run(self, E, net=None, fn="devo_upd_rs_corr_f16"):
        b0, b2, g3, be3, b5, g, be = self.keep
        out = _out(E, R.D)
        _call(fn, self.corr, self.ldc, self.K0, self.img[0], b0, self.img[1], b2, g3, be3, float(self.eps["corr.3"]), self.img[2], b5,
              self.net if net is None else net, self.inp, g, be, float(self.eps["norm"]), out, E)
        return [out]


@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("K0", R.CORR_WIDTHS)
def test_correlation_chain_matches_the_oracle(K0, wide, kind):
    """devo_upd_rs_corr_f16: every accepted kind of width (865: the first with 28 K steps; odd; DEVO's 882; 896: no masked step), rows at a
    pitch of K0 rounded up to even and as a view into a 904-wide buffer, both parameter sets"""
    ldc = 904 if wide else K0 + K0 % 2
    c = _Corr(kind, K0, ldc)
    assert c.corr.data_ptr() % 16 == 4 and c.corr.stride(0) == ldc
    for E, (out,) in _for_row_counts(c.run, f"corr K0={K0} ldc={ldc} {kind}"):
        _assert_ln(out, c.exact[:E], (kind, "out"), f"corr K0={K0} ldc={ldc} E={E}")


@pytest.mark.parametrize("kind", ["plain", "offset"])
def test_correlation_chain_with_an_fp32_state(kind):
    """devo_upd_rs_corr_f16_net32: an fp16-exact state gives the bits of the fp16 form; any other state enters the sum unrounded"""
    c = _Corr(kind, 882, 882)
    g = torch.Generator().manual_seed(3)
    net32 = (c.case["net"] + 1e-3 * torch.randn(R.BASE_ROWS, R.D, generator=g, dtype=torch.float64)).float()
    assert not torch.equal(net32.half().float(), net32)
    sd = R.params(kind)[0]
    exact = R.rs_corr(c.case["corr"], net32.double(), c.case["inp"], sd, c.eps["corr.3"], c.eps["norm"])
    net32, same32 = net32.to(DEV), c.net.float()
    for E, (out,) in _for_row_counts(lambda E: c.run(E, net=net32, fn="devo_upd_rs_corr_f16_net32"), f"corr net32 {kind}"):
        _assert_ln(out, exact[:E], (kind, "out"), f"corr net32 E={E}")
        assert torch.equal(c.run(E, net=same32, fn="devo_upd_rs_corr_f16_net32")[0], c.run(E)[0]), E


def test_correlation_chain_refuses_a_width_its_28_k_steps_do_not_fit():
    """K0 = 800 has 25 K steps in its weight image: the kernel's 28 would read other waves' weights and past the image — an argument
    error, nothing launched; the operator keeps such a layer on the layer-wise path and still matches the fp64 oracle"""
    UA = _ua()
    c = _Corr("plain", 882, 882)
    b0, b2, g3, be3, b5, g, be = c.keep
    with pytest.raises(RuntimeError, match="864 < K0"):
        _call("devo_upd_rs_corr_f16", c.corr, 882, 800, c.img[0], b0, c.img[1], b2, g3, be3, 1e-3, c.img[2], b5, c.net, c.inp, g, be, 1e-3, _out(4, R.D), 4)
    z = torch.zeros(64, 800, dtype=torch.float16, device=DEV)
    assert not UA._rs_chain_ok(torch.float16, 384, c.net[:64], c.inp[:64], z)
    assert UA._rs_chain_ok(torch.float16, 384, c.net[:64], c.inp[:64], c.corr[:64])

    from oracle import update as U
    from devo_amd import synth
    torch.manual_seed(11)
    m = UA.Update(3)
    m.corr[0] = UA.Linear(800, 384)
    sd = {k: R.q16(v.detach().double()) for k, v in m.state_dict().items()}
    m.load_state_dict({k: v.float() for k, v in sd.items()})
    m = m.to(DEV).half().eval()
    ii, jj, kk = synth.full_graph(8, 20)
    E = len(ii)
    assert E >= 1024                                                   # (fewer rows: the library's GEMMs, not the layer-wise HIP kernels)
    net, inp, corr = (R.q16(torch.randn(1, E, w, dtype=torch.float64) * s) for w, s in ((384, 0.5), (384, 0.5), (800, 1.0)))
    ref = U.update(sd, net, inp, corr, ii, jj, kk)
    with torch.no_grad():
        o, (d, w, _) = m(_dev(net), _dev(inp), _dev(corr), None, ii.to(DEV), jj.to(DEV), kk.to(DEV))
    for got, want, what in ((o, ref[0], "net"), (d, ref[1], "delta"), (w, ref[2], "weight")):
        assert torch.isfinite(got).all()
        assert_rel(got.float(), want, 2e-2, f"800-wide corr, fp16 {what}")      # (the fp16 operator's bound in test_update_full_width_fp32_fp16_and_torch_path)


# ---------------------------------------------------------------------------------------------------------------- gru chain
@pytest.mark.parametrize("kind", ["plain", "offset"])
def test_gru_chain_matches_the_oracle_in_both_output_forms(kind):
    """devo_upd_rs_gru_f16 / _out32: LN0 - GatedResidual - LN2 - GatedResidual - heads; the fp32 state is the fp16 one widened, delta and
    weight are the same bits in both forms"""
    case, sd, eps, exact, _ = R.gru_ref(kind)
    v = lambda k: _dev(sd[k])
    cat = lambda a, b: torch.cat([v(a), v(b)], 0).contiguous()
    x, hy, grp = _dev(case["x"]), _dev(case["hy"]), case["grp"].to(DEV)
    keep = []

    def im(w):
        keep.append(w)
        return _ua()._rs_image(w)
    args = [v("gru.0.weight"), v("gru.0.bias"), float(eps["gru.0"]),
            im(cat("gru.1.gate.0.weight", "gru.1.res.0.weight")), cat("gru.1.gate.0.bias", "gru.1.res.0.bias"), im(v("gru.1.res.2.weight")), v("gru.1.res.2.bias"),
            v("gru.2.weight"), v("gru.2.bias"), float(eps["gru.2"]),
            im(cat("gru.3.gate.0.weight", "gru.3.res.0.weight")), cat("gru.3.gate.0.bias", "gru.3.res.0.bias"), im(v("gru.3.res.2.weight")), v("gru.3.res.2.bias"),
            v("d.1.weight"), v("d.1.bias"), v("w.1.weight"), v("w.1.bias")]

    def run(E, out32=False):
        net, delta, weight = _out(E, R.D, torch.float32 if out32 else torch.float16), _out(E, 2), _out(E, 2)
        _call("devo_upd_rs_gru_f16_out32" if out32 else "devo_upd_rs_gru_f16", x, hy, grp, *args, net, delta, weight, E)
        return [net, delta, weight]
    for E, (net, delta, weight) in _for_row_counts(run, f"gru {kind}"):
        for got, k in ((net, "net_out"), (delta, "delta"), (weight, "weight")):
            _assert_ln(got, exact[k][:E], (kind, k), f"gru E={E}")
        n32, d32, w32 = run(E, out32=True)
        assert _canary_ok(n32, E) and _canary_ok(d32, E) and _canary_ok(w32, E)
        assert torch.equal(n32[:E], net.float()) and torch.equal(d32[:E], delta) and torch.equal(w32[:E], weight), E


# ---------------------------------------------------------------------------------------------------------------- Linear - ReLU - Linear
def _mlp2_args(name):
    sd = R.params("plain")[0]
    return (sd[name + ".0.weight"], sd[name + ".0.bias"], sd[name + ".2.weight"], sd[name + ".2.bias"])


@pytest.mark.parametrize("case", ["plain", "gather", "ldx768", "residual_is_x", "residual_is_y", "in_place", "in_place_fg"])
def test_fused_two_layer_chain_matches_the_oracle(case):
    """devo_upd_rs_mlp2_fg_f16: no gather; a gather with -1, indices past the source rows and duplicates; rows at a pitch of 768; the
    residual being x (the operator's call), being y; y being x without a gather, with and without the f | g tail; fg checked in both halves"""
    sd, c = R.params("plain")[0], R.mlp2_case()
    W1, b1, W2, b2 = _mlp2_args("c2")
    Wfg, bfg = R.fg_layer(sd, "agg_kk")
    tail = case != "in_place"
    gather = c["gather"] if case in ("gather", "residual_is_x") else None
    src = c["x"] if gather is not None else c["x"][:R.BASE_ROWS]
    res = {"plain": None, "gather": c["res"], "ldx768": c["res"], "residual_is_x": src[:R.BASE_ROWS], "residual_is_y": c["res"], "in_place": None,
           "in_place_fg": None}[case]
    want = R.rs_mlp2(src, W1, b1, W2, b2, gather=gather, residual=res, fg=(Wfg, bfg) if tail else None, staged=True)
    i1, i2, ifg = _img(W1), _img(W2), _img(Wfg)
    vb1, vb2, vbfg = _dev(b1), _dev(b2), _dev(bfg)
    if case == "ldx768":
        wide = torch.full((src.shape[0], 768), 1000.0, dtype=torch.float16, device=DEV)
        xd = wide[:, 384:]
        xd.copy_(_dev(src))
    else:
        xd = _dev(src)
    gd, resd = _dev(gather, torch.int64), _dev(res)

    def run(E):
        y, fg = _out(E, R.D), _out(E, 2 * R.D)
        x_, r_ = xd, resd
        if case == "residual_is_x":
            r_ = xd
        if case == "residual_is_y":
            y[:E] = resd[:E]
            r_ = y
        if case in ("in_place", "in_place_fg"):
            y[:E] = xd[:E]
            x_ = y
        x_rows = src.shape[0] if gather is not None else E                # (no gather: the call's own rows, as the operator passes them)
        _call("devo_upd_rs_mlp2_fg_f16", x_, x_.stride(0), x_rows, gd, i1, vb1, i2, vb2, r_, y, E, ifg if tail else None, vbfg if tail else None,
              fg if tail else None)
        return [y, fg]
    for E, (y, fg) in _for_row_counts(run, f"mlp2 {case}"):
        _assert_lin(y, want["y"][:E], want["y_mag"][:E], f"mlp2 {case} y E={E}")
        if tail:
            for half in (slice(0, R.D), slice(R.D, 2 * R.D)):
                _assert_lin(fg[:, half], want["fg"][:E, half], want["fg_mag"][:E, half], f"mlp2 {case} fg[{half.start}:] E={E}")


@pytest.mark.parametrize("groups", ["table", "one"])
def test_expand_add_with_the_next_layer_matches_the_oracle(groups):
    """devo_upd_rs_expand_fg_f16: x += hy[group_of] in place — the staged sum bit for bit — and the f | g layer on the new rows; one group
    only; a table whose first and last rows are in use"""
    case, sd = R.gru_ref("plain")[0], R.params("plain")[0]
    W, b = R.fg_layer(sd, "agg_ij")
    hy = case["hy"] if groups == "table" else case["hy"][7:8]
    grp = case["grp"] if groups == "table" else torch.zeros_like(case["grp"])
    assert (grp == 0).any() and (grp == hy.shape[0] - 1).any()
    want = R.rs_expand_fg(case["x"], hy, grp, W, b, staged=True)
    xd, hyd, grpd, img, bd = _dev(case["x"]), _dev(hy), grp.to(DEV), _img(W), _dev(b)

    def run(E):
        x, fg = _out(E, R.D), _out(E, 2 * R.D)
        x[:E] = xd[:E]
        _call("devo_upd_rs_expand_fg_f16", x, hyd, grpd, img, bd, fg, E)
        return [x, fg]
    for E, (x, fg) in _for_row_counts(run, f"expand {groups}"):
        assert torch.equal(x, _dev(want["x"][:E])), E
        for half in (slice(0, R.D), slice(R.D, 2 * R.D)):
            _assert_lin(fg[:, half], want["fg"][:E, half], want["fg_mag"][:E, half], f"expand {groups} fg[{half.start}:] E={E}")


# ---------------------------------------------------------------------------------------------------------------- one Linear layer
def _linear_run(c, K, N, variant):
    x384 = torch.full((R.BASE_ROWS, 384), 1000.0, dtype=torch.float16, device=DEV)      # x: the view [:, :K]; what lies behind K is not part of the rows
    x384[:, :K] = _dev(c["x"])
    img, bd, resd = _img(c["W"]), _dev(c["b"]), _dev(c["res"])

    def run(M):
        y = _out(M, N)
        if variant == "residual":
            y[:M] = resd[:M]
        _call("devo_upd_rs_linear_f16", x384[:, :K], 384, img, bd, y if variant == "residual" else None, y, N, M, N, K, N // 2 if variant == "relu_from" else N)
        return [y]
    return run


@pytest.mark.parametrize("N,variant", [(384, "plain"), (384, "residual"), (768, "relu_from")])
@pytest.mark.parametrize("K", R.LINEAR_K)
def test_row_resident_linear_at_every_advertised_width(K, N, variant):
    """devo_upd_rs_linear_f16 over K in (352, 384] — odd, a multiple of 8, 384 — with x a view of a 384-wide tensor and a large last
    column: the last row's last element must not drop out with the dword that straddles the end of the buffer"""
    c = R.linear_case(K, N)
    want, mag = R.rs_linear(c["x"], c["W"], c["b"], residual=c["res"] if variant == "residual" else None,
                            relu_from=N // 2 if variant == "relu_from" else None, staged=True)
    run = _linear_run(c, K, N, variant)
    for M in (1, 31, 33, 97):
        (y,), (more,) = run(M), run(M + R.PREFIX_EXTRA)
        assert _canary_ok(y, M) and _canary_ok(more, M + R.PREFIX_EXTRA) and torch.equal(y[:M], more[:M]), (K, N, M)
        _assert_lin(y[:M], want[:M], mag[:M], f"rs_linear K={K} N={N} {variant} M={M}")


def test_row_resident_linear_on_its_large_row_tile_with_an_odd_width():
    """12 289 rows: the smallest count that takes the 96-row form of the kernel; K = 383"""
    K, N, M = 383, 384, 12289
    g = torch.Generator().manual_seed(5)
    c = R.linear_case(K, N)
    x = R.q16(0.5 * torch.randn(M, K, generator=g, dtype=torch.float64))
    x[:R.BASE_ROWS], x[:, K - 1] = c["x"], 2 * R.LAST_COL
    want, mag = R.rs_linear(x, c["W"], c["b"], staged=True)
    x384 = torch.full((M, 384), 1000.0, dtype=torch.float16, device=DEV)
    x384[:, :K] = _dev(x)
    y = _out(M, N)
    _call("devo_upd_rs_linear_f16", x384[:, :K], 384, _img(c["W"]), _dev(c["b"]), None, y, N, M, N, K, N)
    assert _canary_ok(y, M)
    _assert_lin(y[:M], want, mag, "rs_linear M=12289 K=383")


@pytest.mark.parametrize("K", [356, 380, 384])
def test_row_resident_split_linear_below_its_python_gate(K):
    """devo_upd_rs_linear_split straight through the ABI (update._linear_split wants 8 192 rows): 1, 95 and 97 rows, K a multiple of 4 in
    (352, 384], the scaled rows of test_row_resident_split_linear_agrees_with_the_ring_kernel; 1e-6 of each output's term magnitude"""
    UA = _ua()
    L, N = UA.L, 384
    g = torch.Generator().manual_seed(K)
    rows = 97 + R.PREFIX_EXTRA
    x = torch.randn(rows, K, generator=g) * torch.rand(rows, 1, generator=g) * 4
    x[1::7] *= 1e-7
    x[2::11] *= 3e5
    x[3::13, 192:] *= 4096.0
    x[6::19] = 0
    w = torch.randn(N, K, generator=g) / 384 ** 0.5
    w[1::5] *= 1e-6
    w[2::9] *= 1e3
    b, res = torch.randn(N, generator=g), torch.randn(rows, N, generator=g)
    ref = torch.nn.functional.linear(x.double(), w.double(), b.double())
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    assert L.lib().devo_upd_rs_split_supported(N, K)
    x384 = torch.full((rows, 384), 1e30, dtype=torch.float32, device=DEV)
    x384[:, :K] = x.to(DEV)
    wd, bd, resd = w.to(DEV), b.to(DEV), res.to(DEV)
    img = torch.empty(int(L.lib().devo_upd_rs_split_weight_bytes(N, K)) // 4, dtype=torch.float32, device=DEV)
    _call("devo_upd_rs_split_weight", wd, wd.stride(0), wd.stride(1), N, K, img)

    def run(M, residual):
        y = _out(M, N, torch.float32)
        if residual:
            y[:M] = resd[:M]
        _call("devo_upd_rs_linear_split", x384[:, :K], 384, img, bd, y if residual else None, None, y, N, M, N, K, N // 2 if not residual else N)
        return y
    relu = ref.clone()
    relu[:, N // 2:].clamp_(min=0)
    for M in (1, 95, 97):
        for residual, want, m in ((False, relu, mag), (True, ref + res.double(), mag + res.double().abs())):
            y, more = run(M, residual), run(M + R.PREFIX_EXTRA, residual)
            assert _canary_ok(y, M) and _canary_ok(more, M + R.PREFIX_EXTRA) and torch.equal(y[:M], more[:M]), (K, M, residual)
            _assert_lin(y[:M], want[:M], m[:M], f"rs_linear_split K={K} M={M} residual={residual}", bound=R.SPLIT_BOUND)
