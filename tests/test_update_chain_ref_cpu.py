"""The staged oracle of the row-resident chain kernels (tests/update_chain_ref.py), checked without a GPU: against the project's pinned
fp64 operator, against its own exact form, and for its power to tell a defective kernel from a correct one at the bounds and the
inputs of tests/test_gpu_update_chains.py."""
import pytest
import torch
from oracle import update as U
from oracle import fastba as FB
from devo_amd import synth
import update_chain_ref as R


def test_exact_composition_in_the_operators_launch_order_equals_the_pinned_oracle():
    """staged=False, composed as Update._forward_rs launches the kernels, equals oracle.update.update (pinned by tests/golden/update_f64.npz)
    at dim 384 on a small graph, to fp64 rounding."""
    sd, _ = R.make_params("plain")
    eps = 1e-3                                                         # (the operator's: oracle/update.py:_ln)
    ii, jj, kk = synth.full_graph(4, 5)
    E = len(ii)
    g = torch.Generator().manual_seed(9)
    net, inp = torch.randn(E, R.D, generator=g, dtype=torch.float64), torch.randn(E, R.D, generator=g, dtype=torch.float64)
    corr = torch.randn(E, 882, generator=g, dtype=torch.float64)
    ref_net, ref_delta, ref_weight = U.update(sd, net[None], inp[None], corr[None], ii, jj, kk)

    ix, jx = FB.neighbors(kk, jj)
    x = R.rs_corr(corr, net, inp, sd, eps, eps)
    m = lambda key: (sd[key + ".0.weight"], sd[key + ".0.bias"], sd[key + ".2.weight"], sd[key + ".2.bias"])
    x = R.rs_mlp2(x, *m("c1"), gather=ix, residual=x)["y"]
    o = R.rs_mlp2(x, *m("c2"), gather=jx, residual=x, fg=R.fg_layer(sd, "agg_kk"))
    x, fg = o["y"], o["fg"]
    _, gk = torch.unique(kk, return_inverse=True)
    _, gp = torch.unique(ii * 12345 + jj, return_inverse=True)
    hy, _ = R.rs_linear(R.soft_agg_sum(fg, gk), sd["agg_kk.h.weight"], sd["agg_kk.h.bias"])
    o = R.rs_expand_fg(x, hy, gk, *R.fg_layer(sd, "agg_ij"))
    x, fg = o["x"], o["fg"]
    hy, _ = R.rs_linear(R.soft_agg_sum(fg, gp), sd["agg_ij.h.weight"], sd["agg_ij.h.bias"])
    out = R.rs_gru(x, hy, gp, sd, eps, eps)
    for got, ref, what in ((out["net_out"], ref_net[0], "net"), (out["delta"], ref_delta[0], "delta"), (out["weight"], ref_weight[0], "weight")):
        assert (got - ref).abs().max().item() <= 1e-10 * max(1.0, ref.abs().max().item()), what


def test_the_plain_rows_are_what_they_claim():
    """the scaled row stays finite in fp16 behind the first layer; the two gate rows saturate, the others do not"""
    for K0 in R.CORR_WIDTHS:
        case, sd, _, _, staged = R.corr_ref("plain", K0)
        h = torch.relu(R.lin(case["corr"], sd["corr.0.weight"], sd["corr.0.bias"]))
        assert h[R.ROW_BIG].max().item() > 100 and torch.isfinite(h.to(torch.float16)).all() and torch.isfinite(staged).all()
        assert case["corr"][R.ROW_ZERO, :K0 - 1].abs().max().item() == 0 and case["corr"][R.ROW_CONST, :K0 - 1].unique().numel() == 1
    case, sd, eps, _, staged = R.gru_ref("plain")
    _, gate = R.ln2_input(case, sd, eps["gru.0"])
    n_sat = (gate.abs() > 20).sum(-1)
    assert all(n_sat[r].item() >= 96 for r in R.ROWS_SAT), n_sat[list(R.ROWS_SAT)]
    assert all(torch.isfinite(v).all() for v in staged.values())
    c = R.mlp2_case()
    h = torch.relu(R.lin(c["x"], sd["c2.0.weight"], sd["c2.0.bias"]))
    assert torch.isfinite(h.to(torch.float16)).all() and h[R.ROW_BIG].max().item() > 50
    vecs = [sd[k + ".bias"] for k in R._LAYERS] + [sd[k + s] for k in R._NORMS for s in (".weight", ".bias")]
    assert all((v != 0).all() for v in vecs)                      # every bias, gamma and beta: no zero element ...
    assert all(not torch.equal(a, b) for i, a in enumerate(vecs) for b in vecs[i + 1:] if a.shape == b.shape)      # ... and no two alike
    assert not torch.equal(sd["d.1.weight"], sd["w.1.weight"]) and len(set(eps.values())) == 4


def test_the_offset_rows_reach_ln2_and_ln3_with_mean_over_std_between_50_and_200():
    case, sd, eps, _, _ = R.gru_ref("offset")
    t, _ = R.ln2_input(case, sd, eps["gru.0"])
    r = R.mean_over_std(t)
    assert r.min().item() > 50 and r.max().item() < 200, (r.min().item(), r.max().item())
    # the rows are ON fp16's grid in front of LN2: the store of LN0's output loses a hair, the same way on every path
    X = R.layer_norm(case["x"] + case["hy"][case["grp"].long()], sd["gru.0.weight"], sd["gru.0.bias"], eps["gru.0"])
    assert ((R.r16(X) - X).abs().max() / R.ULP).item() < 2 * R.OFFSET_HAIR and R.r16(X).unique().numel() > 8
    for K0 in R.CORR_WIDTHS:
        case, sd, eps, _, _ = R.corr_ref("offset", K0)
        l2 = R.ln3_input(case, sd)
        r = R.mean_over_std(l2)
        assert r.min().item() > 50 and r.max().item() < 200, (K0, r.min().item(), r.max().item())
        assert ((R.r16(l2) - l2).abs().max() / R.ULP).item() < 2 * R.OFFSET_HAIR


@pytest.mark.parametrize("kind", ["plain", "offset"])
def test_staged_rounding_stays_within_the_bounds_of_the_gpu_tests(kind):
    """staged=True against staged=False: the fp16 stores of a correct kernel cost no more than the GPU tests allow"""
    _, _, _, exact, staged = R.gru_ref(kind)
    for k in ("net_out", "delta", "weight"):
        assert R.row_err(staged[k], exact[k]).max().item() <= R.BOUNDS[(kind, k)], k
    for K0 in R.CORR_WIDTHS:
        _, _, _, exact, staged = R.corr_ref(kind, K0)
        assert R.row_err(staged, exact).max().item() <= R.BOUNDS[(kind, "out")], K0
    if kind == "plain":
        sd, c = R.params("plain")[0], R.mlp2_case()
        a = (sd["c2.0.weight"], sd["c2.0.bias"], sd["c2.2.weight"], sd["c2.2.bias"])
        kw = dict(gather=c["gather"], residual=c["res"], fg=R.fg_layer(sd, "agg_kk"))
        ex, st = R.rs_mlp2(c["x"], *a, **kw), R.rs_mlp2(c["x"], *a, staged=True, **kw)
        for k in ("y", "fg"):
            assert ((st[k] - ex[k]).abs() <= R.LINEAR_BOUND * st[k + "_mag"]).all(), k


# ---------------------------------------------------------------------------------------------------------------- discriminating power
def _crosses_ln(defect, staged, exact, key):
    """the GPU test's check of an output behind a LayerNorm / sigmoid fails on at least one row — and the defect, not the staging, is why"""
    return (R.row_err(defect, exact) > R.BOUNDS[key]).any().item() and (R.row_err(defect, staged) > R.BOUNDS[key]).any().item()


def _crosses_lin(defect, staged, mag):
    return ((defect - staged).abs() > R.LINEAR_BOUND * mag).any().item()


def _gru(kind, sd=None, eps=None, **kw):
    case, sd0, eps0, _, _ = R.gru_ref(kind)
    sd, eps = sd or sd0, eps or eps0
    return R.rs_gru(case["x"], case["hy"], case["grp"], sd, eps["gru.0"], eps["gru.2"], staged=True, **kw)


def _corr(kind, K0, sd=None, eps=None, corr=None, **kw):
    case, sd0, eps0, _, _ = R.corr_ref(kind, K0)
    sd, eps = sd or sd0, eps or eps0
    return R.rs_corr(case["corr"] if corr is None else corr, case["net"], case["inp"], sd, eps["corr.3"], eps["norm"], staged=True, **kw)


def _without(sd, key, part=slice(None)):
    sd = dict(sd)
    sd[key] = sd[key].clone()
    sd[key][part] = 0
    return sd


def test_two_swapped_epsilons_cross_the_bounds():
    for kind in ("plain", "offset"):
        _, _, eps, exact, staged = R.gru_ref(kind)
        d = _gru(kind, eps=dict(eps, **{"gru.0": eps["gru.2"], "gru.2": eps["gru.0"]}))
        assert _crosses_ln(d["net_out"], staged["net_out"], exact["net_out"], (kind, "net_out")), kind
        for K0 in R.CORR_WIDTHS:
            _, _, eps, exact, staged = R.corr_ref(kind, K0)
            d = _corr(kind, K0, eps=dict(eps, **{"corr.3": eps["norm"], "norm": eps["corr.3"]}))
            assert _crosses_ln(d, staged, exact, (kind, "out")), (kind, K0)


def test_a_dropped_bias_crosses_the_bounds():
    _, sd, _, exact, staged = R.gru_ref("plain")
    d = _gru("plain", sd=_without(sd, "gru.3.res.2.bias"))                                     # b_r2[1]
    assert _crosses_ln(d["net_out"], staged["net_out"], exact["net_out"], ("plain", "net_out"))
    d = _gru("plain", sd=_without(sd, "d.1.bias"))                                             # bd
    assert _crosses_ln(d["delta"], staged["delta"], exact["delta"], ("plain", "delta"))
    for K0 in R.CORR_WIDTHS:
        _, sd, _, exact, staged = R.corr_ref("plain", K0)
        assert _crosses_ln(_corr("plain", K0, sd=_without(sd, "corr.5.bias")), staged, exact, ("plain", "out")), K0      # b5
    sd, c = R.params("plain")[0], R.mlp2_case()
    a = (sd["c2.0.weight"], sd["c2.0.bias"], sd["c2.2.weight"], sd["c2.2.bias"])
    W, b = R.fg_layer(sd, "agg_kk")
    b0 = b.clone()
    b0[R.D:] = 0                                                                               # bfg, second half
    st = R.rs_mlp2(c["x"], *a, gather=c["gather"], residual=c["res"], fg=(W, b), staged=True)
    d = R.rs_mlp2(c["x"], *a, gather=c["gather"], residual=c["res"], fg=(W, b0), staged=True)
    assert _crosses_lin(d["fg"][:, R.D:], st["fg"][:, R.D:], st["fg_mag"][:, R.D:]) and torch.equal(d["fg"][:, :R.D], st["fg"][:, :R.D])
    case = R.gru_ref("plain")[0]
    W, b = R.fg_layer(sd, "agg_ij")
    b0 = b.clone()
    b0[R.D:] = 0
    st = R.rs_expand_fg(case["x"], case["hy"], case["grp"], W, b, staged=True)
    d = R.rs_expand_fg(case["x"], case["hy"], case["grp"], W, b0, staged=True)
    assert _crosses_lin(d["fg"][:, R.D:], st["fg"][:, R.D:], st["fg_mag"][:, R.D:])


def test_swapped_head_weights_cross_the_bounds():
    _, sd, _, exact, staged = R.gru_ref("plain")
    d = _gru("plain", sd=dict(sd, **{"d.1.weight": sd["w.1.weight"], "w.1.weight": sd["d.1.weight"]}))
    assert _crosses_ln(d["delta"], staged["delta"], exact["delta"], ("plain", "delta"))
    assert _crosses_ln(d["weight"], staged["weight"], exact["weight"], ("plain", "weight"))


def test_a_gather_index_past_the_rows_read_as_the_last_row_crosses_the_bound():
    sd, c = R.params("plain")[0], R.mlp2_case()
    a = (sd["c2.0.weight"], sd["c2.0.bias"], sd["c2.2.weight"], sd["c2.2.bias"])
    past = c["gather"] >= R.GATHER_ROWS
    assert past.sum().item() >= 3 and (c["gather"] == R.GATHER_ROWS).any()
    st = R.rs_mlp2(c["x"], *a, gather=c["gather"], residual=c["res"], staged=True)
    d = R.rs_mlp2(c["x"], *a, gather=c["gather"].clamp(max=R.GATHER_ROWS - 1), residual=c["res"], staged=True)
    bad = ((d["y"] - st["y"]).abs() > R.LINEAR_BOUND * st["y_mag"]).any(-1)
    assert torch.equal(bad, past)                                  # every such row, in every prefix that holds one


def test_the_last_row_computed_from_the_row_before_it_crosses_the_bounds_at_every_row_count():
    sd, c = R.params("plain")[0], R.mlp2_case()
    a = (sd["c2.0.weight"], sd["c2.0.bias"], sd["c2.2.weight"], sd["c2.2.bias"])
    m = R.rs_mlp2(c["x"], *a, gather=c["gather"], residual=c["res"], fg=R.fg_layer(sd, "agg_kk"), staged=True)
    lc = R.linear_case(383, 384)
    ly, lmag = R.rs_linear(lc["x"], lc["W"], lc["b"], staged=True)
    for E in R.ROW_COUNTS[1:]:
        a_, b_ = slice(E - 1, E), slice(E - 2, E - 1)
        for kind in ("plain", "offset"):
            _, _, _, exact, staged = R.gru_ref(kind)
            for k in ("net_out", "delta", "weight"):
                if kind == "offset" and k == "weight":
                    continue                                       # (rows of the offset set differ by a few ulps in front of LN2: the sigmoid head levels that)
                assert _crosses_ln(staged[k][b_], staged[k][a_], exact[k][a_], (kind, k)), (E, kind, k)
            for K0 in R.CORR_WIDTHS:
                _, _, _, exact, staged = R.corr_ref(kind, K0)
                assert _crosses_ln(staged[b_], staged[a_], exact[a_], (kind, "out")), (E, kind, K0)
        assert _crosses_lin(m["y"][b_], m["y"][a_], m["y_mag"][a_]) and _crosses_lin(m["fg"][b_], m["fg"][a_], m["fg_mag"][a_]), E
        assert _crosses_lin(ly[b_], ly[a_], lmag[a_]), E


def test_a_dropped_last_element_of_the_last_row_crosses_the_bounds_for_odd_widths():
    for K in (k for k in R.LINEAR_K if k % 2):
        for N in (384, 768):
            c = R.linear_case(K, N)
            st, mag = R.rs_linear(c["x"], c["W"], c["b"], staged=True)
            x = c["x"].clone()
            x[:, K - 1] = 0                                        # (every row: whichever is the last of a call)
            d, _ = R.rs_linear(x, c["W"], c["b"], staged=True)
            assert ((d - st).abs() > R.LINEAR_BOUND * mag).any(-1).all(), (K, N)
    for K0 in (k for k in R.CORR_WIDTHS if k % 2):
        case, _, _, exact, staged = R.corr_ref("plain", K0)
        corr = case["corr"].clone()
        corr[:, K0 - 1] = 0
        d = _corr("plain", K0, corr=corr)
        hit = (R.row_err(d, exact) > R.BOUNDS[("plain", "out")]) & (R.row_err(d, staged) > R.BOUNDS[("plain", "out")])
        assert hit.all(), (K0, (~hit).nonzero().flatten().tolist())


def test_a_one_pass_fp32_variance_crosses_the_bounds_on_the_offset_set():
    """var = q / D - mean^2 in fp32 (what LN2 and LN3 of the chain kernels computed) at |mean| / std near 190"""
    _, _, _, exact, staged = R.gru_ref("offset")
    d = _gru("offset", ln2_one_pass=True)
    assert _crosses_ln(d["net_out"], staged["net_out"], exact["net_out"], ("offset", "net_out")), R.row_err(d["net_out"], exact["net_out"]).max().item()
    for K0 in R.CORR_WIDTHS:
        _, _, _, exact, staged = R.corr_ref("offset", K0)
        d = _corr("offset", K0, ln3_one_pass=True)
        assert _crosses_ln(d, staged, exact, ("offset", "out")), (K0, R.row_err(d, exact).max().item())
