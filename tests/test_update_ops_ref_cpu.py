"""The references, inputs and bounds of tests/update_ops_ref.py, checked without a GPU: the references against torch's own operators,
oracle/update.py and autograd, the special inputs against the properties the GPU tests rely on, and the premise of the large-offset
layer-norm bound (a two-pass fp32 sum in the kernels' order stays under it, a one-pass variance does not)."""
import collections
import pytest
import torch
import torch.nn.functional as F
import update_ops_ref as R
from oracle import update as U

F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_layer_norm_ref_is_torchs_layer_norm_and_the_oracles():
    g = _g(1)
    for dim in (1, 7, 384, 1024):
        x, a, b, res = (torch.randn(33, dim, generator=g, dtype=F64) for _ in range(4))
        gate = torch.randn(33, 2 * dim, generator=g, dtype=F64)
        hy = torch.randn(5, dim, generator=g, dtype=F64)
        grp = torch.randint(0, 5, (33,), generator=g).to(torch.int32)
        gam, bet = torch.randn(dim, generator=g, dtype=F64), torch.randn(dim, generator=g, dtype=F64)
        for eps in (1e-3, 3e-2):
            out, v = R.layer_norm_ref(x, None, None, None, None, None, None, gam, bet, eps, 0)
            assert torch.equal(v, x)
            assert (out - F.layer_norm(x, (dim,), gam, bet, eps)).abs().max() < 1e-12
            pre = x + a + b + hy[grp.long()] + torch.sigmoid(gate[:, :dim]) * res
            out, v = R.layer_norm_ref(x, a, b, hy, grp, gate, res, gam, bet, eps, 1)
            assert (v - pre).abs().max() < 1e-14
            assert (out - torch.relu(F.layer_norm(pre, (dim,), gam, bet, eps))).abs().max() < 1e-12
        out, _ = R.layer_norm_ref(x, a, None, None, None, None, None, gam, bet, 1e-3, 0)
        assert (out - U._ln({"n.weight": gam, "n.bias": bet}, "n", x + a)).abs().max() < 1e-12


def test_softagg_ref_is_the_torch_composition_of_the_module():
    from devo_amd.update import SoftAgg
    g = _g(2)
    dim = 12
    key = R.softagg_groups()
    E = key.numel()
    x = torch.randn(1, E, dim, generator=g, dtype=F64)
    m = SoftAgg(dim).double()
    with torch.no_grad():
        m.h.weight.copy_(torch.eye(dim, dtype=F64)); m.h.bias.zero_()
        got = m(x, key)[0]
        f, gg = F.linear(x[0], m.f.weight, m.f.bias), F.linear(x[0], m.g.weight, m.g.bias)
    _, inv = torch.unique(key, return_inverse=True)
    ref = R.softagg_ref(f, gg, inv)
    assert ref.shape == (len(R.GROUP_SIZES), dim)
    assert (got - ref[inv]).abs().max() < 1e-12


def test_group_tables_are_the_inverse_map_in_stable_order():
    key = R.softagg_groups()
    perm, seg, n, inv = R.group_tables(key)
    assert int(n) == len(R.GROUP_SIZES) and sorted((seg[1:] - seg[:-1]).tolist()) == sorted(R.GROUP_SIZES)
    assert torch.equal(torch.sort(perm.long()).values, torch.arange(key.numel()))
    for s in range(int(n)):
        rows = perm[int(seg[s]):int(seg[s + 1])].long()
        assert bool((inv[rows] == s).all()) and bool((rows[1:] > rows[:-1]).all())
    assert collections.Counter(key.tolist())[977 * 18 + 5] == 130 and int(key.max()) > 100 * int(n)      # sparse keys


def test_analytic_adjoints_are_autograd_of_the_forward_references():
    g = _g(3)
    x, res, dout = (torch.randn(9, 10, generator=g, dtype=F64) for _ in range(3))
    gate = torch.randn(9, 14, generator=g, dtype=F64).requires_grad_(True)
    res.requires_grad_(True)
    ag, ar = torch.autograd.grad((R.gated_residual_ref(x, gate, res) * dout).sum(), (gate, res))
    dg, dr = R.gated_residual_bwd_ref(gate.detach(), res.detach(), dout)
    assert (ag[:, :10] - dg).abs().max() < 1e-14 and (ar - dr).abs().max() < 1e-14 and float(ag[:, 10:].abs().max()) == 0.0
    # SoftAgg: d f_e = w_e dy, d g_e = w_e dy (f_e - y), the form the kernel's comment states
    key = R.softagg_groups()
    _, _, _, inv = R.group_tables(key)
    E = key.numel()
    f, gg, dy = torch.randn(E, 6, generator=g, dtype=F64), torch.randn(E, 6, generator=g, dtype=F64), torch.randn(19, 6, generator=g, dtype=F64)
    df, dgg = R.softagg_bwd_ref(f, gg, inv, dy)
    mx = torch.stack([gg[inv == s].amax(0) for s in range(19)])
    ex = (gg - mx[inv]).exp()
    w = ex / torch.zeros(19, 6, dtype=F64).index_add(0, inv, ex)[inv]
    y = R.softagg_ref(f, gg, inv)
    assert (df - w * dy[inv]).abs().max() < 1e-14 and (dgg - w * dy[inv] * (f - y[inv])).abs().max() < 1e-14


def test_elementwise_references():
    g = _g(4)
    src = torch.randn(7, 5, generator=g).half()
    idx = torch.tensor([-1, 0, 6, 3, -1, 3])
    out = R.masked_gather_ref(src, idx)
    assert out.dtype == src.dtype and torch.equal(out[1:4], src[[0, 6, 3]]) and torch.equal(out[0].view(torch.int16), torch.zeros(5, dtype=torch.int16))
    net, hy = torch.randn(6, 5, generator=g, dtype=F64), torch.randn(3, 5, generator=g, dtype=F64)
    grp = torch.tensor([2, 2, 0, 0, 2, 0], dtype=torch.int32)
    assert torch.equal(R.expand_add_ref(net, hy, grp)[4], net[4] + hy[2])
    W1, W2, b1, b2 = torch.randn(2, 5, generator=g, dtype=F64), torch.randn(2, 5, generator=g, dtype=F64), torch.randn(2, dtype=F64, generator=g), torch.randn(2, dtype=F64, generator=g)
    d, w = R.heads_ref(net, W1, b1, W2, b2)
    assert (d - F.linear(torch.relu(net), W1, b1)).abs().max() < 1e-14 and (w - torch.sigmoid(F.linear(torch.relu(net), W2, b2))).abs().max() < 1e-14
    neg = -net.abs() - 1
    d, w = R.heads_ref(neg, W1, b1, W2, b2)
    assert torch.equal(d, b1.expand(6, 2)) and torch.equal(w, torch.sigmoid(b2).expand(6, 2))


def test_case_table_is_consistent():
    """every kernel of the hand-written list is named by a case of each dtype; ids are unique; every row-wise width of the issue is there"""
    named = {(c["kernel"], c["targ"], c["dtype"]) for c in R.CASES}
    assert named == {(k, t, dt) for k, t in R.KERNELS for dt in (R.F32, R.F16)}
    assert len({c["id"] for c in R.CASES}) == len(R.CASES)
    ln = {(c["dtype"], c["dim"]) for c in R.CASES if c["op"] == "layernorm"}
    assert {d for dt, d in ln if dt == R.F32} == {384, 4, 128, 256, 260, 512, 516, 1024, 2, 6, 1, 7, 1023}
    assert {d for dt, d in ln if dt == R.F16} == {384, 8, 128, 512, 520, 1024, 6, 7}
    for c in R.CASES:
        if c["op"] == "layernorm":
            assert ("gate" in c["terms"]) == (c["ld_gate"] is not None)


# ----------------------------------------------------------------------------------------------------------------- special inputs
@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_softagg_special_inputs(dtype):
    dim = 8
    _, _, _, inv = R.group_tables(R.softagg_groups())
    # dominated: every other row's fp64 weight is below 1e-60, the result is the dominating row's f
    f, g, key, dom = R.softagg_inputs(dtype, dim, "dominated")
    f, g = f.double(), g.double()
    perm, seg, _, _ = R.group_tables(key)
    ranks_33 = None
    for s in range(len(R.GROUP_SIZES)):
        rows = perm[int(seg[s]):int(seg[s + 1])].long()
        w = torch.softmax(g[rows], 0)
        cols = torch.arange(dim)
        assert bool((g[dom[s], cols] == R.DOMINATING).all())
        w[(rows[:, None] == dom[s][None]).nonzero()[:, 0], (rows[:, None] == dom[s][None]).nonzero()[:, 1]] = 0.0
        assert float(w.max()) < 1e-60
        if rows.numel() == 33:
            ranks_33 = {int((rows == dom[s][c]).nonzero()) for c in range(dim)}
    assert ranks_33 == {0, 32, 12, 24}                          # first, last, the middle of the second batch of 8 and of 16 rows
    y = R.softagg_ref(f, g, inv)
    assert (y - f[dom, torch.arange(dim)[None].expand_as(dom)]).abs().max() < 1e-50
    # shifted: the inputs sit at 1000 in the case's dtype, and without the maximum subtracted an fp32 exponential overflows
    f, g, _, _ = R.softagg_inputs(dtype, dim, "shifted")
    assert float(g.float().min()) > 990 and not bool(torch.isfinite(g.float().exp()).any())
    assert bool(torch.isfinite(R.softagg_ref(f.double(), g.double(), inv)).all())
    assert g.unique().numel() > 4                               # ... and still differ from row to row
    # equal: the plain mean
    f, g, _, _ = R.softagg_inputs(dtype, dim, "equal")
    mean = torch.stack([f.double()[inv == s].mean(0) for s in range(len(R.GROUP_SIZES))])
    assert (R.softagg_ref(f.double(), g.double(), inv) - mean).abs().max() < 1e-13
    # size-1 groups: y == f
    f, g, _, _ = R.softagg_inputs(dtype, dim, "plain")
    y = R.softagg_ref(f.double(), g.double(), inv)
    one = [s for s in range(len(R.GROUP_SIZES)) if int((inv == s).sum()) == 1]
    assert len(one) == 1 and torch.equal(y[one[0]], f.double()[inv == one[0]][0])


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_gate_saturation_values(dtype):
    """+-30 and the large values are exact in the dtype; the fp64 sigmoid is within 1e-13 of 0 / 1 there, and s (1 - s) below 2^-43"""
    gate, kind = R.gate_with_saturation(torch.zeros(6, 7, dtype=R.TORCH_DTYPE[dtype]), dtype)
    assert set(kind.unique().tolist()) == {0, 1, 2, 3, 4} and bool((kind[0] == 0).all()) and bool((kind[5] == 0).all())
    for k, v in enumerate(R.GATE_SAT[dtype], 1):
        assert bool((gate[kind == k].double() == v).all())
    s = torch.sigmoid(gate.double())
    assert bool((s[(kind == 1) | (kind == 3)] > 1 - 1e-13).all()) and bool((s[(kind == 2) | (kind == 4)] < 1e-13).all())
    assert float((s * (1 - s))[kind > 0].max()) < 2.0 ** -43


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_layer_norm_special_rows(dtype):
    for dim in (1, 7, 384):
        x, kinds = R.ln_special_rows(dtype, dim)
        assert kinds[:5] == ["big", "bigconst", "eps", "off4", "const"] and set(kinds[5:]) == {"big", "off4", "eps", "rand"}
        x = x.double()
        gam, bet = torch.full((dim,), 1.5, dtype=F64), torch.linspace(-1, 1, dim, dtype=F64)
        for relu in (0, 1):
            out, _ = R.layer_norm_ref(x, None, None, None, None, None, None, gam, bet, 1e-3, relu)
            want = torch.relu(bet) if relu else bet
            for i in (1, 4) if dim > 1 else range(R.E_MAX):    # constant rows, and every row of width 1, give beta
                assert (out[i] - want).abs().max() < 1e-12
        if dim == 384:
            i = kinds.index("eps")
            var = float(x[i].var(unbiased=False))
            assert 2e-4 < var < 8e-4                           # comparable to eps
            a, _ = R.layer_norm_ref(x[i:i + 1], None, None, None, None, None, None, gam, bet * 0, 1e-3, 0)
            b, _ = R.layer_norm_ref(x[i:i + 1], None, None, None, None, None, None, gam, bet * 0, 3e-2, 0)
            c, _ = R.layer_norm_ref(x[i:i + 1], None, None, None, None, None, None, gam, bet * 0, 0.0, 0)
            assert float((a / b)[0, 0]) > 3 and float((c / a)[0, 0]) > 1.3        # a wrong or ignored eps moves the row by tens of percent


FORMS = [("scalar", R.F32, 7, "k_layernorm", "false"), ("q", R.F32, 384, "k_layernorm_q", None), ("pairs", R.F32, 1024, "k_layernorm", "true"),
         ("v", R.F32, 512, "k_layernorm_v", None), ("scalar", R.F32, 1023, "k_layernorm", "false"), ("q", R.F16, 384, "k_layernorm_q", None),
         ("v", R.F16, 1024, "k_layernorm_v", None)]


@pytest.mark.parametrize("form,dtype,dim,kernel,targ", FORMS)
def test_large_offset_bound_separates_two_pass_from_one_pass(form, dtype, dim, kernel, targ):
    """the premise of the large-offset bound: an fp32 restatement that sums like the kernels (lane-strided partial sums, then the butterfly
    over 64 lanes or the 16-lane row sum) stays under it; the one-pass variance E[x^2] - E[x]^2 with the very same sums exceeds it by
    at least 10x at offset 100"""
    x, kinds = R.ln_special_rows(dtype, dim)
    g = _g(5)
    gam, bet = R._q(torch.randn(dim, generator=g), dtype), R._q(torch.randn(dim, generator=g), dtype)
    eps = 1e-3
    ref, v = R.layer_norm_ref(x.double(), None, None, None, None, None, None, gam.double(), bet.double(), eps, 0)
    p, tree = R.ln_elems_per_lane(kernel, targ, dtype, dim)
    assert (p, tree) == {("scalar", 7): (1, 6), ("q", 384): (24, 4), ("pairs", 1024): (16, 6), ("v", 512): (8, 6), ("scalar", 1023): (16, 6), ("v", 1024): (16, 6)}[(form, dim)]
    big = torch.tensor([k in ("big", "bigconst") for k in kinds])
    extra = R.ln_offset_extra(v, gam, eps, p, tree) * big[:, None]
    bd32 = R.bound(ref, R.F32, extra)                           # the fp32 part of the bound (no storage rounding in the restatement)
    two = R.layer_norm_kernel_like_f32(x, gam, bet, eps, form, dtype).double()
    r2 = ((two - ref).abs() / bd32).amax(-1)
    assert float(r2.max()) < 1.0, float(r2.max())
    rnd = torch.tensor([k == "big" for k in kinds])
    if dtype == R.F32:                                          # offset 100 (fp16 rows sit at 16: exact products, a smaller gap)
        one = R.layer_norm_kernel_like_f32(x, gam, bet, eps, form, dtype, one_pass=True).double()
        r1 = ((one - ref).abs() / bd32).amax(-1)[rnd]
        assert float(r1.max()) >= 10.0, float(r1.max())
    # rows at offset 4 stay under the plain bound
    off4 = torch.tensor([k == "off4" for k in kinds])
    assert float(((two - ref).abs() / R.bound(ref, R.F32)).amax(-1)[off4].max()) < 1.0
