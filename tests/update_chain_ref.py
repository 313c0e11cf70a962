"""Staged fp64 oracle of the row-resident chain kernels (devo_amd/csrc/gemm_rs.hip) and the deterministic inputs of their tests.

One function per kernel contract.  Each takes fp16-exact operands widened to fp64, computes in fp64 and — `staged=True` — rounds to fp16
exactly where the kernel stores fp16 (to LDS or to memory); `staged=False` is the exact fp64 composition.  The kernels hold fp32 in
front of every such store, so `r16` rounds through fp32 like they do.  Every LayerNorm here is two-pass.  The composition follows
oracle/update.py (`_ln`, `segment_softmax_sum`, `gated_residual`) — tests/test_update_chain_ref_cpu.py ties the two together — and the
rounding points are read off the kernels (gemm_rs.hip:<line> in the comments).
"""
import math
import numpy as np
import torch

D = 384
ROW_COUNTS = (1, 15, 17, 31, 33, 95, 96, 97, 193, 289)       # around the 16-row matrix tiles, the 32-row rounds, the 96-row workgroup tile
PREFIX_EXTRA = 40                                            # prefix independence: the same rows inside a call with this many more
BASE_ROWS = ROW_COUNTS[-1] + PREFIX_EXTRA
ROW_ZERO, ROW_CONST, ROW_BIG, ROWS_SAT = 3, 5, 7, (9, 11)    # the special rows of the `plain` set
SAT_BLOCK = slice(64, 80)                                    # gate weight columns scaled by SAT_SCALE; only the ROWS_SAT rows are large there
SAT_SCALE = 32.0
ULP, OFFSET_HAIR, OFFSET_BITS = 2.0 ** -8, 4 * 2.0 ** -10, 16       # fp16 spacing in [4, 8); see make_params
OFFSET_RES_SCALE = 0.004                                     # the `offset` set: res[2] of both GatedResiduals, weights and biases

LINEAR_BOUND = 2e-3                                          # |got - staged| <= LINEAR_BOUND * (magnitude of the output's terms): the project's figure
SPLIT_BOUND = 1e-6                                           # fp32 storage, exact hi + lo splits (test_row_resident_split_linear_agrees_with_the_ring_kernel)

# Outputs behind a LayerNorm or a sigmoid: max_i |got_i - exact_i| / rms(exact row) against the staged=False oracle.  Each constant is
# TWICE the figure measured for the layer-wise path (update.RS_CHAINS = False: csrc/mlp2.hip, the LayerNorm / heads kernels of
# csrc/update.hip and the one-layer products, each tested on its own) on an MI355X at these very inputs (BASE_ROWS rows, K0 = 882):
# the chain sums in another order and rounds the gate once more, both below one fp16 ulp per stage.  The chain kernels were never
# measured to set their own bound.  (delta: two elements per row, so a row whose two outputs nearly cancel decides the figure.)
LAYERWISE_MEASURED = {
    ("plain", "out"): 2.523e-3, ("plain", "net_out"): 3.757e-3, ("plain", "delta"): 1.807e-2, ("plain", "weight"): 8.352e-4,
    ("offset", "out"): 2.044e-3, ("offset", "net_out"): 3.093e-3, ("offset", "delta"): 5.326e-3, ("offset", "weight"): 1.064e-3,
}
BOUNDS = {k: 2.0 * v for k, v in LAYERWISE_MEASURED.items()}


def q16(t):
    """the nearest fp16-exact fp64 values (inputs and parameters)"""
    return t.to(torch.float16).to(torch.float64)


def r16(t, staged=True):
    """a kernel's fp16 store of an fp32 value"""
    return t.to(torch.float32).to(torch.float16).to(torch.float64) if staged else t


def row_err(got, exact):
    """max_i |got_i - exact_i| / rms(exact row), per row"""
    got, exact = got.double(), exact.double()
    rms = exact.pow(2).mean(-1).sqrt().clamp(min=1e-30)
    return (got - exact).abs().amax(-1) / rms


def lin(x, W, b):
    return x @ W.t() + b


def lin_mag(x, W, b):
    return x.abs() @ W.abs().t() + b.abs()


def layer_norm(x, g, b, eps):
    """two-pass LayerNorm (oracle/update.py:_ln in fp64)"""
    d = x - x.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * g + b


def layer_norm_one_pass_f32(x, g, b, eps):
    """THE DEFECT form: var = q / D - mean^2 in fp32 with the chain kernels' partial sums (12 elements per lane, the four lanes of a row,
    the eight waves: what LN2 / LN3 of the chain kernels computed before rs_row_stats)"""
    t = x.to(torch.float32).numpy().reshape(x.shape[0], 8, 3, 4, 4)          # [row][wave][tile][kg][r]: column 48 w + 16 t + 4 kg + r
    s = np.zeros((x.shape[0], 8, 4), np.float32)
    q = np.zeros((x.shape[0], 8, 4), np.float32)
    for tt in range(3):
        for r in range(4):
            v = t[:, :, tt, :, r]
            s = (s + v).astype(np.float32)
            q = (q + (v * v).astype(np.float32)).astype(np.float32)
    s = ((s[:, :, 0] + s[:, :, 1]).astype(np.float32) + (s[:, :, 2] + s[:, :, 3]).astype(np.float32)).astype(np.float32)
    q = ((q[:, :, 0] + q[:, :, 1]).astype(np.float32) + (q[:, :, 2] + q[:, :, 3]).astype(np.float32)).astype(np.float32)
    S = np.zeros(x.shape[0], np.float32)
    Q = np.zeros(x.shape[0], np.float32)
    for w in range(8):
        S = (S + s[:, w]).astype(np.float32)
        Q = (Q + q[:, w]).astype(np.float32)
    mean = (S / np.float32(D)).astype(np.float32)
    var = np.maximum((Q / np.float32(D)).astype(np.float32) - (mean * mean).astype(np.float32), np.float32(0)).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    mean, rstd = torch.from_numpy(mean).double()[:, None], torch.from_numpy(rstd).double()[:, None]
    return (x - mean) * rstd * g + b


# ------------------------------------------------------------------------------------------------------------------ kernel contracts
def rs_linear(x, W, b, residual=None, relu_from=None, staged=False):
    """devo_upd_rs_linear_f16 (k_rs_linear_f16): y = act(x W^T + b) [+ residual], one fp16 store (gemm_rs.hip:168) -> (y, term magnitude)"""
    y, mag = lin(x, W, b), lin_mag(x, W, b)
    if relu_from is not None:
        y = torch.cat([y[:, :relu_from], y[:, relu_from:].clamp(min=0)], 1)
    if residual is not None:
        y, mag = y + residual, mag + residual.abs()
    return r16(y, staged), mag


def gather_rows(x, gather):
    """rows x[gather]; an index that is negative or >= the row count of x is a zero row (gemm_rs.hip:529-530)"""
    if gather is None:
        return x
    ok = (gather >= 0) & (gather < x.shape[0])
    return torch.where(ok[:, None], x[gather.clamp(0, x.shape[0] - 1)], torch.zeros((), dtype=x.dtype))


def rs_mlp2(x, W1, b1, W2, b2, gather=None, residual=None, fg=None, staged=False):
    """devo_upd_rs_mlp2_fg_f16 (k_rs_mlp2_f16<true, FG>): y = l2(relu(l1(x[gather]))) [+ residual]; fg = (Wfg [768, 384], bfg): the f | g
    layer on the rows of y.  -> dict(y, y_mag, fg, fg_mag)"""
    xs = gather_rows(x, gather)
    h = r16(torch.relu(lin(xs, W1, b1)), staged)                     # relu(h) into R (gemm_rs.hip:581)
    y, mag = lin(h, W2, b2), lin_mag(h, W2, b2)
    if residual is not None:
        y, mag = y + residual, mag + residual.abs()
    y = r16(y, staged)                                               # the result rows into X, then to memory (gemm_rs.hip:614)
    out = dict(y=y, y_mag=mag, fg=None, fg_mag=None)
    if fg is not None:
        out["fg"], out["fg_mag"] = r16(lin(y, *fg), staged), lin_mag(y, *fg)      # f | g halves through R (gemm_rs.hip:639)
    return out


def rs_expand_fg(x, hy, grp, Wfg, bfg, staged=False):
    """devo_upd_rs_expand_fg_f16 (k_rs_mlp2_f16<false, true>): x += hy[grp] in place; fg = x [Wf | Wg]^T + b -> dict(x, fg, fg_mag)"""
    x = r16(x + hy[grp.long()], staged)                                     # x + hy[grp.long()] as the expand-add stores it (gemm_rs.hip:549)
    return dict(x=x, fg=r16(lin(x, Wfg, bfg), staged), fg_mag=lin_mag(x, Wfg, bfg))      # (gemm_rs.hip:639)


def rs_gru(x, hy, grp, sd, eps0, eps2, staged=False, ln2_one_pass=False):
    """devo_upd_rs_gru_f16 (k_rs_gru_f16): LN0(x + hy[grp.long()]) -> GatedResidual -> LN2 -> GatedResidual -> heads, sd with the operator's
    state-dict keys -> dict(net_out, delta, weight)"""
    X = r16(layer_norm(x + hy[grp.long()], sd["gru.0.weight"], sd["gru.0.bias"], eps0), staged)          # LN0 output into X (gemm_rs.hip:362); the sum stays fp32
    for rep, key in enumerate(("gru.1", "gru.3")):                   # oracle/update.py:gated_residual with the kernel's stores
        R = r16(torch.relu(lin(X, sd[key + ".res.0.weight"], sd[key + ".res.0.bias"])), staged)  # relu(h) into R (gemm_rs.hip:393)
        res = r16(lin(R, sd[key + ".res.2.weight"], sd[key + ".res.2.bias"]), staged)             # res into R (gemm_rs.hip:408)
        gate = r16(lin(X, sd[key + ".gate.0.weight"], sd[key + ".gate.0.bias"]), staged)          # the gate through rs_pack4 (gemm_rs.hip:423)
        t = X + torch.sigmoid(gate) * res
        if rep == 0:
            ln = layer_norm_one_pass_f32 if ln2_one_pass else layer_norm
            X = r16(ln(t, sd["gru.2.weight"], sd["gru.2.bias"], eps2), staged)                    # LN2 output into X (gemm_rs.hip:438)
        else:
            X = r16(t, staged)                                       # the new state into X (gemm_rs.hip:446), to memory as it is
    a = torch.relu(X)
    delta = r16(lin(a, sd["d.1.weight"], sd["d.1.bias"]), staged)                                 # (gemm_rs.hip:492)
    weight = r16(torch.sigmoid(lin(a, sd["w.1.weight"], sd["w.1.bias"])), staged)                 # (gemm_rs.hip:493)
    return dict(net_out=X, delta=delta, weight=weight)


def rs_corr(corr, net, inp, sd, eps3, eps, staged=False, ln3_one_pass=False):
    """devo_upd_rs_corr_f16 (k_rs_corr_f16): out = LN(net + inp + l5(relu(LN3(l2(relu(l0(corr))))))); `net` may be fp32 values (the
    _net32 form: it enters the sum unrounded) -> out"""
    h = r16(torch.relu(lin(corr, sd["corr.0.weight"], sd["corr.0.bias"])), staged)                # relu(h) into R (gemm_rs.hip:754)
    l2 = r16(lin(h, sd["corr.2.weight"], sd["corr.2.bias"]), staged)                              # the rounded l2 output in front of LN3 (gemm_rs.hip:765)
    ln = layer_norm_one_pass_f32 if ln3_one_pass else layer_norm
    X = r16(torch.relu(ln(l2, sd["corr.3.weight"], sd["corr.3.bias"], eps3)), staged)             # relu(LN3) into X (gemm_rs.hip:777)
    c = r16(lin(X, sd["corr.5.weight"], sd["corr.5.bias"]), staged)                               # c into R (gemm_rs.hip:788)
    return r16(layer_norm(net + inp + c, sd["norm.weight"], sd["norm.bias"], eps), staged)        # (gemm_rs.hip:851)


def soft_agg_sum(fg, group_of):
    """the SoftAgg kernel between the chain launches (not under test here): oracle/update.py:segment_softmax_sum on the f | g halves"""
    from oracle.update import segment_softmax_sum
    return segment_softmax_sum(fg[None, :, :D], fg[None, :, D:], group_of)[0]


# ------------------------------------------------------------------------------------------------------------------ inputs
_LAYERS = ("corr.0", "corr.2", "corr.5", "c1.0", "c1.2", "c2.0", "c2.2", "agg_kk.f", "agg_kk.g", "agg_kk.h", "agg_ij.f", "agg_ij.g", "agg_ij.h",
           "gru.1.gate.0", "gru.1.res.0", "gru.1.res.2", "gru.3.gate.0", "gru.3.res.0", "gru.3.res.2", "d.1", "w.1")
_NORMS = ("corr.3", "norm", "gru.0", "gru.2")
EPS = {"plain": {"corr.3": 1e-3, "norm": 3e-2, "gru.0": 3e-3, "gru.2": 1e-2},       # pairwise different, the pair of each chain well apart
       "offset": {"corr.3": 1e-5, "norm": 3e-3, "gru.0": 1e-3, "gru.2": 3e-6}}       # (a small epsilon leaves LN2 / LN3 their variance)


def make_params(kind, K0=882, seed=1):
    """-> (sd, eps): fp16-exact fp64 parameters under the operator's state-dict keys, the epsilons by LayerNorm key.
    plain: weights randn / sqrt(K); every bias, gamma and beta nonzero and distinct per layer; Wd != Ww; SAT_BLOCK of the gate weights
    scaled.  offset: LN2's and LN3's input rows with |mean| / std near 100 (checked by the CPU tests)."""
    assert kind in ("plain", "offset")
    g = torch.Generator().manual_seed(1000 * seed + K0)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {}
    for i, key in enumerate(_LAYERS):
        n = 2 if key in ("d.1", "w.1") else D
        k = K0 if key == "corr.0" else D
        sd[key + ".weight"] = rn(n, k) / math.sqrt(k)
        sd[key + ".bias"] = 0.1 * rn(n) + 0.03 * (i + 1) * (-1) ** i
    for i, key in enumerate(_NORMS):
        sd[key + ".weight"] = 1.0 + 0.1 * rn(D) + 0.05 * i
        sd[key + ".bias"] = 0.1 * rn(D) - 0.04 * (i + 1)
    for key in ("gru.1.gate.0.weight", "gru.3.gate.0.weight"):
        sd[key][:, SAT_BLOCK] *= SAT_SCALE
    if kind == "offset":
        # Sharper than "gamma 0.04, res and W2 scaled by 0.02": a row that reaches LN2 / LN3 through an fp16 store carries that store's
        # rounding (half an ulp of 4 is 2e-3) next to a spread of 4 / 100, which alone puts ANY fp16 path 4e-2 from the exact result and
        # hides a wrong statistic (3e-3).  So the rows enter on fp16's own grid near 4 and 6 (ULP apart), a hair (ULP * OFFSET_HAIR) beyond
        # it so that every path rounds them the same way:
        #   LN0: gamma = ULP (1 + hair) / rstd of a row of +-1 (gru_case), beta = 4 + 0.018 randn  ->  X = beta +- ULP;
        #   l2:  h[:, j] = corr[:, j] in {0, 1} for j < OFFSET_BITS (unit rows of W0, corr_case), W2[n, n % OFFSET_BITS] = +-ULP (1 + hair),
        #        b2 = 6 + 0.032 randn  ->  l2 = b2 + {0, +-ULP};
        # the rest of the spread comes from sigmoid(gate) * res, whose own fp16 steps are a hundred times finer.
        sd["gru.0.weight"] = torch.full((D,), ULP * (1 + OFFSET_HAIR) * math.sqrt(1.0 + EPS["offset"]["gru.0"]), dtype=torch.float64)
        sd["gru.0.bias"] = torch.round((4.0 + 0.018 * rn(D)) / ULP) * ULP           # (on the grid below 4 as well, where fp16 is finer)
        for key in ("gru.1.res.2.weight", "gru.1.res.2.bias", "gru.3.res.2.weight", "gru.3.res.2.bias"):
            sd[key] = sd[key] * OFFSET_RES_SCALE
        for key in ("gru.1.gate.0.weight", "gru.3.gate.0.weight"):
            sd[key][:, SAT_BLOCK] /= SAT_SCALE
        sd["corr.0.weight"][:OFFSET_BITS] = 0
        sd["corr.0.weight"][:OFFSET_BITS, :OFFSET_BITS] = torch.eye(OFFSET_BITS, dtype=torch.float64)
        sd["corr.0.bias"][:OFFSET_BITS] = 0
        sign = torch.sign(rn(D))
        sd["corr.2.weight"] = torch.zeros(D, D, dtype=torch.float64)
        sd["corr.2.weight"][torch.arange(D), torch.arange(D) % OFFSET_BITS] = sign * ULP * (1 + OFFSET_HAIR)
        sd["corr.2.bias"] = 6.0 + 0.032 * rn(D)
    return {k: q16(v) for k, v in sd.items()}, dict(EPS[kind])


def make_rows(kind, width, seed, rows=BASE_ROWS, scale=0.5):
    """[rows, width] fp16-exact inputs.  plain: row ROW_ZERO all zero, ROW_CONST constant, ROW_BIG scaled by 200, and (width 384) the
    SAT_BLOCK columns zero except in the ROWS_SAT rows, where they are large: with the scaled gate weights those rows' gates saturate.
    Every row count of the tests takes a prefix of these rows."""
    g = torch.Generator().manual_seed(77 * seed + width)
    x = scale * torch.randn(rows, width, generator=g, dtype=torch.float64)
    if kind == "plain":
        x[ROW_ZERO] = 0
        x[ROW_CONST] = 0.375
        x[ROW_BIG] *= 200
        if width == D:
            x[:, SAT_BLOCK] = 0
            for r in ROWS_SAT:
                x[r, SAT_BLOCK] = 6.0 * torch.sign(torch.randn(SAT_BLOCK.stop - SAT_BLOCK.start, generator=g, dtype=torch.float64))
    return q16(x)


def make_groups(rows, seed, n_groups=23):
    """edge -> group (i32) with group 0 and the last group in use; the rows of the groups' table hy; hy[0] is zero with the zero row in it"""
    g = torch.Generator().manual_seed(31 * seed)
    grp = torch.randint(0, n_groups, (rows,), generator=g, dtype=torch.int32)
    grp[0], grp[1 % rows] = n_groups - 1, 0
    if rows > ROW_ZERO:
        grp[ROW_ZERO] = 0
    return grp


def gru_case(kind, seed=3):
    """-> dict(x, hy, grp): the inputs of the gru chain, BASE_ROWS rows.  offset: rows of +-1, as many of each, and no group term: mean 0
    and variance 1 exactly, so that LN0 puts them on fp16's grid around beta (make_params)"""
    grp = make_groups(BASE_ROWS, seed)
    if kind == "offset":
        g = torch.Generator().manual_seed(13 * seed)
        x = torch.ones(BASE_ROWS, D, dtype=torch.float64)
        for r in range(BASE_ROWS):
            x[r, torch.randperm(D, generator=g)[:D // 2]] = -1.0
        return dict(x=x, hy=torch.zeros(23, D, dtype=torch.float64), grp=grp)
    x = make_rows(kind, D, seed)
    hy = make_rows("offset", D, seed + 1, rows=23, scale=0.3)        # (no special rows of its own)
    hy[0] = 0
    hy[:, SAT_BLOCK] = 0
    return dict(x=x, hy=q16(hy), grp=grp)


def corr_case(kind, K0, seed=5):
    """-> dict(corr, net, inp): the inputs of the correlation chain, BASE_ROWS rows.  offset: the first OFFSET_BITS inputs are 0 or 1 (make_params)"""
    small = 1.0 if kind == "offset" else 0.5                         # (offset: as large as c, which carries LN3's error: alone, the last LayerNorm would divide a wrong scale out again)
    net = make_rows("offset", D, seed + 1, scale=small)
    inp = make_rows("offset", D, seed + 2, scale=small)
    corr = make_rows(kind, K0, seed, scale=1.0)
    if kind == "offset":
        g = torch.Generator().manual_seed(17 * seed)
        corr[:, :OFFSET_BITS] = torch.randint(0, 2, (BASE_ROWS, OFFSET_BITS), generator=g).double()
    return dict(corr=corr, net=net, inp=inp)


def mean_over_std(t):
    """|mean| / std of every row"""
    return t.mean(-1).abs() / t.std(-1, unbiased=False)


def ln2_input(case, sd, eps0):
    """the rows LN2 of the gru chain normalises (exact composition)"""
    X = layer_norm(case["x"] + case["hy"][case["grp"].long()], sd["gru.0.weight"], sd["gru.0.bias"], eps0)
    gate = lin(X, sd["gru.1.gate.0.weight"], sd["gru.1.gate.0.bias"])
    res = lin(torch.relu(lin(X, sd["gru.1.res.0.weight"], sd["gru.1.res.0.bias"])), sd["gru.1.res.2.weight"], sd["gru.1.res.2.bias"])
    return X + torch.sigmoid(gate) * res, gate


def ln3_input(case, sd):
    """the rows LN3 of the correlation chain normalises (exact composition)"""
    return lin(torch.relu(lin(case["corr"], sd["corr.0.weight"], sd["corr.0.bias"])), sd["corr.2.weight"], sd["corr.2.bias"])


# ------------------------------------------------------------------------------------------------------------------ the tests' cases
import functools

LAST_COL = 4.0          # plain corr rows / the Linear tests' rows: the last input column and its weight column are large, so that a dropped
                        # x[M - 1, K - 1] (odd K: the dword that straddles the end of the buffer) is far above every bound
CORR_WIDTHS = (865, 881, 882, 896)
LINEAR_K = (353, 360, 377, 383, 384)
GATHER_ROWS = BASE_ROWS + 37                                 # source rows of the gathered mlp2 cases


@functools.lru_cache(maxsize=None)
def params(kind, K0=882):
    sd, eps = make_params(kind, K0)
    if kind == "plain":
        sd["corr.0.weight"][:, K0 - 1] = q16(sd["corr.0.weight"][:, K0 - 1] * LAST_COL)
    return sd, eps


@functools.lru_cache(maxsize=None)
def gru_ref(kind):
    """-> (case, sd, eps, exact, staged) of the gru chain over BASE_ROWS rows; shared, never modified"""
    (sd, eps), case = params(kind), gru_case(kind)
    run = lambda staged: rs_gru(case["x"], case["hy"], case["grp"], sd, eps["gru.0"], eps["gru.2"], staged=staged)
    return case, sd, eps, run(False), run(True)


@functools.lru_cache(maxsize=None)
def corr_ref(kind, K0):
    """-> (case, sd, eps, exact, staged) of the correlation chain over BASE_ROWS rows; shared, never modified"""
    (sd, eps), case = params(kind, K0), corr_case(kind, K0)
    if kind == "plain":
        case["corr"][:, K0 - 1] = LAST_COL
    run = lambda staged: rs_corr(case["corr"], case["net"], case["inp"], sd, eps["corr.3"], eps["norm"], staged=staged)
    return case, sd, eps, run(False), run(True)


def fg_layer(sd, name):
    """the concatenated f | g layer of a SoftAgg: (W [768, 384], b [768])"""
    return torch.cat([sd[name + ".f.weight"], sd[name + ".g.weight"]], 0), torch.cat([sd[name + ".f.bias"], sd[name + ".g.bias"]], 0)


@functools.lru_cache(maxsize=None)
def mlp2_case():
    """-> dict(x [GATHER_ROWS, 384], res [BASE_ROWS, 384], gather [BASE_ROWS] with -1, indices >= GATHER_ROWS and duplicates)"""
    g = torch.Generator().manual_seed(41)
    idx = torch.randint(0, GATHER_ROWS, (BASE_ROWS,), generator=g)
    idx[2::7] = -1
    idx[4::11] = GATHER_ROWS + torch.arange(len(idx[4::11])) * 3         # (the first of them: exactly the row count)
    idx[6::13] = idx[5::13][:len(idx[6::13])]                             # duplicates next to each other
    idx[BASE_ROWS - 1] = idx[0]
    return dict(x=make_rows("plain", D, 11, rows=GATHER_ROWS), res=make_rows("offset", D, 12), gather=idx)


@functools.lru_cache(maxsize=None)
def linear_case(K, N):
    """-> dict(x [BASE_ROWS, K], W [N, K], b, res [BASE_ROWS, N]) with the last column of x and of W large"""
    g = torch.Generator().manual_seed(100 * K + N)
    x = make_rows("plain", K, 21)
    x[:, K - 1] = 2 * LAST_COL
    W = torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K)
    W[:, K - 1] *= 2 * LAST_COL * math.sqrt(K) / 4
    return dict(x=x, W=q16(W), b=q16(0.1 * torch.randn(N, generator=g, dtype=torch.float64) + 0.05), res=make_rows("offset", N, 22))
