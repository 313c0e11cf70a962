"""Plain references of the update operator's row kernels (devo_amd/csrc/update.hip), their bounds, their inputs and the case table.

One function per contract, ordinary torch on the CPU, in the dtype of its inputs: fp64 is the yardstick.  fp16 cases hand the functions
fp16-exact values widened to fp64 (update_chain_ref.q16); the kernels compute in fp32 and round once at the store, so nothing here rounds
in between.  tests/test_update_ops_ref_cpu.py ties these functions to torch.nn.functional.layer_norm, oracle/update.py and autograd;
tests/test_gpu_update_ops.py runs every case of CASES against them and checks that each case reaches the kernel it names.
"""
import numpy as np
import torch
from oracle.update import segment_softmax_sum
from update_chain_ref import q16  # noqa: F401  (the fp16 cases' inputs)

F32, F16 = "f32", "f16"
TORCH_DTYPE = {F32: torch.float32, F16: torch.float16}
CHUNK = {F32: 4, F16: 8}                                     # elements of a 16-byte chunk

ROW_COUNTS = (1, 3, 4, 5, 15, 16, 17, 33, 65)                # around the 4-row and the 16-row (quarter wave) workgroups
E_MAX = ROW_COUNTS[-1]
POISON_ROWS = 2                                              # rows behind the last one that must keep their bits
POISON = -1234.0                                             # exact in fp16

GROUP_SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 40, 41, 47, 48, 63, 64, 65, 100, 130)
SOFTAGG_SETS = ("plain", "dominated", "shifted", "equal")
DOMINATING = 200.0
LN_BIG_OFFSET = {F32: 100.0, F16: 16.0}


# ----------------------------------------------------------------------------------------------------------------- references
def layer_norm_ref(x, a, b, hy, group_of, gate, res, gamma, beta, eps, relu):
    """LN(x + a + b + hy[group_of] + sigmoid(gate) * res) * gamma + beta: two-pass, biased variance, optional ReLU.  Any term may be
    None.  `gate` may be wider than x (its own row stride): its first dim columns count.  Returns (out, v), v the normalised sum."""
    v = x.clone()
    if a is not None:
        v = v + a
    if b is not None:
        v = v + b
    if hy is not None:
        v = v + hy[group_of.long()]
    if gate is not None:
        v = v + torch.sigmoid(gate[:, :x.shape[1]]) * res
    d = v - v.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True)
    out = d / torch.sqrt(var + eps) * gamma + beta
    return (torch.relu(out) if relu else out), v


def masked_gather_ref(src, idx):
    """out[e] = src[idx[e]] where idx[e] >= 0, else +0"""
    return torch.where((idx >= 0)[:, None], src[idx.clamp(min=0)], torch.zeros((), dtype=src.dtype))


def expand_add_ref(net, hy, group_of):
    return net + hy[group_of.long()]


def gated_residual_ref(x, gate, res):
    return x + torch.sigmoid(gate[:, :x.shape[1]]) * res


def gated_residual_bwd_ref(gate, res, dout):
    s = torch.sigmoid(gate[:, :res.shape[1]])
    return dout * res * s * (1 - s), dout * s


def softagg_ref(f, g, group_of):
    """y[s] = sum over the rows e of group s of f[e] * softmax over the group of g[e], channel-wise (blocks.py:42-43)"""
    return segment_softmax_sum(f[None], g[None], group_of.long())[0]


def softagg_bwd_ref(f, g, group_of, dy):
    """(df, dg) of sum(softagg_ref(f, g) * dy) by autograd"""
    f = f.detach().clone().requires_grad_(True)
    g = g.detach().clone().requires_grad_(True)
    y = softagg_ref(f, g, group_of)
    return torch.autograd.grad((y * dy).sum(), (f, g))


def heads_ref(net, Wd, bd, Ww, bw):
    r = torch.relu(net)
    return r @ Wd.t() + bd, torch.sigmoid(r @ Ww.t() + bw)


# ----------------------------------------------------------------------------------------------------------------- bounds
def row_scale(ref):
    """max(1, max |ref row|), per row (the form of test_gpu_lietorch)"""
    return ref.abs().amax(-1, keepdim=True).clamp(min=1.0)


def bound(ref, dtype, extra=None):
    """element-wise bound against the fp64 reference.  fp32 storage: 1e-5 of the row's scale (the project's figure for these ops in
    test_update_single_ops).  fp16 storage: one fp16 rounding of an fp32 value (half an ulp, doubled for the binade edge: 2^-10 |ref|),
    the subnormal floor 2^-24, and the same fp32 term.  `extra` [rows, 1] is added (layer norm's large-offset rows)."""
    ref = ref.double()
    bd = 1e-5 * row_scale(ref).expand_as(ref)
    if dtype == F16:
        bd = bd + 2.0 ** -10 * ref.abs() + 2.0 ** -24
    if extra is not None:
        bd = bd + extra
    return bd


def err_ratio(got, ref, dtype, extra=None):
    """max |got - ref| / bound; inf if anything is not finite"""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return float(((got - ref.double()).abs() / bound(ref, dtype, extra)).max())


def ln_elems_per_lane(kernel, targ, dtype, dim):
    """(p, tree): the row elements one lane sums in that layer-norm kernel and the number of cross-lane steps counted with them in the
    bound: 6 for a 64-lane butterfly, 4 for the 16-lane row sum of the quarter-wave form"""
    V = CHUNK[dtype]
    if kernel == "k_layernorm_q":
        return dim // 16, 4
    if kernel == "k_layernorm_v":
        return V * ((dim // V + 63) // 64), 6
    if targ == "true":
        return 2 * ((dim + 127) // 128), 6
    return (dim + 63) // 64, 6


def ln_offset_extra(v, gamma, eps, p, tree):
    """the extra term of a large-offset row: (p + tree) 2^-24 mean|v| rstd max|gamma|, the forward-error bound of the kernel's summation
    tree for the mean (p + tree additions deep, each 2^-24 relative to a partial sum of at most sum|v|), carried through
    (v - mean) rstd gamma"""
    v = v.double()
    d = v - v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return (p + tree) * 2.0 ** -24 * v.abs().mean(-1, keepdim=True) * rstd * float(gamma.abs().max())


# ----------------------------------------------------------------------------------------------------------------- fp32 restatements (CPU premise test)
def _lane_elements(form, dtype, dim):
    """per lane, the row elements it adds, in the kernel's order; `pairs` adds t.x + t.y first"""
    V = CHUNK[dtype]
    lanes = 16 if form == "q" else 64
    out = [[] for _ in range(lanes)]
    if form == "scalar":
        for c in range(dim):
            out[c % 64].append((c,))
    elif form == "pairs":
        for c in range(0, dim, 2):
            out[(c // 2) % 64].append((c, c + 1))
    else:
        for q in range(dim // V):
            out[q % lanes].extend((q * V + i,) for i in range(V))
    return out


def _tree_sum(part):
    """butterfly over the lanes (xor 32 ... 1, or the four rotations of a 16-lane row: the same pairs), fp32"""
    part = part.astype(np.float32)
    off = part.shape[-1] // 2
    while off >= 1:
        part = (part + part[..., np.arange(part.shape[-1]) ^ off]).astype(np.float32)
        off //= 2
    return part[..., 0]


def _lane_sum(vals, lanes_elems):
    rows = vals.shape[0]
    part = np.zeros((rows, len(lanes_elems)), np.float32)
    for l, items in enumerate(lanes_elems):
        s = np.zeros(rows, np.float32)
        for it in items:
            t = vals[:, it[0]]
            if len(it) == 2:
                t = (t + vals[:, it[1]]).astype(np.float32)
            s = (s + t).astype(np.float32)
        part[:, l] = s
    return _tree_sum(part)


def layer_norm_kernel_like_f32(v, gamma, beta, eps, form, dtype, one_pass=False):
    """fp32 restatement that sums like the kernels: lane-strided partial sums, then the lane tree.  `one_pass` is the DEFECT form
    var = E[v^2] - E[v]^2 with the same sums."""
    v32 = v.to(torch.float32).numpy()
    rows, dim = v32.shape
    le = _lane_elements(form, dtype, dim)
    f = np.float32
    mean = (_lane_sum(v32, le) / f(dim)).astype(f)
    d = (v32 - mean[:, None]).astype(f)
    if one_pass:
        var = (_lane_sum((v32 * v32).astype(f), le) / f(dim) - mean * mean).astype(f)
        var = np.maximum(var, f(0))
    else:
        var = (_lane_sum((d * d).astype(f), le) / f(dim)).astype(f)
    rstd = (f(1) / np.sqrt((var + f(eps)).astype(f))).astype(f)
    out = ((d * rstd[:, None]).astype(f) * gamma.to(torch.float32).numpy()).astype(f) + beta.to(torch.float32).numpy()
    return torch.from_numpy(out.astype(f))


# ----------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _q(t, dtype):
    """values of the case's dtype (what the device holds)"""
    return t.to(TORCH_DTYPE[dtype])


def ln_special_rows(dtype, dim, seed=21):
    """[E_MAX, dim] rows and their kinds.  big: offset + N(0, 1), offset 100 (fp32) / 16 (fp16); bigconst: offset + 0.75 everywhere;
    eps: 0.02 N(0, 1) (variance 4e-4: comparable to eps); off4: 4 + N(0, 1); const: 0.375 everywhere; rand: N(0, 1).  The first
    five rows hold one of each special kind, so that the smallest row counts see them."""
    g = _gen(seed + dim)
    off = LN_BIG_OFFSET[dtype]
    kinds = ["big", "bigconst", "eps", "off4", "const"] + [("big", "off4", "eps", "rand")[i % 4] for i in range(E_MAX - 5)]
    n = torch.randn(E_MAX, dim, generator=g)
    x = torch.empty(E_MAX, dim)
    for i, k in enumerate(kinds):
        x[i] = {"big": off + n[i], "bigconst": torch.full((dim,), off + 0.75), "eps": 0.02 * n[i], "off4": 4.0 + n[i],
                "const": torch.full((dim,), 0.375), "rand": n[i]}[k]
    return _q(x, dtype), kinds


GATE_SAT = {F32: (30.0, -30.0, 100.0, -100.0), F16: (30.0, -30.0, 60000.0, -60000.0)}
GATE_SAT_ROWS = (1, 2, 3, 4)


def gate_with_saturation(gate, dtype):
    """rows 1..4 of `gate` (first dim columns passed in) take the pattern +30, -30, +big, -big along the columns, rotated by the row:
    returns (gate, kind) with kind 0 elsewhere and 1..4 at +30, -30, +big, -big"""
    rows, dim = gate.shape
    kind = torch.zeros(rows, dim, dtype=torch.int64)
    sat = torch.tensor(GATE_SAT[dtype], dtype=gate.dtype)
    for r in GATE_SAT_ROWS:
        if r < rows:
            k = (torch.arange(dim) + r) % 4
            gate[r] = sat[k]
            kind[r] = k + 1
    return gate, kind


def group_tables(key):
    """perm (stable: rows of a group in ascending order), seg_start [n + 1], n_seg [1] (all int32) and the inverse map"""
    _, inv = torch.unique(key, return_inverse=True)
    perm = torch.sort(inv, stable=True).indices
    cnt = torch.bincount(inv)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cnt, 0)])
    return perm.to(torch.int32), seg.to(torch.int32), torch.tensor([cnt.numel()], dtype=torch.int32), inv


def softagg_groups(seed=31):
    """sparse keys (group i has key 977 i + 5, GROUP_SIZES[i] rows), the edge list shuffled"""
    g = _gen(seed)
    key = torch.cat([torch.full((n,), 977 * i + 5, dtype=torch.int64) for i, n in enumerate(GROUP_SIZES)])
    return key[torch.randperm(key.numel(), generator=g)]


def softagg_dominating_rank(n, dim):
    """per channel, the rank (position in perm order) of a group's dominating row in a group of n rows: first, last, the middle of the
    second batch of 8 rows (12) and of 16 rows (24), clipped to the group"""
    c = torch.arange(dim) % 4
    r = torch.where(c == 0, 0, torch.where(c == 1, n - 1, torch.where(c == 2, 12, 24)))
    return r.clamp(max=n - 1)


def softagg_inputs(dtype, dim, which, seed=33):
    """f, g [E, dim] of the case's dtype, key, and for `dominated` the index [n_seg, dim] of each channel's dominating row"""
    key = softagg_groups()
    E = key.numel()
    g_ = _gen(seed + dim + SOFTAGG_SETS.index(which))
    f = 2.0 * torch.randn(E, dim, generator=g_)
    dom = None
    if which == "plain":
        g = 2.0 * torch.randn(E, dim, generator=g_)
    elif which == "shifted":
        g = 1000.0 + torch.randn(E, dim, generator=g_)
    elif which == "equal":
        g = torch.full((E, dim), 0.5)
    else:
        g = 8.0 * torch.rand(E, dim, generator=g_)
        perm, seg, _, _ = group_tables(key)
        dom = torch.empty(len(GROUP_SIZES), dim, dtype=torch.int64)
        for s in range(len(GROUP_SIZES)):
            rows = perm[int(seg[s]):int(seg[s + 1])].long()
            dom[s] = rows[softagg_dominating_rank(rows.numel(), dim)]
            g[dom[s], torch.arange(dim)] = DOMINATING
    return _q(f, dtype), _q(g, dtype), key, dom


# ----------------------------------------------------------------------------------------------------------------- the case table
# Per case: the op, dtype, dim, the rows of its launch in the dispatch test, operand offsets (elements into the allocation), strides, the
# SoftAgg hint, and the kernel the launcher in update.hip picks for it today: base name and, for k_layernorm / k_softagg_v, the template
# argument that tells the forms apart.
def _case(op, dtype, dim, kernel, targ=None, **kw):
    c = dict(op=op, dtype=dtype, dim=dim, rows=E_MAX, kernel=kernel, targ=targ, off={}, ld_gate=None, terms=(), relu=0, eps=1e-3,
             rowset="rand", hint=0, ld_fg="2dim", ld_d="dim", group_of=True, gate=False)
    c.update(kw)
    return c


ALL_TERMS = ("a", "b", "hy", "gate")
LN_OPERANDS = ("x", "a", "b", "hy", "gate", "res", "gamma", "beta", "out")

# layer norm widths: (dtype, dim, kernel, template argument)
LN_WIDTHS = [
    (F32, 384, "k_layernorm_q", None),
    (F32, 4, "k_layernorm_v", None), (F32, 128, "k_layernorm_v", None), (F32, 256, "k_layernorm_v", None),
    (F32, 260, "k_layernorm_v", None), (F32, 512, "k_layernorm_v", None),                    # second chunk: one lane, all lanes
    (F32, 516, "k_layernorm", "true"), (F32, 1024, "k_layernorm", "true"), (F32, 2, "k_layernorm", "true"), (F32, 6, "k_layernorm", "true"),
    (F32, 1, "k_layernorm", "false"), (F32, 7, "k_layernorm", "false"), (F32, 1023, "k_layernorm", "false"),
    (F16, 384, "k_layernorm_q", None),
    (F16, 8, "k_layernorm_v", None), (F16, 128, "k_layernorm_v", None), (F16, 512, "k_layernorm_v", None),
    (F16, 520, "k_layernorm_v", None), (F16, 1024, "k_layernorm_v", None),
    (F16, 6, "k_layernorm", "true"), (F16, 7, "k_layernorm", "false"),
]
# the element-wise ops (masked gather, expand-add, gated residual and its adjoint): a 16-byte form and a scalar form
EW_WIDTHS = [(F32, d, True) for d in (384, 4, 128, 256, 260, 512, 516, 1024)] + [(F32, d, False) for d in (2, 6, 1, 7, 1023)] + \
            [(F16, d, True) for d in (384, 8, 128, 512, 520, 1024)] + [(F16, d, False) for d in (6, 7)]
# heads: the 16-byte form covers a row with one chunk per lane (64 chunks)
HEADS_WIDTHS = [(F32, 384, "k_heads_q")] + [(F32, d, "k_heads_v") for d in (4, 128, 256)] + \
               [(F32, d, "k_heads") for d in (260, 512, 516, 1024, 2, 6, 1, 7, 1023)] + \
               [(F16, 384, "k_heads_q")] + [(F16, d, "k_heads_v") for d in (8, 128, 512)] + [(F16, d, "k_heads") for d in (520, 1024, 6, 7)]


def _pair_step(dtype):
    return 2 if dtype == F32 else 4                          # elements of 8 bytes


def _build_cases():
    cs = []
    # ---- layer norm
    for dt, dim, k, ta in LN_WIDTHS:
        cs.append(_case("layernorm", dt, dim, k, ta, terms=ALL_TERMS, ld_gate=dim))
        cs.append(_case("layernorm", dt, dim, k, ta, rowset="special", relu=0))
    for dt in (F32, F16):
        ps = _pair_step(dt)
        every = {n: 1 for n in LN_OPERANDS}
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "false", terms=ALL_TERMS, ld_gate=384, off=every, relu=1))
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "true", terms=ALL_TERMS, ld_gate=384, off={n: ps for n in LN_OPERANDS}, eps=3e-2))
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "false", terms=ALL_TERMS, ld_gate=384, off={"out": 1}))
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "false", terms=ALL_TERMS, ld_gate=384, off={"gamma": 1}, relu=1, eps=3e-2))
        cs.append(_case("layernorm", dt, 384, "k_layernorm_q", None, terms=("gate",), ld_gate=768))
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "true", terms=("gate",), ld_gate=384 + ps, relu=1))
        cs.append(_case("layernorm", dt, 384, "k_layernorm", "false", terms=("gate",), ld_gate=385, eps=3e-2))
    sweep = [(F32, 384, "k_layernorm_q", None), (F16, 384, "k_layernorm_q", None), (F32, 512, "k_layernorm_v", None),
             (F16, 1024, "k_layernorm_v", None), (F32, 6, "k_layernorm", "true"), (F16, 6, "k_layernorm", "true"),
             (F32, 7, "k_layernorm", "false"), (F16, 7, "k_layernorm", "false")]
    for dt, dim, k, ta in sweep:
        for i, terms in enumerate((("a",), ("a", "b"), ("hy",), ("gate",))):
            cs.append(_case("layernorm", dt, dim, k, ta, terms=terms, ld_gate=dim if "gate" in terms else None, relu=i % 2, eps=(1e-3, 3e-2)[(i // 2) % 2]))
    # ---- masked gather, expand-add
    for op, base in (("masked_gather", "k_masked_gather"), ("expand_add", "k_expand_add")):
        for dt, dim, vec in EW_WIDTHS:
            cs.append(_case(op, dt, dim, base + ("_v" if vec else "")))
        for dt in (F32, F16):
            cs.append(_case(op, dt, 384, base, off={"all": 1}))
    # ---- gated residual and its adjoint
    for op, base in (("gated_residual", "k_gated_residual"), ("gated_residual_bwd", "k_gated_residual_bwd")):
        for dt, dim, vec in EW_WIDTHS:
            cs.append(_case(op, dt, dim, base + ("_v" if vec else ""), ld_gate=dim))
        for dt in (F32, F16):
            cs.append(_case(op, dt, 384, base, ld_gate=384, off={"all": 1}))
            cs.append(_case(op, dt, 384, base + "_v", ld_gate=768))
            cs.append(_case(op, dt, 384, base, ld_gate=384 + _pair_step(dt)))              # no 8-byte form of these ops: scalars
            cs.append(_case(op, dt, 384, base, ld_gate=385))
    # ---- heads
    for dt, dim, k in HEADS_WIDTHS:
        cs.append(_case("heads", dt, dim, k))
        cs.append(_case("heads", dt, dim, k, gate=True, ld_gate=dim))
    for dt in (F32, F16):
        cs.append(_case("heads", dt, 384, "k_heads", off={"all": 1}))
        cs.append(_case("heads", dt, 384, "k_heads", gate=True, ld_gate=384, off={"all": 1}))
        cs.append(_case("heads", dt, 384, "k_heads_q", gate=True, ld_gate=768))
        cs.append(_case("heads", dt, 384, "k_heads", gate=True, ld_gate=384 + _pair_step(dt)))
        cs.append(_case("heads", dt, 384, "k_heads", gate=True, ld_gate=385))
    # ---- SoftAgg forward: hints 0 / 41 / 47 -> four waves per group, 1 / 20 / 40 -> one wave per group, 48 / 1000 -> sixteen waves
    E = sum(GROUP_SIZES)
    for dt, dim in ((F32, 384), (F32, 512), (F32, 128), (F32, 4), (F16, 384), (F16, 1024), (F16, 8)):
        wide = dt == F16 and dim == 1024                       # 128 chunks: no one-wave form; 48 dim floats beyond the LDS cap: no 16-wave form
        for hint in (0, 41, 47):
            cs.append(_case("softagg", dt, dim, "k_softagg_v", "4", rows=E, hint=hint, group_of=hint != 41))
        for hint in (1, 20, 40):
            cs.append(_case("softagg", dt, dim, "k_softagg_v" if wide else "k_softagg_w", "4" if wide else None, rows=E, hint=hint, group_of=hint != 20))
        for hint in (48, 1000):
            cs.append(_case("softagg", dt, dim, "k_softagg_v", "4" if wide else "16", rows=E, hint=hint, group_of=hint != 48))
    for dt in (F32, F16):
        for hint, k, ta in ((0, "k_softagg_v", "4"), (20, "k_softagg_w", None), (48, "k_softagg_v", "16")):
            cs.append(_case("softagg", dt, 384, k, ta, rows=E, hint=hint, ld_fg="dim"))
        for hint in (0, 20):
            cs.append(_case("softagg", dt, 384, "k_softagg", None, rows=E, hint=hint, ld_fg="dim+2", group_of=hint == 0))
        ps = _pair_step(dt)                                   # 8-byte aligned operands (4-byte ones are refused): no 16-byte form, whatever the hint
        cs.append(_case("softagg", dt, 384, "k_softagg", None, rows=E, hint=0, ld_fg="dim", off={"f": ps, "g": ps}))
        cs.append(_case("softagg", dt, 384, "k_softagg", None, rows=E, hint=48, ld_fg="dim", off={"g": ps}))
        cs.append(_case("softagg", dt, 384, "k_softagg", None, rows=E, hint=20, ld_fg="2dim", off={"y": ps}))      # (k_softagg_w stores y in 16-byte chunks)
    cs.append(_case("softagg", F16, 848,"k_softagg_v", "16", rows=E, hint=48))              # 48 dim floats just below the LDS cap (dim <= 853)
    cs.append(_case("softagg", F16, 856, "k_softagg_v", "4", rows=E, hint=48))               # ... and just above it
    for dt, dim, ld in ((F32, 6, "2dim"), (F32, 516, "2dim"), (F32, 6, "dim"), (F16, 6, "dim"), (F16, 1030, "dim")):
        cs.append(_case("softagg", dt, dim, "k_softagg", None, rows=E, hint=0, ld_fg=ld))
        cs.append(_case("softagg", dt, dim, "k_softagg", None, rows=E, hint=20, ld_fg=ld, group_of=False))
    # ---- SoftAgg adjoint
    for dt in (F32, F16):
        for dim in (384, 6, 516):
            for ld_d in ("2dim", "dim"):
                cs.append(_case("softagg_bwd", dt, dim, "k_softagg_bwd", None, rows=E, ld_fg="dim" if (dt == F16 and dim == 6) else "2dim", ld_d=ld_d))
    for i, c in enumerate(cs):
        extra = "".join(f"-{k}{v}" for k, v in (("ldg", c["ld_gate"]), ("h", c["hint"] if c["op"] == "softagg" else None)) if v is not None)
        if c["op"].startswith("softagg"):
            extra += "-fg" + c["ld_fg"] + ("-d" + c["ld_d"] if c["op"] == "softagg_bwd" else "") + ("" if c["group_of"] else "-nogrp")
        if c["off"]:
            extra += "-off" + "".join(f"{k}{v}" for k, v in sorted(c["off"].items())) if len(c["off"]) < 3 else "-offevery%d" % next(iter(c["off"].values()))
        if c["op"] == "layernorm":
            extra += "-" + ("".join(t[0] for t in c["terms"]) or "x") + ("-special" if c["rowset"] == "special" else "")
        if c["gate"]:
            extra += "-gated"
        c["id"] = f"{i:03d}-{c['op']}-{c['dtype']}-{c['dim']}{extra}"
    return cs


CASES = _build_cases()

# every __global__ of update.hip behind the eleven entry points (written by hand): base name, distinguishing template argument
KERNELS = [
    ("k_layernorm", "false"), ("k_layernorm", "true"), ("k_layernorm_v", None), ("k_layernorm_q", None),
    ("k_heads", None), ("k_heads_v", None), ("k_heads_q", None),
    ("k_softagg", None), ("k_softagg_v", "4"), ("k_softagg_v", "16"), ("k_softagg_w", None), ("k_softagg_bwd", None),
    ("k_masked_gather", None), ("k_masked_gather_v", None), ("k_expand_add", None), ("k_expand_add_v", None),
    ("k_gated_residual", None), ("k_gated_residual_v", None), ("k_gated_residual_bwd", None), ("k_gated_residual_bwd_v", None),
]
