"""The row kernels of devo_amd/csrc/update.hip, every dispatch variant on its own against the fp64 references of tests/update_ops_ref.py.

Through the C ABI (L.lib(), L.ptr), so that alignment and strides are the test's to choose.  Every case of update_ops_ref.CASES names the
kernel the launcher picks for it; test_every_case_reaches_the_kernel_it_names checks that with the profiler, so a case that passes here
has compared THAT kernel with the reference.  Row-wise cases run at every row count of ROW_COUNTS (around the 4-row and 16-row
workgroups), into buffers with two poison rows behind the last one and NaN in the gaps of strided operands.

Bounds (update_ops_ref.bound): per row against fp64, 1e-5 max(1, max|ref row|) for fp32 storage, one fp16 rounding more for fp16.
Exactness where fp32 arithmetic gives it: a gate at +30 / +100 / +60000 is a sigmoid of exactly 1, at -100 / -60000 exactly 0.  At -30
the fp32 sigmoid is 9.4e-14, a normal fp32 number, not 0: there fp32 storage is held to the bound and to |dgate| <= 2^-43 |dout res|,
fp16 storage (which cannot hold 1e-13) to exactly 0.

Set DEVO_UPDATE_OPS_RECORD to a path to have the last test write the worst error / bound ratio per (op, kernel, dtype) there
(profiles/update_ops.txt is such a record).
"""
import functools
import os
import re
import pytest
import torch
import update_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
RATIOS = {}


def _L():
    from devo_amd import _lib as L
    return L


def _label(c):
    return c["kernel"] + (f"<{c['targ']}>" if c["targ"] else "")


def _note(c, ratio):
    key = (c["op"], _label(c), c["dtype"])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


def _check(c, got, ref, what, extra=None):
    r = R.err_ratio(got, ref, c["dtype"], extra)
    _note(c, r)
    assert r <= 1.0, f"{c['id']} {what}: error / bound = {r:.3f}"


def _gen(c, salt=0):
    return torch.Generator().manual_seed(1000 + 2 * c["dim"] + (c["dtype"] == R.F16) + 7919 * salt)


def _randn(g, dtype, *shape):
    return torch.randn(*shape, generator=g).to(R.TORCH_DTYPE[dtype])


def _off(c, name):
    return c["off"].get(name, c["off"].get("all", 0))


class Buf:
    """A [rows, cols] device view that starts `off` elements into its allocation, row stride ld; `tail` rows behind it hold POISON, the
    gap columns, the elements in front and a few behind hold NaN.  read(E) returns rows [0, E) and checks that the rest kept its bits."""

    def __init__(self, data, off=0, ld=None, tail=0):
        if data.dim() == 1:
            data = data[None]
        self.rows = data.shape[0] + tail
        self.cols = data.shape[1]
        self.ld = ld or self.cols
        self.off = off
        flat = torch.full((off + self.rows * self.ld + 8,), NAN, dtype=data.dtype)
        v = flat[off:off + self.rows * self.ld].view(self.rows, self.ld)
        v[:, :self.cols] = R.POISON
        v[:data.shape[0], :self.cols] = data
        self.flat = flat.to(DEV)
        self.v = self.flat[off:off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]
        assert self.v.data_ptr() == self.flat.data_ptr() + off * flat.element_size()

    def ptr(self):
        return _L().ptr(self.v)

    def read(self, E, what=""):
        flat = self.flat.cpu()
        full = flat[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)
        assert bool((full[E:, :self.cols] == R.POISON).all()), f"{what}: rows behind the last one were written"
        assert bool(torch.isnan(full[:, self.cols:]).all()) and bool(torch.isnan(flat[:self.off]).all()) and \
            bool(torch.isnan(flat[self.off + self.rows * self.ld:]).all()), f"{what}: written outside the rows"
        return full[:E, :self.cols].clone()


def _out(c, E, cols, name="out", ld=None, init=None):
    data = torch.full((E, cols), R.POISON, dtype=R.TORCH_DTYPE[c["dtype"]]) if init is None else init
    return Buf(data, _off(c, name), ld, tail=R.POISON_ROWS)


def _code(c):
    return 0 if c["dtype"] == R.F32 else _L().dtype_code(torch.empty(0, dtype=torch.float16))


def _p(b):
    return None if b is None else (b.ptr() if isinstance(b, Buf) else _L().ptr(b))


def _gate_buf(c, gate, name="gate"):
    return Buf(gate, _off(c, name), c["ld_gate"])


# ----------------------------------------------------------------------------------------------------------------- layer norm
class LayerNorm:
    def __init__(self, c):
        self.c = c
        dt, dim, g = c["dtype"], c["dim"], _gen(c)
        self.kinds = None
        if c["rowset"] == "special":
            self.x, self.kinds = R.ln_special_rows(dt, dim)
        else:
            self.x = _randn(g, dt, R.E_MAX, dim)
        t = c["terms"]
        self.a = _randn(g, dt, R.E_MAX, dim) if "a" in t else None
        self.b = _randn(g, dt, R.E_MAX, dim) if "b" in t else None
        self.hy = _randn(g, dt, 9, dim) if "hy" in t else None
        self.grp = torch.randint(0, 8, (R.E_MAX,), generator=g).to(torch.int32) if "hy" in t else None      # group 8: no row names it
        self.gate = _randn(g, dt, R.E_MAX, dim) if "gate" in t else None
        self.res = _randn(g, dt, R.E_MAX, dim) if "gate" in t else None
        self.gamma, self.beta = _randn(g, dt, dim), _randn(g, dt, dim)
        o = lambda n: _off(c, n)
        mk = lambda v, n: None if v is None else Buf(v, o(n))
        self.d = dict(x=mk(self.x, "x"), a=mk(self.a, "a"), b=mk(self.b, "b"), hy=mk(self.hy, "hy"), res=mk(self.res, "res"),
                      gamma=mk(self.gamma, "gamma"), beta=mk(self.beta, "beta"))
        self.d["gate"] = None if self.gate is None else _gate_buf(c, self.gate)
        self.d["grp"] = None if self.grp is None else self.grp.to(DEV)

    def launch(self, E, relu=None, eps=None, **over):
        c, L, d = self.c, _L(), dict(self.d, **over)
        out = _out(c, E, c["dim"])
        rc = L.lib().devo_upd_layernorm(_p(d["x"]), _p(d["a"]), _p(d["b"]), _p(d["hy"]), _p(d["grp"]), _p(d["gate"]), over.get("ld_gate", c["ld_gate"] or 0),
                                        _p(d["res"]), _p(d["gamma"]), _p(d["beta"]), out.ptr(), E, over.get("dim", c["dim"]),
                                        c["eps"] if eps is None else eps, c["relu"] if relu is None else relu, _code(c), L.stream())
        return rc, out

    def verify(self, E, out, relu=None, eps=None):
        c = self.c
        relu, eps = c["relu"] if relu is None else relu, c["eps"] if eps is None else eps
        w = lambda v: None if v is None else v.double()
        cut = lambda v: None if v is None else v.double()[:E]
        ref, v = R.layer_norm_ref(cut(self.x), cut(self.a), cut(self.b), w(self.hy), None if self.grp is None else self.grp[:E], cut(self.gate),
                                  cut(self.res), w(self.gamma), w(self.beta), eps, relu)
        extra = None
        if self.kinds is not None:
            p, tree = R.ln_elems_per_lane(c["kernel"], c["targ"], c["dtype"], c["dim"])
            big = torch.tensor([k in ("big", "bigconst") for k in self.kinds[:E]], dtype=torch.float64)[:, None]
            extra = R.ln_offset_extra(v, self.gamma.double(), eps, p, tree) * big
        _check(c, out.read(E, c["id"]), ref, f"rows {E} relu {relu} eps {eps}", extra)


# ----------------------------------------------------------------------------------------------------------------- masked gather, expand-add
def _index_sets(g, gather):
    n = R.E_MAX
    rnd = torch.randint(0, n, (n,), generator=g)
    rnd[rnd == 5] = 6                                         # row / group 5: nobody names it
    sets = {"random": rnd.clone(), "identity": torch.arange(n), "one": torch.full((n,), 7)}
    if gather:
        sets["random"][torch.rand(n, generator=g) < 0.3] = -1
        sets["none"] = torch.full((n,), -1)
    return sets


class MaskedGather:
    def __init__(self, c):
        self.c = c
        g = _gen(c)
        self.src = _randn(g, c["dtype"], R.E_MAX, c["dim"])
        self.sets = _index_sets(g, True)
        self.d_src = Buf(self.src, _off(c, "src"))
        self.d_sets = {k: v.to(DEV) for k, v in self.sets.items()}

    def launch(self, E, which="random"):
        c, L = self.c, _L()
        out = _out(c, E, c["dim"])
        rc = L.lib().devo_upd_masked_gather(self.d_src.ptr(), L.ptr(self.d_sets[which]), out.ptr(), E, c["dim"], _code(c), L.stream())
        return rc, out

    def verify(self, E, out, which="random"):
        got, ref = out.read(E, self.c["id"]), R.masked_gather_ref(self.src, self.sets[which][:E])
        it = torch.int32 if self.c["dtype"] == R.F32 else torch.int16
        _note(self.c, 0.0 if torch.equal(got.view(it), ref.view(it)) else float("inf"))
        assert torch.equal(got.view(it), ref.view(it)), f"{self.c['id']} rows {E} index set {which}: not a copy"


class ExpandAdd:
    def __init__(self, c):
        self.c = c
        g = _gen(c)
        self.net, self.hy = _randn(g, c["dtype"], R.E_MAX, c["dim"]), _randn(g, c["dtype"], R.E_MAX, c["dim"])
        self.sets = {k: v.to(torch.int32) for k, v in _index_sets(g, False).items()}
        self.d_hy = Buf(self.hy, _off(c, "hy"))
        self.d_sets = {k: v.to(DEV) for k, v in self.sets.items()}

    def launch(self, E, which="random"):
        c, L = self.c, _L()
        net = _out(c, E, c["dim"], "net", init=self.net[:E])
        rc = L.lib().devo_upd_expand_add(net.ptr(), self.d_hy.ptr(), L.ptr(self.d_sets[which]), E, c["dim"], _code(c), L.stream())
        return rc, net

    def verify(self, E, net, which="random"):
        got, ref = net.read(E, self.c["id"]), R.expand_add_ref(self.net[:E], self.hy, self.sets[which][:E])
        assert ref.dtype == got.dtype
        _note(self.c, 0.0 if torch.equal(got, ref) else float("inf"))
        assert torch.equal(got, ref), f"{self.c['id']} rows {E} group set {which}: not torch's sum in the same dtype"


# ----------------------------------------------------------------------------------------------------------------- gated residual and its adjoint
class Gated:
    def __init__(self, c):
        self.c = c
        dt, dim, g = c["dtype"], c["dim"], _gen(c)
        self.x, self.res, self.dout = (_randn(g, dt, R.E_MAX, dim) for _ in range(3))
        self.gate, self.kind = R.gate_with_saturation(_randn(g, dt, R.E_MAX, dim), dt)
        self.d_x, self.d_res, self.d_dout = Buf(self.x, _off(c, "x")), Buf(self.res, _off(c, "res")), Buf(self.dout, _off(c, "dout"))
        self.d_gate = _gate_buf(c, self.gate)
        self.bwd = c["op"] == "gated_residual_bwd"

    def launch(self, E):
        c, L = self.c, _L()
        if self.bwd:
            dgate, dres = _out(c, E, c["dim"], "dgate"), _out(c, E, c["dim"], "dres")
            rc = L.lib().devo_upd_gated_residual_backward(self.d_gate.ptr(), c["ld_gate"], self.d_res.ptr(), self.d_dout.ptr(), dgate.ptr(), dres.ptr(),
                                                          E, c["dim"], _code(c), L.stream())
            return rc, (dgate, dres)
        out = _out(c, E, c["dim"])
        rc = L.lib().devo_upd_gated_residual(self.d_x.ptr(), self.d_gate.ptr(), c["ld_gate"], self.d_res.ptr(), out.ptr(), E, c["dim"], _code(c), L.stream())
        return rc, out

    def verify(self, E, outs):
        c, k, td = self.c, self.kind[:E], R.TORCH_DTYPE[self.c["dtype"]]
        one, zero, m30 = (k == 1) | (k == 3), k == 4, k == 2
        x, gate, res, dout = self.x[:E], self.gate[:E], self.res[:E], self.dout[:E]
        if not self.bwd:
            got = outs.read(E, c["id"])
            _check(c, got, R.gated_residual_ref(x.double(), gate.double(), res.double()), f"rows {E}")
            assert torch.equal(got[one], (x.float() + res.float()).to(td)[one]), f"{c['id']}: sigmoid(+30 / +big) is not exactly 1"
            assert torch.equal(got[zero], x[zero]), f"{c['id']}: sigmoid(-big) is not exactly 0"
            if c["dtype"] == R.F16:
                assert torch.equal(got[m30], x[m30])
            return
        dgate, dres = (o.read(E, c["id"]) for o in outs)
        rg, rr = R.gated_residual_bwd_ref(gate.double(), res.double(), dout.double())
        _check(c, dgate, rg, f"dgate rows {E}")
        _check(c, dres, rr, f"dres rows {E}")
        sat = one | zero
        assert bool((dgate[sat] == 0).all()), f"{c['id']}: dgate at a saturated gate is not exactly 0"
        assert torch.equal(dres[one], dout[one]) and bool((dres[zero] == 0).all()), f"{c['id']}: dres at a saturated gate"
        if c["dtype"] == R.F16:
            assert bool((dgate[m30] == 0).all()) and bool((dres[m30] == 0).all())
        else:
            assert bool((dgate[m30].double().abs() <= 2.0 ** -43 * (dout[m30].double() * res[m30].double()).abs() * (1 + 1e-6)).all())


# ----------------------------------------------------------------------------------------------------------------- heads
NEG_ROWS = (2, 6)


class Heads:
    def __init__(self, c):
        self.c = c
        dt, dim, g = c["dtype"], c["dim"], _gen(c)
        x = torch.randn(R.E_MAX, dim, generator=g)
        for r in NEG_ROWS:
            x[r] = -50.0 - x[r].abs()                          # all negative, with or without the gated term (|res| stays far below 50)
        self.x = x.to(R.TORCH_DTYPE[dt])
        s = dim ** -0.5
        self.Wd = (torch.randn(2, dim, generator=g) * torch.tensor([[1.0], [4.0]]) * s).to(self.x.dtype)      # rows of different scales: swapped rows show
        self.Ww = (torch.randn(2, dim, generator=g) * torch.tensor([[2.0], [0.5]]) * s).to(self.x.dtype)
        self.bd, self.bw = _randn(g, dt, 2), _randn(g, dt, 2)
        self.d_x, self.d_Wd, self.d_Ww = Buf(self.x, _off(c, "x")), Buf(self.Wd, _off(c, "Wd")), Buf(self.Ww, _off(c, "Ww"))
        self.d_bd, self.d_bw = self.bd.to(DEV), self.bw.to(DEV)
        self.gate = self.res = self.d_gate = self.d_res = None
        if c["gate"]:
            self.res = _randn(g, dt, R.E_MAX, dim)
            self.gate, _ = R.gate_with_saturation(_randn(g, dt, R.E_MAX, dim), dt)
            self.d_gate, self.d_res = _gate_buf(c, self.gate), Buf(self.res, _off(c, "res"))

    def launch(self, E):
        c, L = self.c, _L()
        net_out = _out(c, E, c["dim"], "net_out") if c["gate"] else None
        delta, weight = _out(c, E, 2, "delta"), _out(c, E, 2, "weight")
        rc = L.lib().devo_upd_heads(self.d_x.ptr(), _p(self.d_gate), c["ld_gate"] or 0, _p(self.d_res), _p(net_out), self.d_Wd.ptr(), L.ptr(self.d_bd),
                                    self.d_Ww.ptr(), L.ptr(self.d_bw), delta.ptr(), weight.ptr(), E, c["dim"], _code(c), L.stream())
        return rc, (net_out, delta, weight)

    def verify(self, E, outs):
        c = self.c
        net_out, delta, weight = outs
        delta, weight = delta.read(E, c["id"]), weight.read(E, c["id"])
        net = self.x[:E].double()
        if c["gate"]:
            got_net = net_out.read(E, c["id"])
            _check(c, got_net, R.gated_residual_ref(net, self.gate[:E].double(), self.res[:E].double()), f"net_out rows {E}")
            net = got_net.double()                              # the heads read the stored value
        rd, rw = R.heads_ref(net, self.Wd.double(), self.bd.double(), self.Ww.double(), self.bw.double())
        _check(c, delta, rd, f"delta rows {E}")
        _check(c, weight, rw, f"weight rows {E}")
        for r in NEG_ROWS:
            if r < E:
                assert bool((net[r] < 0).all())
                assert torch.equal(delta[r], self.bd), f"{c['id']}: delta of an all-negative row is not bd"
                # sigmoid(bw) up to the roundings of its own evaluation (an exponential, a sum and a quotient in fp32: 2^-22 of a value
                # below 1) and of the store; nothing of the row may enter
                tol = 2.0 ** -22 + (2.0 ** -11 if c["dtype"] == R.F16 else 0.0)
                assert float((weight[r].double() - torch.sigmoid(self.bw.double())).abs().max()) <= tol, f"{c['id']}: weight of an all-negative row"


# ----------------------------------------------------------------------------------------------------------------- SoftAgg
@functools.lru_cache(maxsize=None)
def _softagg_set(dtype, dim, which):
    f, g, key, dom = R.softagg_inputs(dtype, dim, which)
    perm, seg, n_seg, inv = R.group_tables(key)
    return dict(f=f, g=g, dom=dom, perm=perm, seg=seg, n_seg=n_seg, inv=inv, ref=R.softagg_ref(f.double(), g.double(), inv))


@functools.lru_cache(maxsize=None)
def _softagg_bwd_set(dtype, dim):
    s = _softagg_set(dtype, dim, "plain")
    dy = _randn(torch.Generator().manual_seed(77 + dim), dtype, int(s["n_seg"]), dim)
    df, dg = R.softagg_bwd_ref(s["f"].double(), s["g"].double(), s["inv"], dy.double())
    return dict(s, dy=dy, df=df, dg=dg)


class SoftAgg:
    def __init__(self, c):
        self.c = c
        self.dev = {}
        self.bwd = c["op"] == "softagg_bwd"
        s = _softagg_set(c["dtype"], c["dim"], "plain")
        self.E, self.n = s["f"].shape[0], int(s["n_seg"])
        assert self.E == c["rows"]
        self.tables = tuple(s[k].to(DEV) for k in ("perm", "seg", "n_seg"))
        self.inputs("plain")
        if self.bwd:
            self.d_dy = Buf(_softagg_bwd_set(c["dtype"], c["dim"])["dy"], _off(c, "dy"))

    def inputs(self, which):
        """f and g on the device: the two halves of one [E, 2 dim] buffer (`2dim`), or two tensors of row stride dim / dim + 2"""
        if which not in self.dev:
            c, dim = self.c, self.c["dim"]
            s = _softagg_set(c["dtype"], dim, which)
            if c["ld_fg"] == "2dim":
                fg = Buf(torch.cat([s["f"], s["g"]], 1), _off(c, "f"))
                self.dev[which] = (fg, fg.v, fg.v[:, dim:], 2 * dim)
            else:
                ld = dim if c["ld_fg"] == "dim" else dim + 2
                f, g = Buf(s["f"], _off(c, "f"), ld), Buf(s["g"], _off(c, "g"), ld)
                self.dev[which] = ((f, g), f.v, g.v, ld)
        return self.dev[which]

    def launch(self, E=None, which="plain", hint=None):
        c, L = self.c, _L()
        _, f, g, ld = self.inputs(which)
        perm, seg, n_seg = self.tables
        if self.bwd:
            ld_d = c["dim"] * (2 if c["ld_d"] == "2dim" else 1)
            df, dg = _out(c, self.E, c["dim"], "df", ld=ld_d), _out(c, self.E, c["dim"], "dg", ld=ld_d)
            rc = L.lib().devo_upd_softagg_backward(L.ptr(f), L.ptr(g), ld, L.ptr(perm), L.ptr(seg), L.ptr(n_seg), self.d_dy.ptr(), df.ptr(), dg.ptr(), ld_d,
                                                   self.E, c["dim"], _code(c), L.stream())
            return rc, (df, dg)
        y = _out(c, self.n, c["dim"], "y")
        grp = torch.full((self.E,), -1, dtype=torch.int32, device=DEV) if c["group_of"] else None
        rc = L.lib().devo_upd_softagg_hint(L.ptr(f), L.ptr(g), ld, L.ptr(perm), L.ptr(seg), L.ptr(n_seg), y.ptr(), L.ptr(grp), self.E, c["dim"], _code(c),
                                           c["hint"] if hint is None else hint, L.stream())
        return rc, (y, grp)

    def verify(self, E, outs, which="plain"):
        c = self.c
        if self.bwd:
            s = _softagg_bwd_set(c["dtype"], c["dim"])
            _check(c, outs[0].read(self.E, c["id"]), s["df"], "df")
            _check(c, outs[1].read(self.E, c["id"]), s["dg"], "dg")
            return
        s = _softagg_set(c["dtype"], c["dim"], which)
        y, grp = outs
        y = y.read(self.n, c["id"])                             # (checks that the rows beyond n_seg kept their poison)
        _check(c, y, s["ref"], which)
        if grp is not None:
            assert torch.equal(grp.cpu().long(), s["inv"]), f"{c['id']}: group_of is not the inverse map"
        cnt = torch.bincount(s["inv"])
        for one in (cnt == 1).nonzero().flatten().tolist():     # a group of one row: y == f
            assert torch.equal(y[one], s["f"][s["inv"] == one][0]), f"{c['id']} {which}: a one-row group is not its row"
        if which == "dominated":                                # every other weight is exactly 0 in fp32
            assert torch.equal(y, s["f"][s["dom"], torch.arange(c["dim"])[None].expand_as(s["dom"])]), f"{c['id']}: dominated groups"


OPS = {"layernorm": LayerNorm, "masked_gather": MaskedGather, "expand_add": ExpandAdd, "gated_residual": Gated, "gated_residual_bwd": Gated,
       "heads": Heads, "softagg": SoftAgg, "softagg_bwd": SoftAgg}


def _cases(*ops):
    cs = [c for c in R.CASES if c["op"] in ops]
    return pytest.mark.parametrize("c", cs, ids=[c["id"] for c in cs])


def _run(p, E, **kw):
    rc, outs = p.launch(E, **kw)
    _L().check(rc, p.c["id"])
    return outs


# ----------------------------------------------------------------------------------------------------------------- the tests
@_cases("layernorm")
def test_layernorm(c):
    p = LayerNorm(c)
    for E in R.ROW_COUNTS:
        p.verify(E, _run(p, E))
    for relu in (0, 1):
        for eps in (1e-3, 3e-2):
            if (relu, eps) != (c["relu"], c["eps"]):
                p.verify(R.E_MAX, _run(p, R.E_MAX, relu=relu, eps=eps), relu=relu, eps=eps)


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_layernorm_refusals(dtype):
    """dim 1025, hy without group_of, gate without res, ld_gate < dim: an error, and `out` untouched"""
    c = next(c for c in R.CASES if c["op"] == "layernorm" and c["dtype"] == dtype and c["dim"] == 384 and c["terms"] == R.ALL_TERMS and not c["off"])
    p = LayerNorm(c)
    wide = dict(c, dim=1025, terms=(), ld_gate=None, id="dim1025")
    for what, q, over in (("dim 1025", LayerNorm(wide), {}), ("hy without group_of", p, dict(grp=None)), ("gate without res", p, dict(res=None)),
                          ("ld_gate < dim", p, dict(ld_gate=383))):
        rc, out = q.launch(17, **over)
        assert rc != 0, what
        with pytest.raises(RuntimeError):
            _L().check(rc, what)
        torch.cuda.synchronize()
        assert out.read(0, what).numel() == 0                   # all 17 + 2 rows still hold the poison


@_cases("masked_gather", "expand_add")
def test_gather_and_expand_add_are_bit_equal(c):
    p = OPS[c["op"]](c)
    for E in R.ROW_COUNTS:
        p.verify(E, _run(p, E))
    for which in p.sets:
        p.verify(R.E_MAX, _run(p, R.E_MAX, which=which), which=which)


@_cases("gated_residual", "gated_residual_bwd")
def test_gated_residual_and_adjoint(c):
    p = Gated(c)
    for E in R.ROW_COUNTS:
        p.verify(E, _run(p, E))


@_cases("heads")
def test_heads(c):
    p = Heads(c)
    for E in R.ROW_COUNTS:
        p.verify(E, _run(p, E))


@_cases("softagg")
def test_softagg_forward(c):
    p = SoftAgg(c)
    for which in R.SOFTAGG_SETS:
        p.verify(None, _run(p, None, which=which), which=which)


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_softagg_refusals(dtype):
    """odd dim, odd ld_fg, an operand that is only 4-byte aligned: an error, y untouched"""
    L = _L()
    td = R.TORCH_DTYPE[dtype]
    key = R.softagg_groups()
    perm, seg, n_seg, _ = (t.to(DEV) for t in R.group_tables(key))
    E, n = key.numel(), len(R.GROUP_SIZES)
    code = 0 if dtype == R.F32 else L.dtype_code(torch.empty(0, dtype=td))
    step = 4 // torch.empty(0, dtype=td).element_size()        # elements of 4 bytes
    for what, dim, ld, off in (("odd dim", 7, 8, 0), ("odd ld_fg", 6, 7, 0), ("4-byte aligned f", 6, 6, step)):
        f, g = Buf(torch.zeros(E, dim, dtype=td), off, ld), Buf(torch.zeros(E, dim, dtype=td), 0, ld)
        y = Buf(torch.full((n, dim), R.POISON, dtype=td), 0, tail=R.POISON_ROWS)
        rc = L.lib().devo_upd_softagg_hint(f.ptr(), g.ptr(), ld, L.ptr(perm), L.ptr(seg), L.ptr(n_seg), y.ptr(), None, E, dim, code, 0, L.stream())
        assert rc != 0, what
        with pytest.raises(RuntimeError):
            L.check(rc, what)
        torch.cuda.synchronize()
        assert y.read(0, what).numel() == 0
        # the adjoint states the same contract
        dy, df, dg = (Buf(torch.full((r, dim), R.POISON, dtype=td), 0, ld if r == E else None) for r in (n, E, E))
        rc = L.lib().devo_upd_softagg_backward(f.ptr(), g.ptr(), ld, L.ptr(perm), L.ptr(seg), L.ptr(n_seg), dy.ptr(), df.ptr(), dg.ptr(), ld, E, dim, code, L.stream())
        assert rc != 0, what + " (adjoint)"
        torch.cuda.synchronize()
        assert df.read(0, what).numel() == 0 and dg.read(0, what).numel() == 0


@_cases("softagg_bwd")
def test_softagg_adjoint(c):
    p = SoftAgg(c)
    p.verify(None, _run(p, None))


@pytest.mark.parametrize("dtype", [R.F32, R.F16])
def test_scalar_forms_beyond_one_grid(dtype):
    """The scalar element-wise forms launch at most 8192 workgroups of 256 threads and stride over the rest: 2100 rows of 1023 values are
    51 148 elements more than one sweep of the grid, the one size at which these four kernels take their loop's second trip.  (The 16-byte
    forms stride beyond 4 194 304 chunks, 64 MiB an operand: no call of the operator comes near, and no test here.)"""
    L = _L()
    rows, dim = 2100, 1023
    assert rows * dim > 8192 * 256
    td, code = R.TORCH_DTYPE[dtype], 0 if dtype == R.F32 else L.dtype_code(torch.empty(0, dtype=torch.float16))
    g = torch.Generator().manual_seed(91)
    x, gate, res, dout = (torch.randn(rows, dim, generator=g).to(td) for _ in range(4))
    idx = torch.randint(-1, rows, (rows,), generator=g)
    grp = torch.randint(0, rows, (rows,), generator=g).to(torch.int32)
    c = dict(op="beyond_one_grid", kernel="", targ=None, dtype=dtype, id="2100 x 1023", off={})
    d_x, d_gate, d_res, d_dout = (Buf(t) for t in (x, gate, res, dout))
    new = lambda init=None: _out(c, rows, dim, init=init)
    out = new()
    L.check(L.lib().devo_upd_masked_gather(d_x.ptr(), L.ptr(idx.to(DEV)), out.ptr(), rows, dim, code, L.stream()), "gather")
    assert torch.equal(out.read(rows), R.masked_gather_ref(x, idx))
    net = new(init=res)
    L.check(L.lib().devo_upd_expand_add(net.ptr(), d_x.ptr(), L.ptr(grp.to(DEV)), rows, dim, code, L.stream()), "expand")
    assert torch.equal(net.read(rows), R.expand_add_ref(res, x, grp))
    out = new()
    L.check(L.lib().devo_upd_gated_residual(d_x.ptr(), d_gate.ptr(), dim, d_res.ptr(), out.ptr(), rows, dim, code, L.stream()), "gated")
    c["kernel"] = "k_gated_residual"
    _check(c, out.read(rows), R.gated_residual_ref(x.double(), gate.double(), res.double()), "gated residual")
    dgate, dres = new(), new()
    L.check(L.lib().devo_upd_gated_residual_backward(d_gate.ptr(), dim, d_res.ptr(), d_dout.ptr(), dgate.ptr(), dres.ptr(), rows, dim, code, L.stream()), "gated bwd")
    rg, rr = R.gated_residual_bwd_ref(gate.double(), res.double(), dout.double())
    c["kernel"] = "k_gated_residual_bwd"
    _check(c, dgate.read(rows), rg, "dgate")
    _check(c, dres.read(rows), rr, "dres")


# ----------------------------------------------------------------------------------------------------------------- dispatch
NAMES = []
_NAME = re.compile(r"\b(k_[a-z0-9_]+)\b(?:<([^()]*)>)?")


def _parse(name):
    """(base, dtype or None, last template argument or None) of a device event's name, None if it is no kernel of update.hip"""
    m = _NAME.search(name)
    if not m or m.group(1) not in {k for k, _ in R.KERNELS}:
        return None
    targs = [t.strip() for t in m.group(2).split(",")] if m.group(2) else []
    dt = None if not targs else (R.F16 if "half" in targs[0] else R.F32 if "float" in targs[0] else None)
    last = targs[-1].replace("(bool)", "").replace("(int)", "") if len(targs) > 1 else None
    return m.group(1), dt, last


def test_every_case_reaches_the_kernel_it_names():
    """Every case of the table, launched once in table order inside one profiler session: the device events that carry a kernel name of
    update.hip, in start order, are the table's kernels.  The profiler's names are the demangled ones and carry the template arguments
    (`void devo::k_layernorm<float, true>(float const*, ...)`, `void devo::k_softagg_v<float, 4>(...)`: profiles/update_ops.txt keeps two
    of them), so the dtype, true / false of k_layernorm and 4 / 16 of k_softagg_v are checked too; a name without its arguments fails the
    test, so that the check cannot fall back to base names unnoticed.  Afterwards every __global__ behind the entry points
    (update_ops_ref.KERNELS, written by hand) has been seen in both dtypes."""
    from torch.profiler import profile, ProfilerActivity
    preps = [OPS[c["op"]](c) for c in R.CASES]                  # all inputs first
    for p in preps:
        _run(p, p.c["rows"])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for p in preps:
            _run(p, p.c["rows"])
        torch.cuda.synchronize()
    evs = [ev for ev in prof.events() if "cuda" in str(getattr(ev, "device_type", "")).lower()]
    evs.sort(key=lambda ev: ev.time_range.start)
    seen = [(ev.name, _parse(ev.name)) for ev in evs]
    seen = [(n, s) for n, s in seen if s is not None]
    assert len(seen) == len(R.CASES), f"{len(seen)} kernels of update.hip for {len(R.CASES)} cases; device events: {[ev.name for ev in evs[:8]]}"
    covered = set()
    for c, (name, (base, dt, last)) in zip(R.CASES, seen):
        assert base == c["kernel"], f"{c['id']}: expected {_label(c)}, ran {name}"
        if dt is not None:
            assert dt == c["dtype"], f"{c['id']}: expected {c['dtype']}, ran {name}"
        if c["targ"] is not None and last is not None:
            assert last == c["targ"], f"{c['id']}: expected {_label(c)}, ran {name}"
        covered.add((base, c["targ"], c["dtype"]))
    assert covered == {(k, t, dt) for k, t in R.KERNELS for dt in (R.F32, R.F16)}
    NAMES[:] = [seen[0][0], next(n for n, s in seen if s[0] == "k_softagg_v")]
    assert all(s[1] is not None for _, s in seen), "a device event name without its template arguments"      # (see the docstring)


def test_zz_record_of_error_over_bound():
    """prints (and, with DEVO_UPDATE_OPS_RECORD set, writes) the worst error / bound per (op, kernel, dtype) of the tests above"""
    lines = [f"{'op':<20}{'kernel':<28}{'dtype':<6}{'worst error / bound':>20}"]
    for (op, k, dt), r in sorted(RATIOS.items()):
        lines.append(f"{op:<20}{k:<28}{dt:<6}{r:>20.4f}")
    lines += [f"device event name in the dispatch test: {n}" for n in NAMES]
    text = "\n".join(lines) + "\n"
    print(text)
    path = os.environ.get("DEVO_UPDATE_OPS_RECORD")
    if path:
        with open(path, "w") as fh:
            fh.write(text)
    assert all(r <= 1.0 for r in RATIOS.values())
