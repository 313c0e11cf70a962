"""devo_amd.losses without a GPU: the new symbols are declared in all three places, the ABI version did not move, the fixture
tests/golden/train_loss_f64.npz (tools/gen_golden_loss.py: the reference's loss on CPU in fp64) agrees with an independent fp64
restatement composed from oracle/se3.py, and the module refuses what it cannot run."""
import os
import re
import numpy as np
import pytest
import torch

from oracle import se3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("devo_loss_state_bytes", "devo_loss_forward", "devo_loss_backward")
FIELDS = ("flow", "pose", "tr", "ro", "px1", "r1", "r2", "t1", "t2", "scores", "scale")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "train_loss_f64.npz"))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_are_declared_in_header_ctypes_table_and_binding():
    from devo_amd import _lib
    header, bind = _read("include", "devo_hip.h"), _read("devo_amd", "csrc", "bind.cpp")
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", header), s
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert re.search(r"\b" + s + r"\(", bind), s
    assert 'def_submodule("losses"' in bind
    assert 'm.def("loss_forward(' in bind and 'm.def("loss_backward(' in bind
    assert "loss.hip" in __import__("devo_amd.build", fromlist=["SOURCES"]).SOURCES


def test_abi_version_is_still_9():
    from devo_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert re.search(r"#define DEVO_ABI_VERSION 9\b", _read("include", "devo_hip.h"))


def restate(g, name, P=3):
    """train.py:176-236 and :254-266 for one case of the fixture, from oracle/se3.py and torch.linalg.svdvals -> the eleven statistics."""
    k = "case/" + name + "/"
    d = lambda f: torch.from_numpy(g[k + f]).double()
    v, x, y, Gs, Ps = d("v"), d("x"), d("y"), d("Gs")[0], d("Ps")[0]
    e = (x - y).norm(dim=-1).reshape(-1, P * P)
    flow = e[v.reshape(-1) > 0.5].min(dim=-1).values.mean()
    px1 = (e < 0.25).double().mean()
    sc = torch.zeros((), dtype=torch.float64)
    if k + "scores" in g.files:
        s, vf, xf, yf, w, kk = d("scores"), d("v_full"), d("x_full"), d("y_full"), d("ba_weights"), torch.from_numpy(g[k + "kk"])
        ok = vf >= 0.5
        ef = (xf - yf).norm(dim=-1).reshape(-1, P * P)[ok].min(dim=-1).values
        sc = ((-0.5 * w[ok].mean(dim=-1).log() + 1) * s[kk[ok]] * ef).mean() + (-torch.clamp(s, min=1e-6).log()).mean()
    A, B = se3.inv(Gs), se3.inv(Ps)
    t1, t2 = A[:, :3], B[:, :3]
    c1, c2 = t1 - t1.mean(0), t2 - t2.mean(0)
    var = (c2.norm(dim=1) ** 2).mean()
    H = c2.T @ c1 / len(t1)
    scale = torch.clamp(var / torch.linalg.svdvals(H).sum(), max=10.0)
    A = torch.cat([A[:, :3] * scale, A[:, 3:]], -1)
    n = len(A)
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    keep = ii != jj
    ii, jj = ii[keep], jj[keep]
    dP = se3.mul(se3.inv(A[ii]), A[jj])
    dG = se3.mul(se3.inv(B[ii]), B[jj])
    e1 = se3.logm(se3.mul(dP, se3.inv(dG)))
    tr, ro = e1[:, :3].norm(dim=-1), e1[:, 3:].norm(dim=-1)
    f = lambda m: m.double().mean()
    return torch.stack([flow, tr.mean() + ro.mean(), tr.mean(), ro.mean(), px1, f(ro < .001), f(ro < .01), f(tr < .001), f(tr < .01), sc, scale])


def test_fixture_agrees_with_an_independent_restatement(golden):
    names = [str(n) for n in golden["names"]]
    assert len(names) == 28
    fw, pw, sw = golden["weights"]
    for name in names:
        want = torch.from_numpy(golden["case/" + name + "/stats"])
        got = restate(golden, name)
        nan = torch.isnan(want)
        assert torch.equal(nan, torch.isnan(got)), name
        scale = max(1.0, float(want[~nan].abs().max()))
        err = float((want - got)[~nan].abs().max())
        assert err <= 1e-10 * scale, f"{name}: {err:.3e}"
        total = fw * got[0] + sw * got[9] + pw * got[1]
        if not bool(torch.isnan(total)):
            assert abs(float(total) - float(golden["case/" + name + "/loss"])) <= 1e-10 * max(1.0, abs(float(total))), name


def test_fixture_covers_the_listed_cases(golden):
    s = lambda name: dict(zip(FIELDS, golden["case/" + name + "/stats"]))
    assert np.isnan(s("flow/none_65")["flow"]) and not golden["case/flow/none_65/g_coords"].any()
    assert (golden["case/flow/none_65/v"] == 0.5).any() and golden["case/flow/mixed_65/v"][0, 3] == 0.5 and golden["case/score/general/v_full"][2] == 0.5
    x, y = golden["case/flow/mixed_513/x"], golden["case/flow/mixed_513/y"]
    assert (x[0, 5, 1, 2] == y[0, 5, 1, 2]).all() and not golden["case/flow/mixed_513/g_coords"][0, 5].any()
    for n in (2, 3, 15):
        assert s(f"pose/identity_{n}")["scale"] == 10.0 and np.isinf(golden[f"case/pose/identity_{n}/raw_scale"])
        assert s(f"pose/twentieth_{n}")["scale"] == 10.0 and 19 < golden[f"case/pose/twentieth_{n}/raw_scale"] < 21
        assert s(f"pose/same_{n}")["scale"] == 1.0 and s(f"pose/same_{n}")["pose"] == 0.0 and not golden[f"case/pose/same_{n}/g_Gs"].any()
        assert abs(s(f"pose/same_rot_{n}")["scale"] - 1.0) < 1e-12
    sc = golden["case/score/general/scores"]
    assert (sc < 1e-6).sum() == 3 and (sc != np.float32(1e-6)).all()
    assert np.bincount(golden["case/score/general/kk"]).max() <= 40
    assert np.isnan(s("score/none")["scores"])


def test_losses_refuse_cpu_tensors_and_a_batch_of_two():
    from devo_amd import losses
    mk = lambda B: (torch.ones(B, 4), torch.zeros(B, 4, 3, 3, 2), torch.ones(B, 4, 3, 3, 2), torch.zeros(B, 3, 7), torch.zeros(B, 3, 7))
    with pytest.raises(RuntimeError, match="GPU"):
        losses.iteration_loss(*mk(1), index=2)
    with pytest.raises(ValueError, match="one sequence"):
        losses.iteration_loss(*mk(2), index=2)
    with pytest.raises(ValueError):
        losses.sequence_loss([])
    assert (losses.FLOW_WEIGHT, losses.POSE_WEIGHT, losses.SCORES_WEIGHT) == (0.1, 10.0, 0.05)
