"""devo_amd.optim (csrc/optim.hip): clip + AdamW in two launches against tests/optim_ref.py, the fp64 restatement.

Units.  Differences from the restatement are counted in units of 2^-24 times a per-tensor scale: for p max|p_ref| + steps * max_lr, for m
(1 - beta1^steps) * max|g coef|, for v (1 - beta2^steps) * max|g coef|^2.  The yardstick is torch's own fp32 CPU optimiser on the same inputs,
measured in the same units in the same run; the kernel is allowed 4 x torch's figure per quantity with a floor of 1 unit (an equally valid
operation order doubles the roundings; a wrong formula shows as hundreds of units).  Measured figures: profiles/optim.txt.

The file's name puts it behind test_gpu_train_graph.py in the suite's order.  test_reference_schedule_end_to_end there bounds a difference
by the difference between the process's first two runs of TrainNet at a workload; a module that runs TrainNet at "tiny" before it (the
real-model and training-step tests below do) takes the first-run effects out of that difference and with them the bound's slack."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
UNIT = 2.0 ** -24
NAMES = [n for n, _ in R.SHAPES]


# ------------------------------------------------------------------------------------------------ runners
def _tensor(a, name, device):
    t = torch.from_numpy(a).to(device)
    return t.contiguous(memory_format=torch.channels_last) if name == "cl" else t


def _params(params, device):
    return [torch.nn.Parameter(_tensor(params[n], n, device)) for n in NAMES]


def _set_grads(ps, g, device):
    for q, n in zip(ps, NAMES):
        q.grad = None if g[n] is None else _tensor(g[n], n, device)


def _collect(ps, moments, norms=None):
    out = dict(p={n: q.detach().cpu().contiguous() for n, q in zip(NAMES, ps)}, m={}, v={}, norms=norms)
    for i, n in enumerate(NAMES):
        s = moments.get(i)
        out["m"][n] = torch.zeros(ps[i].shape) if s is None else s["exp_avg"].cpu().contiguous()
        out["v"][n] = torch.zeros(ps[i].shape) if s is None else s["exp_avg_sq"].cpu().contiguous()
    return out


def run_fused(steps, scale, skip_nonfinite=False):
    """the case under devo_amd.optim.AdamW with torch's OneCycleLR driving the rate -> p, m, v on the host and the norm of every step"""
    from devo_amd import optim
    params, grads = R.make_case(steps, scale)
    ps = _params(params, DEV)
    opt = optim.AdamW(ps, lr=R.MAX_LR, max_norm=R.MAX_NORM, skip_nonfinite=skip_nonfinite, names=NAMES, **R.HYPER)
    sched = optim.one_cycle(opt, R.MAX_LR, R.TOTAL_STEPS)
    norms = []
    for g in grads:
        _set_grads(ps, g, DEV)
        opt.step()
        sched.step()
        norms.append(float(opt.grad_norm))
    assert isinstance(opt.grad_norm, torch.Tensor) and opt.grad_norm.dtype == torch.float64 and opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
    return _collect(ps, opt.state_dict()["state"], norms)


def run_torch(steps, scale, device="cpu"):
    """torch's own fp32 optimiser on the same inputs: clip_grad_norm_ + AdamW + OneCycleLR"""
    params, grads = R.make_case(steps, scale)
    ps = _params(params, device)
    opt = torch.optim.AdamW(ps, lr=R.MAX_LR, **R.HYPER)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, R.MAX_LR, R.TOTAL_STEPS, pct_start=0.01, cycle_momentum=False, anneal_strategy="linear")
    for g in grads:
        _set_grads(ps, g, device)
        torch.nn.utils.clip_grad_norm_(ps, R.MAX_NORM)
        opt.step()
        sched.step()
    return _collect(ps, {i: opt.state[q] for i, q in enumerate(ps) if q in opt.state})


def scales(ref, grads, steps):
    """per tensor: the unit scales of p, m, v"""
    b1, b2 = R.HYPER["betas"]
    out = {}
    for n in NAMES:
        gmax = max((float(np.abs(g[n]).max()) * c for g, c in zip(grads, ref["coefs"]) if g[n] is not None), default=0.0)
        out[n] = dict(p=float(np.abs(ref["p"][n]).max()) + steps * R.MAX_LR, m=(1 - b1 ** steps) * gmax, v=(1 - b2 ** steps) * gmax * gmax)
    return out


def units(got, ref, sc):
    """-> {quantity: the worst difference from the restatement over all tensors, in units}; a zero scale demands exact zeros"""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for q in worst:
        for n in NAMES:
            d = float(np.abs(got[q][n].numpy().astype(np.float64) - ref[q][n]).max())
            if sc[n][q] == 0.0:
                assert d == 0.0 and float(np.abs(ref[q][n]).max()) == 0.0, (q, n, d)
                continue
            worst[q] = max(worst[q], d / (UNIT * sc[n][q]))
    return worst


@functools.lru_cache(maxsize=None)
def case(steps, scale):
    """computed once per (steps, scale) and shared: the restatement, the unit scales, torch's fp32 CPU figure and the bound it sets"""
    params, grads = R.make_case(steps, scale)
    ref = R.run(params, grads)
    sc = scales(ref, grads, steps)
    yard = units(run_torch(steps, scale), ref, sc)
    bound = {q: max(1.0, 4.0 * yard[q]) for q in yard}
    return params, grads, ref, sc, yard, bound


def within(got, steps, scale, what):
    params, grads, ref, sc, yard, bound = case(steps, scale)
    u = units(got, ref, sc)
    print(f"{what}: steps {steps} scale {scale}: units p {u['p']:.2f} m {u['m']:.2f} v {u['v']:.2f} | torch fp32 CPU p {yard['p']:.2f} m {yard['m']:.2f} v {yard['v']:.2f}"
          f" | bound p {bound['p']:.2f} m {bound['m']:.2f} v {bound['v']:.2f}")
    for q in u:
        assert u[q] <= bound[q], (what, q, u[q], bound[q])
    return u


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(a[q][n]), bits(b[q][n])) for q in "pmv" for n in NAMES)


# ------------------------------------------------------------------------------------------------ the step against the restatement
@pytest.mark.parametrize("scale", [0.01, 3.0])
@pytest.mark.parametrize("steps", [1, 12])
def test_step_matches_the_restatement(steps, scale):
    params, grads, ref, sc, yard, bound = case(steps, scale)
    got = run_fused(steps, scale)
    for k, (a, b) in enumerate(zip(got["norms"], ref["norms"])):
        assert abs(a - b) <= 1e-10 * b, (k, a, b)                      # fp64 summation: n 2^-53 is far below this at these sizes
    assert (max(ref["coefs"]) < 1.0) == (scale == 3.0)                  # the clip is active at 3.0 and idle at 0.01
    within(got, steps, scale, "fused")
    # no gradient: bit-unchanged, moments stay zero.  All-zero gradient: m and v exactly zero, p only decays.
    assert torch.equal(bits(got["p"]["none"]), bits(torch.from_numpy(params["none"]))) and not got["m"]["none"].any() and not got["v"]["none"].any()
    assert not got["m"]["zero"].any() and not got["v"]["zero"].any()
    decay = np.prod([1.0 - lr * R.HYPER["weight_decay"] for lr in ref["lrs"]])
    # (per step the fp32 factor 1 - lr wd and the product each round once: at most half a unit of |p| each; twice that is allowed)
    assert np.abs(got["p"]["zero"].numpy() - params["zero"].astype(np.float64) * decay).max() <= 2 * steps * UNIT * np.abs(params["zero"]).max()
    assert got["p"]["cl"].shape == (8, 3, 3, 3)


# ------------------------------------------------------------------------------------------------ reproducibility, the two bindings
_LEG = r"""
import os, sys
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_train_optim as T
from devo_amd import backends as B
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
out = T.run_fused(12, 3.0)
torch.save({q: out[q] for q in "pmv"} | {"norms": out["norms"]}, sys.argv[2])
"""


def test_two_runs_and_both_bindings_give_the_same_bits(tmp_path):
    a, b = run_fused(12, 3.0), run_fused(12, 3.0)
    assert same_bits(a, b) and a["norms"] == b["norms"]
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        c = torch.load(path)
        assert same_bits(a, c) and a["norms"] == c["norms"], binding


# ------------------------------------------------------------------------------------------------ the host runs ahead of the device
def test_steps_enqueued_ahead_of_the_device():
    """several large matmuls (about 10 ms) keep the device busy while the host enqueues two steps back to back, each with freshly allocated
    gradients of other values (the first step's are freed before the second's are made, so the allocator may hand out the same addresses):
    bit-equal to the same two steps with a synchronise between them"""
    from devo_amd import optim
    params, grads = R.make_case(2, 3.0)
    stash = [{n: None if g[n] is None else _tensor(g[n], n, DEV) for n in NAMES} for g in grads]
    big = torch.randn(8192, 8192, device=DEV)

    def run(sync):
        ps = _params(params, DEV)
        opt = optim.AdamW(ps, lr=R.MAX_LR, max_norm=R.MAX_NORM, names=NAMES, **R.HYPER)
        torch.cuda.synchronize()
        if not sync:
            for _ in range(3):
                big @ big
        for k in range(2):
            for q, n in zip(ps, NAMES):
                q.grad = None if stash[k][n] is None else stash[k][n].clone(memory_format=torch.preserve_format)
            opt.param_groups[0]["lr"] = R.one_cycle_lr(k, R.MAX_LR, R.TOTAL_STEPS)
            opt.step()
            opt.zero_grad(set_to_none=True)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return _collect(ps, opt.state_dict()["state"])

    a, b = run(True), run(False)
    assert same_bits(a, b)
    within(b, 2, 3.0, "enqueued ahead")


# ------------------------------------------------------------------------------------------------ resume across the two optimisers
def _manual_steps(opt, ps, grads, first, clip):
    for k, g in enumerate(grads):
        _set_grads(ps, g, DEV)
        opt.param_groups[0]["lr"] = R.one_cycle_lr(first + k, R.MAX_LR, R.TOTAL_STEPS)
        if clip:
            torch.nn.utils.clip_grad_norm_(ps, R.MAX_NORM)
        opt.step()


@pytest.mark.parametrize("first", ["fused", "torch"])
def test_resume_in_the_other_optimiser(first):
    """3 steps in one optimiser, its state_dict() loaded into the other, 3 more steps in each: both stay within the 6-step bound"""
    from devo_amd import optim
    params, grads = R.make_case(6, 3.0)
    ps = _params(params, DEV)
    fused = lambda q: optim.AdamW(q, lr=R.MAX_LR, max_norm=R.MAX_NORM, names=NAMES, **R.HYPER)
    plain = lambda q: torch.optim.AdamW(q, lr=R.MAX_LR, **R.HYPER)
    a = (fused if first == "fused" else plain)(ps)
    _manual_steps(a, ps, grads[:3], 0, clip=first == "torch")
    sd = copy.deepcopy(a.state_dict())
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3.0
    assert set(sd["param_groups"][0]) == set(torch.optim.AdamW([torch.zeros(1)], lr=1e-3).state_dict()["param_groups"][0])
    ps2 = [torch.nn.Parameter(q.detach().clone(memory_format=torch.preserve_format)) for q in ps]
    b = (plain if first == "fused" else fused)(ps2)
    b.load_state_dict(sd)
    _manual_steps(a, ps, grads[3:], 3, clip=first == "torch")
    _manual_steps(b, ps2, grads[3:], 3, clip=first == "fused")
    for opt, q, what in ((a, ps, first), (b, ps2, "the other")):
        state = opt.state_dict()["state"] if isinstance(opt, optim.AdamW) else {i: opt.state[t] for i, t in enumerate(q) if t in opt.state}
        assert all(float(s["step"]) == 6.0 for i, s in state.items() if NAMES[i] != "none")
        within(_collect(q, state), 6, 3.0, f"resume from {first}: {what}")


def test_a_state_with_differing_step_counts_is_refused():
    from devo_amd import optim
    params, grads = R.make_case(1, 3.0)
    ps = _params(params, DEV)
    opt = optim.AdamW(ps, lr=R.MAX_LR, names=NAMES)
    _set_grads(ps, grads[0], DEV)
    opt.step()
    sd = opt.state_dict()
    sd["state"][2]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="step counts differ"):
        opt.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------ skip_nonfinite
def test_skip_nonfinite():
    from devo_amd import optim
    params, grads = R.make_case(1, 3.0)
    ps = _params(params, DEV)
    opt = optim.AdamW(ps, lr=R.MAX_LR, max_norm=R.MAX_NORM, skip_nonfinite=True, names=NAMES, **R.HYPER)
    opt.param_groups[0]["lr"] = R.one_cycle_lr(0, R.MAX_LR, R.TOTAL_STEPS)
    bad = {n: None if g is None else g.copy() for n, g in grads[0].items()}
    bad["five"][3] = np.inf
    _set_grads(ps, bad, DEV)
    opt.step()
    assert opt.counters() == (0, 1) and float(opt.grad_norm) == float("inf")
    assert all(torch.equal(bits(q.detach().cpu()), bits(torch.from_numpy(params[n]))) for q, n in zip(ps, NAMES))
    assert not opt._m.any() and not opt._v.any() and opt.state_dict()["state"] == {}
    _set_grads(ps, grads[0], DEV)
    opt.step()
    assert opt.counters() == (1, 1)
    within(_collect(ps, opt.state_dict()["state"]), 1, 3.0, "first finite step after a skipped one")
    # without the switch the non-finite values propagate, as in torch
    ps = _params(params, DEV)
    opt = optim.AdamW(ps, lr=R.MAX_LR, max_norm=R.MAX_NORM, names=NAMES, **R.HYPER)
    _set_grads(ps, bad, DEV)
    opt.step()
    assert opt.counters() == (1, 0) and torch.isnan(ps[NAMES.index("five")].detach()).any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from devo_amd import optim
    new = lambda *shape: torch.nn.Parameter(torch.randn(*shape, device=DEV))
    with pytest.raises(ValueError, match="CPU"):
        optim.AdamW([new(4), torch.nn.Parameter(torch.zeros(4))], lr=1e-3)
    with pytest.raises(ValueError, match="float32 only"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))], lr=1e-3)
    with pytest.raises(ValueError, match="groups"):
        optim.AdamW([{"params": [new(4)]}, {"params": [new(4)]}], lr=1e-3)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW([new(4)], lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.AdamW([new(4)], lr=1e-3, maximize=True)
    with pytest.raises(ValueError, match="not non-overlapping and dense"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, 10, device=DEV)[:, ::2])], lr=1e-3, names=["gappy"])
    with pytest.raises(ValueError, match="odd.*not 16-byte aligned"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(9, device=DEV)[1:])], lr=1e-3, names=["odd"])

    w = torch.nn.Parameter(torch.randn(8, 3, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last))
    v = new(8)
    opt = optim.AdamW([w, v], lr=1e-3, names=["w", "v"])
    with pytest.raises(ValueError, match="more than one parameter group"):
        opt.add_param_group({"params": [new(4)]})
    before = (w.detach().clone(), v.detach().clone())

    def refused(match, **grads):
        w.grad, v.grad = grads.get("w"), grads.get("v", torch.ones(8, device=DEV))
        with pytest.raises(ValueError, match=match):
            opt.step()

    w.grad, v.grad = torch.empty_like(w), torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: 0.0)
    refused("w .*strides", w=torch.randn(8, 3, 3, 3, device=DEV))                                   # contiguous gradient of a channels-last weight
    refused("v .*sparse", v=torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (8,), device=DEV))
    refused("v .*not 16-byte aligned", v=torch.ones(9, device=DEV)[1:])
    with pytest.raises((ValueError, RuntimeError)):                                                 # torch itself refuses to hold such a gradient
        v.grad = torch.ones(8, device=DEV, dtype=torch.float16)
        opt.step()
    v.grad = torch.ones(8, device=DEV)
    v.data = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="storage of parameter v"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), before[0]) and opt.counters() == (0, 0)                          # nothing was launched


# ------------------------------------------------------------------------------------------------ the real model
@functools.lru_cache(maxsize=None)
def _trained_once():
    """one forward + backward of TrainNet at the smallest workload synth offers -> (net, cloned gradients by name)"""
    from devo_amd import training as T
    net, model, _ = T.build_trainer(DEV, 1)
    batch = T.make_batch("tiny", 1234, DEV)
    loss = model(batch, iters=6, schedule="reference", init_frames=2, warmup=2)
    loss.backward()
    return net, {k: None if q.grad is None else q.grad.detach().clone(memory_format=torch.preserve_format) for k, q in net.named_parameters()}


def test_the_real_model():
    """all of TrainNet's tensors after one step, against the restatement, within 4 x what torch's fp32 CPU optimiser shows on the same inputs"""
    from devo_amd import optim, training as T
    net, grads = _trained_once()
    lr, wd, clip = 8e-5, 1e-6, 10.0
    names = [k for k, _ in net.named_parameters()]
    assert len(names) == 102 and sum(g is not None for g in grads.values()) > 50
    start = {k: q.detach().cpu().contiguous().numpy().copy() for k, q in net.named_parameters()}
    g_np = {k: None if g is None else g.cpu().contiguous().numpy() for k, g in grads.items()}
    p = [start[k].astype(np.float64) for k in names]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    norm, coef = R.step(p, [g_np[k] for k in names], m, v, 1, lr, weight_decay=wd, max_norm=clip)
    # torch on copies of the parameters, fp32 on the CPU (the module itself holds device events and cannot be deep-copied)
    cpu = {k: torch.nn.Parameter(q.detach().cpu()) for k, q in net.named_parameters()}
    for k, q in cpu.items():
        q.grad = None if grads[k] is None else grads[k].cpu()
    topt = torch.optim.AdamW(cpu.values(), lr=lr, weight_decay=wd)
    torch.nn.utils.clip_grad_norm_(cpu.values(), clip)
    topt.step()
    # the new step on copies on the device, laid out like the model's own tensors (the shared model stays as it is)
    dev = {k: torch.nn.Parameter(q.detach().clone(memory_format=torch.preserve_format)) for k, q in net.named_parameters()}
    assert all(a.stride() == b.stride() for a, b in zip(dev.values(), net.parameters()))
    for k, q in dev.items():
        q.grad = None if grads[k] is None else grads[k].clone(memory_format=torch.preserve_format)
    opt = optim.AdamW(dev.values(), lr=lr, weight_decay=wd, max_norm=clip, names=names)
    opt.step()
    assert abs(float(opt.grad_norm) - norm) <= 1e-10 * norm
    state = opt.state_dict()["state"]
    b1, b2 = 0.9, 0.999
    worst = {w: dict(p=0.0, m=0.0, v=0.0) for w in ("torch", "fused")}
    for i, k in enumerate(names):
        if g_np[k] is None:
            assert torch.equal(dev[k].detach().cpu().contiguous(), torch.from_numpy(start[k]))
            continue
        gmax = float(np.abs(g_np[k]).max()) * coef
        sc = dict(p=float(np.abs(p[i]).max()) + lr, m=(1 - b1) * gmax, v=(1 - b2) * gmax * gmax)
        tq = cpu[k]
        got = {"torch": dict(p=tq.detach(), m=topt.state[tq]["exp_avg"], v=topt.state[tq]["exp_avg_sq"]),
               "fused": dict(p=dev[k].detach().cpu(), m=state[i]["exp_avg"].cpu(), v=state[i]["exp_avg_sq"].cpu())}
        for w in got:
            for q, ref in (("p", p[i]), ("m", m[i]), ("v", v[i])):
                d = float(np.abs(got[w][q].contiguous().numpy().astype(np.float64) - ref).max())
                if sc[q] == 0.0:
                    assert d == 0.0, (w, k, q)
                else:
                    worst[w][q] = max(worst[w][q], d / (UNIT * sc[q]))
    print(f"TrainNet, 1 step, norm {norm:.4f} coef {coef:.4f}: fused units {worst['fused']} | torch fp32 CPU {worst['torch']}")
    for q in "pmv":
        assert worst["fused"][q] <= max(1.0, 4.0 * worst["torch"][q]), (q, worst)


# ------------------------------------------------------------------------------------------------ the training step
def test_training_step_with_the_fused_optimiser_schedule_and_checkpoint(tmp_path):
    """build_trainer(optimizer="fused", total_steps=300) + train_step: the rate follows torch's schedule from 3.2e-6 on; save_checkpoint ->
    load_checkpoint -> one more step equals the uninterrupted run bit for bit"""
    from devo_amd import optim, training as T
    batch = T.make_batch("tiny", 1234, DEV)

    def fresh():
        net, model, opt, sched = T.build_trainer(DEV, 1, optimizer="fused", total_steps=300)
        assert isinstance(opt, optim.AdamW) and opt.max_norm == 10.0 and isinstance(sched, torch.optim.lr_scheduler.OneCycleLR)
        return net, model, opt, sched

    def one_step(model, opt, sched):
        return T.train_step(model, opt, batch, scheduler=sched, iters=6, schedule="reference", init_frames=2, warmup=2)

    net, model, opt, sched = fresh()
    assert abs(opt.param_groups[0]["lr"] - 3.2e-6) < 1e-12
    lrs = []
    for k in range(3):
        loss = one_step(model, opt, sched)
        lrs.append(opt.param_groups[0]["lr"])
    assert torch.isfinite(loss) and torch.isfinite(opt.grad_norm) and float(opt.grad_norm) > 0
    want = [R.one_cycle_lr(k, 8e-5, 300) for k in (1, 2, 3)]
    assert max(abs(a - b) for a, b in zip(lrs, want)) < 1e-15 and lrs[1] > lrs[0] and lrs[2] < lrs[1]      # up to the peak at step 2, then down
    assert opt.counters() == (3, 0)

    # checkpoint: the state after 3 steps written, read into a fresh trainer; then the SAME gradients are applied to both (the model's own
    # backward has float atomics in it: two runs of it do not give the same bits, whatever the optimiser)
    path = str(tmp_path / "ckpt.pth")
    T.save_checkpoint(path, 3, model, opt, sched)
    ckpt = torch.load(path)
    assert set(ckpt) == {"steps", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"} and ckpt["steps"] == 3
    net2, model2, opt2, sched2 = fresh()
    assert T.load_checkpoint(path, model2, opt2, sched2) == 3
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] and sched2.last_epoch == sched.last_epoch
    for (k, a), (_, b) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
    g = torch.Generator(device=DEV).manual_seed(5)
    shared = [torch.randn(q.shape, device=DEV, generator=g) for q in net.parameters()]
    for m_, o_, s_ in ((net, opt, sched), (net2, opt2, sched2)):
        for q, gq in zip(m_.parameters(), shared):
            q.grad = torch.empty_like(q).copy_(gq)
        o_.step()
        s_.step()
    assert torch.equal(opt.grad_norm, opt2.grad_norm)
    for (k, a), (_, b) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
    sa, sb = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert all(torch.equal(sa[i][key], sb[i][key]) for i in sa for key in ("step", "exp_avg", "exp_avg_sq"))

    # the legacy form: a bare state dict with DDP's prefix and one entry of another shape
    legacy = {"module." + k: v for k, v in net.state_dict().items()}
    odd = next(iter(legacy))
    legacy[odd] = torch.zeros(3, 5)
    torch.save(legacy, path)
    net3 = fresh()[0]
    kept = net3.state_dict()[odd.replace("module.", "")].clone()
    assert T.load_checkpoint(path, net3) == 0
    for k, v in net3.state_dict().items():
        assert torch.equal(v, kept if "module." + k == odd else net.state_dict()[k]), k
