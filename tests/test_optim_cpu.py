"""tests/optim_ref.py (the fp64 restatement of clip + AdamW + the one-cycle rate) against torch itself in fp64, and the host parts of
devo_amd.optim that need no GPU: the refusals that can be seen without one."""
import numpy as np
import pytest
import torch

import optim_ref as R

STEPS = 12                                     # of a 300-step schedule: the warm-up peak at step 2 is crossed


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    return 0.0 if scale == 0 and np.abs(a).max() == 0 else float(np.abs(a - b).max() / scale)


@pytest.mark.parametrize("scale", [0.01, 3.0])
def test_restatement_matches_torch_in_fp64(scale):
    params, grads = R.make_case(STEPS, scale)
    names = list(params)
    tp = [torch.nn.Parameter(torch.from_numpy(params[n]).double()) for n in names]
    opt = torch.optim.AdamW(tp, lr=R.MAX_LR, foreach=False, **R.HYPER)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, R.MAX_LR, R.TOTAL_STEPS, pct_start=0.01, cycle_momentum=False, anneal_strategy="linear")
    norms, lrs = [], []
    for g in grads:
        for q, n in zip(tp, names):
            q.grad = None if g[n] is None else torch.from_numpy(g[n]).double()
        lrs.append(opt.param_groups[0]["lr"])
        norms.append(float(torch.nn.utils.clip_grad_norm_(tp, R.MAX_NORM)))
        opt.step()
        sched.step()
    ref = R.run(params, grads)
    assert (max(ref["coefs"]) < 1.0) == (scale == 3.0) and (min(ref["coefs"]) == 1.0) == (scale == 0.01)      # the clip is active / idle as intended
    assert abs(ref["lrs"][0] - R.MAX_LR / 25) < 1e-18 and max(ref["lrs"]) == ref["lrs"][2] and abs(ref["lrs"][2] - R.MAX_LR) < 1e-18
    worst = max(_rel(ref["lrs"], lrs), _rel(ref["norms"], norms))
    for q, n in zip(tp, names):
        worst = max(worst, _rel(ref["p"][n], q.detach().numpy()))
        if n == "none":
            assert q not in opt.state and np.array_equal(ref["p"][n], params[n].astype(np.float64))
            continue
        worst = max(worst, _rel(ref["m"][n], opt.state[q]["exp_avg"].numpy()), _rel(ref["v"][n], opt.state[q]["exp_avg_sq"].numpy()))
    print(f"scale {scale}: restatement vs torch fp64, worst relative difference {worst:.2e}")
    assert worst <= 1e-11


def test_refusals_without_a_gpu():
    from devo_amd import optim
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(ValueError, match="CPU"):
        optim.AdamW([p], lr=1e-3)
    with pytest.raises(ValueError, match="groups"):
        optim.AdamW([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], lr=1e-3)
    for kw in ({"amsgrad": True}, {"maximize": True}):
        with pytest.raises(ValueError, match="amsgrad and maximize"):
            optim.AdamW([p], lr=1e-3, **kw)
    with pytest.raises(ValueError, match="max_norm"):
        optim.AdamW([p], lr=1e-3, max_norm=0.0)
    with pytest.raises(ValueError, match="no parameters"):
        optim.AdamW([], lr=1e-3)
    with pytest.raises(ValueError, match="at least 200"):
        optim.one_cycle(torch.optim.SGD([p], lr=1e-3), 1e-3, 100)
    assert optim._dense((8, 3, 3, 3), (27, 1, 9, 3)) and optim._dense((4, 1, 5), (5, 77, 1)) and not optim._dense((4, 5), (10, 1)) and not optim._dense((4, 5), (0, 1))
