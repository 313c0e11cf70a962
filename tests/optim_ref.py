"""fp64 numpy restatement of the tail of a training step (train.py:248-250): clip_grad_norm_ -> torch.optim.AdamW.step() -> OneCycleLR.step().
fp32 inputs, fp64 arithmetic; tests/test_optim_cpu.py holds it against torch itself in fp64, tests/test_gpu_train_optim.py holds devo_amd.optim against it.
Also the shared inputs of those tests (`make_case`): plain numpy, so a child process rebuilds the same bits."""
import numpy as np

CHUNK = 2048                                  # DEVO_OPTIM_CHUNK: the test shapes straddle it


def one_cycle_lr(step, max_lr, total_steps, pct_start=0.01, div_factor=25.0, final_div_factor=1e4):
    """the rate OneCycleLR(anneal_strategy='linear', three_phase=False) sets for optimiser step number `step` (0-based)"""
    initial, min_lr = max_lr / div_factor, max_lr / div_factor / final_div_factor
    end1, end2 = float(pct_start * total_steps) - 1.0, float(total_steps) - 1.0
    if step <= end1:
        return (max_lr - initial) * (step / end1) + initial
    return (min_lr - max_lr) * ((step - end1) / (end2 - end1)) + max_lr


def grad_norm(grads):
    """sqrt of the sum of squares over every gradient that is not None, in fp64"""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s factor: min(1, max_norm / (norm + 1e-6)); None: no clipping"""
    return 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))


def step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
    """One step in place over lists of fp64 arrays (g entries fp32 / fp64 arrays or None: that tensor is skipped whole); t = 1 for the first
    step.  -> (norm before clipping, coef)."""
    b1, b2 = betas
    norm = grad_norm(g)
    coef = clip_coef(norm, max_norm)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for i in range(len(p)):
        if g[i] is None:
            continue
        gi = np.asarray(g[i], dtype=np.float64) * coef
        p[i] *= 1.0 - lr * weight_decay
        m[i] += (gi - m[i]) * (1.0 - b1)
        v[i] *= b2
        v[i] += (1.0 - b2) * gi * gi
        p[i] -= (lr / bc1) * m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + eps)
    return norm, coef


# ------------------------------------------------------------------------------------------------ the shared inputs
# name -> shape; "cl" is an (8, 3, 3, 3) convolution weight kept channels-last, "zero" gets an all-zero gradient, "none" no gradient at all,
# "tiny" gradients of the size of eps
SHAPES = (("one", (1,)), ("three", (3,)), ("five", (5,)), ("chunk", (CHUNK,)), ("chunk+1", (CHUNK + 1,)), ("3chunks+2", (3 * CHUNK + 2,)), ("cl", (8, 3, 3, 3)),
          ("zero", (7,)), ("none", (9,)), ("tiny", (33,)))
MAX_LR, TOTAL_STEPS, MAX_NORM = 1e-3, 300, 10.0
HYPER = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def make_case(steps, scale, seed=0):
    """-> (params {name: fp32 array}, grads [step] {name: fp32 array or None}) for SHAPES.  Gradients are `scale` x N(0, 1): with
    scale 0.01 the norm stays below MAX_NORM (the clip is idle), with 3.0 it is far above (the clip is active)."""
    rng = np.random.default_rng(20240 + seed)
    params = {n: rng.standard_normal(s).astype(np.float32) for n, s in SHAPES}
    grads = []
    for _ in range(steps):
        g = {n: (scale * rng.standard_normal(s)).astype(np.float32) for n, s in SHAPES}
        g["zero"] = np.zeros_like(g["zero"])
        g["none"] = None
        g["tiny"] = (1e-7 * rng.standard_normal(dict(SHAPES)["tiny"])).astype(np.float32)
        grads.append(g)
    return params, grads


def run(params, grads, first_step=0, state=None, max_norm=MAX_NORM):
    """the restatement over a case: -> dict(p, m, v {name: fp64}, norms [step], coefs [step], lrs [step]); `state` = (m, v) to resume from,
    `first_step` the number of steps already taken"""
    names = list(params)
    p = [params[n].astype(np.float64) for n in names]
    m = [np.zeros_like(x) for x in p] if state is None else [state[0][n].astype(np.float64) for n in names]
    v = [np.zeros_like(x) for x in p] if state is None else [state[1][n].astype(np.float64) for n in names]
    norms, coefs, lrs = [], [], []
    for k, g in enumerate(grads):
        lr = one_cycle_lr(first_step + k, MAX_LR, TOTAL_STEPS)
        norm, coef = step(p, [g[n] for n in names], m, v, first_step + k + 1, lr, max_norm=max_norm, **HYPER)
        norms.append(norm), coefs.append(coef), lrs.append(lr)
    return dict(p=dict(zip(names, p)), m=dict(zip(names, m)), v=dict(zip(names, v)), norms=norms, coefs=coefs, lrs=lrs)
