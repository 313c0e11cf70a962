#!/usr/bin/env python3
"""Evidence for the RxSO3 / Sim3 numerics ("All four groups"): profiles/lie_groups.txt.
  1. deviation of exp, log, Jinv, exp_backward, log_backward from the fp64 series reference (tests/lie_groups_ref.py) over the sweep
     theta x sigma of tests/test_gpu_lie_groups.py, per theta row (maximum over the 19 sigma values, and where), next to the deviation of the
     reference project's own forms restated in numpy in the same arithmetic: the four-corner closed form of W (rxso3.h:190-233) for exp's
     translation, the truncated polynomials of sim3.h:167-191 for the two backward passes;
  2. the switch points;
  3. time of exp + log forward and backward at n = 2^20 per group and dtype: warm, medians of interleaved repeats.
python tools/bench_lie_groups.py [out.txt]"""
import math
import os
import re
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lie_groups_ref as R                                                   # noqa: E402
from devo_amd.backends import lietorch_backends as B                         # noqa: E402

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def P(*a):
    print(*a, file=out, flush=True)


def hat(p):
    z = np.zeros_like(p[0])
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=p.dtype)


def w_reference_form(phi, sigma, dt):
    """rxso3.h:190-233 restated, evaluated in dt."""
    EPS = dt(1e-6)
    one, half = dt(1), dt(0.5)
    phi = phi.astype(dt)
    sigma = dt(sigma)
    theta = np.sqrt((phi * phi).sum(dtype=dt))
    Phi = hat(phi)
    scale = np.exp(sigma)
    if abs(sigma) < EPS:
        C = one
        if abs(theta) < EPS:
            A, Bc = half, dt(1.0 / 6.0)
        else:
            t2 = theta * theta
            A, Bc = (one - np.cos(theta)) / t2, (theta - np.sin(theta)) / (t2 * theta)
    else:
        C = (scale - one) / sigma
        if abs(theta) < EPS:
            s2 = sigma * sigma
            A = ((sigma - one) * scale + one) / s2
            Bc = (scale * half * s2 + scale - one - sigma * scale) / (s2 * sigma)
        else:
            t2 = theta * theta
            a, b, c = scale * np.sin(theta), scale * np.cos(theta), t2 + sigma * sigma
            A = (a * sigma + (one - b) * theta) / (theta * c)
            Bc = (C - ((b - one) * sigma + a * theta) / c) * one / t2
    return (A * Phi + Bc * (Phi @ Phi) + C * np.eye(3, dtype=dt)).astype(dt)


def sim3_polynomials(a, dt):
    """sim3.h:167-191 restated (the dropped ad^5 term included: it is dropped there too), evaluated in dt."""
    X = R.ad_matrix(4, torch.from_numpy(a[None].astype(np.float64)))[0].numpy().astype(dt)
    X2 = X @ X
    X4 = X2 @ X2
    I = np.eye(7, dtype=dt)
    return (I + dt(0.5) * X + dt(1 / 6) * X2 + dt(1 / 24) * (X @ X2) + dt(1 / 120) * X4,
            I - dt(0.5) * X + dt(1 / 12) * X2 - dt(1 / 720) * X4)


def deviation_tables():
    for gid in (2, 4):
        for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
            S, bands = R.sweep_batch(gid, dt)
            d = lambda k: S[k].cuda().contiguous()
            ref = {"exp": R.expm(gid, S["a"]), "log": R.logm(gid, S["X"]), "Jinv": R.jinv(gid, S["X"], S["b"]),
                   "exp_backward": R.expm_backward(gid, S["gN"], S["a"]), "log_backward": R.logm_backward(gid, S["b"], S["X"])}
            got = {"exp": B.expm(gid, d("a")), "log": B.logm(gid, d("X")), "Jinv": B.Jinv(gid, d("X"), d("b")),
                   "exp_backward": B.expm_backward(gid, d("gN"), d("a"))[0], "log_backward": B.logm_backward(gid, d("b"), d("X"))[0]}
            theirs = {}
            if gid == 4:                                                     # the reference project's forms on the same rounded inputs
                a = S["a"].double().numpy()
                t_ref = ref["exp"][:, :3].numpy()
                Jl, Jli = R.left_jacobian(4, S["a"]).numpy(), R.left_jacobian_inverse(4, S["a"]).numpy()
                e_exp, e_jl, e_jli = np.zeros(len(a)), np.zeros(len(a)), np.zeros(len(a))
                for i in range(len(a)):
                    W = w_reference_form(a[i, 3:6], a[i, 6], npdt)
                    e_exp[i] = np.abs(W.astype(np.float64) @ a[i, :3].astype(npdt).astype(np.float64) - t_ref[i]).max()
                    pj, pji = sim3_polynomials(a[i], npdt)
                    e_jl[i], e_jli[i] = np.abs(pj - Jl[i]).max(), np.abs(pji - Jli[i]).max()
                theirs = {"exp": e_exp, "exp_backward": e_jl, "log_backward": e_jli}
            for name in got:
                o = got[name].double().cpu()
                P(f"\n{R.NAMES[gid]} {name} {str(dt)[6:]}: max |kernel - reference| / max(1, |reference|) per theta, maximum over sigma in +-{{0, 1e-7 .. 1e-2, 0.1, 0.3, 1}}"
                  + ("; right: the reference project's form, same arithmetic (matrix entries for the two backward passes)" if name in theirs else ""))
                for theta in R.SWEEP_THETAS:
                    worst, at, tw, tat = 0.0, 0.0, 0.0, 0.0
                    for th, sg, i0, i1 in bands:
                        if th != theta:
                            continue
                        r = ref[name][i0:i1]
                        e = (o[i0:i1] - r).abs().max().item() / max(1.0, r.abs().max().item())
                        if not e <= worst:
                            worst, at = e, sg
                        if name in theirs:
                            t = float(theirs[name][i0:i1].max())
                            if not t <= tw:
                                tw, tat = t, sg
                    line = f"  theta = {theta:<9.4g} {worst:9.2e} (sigma = {at:g})"
                    if name in theirs:
                        line += f"      {tw:9.2e} (sigma = {tat:g})"
                    P(line)


def timings():
    n = 1 << 20
    P(f"\nTimings, n = 2^20, microseconds: medians of 15 interleaved repeats after 3 warm rounds (events around one launch each)")
    P(f"{'group':6s} {'dtype':8s} {'exp':>9s} {'log':>9s} {'exp_bwd':>9s} {'log_bwd':>9s}")
    cases = []
    for gid in (1, 2, 3, 4):
        for dt in (torch.float32, torch.float64):
            ops = R.random_batch(gid, 4096, 1, dt)
            rep = lambda t: t.repeat(n // 4096, 1).cuda().contiguous()
            a, X, gN, gK = rep(ops["a"]), rep(ops["X"]), rep(ops["gN"]), rep(ops["gK"])
            cases.append((gid, dt, [lambda a=a, g=gid: B.expm(g, a), lambda X=X, g=gid: B.logm(g, X), lambda a=a, gN=gN, g=gid: B.expm_backward(g, gN, a),
                                    lambda X=X, gK=gK, g=gid: B.logm_backward(g, gK, X)]))
    times = {(c[0], c[1], k): [] for c in cases for k in range(4)}
    for rnd in range(18):
        for gid, dt, fns in cases:
            for k, f in enumerate(fns):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                e.synchronize()
                if rnd >= 3:
                    times[(gid, dt, k)].append(s.elapsed_time(e) * 1e3)
    for gid, dt, _ in cases:
        P(f"{R.NAMES[gid]:6s} {str(dt)[6:]:8s} " + " ".join(f"{float(np.median(times[(gid, dt, k)])):9.1f}" for k in range(4)))


if __name__ == "__main__":
    src = open(os.path.join(ROOT, "devo_amd", "csrc", "lie_dev.h")).read()
    P("Switch points (devo_amd/csrc/lie_dev.h, LieConsts<T>; the SO3 coefficients keep se3_dev.h's Consts<T>::series_max = 1.0 float / 0.3 double):")
    for m in re.finditer(r"template <> struct LieConsts<(\w+)>\s*\{([^}]*)\}", src):
        P(f"  {m.group(1):7s} {' '.join(m.group(2).split())}")
    deviation_tables()
    timings()
