"""tests/se3_series_ref.py (branch-free power series, fp64) against oracle/se3.py (the reference's closed forms and eps = 1e-6 switch), on the CPU.
Outside the band where the closed forms cancel, |phi| < 1e-6 and |phi| >= 0.3, the two are independent statements of the same maps and must
agree to 1e-12.  Inside it the oracle's fp64 closed forms lose digits — the largest deviation measured is 4.6e-9 (expm_backward at 1e-4 rad) —
and must stay within 1e-7: that documents the oracle's known deviation, and a broken series reference fails either half."""
import math
import pytest
import torch
from oracle import se3 as K

import se3_series_ref as S

OUTSIDE = [1e-7, 9e-7, 0.3, 0.5, 0.99, 1.01, 2.0, 3.1, math.pi - 1e-3]
INSIDE = [1.1e-6, 3e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-2, 0.1]


def _errors(theta):
    a, X, g7, b = S.sweep_inputs(theta, torch.float64)
    pairs = {
        "expm": (K.expm(a), S.exp_ref(a)),
        "logm": (K.logm(X), S.log_ref(X)),
        "expm_backward": (K.expm_backward(g7, a), S.expm_backward(g7, a)),
        "logm_backward": (K.logm_backward(b, X), S.logm_backward(b, X)),
        "jinv": (K.jinv(X, b), S.jinv(X, b)),
    }
    return {k: (got - want).abs().max().item() for k, (got, want) in pairs.items()}


@pytest.mark.parametrize("theta", OUTSIDE)
def test_series_reference_agrees_with_the_oracle_outside_the_band(theta):
    for name, err in _errors(theta).items():
        assert err <= 1e-12, f"{name} at |phi| = {theta:g}: {err:.2e}"


@pytest.mark.parametrize("theta", INSIDE)
def test_oracle_fp64_deviation_inside_the_band_is_bounded(theta):
    for name, err in _errors(theta).items():
        assert err <= 1e-7, f"{name} at |phi| = {theta:g}: {err:.2e}"


def test_the_sweep_brackets_the_switch_points_of_the_header():
    """S.SWITCH_POINTS is what devo_amd/csrc/se3_dev.h declares, and S.SWEEP_THETAS has a magnitude within 3 % (eps: 10 %) on either side of each."""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "devo_amd", "csrc", "se3_dev.h")) as f:
        src = f.read()
    found = {}
    for ty, body in re.findall(r"template <> struct Consts<(float|double)>\s*\{(.*?)\};", src):
        for name, val in re.findall(r"static constexpr \w+\s+(\w+) = ([0-9.e+-]+)f?;", body):
            found.setdefault(name, {})[ty] = float(val)
    assert found == S.SWITCH_POINTS, (
        f"se3_dev.h declares {found}, tests/se3_series_ref.py lists {S.SWITCH_POINTS}: if a switch point moved, update SWITCH_POINTS and bracket it in "
        "SWEEP_THETAS (0.97x, 1.03x); if only the layout of the Consts<T> specialisations changed, update the two patterns above")
    for name, per_type in S.SWITCH_POINTS.items():
        w = 0.1 if name == "eps" else 0.03
        for v in per_type.values():
            assert any((1 - w) * v * (1 - 1e-12) <= t < v for t in S.SWEEP_THETAS), (name, v)
            assert any(v < t <= (1 + w) * v * (1 + 1e-12) for t in S.SWEEP_THETAS), (name, v)


def test_log_inverts_exp_and_the_jacobian_is_the_derivative_of_exp():
    """The reference against itself: log_ref(exp_ref a) = a, and J_l(a) b = Log(Exp(a + h b) Exp(a)^-1) / h to the order of h (central)."""
    a, _, _, b = S.sweep_inputs(1e-3, torch.float64, n=32, seed=5)
    assert (S.log_ref(S.exp_ref(a)) - a).abs().max().item() <= 1e-13
    h = 1e-5
    num = (S.log_ref(K.mul(S.exp_ref(a + h * b), K.inv(S.exp_ref(a)))) - S.log_ref(K.mul(S.exp_ref(a - h * b), K.inv(S.exp_ref(a))))) / (2 * h)
    want = (S.left_jacobian(a) @ b[..., None])[..., 0]
    assert (num - want).abs().max().item() <= 1e-8
