"""HIP-backed module with the interface of the reference's `lietorch_backends` extension
(devo/lietorch/src/lietorch.cpp:286-316): 19 functions taking the group id first, for SO3 (1), RxSO3 (2), SE3 (3) and Sim3 (4).
Inputs arrive flattened [batch, dim] and contiguous (lietorch.cpp:7 CHECK_CONTIGUOUS); unlike the reference, the last dimension of
every operand is checked against the group (a wrong one would read out of bounds).  No CPU fallback."""
import torch
from .. import _lib as L

SE3_ID = 3
GROUP_DIMS = {1: (4, 3), 2: (5, 4), 3: (7, 6), 4: (8, 7)}          # group id -> (N embedded, K manifold): dispatch.h, so3.h:14-15 ... sim3.h:19-20


def _chk(group_id, *ts):
    """ts: (tensor, what) with what in 'N' (element), 'K' (tangent), 3 or 4 (points)."""
    if group_id not in GROUP_DIMS:
        raise RuntimeError(f"lietorch_backends (devo_amd): group_id must be 1 (SO3), 2 (RxSO3), 3 (SE3) or 4 (Sim3), got {group_id}")
    N, K = GROUP_DIMS[group_id]
    L.require_gpu(*[t for t, _ in ts])
    d = ts[0][0].dtype
    for t, what in ts:
        if not t.is_contiguous():
            raise RuntimeError("lietorch_backends: input must be contiguous")      # lietorch.cpp:7
        if t.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"lietorch_backends: float32/float64 only, got {t.dtype}")
        if t.dtype != d:
            raise RuntimeError("lietorch_backends: mixed dtypes")
        want = {"N": N, "K": K}.get(what, what)
        if t.dim() < 2 or t.shape[-1] != want or t.shape[0] != ts[0][0].shape[0] or t.numel() != t.shape[0] * want:
            raise RuntimeError(f"lietorch_backends: expected a [{ts[0][0].shape[0]}, {want}] tensor for group {group_id}, got {tuple(t.shape)}")
    return N, K


def _dim(what, N, K):
    return {"N": N, "K": K}.get(what, what)


def _unary(name, x, out):
    def f(group_id, X):
        N, K = _chk(group_id, (X, x))
        n = X.shape[0]
        o = torch.empty(n, _dim(out, N, K), dtype=X.dtype, device=X.device)
        L.check(getattr(L.lib(), name)(group_id, L.ptr(X), L.ptr(o), n, L.dtype_code(X), L.stream()), name)
        return o
    return f


def _unary_bwd(name, g, x, out):
    def f(group_id, grad, X):
        N, K = _chk(group_id, (grad, g), (X, x))
        n = X.shape[0]
        o = torch.empty(n, _dim(out, N, K), dtype=X.dtype, device=X.device)
        L.check(getattr(L.lib(), name)(group_id, L.ptr(grad), L.ptr(X), L.ptr(o), n, L.dtype_code(X), L.stream()), name)
        return [o]
    return f


def _binary(name, y, out):
    def f(group_id, X, Y):
        N, K = _chk(group_id, (X, "N"), (Y, y))
        n = X.shape[0]
        o = torch.empty(n, _dim(out, N, K), dtype=X.dtype, device=X.device)
        L.check(getattr(L.lib(), name)(group_id, L.ptr(X), L.ptr(Y), L.ptr(o), n, L.dtype_code(X), L.stream()), name)
        return o
    return f


def _binary_bwd(name, g, y):
    def f(group_id, grad, X, Y):
        N, K = _chk(group_id, (grad, g), (X, "N"), (Y, y))
        n = X.shape[0]
        dX = torch.empty(n, N, dtype=X.dtype, device=X.device)
        dy = torch.empty(n, _dim(y, N, K), dtype=X.dtype, device=X.device)
        L.check(getattr(L.lib(), name)(group_id, L.ptr(grad), L.ptr(X), L.ptr(Y), L.ptr(dX), L.ptr(dy), n, L.dtype_code(X),
                                       L.stream()), name)
        return [dX, dy]
    return f


expm, expm_backward = _unary("devo_lie_exp", "K", "N"), _unary_bwd("devo_lie_exp_backward", "N", "K", "K")
logm, logm_backward = _unary("devo_lie_log", "N", "K"), _unary_bwd("devo_lie_log_backward", "K", "N", "N")
inv, inv_backward = _unary("devo_lie_inv", "N", "N"), _unary_bwd("devo_lie_inv_backward", "N", "N", "N")
mul, mul_backward = _binary("devo_lie_mul", "N", "N"), _binary_bwd("devo_lie_mul_backward", "N", "N")
adj, adj_backward = _binary("devo_lie_adj", "K", "K"), _binary_bwd("devo_lie_adj_backward", "K", "K")
adjT, adjT_backward = _binary("devo_lie_adjT", "K", "K"), _binary_bwd("devo_lie_adjT_backward", "K", "K")
act, act_backward = _binary("devo_lie_act", 3, 3), _binary_bwd("devo_lie_act_backward", 3, 3)
act4, act4_backward = _binary("devo_lie_act4", 4, 4), _binary_bwd("devo_lie_act4_backward", 4, 4)
Jinv = _binary("devo_lie_jinv", "K", "K")


def as_matrix(group_id, X):
    _chk(group_id, (X, "N"))
    n = X.shape[0]
    out = torch.empty(n, 4, 4, dtype=X.dtype, device=X.device)
    L.check(L.lib().devo_lie_as_matrix(group_id, L.ptr(X), L.ptr(out), n, L.dtype_code(X), L.stream()), "devo_lie_as_matrix")
    return out


def projector(group_id, X):
    """[n, N, N]: d(embedded coordinates) / d(left perturbation), last column zero — what ToVec / FromVec differentiate through."""
    N, _ = _chk(group_id, (X, "N"))
    n = X.shape[0]
    out = torch.empty(n, N, N, dtype=X.dtype, device=X.device)
    L.check(L.lib().devo_lie_projector(group_id, L.ptr(X), L.ptr(out), n, L.dtype_code(X), L.stream()), "devo_lie_projector")
    return out


# The compiled binding (devo_amd._C.lietorch_backends: the same 19 functions taking torch::Tensor) replaces the ctypes forms above when present.
from . import native as _native_binding
_N = _native_binding()
if _N is not None:
    for _name in ("expm", "logm", "inv", "mul", "adj", "adjT", "act", "act4"):
        globals()[_name] = getattr(_N.lietorch_backends, _name)
        globals()[_name + "_backward"] = getattr(_N.lietorch_backends, _name + "_backward")
    as_matrix, Jinv, projector = _N.lietorch_backends.as_matrix, _N.lietorch_backends.Jinv, _N.lietorch_backends.projector
