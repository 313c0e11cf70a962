"""Lie group types + autograd ops over the HIP kernels — the host-side mirror of the reference's Python lietorch layer
(devo/lietorch/groups.py:51-323 LieGroup / SO3 / RxSO3 / SE3 / Sim3 / cat / stack, group_ops.py:7-101 GroupOp, the op classes and
ToVec / FromVec, broadcasting.py:9-31).  LieGroupParameter and quaternion() (which names an op the reference does not define) are left out.

Same call conventions as the reference: data[..., N] per group (SO3 q_xyzw; RxSO3 q, s; SE3 t, q; Sim3 t, q, s); gradients of group
elements are K-vectors in the first K of the N slots; binary ops broadcast leading dimensions; `retr(a) = Exp(a) * X`.
"""
import numpy as np
import torch
from .backends import lietorch_backends as _be


class _GroupOp(torch.autograd.Function):
    """group_ops.py:7-25: save inputs, call the forward kernel; backward calls the matching *_backward.  The class carries the group id
    (the reference passes it through apply)."""
    fwd = bwd = None
    gid = 3

    @classmethod
    def forward(cls, ctx, *inputs):
        ctx.save_for_backward(*inputs)
        return cls.fwd(cls.gid, *inputs)

    @classmethod
    def backward(cls, ctx, grad):
        if cls.bwd is None:
            raise RuntimeError(f"Backward operation not implemented for {cls}")
        return tuple(cls.bwd(cls.gid, grad.contiguous(), *ctx.saved_tensors))


class _FromVec(torch.autograd.Function):
    """group_ops.py:73-86: the embedded coordinates as a group element; grad (a tangent in K of N slots) -> grad * pinv(J), J = projector."""
    gid = 3

    @classmethod
    def forward(cls, ctx, x):
        ctx.save_for_backward(x)
        return x.view_as(x)

    @classmethod
    def backward(cls, ctx, grad):
        J = _be.projector(cls.gid, *ctx.saved_tensors)
        return torch.matmul(grad.unsqueeze(-2), torch.linalg.pinv(J)).squeeze(-2)


class _ToVec(_FromVec):
    """group_ops.py:88-101: a group element as its embedded coordinates; grad -> grad * J."""

    @classmethod
    def backward(cls, ctx, grad):
        J = _be.projector(cls.gid, *ctx.saved_tensors)
        return torch.matmul(grad.unsqueeze(-2), J).squeeze(-2)


_OP_TABLE = (("Exp", _be.expm, _be.expm_backward), ("Log", _be.logm, _be.logm_backward), ("Inv", _be.inv, _be.inv_backward),
             ("Mul", _be.mul, _be.mul_backward), ("Adj", _be.adj, _be.adj_backward), ("AdjT", _be.adjT, _be.adjT_backward),
             ("Act3", _be.act, _be.act_backward), ("Act4", _be.act4, _be.act4_backward), ("Jinv", _be.Jinv, None),
             ("ToMatrix", _be.as_matrix, None))


class _Ops:
    """The op classes of one group."""

    def __init__(self, gid, name):
        for op, fwd, bwd in _OP_TABLE:
            setattr(self, op, type(f"{op}_{name}", (_GroupOp,), {"fwd": staticmethod(fwd), "bwd": staticmethod(bwd) if bwd else None, "gid": gid}))
        self.ToVec = type(f"ToVec_{name}", (_ToVec,), {"gid": gid})
        self.FromVec = type(f"FromVec_{name}", (_FromVec,), {"gid": gid})


_OPS = {gid: _Ops(gid, name) for gid, name in ((1, "SO3"), (2, "RxSO3"), (3, "SE3"), (4, "Sim3"))}
# SE3's op classes under the names this module always had
Exp, Log, Inv, Mul, Adj, AdjT, Act3, Act4, Jinv, ToMatrix = (getattr(_OPS[3], n) for n, _, _ in _OP_TABLE)


def broadcast_inputs(x, y):
    """broadcasting.py:9-31: flatten to [batch, dim] contiguous, broadcasting size-1 leading dims."""
    if y is None:
        return (x.reshape(-1, x.shape[-1]).contiguous(),), tuple(x.shape[:-1])
    if x.dim() != y.dim():
        raise AssertionError("lietorch: operands must have the same number of dimensions")
    xs, ys = x.shape[:-1], y.shape[:-1]
    for n, m in zip(xs, ys):
        if not (n == m or n == 1 or m == 1):
            raise AssertionError(f"lietorch: shapes {tuple(xs)} and {tuple(ys)} do not broadcast")
    out = tuple(max(n, m) for n, m in zip(xs, ys))
    x1 = x.expand(*out, x.shape[-1]).reshape(-1, x.shape[-1]).contiguous()
    y1 = y.expand(*out, y.shape[-1]).reshape(-1, y.shape[-1]).contiguous()
    return (x1, y1), out


def _apply(op, x, y=None):
    inputs, shape = broadcast_inputs(x, y)
    return op.apply(*inputs).view(shape + (-1,))


class LieGroup:
    """groups.py:51-233.  Subclasses set group_name, group_id, manifold_dim, embedded_dim, id_elem."""
    group_name = None
    group_id = None

    def __init__(self, data):
        self.data = data

    def __repr__(self):
        return f"{self.group_name}: size={tuple(self.shape)}, device={self.device}, dtype={self.dtype}"

    shape = property(lambda self: self.data.shape[:-1])
    device = property(lambda self: self.data.device)
    dtype = property(lambda self: self.data.dtype)
    tangent_shape = property(lambda self: self.data.shape[:-1] + (self.manifold_dim,))

    @classmethod
    def _ops(cls):
        return _OPS[cls.group_id]

    # ---- constructors
    @classmethod
    def Identity(cls, *batch_shape, **kwargs):
        if isinstance(batch_shape[0], (tuple, list, torch.Size)):
            batch_shape = tuple(batch_shape[0])
        data = cls.id_elem.to(**kwargs).repeat(int(np.prod(batch_shape)), 1)
        return cls(data.view(tuple(batch_shape) + (cls.embedded_dim,)))

    @classmethod
    def IdentityLike(cls, G):
        return cls.Identity(G.shape, device=G.data.device, dtype=G.data.dtype)

    @classmethod
    def InitFromVec(cls, data):
        return cls(_apply(cls._ops().FromVec, data))

    @classmethod
    def Random(cls, *batch_shape, sigma=1.0, **kwargs):
        if isinstance(batch_shape[0], (tuple, list, torch.Size)):
            batch_shape = tuple(batch_shape[0])
        return cls.exp(sigma * torch.randn(tuple(batch_shape) + (cls.manifold_dim,), **kwargs))

    @classmethod
    def exp(cls, a):
        return cls(_apply(cls._ops().Exp, a))

    # ---- group operations
    def vec(self):
        return _apply(self._ops().ToVec, self.data)

    def log(self):
        return _apply(self._ops().Log, self.data)

    def inv(self):
        return self.__class__(_apply(self._ops().Inv, self.data))

    def mul(self, other):
        return self.__class__(_apply(self._ops().Mul, self.data, other.data))

    def retr(self, a):
        ops = self._ops()
        return self.__class__(_apply(ops.Mul, _apply(ops.Exp, a), self.data))

    def adj(self, a):
        return _apply(self._ops().Adj, self.data, a)

    def adjT(self, a):
        return _apply(self._ops().AdjT, self.data, a)

    def Jinv(self, a):
        return _apply(self._ops().Jinv, self.data, a)

    def act(self, p):
        if p.shape[-1] == 3:
            return _apply(self._ops().Act3, self.data, p)
        if p.shape[-1] == 4:
            return _apply(self._ops().Act4, self.data, p)
        raise RuntimeError(f"{self.group_name}.act: points must have 3 or 4 components")

    def matrix(self):
        """4x4 matrices, via the action on the identity like the reference (groups.py:180-184)."""
        I = torch.eye(4, dtype=self.dtype, device=self.device).view([1] * (self.data.dim() - 1) + [4, 4])
        return self.__class__(self.data[..., None, :]).act(I).transpose(-1, -2)

    def translation(self):
        p = torch.eye(4, dtype=self.dtype, device=self.device)[3]               # (made on the device: a list -> GPU tensor is a blocking copy)
        return _apply(self._ops().Act4, self.data, p.view([1] * (self.data.dim() - 1) + [4]))

    def __mul__(self, other):
        if isinstance(other, LieGroup):
            return self.mul(other)
        if isinstance(other, torch.Tensor):
            return self.act(other)
        return NotImplemented

    # ---- tensor-like plumbing
    def __getitem__(self, index):
        return self.__class__(self.data[index])

    def __setitem__(self, index, item):
        self.data[index] = item.data

    def detach(self):
        return self.__class__(self.data.detach())

    def view(self, dims):
        return self.__class__(self.data.view(tuple(dims) + (self.embedded_dim,)))

    def to(self, *args, **kwargs):
        return self.__class__(self.data.to(*args, **kwargs))

    def cpu(self):
        return self.__class__(self.data.cpu())

    def cuda(self):
        return self.__class__(self.data.cuda())

    def float(self):
        return self.__class__(self.data.float())

    def double(self):
        return self.__class__(self.data.double())

    def unbind(self, dim=0):
        return [self.__class__(x) for x in self.data.unbind(dim=dim)]


class SO3(LieGroup):
    """groups.py:234-247; SO3(SE3) takes the rotation."""
    group_name = "SO3"
    group_id = 1
    manifold_dim = 3
    embedded_dim = 4
    id_elem = torch.as_tensor([0.0, 0.0, 0.0, 1.0])

    def __init__(self, data):
        if isinstance(data, SE3):
            data = data.data[..., 3:7]
        elif isinstance(data, SO3):
            data = data.data
        super().__init__(data)


class RxSO3(LieGroup):
    """groups.py:250-263; RxSO3(Sim3) takes rotation and scale."""
    group_name = "RxSO3"
    group_id = 2
    manifold_dim = 4
    embedded_dim = 5
    id_elem = torch.as_tensor([0.0, 0.0, 0.0, 1.0, 1.0])

    def __init__(self, data):
        if isinstance(data, Sim3):
            data = data.data[..., 3:8]
        elif isinstance(data, RxSO3):
            data = data.data
        super().__init__(data)


class SE3(LieGroup):
    """groups.py:266-285; SE3(SO3) has zero translation."""
    group_name = "SE3"
    group_id = 3
    manifold_dim = 6
    embedded_dim = 7
    id_elem = torch.as_tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])

    def __init__(self, data):
        if isinstance(data, SO3):
            data = torch.cat([torch.zeros_like(data.data[..., :3]), data.data], -1)
        elif isinstance(data, SE3):
            data = data.data
        self.data = data

    def scale(self, s):
        t, q = self.data.split([3, 4], -1)
        return SE3(torch.cat([t * s.unsqueeze(-1), q], dim=-1))


class Sim3(LieGroup):
    """groups.py:288-311.  Sim3(SO3) is done as intended (zero translation, unit scale): groups.py:299-302 reads a class attribute instead
    of its argument and cannot work."""
    group_name = "Sim3"
    group_id = 4
    manifold_dim = 7
    embedded_dim = 8
    id_elem = torch.as_tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0])

    def __init__(self, data):
        if isinstance(data, SO3):
            q = data.data
            data = torch.cat([torch.zeros_like(q[..., :3]), q, torch.ones_like(q[..., :1])], -1)
        elif isinstance(data, SE3):
            data = torch.cat([data.data, torch.ones_like(data.data[..., :1])], -1)
        elif isinstance(data, Sim3):
            data = data.data
        super().__init__(data)


def cat(group_list, dim):
    return group_list[0].__class__(torch.cat([X.data for X in group_list], dim=dim))


def stack(group_list, dim):
    return group_list[0].__class__(torch.stack([X.data for X in group_list], dim=dim))
