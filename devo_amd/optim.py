"""The optimiser step on the GPU over csrc/optim.hip: gradient-norm clip + AdamW in two launches, the last three lines of the reference's
training loop (train.py:248-250: `clip_grad_norm_(10)` -> `AdamW.step()` -> `OneCycleLR.step()`) and its checkpoints (train.py:133-136, 271-280).

`AdamW` is a `torch.optim.Optimizer`: `param_groups[0]["lr"]` is read at every step, so the reference's own
`torch.optim.lr_scheduler.OneCycleLR(optimizer, lr, steps, pct_start=0.01, cycle_momentum=False, anneal_strategy='linear')` (`one_cycle`
below) drives it unchanged, on the host.  `step()` launches the norm and the update (include/devo_hip.h states both operation by
operation); `grad_norm` is the 0-d fp64 device tensor of the last step, what `clip_grad_norm_` returns, and nothing is read back.
`state_dict()` / `load_state_dict()` speak `torch.optim.AdamW`'s format: a checkpoint written by either resumes in the other.

How a step reaches the device.  The chunk table, the parameter addresses and the moment offsets are fixed and uploaded at construction.  The
gradient addresses change every step (autograd allocates anew after `zero_grad(set_to_none=True)`): they travel as kernel arguments, so a
step may be enqueued before the one before it has run, and everything launches on torch's current stream, whose allocator ordering covers the
gradients' lifetime.

Deviations from the reference: `.grad` is left unclipped (the clipped gradient exists in registers only); there is ONE
step count for all tensors (torch counts per parameter: a state whose counts differ is refused); the step is not capturable in a HIP
graph (its host-computed scalars and the gradient addresses are arguments).

Refused with ValueError naming the parameter, before any launch: CPU tensors (no CPU path), parameters or gradients that are not fp32, sparse
gradients, more than one parameter group, amsgrad, maximize, a closure, a parameter that is not non-overlapping and dense, a gradient whose
strides differ from its parameter's (channels-last weights with like-strided gradients are the normal case and work), and data or gradient
addresses that are not 16-byte aligned.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import backends

CHUNK = 2048                              # DEVO_OPTIM_CHUNK
MAX_TENSORS = 4096                        # DEVO_OPTIM_MAX_TENSORS


# ------------------------------------------------------------------------------------------------ host parts (no GPU)
def one_cycle(optimizer, max_lr, total_steps):
    """train.py:110-111: the reference's schedule, torch's own (host arithmetic only).  total_steps below 200 makes torch divide by zero
    (pct_start = 0.01 of it, minus one)."""
    if int(total_steps) < 200:
        raise ValueError(f"one_cycle: total_steps {total_steps} (at least 200: the warm-up is 1 % of it)")
    return torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr, int(total_steps), pct_start=0.01, cycle_momentum=False, anneal_strategy="linear")


def _dense(sizes, strides):
    """non-overlapping and dense: some permutation of a contiguous layout (dimensions of size 1 carry no layout)"""
    dims = sorted((st, sz) for sz, st in zip(sizes, strides) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


def _same_layout(sizes, a, b):
    return all(sz == 1 or x == y for sz, x, y in zip(sizes, a, b))


def _plan(numel):
    """-> (chunk table int32 [chunks, 4], moment offsets int64 [n], elements of a moment buffer), host tensors"""
    nat = backends.native()
    if nat is not None:
        table, offs, elems = nat.optim.plan(list(numel))
        return table, offs, int(elems)
    h, n = L.lib(), len(numel)
    arr = L.i64arr(numel)
    chunks, elems = h.devo_optim_chunks(arr, n), h.devo_optim_moment_elems(arr, n)
    if chunks <= 0:
        L.check(1, "optim.plan")
    table, offs = np.empty((chunks, 4), dtype=np.int32), np.empty(n, dtype=np.int64)
    L.check(h.devo_optim_plan(arr, n, table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "optim.plan")
    return torch.from_numpy(table), torch.from_numpy(offs), int(elems)


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW with `clip_grad_norm_(params, max_norm)` in front of it (max_norm None: no clipping; the norm is computed either
    way), as two launches.  `names` (optional, one per parameter) only serve the error messages.

    skip_nonfinite: a step whose gradient norm is inf or NaN writes nothing to the parameters or moments; two int64 device counters
    (`counters()` -> (applied, skipped), one copy on demand) advance instead, and the bias correction uses the device's applied count.  Off
    (the default), non-finite values propagate as in torch."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=False, amsgrad=False, maximize=False, names=None):
        if amsgrad or maximize:
            raise ValueError("optim.AdamW: amsgrad and maximize are not implemented")
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError(f"optim.AdamW: {len(params)} parameter groups (one is supported)")
            params = [dict(params[0], params=list(params[0]["params"]))]
            plist = params[0]["params"]
        else:
            plist = params
        lr, eps, weight_decay = float(lr), float(eps), float(weight_decay)
        b1, b2 = float(betas[0]), float(betas[1])
        if not (math.isfinite(lr) and lr >= 0 and math.isfinite(eps) and eps >= 0 and math.isfinite(weight_decay) and weight_decay >= 0 and 0 <= b1 < 1 and 0 <= b2 < 1):
            raise ValueError(f"optim.AdamW: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        if max_norm is not None and not (float(max_norm) > 0):
            raise ValueError(f"optim.AdamW: max_norm {max_norm!r} (a positive number, inf included, or None)")
        if not plist:
            raise ValueError("optim.AdamW: no parameters")
        if len(plist) > MAX_TENSORS:
            raise ValueError(f"optim.AdamW: {len(plist)} parameters (at most {MAX_TENSORS})")
        self._names = [str(n) for n in names] if names is not None else [f"#{i}" for i in range(len(plist))]
        if len(self._names) != len(plist):
            raise ValueError(f"optim.AdamW: {len(self._names)} names for {len(plist)} parameters")
        for i, p in enumerate(plist):
            self._check_param(i, p, plist[0])
        # the keys torch.optim.AdamW writes into a checkpoint's param_groups, with its own defaults (a host-only instance gives them)
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay).defaults)
        self._built = False
        super().__init__(params, defaults)
        self._built = True
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._params = plist
        self._device = dev = plist[0].device
        self._numel = [p.numel() for p in plist]
        self._strides = [p.stride() for p in plist]
        self._addr = [p.data_ptr() for p in plist]
        self._t = 0                                           # steps taken (with skip_nonfinite the device's `applied` count rules)
        with torch.cuda.device(dev):
            table, offs, elems = _plan(self._numel)
            self._offsets = offs.tolist()
            self._n_chunks = int(table.shape[0])
            self._chunks = table.to(dev)
            self._tensors = torch.stack([torch.tensor(self._addr, dtype=torch.int64), offs], 1).contiguous().to(dev)
            self._m = torch.zeros(elems, dtype=torch.float32, device=dev)
            self._v = torch.zeros(elems, dtype=torch.float32, device=dev)
            self._counters = torch.zeros(2, dtype=torch.int64, device=dev)
            self._norm = torch.zeros((), dtype=torch.float64, device=dev)
            nat = backends.native()
            ws = nat.optim.workspace_bytes() if nat is not None else L.lib().devo_optim_workspace_bytes()
            self._ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        self._numel_c = L.i64arr(self._numel)                 # (the ctypes leg's)
        self._grads_c = (ctypes.c_void_p * len(plist))()

    # ---------------------------------------------------------------------------------------------- checks
    def _name(self, i):
        return f"parameter {self._names[i]} {tuple(self._params[i].shape)}"

    def _check_param(self, i, p, first):
        name = f"parameter {self._names[i]}"
        if not torch.is_tensor(p):
            raise ValueError(f"optim.AdamW: {name} is not a tensor")
        name += f" {tuple(p.shape)}"
        if not p.is_cuda:
            raise ValueError(f"optim.AdamW: {name} lives on the CPU (the HIP path has no CPU fallback)")
        if p.device != first.device:
            raise ValueError(f"optim.AdamW: {name} is on {p.device}, the first parameter on {first.device}")
        if p.dtype != torch.float32:
            raise ValueError(f"optim.AdamW: {name} is {p.dtype} (float32 only)")
        if p.layout != torch.strided or not _dense(p.shape, p.stride()):
            raise ValueError(f"optim.AdamW: {name} with strides {p.stride()} is not non-overlapping and dense")
        if not 1 <= p.numel() < 1 << 31:
            raise ValueError(f"optim.AdamW: {name} has {p.numel()} elements (1 .. 2^31 - 1)")
        if p.data_ptr() % 16:
            raise ValueError(f"optim.AdamW: the data of {name} is not 16-byte aligned")

    def add_param_group(self, param_group):
        if self._built or self.param_groups:
            raise ValueError("optim.AdamW: more than one parameter group")
        super().add_param_group(param_group)

    def _grad_addresses(self):
        """this step's gradient addresses (0: none), every refusal raised before anything is launched"""
        addrs = []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                addrs.append(0)
                continue
            if g.layout != torch.strided:
                raise ValueError(f"optim.AdamW: the gradient of {self._name(i)} is sparse ({g.layout})")
            if g.dtype != torch.float32:
                raise ValueError(f"optim.AdamW: the gradient of {self._name(i)} is {g.dtype} (float32 only)")
            if g.device != self._device:
                raise ValueError(f"optim.AdamW: the gradient of {self._name(i)} is on {g.device}, the parameter on {self._device}")
            if p.data_ptr() != self._addr[i] or p.stride() != self._strides[i]:
                raise ValueError(f"optim.AdamW: the storage of {self._name(i)} has changed since construction")
            if g.stride() != self._strides[i] and (g.shape != p.shape or not _same_layout(p.shape, g.stride(), self._strides[i])):
                raise ValueError(f"optim.AdamW: the gradient of {self._name(i)} has strides {g.stride()}, the parameter {self._strides[i]}")
            a = g.data_ptr()
            if a % 16:
                raise ValueError(f"optim.AdamW: the gradient of {self._name(i)} is not 16-byte aligned")
            addrs.append(a)
        return addrs

    # ---------------------------------------------------------------------------------------------- the step
    @property
    def grad_norm(self):
        """0-d fp64 device tensor: the gradient norm of the last step BEFORE clipping (what clip_grad_norm_ returns); rewritten by every step"""
        return self._norm

    def counters(self):
        """(applied, skipped) steps.  With skip_nonfinite they are the device's counters, read in one copy; without, every step is applied."""
        if not self.skip_nonfinite:
            return self._t, 0
        a, s = self._counters.tolist()
        return a, s

    def step(self, closure=None):
        if closure is not None:
            raise ValueError("optim.AdamW: a closure is not supported")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("optim.AdamW: amsgrad and maximize are not implemented")
        lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        addrs = self._grad_addresses()
        t = self._t + 1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        max_norm = -1.0 if self.max_norm is None else self.max_norm
        with torch.cuda.device(self._device):
            nat = backends.native()
            if nat is not None:
                nat.optim.step(self._chunks, self._tensors, addrs, self._numel, self._m, self._v, lr, b1, b2, eps, wd, max_norm, bc1, bc2, self.skip_nonfinite,
                               self._counters, self._norm, self._ws)
            else:
                gc = self._grads_c
                for i, a in enumerate(addrs):
                    gc[i] = a or None
                L.check(L.lib().devo_optim_step(L.ptr(self._chunks), self._n_chunks, L.ptr(self._tensors), gc, self._numel_c, len(addrs), L.ptr(self._m), L.ptr(self._v), lr,
                                                b1, b2, eps, wd, max_norm, bc1, bc2, int(self.skip_nonfinite), L.ptr(self._counters), L.ptr(self._norm), L.ptr(self._ws),
                                                self._ws.numel(), L.stream()), "optim.step")
        self._t = t
        return None

    # ---------------------------------------------------------------------------------------------- checkpoints
    def _moment_view(self, buf, i):
        p = self._params[i]
        return torch.as_strided(buf, p.shape, p.stride(), self._offsets[i])

    def state_dict(self):
        """torch.optim.AdamW's format: state[i] = {step (0-d fp32 host tensor), exp_avg, exp_avg_sq (copies, shaped and laid out like the
        parameter)}, param_groups = the group's keys with parameter indices.  Before the first step the state is empty, as torch's is."""
        t = self.counters()[0] if self.skip_nonfinite else self._t
        state = {}
        if t > 0:
            for i in range(len(self._params)):
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32), "exp_avg": self._moment_view(self._m, i).clone(),
                            "exp_avg_sq": self._moment_view(self._v, i).clone()}
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """A state_dict of this class or of torch.optim.AdamW over the same parameters in the same order (the reference's
        `optimizer_state_dict`).  The moments are copied into the flat buffers; parameters without an entry get zero moments."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"optim.AdamW.load_state_dict: {len(groups)} parameter groups (one is supported)")
        saved = groups[0]
        n = len(self._params)
        if len(saved["params"]) != n:
            raise ValueError(f"optim.AdamW.load_state_dict: the state has {len(saved['params'])} parameters, the optimiser {n}")
        if saved.get("amsgrad") or saved.get("maximize"):
            raise ValueError("optim.AdamW.load_state_dict: amsgrad and maximize are not implemented")
        state = {saved["params"].index(k) if k in saved["params"] else k: v for k, v in state_dict["state"].items()}
        steps = {i: int(round(float(s["step"]))) for i, s in state.items()}
        if len(set(steps.values())) > 1:
            odd = next(i for i, s in steps.items() if s != next(iter(steps.values())))
            raise ValueError(f"optim.AdamW.load_state_dict: the per-parameter step counts differ ({self._name(odd)} has {steps[odd]}, "
                             f"{self._name(next(iter(steps)))} {next(iter(steps.values()))}): this optimiser keeps one count")
        for i, s in state.items():
            for key in ("exp_avg", "exp_avg_sq"):
                if not 0 <= i < n or tuple(s[key].shape) != tuple(self._params[i].shape):
                    raise ValueError(f"optim.AdamW.load_state_dict: {key} of entry {i} does not match its parameter's shape")
        t = next(iter(steps.values())) if steps else 0
        with torch.cuda.device(self._device), torch.no_grad():
            self._m.zero_()
            self._v.zero_()
            for i, s in state.items():
                self._moment_view(self._m, i).copy_(s["exp_avg"])
                self._moment_view(self._v, i).copy_(s["exp_avg_sq"])
            self._counters[0] = t
        self._t = t
        for k, v in saved.items():
            if k != "params":
                self.param_groups[0][k] = v
