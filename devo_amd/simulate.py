"""Event simulation on the GPU over csrc/esim.hip: contrast-threshold events from frames, the stage that MAKES DEVO's training data.  The
reference's scripts/convert_tartan.py:198-297 does it with esim_torch.ESIM, a CUDA-only extension; this module is that simulator with the
same interface, the `np.log` in front of it and the voxelisation loop behind it.

The model (include/devo_hip.h states it operation by operation).  Every pixel keeps a reference level `ref` (fp64) and the stamp `last_t`
(int64) of its last emitted event, "none" at first.  For two consecutive frames with log-intensities i0, i1 and stamps t0 < t1:
d = i1 - ref decides the polarity and the threshold C (C_pos for d >= 0, C_neg otherwise); n = floor(|d| / C) levels L_k = ref +- k C are
crossed (a level reached exactly counts); level k is crossed at t_k = t0 + floor(f (t1 - t0)) with f = (L_k - i0) / (i1 - i0) clamped to
[0, 1] (1 when i1 == i0); the event is emitted iff the pixel has none yet or t_k - last_t >= refractory_period_ns; ref = L_n either way.
All of it is fp64 with single roundings in that order, on the device as in tests/esim_ref.py, so the two agree bit for bit on every input.

Deliberate choices: fp64 state; a "none" sentinel instead of esim_torch's last_t = 0 with a `t > 0` filter (which drops
true events at stamp 0); `>=` in the refractory test; and ONE reproducible total order of a call's events — (t, y W + x, p) with -1 before
+1 — where esim_torch sorts by t with an unstable sort.

Limits, refused with ValueError before any launch where the host can see them: frame sides 1 .. 32767 (int16 coordinates); a call's time
span (its last stamp minus the stamp of the frame before its first) below `max_span_ns(H, W)` = 2^(62 - bits of H W - 1) ns (the stamp
shares the 64-bit sort key with the pixel index: 2^43 ns = 2.4 h at 480 x 640); thresholds finite and >= 1e-3; refractory period >= 0.
Found on the device (RuntimeError, the state stays as it was): non-finite log-intensities, stamps on the device that do not increase or
exceed the span, and more than 2^20 levels crossed by one pixel in one frame pair.  No CPU fallback: CPU frames raise.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import backends

NO_EVENT = -(1 << 63)                     # DEVO_ESIM_NO_EVENT: `last_t` of a pixel that has emitted nothing
MIN_THRESHOLD = 1e-3                      # DEVO_ESIM_MIN_THRESHOLD
MAX_SIDE = 32767                          # DEVO_ESIM_MAX_SIDE
_STATUS = ((1, "a log-intensity is not finite"), (2, "the stamps on the device are not strictly increasing"),
           (4, "the call's time span reaches the limit of the sort key (max_span_ns)"),
           (8, "a pixel crosses more than 2^20 contrast levels in one frame pair"))


# ------------------------------------------------------------------------------------------------ host parts (no GPU, no library)
def log_table():
    """fp32 [256]: convert_tartan.py:244's `np.log(img.astype("float32") / 255 + 1e-5)` of every uint8 value, by that very expression"""
    return np.log(np.arange(256, dtype=np.uint8).astype("float32") / 255 + 1e-5)


def max_span_ns(H, W):
    """the largest time span one call may cover, exclusive: 2^(62 - b) ns with b = the bits of H W - 1 (at least 1)"""
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"simulate: frame size {H} x {W} (sides 1 .. {MAX_SIDE}: int16 coordinates)")
    return 1 << (62 - max(1, (H * W - 1).bit_length()))


def _host_stamps(v, what):
    """int / sequence / numpy / CPU tensor -> int64 numpy [n]"""
    if torch.is_tensor(v):
        v = v.detach().numpy()
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: stamps are integer nanoseconds, got dtype {a.dtype}")
    if a.dtype.kind == "u" and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"{what}: a stamp does not fit int64")
    return a.astype(np.int64).reshape(-1)


def window_bounds(tss_imgs_ns, t_base):
    """The real-frame windows of `frames_to_voxels` as `events.voxel_grids` takes them: stamps T[0..R-1] (int64 ns) and the base every event
    stamp is taken relative to -> (t0, t1) float64 [R - 1].  Window r = 1 .. R-1 holds the events with T[r-1] < t <= T[r]; the first has no
    lower and the last no upper bound (convert_tartan.py:262-318).  Stamps are integers, so (a, b] is [a + 1, b + 1): t0[r-1] = T[r-1] + 1
    - t_base, t1[r-1] = T[r] + 1 - t_base, -inf and +inf at the two ends.  The shift happens in int64, before anything becomes fp64."""
    T = _host_stamps(tss_imgs_ns, "window_bounds")
    if T.size < 2 or not (np.diff(T) > 0).all():
        raise ValueError("window_bounds: at least two strictly increasing real-frame stamps are needed")
    rel = T - np.int64(int(t_base)) + 1
    if np.abs(rel).max() >= 1 << 53:
        raise ValueError("window_bounds: a real-frame stamp lies 2^53 ns or more from t_base")
    t0, t1 = rel[:-1].astype(np.float64), rel[1:].astype(np.float64)
    t0[0], t1[-1] = -np.inf, np.inf
    return t0, t1


# ------------------------------------------------------------------------------------------------ log intensity
_tables = {}                              # device -> the table on it


def log_intensity(frames_uint8):
    """uint8 frames of any shape on the GPU -> fp32 `np.log(frames.astype("float32") / 255 + 1e-5)`, bit for bit: a gather from the 256
    values numpy computes on the host (a device logf is not numpy's)."""
    if not torch.is_tensor(frames_uint8) or frames_uint8.dtype != torch.uint8:
        raise ValueError("log_intensity: a uint8 tensor is expected")
    if not frames_uint8.is_cuda:
        raise ValueError("log_intensity: frames must live on the GPU (the HIP path has no CPU fallback)")
    img = frames_uint8.contiguous()
    table = _tables.get(img.device)
    if table is None:
        table = _tables[img.device] = torch.from_numpy(log_table()).to(img.device)
    nat = backends.native()
    if nat is not None:
        return nat.simulate.log_intensity(img, table)
    with torch.cuda.device(img.device):
        out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
        L.check(L.lib().devo_log_intensity(L.ptr(img), img.numel(), L.ptr(table), L.ptr(out), L.stream()), "simulate.log_intensity")
    return out


def clear_cache():
    """drop the log tables kept on the devices"""
    _tables.clear()


# ------------------------------------------------------------------------------------------------ the simulator
def _count(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr):
    nat = backends.native()
    if nat is not None:
        return nat.simulate.count(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr)
    T, H, W = frames.shape
    counts = torch.empty(H * W, dtype=torch.int64, device=frames.device)
    status_span = torch.empty(2, dtype=torch.int64, device=frames.device)
    rc = L.lib().devo_esim_count(L.ptr(prev), L.ptr(frames), L.ptr(prev_stamp), L.ptr(stamps), T, H, W, L.ptr(ref), L.ptr(last), cn, cp, refr, L.ptr(counts),
                                 L.ptr(status_span), L.stream())
    L.check(rc, "simulate.count")
    return counts, status_span


def _emit(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr, offsets, total):
    nat = backends.native()
    if nat is not None:
        return nat.simulate.emit(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr, offsets, total)
    T, H, W = frames.shape
    keys = torch.empty(total, dtype=torch.int64, device=frames.device)
    ref_out, last_out = torch.empty_like(ref), torch.empty_like(last)
    rc = L.lib().devo_esim_emit(L.ptr(prev), L.ptr(frames), L.ptr(prev_stamp), L.ptr(stamps), T, H, W, L.ptr(ref), L.ptr(last), cn, cp, refr, L.ptr(offsets), total,
                                L.ptr(keys) if total else None, L.ptr(ref_out), L.ptr(last_out), L.stream())
    L.check(rc, "simulate.emit")
    return keys, ref_out, last_out


def _sort(keys, H, W, span):
    nat = backends.native()
    if nat is not None:
        return nat.simulate.sort(keys, H, W, span)
    n, h = keys.numel(), L.lib()
    out = torch.empty_like(keys)
    if n:
        ws = torch.empty(h.devo_esim_sort_workspace_bytes(n, H, W, span), dtype=torch.uint8, device=keys.device)
        L.check(h.devo_esim_sort_keys(L.ptr(keys), L.ptr(out), n, H, W, span, L.ptr(ws) if ws.numel() else None, ws.numel(), L.stream()), "simulate.sort")
    return out


def _decode(keys, H, W, first_stamp):
    nat = backends.native()
    if nat is not None:
        return nat.simulate.decode(keys, H, W, first_stamp)
    n, dev = keys.numel(), keys.device
    x, y = torch.empty(n, dtype=torch.int16, device=dev), torch.empty(n, dtype=torch.int16, device=dev)
    t, p = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    if n:
        L.check(L.lib().devo_esim_decode(L.ptr(keys), n, H, W, L.ptr(first_stamp), L.ptr(x), L.ptr(y), L.ptr(t), L.ptr(p), L.stream()), "simulate.decode")
    return x, y, t, p


class ESIM:
    """esim_torch.ESIM on the GPU.  `forward(log_images, timestamps)` takes fp32 log-intensity frames [H, W] or [T, H, W] on the GPU and their
    int64 nanosecond stamps (a 0-d / [T] tensor on either side, an int, a sequence or numpy) and returns None while no frame pair is
    available (the very first frame), else {"x": int16 [N], "y": int16 [N], "t": int64 [N], "p": int8 [N] in {-1, +1}} on the device, in
    the order (t, y W + x, p).  The first frame seen sets `ref`; the last frame and stamp of every call are kept and prepended to the next,
    so a clip fed in calls of any sizes gives the events of one call, call by call, and the same final `ref` and `last_t`.  (The events of
    one call are sorted together: where a crossing lands EXACTLY on the stamp that ends one call and a crossing of the next call's first
    pair lands on that same stamp, one call orders them by pixel and two calls by call.)  A call that raises leaves the state untouched."""

    def __init__(self, contrast_threshold_neg=0.2, contrast_threshold_pos=0.2, refractory_period_ns=0):
        cn, cp = float(contrast_threshold_neg), float(contrast_threshold_pos)
        if not (math.isfinite(cn) and math.isfinite(cp) and cn >= MIN_THRESHOLD and cp >= MIN_THRESHOLD):
            raise ValueError(f"ESIM: contrast thresholds must be finite and at least {MIN_THRESHOLD} (got {cn}, {cp})")
        if int(refractory_period_ns) != refractory_period_ns or refractory_period_ns < 0 or refractory_period_ns >= 1 << 63:
            raise ValueError(f"ESIM: refractory_period_ns must be a non-negative integer (got {refractory_period_ns!r})")
        self.contrast_threshold_neg, self.contrast_threshold_pos, self.refractory_period_ns = cn, cp, int(refractory_period_ns)
        self.reset()

    def reset(self):
        """forget every frame seen: the next frame sets `ref` again and produces no event"""
        self._ref = self._last = self._prev = self._prev_stamp = None
        self._prev_host = None           # the kept stamp as an int where the host has seen it

    @property
    def ref(self):
        """fp64 [H, W]: a copy of the reference levels (None before the first frame)"""
        return None if self._ref is None else self._ref.clone()

    @property
    def last_t(self):
        """int64 [H, W]: a copy of the stamps of each pixel's last emitted event, NO_EVENT where it has none (None before the first frame)"""
        return None if self._last is None else self._last.clone()

    def _stamps(self, timestamps, T, H, W, device):
        """-> (int64 [T] on the device, the last stamp as an int or None); everything the host can see is checked here"""
        if torch.is_tensor(timestamps) and timestamps.is_cuda:
            if timestamps.dtype != torch.int64 or timestamps.numel() != T or timestamps.device != device:
                raise ValueError(f"ESIM.forward: timestamps must be {T} int64 nanosecond stamps on the frames' GPU")
            return timestamps.reshape(-1).contiguous(), None
        ts = _host_stamps(timestamps, "ESIM.forward")
        if ts.size != T:
            raise ValueError(f"ESIM.forward: {T} frames but {ts.size} stamps")
        seen = ts if self._prev_host is None else np.concatenate([np.asarray([self._prev_host], dtype=np.int64), ts])
        if not all(int(b) > int(a) for a, b in zip(seen[:-1], seen[1:])):
            raise ValueError("ESIM.forward: stamps must be strictly increasing (also across calls)")
        if int(seen[-1]) - int(seen[0]) >= max_span_ns(H, W):
            raise ValueError(f"ESIM.forward: the call spans {int(seen[-1]) - int(seen[0])} ns, the limit at {H} x {W} is {max_span_ns(H, W)} ns: feed it in shorter calls")
        return torch.from_numpy(ts).to(device), int(ts[-1])

    def forward(self, log_images, timestamps):
        if not torch.is_tensor(log_images):
            raise ValueError("ESIM.forward: log_images must be a tensor")
        if not log_images.is_cuda:
            raise ValueError("ESIM.forward: log_images must live on the GPU (the HIP path has no CPU fallback)")
        if log_images.dtype != torch.float32 or log_images.dim() not in (2, 3) or log_images.numel() == 0:
            raise ValueError("ESIM.forward: log_images must be float32 [H, W] or [T, H, W]")
        frames = (log_images if log_images.dim() == 3 else log_images.unsqueeze(0)).contiguous()
        T, H, W = frames.shape
        max_span_ns(H, W)                                             # (refuses the frame size)
        if self._ref is not None and (tuple(self._ref.shape) != (H, W) or self._ref.device != frames.device):
            raise ValueError(f"ESIM.forward: frames are {H} x {W} on {frames.device}, the state is {tuple(self._ref.shape)} on {self._ref.device} (reset() starts anew)")
        with torch.cuda.device(frames.device):
            stamps, last_host = self._stamps(timestamps, T, H, W, frames.device)
            if self._ref is None:                                     # the first frame sets ref and pairs with the rest of the call
                ref, last = frames[0].double(), torch.full((H, W), NO_EVENT, dtype=torch.int64, device=frames.device)
                prev, prev_stamp, frames, stamps = frames[0], stamps[:1], frames[1:], stamps[1:]
            else:
                ref, last, prev, prev_stamp = self._ref, self._last, self._prev, self._prev_stamp
            events = None
            if frames.shape[0]:
                events, ref, last = self._pairs(prev, frames, prev_stamp, stamps, ref, last)
                prev, prev_stamp = frames[-1], stamps[-1:]
            self._ref, self._last, self._prev, self._prev_stamp, self._prev_host = ref, last, prev.clone(), prev_stamp.clone(), last_host
        return events

    __call__ = forward

    def _pairs(self, prev, frames, prev_stamp, stamps, ref, last):
        """the call's frame pairs -> (events, new ref, new last_t); nothing of self changes here"""
        H, W = frames.shape[1:]
        cn, cp, refr = self.contrast_threshold_neg, self.contrast_threshold_pos, self.refractory_period_ns
        counts, status_span = _count(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr)
        offsets = torch.cumsum(counts, 0)                             # inclusive: pixel i writes at [offsets[i - 1], offsets[i])
        total, status, span = torch.cat((offsets[-1:], status_span)).tolist()      # the call's one read-back: it sizes the output (and the sort's bit range)
        if status:
            raise RuntimeError("ESIM.forward: " + "; ".join(msg for bit, msg in _STATUS if status & bit) + " (the simulator's state is unchanged)")
        if total == 0:                                                # no level crossed anywhere: ref and last_t stay
            x, y, t, p = _decode(torch.empty(0, dtype=torch.int64, device=frames.device), H, W, prev_stamp)
            return {"x": x, "y": y, "t": t, "p": p}, ref, last
        keys, ref, last = _emit(prev, frames, prev_stamp, stamps, ref, last, cn, cp, refr, offsets, total)
        x, y, t, p = _decode(_sort(keys, H, W, span), H, W, prev_stamp)
        return {"x": x, "y": y, "t": t, "p": p}, ref, last


# ------------------------------------------------------------------------------------------------ clip -> voxel grids
def frames_to_voxels(sim, log_images, tss_ns, tss_imgs_ns, bins=5, frames_per_call=None):
    """The loop of convert_tartan.py:242-318 for a clip held in memory: `sim` (reset first) runs over the simulator frames `log_images`
    [T, H, W] with stamps `tss_ns` [T]; the events are cut at the real frames' stamps `tss_imgs_ns` [R] (host values) into R - 1 windows —
    t <= T[1] for the first, T[r-1] < t <= T[r] in between, everything after T[R-2] for the last — and every window becomes one voxel
    grid by `events.voxel_grids` (integer coordinates, no map).  Stamps are taken relative to the first simulator stamp in int64 before
    they become fp64, so epoch-sized stamps stay exact.  `frames_per_call` only splits the simulator calls (None: one call).
    -> (grids [R - 1, bins, H, W] fp32, counts int64 [R - 1]) on the device."""
    from . import events as E
    if not isinstance(sim, ESIM):
        raise TypeError("frames_to_voxels: sim must be a simulate.ESIM")
    if not torch.is_tensor(log_images) or log_images.dim() != 3 or log_images.shape[0] < 2:
        raise ValueError("frames_to_voxels: log_images must be [T, H, W] with at least two frames")
    T, H, W = log_images.shape
    step = T if frames_per_call is None else int(frames_per_call)
    if step < 1:
        raise ValueError(f"frames_to_voxels: frames_per_call {frames_per_call!r}")
    on_device = torch.is_tensor(tss_ns) and tss_ns.is_cuda
    stamps = tss_ns.reshape(-1) if on_device else _host_stamps(tss_ns, "frames_to_voxels")
    if len(stamps) != T:
        raise ValueError(f"frames_to_voxels: {T} frames but {len(stamps)} stamps")
    t_base = int(stamps[0])
    t0, t1 = window_bounds(tss_imgs_ns.cpu() if torch.is_tensor(tss_imgs_ns) else tss_imgs_ns, t_base)
    sim.reset()
    parts = []
    for a in range(0, T, step):
        ev = sim.forward(log_images[a:a + step], stamps[a:a + step])
        if ev is not None:
            parts.append(ev)
    x, y, t, p = (torch.cat([ev[k] for ev in parts]) for k in "xytp")
    return E.voxel_grids(x, y, (t - t_base).double(), p, t0, t1, H, W, bins=bins)
