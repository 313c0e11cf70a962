"""Numpy / Python fp64 restatement of the event simulator, written from the model's text (include/devo_hip.h, devo_amd/simulate.py) with
scalar loops: the shapes of the tests are tiny.  Python floats are IEEE doubles and every operation below rounds once, in the order the
model states, so the device's output is compared with `==`, not with a tolerance.

Per pixel: ref (fp64), last_t (int64, NO_EVENT = none yet).  Per frame pair (i0, i1 fp32 widened; t0 < t1 int64 ns; dt = t1 - t0):
  d = i1 - ref;  d >= 0: pol +1, C = C_pos, n = floor(d / C);  else pol -1, C = C_neg, n = floor(-d / C)
  k = 1..n:  L_k = ref + pol * (k * C);  f = (L_k - i0) / (i1 - i0) clamped to [0, 1] (1 when i1 == i0);  t_k = t0 + floor(f * dt)
             emitted iff last_t is none or t_k - last_t >= refractory_ns; then last_t = t_k
  ref = L_n when n > 0.
A call's events are ordered by (t, y * W + x, p), -1 before +1."""
import math

import numpy as np

NO_EVENT = -(1 << 63)


def log_intensity(img_u8):
    """scripts/convert_tartan.py:244 of the reference"""
    return np.log(np.asarray(img_u8, dtype=np.uint8).astype("float32") / 255 + 1e-5)


class ESIM:
    def __init__(self, contrast_threshold_neg=0.2, contrast_threshold_pos=0.2, refractory_period_ns=0):
        self.cn, self.cp, self.refr = float(contrast_threshold_neg), float(contrast_threshold_pos), int(refractory_period_ns)
        self.reset()

    def reset(self):
        self.ref = self.last_t = self._prev = self._prev_t = None

    def _pair(self, i0s, i1s, t0, t1, out):
        dt = float(t1 - t0)
        assert t1 > t0
        H, W = i0s.shape
        for y in range(H):
            for x in range(W):
                i0, i1, ref, last = float(i0s[y, x]), float(i1s[y, x]), float(self.ref[y, x]), int(self.last_t[y, x])
                d = i1 - ref
                if d >= 0.0:
                    pol, C, n = 1, self.cp, math.floor(d / self.cp)
                else:
                    pol, C, n = -1, self.cn, math.floor(-d / self.cn)
                if n <= 0:
                    continue
                L = ref
                for k in range(1, n + 1):
                    L = ref + pol * (k * C)
                    if i1 == i0:
                        f = 1.0
                    else:
                        f = min(max((L - i0) / (i1 - i0), 0.0), 1.0)
                    t = t0 + int(math.floor(f * dt))
                    if last == NO_EVENT or t - last >= self.refr:
                        last = t
                        out.append((t, y * W + x, pol))
                self.ref[y, x] = L
                self.last_t[y, x] = last

    def forward(self, log_images, timestamps):
        frames = np.asarray(log_images, dtype=np.float32)
        frames = frames[None] if frames.ndim == 2 else frames
        stamps = [int(v) for v in np.asarray(timestamps).reshape(-1)]
        assert len(stamps) == len(frames)
        first = self.ref is None
        if first:
            self.ref = frames[0].astype(np.float64)
            self.last_t = np.full(frames[0].shape, NO_EVENT, dtype=np.int64)
            self._prev, self._prev_t = frames[0], stamps[0]
            frames, stamps = frames[1:], stamps[1:]
            if not len(frames):
                return None
        out = []
        for img, t in zip(frames, stamps):
            self._pair(self._prev, img, self._prev_t, t, out)
            self._prev, self._prev_t = img, t
        out.sort()
        W = frames[0].shape[1]
        ev = np.asarray(out, dtype=np.int64).reshape(-1, 3)
        return {"x": (ev[:, 1] % W).astype(np.int16), "y": (ev[:, 1] // W).astype(np.int16), "t": ev[:, 0].copy(), "p": ev[:, 2].astype(np.int8)}


def simulate_clip(frames, stamps, chunks=None, **kw):
    """the clip through a fresh ESIM in calls of the given sizes (None: one call) -> (concatenated events, ref, last_t)"""
    sim = ESIM(**kw)
    parts, a = [], 0
    for c in ([len(frames)] if chunks is None else chunks):
        ev = sim.forward(frames[a:a + c], stamps[a:a + c])
        a += c
        if ev is not None:
            parts.append(ev)
    assert a == len(frames)
    return {k: np.concatenate([e[k] for e in parts]) for k in "xytp"}, sim.ref, sim.last_t


def window_of(t, tss_imgs_ns):
    """the real-frame window (0 .. R-2) of an event at stamp t: window r-1 holds T[r-1] < t <= T[r]; the first window has no lower bound,
    the last no upper bound"""
    T = [int(v) for v in tss_imgs_ns]
    for r in range(1, len(T) - 1):
        if t <= T[r]:
            return r - 1
    return len(T) - 2


def window_bounds(tss_imgs_ns, t_base):
    """[t0, t1) in fp64 of every window for stamps taken relative to t_base: (a, b] of integers is [a + 1, b + 1)"""
    T = [int(v) - int(t_base) for v in tss_imgs_ns]
    t0 = [-math.inf] + [float(T[r - 1] + 1) for r in range(2, len(T))]
    t1 = [float(T[r] + 1) for r in range(1, len(T) - 1)] + [math.inf]
    return np.asarray(t0, dtype=np.float64), np.asarray(t1, dtype=np.float64)
