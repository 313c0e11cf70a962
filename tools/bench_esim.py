"""Event simulation per call: devo_amd.simulate.ESIM (csrc/esim.hip) against the same model composed from torch operations on the same GPU
and its vectorised numpy form on the host.

    python tools/bench_esim.py --out profiles/esim.txt          # the table
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_esim.py --profile 20     # a run of its own
    python tools/bench_esim.py --split DIR/.../k_kernel_stats.csv --calls-profiled 20 --append profiles/esim.txt    # the per-kernel split

The clip: 480 x 640, a smooth random texture that is periodic over 32 px and moves 2 px per simulator frame, so 16 frames are one period
and every call continues the one before; uint8 -> `simulate.log_intensity`; 16 simulator frames per call, 1 ms apart; C = 0.25 both ways,
no refractory period.  The event rate is printed with the table.  All three paths return the call's events in the order (t, pixel, p) and
are checked against each other before anything is timed.

The torch composition (here, not in the package): per frame pair n = floor(|i1 - ref| / C) as a tensor, one [max n, H W] grid of levels,
their stamps, a mask; the pairs' events as one int64 key each, one torch.sort, div / mod to decode.  It reads the largest n of every pair back
(15 synchronisations a call).  The numpy form is the same composition on the host.

A batch of --calls calls is timed on the host clock until the device has finished; batches of the paths alternate after a warm-up batch
each; medians over the batches with the p90 - p10 spread.  Bytes of the kernel path, from the shapes: the two passes over the 17 frames
(2 x 17 x H W x 4), the state read twice and written once (3 x H W x 16), the counts written, scanned and read (4 x H W x 8), and the
keys: written by the emitting pass (8 N), read and written once by the sort (16 N: a radix sort moves them once per 8-bit digit, so this
is a lower bound), read by the decoding kernel, which writes 13 N.  The fraction is those bytes over the call's time over 8.0 TB/s (the
spec rate of the HBM): an end-to-end figure of the whole call, the read-back included, not a kernel's share of peak."""
import argparse
import csv
import os
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from devo_amd import simulate as S                                      # noqa: E402

H, W, T, DT, C, HBM = 480, 640, 16, 1_000_000, 0.25, 8.0e12


def make_clip():
    """uint8 [16, H, W]: frame k is the texture rolled by 2 k px; the texture has period 32 px along x"""
    g = np.random.default_rng(0)
    tile = g.random((H + 16, 48))
    k = np.hanning(9)
    k /= k.sum()
    tile = np.apply_along_axis(lambda v: np.convolve(np.concatenate([v[-4:], v, v[:4]]), k, "valid"), 1, tile[:, :32])      # periodic along x
    tile = np.apply_along_axis(lambda v: np.convolve(v, k, "valid"), 0, np.concatenate([tile, tile[:8]]))[:H]
    tile = (tile - tile.min()) / (tile.max() - tile.min())
    tex = np.tile(tile, (1, W // 32))
    return np.stack([np.roll((255 * tex).astype(np.uint8), 2 * f, axis=1) for f in range(T)])


class Composed:
    """the model on whole frames with the array module `xp` semantics of torch (device) or numpy (host); refractory period 0"""

    def __init__(self, frame0, t0, host):
        self.host = host
        self.ref = frame0.astype(np.float64) if host else frame0.double()
        self.prev, self.prev_t = frame0, t0

    def forward(self, frames, stamps):
        host = self.host
        where, floor = (np.where, np.floor) if host else (torch.where, torch.floor)
        keys, t_first, hw = [], self.prev_t, H * W
        for img, t1 in zip(frames, stamps):
            i0 = (self.prev.astype(np.float64) if host else self.prev.double()).reshape(-1)
            i1 = (img.astype(np.float64) if host else img.double()).reshape(-1)
            ref = self.ref.reshape(-1)
            d = i1 - ref
            up = d >= 0
            n = floor(abs(d) / C)
            kmax = int(n.max())
            if kmax:
                k = (np.arange(1, kmax + 1, dtype=np.float64) if host else torch.arange(1, kmax + 1, dtype=torch.float64, device=img.device))[:, None]
                step = k * C
                L = where(up[None], ref[None] + step, ref[None] - step)
                den = (i1 - i0)[None]
                one = np.ones_like(den) if host else torch.ones_like(den)
                f = where(den != 0, (L - i0[None]) / where(den != 0, den, one), one)
                f = f.clip(0.0, 1.0) if host else f.clamp(0.0, 1.0)
                tk = floor(f * float(t1 - self.prev_t))
                tk = (tk.astype(np.int64) if host else tk.long()) + (self.prev_t - t_first)
                pix = (np.arange(hw, dtype=np.int64) if host else torch.arange(hw, device=img.device))[None]
                key = tk * (2 * hw) + pix * 2 + (up[None].astype(np.int64) if host else up[None].long())
                keys.append(key[k <= n[None]])
                nC = n * C
                self.ref = where(n > 0, where(up, ref + nC, ref - nC), ref)
            self.prev, self.prev_t = img, t1
        key = np.sort(np.concatenate(keys)) if host else torch.sort(torch.cat(keys)).values
        pix = (key // 2) % hw
        return {"x": pix % W, "y": pix // W, "t": key // (2 * hw) + t_first, "p": (key % 2) * 2 - 1}


def batch(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def split(path, calls, append):
    groups = (("count", "k_esim_count"), ("emit", "k_esim_emit"), ("decode", "k_esim_decode"), ("log_intensity", "k_log_intensity"), ("sort", "sort"), ("sort", "radix"),
              ("sort", "onesweep"), ("scan", "scan"), ("scan", "cumsum"))
    tot = {}
    for row in csv.DictReader(open(path)):
        name = next((g for g, key in groups if key in row["Name"].lower()), "other")
        tot[name] = tot.get(name, 0) + int(row["TotalDurationNs"])
    whole = sum(tot.values())
    lines = [f"# per-kernel split: rocprofv3 --kernel-trace --stats of `tools/bench_esim.py --profile {calls}` (a run of its own: {calls} calls after 2 warm-up calls, all in the trace;",
             "# kernel time per call, us; `other` is the runtime's fill and copy kernels: memsets of the sort and of the status word, the kept frame, the stamps)"]
    calls += 2
    for name in ("count", "scan", "emit", "sort", "decode", "log_intensity", "other"):
        if name in tot:
            lines.append(f"{name:>16} {tot[name] / 1e3 / calls:>10.1f} us  {100.0 * tot[name] / whole:>5.1f} %")
    print("\n".join(lines))
    if append:
        with open(append, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="calls per timed batch (the host path: 1)")
    ap.add_argument("--repeats", type=int, default=7, help="alternating batches per path")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="only run this many calls of the kernel path (for a profiler)")
    ap.add_argument("--split", default=None, help="a rocprofv3 kernel_stats.csv to sum by stage")
    ap.add_argument("--calls-profiled", type=int, default=20)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    if a.split:
        return split(a.split, a.calls_profiled, a.append)
    if not torch.cuda.is_available():
        raise SystemExit("bench_esim needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    u8 = make_clip()
    log = S.log_intensity(torch.from_numpy(u8).to(dev))
    log_host = log.cpu().numpy()
    assert np.array_equal(log_host.view(np.int32), np.log(u8.astype("float32") / 255 + 1e-5).view(np.int32))
    stamp = lambda call: DT * (1 + T * call + np.arange(T, dtype=np.int64))

    class Clock:                                                      # every path is fed the same endless clip: call c covers stamps DT (1 + 16 c) ...
        def __init__(self, make):
            self.sim, self.call = make(), 0

        def __call__(self):
            out = self.sim.forward(self.frames, self.stamps(self.call))
            self.call += 1
            return out

    def kernel():
        k = Clock(lambda: S.ESIM(C, C, 0))
        k.sim.forward(log[-1], 0)
        k.frames, k.stamps = log, stamp
        return k

    def composed(host):
        k = Clock(lambda: Composed(log_host[-1] if host else log[-1], 0, host))
        k.frames, k.stamps = (log_host if host else log), (lambda c: [int(v) for v in stamp(c)])
        return k

    if a.profile:
        k = kernel()
        for _ in range(2 + a.profile):
            k()
        torch.cuda.synchronize()
        return
    paths = {"kernel": kernel(), "torch on GPU": composed(False), "numpy on host": composed(True)}
    first = {name: p() for name, p in paths.items()}                  # call 0 of every path: the same events in the same order
    second = {name: p() for name, p in paths.items()}
    for got in (first, second):
        for name in ("torch on GPU", "numpy on host"):
            for key in "xytp":
                a_, b_ = got["kernel"][key].cpu().numpy().astype(np.int64), got[name][key]
                assert np.array_equal(a_, b_ if isinstance(b_, np.ndarray) else b_.cpu().numpy()), (name, key)
    N = int(second["kernel"]["t"].numel())
    nbytes = 2 * (T + 1) * H * W * 4 + 3 * H * W * 16 + 4 * H * W * 8 + (8 + 16 + 8 + 13) * N
    q = lambda v, p: float(np.quantile(np.asarray(v), p))
    lines = [f"# python tools/bench_esim.py  ({torch.cuda.get_device_name(0)}; {H} x {W}, {T} simulator frames per call, moving texture, C = {C}: {N} events per call = "
             f"{N / (T * H * W):.2f} per pixel and frame; ms per call over batches of {a.calls} calls (numpy: 1), batches of the paths alternating after one warm-up batch each; "
             f"median (p90 - p10) of {a.repeats} batches; bytes per call of the kernel path {nbytes / 1e6:.1f} MB, fraction of {HBM / 1e12:.1f} TB/s end to end)",
             f"{'path':>15} {'ms per call':>18} {'Mevents/s':>10} {'GB/s':>7} {'of HBM':>7}"]
    times = {k: [] for k in paths}
    for r in range(1 + a.repeats):
        for name, fn in paths.items():
            ms = batch(fn, 1 if name == "numpy on host" else a.calls)
            if r >= 1:
                times[name].append(ms)
    for name in paths:
        v = times[name]
        sec = q(v, 0.5) * 1e-3
        tail = f"{nbytes / sec / 1e9:>7.0f} {100.0 * nbytes / sec / HBM:>6.1f}%" if name == "kernel" else ""
        lines.append(f"{name:>15} {q(v, 0.5):>9.3f} ({q(v, 0.9) - q(v, 0.1):>6.3f}) {N / sec / 1e6:>10.1f} {tail}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
