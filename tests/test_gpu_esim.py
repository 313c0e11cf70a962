"""devo_amd.simulate (csrc/esim.hip) against tests/esim_ref.py, the fp64 restatement checked by hand in test_esim_cpu.py.  The device does
the model's fp64 arithmetic with the same single roundings in the same order, so everything is compared with torch.equal: x, y, t, p, the
final `last_t`, and the final `ref` as bit patterns.  The restatement of a clip is computed once and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import esim_ref as R
from util import assert_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((5, 7), (33, 70), (64, 64))                                # one ragged wave; a ragged last wave and a ragged last row; whole blocks
BASE = 1_600_000_000_000_000_000                                      # an epoch-sized stamp in ns: not representable in fp64 to the nanosecond


def S():
    from devo_amd import simulate
    return simulate


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """the module's device tensors, the log table and the allocator's cached blocks go when its last test has run"""
    yield
    _clip.cache_clear()
    _want.cache_clear()
    S().clear_cache()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ clips
def _stamps(T, seed, base=0, lo=8_000_000, hi=12_000_000):
    return base + np.cumsum(np.random.default_rng(seed).integers(lo, hi, T)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _clip(kind, H, W, T=6):
    """-> (frames fp32 [T, H, W] numpy, stamps int64 [T] numpy, simulator arguments)"""
    g = np.random.default_rng(H * 1000 + W)
    if kind in ("random", "random_refractory", "random_dt3", "random_large"):
        frames = R.log_intensity(g.integers(0, 256, (T, H, W), dtype=np.uint8))
        kw = dict(contrast_threshold_neg=0.19, contrast_threshold_pos=0.31)
        if kind == "random_refractory":
            kw["refractory_period_ns"] = 2_000_000
        stamps = 3 * np.arange(1, T + 1, dtype=np.int64) if kind == "random_dt3" else _stamps(T, 1, BASE if kind == "random_large" else 0)
        return frames, stamps, kw
    if kind == "smooth":                                               # a slowly drifting pattern: few events per pixel, none where its amplitude is small
        y, x = np.mgrid[0:H, 0:W]
        frames = np.stack([0.3 * np.sin(x / 5.0 + 0.35 * t) * np.cos(y / 7.0) for t in range(T)]).astype(np.float32)
        return frames, _stamps(T, 2), dict(contrast_threshold_neg=0.05, contrast_threshold_pos=0.05)
    if kind == "step":                                                 # all 0 then all 255: about 230 events at every pixel from one pair
        u8 = np.full((T, H, W), 255, dtype=np.uint8)
        u8[0] = 0
        return R.log_intensity(u8), _stamps(T, 3), dict(contrast_threshold_neg=0.05, contrast_threshold_pos=0.05)
    if kind == "dyadic":                                               # multiples of 1/64 and C = 1/4: levels are hit exactly, f is 0 and 1 exactly
        frames = (g.integers(-128, 129, (T, H, W)) / 64.0).astype(np.float32)
        frames[:, 0, 0] = [0.0, 0.5, -3.5, 0.5, 0.5, -0.25]           # reverses exactly on a frame boundary: +1 at f = 1, then -1 at floor(f dt) = 0
        frames[:, 0, 1] = frames[:, 0, 0]                              # an identical neighbour: every tie is broken by the pixel index
        frames[:, 1, 2] = frames[:, 1, 3] = [1.0, 1.25, 1.5, 1.5, 0.75, 1.0]
        return frames, np.asarray([10, 13, 16, 1016, 1019, 2019], dtype=np.int64), dict(contrast_threshold_neg=0.25, contrast_threshold_pos=0.25)
    raise KeyError(kind)


def _u8(kind, H, W, T=6):
    """the uint8 frames behind the "random" and "step" clips (the same draws as in _clip)"""
    if kind == "step":
        u8 = np.full((T, H, W), 255, dtype=np.uint8)
        u8[0] = 0
        return u8
    return np.random.default_rng(H * 1000 + W).integers(0, 256, (T, H, W), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(kind, H, W, T=6):
    """the restatement of the clip in one call -> (events as tensors on the host, ref bits int64, last_t)"""
    frames, stamps, kw = _clip(kind, H, W, T)
    ev, ref, last = R.simulate_clip(frames, stamps, None, **kw)
    return {k: torch.from_numpy(v) for k, v in ev.items()}, torch.from_numpy(ref.view(np.int64).copy()), torch.from_numpy(last.copy())


def _run(frames, stamps, kw, chunks=None, stamps_on="host"):
    """the clip through a fresh simulate.ESIM in calls of the given sizes -> (concatenated events, ref bits, last_t, the simulator), on the host"""
    sim = S().ESIM(**kw)
    dev = frames if torch.is_tensor(frames) else torch.from_numpy(frames).to(DEV)
    ts = torch.from_numpy(stamps).to(DEV) if stamps_on == "device" else stamps
    parts, a = [], 0
    for c in ([len(frames)] if chunks is None else chunks):
        ev = sim.forward(dev[a:a + c], ts[a:a + c])
        a += c
        if ev is not None:
            parts.append(ev)
    ev = {k: torch.cat([e[k] for e in parts]).cpu() for k in "xytp"}
    return ev, sim.ref.view(torch.int64).cpu(), sim.last_t.cpu(), sim


def _assert_same(got, want, what):
    ev, ref, last = got[:3]
    wev, wref, wlast = want
    for k, dt in zip("xytp", (torch.int16, torch.int16, torch.int64, torch.int8)):
        assert ev[k].dtype == dt and ev[k].shape == wev[k].shape, f"{what}: {k} is {ev[k].dtype} {tuple(ev[k].shape)}, the restatement has {tuple(wev[k].shape)}"
        assert torch.equal(ev[k], wev[k]), f"{what}: {k} differs"
    assert torch.equal(ref, wref), f"{what}: ref differs in {int((ref != wref).sum())} pixels"
    assert torch.equal(last, wlast), f"{what}: last_t differs"


# ------------------------------------------------------------------------------------------------ the model, bit for bit
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ("random", "smooth", "step"))
def test_events_equal_the_restatement(kind, shape):
    frames, stamps, kw = _clip(kind, *shape)
    want = _want(kind, *shape)
    n, hw = len(want[0]["t"]), shape[0] * shape[1]
    if kind == "step":
        assert 225 * hw <= n <= 235 * hw and int((want[2] == R.NO_EVENT).sum()) == 0
    if kind == "smooth":
        assert 0 < n < 5 * hw and (hw < 100 or int((want[2] == R.NO_EVENT).sum()) > hw // 20)      # few events per pixel, many pixels with none
    if kind == "random":
        assert n > 5 * hw
    if kind != "smooth":                                               # uint8 frames through simulate.log_intensity: numpy's values to the bit
        dev = S().log_intensity(torch.from_numpy(_u8(kind, *shape)).to(DEV))
        assert torch.equal(dev.cpu().view(torch.int32), torch.from_numpy(frames).view(torch.int32))
        frames = dev
    _assert_same(_run(frames, stamps, kw), want, f"{kind} {shape}")


def test_log_intensity_is_numpys_bit_for_bit():
    g = np.random.default_rng(5)
    for shape in ((6, 33, 70), (256,), (3, 5, 7), (1,)):
        u8 = np.arange(256, dtype=np.uint8) if shape == (256,) else g.integers(0, 256, shape, dtype=np.uint8)
        got = S().log_intensity(torch.from_numpy(u8).to(DEV))
        assert got.dtype == torch.float32 and got.shape == u8.shape and got.is_cuda
        assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(R.log_intensity(u8)).view(torch.int32))
    odd = torch.from_numpy(g.integers(0, 256, 1003, dtype=np.uint8)).to(DEV)[1:]          # a base address no 4-byte load may touch
    assert torch.equal(S().log_intensity(odd).cpu().view(torch.int32), torch.from_numpy(R.log_intensity(odd.cpu().numpy())).view(torch.int32))


def test_dyadic_levels_are_hit_exactly():
    """f = 0 and f = 1 exactly, a reversal on a frame boundary (equal stamps of opposite polarity, -1 first), ties between identical pixels"""
    frames, stamps, kw = _clip("dyadic", 5, 7)
    want = _want("dyadic", 5, 7)
    ev = want[0]
    at = (ev["t"] == 13) & (ev["y"] == 0) & (ev["x"] == 0)
    assert ev["p"][at].tolist() == [-1] * 5 + [1]                      # +1 at the end of pair (0, 0.5); floor(3 k / 16) = 0 for the first five levels of pair (0.5, -3.5)
    twin = (ev["y"] == 0) & (ev["x"] == 1)                              # the identical neighbour: the same stamps and polarities, each tie after pixel 0
    assert ev["t"][twin].tolist() == ev["t"][(ev["y"] == 0) & (ev["x"] == 0)].tolist() and int(twin.sum()) >= 20
    _assert_same(_run(frames, stamps, kw), want, "dyadic")


def test_three_nanosecond_pairs_share_stamps():
    frames, stamps, kw = _clip("random_dt3", 5, 7)
    want = _want("random_dt3", 5, 7)
    assert len(torch.unique(want[0]["t"])) <= 16 and len(want[0]["t"]) > 200
    _assert_same(_run(frames, stamps, kw), want, "dt = 3 ns")


@pytest.mark.parametrize("stamps_on", ("host", "device"))
def test_epoch_sized_stamps_stay_exact(stamps_on):
    frames, stamps, kw = _clip("random_large", 5, 7)
    assert any(int(np.float64(s)) != int(s) for s in stamps)                      # fp64 cannot hold them
    _assert_same(_run(frames, stamps, kw, stamps_on=stamps_on), _want("random_large", 5, 7), f"large stamps on the {stamps_on}")


# ------------------------------------------------------------------------------------------------ state
def test_any_chunking_gives_the_events_and_state_of_one_call():
    frames, stamps, kw = _clip("random", 33, 70)
    want = _want("random", 33, 70)
    for chunks in ((1, 2, 3), (1,) * 6, None):
        _assert_same(_run(frames, stamps, kw, chunks), want, f"chunks {chunks}")


def test_first_frame_returns_none_and_reset_restores_it():
    frames, stamps, kw = _clip("random", 5, 7)
    want = _want("random", 5, 7)
    dev = torch.from_numpy(frames).to(DEV)
    sim = S().ESIM(**kw)
    assert sim.ref is None and sim.last_t is None
    assert sim.forward(dev[0], int(stamps[0])) is None
    assert torch.equal(sim.ref.cpu(), torch.from_numpy(frames[0]).double()) and bool((sim.last_t == S().NO_EVENT).all())
    first = sim.forward(dev[1:4], stamps[1:4])
    assert first is not None and len(first["t"]) > 0
    sim.reset()
    assert sim.ref is None
    assert sim.forward(dev[0], torch.tensor(int(stamps[0]))) is None              # a 0-d stamp tensor
    ev = sim(dev[1:], torch.from_numpy(stamps[1:]))                               # a CPU stamp tensor; __call__
    for k in "xytp":
        assert torch.equal(ev[k].cpu(), want[0][k])
    assert torch.equal(sim.ref.view(torch.int64).cpu(), want[1]) and torch.equal(sim.last_t.cpu(), want[2])


def test_refractory_period():
    frames, stamps, kw = _clip("random_refractory", 33, 70)
    want, free = _want("random_refractory", 33, 70), _want("random", 33, 70)
    assert 0 < len(want[0]["t"]) < len(free[0]["t"])
    got = _run(frames, stamps, kw)
    _assert_same(got, want, "refractory")
    assert torch.equal(got[1], free[1])                                           # suppressed events moved ref all the same


def test_no_event_gives_four_empty_tensors():
    frames = np.zeros((3, 5, 7), dtype=np.float32)
    frames[1] += 0.01
    sim = S().ESIM(0.2, 0.2)
    ev = sim.forward(torch.from_numpy(frames).to(DEV), [5, 6, 7])
    assert ev is not None and [ev[k].dtype for k in "xytp"] == [torch.int16, torch.int16, torch.int64, torch.int8]
    assert all(ev[k].shape == (0,) and ev[k].is_cuda for k in "xytp")
    assert bool((sim.ref == 0).all()) and bool((sim.last_t == S().NO_EVENT).all())


# ------------------------------------------------------------------------------------------------ refusals
def _state(sim):
    return sim.ref.view(torch.int64).cpu(), sim.last_t.cpu()


def test_host_side_refusals_raise_value_error():
    frames, stamps, kw = _clip("random", 5, 7)
    dev = torch.from_numpy(frames).to(DEV)
    sim = S().ESIM(**kw)
    bad = [lambda: sim.forward(dev[:3], [5, 5, 6]), lambda: sim.forward(dev[:3], [5, 4, 6]), lambda: sim.forward(dev[:3], [5, 6]),
           lambda: sim.forward(dev[:2], [0, 1 << 62]), lambda: sim.forward(dev[:2], [0.5, 1.5]), lambda: sim.forward(dev[:2].cpu(), [0, 1]),
           lambda: sim.forward(dev[:2].double(), [0, 1]), lambda: sim.forward(dev[:2], torch.tensor([0.0, 1.0], device=DEV)),
           lambda: S().ESIM(contrast_threshold_neg=1e-4), lambda: S().ESIM(contrast_threshold_pos=float("nan")), lambda: S().ESIM(refractory_period_ns=-5),
           lambda: S().log_intensity(torch.zeros(4, 4, dtype=torch.uint8)), lambda: S().log_intensity(torch.zeros(4, 4, device=DEV))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert sim.ref is None                                                        # nothing above touched the state
    sim.forward(dev[:3], stamps[:3])
    before = _state(sim)
    bad = [lambda: sim.forward(dev[3, :4], int(stamps[3])), lambda: sim.forward(dev[3], int(stamps[2])), lambda: sim.forward(dev[3], int(stamps[2]) - 1),
           lambda: sim.forward(dev[3], int(stamps[2]) + S().max_span_ns(5, 7))]
    for call in bad:                                                              # another frame size; a stamp not after the kept one; too long a span
        with pytest.raises(ValueError):
            call()
    assert all(torch.equal(a, b) for a, b in zip(before, _state(sim)))
    rest = sim.forward(dev[3:], stamps[3:])                                       # and the simulator goes on as if nothing had happened
    assert torch.equal(sim.last_t.cpu(), _want("random", 5, 7)[2]) and len(rest["t"]) > 0


def test_device_flagged_failures_leave_the_state():
    frames, stamps, kw = _clip("random", 5, 7)
    want = _want("random", 5, 7)
    dev = torch.from_numpy(frames).to(DEV)
    sim = S().ESIM(**kw)
    first = sim.forward(dev[:3], stamps[:3])
    before = _state(sim)
    poisoned = dev[3:].clone()
    poisoned[1, 2, 3] = float("nan")
    with pytest.raises(RuntimeError, match="not finite"):
        sim.forward(poisoned, stamps[3:])
    assert all(torch.equal(a, b) for a, b in zip(before, _state(sim)))
    poisoned[1, 2, 3] = float("inf")
    with pytest.raises(RuntimeError, match="not finite"):
        sim.forward(poisoned, torch.from_numpy(stamps[3:]).to(DEV))
    down = torch.from_numpy(np.asarray([stamps[3], stamps[5], stamps[4]])).to(DEV)
    with pytest.raises(RuntimeError, match="increasing"):
        sim.forward(dev[3:], down)
    with pytest.raises(RuntimeError, match="increasing"):                         # not after the stamp kept from the previous call
        sim.forward(dev[3:], torch.from_numpy(stamps[3:] - stamps[3] + stamps[2]).to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(before, _state(sim)))
    rest = sim.forward(dev[3:], torch.from_numpy(stamps[3:]).to(DEV))
    for k in "xytp":
        assert torch.equal(torch.cat([first[k], rest[k]]).cpu(), want[0][k])
    assert torch.equal(sim.ref.view(torch.int64).cpu(), want[1]) and torch.equal(sim.last_t.cpu(), want[2])
    fresh = S().ESIM(**kw)                                                        # a first call that fails sets nothing
    with pytest.raises(RuntimeError, match="not finite"):
        fresh.forward(torch.cat([dev[:1], poisoned]), [1, 2, 3, 4])
    assert fresh.ref is None and fresh.last_t is None


def test_a_call_on_a_side_stream_is_ordered_with_that_stream():
    frames, stamps, kw = _clip("random", 64, 64)
    want = _want("random", 64, 64)
    src = torch.from_numpy(frames).pin_memory()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = torch.ones(2048, 2048, device=DEV)
        for _ in range(8):                                                        # work in front of the upload on this stream
            a = (a @ a) * (1.0 / 2048)
        dev = torch.empty(frames.shape, dtype=torch.float32, device=DEV).fill_(float("nan"))
        dev.copy_(src, non_blocking=True)
        sim = S().ESIM(**kw)
        ev = sim.forward(dev, stamps)
        n_on_stream = ev["t"].numel() + int(a[0, 0] > 2)                          # consumed on the same stream
        got = {k: v.cpu() for k, v in ev.items()}
    torch.cuda.current_stream().wait_stream(side)
    assert n_on_stream == len(want[0]["t"])
    for k in "xytp":
        assert torch.equal(got[k], want[0][k])


# ------------------------------------------------------------------------------------------------ clip -> voxel grids
def test_frames_to_voxels():
    """33 x 70, 13 simulator frames, every fourth a real frame; row 0 ramps by exactly one threshold per frame, so events fall EXACTLY on every
    simulator stamp, the real frames' among them, and must be counted in the earlier window"""
    from devo_amd import events as E
    H, W, T, bins = 33, 70, 13, 5
    frames, _, _ = _clip("random", H, W, T)
    frames = frames.copy()
    frames[:, 0, :] = 0.25 * np.arange(T, dtype=np.float32)[:, None]
    stamps = _stamps(T, 7, BASE)
    real = stamps[::4]
    kw = dict(contrast_threshold_neg=0.25, contrast_threshold_pos=0.25)
    ev, _, _ = R.simulate_clip(frames, stamps, None, **kw)
    win = np.asarray([R.window_of(int(t), real) for t in ev["t"]])
    want_counts = np.bincount(win, minlength=3)
    assert ((ev["t"] == real[1]) & (win == 0)).sum() >= W and ((ev["t"] == real[2]) & (win == 1)).sum() >= W and want_counts.min() > 1000
    t0, t1 = R.window_bounds(real, stamps[0])
    d = lambda v: torch.from_numpy(v).to(DEV)
    want_grids, c = E.voxel_grids(d(ev["x"]), d(ev["y"]), d((ev["t"] - stamps[0]).astype(np.float64)), d(ev["p"]), t0, t1, H, W, bins=bins)
    assert c.tolist() == want_counts.tolist()
    dev = d(frames)
    sim = S().ESIM(**kw)
    for per_call, ts in ((None, stamps), (1, stamps), (5, d(stamps))):
        grids, counts = S().frames_to_voxels(sim, dev, ts, real, bins=bins, frames_per_call=per_call)
        assert grids.shape == (3, bins, H, W) and grids.dtype == torch.float32 and counts.dtype == torch.int64
        assert counts.tolist() == want_counts.tolist(), f"frames_per_call {per_call}"
        assert_rel(grids, want_grids, 1e-5, f"frames_per_call {per_call}")


# ------------------------------------------------------------------------------------------------ the two bindings
_LEG = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import esim_ref as R
from devo_amd import simulate as S, backends as B
assert (B.native() is None) == (os.environ.get("DEVO_BINDING") == "ctypes")
g = np.random.default_rng(33070)
u8 = g.integers(0, 256, (6, 33, 70), dtype=np.uint8)
stamps = np.cumsum(g.integers(8_000_000, 12_000_000, 6)).astype(np.int64)
sim = S.ESIM(0.19, 0.31, 1_000_000)
log = S.log_intensity(torch.from_numpy(u8).cuda())
parts = [sim.forward(log[:2], stamps[:2]), sim.forward(log[2:], torch.from_numpy(stamps[2:]).cuda())]
out = {k: torch.cat([p[k] for p in parts]).cpu() for k in "xytp"}
out["log"], out["ref"], out["last_t"] = log.cpu(), sim.ref.cpu(), sim.last_t.cpu()
torch.save(out, sys.argv[2])
"""


def test_compiled_and_ctypes_bindings_give_the_same_bits(tmp_path):
    res = []
    for binding in ("native", "ctypes"):
        env = dict(os.environ)
        env["DEVO_BINDING"] = binding
        path = str(tmp_path / f"{binding}.pt")
        r = subprocess.run([sys.executable, "-c", _LEG, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res.append(torch.load(path))
    a, b = res
    assert set(a) == set(b)
    bits = lambda v: v.view(torch.int64) if v.dtype == torch.float64 else v.view(torch.int32) if v.dtype == torch.float32 else v
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(bits(a[k]), bits(b[k])), k
    g = np.random.default_rng(33070)
    u8 = g.integers(0, 256, (6, 33, 70), dtype=np.uint8)
    stamps = np.cumsum(g.integers(8_000_000, 12_000_000, 6)).astype(np.int64)
    ev, ref, last = R.simulate_clip(R.log_intensity(u8), stamps, None, contrast_threshold_neg=0.19, contrast_threshold_pos=0.31, refractory_period_ns=1_000_000)
    assert len(ev["t"]) > 10000
    for k in "xytp":
        assert torch.equal(a[k], torch.from_numpy(ev[k])), k
    assert torch.equal(a["ref"].view(torch.int64), torch.from_numpy(ref).view(torch.int64)) and torch.equal(a["last_t"], torch.from_numpy(last))
