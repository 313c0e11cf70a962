"""tests/esim_ref.py (the restatement the GPU simulator is compared with) on hand-worked cases, and the host parts of devo_amd.simulate
against it.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import esim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(values, stamps, **kw):
    """a one-pixel clip in one call -> (list of (t, p), ref)"""
    ev, ref, _ = R.simulate_clip(np.asarray(values, dtype=np.float32).reshape(-1, 1, 1), stamps, **kw)
    return list(zip(ev["t"].tolist(), ev["p"].tolist())), float(ref[0, 0])


def test_ramp_up_crosses_four_levels():
    ev, ref = _one([0.0, 1.0], [0, 1000], contrast_threshold_pos=0.25, contrast_threshold_neg=0.5)
    assert ev == [(250, 1), (500, 1), (750, 1), (1000, 1)] and ref == 1.0      # (the level reached exactly counts)


def test_ramp_down_is_the_mirror():
    ev, ref = _one([1.0, 0.0], [0, 1000], contrast_threshold_pos=0.5, contrast_threshold_neg=0.25)
    assert ev == [(250, -1), (500, -1), (750, -1), (1000, -1)] and ref == 0.0


def test_remainder_is_carried_in_ref():
    """0 -> 0.375 crosses 0.25 at 2/3 of the pair and leaves ref there; 0.375 -> 0.625 crosses 0.5 (at (0.5 - 0.375) / 0.25 of the pair) from ref = 0.25"""
    ev, ref = _one([0.0, 0.375, 0.625], [0, 1000, 2000], contrast_threshold_pos=0.25)
    assert ev == [(666, 1), (1500, 1)] and ref == 0.5


def test_equal_frames_emit_nothing_and_f_is_one():
    ev, ref = _one([0.5, 0.5, 0.5], [0, 10, 20], contrast_threshold_pos=0.25)
    assert ev == [] and ref == 0.5
    sim = R.ESIM(0.25, 0.25)                                         # i1 == i0 with a level still to cross: f = 1, the event lands on t1
    sim.forward(np.zeros((1, 1), np.float32), [0])
    sim.ref[0, 0] = -0.25
    got = sim.forward(np.zeros((1, 1), np.float32), [100])
    assert got["t"].tolist() == [100] and got["p"].tolist() == [1] and sim.ref[0, 0] == 0.0


def test_refractory_suppresses_events_but_moves_ref():
    ev, ref = _one([0.0, 1.0], [0, 1000], contrast_threshold_pos=0.25, refractory_period_ns=500)
    assert ev == [(250, 1), (750, 1)] and ref == 1.0                 # 500 - 250 < 500 suppressed; 750 - 250 >= 500 emitted (>=); 1000 - 750 suppressed
    ev, _ = _one([0.0, 1.0], [0, 1000], contrast_threshold_pos=0.25, refractory_period_ns=250)
    assert [t for t, _ in ev] == [250, 500, 750, 1000]              # exactly the period apart: emitted


def test_event_at_stamp_zero_is_kept():
    ev, _ = _one([0.25, 0.5, 1.0], [-10, 0, 10], contrast_threshold_pos=0.25)
    assert ev == [(0, 1), (5, 1), (10, 1)]


def _clip(seed=0, T=6, H=3, W=4):
    g = np.random.default_rng(seed)
    frames = R.log_intensity(g.integers(0, 256, (T, H, W), dtype=np.uint8))
    stamps = np.cumsum(g.integers(900_000, 1_100_000, T)).astype(np.int64)
    return frames, stamps


def test_chunked_feeding_equals_one_call():
    frames, stamps = _clip()
    kw = dict(contrast_threshold_neg=0.19, contrast_threshold_pos=0.31, refractory_period_ns=20_000)
    one, ref1, last1 = R.simulate_clip(frames, stamps, None, **kw)
    assert len(one["t"]) > 100
    sim = R.ESIM(**kw)
    assert sim.forward(frames[0], stamps[0]) is None                 # the first frame alone gives no pair
    for chunks in ((1, 2, 3), (1,) * 6):
        got, ref, last = R.simulate_clip(frames, stamps, chunks, **kw)
        assert all(np.array_equal(got[k], one[k]) for k in "xytp")
        assert np.array_equal(ref.view(np.int64), ref1.view(np.int64)) and np.array_equal(last, last1)


def test_ties_are_ordered_by_pixel_then_polarity():
    """three pixels, dt = 4: pixels 0 and 2 ramp up, pixel 1 reverses exactly on the frame boundary; at stamp 4 the order is pixel 0 (+1), pixel 1 (-1 before +1), pixel 2"""
    frames = np.asarray([[[0.0, 0.0, 0.0]], [[0.25, 0.25, 0.25]], [[0.5, -0.75, 0.5]]], dtype=np.float32)
    ev, _, _ = R.simulate_clip(frames, [0, 4, 5], contrast_threshold_neg=0.25, contrast_threshold_pos=0.25)
    got = list(zip(ev["t"].tolist(), ev["x"].tolist(), ev["p"].tolist()))
    assert got == [(4, 0, 1), (4, 1, -1), (4, 1, -1), (4, 1, -1), (4, 1, 1), (4, 2, 1), (5, 0, 1), (5, 1, -1), (5, 2, 1)]
    assert ev["y"].tolist() == [0] * 9 and ev["x"].dtype == np.int16 and ev["p"].dtype == np.int8 and ev["t"].dtype == np.int64


# ------------------------------------------------------------------------------------------------ devo_amd.simulate's host parts
def S():
    from devo_amd import simulate
    return simulate


def test_log_table_is_numpys_expression():
    table = S().log_table()
    assert table.dtype == np.float32 and table.shape == (256,)
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(table[img].view(np.int32), R.log_intensity(img).view(np.int32))
    assert np.array_equal(table[img[::-1].copy()].view(np.int32), np.log(img[::-1].astype("float32") / 255 + 1e-5).view(np.int32))


def test_window_bounds_against_the_restatement():
    base = 1_600_000_000_000_000_000
    T = np.asarray([base + 7, base + 1_000_003, base + 2_000_001, base + 3_000_000], dtype=np.int64)
    t0, t1 = S().window_bounds(T, base + 7)
    w0, w1 = R.window_bounds(T, base + 7)
    assert t0.dtype == np.float64 and np.array_equal(t0, w0) and np.array_equal(t1, w1)
    assert t0.tolist() == [-np.inf, 1_000_003 - 7 + 1, 2_000_001 - 7 + 1] and t1.tolist() == [1_000_003 - 7 + 1, 2_000_001 - 7 + 1, np.inf]
    for t in (base, base + 8, base + 1_000_003, base + 1_000_004, base + 2_000_001, base + 2_000_002, base + 3_000_000, base + 9_000_000):
        rel = float(t - (base + 7))                                   # an event exactly on a real frame's stamp falls in the earlier window
        (w,) = np.nonzero((t0 <= rel) & (rel < t1))[0]
        assert w == R.window_of(t, T)
    assert R.window_of(base + 1_000_003, T) == 0 and R.window_of(base + 1_000_004, T) == 1 and R.window_of(base + 2_000_002, T) == 2
    t0, t1 = S().window_bounds([5, 9], 0)                             # two real frames: one window holding everything
    assert t0.tolist() == [-np.inf] and t1.tolist() == [np.inf]
    for bad in ([5], [5, 5], [9, 5], [1.5, 2.5]):
        with pytest.raises(ValueError):
            S().window_bounds(bad, 0)


def test_limits_and_host_refusals_need_no_gpu():
    sim = S()
    assert sim.max_span_ns(480, 640) == 1 << 43 and sim.max_span_ns(1, 1) == 1 << 61 and sim.max_span_ns(5, 7) == 1 << 56
    for H, W in ((0, 4), (4, 0), (32768, 4), (4, 32768)):
        with pytest.raises(ValueError):
            sim.max_span_ns(H, W)
    for kw in (dict(contrast_threshold_neg=5e-4), dict(contrast_threshold_pos=0.0), dict(contrast_threshold_pos=float("nan")), dict(contrast_threshold_neg=float("inf")),
               dict(refractory_period_ns=-1), dict(refractory_period_ns=0.5)):
        with pytest.raises(ValueError):
            sim.ESIM(**kw)
    e = sim.ESIM(0.2, 0.3, 1000)
    assert e.ref is None and e.last_t is None
    with pytest.raises(ValueError, match="GPU"):                      # no CPU fallback
        e.forward(torch.zeros(2, 4, 4), [0, 1])
    with pytest.raises(ValueError, match="GPU"):
        sim.log_intensity(torch.zeros(4, 4, dtype=torch.uint8))
    assert e.ref is None


def test_every_layer_carries_the_simulator():
    """header, ctypes table, build list, compiled binding and package exports name the new entry points; the ABI version is still 9"""
    from devo_amd import _lib, build
    import devo_amd
    txt = open(os.path.join(ROOT, "include", "devo_hip.h")).read()
    version_comment = txt[txt.index("#define DEVO_ABI_VERSION"):txt.index("int devo_abi_version")]
    assert _lib.ABI_VERSION == 9 and re.search(r"#define DEVO_ABI_VERSION 9\b", txt)
    for name in ("devo_esim_count", "devo_esim_emit", "devo_esim_sort_keys", "devo_esim_sort_workspace_bytes", "devo_esim_decode", "devo_esim_max_span_ns", "devo_log_intensity"):
        assert name in version_comment and re.search(r"\b" + name + r"\(", txt) and name in _lib.EXPORTED_SYMBOLS
    assert "esim.hip" in build.SOURCES
    bind = open(os.path.join(ROOT, "devo_amd", "csrc", "bind.cpp")).read()
    for op in ("esim_count", "esim_emit", "esim_sort", "esim_decode", "log_intensity"):
        assert f'm.def("{op}(' in bind and f'm.impl("{op}"' in bind
    assert devo_amd.simulate is S() and callable(devo_amd.simulate.frames_to_voxels)
    src = open(os.path.join(ROOT, "devo_amd", "csrc", "esim.hip")).read()
    assert "#pragma clang fp contract(off)" in src
