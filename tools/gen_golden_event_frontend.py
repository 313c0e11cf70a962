#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Generate tests/golden/event_frontend.npz by running the REAL reference loader front end from /root/reference on CPU over
seeded synthetic recordings: EventSlicer (utils/event_utils.py) over an in-memory dict shaped like the h5 file (x, y, t, p,
ms_to_idx, t_offset), utils/load_utils.py:get_real_data_list with an identity resize and RemoveHotPixelsVoxel(num_stds)
(k = 6 as for TUM-VIE, k = 10 as for EDS), to_voxel_grid on unrectified fractional coordinates per window, and
utils/voxel_utils.py:rescale (on the first three windows).  Each recording has one injected hot pixel, an event gap (an empty window), overlapping and
touching windows and one window past the end of ms_to_idx.  The file holds data only (inputs + expected outputs).
Import-time stubs: h5py, hdf5plugin, numba (jit = identity), cv2, torchvision, and the loaders' plotting / transform helpers."""
import os
import sys
import types
import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
MARGIN = 1e-4          # no voxel within this relative distance of its hot-pixel threshold (f32 vs f64 statistics cannot flip a bit)


def _mod(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _stubs():
    _mod("h5py", File=object)
    _mod("hdf5plugin")
    _mod("cv2")
    _mod("numba", jit=lambda *a, **k: (lambda f: f))
    tv = _mod("torchvision")
    tr = _mod("torchvision.transforms", Resize=lambda *a, **k: (lambda x: x))
    tv.transforms = tr
    tr.functional = _mod("torchvision.transforms.functional")
    sys.path.insert(0, REF)
    import utils  # noqa: F401  (the namespace package, before its sub-modules are stubbed)
    _mod("utils.viz_utils", visualize_voxel=None, visualize_N_voxels=None, render=None)
    _mod("utils.transform_utils", transform_rescale=None)


def recording(rng, N, H, W, t_offset, hot):
    """Events over 0..60 ms (relative to t_offset) with no event in [30.3, 38) ms; 4 % of them on the hot pixel `hot` (x, y)."""
    t = np.concatenate([rng.integers(0, 30300, N // 2), rng.integers(38000, 60000, N - N // 2)])
    t = np.sort(t).astype(np.int64)
    x = rng.integers(0, W, N).astype(np.uint16)
    y = rng.integers(0, H, N).astype(np.uint16)
    p = rng.integers(0, 2, N).astype(np.uint8)
    h = rng.random(N) < 0.04
    x[h], y[h], p[h] = hot[0], hot[1], 1
    n_ms = int(np.ceil(t[-1] / 1000)) + 1
    ms_to_idx = np.searchsorted(t, np.arange(n_ms) * 1000, side="left").astype(np.int64)
    xf = (x + rng.uniform(-1.5, 1.5, N)).astype(np.float32)             # unrectified fractional coordinates, some outside
    yf = (y + rng.uniform(-1.5, 1.5, N)).astype(np.float32)
    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rmap = np.stack([gx * 1.03 - 0.7 + 0.4 * np.sin(gy / 7.0), gy * 0.98 + 0.3 + 0.5 * np.cos(gx / 9.0)], -1).astype(np.float32)
    return dict(x=x, y=y, t=t, p=p, ms_to_idx=ms_to_idx, t_offset=np.array(t_offset, dtype=np.int64)), xf, yf, rmap


def check_margin(raw, k, what):
    v = raw.double().flatten()
    thr = float(v.mean() + k * v.std())
    gap = float(((v.abs() - thr).abs() / abs(thr)).min())
    assert gap > MARGIN, f"{what}: a voxel lies {gap:.2e} (relative) from its hot-pixel threshold; pick another seed"


def main():
    _stubs()
    from utils.event_utils import EventSlicer, to_voxel_grid, RemoveHotPixelsVoxel
    from utils.load_utils import get_real_data_list
    from utils.voxel_utils import rescale

    rng = np.random.default_rng(32)
    out = {}
    # starts (us after t_offset): touching (500 / 4500 / 8500), overlapping (8500 / 10000), in the gap (30500: empty; its
    # conservative millisecond range [30, 35) does hold events, else the reference's slicer fails on an empty array), across its
    # end (34500), past the end of ms_to_idx (57500 + 4 ms -> ms 62 >= 61: EventSlicer returns None)
    starts = np.array([500, 4500, 8500, 10000.25, 14000, 20000, 26500.5, 30500, 34500, 45000, 52000.75, 57500])
    for tag, (N, H, W, k, t_offset, hot) in {"tumvie": (1600, 48, 64, 6, 1_234_567_000, (17, 29)),
                                             "eds": (1400, 40, 56, 10, 0, (40, 11))}.items():
        h5, xf, yf, rmap = recording(rng, N, H, W, t_offset, hot)
        tss = starts + t_offset
        dT_ms, intr = 4.0, [float(W), float(W), W / 2.0, H / 2.0]
        slicer = EventSlicer(h5)
        hot_list = get_real_data_list(slicer, tss, intr, rmap, [lambda v: v, RemoveHotPixelsVoxel(num_stds=k)], dT_ms, H, W)
        raw_list = get_real_data_list(slicer, tss, intr, rmap, [lambda v: v], dT_ms, H, W)
        mids = [m for _, _, m in raw_list]
        assert [m for _, _, m in hot_list] == mids and 6 <= len(mids) < len(tss)
        idx = [int(np.nonzero((tss + (tss + dT_ms * 1e3)) / 2 == m)[0][0]) for m in mids]
        raw = torch.stack([v for v, _, _ in raw_list])
        hot_vox = torch.stack([v for v, _, _ in hot_list])
        for i, r in enumerate(raw):
            check_margin(r, k, f"{tag} window {idx[i]}")
        assert int((hot_vox != raw).sum()) > 0, "the hot pixel was not caught"
        # no rectification: fractional coordinates straight into to_voxel_grid, windows sliced by EventSlicer
        sl_f = EventSlicer(dict(h5, x=xf, y=yf))
        nm_idx, nm_raw, nm_hot = [], [], []
        for i, a in enumerate(tss):
            ev = sl_f.get_events(a, a + dT_ms * 1e3)
            if ev is None or len(ev["t"]) == 0:
                continue
            v = to_voxel_grid(ev["x"], ev["y"], ev["t"], ev["p"], H=H, W=W, nb_of_time_bins=5)
            check_margin(v, k, f"{tag} unrectified window {i}")
            nm_idx.append(i)
            nm_raw.append(v)
            nm_hot.append(RemoveHotPixelsVoxel(num_stds=k)(v.clone()))
        nm_raw, nm_hot = torch.stack(nm_raw), torch.stack(nm_hot)
        seq = hot_vox[None, :3].contiguous()                                    # rescale: the first three windows as one sequence
        rs_seq, rs_frame = rescale(seq.clone(), sequence=True), rescale(seq.clone(), sequence=False)
        assert torch.equal(rs_seq, rs_frame)                                   # the reference's flag changes nothing
        for key, val in dict(x=h5["x"], y=h5["y"], t=h5["t"], p=h5["p"], ms_to_idx=h5["ms_to_idx"], t_offset=h5["t_offset"], xf=xf, yf=yf,
                             rmap=rmap, tss=tss, dT_ms=np.float64(dT_ms), intrinsics=np.array(intr), k=np.float64(k),
                             list_idx=np.array(idx), list_mid=np.array(mids, dtype=np.float64), list_raw=raw.numpy(),
                             list_hot=torch.nonzero((hot_vox == 0) & (raw != 0)).numpy().astype(np.int32),
                             nomap_idx=np.array(nm_idx), nomap_raw=nm_raw.numpy(),
                             nomap_hot=torch.nonzero((nm_hot == 0) & (nm_raw != 0)).numpy().astype(np.int32),
                             rescale=rs_seq[0].numpy()).items():
            out[f"{tag}/{key}"] = np.asarray(val)
        print(tag, "windows", len(tss), "served", len(idx), "hot voxels", len(out[f"{tag}/list_hot"]), len(out[f"{tag}/nomap_hot"]))
    path = os.path.join(ROOT, "tests", "golden", "event_frontend.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
