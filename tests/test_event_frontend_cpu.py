"""CPU checks of the event front end (devo_amd/events.py): CPU tensors are refused (the HIP path has no CPU fallback), and the
top-k mode of RemoveHotPixelsVoxel, which no loader uses, is refused with a clear error."""
import pytest
import torch


def test_front_end_refuses_cpu_tensors():
    from devo_amd import events
    x = torch.zeros(4, dtype=torch.int32)
    ts = torch.arange(4, dtype=torch.int64)
    p = torch.ones(4, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="GPU"):
        events.voxel_grids(x.float(), x.float(), ts, p, [0.0], [5.0], 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        events.voxel_grids(x, x, ts, p, [0.0], [5.0], 4, 4, rectify_map=torch.zeros(4, 4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        next(events.real_data_voxels(x, x, ts, p, [0.0], 5.0, [1.0, 1.0, 2.0, 2.0], torch.zeros(4, 4, 2), 4, 4, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        events.remove_hot_pixels(torch.zeros(5, 4, 4), 6)
    with pytest.raises(RuntimeError, match="GPU"):
        events.RemoveHotPixelsVoxel(num_stds=6)(torch.zeros(5, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        events.rescale(torch.zeros(1, 2, 5, 4, 4))


def test_hot_pixel_top_k_mode_is_refused():
    from devo_amd import events
    with pytest.raises(NotImplementedError, match="num_hot_pixels"):
        events.RemoveHotPixelsVoxel(num_hot_pixels=100)
    assert events.RemoveHotPixelsVoxel(num_stds=10).num_stds == 10
