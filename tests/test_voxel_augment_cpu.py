"""CPU checks of the voxel augmentation and the training input normalisation (devo_amd/events.py voxel_augment, devo_amd/training.py
TrainNet): CPU tensors are refused, unknown ops and norms raise, the factor table and the seeded op draw match the reference's
(tests/golden/voxel_augment.npz, tools/gen_golden_voxel_augment.py), and TrainNet's defaults leave its inputs alone."""
import os
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "voxel_augment.npz"))


def test_augmentation_refuses_cpu_tensors():
    from devo_amd import events
    x = torch.zeros(1, 2, 5, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        events.voxel_augment(x)
    with pytest.raises(RuntimeError, match="GPU"):
        events.voxel_augment(x, op="invert")
    with pytest.raises(RuntimeError, match="GPU"):
        events.augment(x, "adjust_brightness", 3)


def test_unknown_op_and_norm_raise():
    from devo_amd import events
    from devo_amd.training import TrainNet
    x = torch.zeros(1, 2, 5, 4, 4)
    with pytest.raises(ValueError, match="unknown augmentation op"):
        events.augment(x, "equalize", 0)
    with pytest.raises(ValueError, match="unknown augmentation op"):
        events.voxel_augment(x, op=7, factor_index=0)
    with pytest.raises(ValueError, match="factor_index"):
        events.augment(x, "solarize")
    with pytest.raises(NotImplementedError, match="norm"):
        TrainNet(norm="minmax")


def test_aug_factors_match_reference(gold):
    from devo_amd import events
    got = events.aug_factors(10)
    assert len(got) == len(events.AUG_OPS) == 7
    for i, t in enumerate(got):
        ref = gold[f"factors/{i}"]
        assert t.numpy().dtype == ref.dtype, f"factor table {i}: dtype {t.numpy().dtype} != {ref.dtype}"
        np.testing.assert_array_equal(t.numpy(), ref, err_msg=f"factor table {i}")


def test_seeded_draw_matches_reference(gold):
    from devo_amd import events
    seeds = sorted({int(k.split("/")[2]) for k in gold.files if k.startswith("va/") and k.endswith("/choice")})
    assert len(seeds) >= 5
    for s in seeds:
        torch.manual_seed(s)
        got = events.draw_augmentation(10)
        assert list(got) == gold[f"va/1/{s}/choice"].tolist() == gold[f"va/0/{s}/choice"].tolist(), f"seed {s}"


def test_trainnet_defaults_keep_inputs():
    import inspect
    from devo_amd.training import TrainNet, build_trainer
    sig = inspect.signature(TrainNet.__init__).parameters
    assert sig["norm"].default == "none" and sig["randaug"].default is False
    sig = inspect.signature(build_trainer).parameters
    assert sig["norm"].default == "none" and sig["randaug"].default is False
    net = TrainNet().train()
    assert net.norm == "none" and net.randaug is False
    x = torch.randn(1, 2, 5, 8, 8)
    assert net.normalise_images(x) is x                         # norm "none" without randaug: the grids go to the patchifier as given
