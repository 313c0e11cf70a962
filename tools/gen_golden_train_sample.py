#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (fixture generator; build container only — it imports the reference).

Generate tests/golden/train_sample.npz by running the REAL reference code from /root/reference on CPU with one torch thread, as its
DataLoader workers do: devo/data_readers/augmentation.py (voxel_color_jitter, EVSDAugmentor), utils/transform_utils.py
(transform_rescale) and EVSDDataset.__getitem__ (devo/data_readers/base.py) itself.  The dataset object is made with __new__, given
an in-memory scene_info, and its voxel_read / depth_read return arrays held here.

Missing modules are stubbed: torchvision (0.13's Resize on a tensor is F.interpolate(size, 'bilinear', align_corners=False) without
antialias, after unsqueezing a 3-d tensor to [1, ...]), and h5py, cv2, hdf5plugin, numba, evo and the compiled lietorch backends,
which none of the code run here calls.  Every bilinear output here is larger than 128 in height + width, so that ATen takes the
separable generic kernel it takes at the training size (below that it switches to its channels-last kernel).  The file holds data only.

Contents (v: voxels, d: disparities = 1 / depth, float32; voxel inputs are int8 / 8, depths uint16 / 64):
  in/vox_q [2, 2, 11, 141], in/depth_q [2, 11, 141], in/poses [2, 7], in/intr [2, 4]   the augmentor's input (crop 8 x 120)
  aug/<s>/{scale, rand, uniform, branch, v, d, intr}  EVSDAugmentor(crop)(v, poses, d, intr) after np.random.seed(s),
                                                      torch.manual_seed(s): its np draws (uniform: NaN when not drawn), outputs
  fix/<f>/<s>/scale                                    voxel_spatial_transform's scale for fix_scale = f after np.random.seed(s)
  tr/vox_q [1, 2, 5, 261], tr/depth_q [1, 5, 261]; tr/<scale>/{v, d, poses, intr}      transform_rescale
  gi/vox_q [2, 2, 21, 283], gi/depth_q [2, 21, 283]   EVSDDataset's input at dataset scale 0.5 and 0.75 (crop 16 x 250, scaled);
                                                      at scale 1 it reads in/ (crop 8 x 120); poses and intrinsics: in/
  gi/<scale>/<s>/{scale_drawn, v, d, poses, intr}     __getitem__(0) after np.random.seed(s), torch.manual_seed(s)
  q/<case>/{x, s, d, poses}                            the depth normalisation on [n, H, W] disparities with inf, NaN, ties
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types
import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
REF = "/root/reference"
AUG_SEEDS = (0, 1, 2, 3, 4, 5)
GI_SEEDS = {1.0: (0, 5), 0.5: (8,), 0.75: (9,)}
CROP = (8, 120)
GI_CROP = (16, 250)


class _Any:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]                                       # a decorator (numba.jit(...)(f))
        return _Any()

    def __getattr__(self, name):
        return _Any()


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    NAMES = ("h5py", "cv2", "hdf5plugin", "numba", "evo", "lietorch_backends")

    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in self.NAMES:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = types.ModuleType(spec.name)
        m.__path__ = []
        m.__getattr__ = lambda n: _Any()
        return m

    def exec_module(self, module):
        pass


def _torchvision():
    class Resize:
        def __init__(self, size, interpolation=None):
            self.size = list(size)

        def __call__(self, img):
            x = img.unsqueeze(0) if img.dim() < 4 else img
            x = F.interpolate(x, size=self.size, mode="bilinear", align_corners=False)
            return x.squeeze(0) if img.dim() < 4 else x

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")
    tr.Resize = Resize
    tr.Compose = tr.ToPILImage = tr.ColorJitter = tr.RandomGrayscale = tr.RandomInvert = tr.ToTensor = _Any
    tr.InterpolationMode = _Any()
    tr.functional = fn
    tv.transforms = tr
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})


class _Draws:
    """Records np.random.rand / np.random.uniform calls (the augmentor's draws) while active."""

    def __enter__(self):
        self.rand, self.uniform = [], []
        self._r, self._u = np.random.rand, np.random.uniform

        def rand(*a):
            v = self._r(*a)
            self.rand.append(float(v))
            return v

        def uniform(*a, **k):
            v = self._u(*a, **k)
            self.uniform.append(float(v))
            return v

        np.random.rand, np.random.uniform = rand, uniform
        return self

    def __exit__(self, *e):
        np.random.rand, np.random.uniform = self._r, self._u


def _inputs(rng, n, bins, H, W):
    vq = rng.integers(-24, 25, size=(n, bins, H, W)).astype(np.int8)
    vq[rng.random(vq.shape) < 0.5] = 0                        # sparse, as voxel grids are
    dq = rng.integers(40, 4000, size=(n, H, W)).astype(np.uint16)
    return vq, dq


def vox_of(vq):
    return vq.astype(np.float32) / np.float32(8)


def depth_of(dq):
    return dq.astype(np.float32) / np.float32(64)


def main():
    torch.set_num_threads(1)
    sys.meta_path.insert(0, _StubFinder())
    _torchvision()
    sys.path.insert(0, REF)
    from devo.data_readers import augmentation as A
    from devo.data_readers.base import EVSDDataset
    from utils.transform_utils import transform_rescale

    rng = np.random.default_rng(20261016)
    out = {}
    poses = rng.standard_normal((2, 7)).astype(np.float32)
    intr = np.array([[320.0, 321.5, 70.25, 5.5], [319.0, 322.0, 70.75, 5.25]], np.float32)

    # ---- the augmentor
    vq, dq = _inputs(rng, 2, 2, 11, 141)
    out.update({"in/vox_q": vq, "in/depth_q": dq, "in/poses": poses, "in/intr": intr})
    for s in AUG_SEEDS:
        np.random.seed(s)
        torch.manual_seed(s)
        aug = A.EVSDAugmentor(list(CROP))
        with _Draws() as dr:
            v, p, d, k = aug(torch.from_numpy(vox_of(vq)), torch.from_numpy(poses), torch.from_numpy(1.0 / depth_of(dq)), torch.from_numpy(intr))
        scale = 2 ** dr.uniform[0] if dr.uniform else 1.0
        out.update({f"aug/{s}/scale": np.float64(scale), f"aug/{s}/rand": np.float64(dr.rand[0]),
                    f"aug/{s}/uniform": np.float64(dr.uniform[0] if dr.uniform else np.nan), f"aug/{s}/branch": np.int32(bool(dr.uniform)),
                    f"aug/{s}/v": v.numpy(), f"aug/{s}/d": d.numpy(), f"aug/{s}/intr": k.numpy()})
    for f in (0.9, 1.25):
        for s in (0, 1):
            np.random.seed(s)
            aug = A.EVSDAugmentor(list(CROP))
            with _Draws() as dr:
                aug.voxel_spatial_transform(torch.from_numpy(vox_of(vq)), torch.from_numpy(poses), torch.from_numpy(1.0 / depth_of(dq)),
                                            torch.from_numpy(intr), fix_scale=f)
            out[f"fix/{f}/{s}/scale"] = np.float64(2 ** dr.uniform[0] if dr.uniform else f)

    # ---- transform_rescale
    tvq, tdq = _inputs(rng, 1, 2, 5, 261)
    out.update({"tr/vox_q": tvq, "tr/depth_q": tdq})
    for sc in (0.5, 0.75):
        v, d, p, k = transform_rescale(sc, torch.from_numpy(vox_of(tvq)), torch.from_numpy(1.0 / depth_of(tdq)), torch.from_numpy(poses[:1]).clone(),
                                       torch.from_numpy(intr[:1]))
        out.update({f"tr/{sc}/v": v.numpy(), f"tr/{sc}/d": d.numpy(), f"tr/{sc}/poses": p.numpy(), f"tr/{sc}/intr": k.numpy()})

    # ---- EVSDDataset.__getitem__
    gvq, gdq = _inputs(rng, 2, 2, 21, 283)
    out.update({"gi/vox_q": gvq, "gi/depth_q": gdq})

    for sc in (1.0, 0.5, 0.75):
        src_v, src_d = (vq, dq) if sc == 1.0 else (gvq, gdq)

        class Mem(EVSDDataset):
            @staticmethod
            def voxel_read(i, v=src_v):
                return vox_of(v[i])

            @staticmethod
            def depth_read(i, d=src_d):
                return depth_of(d[i])

        ds = Mem.__new__(Mem)
        ds.n_frames, ds.fmin, ds.fmax, ds.sample, ds.scale, ds.return_fname = 2, 10.0, 75.0, True, sc, False
        crop = list(CROP) if sc == 1.0 else np.floor(sc * np.array(GI_CROP)).astype(int).tolist()
        ds.aug = A.EVSDAugmentor(crop_size=crop)
        ds.scene_info = {"s": {"graph": {0: (np.array([1]), np.array([20.0])), 1: (np.array([0]), np.array([20.0]))},
                               "voxels": [0, 1], "depths": [0, 1], "poses": list(poses), "intrinsics": list(intr)}}
        ds.dataset_index = [("s", 0)]
        for s in GI_SEEDS[sc]:
            np.random.seed(s)
            torch.manual_seed(s)
            with _Draws() as dr:
                v, p, d, k = ds[0]
            out.update({f"gi/{sc}/{s}/scale_drawn": np.float64(2 ** dr.uniform[-1] if dr.uniform and dr.rand[-1] < 0.8 else 1.0),
                        f"gi/{sc}/{s}/v": v.numpy(), f"gi/{sc}/{s}/d": d.numpy(), f"gi/{sc}/{s}/poses": p.numpy(), f"gi/{sc}/{s}/intr": k.numpy()})

    # ---- the depth normalisation (base.py:366-369) on [n, H, W]
    cases = {}
    x = 1.0 / depth_of(rng.integers(40, 4000, size=(2, 7, 9)).astype(np.uint16))
    cases["plain"] = x
    y = x.copy(); y.flat[[3, 50, 77]] = np.inf; cases["inf_few"] = y                       # depth 0: +inf sorts last
    y = x.copy(); y.flat[rng.permutation(y.size)[:20]] = np.inf; cases["inf_at_q"] = y     # the 98 % rank lands on +inf
    y = x.copy(); y.flat[[5, 60]] = np.nan; cases["nan"] = y
    y = np.round(x * 4) / 4; cases["ties"] = y.astype(np.float32)
    cases["equal"] = np.full((2, 7, 9), 0.375, np.float32)
    for name, x in cases.items():
        disps = torch.from_numpy(x.astype(np.float32))
        p = torch.from_numpy(poses).clone()
        s = .7 * torch.quantile(disps, .98)
        disps = disps / s
        p[..., :3] *= s
        out.update({f"q/{name}/x": x.astype(np.float32), f"q/{name}/s": s.numpy(), f"q/{name}/d": disps.numpy(), f"q/{name}/poses": p.numpy()})

    path = os.path.join(ROOT, "tests", "golden", "train_sample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for s in AUG_SEEDS:
        print("aug seed", s, "scale", float(out[f"aug/{s}/scale"]), "branch", int(out[f"aug/{s}/branch"]))
    for sc in (1.0, 0.5, 0.75):
        for s in GI_SEEDS[sc]:
            print("getitem", sc, s, "scale", float(out[f"gi/{sc}/{s}/scale_drawn"]), out[f"gi/{sc}/{s}/v"].shape)


if __name__ == "__main__":
    main()
