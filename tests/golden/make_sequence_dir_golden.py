"""Generates tests/golden/sequence_dir_golden.npz: the REFERENCE's `PeopleSnapshotDataset` and `CustomDataset`
(instant_avatar/datasets/peoplesnapshot.py:39-151, custom.py:39-149) executing on the CPU on the tiny sequence directory of
tests/sequence_fixture.py, for every option set of its CASES: the sliced file lists, image_shape, the SMPL parameters with
the pose file each precedence rule picks, the camera handed to make_rays and its rays, and -- for the val-split cases --
`__getitem__(0)` (rgb, alpha, near, far).

Stand-ins (cv2, hydra and pytorch_lightning are not installed): cv2.imread is PIL with the channel flip (IMREAD_GRAYSCALE:
the grey PNG as it is); cv2.resize is not needed, every option set has downscale 1.  `Opt` comes from ref_cpu_harness.py.
Run from the repo root:  python tests/golden/make_sequence_dir_golden.py"""
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "sequence_dir_golden.npz")


def main():
    import torch  # noqa: F401  (the reference modules import it)
    from PIL import Image
    from ref_cpu_harness import REF, Opt
    import sequence_fixture as fx

    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_GRAYSCALE = 0

    def imread(path, flag=None):
        with Image.open(path) as im:
            if flag == cv2.IMREAD_GRAYSCALE:
                assert im.mode == "L", im.mode
                return np.asarray(im).copy()
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])
    cv2.imread = imread
    sys.modules["cv2"] = cv2
    hydra = types.ModuleType("hydra")
    hydra.utils = types.SimpleNamespace(to_absolute_path=lambda p: p, instantiate=lambda node: None)
    sys.modules["hydra"] = hydra
    pl = types.ModuleType("pytorch_lightning")
    pl.LightningDataModule = object
    sys.modules["pytorch_lightning"] = pl
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import instant_avatar.datasets.custom as cu_mod
    import instant_avatar.datasets.peoplesnapshot as ps_mod

    out = {}
    for name, kind, split, opt, cached in fx.CASES:
        mod = ps_mod if kind == "peoplesnapshot" else cu_mod
        cls = mod.PeopleSnapshotDataset if kind == "peoplesnapshot" else mod.CustomDataset
        seen = {}
        orig = mod.make_rays

        def make_rays(K, c2w, H, W, orig=orig, seen=seen):
            seen["K"], seen["c2w"] = np.array(K, np.float64), np.array(c2w, np.float64)
            return orig(K, c2w, H, W)
        mod.make_rays = make_rays
        with tempfile.TemporaryDirectory() as tmp:
            fx.write_sequence(tmp, kind, cached=cached)
            try:
                ds = cls(Path(tmp), "subject", split, Opt(dict(opt, sampler=None)))
            finally:
                mod.make_rays = orig
            out[name + "/image_files"] = np.array([os.path.basename(f) for f in ds.img_lists])
            out[name + "/mask_files"] = np.array([os.path.basename(f) for f in ds.msk_lists])
            out[name + "/image_shape"] = np.array([int(v) for v in ds.image_shape], np.int64)
            for k, v in ds.smpl_params.items():
                out[name + "/smpl/" + k] = v
            out[name + "/K"], out[name + "/c2w"] = seen["K"], seen["c2w"]
            out[name + "/rays_o"], out[name + "/rays_d"] = ds.rays_o, ds.rays_d
            if name in fx.VAL_CASES:
                datum = ds[0]
                for k in ("rgb", "alpha", "near", "far"):
                    out[name + "/item/" + k] = np.asarray(datum[k])
        print(name, len(ds.img_lists), "frames,", {k: v.shape for k, v in ds.smpl_params.items()})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
