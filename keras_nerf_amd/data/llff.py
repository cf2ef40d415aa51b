"""LLFFDatasetLoader -- forward-facing captures in the LLFF layout: `poses_bounds.npy` plus a folder of photographs.  Extension, no
reference counterpart (the reference loads nerf_synthetic directories only, data/loader.py).

The layout (public; restated from the LLFF / original NeRF releases' documentation):
  poses_bounds.npy  [V,17]: the first 15 values of a row reshape to 3x5 -- columns 0-3 camera-to-world in axes (down, right,
                    backwards), column 4 = (H, W, focal) -- and the last two are the near and far depth bounds of the view
  images/           V photographs, matched to the rows in sorted order; images_{factor}/ holds them reduced by `factor`, and
                    H, W and focal are divided by it

`load_dataset` returns [train, val, test] `RayImageDataset`s like `DatasetLoader`: batches, device residency, `take`,
`private_view`, `ray_batches` and data-parallel slicing work unchanged.  Every `holdout`-th view (0, holdout, ...) is held out and
serves as both val and test.  Normalisation: rotation columns to (right, up, backwards); translations and bounds scaled by
1 / (bounds.min() * bd_factor), so that the nearest depth sits at 1 / bd_factor; poses recentred on their average.  With `ndc`
(the default) the rays are NDC rays with the near plane at 1 and samples over the whole ray and the
near / far arguments of `load_dataset` are not used; without it they are pinhole rays sampled between near and far, linearly in
depth or in disparity."""
from __future__ import annotations

import logging
import os
from typing import List

import numpy as np

from .image import ImageLoader
from .loader import RayImageDataset
from .utils import recenter_poses

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")
SPACINGS = ("linear", "disparity")


class LLFFDatasetLoader:
    def __init__(self, data_dir: str, factor: int = 1, bd_factor: float = 0.75, recenter: bool = True, holdout: int = 8,
                 ndc: bool = True, spacing: str = "linear", **kwargs):
        self.data_dir, self.factor, self.bd_factor = data_dir, int(factor), bd_factor
        self.recenter, self.holdout, self.ndc, self.spacing = bool(recenter), int(holdout), bool(ndc), spacing
        if self.factor < 1:
            raise ValueError(f"factor = {factor}: expected an integer >= 1")
        if self.holdout < 2:
            raise ValueError(f"holdout = {holdout}: every holdout-th view is held out, so it must be at least 2")
        if spacing not in SPACINGS:
            raise ValueError(f"spacing = {spacing!r}: expected one of {SPACINGS}")
        if self.ndc and spacing == "disparity":
            raise ValueError("NDC rays are sampled linearly in NDC depth; spacing='disparity' needs ndc=False")
        if bd_factor is not None and not bd_factor > 0:
            raise ValueError(f"bd_factor = {bd_factor}: expected a positive number or None")
        self.poses = self.bounds = self.focal = self.hwf = self.image_paths = None

    def _image_paths(self) -> list:
        folder = os.path.join(self.data_dir, "images" if self.factor == 1 else f"images_{self.factor}")
        if not os.path.isdir(folder):
            raise ValueError(f"{folder} is missing (factor = {self.factor})")
        return [os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.lower().endswith(IMAGE_SUFFIXES)]

    def _load_poses(self, image_width: int, image_height: int):
        """sets image_paths, poses [V,4,4] float64 in (right, up, backwards), bounds [V,2], focal and hwf at the requested size"""
        from PIL import Image
        arr = np.load(os.path.join(self.data_dir, "poses_bounds.npy")).astype(np.float64)
        if arr.ndim != 2 or arr.shape[1] != 17:
            raise ValueError(f"poses_bounds.npy has shape {arr.shape}, expected [V, 17]")
        raw = arr[:, :15].reshape(-1, 3, 5)
        bounds = arr[:, 15:].copy()
        paths = self._image_paths()
        if len(paths) != len(raw):
            raise ValueError(f"poses_bounds.npy describes {len(raw)} views but {os.path.dirname(paths[0]) if paths else self.data_dir} "
                             f"holds {len(paths)} images")
        H, W, focal = raw[0, :, 4] / self.factor
        with Image.open(paths[0]) as im:
            file_w, file_h = im.size
        if abs(image_width * file_h / file_w - image_height) > 1.0:
            raise ValueError(f"{image_width} x {image_height} (width x height) does not keep the aspect of the {file_w} x {file_h} "
                             f"images (within one pixel)")
        poses = np.tile(np.eye(4), (len(raw), 1, 1))
        poses[:, :3, :4] = np.stack([raw[:, :, 1], -raw[:, :, 0], raw[:, :, 2], raw[:, :, 3]], -1)
        sc = 1.0 if self.bd_factor is None else 1.0 / (bounds.min() * self.bd_factor)
        poses[:, :3, 3] *= sc
        bounds *= sc
        if self.recenter:
            poses = recenter_poses(poses)
        self.image_paths, self.poses, self.bounds = paths, poses, bounds
        self.focal = float(focal * image_width / W)
        self.hwf = (int(image_height), int(image_width), self.focal)

    def split(self, n_views: int):
        """(train indices, held-out indices): every holdout-th view, starting with view 0, is held out"""
        held = [i for i in range(n_views) if i % self.holdout == 0]
        return [i for i in range(n_views) if i % self.holdout != 0], held

    def load_dataset(self, batch_size: int, image_width: int, image_height: int, near: float, far: float,
                     n_sample: int) -> List[RayImageDataset]:
        """[train, val, test]; batch_size is the GLOBAL batch as in DatasetLoader.load_dataset.  near, far: the sample range of pinhole
        rays (ndc=False), in the normalised scene's units (see `bounds`); NDC rays are sampled over the whole ray."""
        self._load_poses(image_width, image_height)
        image_loader = ImageLoader(image_width, image_height, height_first=True)
        if self.ndc:
            model = dict(ndc=True, ndc_near=1.0, spacing="linear", near=0.0, far=1.0)
        else:
            model = dict(ndc=False, spacing=self.spacing, near=near, far=far)
        focal = self.focal
        train_idx, held_idx = self.split(len(self.image_paths))
        out = []
        for k, (subset, idx) in enumerate([("train", train_idx), ("val", held_idx), ("test", held_idx)]):
            def factory(rank=0, k=k):
                from .rays import RaysGenerator
                return RaysGenerator(focal_length=focal, image_width=image_width, image_height=image_height, n_sample=n_sample,
                                     seed=1000 + k + 4096 * rank, **model)                  # replicas jitter differently
            out.append(RayImageDataset([self.image_paths[i] for i in idx], [self.poses[i].astype(np.float32) for i in idx],
                                       image_loader, factory, batch_size, seed=k))
            logging.info(f"Loaded {subset} dataset. {len(idx)} images.")
        return out
